"""config/chroma/chroma_fft.conf as a fused batch set, host part (no GPU): cTonespec's tables and rows and cChroma's rows as
opensmile_amd/csrc/lld_chroma_ops.hpp and chroma_tables.cpp state them, compiled with g++ (tests/helpers/chroma_check.cpp), held to
the real binary's `tonespec` and `chroma` levels bit for bit on the golden inputs (tests/golden/make_golden_chroma_fft.py), starting
from the binary's own `fftmag` rows; the rows rule, the library's own tables, the preset and its geometry, the config struct's
struct_size rules, the element names and the front end's `--set chroma_fft -C file` mapping with its refusals. The GPU tests
(tests/test_gpu_chroma_fft.py) then show that the kernels produce those values."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from helpers import chroma_host as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "opensmile_amd", "smilextract_hip")
GOLD = os.path.join(ROOT, "tests", "golden")
NAMES = ["chroma[%d]" % i for i in range(12)]

# the edited copies of the golden script: the config struct's fields, the host helper's options, the level's width, and the same
# edits on the minimal configuration text below
EDITED = {
    "o5tri": dict(cfg=dict(tonespec_n_octaves=5, tonespec_first_note=110.0, tonespec_filter_type=1, tonespec_use_power=0, tonespec_dba=0),
                  opts=dict(n_octaves=5, first_note=110.0, filter_type="tri", use_power=0, dba=0), octave_size=12, sil_thresh=0.001,
                  minimal={"nOctaves=6": "nOctaves=5", "firstNote=55": "firstNote=110", "filterType=gau": "filterType=tri", "usePower=1": "usePower=0",
                           "dbA=1": "dbA=0"},
                  params=dict(tonespec_n_octaves=5, tonespec_first_note=110, tonespec_filter_type=1, tonespec_use_power=0, tonespec_dba=0)),
    "trp": dict(cfg=dict(tonespec_filter_type=2), opts=dict(filter_type="trp"), octave_size=12, sil_thresh=0.001,
                minimal={"filterType=gau": "filterType=trp"}, params=dict(tonespec_filter_type=2)),
    "rec": dict(cfg=dict(tonespec_filter_type=3), opts=dict(filter_type="rec"), octave_size=12, sil_thresh=0.001,
                minimal={"filterType=gau": "filterType=rec"}, params=dict(tonespec_filter_type=3)),
    "os24": dict(cfg=dict(chroma_octave_size=24), opts={}, octave_size=24, sil_thresh=0.001,
                 minimal={"octaveSize=12": "octaveSize=24"}, params=dict(chroma_octave_size=24)),
    "sil0": dict(cfg=dict(chroma_sil_thresh=0.0), opts={}, octave_size=12, sil_thresh=0.0,
                 minimal={"octaveSize=12": "octaveSize=12\nsilThresh=0"}, params=dict(chroma_sil_thresh=0)),
}


@pytest.fixture(scope="module")
def capi():
    from opensmile_amd import capi as m
    m.load()
    return m


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLD, "chroma_fft_synth.npz"))


def geometry(fs):
    """samples per 64 ms frame and per 10 ms step (lround, as the framer takes them)"""
    return int(np.floor(0.064 * fs + 0.5)), int(np.floor(0.01 * fs + 0.5))


def gold_pcm(gold, k):
    """the samples of golden input k: synth.utterance(index, n) floor-divided by the input's divisor (make_golden_chroma_fft.cut)"""
    from opensmile_amd import synth
    idx, n, fs, div = (int(v) for v in gold["inputs"][k])
    if not n:
        return np.zeros(0, np.int16), fs
    return (synth.utterance(idx, n).astype(np.int32) // div).astype(np.int16), fs


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_same_bits(got, ref, what):
    got, ref = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(ref, np.float32)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    bad = np.argwhere(bits(got) != bits(ref))
    assert len(bad) == 0, "%s: %d of %d cells differ, first at %s: %r != %r" % (what, len(bad), ref.size, tuple(bad[0]), got[tuple(bad[0])], ref[tuple(bad[0])])


# ------------------------------------------------------------------------------------------------ the row functions on the host
def test_tonespec_rows_from_the_binary_s_magnitudes(gold):
    """chroma::tonespec_row on make_tonespec_tables' tables, from the binary's own fftmag rows, is the binary's tonespec level at
    every rate: this pins pitchClassFreq, the binKey walk, nbins, filterMap, the dbA offset and the bin width (float)(1 / frameSizeSec)
    with frameSizeSec scaled by Nfft / N"""
    rates, cells = set(), 0
    for k, (idx, n, fs, div) in enumerate(gold["inputs"]):
        if "fftmag_%d" % k not in gold.files or len(gold["fftmag_%d" % k]) == 0:
            continue
        mag, ts = gold["fftmag_%d" % k], gold["tonespec_%d" % k]
        N, _ = geometry(int(fs))
        assert mag.shape[1] == (1 << (N - 1).bit_length()) // 2 + 1 and ts.shape == (len(mag), 72)
        assert_same_bits(H.tonespec_rows(mag, H.frame_size_sec(int(fs))), ts, "tonespec, input %d at %d Hz" % (k, fs))
        rates.add(int(fs))
        cells += int((ts != 0).sum())
    assert rates == {8000, 11025, 16000, 22050, 32000, 44100, 48000} and cells > 1000
    # the frame is no power of two at four of the rates: the unscaled frameSizeSec gives another level there
    k = [i for i, r in enumerate(gold["inputs"]) if r[2] == 44100][0]
    assert bits(H.tonespec_rows(gold["fftmag_%d" % k], 0.064)).tobytes() != bits(gold["tonespec_%d" % k]).tobytes()


@pytest.mark.parametrize("tag", sorted(EDITED))
def test_tonespec_rows_of_the_edited_copies(gold, tag):
    e = EDITED[tag]
    mag, ts = gold["fftmag_%s_5" % tag], gold["tonespec_%s_5" % tag]
    assert len(mag) == 3 and ts.shape[1] == 12 * e["opts"].get("n_octaves", 6)
    assert_same_bits(H.tonespec_rows(mag, 0.064, e["opts"]), ts, "tonespec, %s" % tag)
    if e["opts"]:
        assert ts.shape != gold["tonespec_5"].shape or bits(ts).tobytes() != bits(gold["tonespec_5"]).tobytes()
    if tag == "rec":
        assert (ts == 0).all()                             # a rectangular filter leaves the map at zero (tonespec.cpp:268-276)


def test_chroma_rows_from_the_binary_s_tonespec(gold):
    zero = one = 0
    for k in range(len(gold["inputs"])):
        ts, ch = gold["tonespec_%d" % k], gold["chroma_%d" % k]
        if len(ts) == 0:
            continue
        got = H.chroma_rows(ts)
        assert_same_bits(got, ch, "chroma, input %d" % k)
        nz = (ch != 0).any(axis=1)
        zero += int((~nz).sum())
        one += int(nz.sum())
        assert np.allclose(ch[nz].astype(np.float64).sum(axis=1), 1.0, atol=1e-5)
    assert zero > 40 and one > 300                         # both branches of the silence flag
    for tag, e in EDITED.items():
        for k in (5, 6):
            ts, ch = gold["tonespec_%s_%d" % (tag, k)], gold["chroma_%s_%d" % (tag, k)]
            assert ch.shape == (len(ts), e["octave_size"])
            assert_same_bits(H.chroma_rows(ts, e["octave_size"], e["sil_thresh"]), ch, "chroma, %s, input %d" % (tag, k))
    assert (gold["chroma_sil0_6"] != 0).any(axis=1).all() and not (gold["chroma_6"] != 0).any(axis=1).all()


def test_what_the_fixture_holds(gold):
    """the golden script's own assertions: zero rows and rows that sum to 1, a quarter of the long inputs' rows non-zero, and a note
    without bins between notes with some"""
    long_ones = [k for k, r in enumerate(gold["inputs"]) if r[2] == 16000 and r[1] >= r[2]]
    assert len(long_ones) == 2
    rows = nonzero = 0
    for k in long_ones:
        ch = gold["chroma_%d" % k]
        nz = (ch != 0).any(axis=1)
        assert nz.any() and (~nz).any()
        rows, nonzero = rows + len(ch), nonzero + int(nz.sum())
    assert 4 * nonzero >= rows
    t = H.tables(513, 0.064)
    rec = t["note_rec"]
    empty = [n for n in range(72) if rec[n, 2] == 0]
    ts = gold["tonespec_%d" % long_ones[0]]
    assert any((ts[:, :n] != 0).any() and (ts[:, n + 1:] != 0).any() and (ts[:, n] == 0).all() for n in empty)


def test_rows_of_is_the_measured_rule(gold):
    L = H.load()
    seen = set()
    for k, (idx, n, fs, div) in enumerate(gold["inputs"]):
        N, Hs = geometry(int(fs))
        rows = L.chroma_rows_of(int(n), N, Hs)
        assert rows == (0 if n < N else (int(n) - N) // Hs + 1)
        assert len(gold["chroma_%d" % k]) == len(gold["tonespec_%d" % k]) == rows == len(str(gold["csv_%d" % k]).splitlines()), (k, n, fs)
        seen.add(rows)
    assert {0, 1, 2, 3, 94, 294} <= seen
    assert [int(r[1]) for r in gold["inputs"][:6]] == [0, 1023, 1024, 1183, 1184, 1344]


# ------------------------------------------------------------------------------------------------ the library's tables
OPTION_SETS = [({}, 513, 16000), ({}, 257, 8000), ({}, 513, 11025), ({}, 2049, 44100), ({}, 2049, 48000)] + \
              [(e["opts"], 513, 16000) for e in EDITED.values() if e["opts"]]


@pytest.mark.parametrize("opts,K,fs", OPTION_SETS, ids=lambda v: str(v).replace(" ", ""))
def test_library_tables_equal_the_helper_s(capi, opts, K, fs):
    """smilehip_tonespec_op_tables (the library's build of chroma_tables.cpp) against the g++ build the level tests above hold to the binary"""
    fss = H.frame_size_sec(fs)
    o = capi.tonespec_opts(**dict(H.SHIPPED, **opts))
    lib, ref = capi.tonespec_tables(o, K, fss), H.tables(K, fss, opts)
    for key in ("pitch_class_freq", "bin_key", "nbins", "filter_map", "note_rec", "first_last"):
        assert lib[key].dtype == ref[key].dtype and lib[key].tobytes() == ref[key].tobytes(), key
    rec, key_of = ref["note_rec"], ref["bin_key"]
    first, last = (int(v) for v in ref["first_last"])
    assert 1 <= first <= last < K
    assert (np.diff(key_of) >= 0).all()                    # monotone: a note's bins are one run
    for n in range(len(rec)):
        run = [i for i in range(first, last + 1) if key_of[i] == n + 1]
        assert rec[n, 1] == len(run) == rec[n, 2] == ref["nbins"][n + 1] and (not run or (rec[n, 0] == run[0] and run[-1] - run[0] + 1 == len(run)))
    assert (ref["filter_map"][:first] == 0).all() and (ref["filter_map"][last + 1:] == 0).all()
    if dict(H.SHIPPED, **opts)["dba"]:
        assert ref["filter_map"][first] == 0               # the dbA curve is read from its element 0: log(0)


def test_table_refusals(capi):
    L = capi.load()
    for kw, K, fss, word in ((dict(n_octaves=0), 513, 0.064, b"nOctaves"), (dict(n_octaves=11), 513, 0.064, b"nOctaves"),
                             (dict(first_note=0.0), 513, 0.064, b"firstNote"), (dict(filter_type=4), 513, 0.064, b"filterType"),
                             ({}, 1, 0.064, b"bins"), ({}, 513, 0.0, b"frameSizeSec")):
        o = capi.tonespec_opts(**dict(H.SHIPPED, **kw))
        assert L.smilehip_tonespec_op_tables(C.byref(o), K, fss, None, None, None, None, None, None) < 0 and word in L.smilehip_last_error(), kw


# ------------------------------------------------------------------------------------------------ preset, ABI, geometry
def test_preset_values_and_export(capi):
    hdr = open(os.path.join(ROOT, "include", "smilehip.h")).read()
    for sym in ("smilehip_config_chroma_fft", "smilehip_batch_chroma_taps", "smilehip_tonespec_op_create", "smilehip_tonespec_op_n_out",
                "smilehip_tonespec_op_frames", "smilehip_tonespec_op_destroy", "smilehip_tonespec_op_tables", "smilehip_chroma_op_create",
                "smilehip_chroma_op_frames", "smilehip_chroma_op_destroy"):
        assert sym in capi.SYMBOLS and re.search(r"\b%s\s*\(" % sym, hdr), sym
    assert re.search(r"#define\s+SMILEHIP_CHAIN_CHROMA_FFT\s+9\b", hdr) and capi.CHAIN_CHROMA_FFT == 9
    c = capi.chroma_fft_config(22050.0)
    assert c.chain_kind == 9 and c.struct_size == C.sizeof(capi.LldConfigChroma) > C.sizeof(capi.LldConfig) and c.sample_rate == 22050.0
    assert (c.frame_size_sec, c.frame_step_sec) == (0.064, 0.010)
    assert (c.win_func, c.win_sigma, c.win_gain, c.win_offset) == (capi.prosody_acf_config().win_func, 0.4, 1.0, 0.0)      # gauss
    assert c.zero_pad_symmetric == 1 and c.preemph == 0 and c.n_delta == 0
    assert (c.tonespec_n_octaves, c.tonespec_first_note, c.tonespec_filter_type, c.tonespec_use_power, c.tonespec_dba) == (6, 55.0, 0, 1, 1)
    assert (c.chroma_octave_size, c.chroma_sil_thresh) == (12, np.float32(0.001))
    m = re.search(r"#define\s+SMILEHIP_LLD_CONFIG_SIZE_V1\s+(\d+)u", hdr)
    assert m and int(m.group(1)) == C.sizeof(capi.LldConfig) == capi.LLD_CONFIG_SIZE_V1


def test_a_header_of_the_older_struct_size_is_still_accepted(capi):
    """the struct_size rules: the older presets fill and report the older size, whatever lies behind it in the caller's memory, and a
    plan is made from such a struct; the chroma chain needs the full one"""
    L = capi.load()
    old = C.sizeof(capi.LldConfig)

    class Guarded(C.Structure):
        _fields_ = [("cfg", capi.LldConfig), ("guard", C.c_uint8 * 64)]
    g = Guarded()
    C.memset(C.byref(g), 0xA5, C.sizeof(g))
    L.smilehip_config_prosody_acf(C.cast(C.byref(g), C.POINTER(capi.LldConfig)))
    assert g.cfg.struct_size == old and bytes(g.guard) == b"\xa5" * 64      # nothing written past the older struct's end
    h = C.c_void_p()
    capi._check(L.smilehip_plan_create_host_only(C.byref(g.cfg), C.byref(h)))      # ... and garbage behind it is not read
    geo = capi.Geometry()
    capi._check(L.smilehip_plan_geometry(h, C.byref(geo)))
    assert (geo.frame_size, geo.n_out) == (800, 3)
    L.smilehip_plan_destroy(h)
    full = capi.chroma_fft_config()
    capi._check(L.smilehip_plan_create_host_only(C.byref(full), C.byref(h)))
    L.smilehip_plan_destroy(h)
    full.struct_size = old                                 # a struct that ends before the chroma fields cannot ask for the chroma chain
    assert L.smilehip_plan_create_host_only(C.byref(full), C.byref(h)) != 0 and b"struct_size" in L.smilehip_last_error()
    full.struct_size = old + 8                             # neither size
    assert L.smilehip_plan_create_host_only(C.byref(full), C.byref(h)) != 0 and b"struct_size" in L.smilehip_last_error()


def test_geometry_and_refusals(capi):
    L = capi.load()
    for fs, want in ((8000, (512, 80, 512)), (11025, (706, 110, 1024)), (16000, (1024, 160, 1024)), (22050, (1411, 221, 2048)),
                     (32000, (2048, 320, 2048)), (44100, (2822, 441, 4096)), (48000, (3072, 480, 4096))):
        c = capi.chroma_fft_config(fs)
        h = C.c_void_p()
        capi._check(L.smilehip_plan_create_host_only(C.byref(c), C.byref(h)))
        try:
            g = capi.Geometry()
            capi._check(L.smilehip_plan_geometry(h, C.byref(g)))
            assert (g.frame_size, g.frame_step, g.fft_size) == want and g.n_bins == want[2] // 2 + 1 and (g.n_static, g.n_out) == (12, 12)
            assert (g.frame_size, g.frame_step) == geometry(fs)
            assert g.fft_frame_size_sec == H.frame_size_sec(fs)
            assert [round(L.smilehip_row_time(h, 9, r) / c.frame_step_sec) for r in range(9)] == list(range(9))
            for n in (0, want[0] - 1, want[0], want[0] + want[1] - 1, want[0] + want[1], 100000):
                assert L.smilehip_num_frames(h, n) == H.load().chroma_rows_of(n, want[0], want[1])
        finally:
            L.smilehip_plan_destroy(h)
    h = C.c_void_p()
    for field, value, word in (("n_delta", 1, b"n_delta"), ("preemph", 1, b"preemph"), ("chroma_octave_size", 0, b"chroma_octave_size"),
                               ("chroma_octave_size", 65, b"chroma_octave_size"), ("chroma_octave_size", 5, b"no multiple"),
                               ("tonespec_n_octaves", 0, b"tonespec_n_octaves"), ("tonespec_n_octaves", 11, b"tonespec_n_octaves"),
                               ("tonespec_filter_type", 7, b"filterType"), ("tonespec_first_note", -1.0, b"firstNote"),
                               ("frame_size_sec", 0.001, b"transform length"), ("frame_size_sec", 0.6, b"8192")):
        c = capi.chroma_fft_config()
        setattr(c, field, value)
        assert L.smilehip_plan_create_host_only(C.byref(c), C.byref(h)) != 0 and word in L.smilehip_last_error(), (field, L.smilehip_last_error())


def test_hard_signal_fixture_shape():
    h = np.load(os.path.join(GOLD, "hard_chroma_fft.npz"))
    from helpers import hard_signals
    assert sorted(h.files) == sorted("chroma_" + n for n in hard_signals.NAMES)
    for n in hard_signals.NAMES:
        assert h["chroma_" + n].shape == (144, 12)         # 1.5 s: (24000 - 1024) / 160 + 1 frames
    assert (h["chroma_lsb_noise"] == 0).all() and (h["chroma_dc"] != 0).any(axis=1).all()
    z = (h["chroma_zeros_voiced_zeros"] != 0).any(axis=1)
    assert z.any() and (~z).any()


# ------------------------------------------------------------------------------------------------ names, front end
def test_names_and_csv_header(gold):
    assert str(gold["csv_header"]) == ";".join(NAMES)
    src = open(os.path.join(ROOT, "opensmile_amd", "host", "feature_names.cpp")).read()
    assert "lld_names_chroma_fft" in src and '"chroma["' in src
    for stem, rows in (("u2_8000", (8000 - 1024) // 160 + 1), ("u3_4000", (4000 - 1024) // 160 + 1)):     # 16 kHz files of 8000 / 4000 samples
        lines = open(os.path.join(GOLD, "files", "chroma_fft_%s.csv" % stem)).read().splitlines()
        assert len(lines) == rows and all(len(ln.split(";")) == 12 for ln in lines) and not lines[0].startswith("'")


needs_exe = pytest.mark.skipif(not os.path.exists(EXE), reason="smilextract_hip not built")

# a minimal configuration text of the same graph, not the shipped file: own wording
MINIMAL = """
[componentInstances:cComponentManager]
instance[dataMemory].type=cDataMemory
instance[wave].type=cWaveSource
instance[fr].type=cFramer
instance[w].type=cWindower
instance[f].type=cTransformFFT
instance[m].type=cFFTmagphase
instance[notes].type=cTonespec
instance[classes].type=cChroma
instance[out].type=cCsvSink
[wave:cWaveSource]
writer.dmLevel=wave
filename=\\cm[inputfile(I){in.wav}:input]
monoMixdown=1
[fr:cFramer]
reader.dmLevel=wave
writer.dmLevel=frames
frameSize=0.064
frameStep=0.01
[w:cWindower]
reader.dmLevel=frames
writer.dmLevel=windowed
winFunc=gauss
sigma=0.4
[f:cTransformFFT]
reader.dmLevel=windowed
writer.dmLevel=spec
[m:cFFTmagphase]
reader.dmLevel=spec
writer.dmLevel=mag
[notes:cTonespec]
reader.dmLevel=mag
writer.dmLevel=semitones
processArrayFields=0
nOctaves=6
firstNote=55
filterType=gau
usePower=1
dbA=1
[classes:cChroma]
reader.dmLevel=semitones
writer.dmLevel=pitchclasses
processArrayFields=0
octaveSize=12
[out:cCsvSink]
reader.dmLevel=pitchclasses
filename=\\cm[outputfile(O){chroma.csv}:output]
timestamp=0
number=0
printHeader=0
"""


def describe(path, *more):
    r = subprocess.run([EXE, "--set", "chroma_fft", "-C", path, "--describe", *more], capture_output=True, text=True)
    kv = dict(l.split("=", 1) for l in r.stdout.split("\n") if "=" in l)
    return r.returncode, kv, r.stderr


def write_conf(tmp_path, text, name="c.conf"):
    p = tmp_path / name
    p.write_text(text)
    return str(p)


@needs_exe
def test_minimal_text_maps_to_the_set(tmp_path):
    rc, kv, err = describe(write_conf(tmp_path, MINIMAL))
    assert rc == 0 and kv["preset"] == "chroma_fft" and "every processing component and option identical" in err, err
    assert not [k for k in kv if k.startswith("param.")]


@needs_exe
@pytest.mark.parametrize("tag", sorted(EDITED))
def test_allowed_edits_show_up(tmp_path, tag):
    text = MINIMAL
    for a, b in EDITED[tag]["minimal"].items():
        assert text.count(a) == 1, a
        text = text.replace(a, b)
    rc, kv, err = describe(write_conf(tmp_path, text))
    assert rc == 0 and kv["preset"] == "chroma_fft", err
    got = {k[6:]: float(v) for k, v in kv.items() if k.startswith("param.")}
    want = dict(tonespec_n_octaves=6, tonespec_first_note=55, tonespec_filter_type=0, tonespec_use_power=1, tonespec_dba=1, chroma_octave_size=12,
                chroma_sil_thresh=float(np.float32(0.001)))
    want.update(EDITED[tag]["params"])
    assert got.keys() == want.keys() and all(abs(got[k] - want[k]) < 1e-9 for k in want), got


REFUSED = [  # (text of the minimal configuration, its replacement, what the message must name)
    ("winFunc=gauss", "winFunc=ham", "winFunc"),
    ("frameSize=0.064", "frameSize=0.05", "frameSize"),
    ("writer.dmLevel=spec", "writer.dmLevel=spec\nzeroPadSymmetric=0", "zeroPadSymmetric"),
    ("octaveSize=12", "octaveSize=7", "octaveSize"),
    ("nOctaves=6", "nOctaves=12", "nOctaves"),
    ("filterType=gau", "filterType=hexagonal", "filterType"),
    ("processArrayFields=0\noctaveSize", "processArrayFields=0\nnameAppend=pc\noctaveSize", "nameAppend"),
    ("printHeader=0", "printHeader=1", "printHeader"),
    ("timestamp=0", "timestamp=1", "timestamp"),
    ("reader.dmLevel=pitchclasses", "reader.dmLevel=semitones", "semitones"),
    ("instance[out].type=cCsvSink", "instance[out].type=cCsvSink\ninstance[e].type=cEnergy", "cEnergy"),
]


@needs_exe
@pytest.mark.parametrize("old,new,option", REFUSED, ids=["%s:%s" % (r[2], r[1].split("\n")[-1]) for r in REFUSED])
def test_refused_edit_names_the_option(tmp_path, old, new, option):
    assert MINIMAL.count(old) == 1
    text = MINIMAL.replace(old, new)
    if "cEnergy" in new:
        text += "[e:cEnergy]\nreader.dmLevel=frames\nwriter.dmLevel=energy\n"
    rc, kv, err = describe(write_conf(tmp_path, text))
    assert rc != 0 and "preset" not in kv
    assert option in err, err


@needs_exe
def test_plain_conf_keeps_refusing_the_file(tmp_path):
    p = write_conf(tmp_path, MINIMAL)
    r = subprocess.run([EXE, "-C", p, "--describe"], capture_output=True, text=True)
    assert r.returncode != 0 and "cannot run on the fused path" in r.stderr and "--set chroma_fft -C" in r.stderr
    r = subprocess.run([EXE, "--set", "prosody_acf", "-C", p, "--describe"], capture_output=True, text=True)    # the set name picks the walker
    assert r.returncode != 0 and "prosodyAcf.conf" in r.stderr
    r = subprocess.run([EXE, "--set", "chroma_fft"], capture_output=True, text=True)      # the set name is known: what is missing is the input
    assert r.returncode != 0 and "no input" in r.stderr and "--set must be" not in r.stderr


@needs_exe
@pytest.mark.skipif(not os.path.isdir(os.path.join(ROOT, "oracle", "_ref", "config")), reason="the reference's configuration files are not there (oracle/_ref not built)")
def test_shipped_file_is_recognised():
    conf = os.path.join(ROOT, "oracle", "_ref", "config", "chroma", "chroma_fft.conf")
    rc, kv, err = describe(conf)
    assert rc == 0 and kv["preset"] == "chroma_fft" and "every processing component and option identical" in err, err
    r = subprocess.run([EXE, "-C", conf, "--describe"], capture_output=True, text=True)
    assert r.returncode != 0 and "cannot run on the fused path" in r.stderr and "--set chroma_fft -C" in r.stderr
