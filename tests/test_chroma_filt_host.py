"""config/chroma/chroma_filt.conf without a GPU: the row functions of the scan kernel (opensmile_amd/csrc/lld_tonefilt_ops.hpp with the
C library's sin / cos, tonefilt_tables.cpp, lld_chroma_ops.hpp) built with g++ (tests/helpers/tonefilt_check.cpp) and held bit for
bit to the levels `tonespec` and `chroma` the REAL binary wrote (tests/golden/make_golden_chroma_filt.py), the block length and the
row rule at seven rates, the tables, the struct-size rules, the front end's mapping of the file, and the Python mirror."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from helpers import chroma_host
from helpers import tonefilt_host as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "opensmile_amd", "smilextract_hip")
GOLD = os.path.join(ROOT, "tests", "golden")
NAMES = ["chroma[%d]" % i for i in range(12)]
BLOCK = {8000: 80, 11025: 110, 16000: 160, 22050: 221, 32000: 320, 44100: 441, 48000: 480}     # P as the binary's rows pin it
N16 = 7                                                    # the 16 kHz inputs: 0 .. 6
LONG = 13                                                  # 60 s at 8 kHz: every 50th row and the last 20 are in the fixture

# the edited copies of the golden script: the config struct's fields, the host helper's options, and the same edits on the minimal
# configuration text below
EDITED = {
    "n48": dict(cfg=dict(tonefilt_n_notes=48, tonefilt_first_note=110.0, tonefilt_decay_f0=0.9995, tonefilt_decay_fn=0.998),
                opts=dict(n_notes=48, first_note=110.0, decay_f0=0.9995, decay_fn=0.998), octave_size=12, sil_thresh=0.001,
                minimal={"nNotes=72": "nNotes=48", "firstNote=55": "firstNote=110", "decayF0=0.9999": "decayF0=0.9995", "decayFN=0.999": "decayFN=0.998"},
                params=dict(tonefilt_n_notes=48, tonefilt_first_note=110, tonefilt_decay_f0=0.9995, tonefilt_decay_fn=0.998)),
    "op25": dict(cfg=dict(tonefilt_output_period=0.025, frame_size_sec=0.025, frame_step_sec=0.025), opts=dict(output_period=0.025), octave_size=12,
                 sil_thresh=0.001, minimal={"outputPeriod=0.01": "outputPeriod=0.025"}, params=dict(tonefilt_output_period=0.025)),
    "os24": dict(cfg=dict(chroma_octave_size=24), opts={}, octave_size=24, sil_thresh=0.001,
                 minimal={"octaveSize=12": "octaveSize=24"}, params=dict(chroma_octave_size=24)),
    "sil0": dict(cfg=dict(chroma_sil_thresh=0.0), opts={}, octave_size=12, sil_thresh=0.0,
                 minimal={"octaveSize=12": "octaveSize=12\nsilThresh=0"}, params=dict(chroma_sil_thresh=0)),
}
EDIT_INPUTS = (5, 6)


@pytest.fixture(scope="module")
def capi():
    from opensmile_amd import capi as m
    m.load()
    return m


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLD, "chroma_filt_synth.npz"))


def gold_pcm(gold, k):
    """the samples of golden input k: synth.utterance(index, n) floor-divided by the input's divisor (make_golden_chroma_filt.cut)"""
    from opensmile_amd import synth
    idx, n, fs, div = (int(v) for v in gold["inputs"][k])
    if not n:
        return np.zeros(0, np.int16), fs
    return (synth.utterance(idx, n).astype(np.int32) // div).astype(np.int16), fs


def kept_rows(gold, k, n_rows):
    """the rows of input k the fixture holds (make_golden_chroma_filt.kept_rows)"""
    if k != LONG:
        return np.arange(n_rows)
    return np.unique(np.concatenate([np.arange(0, n_rows, int(gold["long_keep"])), np.arange(max(n_rows - 20, 0), n_rows)]))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_same_bits(got, ref, what):
    got, ref = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(ref, np.float32)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    bad = np.argwhere(bits(got) != bits(ref))
    assert len(bad) == 0, "%s: %d of %d cells differ, first at %s: %r != %r" % (what, len(bad), ref.size, tuple(bad[0]), got[tuple(bad[0])], ref[tuple(bad[0])])


_HOST = {}


def host_levels(gold, k, tag=None):
    """(tonespec, chroma, s, c) of the g++ row functions on golden input k, all rows; computed once per input and edit"""
    if (k, tag) not in _HOST:
        pcm, fs = gold_pcm(gold, k)
        e = EDITED[tag] if tag else dict(opts={}, octave_size=12, sil_thresh=0.001)
        ts, s, c = H.tonespec_rows(H.padded(pcm, fs, e["opts"]), fs, e["opts"])
        ch = chroma_host.chroma_rows(ts, e["octave_size"], e["sil_thresh"]) if len(ts) else np.zeros((0, e["octave_size"]), np.float32)
        _HOST[(k, tag)] = (ts, ch, s, c)
    return _HOST[(k, tag)]


# ------------------------------------------------------------------------------------------------ row functions against the binary
@pytest.mark.parametrize("k", range(14))
def test_host_rows_equal_the_binary_s_levels(gold, k):
    ts, ch, s, c = host_levels(gold, k)
    n = int(gold["n_rows_%d" % k])
    assert len(ts) == n
    if not n:
        assert gold["tonespec_%d" % k].size == 0 and str(gold["csv_%d" % k]) == ""
        return
    keep = kept_rows(gold, k, n)
    assert_same_bits(ts[keep], gold["tonespec_%d" % k], "level tonespec, input %d" % k)
    assert_same_bits(ch[keep], gold["chroma_%d" % k], "level chroma, input %d" % k)
    assert (s == gold["state_s_%d" % k]).all() and (c == gold["state_c_%d" % k]).all()      # the stored host states are this build's


@pytest.mark.parametrize("tag", sorted(EDITED))
def test_host_rows_of_the_edited_copies(gold, tag):
    for k in EDIT_INPUTS:
        ts, ch, s, c = host_levels(gold, k, tag)
        assert_same_bits(ts, gold["tonespec_%s_%d" % (tag, k)], "level tonespec, %s, input %d" % (tag, k))
        assert_same_bits(ch, gold["chroma_%s_%d" % (tag, k)], "level chroma, %s, input %d" % (tag, k))
    assert str(gold["csv_%s_6" % tag]) != str(gold["csv_6"])


def test_what_the_fixture_holds(gold):
    """zero rows, rows that sum to 1, at least a quarter non-zero; every rate; D of every input is the size the issue measured"""
    ch = gold["chroma_6"]
    nz = (ch != 0).any(axis=1)
    assert len(ch) == 100 and (~nz).any() and 4 * nz.sum() >= len(ch)
    assert (np.abs(ch[nz].astype(np.float64).sum(axis=1) - 1.0) < 1e-5).all()
    assert sorted(set(int(r[2]) for r in gold["inputs"])) == sorted(BLOCK)
    assert int(gold["inputs"][LONG][1]) == 480000 and int(gold["inputs"][LONG][2]) == 8000 and len(gold["chroma_%d" % LONG]) == 120 + 20
    for k in range(14):
        assert 0 <= float(gold["D_%d" % k]) < 1e-10, k
    # nNotes no multiple of octaveSize: the binary writes rows of zeros (what the chain and the front end refuse)
    assert int(gold["n70_rc"]) == 0 and set(str(gold["n70_csv"]).split()) == {"0;0;0;0;0;0;0;0;0;0;0;0"}


def test_block_length_and_row_rule(gold, capi):
    """P at seven rates and ceil(n / P) rows, the last block padded with the last sample: as measured against the binary"""
    L = capi.load()
    for fs, P in BLOCK.items():
        assert H.block_len(fs) == P == capi.tonefilt_tables(capi.tonefilt_opts(), fs)["P"]
        for n, rows in ((0, 0), (1, 1), (P - 1, 1), (P, 1), (P + 1, 2), (2 * P - 1, 2), (2 * P, 2), (2 * P + 1, 3)):
            assert H.rows_of(n, P) == rows
        plan = capi.Plan(None, capi.chroma_filt_config(fs))
        g = plan.geometry
        assert (g.frame_size, g.frame_step, g.n_static, g.n_out) == (P, P, 12, 12) and g.frame_period == 0.01
        assert [plan.num_frames(n) for n in (0, 1, P - 1, P, P + 1, 2 * P - 1, 2 * P, 2 * P + 1)] == [0, 1, 1, 1, 2, 2, 2, 3]
        assert [round(L.smilehip_row_time(plan._h, 9, r) / 0.01) for r in range(9)] == list(range(9))
    assert H.block_len(16000, 0.025) == 400 and H.block_len(16000, 1e-6) == 1 and H.block_len(16000, 0.0) == 1600
    for k, (idx, n, fs, div) in enumerate(gold["inputs"]):
        assert int(gold["n_rows_%d" % k]) == H.rows_of(int(n), BLOCK[int(fs)]), k
    assert [int(gold["n_rows_%d" % k]) for k in range(6)] == [0, 1, 1, 2, 2, 2]      # 0, P - 1, P, P + 1, 2P - 1, 2P samples
    lines = str(gold["csv_header_copy"]).splitlines()      # names and row times: a copy that prints header and time stamps
    assert lines[0] == "frameTime;" + ";".join(NAMES)
    assert [ln.split(";")[0] for ln in lines[1:]] == ["%.6f" % (0.01 * r) for r in range(len(lines) - 1)] and len(lines) == 1 + 11


def test_tables(capi):
    """freq and decayF in double, as tonefilt.cpp:180-189 writes them, with the clamps of myFetchConfig"""
    for opts, fs in (({}, 16000), ({}, 44100), (EDITED["n48"]["opts"], 16000), (dict(decay_f0=0.5, decay_fn=0.9), 8000),
                     (dict(decay_f0=1.5, decay_fn=-1.0, first_note=-3.0, n_notes=0), 8000)):
        o = dict(H.SHIPPED, **opts)
        t = H.tables(fs, opts)
        lib = capi.tonefilt_tables(capi.tonefilt_opts(**o), fs)
        fn = min(max(o["decay_fn"], 0.0), 1.0)
        f0 = min(max(max(o["decay_f0"], fn), 0.0), 1.0)
        first = o["first_note"] if o["first_note"] > 0 else 1.0
        n = max(o["n_notes"], 1)
        freq = np.array([first * 2.0 ** (k / 12.0) for k in range(n)])
        assert len(t["freq"]) == n and np.abs(t["freq"] / freq - 1).max() < 4e-16       # pow is the C library's: within its error
        decay = fn + (f0 - fn) * (t["freq"] - t["freq"][0]) / t["freq"][-1]
        assert (t["decay"] == decay).all() and (t["w"] == 2.0 * np.pi * t["freq"]).all()
        assert (lib["freq"] == t["freq"]).all() and (lib["decay"] == t["decay"]).all() and lib["P"] == t["P"]
    t = H.tables(16000)
    assert t["freq"][0] == 55.0 and t["freq"][12] == 110.0 and t["decay"][0] == 0.999 and 0.999 < t["decay"][-1] < 0.9999
    L = capi.load()
    for kw, word in ((dict(n_notes=121), b"nNotes"), (dict(first_note=float("nan")), b"finite"), (dict(output_period=1e6), b"outputPeriod")):
        o = capi.tonefilt_opts(**kw)
        assert L.smilehip_tonefilt_op_tables(C.byref(o), 16000.0, None, None, None) < 0 and word in L.smilehip_last_error(), kw


def test_sincos_d_host_build_within_one_ulp():
    """the same arithmetic as the device's (explicit fma for fma), against sinl / cosl: the chain's own arguments and seeded ones"""
    rng = np.random.default_rng(7)
    D = H.load().tonefilt_domain()
    assert D == 2.0 ** 30
    w = H.tables(16000)["w"]
    x = np.concatenate([rng.uniform(-D, D, 1 << 18), (w[:, None] * (np.arange(0, 4000)[None, :] * (1.0 / 16000))).ravel(),
                        np.arange(1, 1 << 14) * (np.pi / 2), np.array([0.0, -0.0, 1e-300, 2.0 ** -27, D, -D])])
    _, _, err, at = H.sincos_check(x)
    assert err.max() <= 1.0, (err, at)


# ------------------------------------------------------------------------------------------------ preset, ABI
def test_preset_values_and_export(capi):
    hdr = open(os.path.join(ROOT, "include", "smilehip.h")).read()
    for sym in ("smilehip_config_chroma_filt", "smilehip_tonefilt_op_create", "smilehip_tonefilt_op_n_out", "smilehip_tonefilt_op_block_len",
                "smilehip_tonefilt_op_blocks", "smilehip_tonefilt_op_state", "smilehip_tonefilt_op_reset", "smilehip_tonefilt_op_destroy",
                "smilehip_tonefilt_op_tables", "smilehip_sincos_d_values"):
        assert sym in capi.SYMBOLS and re.search(r"\b%s\s*\(" % sym, hdr), sym
    assert re.search(r"#define\s+SMILEHIP_CHAIN_CHROMA_FILT\s+10\b", hdr) and capi.CHAIN_CHROMA_FILT == 10
    c = capi.chroma_filt_config(22050.0)
    assert c.chain_kind == 10 and c.struct_size == C.sizeof(capi.LldConfigChromaFilt) > C.sizeof(capi.LldConfigChroma) and c.sample_rate == 22050.0
    assert (c.tonefilt_n_notes, c.tonefilt_first_note, c.tonefilt_decay_f0, c.tonefilt_decay_fn, c.tonefilt_output_period) == (72, 55.0, 0.9999, 0.999, 0.01)
    assert (c.frame_size_sec, c.frame_step_sec, c.preemph, c.n_delta) == (0.01, 0.01, 0, 0)
    assert (c.chroma_octave_size, c.chroma_sil_thresh) == (12, np.float32(0.001))
    m = re.search(r"#define\s+SMILEHIP_LLD_CONFIG_SIZE_V2\s+(\d+)u", hdr)
    assert m and int(m.group(1)) == C.sizeof(capi.LldConfigChroma) == capi.LLD_CONFIG_SIZE_V2
    # the mirrors match the header: every field of the struct's tail, in order, and the operator's options
    tail = hdr[hdr.index("int32_t  tonefilt_n_notes"):hdr.index("} smilehip_lld_config;")]
    assert re.findall(r"^\s*(?:int32_t|double)\s+(\w+);", tail, re.M) == [f[0] for f in capi.LldConfigChromaFilt._fields_]
    opts = hdr[hdr.index("typedef struct smilehip_tonefilt_opts {"):hdr.index("} smilehip_tonefilt_opts;")]
    assert re.findall(r"^\s*(?:int32_t|double)\s+(\w+);", opts, re.M) == [f[0] for f in capi.TonefiltOpts._fields_]
    assert C.sizeof(capi.TonefiltOpts) == 40 and C.sizeof(capi.LldConfigChromaFilt) == capi.LLD_CONFIG_SIZE_V2 + 40


def test_struct_size_rules(capi):
    """V1, V2 and the full size are accepted and uncovered fields read as zero; smilehip_config_chroma_fft fills and reports exactly V2;
    the chroma_filt chain needs the full size"""
    L = capi.load()
    v1, v2, full = C.sizeof(capi.LldConfig), C.sizeof(capi.LldConfigChroma), C.sizeof(capi.LldConfigChromaFilt)
    assert (v1, v2) == (capi.LLD_CONFIG_SIZE_V1, capi.LLD_CONFIG_SIZE_V2) and full > v2

    class Guarded(C.Structure):
        _fields_ = [("cfg", capi.LldConfigChroma), ("guard", C.c_uint8 * 64)]
    g = Guarded()
    C.memset(C.byref(g), 0xA5, C.sizeof(g))
    L.smilehip_config_chroma_fft(C.cast(C.byref(g), C.POINTER(capi.LldConfigChroma)), 16000.0)
    assert g.cfg.struct_size == v2 and bytes(g.guard) == b"\xa5" * 64       # nothing written past the V2 struct's end
    h = C.c_void_p()
    capi._check(L.smilehip_plan_create_host_only(C.byref(g.cfg), C.byref(h)))       # ... and garbage behind it is not read
    geo = capi.Geometry()
    capi._check(L.smilehip_plan_geometry(h, C.byref(geo)))
    assert (geo.frame_size, geo.frame_step, geo.n_out) == (1024, 160, 12)
    L.smilehip_plan_destroy(h)
    g1 = capi.LldConfigChromaFilt()
    C.memset(C.byref(g1), 0xA5, C.sizeof(g1))
    L.smilehip_config_prosody_acf(C.cast(C.byref(g1), C.POINTER(capi.LldConfig)))
    assert g1.struct_size == v1 and g1.chroma_octave_size == C.c_int32(0xA5A5A5A5).value      # V1 presets still stop at V1
    capi._check(L.smilehip_plan_create_host_only(C.byref(g1), C.byref(h)))
    L.smilehip_plan_destroy(h)
    fft_full = capi.LldConfigChromaFilt()                  # the chroma_fft chain in a full-sized struct
    L.smilehip_config_chroma_fft(C.cast(C.byref(fft_full), C.POINTER(capi.LldConfigChroma)), 16000.0)
    fft_full.struct_size = full
    capi._check(L.smilehip_plan_create_host_only(C.byref(fft_full), C.byref(h)))
    L.smilehip_plan_destroy(h)
    c = capi.chroma_filt_config()
    capi._check(L.smilehip_plan_create_host_only(C.byref(c), C.byref(h)))
    L.smilehip_plan_destroy(h)
    for size in (v2, v1):                                  # a struct that ends before the tonefilt fields cannot ask for this chain
        c = capi.chroma_filt_config()
        c.struct_size = size
        assert L.smilehip_plan_create_host_only(C.byref(c), C.byref(h)) != 0 and b"struct_size" in L.smilehip_last_error()
    c = capi.chroma_filt_config()
    c.struct_size = v2 + 8                                 # no known size
    assert L.smilehip_plan_create_host_only(C.byref(c), C.byref(h)) != 0 and b"struct_size" in L.smilehip_last_error()


def test_plan_refusals(capi):
    L = capi.load()
    h = C.c_void_p()
    for field, value, word in (("n_delta", 1, b"n_delta"), ("preemph", 1, b"preemph"), ("chroma_octave_size", 0, b"chroma_octave_size"),
                               ("chroma_octave_size", 65, b"chroma_octave_size"), ("chroma_octave_size", 5, b"no multiple"),
                               ("tonefilt_n_notes", 70, b"no multiple"), ("tonefilt_n_notes", 132, b"nNotes"),
                               ("tonefilt_output_period", 0.02, b"frame_size_sec"), ("frame_size_sec", 0.02, b"frame_size_sec"),
                               ("tonefilt_first_note", float("inf"), b"finite")):
        c = capi.chroma_filt_config()
        setattr(c, field, value)
        assert L.smilehip_plan_create_host_only(C.byref(c), C.byref(h)) != 0 and word in L.smilehip_last_error(), (field, L.smilehip_last_error())


def test_hard_signal_fixture_shape():
    from helpers import hard_signals
    h = np.load(os.path.join(GOLD, "hard_chroma_filt.npz"))
    assert sorted(h.files) == sorted(p + n for n in hard_signals.NAMES for p in ("chroma_", "tonespec_"))
    assert all(h["chroma_" + n].shape == (150, 12) and h["tonespec_" + n].shape == (150, 72) for n in hard_signals.NAMES)
    assert sum(1 for n in hard_signals.NAMES if (h["chroma_" + n] != 0).any()) >= 10


def test_hard_signals_on_the_host():
    """the hard-signal corpus through the g++ row functions: the binary's bits"""
    from helpers import hard_signals
    h = np.load(os.path.join(GOLD, "hard_chroma_filt.npz"))
    for name, pcm in hard_signals.signals().items():
        ts, _, _ = H.tonespec_rows(H.padded(pcm, 16000), 16000)
        assert_same_bits(ts, h["tonespec_" + name], "level tonespec, " + name)
        assert_same_bits(chroma_host.chroma_rows(ts), h["chroma_" + name], "level chroma, " + name)


def test_names_and_files(gold):
    for stem, n in (("u2_8000", 8000), ("u3_4000", 4000)):      # 16 kHz files of 8000 / 4000 samples
        lines = open(os.path.join(GOLD, "files", "chroma_filt_%s.csv" % stem)).read().splitlines()
        assert len(lines) == H.rows_of(n, 160) and all(len(ln.split(";")) == 12 for ln in lines) and not lines[0].startswith("'")


# ------------------------------------------------------------------------------------------------ the front end's mapping of the file
needs_exe = pytest.mark.skipif(not os.path.exists(EXE), reason="smilextract_hip not built")

# a minimal configuration text of the same graph, not the shipped file: own wording
MINIMAL = """
[componentInstances:cComponentManager]
instance[dataMemory].type=cDataMemory
instance[src].type=cWaveSource
instance[bank].type=cTonefilt
instance[fold].type=cChroma
instance[out].type=cCsvSink
[src:cWaveSource]
writer.dmLevel=pcm
filename=\\cm[inputfile(I){in.wav}:input]
monoMixdown=1
[bank:cTonefilt]
reader.dmLevel=pcm
writer.dmLevel=semitones
nNotes=72
firstNote=55
decayF0=0.9999
decayFN=0.999
outputPeriod=0.01
[fold:cChroma]
reader.dmLevel=semitones
writer.dmLevel=pitchclasses
nameAppend=chroma
copyInputName=0
processArrayFields=0
octaveSize=12
[out:cCsvSink]
reader.dmLevel=pitchclasses
filename=\\cm[outputfile(O){out.csv}:output]
delimChar=;
append=0
timestamp=0
number=0
printHeader=0
"""


def describe(path, *more, set_name="chroma_filt"):
    r = subprocess.run([EXE, "--set", set_name, "-C", path, "--describe", *more], capture_output=True, text=True)
    kv = dict(l.split("=", 1) for l in r.stdout.split("\n") if "=" in l)
    return r.returncode, kv, r.stderr


def write_conf(tmp_path, text, name="c.conf"):
    p = tmp_path / name
    p.write_text(text)
    return str(p)


@needs_exe
def test_minimal_text_maps_to_the_set(tmp_path):
    rc, kv, err = describe(write_conf(tmp_path, MINIMAL))
    assert rc == 0 and kv["preset"] == "chroma_filt" and "every processing component and option identical" in err, err
    assert not [k for k in kv if k.startswith("param.")]


@needs_exe
@pytest.mark.parametrize("tag", sorted(EDITED))
def test_allowed_edits_show_up(tmp_path, tag):
    text = MINIMAL
    for a, b in EDITED[tag]["minimal"].items():
        assert text.count(a) == 1, a
        text = text.replace(a, b)
    rc, kv, err = describe(write_conf(tmp_path, text))
    assert rc == 0 and kv["preset"] == "chroma_filt", err
    got = {k[6:]: float(v) for k, v in kv.items() if k.startswith("param.")}
    want = dict(tonefilt_n_notes=72, tonefilt_first_note=55, tonefilt_decay_f0=0.9999, tonefilt_decay_fn=0.999, tonefilt_output_period=0.01,
                chroma_octave_size=12, chroma_sil_thresh=float(np.float32(0.001)))
    want.update(EDITED[tag]["params"])
    assert got.keys() == want.keys() and all(abs(got[k] - want[k]) < 1e-9 for k in want), got


REFUSED = [  # (text of the minimal configuration, its replacement, what the message must name)
    ("octaveSize=12", "octaveSize=7", "octaveSize"),
    ("nNotes=72", "nNotes=70", "octaveSize"),              # no multiple of octaveSize: the binary writes rows of zeros
    ("nNotes=72", "nNotes=132", "nNotes"),
    ("firstNote=55", "firstNote=-1", "firstNote"),
    ("outputPeriod=0.01", "outputPeriod=0", "outputPeriod"),
    ("monoMixdown=1", "monoMixdown=0", "monoMixdown"),
    ("processArrayFields=0\noctaveSize", "processArrayFields=0\nnameAppend=pc\noctaveSize", "nameAppend"),
    ("copyInputName=0", "copyInputName=1", "copyInputName"),
    ("outputPeriod=0.01", "outputPeriod=0.01\noutputBuffersize=5", "outputBuffersize"),     # (no option of the component)
    ("printHeader=0", "printHeader=1", "printHeader"),
    ("timestamp=0", "timestamp=1", "timestamp"),
    ("reader.dmLevel=pitchclasses", "reader.dmLevel=semitones", "semitones"),
    ("reader.dmLevel=semitones", "reader.dmLevel=pcm", "pcm"),
    ("instance[out].type=cCsvSink", "instance[out].type=cCsvSink\ninstance[e].type=cEnergy", "cEnergy"),
]


@needs_exe
@pytest.mark.parametrize("old,new,option", REFUSED, ids=["%s:%s" % (r[2], r[1].split("\n")[-1]) for r in REFUSED])
def test_refused_edit_names_the_option(tmp_path, old, new, option):
    assert MINIMAL.count(old) == 1
    text = MINIMAL.replace(old, new)
    if "cEnergy" in new:
        text += "[e:cEnergy]\nreader.dmLevel=pcm\nwriter.dmLevel=energy\n"
    rc, kv, err = describe(write_conf(tmp_path, text))
    assert rc != 0 and "preset" not in kv
    assert option in err, err


@needs_exe
def test_plain_conf_keeps_refusing_the_file(tmp_path):
    p = write_conf(tmp_path, MINIMAL)
    r = subprocess.run([EXE, "-C", p, "--describe"], capture_output=True, text=True)
    assert r.returncode != 0 and "cannot run on the fused path" in r.stderr and "--set chroma_filt -C" in r.stderr
    rc, kv, err = describe(p, set_name="chroma_fft")       # the set name picks the walker
    assert rc != 0 and "chroma_fft.conf" in err
    r = subprocess.run([EXE, "--set", "chroma_filt"], capture_output=True, text=True)     # the set name is known: what is missing is the input
    assert r.returncode != 0 and "no input" in r.stderr and "--set must be" not in r.stderr


@needs_exe
@pytest.mark.skipif(not os.path.isdir(os.path.join(ROOT, "oracle", "_ref", "config")), reason="the reference's configuration files are not there (oracle/_ref not built)")
def test_shipped_file_is_recognised():
    conf = os.path.join(ROOT, "oracle", "_ref", "config", "chroma", "chroma_filt.conf")
    rc, kv, err = describe(conf)
    assert rc == 0 and kv["preset"] == "chroma_filt" and "every processing component and option identical" in err, err
    r = subprocess.run([EXE, "-C", conf, "--describe"], capture_output=True, text=True)
    assert r.returncode != 0 and "cannot run on the fused path" in r.stderr and "--set chroma_filt -C" in r.stderr
