"""config/prosody/prosodyShs.conf as a fused batch set, host part (no GPU): the preset and its geometry, the rows rule, the
element names, the front end's `--set prosody_shs -C file` mapping with its refusals, and the tail -- cPitchSmoother, cIntensity, cContourSmoother as
opensmile_amd/csrc/lld_prosody_ops.hpp states them, compiled with g++ (tests/helpers/prosody_shs_check.cpp) -- held to the real
binary's lld level bit for bit on the golden inputs (tests/golden/make_golden_prosody_shs.py), starting from the binary's own
cPitchShs rows. The GPU tests (tests/test_gpu_prosody_shs.py) then show that the kernels produce those rows and call the same
function on the right ones."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from opensmile_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "opensmile_amd", "smilextract_hip")
GOLD = os.path.join(ROOT, "tests", "golden")
CONF = os.path.join(ROOT, "oracle", "_ref", "config")
NAMES = ["F0final_sma", "voicingFinalUnclipped_sma", "pcm_loudness_sma"]


@pytest.fixture(scope="module")
def capi():
    from opensmile_amd import capi as m
    m.load()
    return m


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLD, "prosody_shs_synth.npz"))


@pytest.fixture(scope="module")
def ops():
    src = os.path.join(ROOT, "tests", "helpers", "prosody_shs_check.cpp")
    so = os.path.join(ROOT, "tests", "helpers", "_prosody_shs_check.so")
    hdrs = [os.path.join(ROOT, "opensmile_amd", "csrc", h) for h in ("lld_prosody_ops.hpp", "lld_is10_ops.hpp", "glibc_float.hpp")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(p) for p in [src] + hdrs):
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-mfma", "-o", so, src, "-lm"], check=True)
    L = C.CDLL(so)
    L.prosody_rows.restype = C.c_int64
    L.prosody_rows.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_float, C.c_int, C.c_int, C.c_double, C.c_double, C.c_void_p]
    for f in (L.prosody_pitch_level_windowed, L.prosody_pitch_level_sequential):
        f.restype = None
        f.argtypes = [C.c_void_p, C.c_int64, C.c_float, C.c_void_p]
    return L


def shs21(rows15):
    """The binary's pitchShs rows (nCandidates | F0Cand[4] | candVoicing[4] | candScore[4] | F0raw | voicingClip) in the library's
    21-value layout: six slots per field, the unused ones zero."""
    if np.ndim(rows15) == 2 and np.shape(rows15)[1] == 21:        # nCandidates = 6: the level has the library's layout already
        return np.ascontiguousarray(rows15, np.float32)
    r = np.asarray(rows15, np.float32).reshape(-1, 15)
    o = np.zeros((len(r), 21), np.float32)
    o[:, 0] = r[:, 0]
    for f in range(3):
        o[:, 1 + 6 * f:5 + 6 * f] = r[:, 1 + 4 * f:5 + 4 * f]
    o[:, 19:21] = r[:, 13:15]
    return o


def hamming_consts(N):
    """cIntensity::setupNamesForField (intensity.cpp:91-112): the window's first value and its sum in index order, in double"""
    s = 0.0
    for i in range(N):
        s += 0.54 - 0.46 * np.cos((2.0 * np.pi * float(i)) / (float(N) - 1.0))
    return 0.54 - 0.46 * np.cos(0.0), s


def host_rows(L, shs, pcm, N, H, W=1, cutoff=0.7):
    shs = np.ascontiguousarray(shs, np.float32)
    T = len(shs)
    out = np.zeros((max(T - 1 + W, 1), 3), np.float32)
    w0, ws = hamming_consts(N)
    if np.asarray(pcm).dtype == np.int16:
        p = np.ascontiguousarray(pcm, np.int16)
        rows = L.prosody_rows(shs.ctypes.data, T, p.ctypes.data, None, cutoff, W, H, w0, ws, out.ctypes.data)
    else:
        p = np.ascontiguousarray(pcm, np.float32)
        rows = L.prosody_rows(shs.ctypes.data, T, None, p.ctypes.data, cutoff, W, H, w0, ws, out.ctypes.data)
    return out[:rows]


def gold_pcm(gold, k):
    idx, n, fs = (int(v) for v in gold["inputs"][k])
    return (synth.utterance(idx, n) if n else np.zeros(0, np.int16)), fs


# ------------------------------------------------------------------------------------------------ preset, ABI, geometry
def test_preset_values_and_export(capi):
    assert "smilehip_config_prosody_shs" in capi.SYMBOLS
    hdr = open(os.path.join(ROOT, "include", "smilehip.h")).read()
    assert re.search(r"void\s+smilehip_config_prosody_shs\s*\(", hdr) and re.search(r"#define\s+SMILEHIP_CHAIN_PROSODY_SHS\s+7\b", hdr)
    c = capi.prosody_shs_config()
    assert c.chain_kind == 7 and c.struct_size == C.sizeof(capi.LldConfig)
    assert (c.frame_size_sec, c.frame_step_sec) == (0.050, 0.010)
    assert (c.win_func, c.win_sigma, c.win_gain, c.win_offset) == (capi.prosody_shs_config().win_func, 0.4, 1.0, 0.0)
    assert c.win_func == capi.compare16_f0_config().win_func                       # gauss
    assert c.zero_pad_symmetric == 0 and c.preemph == 0 and c.n_delta == 0
    assert (c.pitch_min, c.pitch_max, c.voicing_cutoff) == (52.0, 620.0, 0.7)
    assert c.shs_n_candidates == 4 and c.shs_n_harmonics == 15 and c.shs_compression == np.float32(0.85)
    assert c.shs_old_peak_algo == 1 and c.specscale_off == 0 and c.specscale_min_f in (0.0, 25.0)
    assert c.sma_win == 3


def test_geometry_and_rows(capi):
    L = capi.load()
    c = capi.prosody_shs_config()
    h = C.c_void_p()
    capi._check(L.smilehip_plan_create_host_only(C.byref(c), C.byref(h)))
    try:
        g = capi.Geometry()
        capi._check(L.smilehip_plan_geometry(h, C.byref(g)))
        assert (g.frame_size, g.frame_step, g.fft_size, g.n_bins, g.n_out) == (800, 160, 1024, 513, 3)
        # frame times of the rows: the time stamps of cPitchSmoother's level (frame j = input frame j + 1), the last one repeated
        L.smilehip_row_time.restype = C.c_double
        L.smilehip_row_time.argtypes = [C.c_void_p, C.c_int64, C.c_int64]
        assert [round(L.smilehip_row_time(h, 9, r), 6) for r in range(9)] == [0.01, 0.02, 0.03, 0.04, 0.05, 0.06, 0.07, 0.08, 0.08]
    finally:
        L.smilehip_plan_destroy(h)
    c.sma_win = 4
    assert L.smilehip_plan_create_host_only(C.byref(c), C.byref(h)) != 0 and b"smaWin" in L.smilehip_last_error()


def test_golden_rows_rule(gold):
    """what the binary writes: T - 1 + 1 rows for T >= 2 frames of 50 ms, none below; times (min(n, T - 2) + 1) x 10 ms"""
    for k, (idx, n, fs) in enumerate(gold["inputs"]):
        N, H = int(round(0.05 * fs)), int(round(0.01 * fs))
        T = 0 if n < N else (int(n) - N) // H + 1
        assert len(gold["shs_%d" % k]) == T
        rows = T if T >= 2 else 0
        assert gold["lld_%d" % k].shape == (rows, 3), (k, n, fs)
        want = [(min(r, T - 2) + 1) * 0.01 for r in range(rows)]
        assert np.allclose(gold["times_%d" % k], want, rtol=0, atol=1e-9)
    long_ones = [k for k, (idx, n, fs) in enumerate(gold["inputs"]) if n >= fs]
    assert long_ones
    for k in long_ones:                                    # both branches of F0final in every file of a second or more
        f0 = gold["lld_%d" % k][:, 0]
        assert (f0 > 0).sum() * 4 >= len(f0) and (f0 == 0).any()


# ------------------------------------------------------------------------------------------------ the tail on the host
def test_host_tail_equals_the_binary_bit_for_bit(ops, gold):
    from tolerance import assert_bits_equal
    for k, (idx, n, fs) in enumerate(gold["inputs"]):
        pcm, fs = gold_pcm(gold, k)
        N, H = int(round(0.05 * fs)), int(round(0.01 * fs))
        ref = gold["lld_%d" % k]
        shs = shs21(gold["shs_%d" % k])
        out = host_rows(ops, shs, pcm, N, H) if len(shs) else np.zeros((0, 3), np.float32)
        assert out.shape == ref.shape, (k, out.shape, ref.shape)
        if len(ref):
            assert_bits_equal(out, ref, "input %d (%d samples at %d Hz)" % (k, n, fs))
            # float samples (what smilehip_lld_run_f32 reads): the same bits
            assert_bits_equal(host_rows(ops, shs, (pcm.astype(np.float32) / np.float32(32767.0)).astype(np.float32), N, H), ref, "f32 %d" % k)


def test_host_tail_wider_windows(ops, gold):
    """smaWin 5 and 7 on short inputs: the rows the binary wrote for an edited copy of the file (recorded by the golden script)"""
    from tolerance import assert_bits_equal
    seen = 0
    for key in gold.files:
        m = re.match(r"lld_w(\d)_(\d+)$", key)
        if not m:
            continue
        sw, k = int(m.group(1)), int(m.group(2))
        pcm, fs = gold_pcm(gold, k)
        shs = shs21(gold["shs_%d" % k])
        out = host_rows(ops, shs, pcm, 800, 160, W=sw // 2)
        assert out.shape == gold[key].shape == (len(shs) - 1 + sw // 2, 3)
        assert_bits_equal(out, gold[key], key)
        seen += 1
    assert seen >= 8


def test_host_tail_with_edited_parameters(ops, gold):
    """copies of the file with the chain's other parameters edited (make_golden_prosody_shs.EDITS): the tail from the binary's own
    cPitchShs rows of that run; `all` has voicingCutoff = 0.6 and six candidates"""
    from tolerance import assert_bits_equal
    for tag, cutoff in (("maxpitch400", 0.7), ("all", 0.6)):
        for k in (7, 8):
            pcm, fs = gold_pcm(gold, k)
            out = host_rows(ops, shs21(gold["shs_%s_%d" % (tag, k)]), pcm, 800, 160, cutoff=cutoff)
            assert_bits_equal(out, gold["lld_%s_%d" % (tag, k)], "%s, input %d" % (tag, k))
    assert gold["lld_all_8"].tobytes() != gold["lld_8"].tobytes() and gold["shs_all_8"].shape[1] == 21


def test_windowed_smoother_replay_equals_the_sequential_pass(ops):
    """pitch_level_frame replays three calls from a cleared state; the component runs one pass over the whole contour. Random
    contours with every pattern of voiced / unvoiced runs, single-frame spikes, octave jumps up and down, at every position."""
    rng = np.random.default_rng(7)
    n_diff = 0
    for trial in range(400):
        T = int(rng.integers(2, 60))
        base = rng.choice([100.0, 200.0, 400.0, 150.0, 75.0])
        f0 = base * rng.choice([0.5, 1.0, 1.0, 1.0, 2.0, 1.19, 0.81, 1.21, 0.79], T) * rng.choice([1.0, 1.01], T)
        voiced = rng.random(T) < rng.choice([0.2, 0.5, 0.8, 0.95])
        v = np.where(voiced, 0.7 + 0.3 * rng.random(T), 0.7 * rng.random(T))
        v[rng.random(T) < 0.05] = 0.7                      # exactly the cut-off: unvoiced (the comparison is >)
        shs = np.zeros((T, 21), np.float32)
        shs[:, 1], shs[:, 7] = f0, v
        a, b = np.zeros((T - 1, 2), np.float32), np.zeros((T - 1, 2), np.float32)
        ops.prosody_pitch_level_windowed(shs.ctypes.data, T, 0.7, a.ctypes.data)
        ops.prosody_pitch_level_sequential(shs.ctypes.data, T, 0.7, b.ctypes.data)
        assert a.tobytes() == b.tobytes(), (trial, np.nonzero((a != b).any(axis=1))[0][:5])
        raw = np.where(shs[:-1, 7] > np.float32(0.7), shs[:-1, 1], 0)
        n_diff += int((b[1:, 0] != raw[1:]).sum())
    assert n_diff > 500                                    # the smoother did change contours: the test is not vacuous


def test_hard_signal_fixture_shape():
    h = np.load(os.path.join(GOLD, "hard_prosody_shs.npz"))
    from helpers import hard_signals
    assert sorted(h.files) == sorted("lld_" + n for n in hard_signals.NAMES)
    for n in hard_signals.NAMES:
        assert h["lld_" + n].shape == (146, 3)             # 1.5 s: T = 146 frames, T - 1 + 1 rows
    assert (h["lld_dc"][:, 2] > 0).all() and (h["lld_clicks_in_zeros"][:, 2] == 0).any()    # loudness through pow: DC and digital zero


# ------------------------------------------------------------------------------------------------ names, front end
def test_names_and_csv_header(gold):
    hdr = str(gold["csv_header"])
    assert hdr == "name;frameTime;" + ";".join(NAMES)
    src = open(os.path.join(ROOT, "opensmile_amd", "host", "feature_names.cpp")).read()
    for n in NAMES:
        assert '"%s"' % n in src
    for stem in ("u2_8000", "u3_4000"):
        lines = open(os.path.join(GOLD, "files", "prosody_shs_%s.csv" % stem)).read().splitlines()
        assert lines[0] == hdr and lines[1].startswith("'%s';0.010000;" % stem)


needs_exe = pytest.mark.skipif(not os.path.exists(EXE), reason="smilextract_hip not built")

# a minimal configuration text of the same graph, not the shipped file: own wording, no includes
MINIMAL = """
[componentInstances:cComponentManager]
instance[dataMemory].type=cDataMemory
instance[wave].type=cWaveSource
instance[fr].type=cFramer
instance[loud].type=cIntensity
instance[w].type=cWindower
instance[f].type=cTransformFFT
instance[m].type=cFFTmagphase
instance[oct].type=cSpecScale
instance[p].type=cPitchShs
instance[ps].type=cPitchSmoother
instance[sm].type=cContourSmoother
instance[out].type=cCsvSink
[wave:cWaveSource]
writer.dmLevel=wave
filename=\\cm[inputfile(I){in.wav}:input]
[fr:cFramer]
reader.dmLevel=wave
writer.dmLevel=frames
frameSize=0.05
frameStep=0.01
[loud:cIntensity]
reader.dmLevel=frames
writer.dmLevel=loudness
intensity=0
loudness=1
[w:cWindower]
reader.dmLevel=frames
writer.dmLevel=windowed
winFunc=gauss
sigma=0.4
[f:cTransformFFT]
reader.dmLevel=windowed
writer.dmLevel=spec
zeroPadSymmetric=0
[m:cFFTmagphase]
reader.dmLevel=spec
writer.dmLevel=mag
[oct:cSpecScale]
reader.dmLevel=mag
writer.dmLevel=octave
scale=octave
minF=25
specSmooth=1
specEnhance=1
auditoryWeighting=1
[p:cPitchShs]
reader.dmLevel=octave
writer.dmLevel=cands
minPitch=52
maxPitch=620
nCandidates=4
F0raw=1
voicingClip=1
[ps:cPitchSmoother]
reader.dmLevel=cands
writer.dmLevel=f0
octaveCorrection=0
voicingFinalUnclipped=1
[sm:cContourSmoother]
reader.dmLevel=f0;loudness
writer.dmLevel=lld
smaWin=3
[out:cCsvSink]
reader.dmLevel=lld
filename=\\cm[csvoutput{?}:csv]
"""


def describe(path):
    r = subprocess.run([EXE, "--set", "prosody_shs", "-C", path, "--describe"], capture_output=True, text=True)
    kv = dict(l.split("=", 1) for l in r.stdout.split("\n") if "=" in l)
    return r.returncode, kv, r.stderr


def write_conf(tmp_path, text, name="p.conf"):
    p = tmp_path / name
    p.write_text(text)
    return str(p)


@needs_exe
def test_minimal_text_maps_to_the_set(tmp_path):
    rc, kv, err = describe(write_conf(tmp_path, MINIMAL))
    assert rc == 0 and kv["preset"] == "prosody_shs", err
    assert float(kv["param.pitch_min"]) == 52 and float(kv["param.pitch_max"]) == 620 and float(kv["param.shs_n_candidates"]) == 4
    assert float(kv["param.sma_win"]) == 3 and float(kv["param.specscale_min_f"]) == 25 and float(kv["param.voicing_cutoff"]) == 0.7
    assert float(kv["param.shs_n_harmonics"]) == 15 and float(kv["param.shs_compression"]) == 0.85


@needs_exe
def test_edited_parameters_show_up(tmp_path):
    text = MINIMAL.replace("minPitch=52", "minPitch=60").replace("nCandidates=4", "nCandidates=6").replace("smaWin=3", "smaWin=5")
    text = text.replace("minF=25", "minF=20").replace("maxPitch=620", "maxPitch=400\nvoicingCutoff=0.6\nnHarmonics=12\ncompressionFactor=0.8")
    rc, kv, err = describe(write_conf(tmp_path, text))
    assert rc == 0 and kv["preset"] == "prosody_shs", err
    got = {k[6:]: float(v) for k, v in kv.items() if k.startswith("param.")}
    assert got == {"pitch_min": 60, "pitch_max": 400, "shs_n_candidates": 6, "sma_win": 5, "specscale_min_f": 20, "voicing_cutoff": 0.6,
                   "shs_n_harmonics": 12, "shs_compression": 0.8}


REFUSED = [  # (edit of the minimal text, the option the message must name)
    ("octaveCorrection=0\nvoicingFinalUnclipped=1", "octaveCorrection=0\nvoicingFinalUnclipped=1\npostSmoothing=1", "postSmoothing"),
    ("octaveCorrection=0\nvoicingFinalUnclipped=1", "octaveCorrection=0\nvoicingFinalUnclipped=1\npostSmoothingMethod=median", "postSmoothingMethod"),
    ("octaveCorrection=0\nvoicingFinalUnclipped=1", "octaveCorrection=0\nvoicingFinalUnclipped=1\nmedianFilter0=3", "medianFilter0"),
    ("octaveCorrection=0\nvoicingFinalUnclipped=1", "octaveCorrection=1\nvoicingFinalUnclipped=1", "octaveCorrection"),
    ("octaveCorrection=0\nvoicingFinalUnclipped=1", "voicingFinalUnclipped=1", "octaveCorrection"),            # the component's default is 1
    ("voicingFinalUnclipped=1", "voicingFinalUnclipped=1\nvoicingFinalClipped=1", "voicingFinalClipped"),
    ("voicingFinalUnclipped=1", "voicingFinalUnclipped=1\nF0finalEnv=1", "F0finalEnv"),
    ("voicingFinalUnclipped=1", "voicingFinalUnclipped=0", "voicingFinalUnclipped"),
    ("voicingFinalUnclipped=1", "voicingFinalUnclipped=1\nF0final=0", "F0final"),
    ("intensity=0", "intensity=1", "intensity"),
    ("loudness=1", "loudness=0", "loudness"),
    ("nCandidates=4", "nCandidates=7", "nCandidates"),
    ("nCandidates=4", "nCandidates=0", "nCandidates"),
    ("smaWin=3", "smaWin=4", "smaWin"),
    ("smaWin=3", "smaWin=11", "smaWin"),
    ("smaWin=3", "smaWin=3\nnoZeroSma=1", "noZeroSma"),
    ("smaWin=3", "smaWin=3\nnoPostEOIprocessing=1", "noPostEOIprocessing"),
    ("frameSize=0.05", "frameSize=0.06", "frameSize"),
    ("frameStep=0.01", "frameStep=0.02", "frameStep"),
    ("winFunc=gauss", "winFunc=ham", "winFunc"),
    ("sigma=0.4", "sigma=0.3", "sigma"),
    ("zeroPadSymmetric=0", "zeroPadSymmetric=1", "zeroPadSymmetric"),
    ("scale=octave", "scale=log", "scale"),
    ("specEnhance=1", "specEnhance=0", "specEnhance"),
    ("specSmooth=1", "specSmooth=0", "specSmooth"),
    ("auditoryWeighting=1", "auditoryWeighting=0", "auditoryWeighting"),
    ("F0raw=1", "F0raw=1\ngreedyPeakAlgo=1", "greedyPeakAlgo"),
    ("F0raw=1", "F0raw=1\noctaveCorrection=1", "octaveCorrection"),
    ("F0raw=1", "F0raw=1\nscores=0", "scores"),
    ("reader.dmLevel=f0;loudness", "reader.dmLevel=loudness;f0", "reader.dmLevel"),
]


@needs_exe
@pytest.mark.parametrize("old,new,option", REFUSED, ids=["%s:%s" % (r[2], r[1].split("\n")[-1]) for r in REFUSED])
def test_refused_edit_names_the_option(tmp_path, old, new, option):
    assert MINIMAL.count(old) == 1
    rc, kv, err = describe(write_conf(tmp_path, MINIMAL.replace(old, new)))
    assert rc != 0 and "preset" not in kv
    assert option in err, err


@needs_exe
def test_frame_modes_stay_refused(tmp_path):
    for mode in (["-frameMode", "fixed", "-frameSize", "1", "-frameStep", "1"], ["-frameMode", "list", "-frameList", "0-10"]):
        r = subprocess.run([EXE, "--set", "prosody_shs", "-I", os.path.join(GOLD, "files", "u2_8000.wav"), "-O", str(tmp_path / "o.htk"), *mode],
                           capture_output=True, text=True)
        assert r.returncode != 0 and "is09_emotion only" in r.stderr and not (tmp_path / "o.htk").exists()
    r = subprocess.run([EXE, "--set", "prosody_shs"], capture_output=True, text=True)     # the set name is known: what is missing is the input
    assert r.returncode != 0 and "no input" in r.stderr and "--set must be" not in r.stderr


@needs_exe
@pytest.mark.skipif(not os.path.isdir(CONF), reason="the reference's configuration files are not there (oracle/_ref not built)")
def test_shipped_file_is_recognised():
    rc, kv, err = describe(os.path.join(CONF, "prosody", "prosodyShs.conf"))
    assert rc == 0 and kv["preset"] == "prosody_shs" and "every processing component and option identical" in err
    assert not [k for k in kv if k.startswith("param.")]
    # -C alone maps what it mapped before: this file is refused there, with the way to run it
    r = subprocess.run([EXE, "-C", os.path.join(CONF, "prosody", "prosodyShs.conf"), "--describe"], capture_output=True, text=True)
    assert r.returncode != 0 and "cannot run on the fused path" in r.stderr and "--set prosody_shs -C" in r.stderr
