"""config/prosody/prosodyAcf.conf as a fused batch set, host part (no GPU): the preset and its geometry, the rows rule, the element
names, the front end's `--set prosody_acf -C file` mapping with its refusals, and what follows cAcf -- cPitchACF's voicing cut-off
and contour, cIntensity, cContourSmoother as opensmile_amd/csrc/lld_prosody_acf_ops.hpp states them, compiled with g++
(tests/helpers/prosody_acf_check.cpp) -- held to the real binary's `pitch`, `intens` and lld levels bit for bit on the golden inputs
(tests/golden/make_golden_prosody_acf.py), starting from the binary's own voiceProb and F0raw. The GPU tests
(tests/test_gpu_prosody_acf.py) then show that the kernels produce those values."""
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
NAMES = ["voiceProb_sma", "F0_sma", "pcm_loudness_sma"]


@pytest.fixture(scope="module")
def capi():
    from opensmile_amd import capi as m
    m.load()
    return m


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLD, "prosody_acf_synth.npz"))


@pytest.fixture(scope="module")
def ops():
    src = os.path.join(ROOT, "tests", "helpers", "prosody_acf_check.cpp")
    so = os.path.join(ROOT, "tests", "helpers", "_prosody_acf_check.so")
    hdrs = [os.path.join(ROOT, "opensmile_amd", "csrc", h)
            for h in ("lld_prosody_acf_ops.hpp", "lld_pitch_contour.hpp", "lld_prosody_ops.hpp", "lld_is10_ops.hpp", "glibc_float.hpp")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(p) for p in [src] + hdrs):
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-mfma", "-o", so, src, "-lm"], check=True)
    L = C.CDLL(so)
    L.prosody_acf_rows_of.restype = C.c_int64
    L.prosody_acf_rows_of.argtypes = [C.c_int64, C.c_int]
    L.prosody_acf_row_time_frame.restype = C.c_int64
    L.prosody_acf_row_time_frame.argtypes = [C.c_int64, C.c_int64]
    L.prosody_acf_levels.restype = None
    L.prosody_acf_levels.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_double, C.c_int, C.c_double, C.c_double, C.c_void_p]
    L.prosody_acf_smooth.restype = C.c_int64
    L.prosody_acf_smooth.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_void_p]
    return L


def hamming_consts(N):
    """cIntensity::setupNamesForField (intensity.cpp:91-112): the window's first value and its sum in index order, in double"""
    s = 0.0
    for i in range(N):
        s += 0.54 - 0.46 * np.cos((2.0 * np.pi * float(i)) / (float(N) - 1.0))
    return 0.54 - 0.46 * np.cos(0.0), s


def geometry(fs):
    """samples per 50 ms frame and per 10 ms step (lround, as the framer takes them)"""
    return int(np.floor(0.05 * fs + 0.5)), int(np.floor(0.01 * fs + 0.5))


def host_levels(L, voice_prob, f0raw, pcm, N, H, cutoff=0.55):
    vp = np.ascontiguousarray(voice_prob, np.float32).reshape(-1)
    raw = np.ascontiguousarray(f0raw, np.float32).reshape(-1)
    T = len(vp)
    assert len(raw) == T
    lv = np.zeros((max(T, 1), 3), np.float32)
    w0, ws = hamming_consts(N)
    if np.asarray(pcm).dtype == np.int16:
        p = np.ascontiguousarray(pcm, np.int16)
        L.prosody_acf_levels(vp.ctypes.data, raw.ctypes.data, T, p.ctypes.data, None, cutoff, H, w0, ws, lv.ctypes.data)
    else:
        p = np.ascontiguousarray(pcm, np.float32)
        L.prosody_acf_levels(vp.ctypes.data, raw.ctypes.data, T, None, p.ctypes.data, cutoff, H, w0, ws, lv.ctypes.data)
    return lv[:T]


def host_smooth(L, level, W=1):
    lv = np.ascontiguousarray(level, np.float32).reshape(-1, 3)
    T = len(lv)
    out = np.zeros((T + W + 1, 3), np.float32)
    rows = L.prosody_acf_smooth(lv.ctypes.data, T, W, out.ctypes.data)
    return out[:rows]


def gold_pcm(gold, k):
    idx, n, fs = (int(v) for v in gold["inputs"][k])
    return (synth.utterance(idx, n) if n else np.zeros(0, np.int16)), fs


# ------------------------------------------------------------------------------------------------ preset, ABI, geometry
def test_preset_values_and_export(capi):
    assert "smilehip_config_prosody_acf" in capi.SYMBOLS and "smilehip_batch_prosody_acf_taps" in capi.SYMBOLS
    hdr = open(os.path.join(ROOT, "include", "smilehip.h")).read()
    assert re.search(r"void\s+smilehip_config_prosody_acf\s*\(", hdr) and re.search(r"#define\s+SMILEHIP_CHAIN_PROSODY_ACF\s+8\b", hdr)
    assert re.search(r"int\s+smilehip_batch_prosody_acf_taps\s*\(", hdr)
    c = capi.prosody_acf_config()
    assert c.chain_kind == 8 == capi.CHAIN_PROSODY_ACF and c.struct_size == C.sizeof(capi.LldConfig)
    assert (c.frame_size_sec, c.frame_step_sec) == (0.050, 0.010)
    assert (c.win_func, c.win_sigma, c.win_gain, c.win_offset) == (capi.compare16_f0_config().win_func, 0.4, 1.0, 0.0)   # gauss
    assert c.zero_pad_symmetric == 0 and c.preemph == 0 and c.n_delta == 0
    assert (c.pitch_max, c.voicing_cutoff, c.sma_win) == (500.0, 0.55, 3)
    assert c.acf_cep_use_power == 0                        # [cep:cAcf] does not set usePower: the cepstrum of log(mag + 1)
    # the new field is the struct's last one and the other presets leave it zero
    assert capi.LldConfig._fields_[-1][0] == "acf_cep_use_power"
    assert capi.prosody_shs_config().acf_cep_use_power == 0 and capi.is09_lld_config().acf_cep_use_power == 0


def test_geometry_rows_and_refusals(capi, ops):
    L = capi.load()
    for fs, want in ((8000, (400, 80, 512)), (11025, (551, 110, 1024)), (16000, (800, 160, 1024)), (22050, (1103, 221, 2048)),
                     (32000, (1600, 320, 2048)), (44100, (2205, 441, 4096)), (48000, (2400, 480, 4096))):
        c = capi.prosody_acf_config()
        c.sample_rate = fs
        h = C.c_void_p()
        capi._check(L.smilehip_plan_create_host_only(C.byref(c), C.byref(h)))
        try:
            g = capi.Geometry()
            capi._check(L.smilehip_plan_geometry(h, C.byref(g)))
            assert (g.frame_size, g.frame_step, g.fft_size) == want and g.n_bins == want[2] // 2 + 1 and (g.n_static, g.n_out) == (3, 3)
            assert (g.frame_size, g.frame_step) == geometry(fs)
            for T in (1, 2, 3, 9):
                for W in (1, 2, 4):
                    rows = ops.prosody_acf_rows_of(T, W)
                    for r in range(rows):
                        assert L.smilehip_row_time(h, T, r) == L.smilehip_frame_time(h, ops.prosody_acf_row_time_frame(T, r))
            assert [round(L.smilehip_row_time(h, 9, r) / c.frame_step_sec) for r in range(10)] == [0, 1, 2, 3, 4, 5, 6, 7, 8, 8]
            assert [round(L.smilehip_row_time(h, 1, r) / c.frame_step_sec) for r in range(2)] == [0, 1]
        finally:
            L.smilehip_plan_destroy(h)
    h = C.c_void_p()
    for field, value, word in (("sma_win", 4, b"sma_win"), ("sma_win", 11, b"sma_win"), ("sma_win", 1, b"sma_win"), ("n_delta", 1, b"n_delta"),
                               ("preemph", 1, b"preemph"), ("zero_pad_symmetric", 1, b"zero_pad_symmetric"),
                               ("acf_cep_use_power", 2, b"acf_cep_use_power"), ("frame_size_sec", 0.001, b"transform length"),
                               ("frame_size_sec", 0.6, b"8192")):
        c = capi.prosody_acf_config()
        setattr(c, field, value)
        assert L.smilehip_plan_create_host_only(C.byref(c), C.byref(h)) != 0 and word in L.smilehip_last_error(), (field, L.smilehip_last_error())


def test_rows_of_is_the_measured_rule(ops, gold):
    """what the binary writes: T + smaWin / 2 rows for T >= 1 frames of 50 ms, none for T = 0 (the 0, 100 and 799 sample inputs);
    row n carries the time of frame min(n, T - 1), the second row of the one-frame input that of frame 1"""
    seen_T = set()
    for k, (idx, n, fs) in enumerate(gold["inputs"]):
        N, H = geometry(int(fs))
        T = 0 if n < N else (int(n) - N) // H + 1
        seen_T.add(T)
        assert len(gold["pitch_%d" % k]) == len(gold["intens_%d" % k]) == len(gold["f0raw_%d" % k]) == T, (k, T)
        rows = ops.prosody_acf_rows_of(T, 1)
        assert rows == (T + 1 if T >= 1 else 0)
        assert gold["lld_%d" % k].shape == (rows, 3), (k, n, fs)
        period = H / float(fs)
        want = [ops.prosody_acf_row_time_frame(T, r) * period for r in range(rows)]
        assert np.allclose(gold["times_%d" % k], want, rtol=0, atol=6e-7), (k, gold["times_%d" % k][-3:], want[-3:])   # (the CSV has six decimals)
    assert {0, 1, 2, 3, 4, 9} <= seen_T
    assert sorted(set(int(fs) for _, _, fs in gold["inputs"])) == [8000, 11025, 16000, 22050, 32000, 44100, 48000]
    for sw in (5, 7, 9):
        for k in (4, 5, 6, 7, 8):
            assert len(gold["lld_w%d_%d" % (sw, k)]) == ops.prosody_acf_rows_of(len(gold["pitch_%d" % k]), sw // 2)
    long_ones = [k for k, (idx, n, fs) in enumerate(gold["inputs"]) if n >= fs]
    assert len(long_ones) >= 2
    reonset = False
    for k in long_ones:                                    # both branches of F0 in every input of a second or more ...
        f0 = gold["lld_%d" % k][:, 1]
        assert (f0 > 0).any() and (f0 == 0).any()
        v = np.where(gold["pitch_%d" % k][:, 0].astype(np.float64) < 0.55, 0, gold["f0raw_%d" % k][:, 0]) > 0
        reonset = reonset or any(v[i] and not v[i - 1] and v[:i - 1].any() for i in range(2, len(v)))
    assert reonset                                         # ... and a voiced run that starts after an unvoiced one: the contour's onset branches


# ------------------------------------------------------------------------------------------------ the row functions on the host
def test_host_levels_and_rows_equal_the_binary_bit_for_bit(ops, gold):
    from tolerance import assert_bits_equal
    n_contour = 0
    for k, (idx, n, fs) in enumerate(gold["inputs"]):
        pcm, fs = gold_pcm(gold, k)
        N, H = geometry(fs)
        pitch, intens, raw, ref = gold["pitch_%d" % k], gold["intens_%d" % k], gold["f0raw_%d" % k], gold["lld_%d" % k]
        T = len(pitch)
        if T == 0:
            assert len(ref) == 0
            continue
        what = "input %d (%d samples at %d Hz)" % (k, n, fs)
        lv = host_levels(ops, pitch[:, 0], raw[:, 0], pcm, N, H)
        assert_bits_equal(lv[:, :2], pitch, "level pitch, " + what)       # voicing cut-off + contour
        assert_bits_equal(lv[:, 2:], intens, "level intens, " + what)     # loudness from the samples
        n_contour += int((lv[:, 1] != np.where(pitch[:, 0] < 0.55, 0, raw[:, 0])).sum())
        assert_bits_equal(host_smooth(ops, lv), ref, "lld, " + what)
        # float samples (what smilehip_lld_run_f32 reads): the same bits
        lf = host_levels(ops, pitch[:, 0], raw[:, 0], (pcm.astype(np.float32) / np.float32(32767.0)).astype(np.float32), N, H)
        assert lf.tobytes() == lv.tobytes()
    assert n_contour > 100                                 # the contour did change the candidates: the test is not vacuous


def test_host_rows_wider_windows(ops, gold):
    """smaWin 5, 7 and 9 on short inputs: the rows the binary wrote for an edited copy of the file (recorded by the golden script)"""
    from tolerance import assert_bits_equal
    seen = 0
    for key in gold.files:
        m = re.match(r"lld_w(\d)_(\d+)$", key)
        if not m:
            continue
        sw, k = int(m.group(1)), int(m.group(2))
        lv = np.concatenate([gold["pitch_%d" % k], gold["intens_%d" % k]], axis=1)
        out = host_smooth(ops, lv, W=sw // 2)
        assert out.shape == gold[key].shape == (len(lv) + sw // 2, 3)
        assert_bits_equal(out, gold[key], key)
        seen += 1
    assert seen == 15


def test_host_rows_with_edited_parameters(ops, gold):
    """copies of the file with maxPitch = 300 and voicingCutoff = 0.7, and with voicingCutoff = 1.5 (clamped to 1, pitchACF.cpp:96-98):
    levels and rows from the binary's own voiceProb / F0raw of that run"""
    from tolerance import assert_bits_equal
    for tag, cutoff in (("mp300", 0.7), ("vc15", 1.5)):
        for k in (7, 8):
            pcm, fs = gold_pcm(gold, k)
            pitch, raw = gold["pitch_%s_%d" % (tag, k)], gold["f0raw_%s_%d" % (tag, k)]
            lv = host_levels(ops, pitch[:, 0], raw[:, 0], pcm, 800, 160, cutoff=cutoff)
            assert_bits_equal(lv[:, :2], pitch, "%s, level pitch, input %d" % (tag, k))
            assert_bits_equal(host_smooth(ops, lv), gold["lld_%s_%d" % (tag, k)], "%s, input %d" % (tag, k))
        assert gold["lld_%s_8" % tag].tobytes() != gold["lld_8"].tobytes()
    assert (gold["pitch_vc15_8"][:, 0] < 1.0).all() and (gold["pitch_vc15_8"][:, 1] == 0).all()    # cut-off 1: nothing is voiced
    assert (gold["pitch_mp300_8"][:, 0] != gold["pitch_8"][:, 0]).any()                            # maxPitch moves the ACF peak search: voiceProb


def test_hard_signal_fixture_shape():
    h = np.load(os.path.join(GOLD, "hard_prosody_acf.npz"))
    from helpers import hard_signals
    assert sorted(h.files) == sorted("lld_" + n for n in hard_signals.NAMES)
    for n in hard_signals.NAMES:
        assert h["lld_" + n].shape == (147, 3)             # 1.5 s: T = 146 frames, T + 1 rows
    assert (h["lld_dc"][:, 2] > 0).all() and (h["lld_clicks_in_zeros"][:, 2] == 0).any()    # loudness through pow: DC and digital zero


# ------------------------------------------------------------------------------------------------ names, front end
def test_names_and_csv_header(gold):
    hdr = str(gold["csv_header"])
    assert hdr == "name;frameTime;" + ";".join(NAMES)
    src = open(os.path.join(ROOT, "opensmile_amd", "host", "feature_names.cpp")).read()
    for n in NAMES:
        assert '"%s"' % n in src
    for stem in ("u2_8000", "u3_4000"):
        lines = open(os.path.join(GOLD, "files", "prosody_acf_%s.csv" % stem)).read().splitlines()
        assert lines[0] == hdr and lines[1].startswith("'%s';0.000000;" % stem)


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
instance[ac].type=cAcf
instance[ce].type=cAcf
instance[p].type=cPitchACF
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
[ac:cAcf]
reader.dmLevel=mag
writer.dmLevel=lags
[ce:cAcf]
reader.dmLevel=mag
writer.dmLevel=quef
cepstrum=1
[p:cPitchACF]
reader.dmLevel=lags;quef
writer.dmLevel=f0
processArrayFields=0
maxPitch=500
voicingCutoff=0.55
voiceProb=1
F0=1
[sm:cContourSmoother]
reader.dmLevel=f0;loudness
writer.dmLevel=lld
smaWin=3
[out:cCsvSink]
reader.dmLevel=lld
filename=\\cm[csvoutput{?}:csv]
"""


def describe(path):
    r = subprocess.run([EXE, "--set", "prosody_acf", "-C", path, "--describe"], capture_output=True, text=True)
    kv = dict(l.split("=", 1) for l in r.stdout.split("\n") if "=" in l)
    return r.returncode, kv, r.stderr


def write_conf(tmp_path, text, name="p.conf"):
    p = tmp_path / name
    p.write_text(text)
    return str(p)


@needs_exe
def test_minimal_text_maps_to_the_set(tmp_path):
    rc, kv, err = describe(write_conf(tmp_path, MINIMAL))
    assert rc == 0 and kv["preset"] == "prosody_acf", err
    got = {k[6:]: float(v) for k, v in kv.items() if k.startswith("param.")}
    assert got == {"pitch_max": 500, "voicing_cutoff": 0.55, "sma_win": 3}


@needs_exe
def test_edited_parameters_show_up(tmp_path):
    text = MINIMAL.replace("maxPitch=500", "maxPitch=300").replace("voicingCutoff=0.55", "voicingCutoff=0.7").replace("smaWin=3", "smaWin=5")
    rc, kv, err = describe(write_conf(tmp_path, text))
    assert rc == 0 and kv["preset"] == "prosody_acf", err
    got = {k[6:]: float(v) for k, v in kv.items() if k.startswith("param.")}
    assert got == {"pitch_max": 300, "voicing_cutoff": 0.7, "sma_win": 5}
    # voicingCutoff is clamped as cPitchACF::myFetchConfig does (pitchACF.cpp:96-98)
    rc, kv, err = describe(write_conf(tmp_path, MINIMAL.replace("voicingCutoff=0.55", "voicingCutoff=1.5")))
    assert rc == 0 and float(kv["param.voicing_cutoff"]) == 1.0, err
    rc, kv, err = describe(write_conf(tmp_path, MINIMAL.replace("voicingCutoff=0.55", "voicingCutoff=-2")))
    assert rc == 0 and float(kv["param.voicing_cutoff"]) == 0.0, err


REFUSED = [  # (text of the minimal configuration, its replacement, the option the message must name)
    ("voiceProb=1", "voiceProb=0", "voiceProb"),
    ("F0=1", "F0=0", "F0"),
    ("F0=1", "F0=1\nF0raw=1", "F0raw"),
    ("F0=1", "F0=1\nF0env=1", "F0env"),
    ("F0=1", "F0=1\nHNR=1", "HNR"),
    ("F0=1", "F0=1\nHNRdB=1", "HNRdB"),
    ("F0=1", "F0=1\nlinHNR=1", "linHNR"),
    ("F0=1", "F0=1\nvoiceQual=1", "voiceQual"),
    ("writer.dmLevel=lags", "writer.dmLevel=lags\nusePower=0", "usePower"),
    ("writer.dmLevel=lags", "writer.dmLevel=lags\ncepstrum=1", "cepstrum"),
    ("writer.dmLevel=lags", "writer.dmLevel=lags\nacfCepsNormOutput=0", "acfCepsNormOutput"),
    ("cepstrum=1", "cepstrum=1\nusePower=1", "usePower"),
    ("cepstrum=1", "cepstrum=0", "cepstrum"),
    ("cepstrum=1", "cepstrum=1\nacfCepsNormOutput=0", "acfCepsNormOutput"),
    ("cepstrum=1", "cepstrum=1\ncosLifterCepstrum=1", "cosLifterCepstrum"),
    ("cepstrum=1", "cepstrum=1\nabsCepstrum=1", "absCepstrum"),
    ("cepstrum=1", "cepstrum=1\noldCompatCepstrum=1", "oldCompatCepstrum"),
    ("cepstrum=1", "cepstrum=1\nsymmetricData=0", "symmetricData"),
    ("winFunc=gauss", "winFunc=ham", "winFunc"),
    ("sigma=0.4", "sigma=0.3", "sigma"),
    ("sigma=0.4", "sigma=0.4\ngain=2", "gain"),
    ("frameSize=0.05", "frameSize=0.06", "frameSize"),
    ("frameStep=0.01", "frameStep=0.02", "frameStep"),
    ("frameStep=0.01", "frameStep=0.01\nframeCenterSpecial=center", "frameCenterSpecial"),
    ("zeroPadSymmetric=0", "zeroPadSymmetric=1", "zeroPadSymmetric"),
    ("intensity=0", "intensity=1", "intensity"),
    ("loudness=1", "loudness=0", "loudness"),
    ("reader.dmLevel=f0;loudness", "reader.dmLevel=loudness;f0", "reader.dmLevel"),
    ("reader.dmLevel=lags;quef", "reader.dmLevel=quef;lags", "reader.dmLevel"),
    ("smaWin=3", "smaWin=4", "smaWin"),
    ("smaWin=3", "smaWin=11", "smaWin"),
    ("smaWin=3", "smaWin=3\nnoZeroSma=1", "noZeroSma"),
    ("smaWin=3", "smaWin=3\nnoPostEOIprocessing=1", "noPostEOIprocessing"),
    ("processArrayFields=0\nmaxPitch", "processArrayFields=1\nmaxPitch", "processArrayFields"),
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
        r = subprocess.run([EXE, "--set", "prosody_acf", "-I", os.path.join(GOLD, "files", "u2_8000.wav"), "-O", str(tmp_path / "o.htk"), *mode],
                           capture_output=True, text=True)
        assert r.returncode != 0 and "is09_emotion only" in r.stderr and not (tmp_path / "o.htk").exists()
    r = subprocess.run([EXE, "--set", "prosody_acf"], capture_output=True, text=True)     # the set name is known: what is missing is the input
    assert r.returncode != 0 and "no input" in r.stderr and "--set must be" not in r.stderr


@needs_exe
def test_the_other_prosody_set_keeps_its_own_graph(tmp_path):
    """--set prosody_shs -C refuses this graph and --set prosody_acf -C refuses that one: the set name picks the walker"""
    p = write_conf(tmp_path, MINIMAL)
    r = subprocess.run([EXE, "--set", "prosody_shs", "-C", p, "--describe"], capture_output=True, text=True)
    assert r.returncode != 0 and "prosodyShs.conf" in r.stderr
    r = subprocess.run([EXE, "-C", p, "--describe"], capture_output=True, text=True)      # plain -C: refused, with the way to run it
    assert r.returncode != 0 and "cannot run on the fused path" in r.stderr and "--set prosody_acf -C" in r.stderr


@needs_exe
@pytest.mark.skipif(not os.path.isdir(CONF), reason="the reference's configuration files are not there (oracle/_ref not built)")
def test_shipped_file_is_recognised():
    rc, kv, err = describe(os.path.join(CONF, "prosody", "prosodyAcf.conf"))
    assert rc == 0 and kv["preset"] == "prosody_acf" and "every processing component and option identical" in err
    assert not [k for k in kv if k.startswith("param.")]
    # -C alone maps what it mapped before: this file is refused there, with the way to run it
    r = subprocess.run([EXE, "-C", os.path.join(CONF, "prosody", "prosodyAcf.conf"), "--describe"], capture_output=True, text=True)
    assert r.returncode != 0 and "cannot run on the fused path" in r.stderr and "--set prosody_acf -C" in r.stderr
