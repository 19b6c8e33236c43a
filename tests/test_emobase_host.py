"""config/emobase/emobase.conf, levels lld and lld_de, as a fused batch set -- host part (no GPU): the preset and its geometry, the row
rule, the element names, the front end's `--set emobase -C file` mapping with its refusals, and everything of the chain that is
__host__ __device__ in opensmile_amd/csrc/lld_emobase_ops.hpp, compiled with g++ (tests/helpers/emobase_check.cpp) and held to the
real binary's levels bit for bit on the golden inputs (tests/golden/make_golden_emobase.py), in two steps: from the tapped levels
intens | mfcc1 | lsp | mzcr | pitch to lld and lld_de on every input and window width (the row rule, the time stamps), and from the
samples to the tapped levels (cIntensity, cMZcr, cLpc, cLsp; cPitchACF's cut-off, contour and F0env from the binary's own voiceProb
and F0raw). The GPU tests (tests/test_gpu_emobase.py) then show that the kernels produce those values."""
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
LEVELS25 = ("intens", "mfcc1", "lsp", "mzcr")


def names(p=8):
    base = [("pcm_intensity", ""), ("pcm_loudness", "")] + [("mfcc", "[%d]" % i) for i in range(1, 13)] + \
           [("lspFreq", "[%d]" % i) for i in range(p)] + [(n, "") for n in ("pcm_zcr", "voiceProb", "F0", "F0env")]
    return [a + "_sma" + b for a, b in base] + [a + "_sma_de" + b for a, b in base]


@pytest.fixture(scope="module")
def capi():
    from opensmile_amd import capi as m
    m.load()
    return m


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLD, "emobase_synth.npz"))


@pytest.fixture(scope="module")
def ops():
    src = os.path.join(ROOT, "tests", "helpers", "emobase_check.cpp")
    so = os.path.join(ROOT, "tests", "helpers", "_emobase_check.so")
    hdrs = [os.path.join(ROOT, "opensmile_amd", "csrc", h)
            for h in ("lld_emobase_ops.hpp", "lld_prosody_acf_ops.hpp", "lld_pitch_contour.hpp", "lld_prosody_ops.hpp", "lld_is10_ops.hpp", "glibc_float.hpp")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(p) for p in [src] + hdrs):
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-mfma", "-o", so, src, "-lm"], check=True)
    L = C.CDLL(so)
    L.emobase_rows_of.restype = C.c_int64
    L.emobase_rows_of.argtypes = [C.c_int64, C.c_int64, C.c_int]
    L.emobase_row_time_frame.restype = C.c_int64
    L.emobase_row_time_frame.argtypes = [C.c_int64, C.c_int64, C.c_int, C.c_int64]
    L.emobase_frames25.restype = None
    L.emobase_frames25.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_float, C.c_double, C.c_double, C.c_double, C.c_int, C.c_void_p]
    L.emobase_pitch_level.restype = None
    L.emobase_pitch_level.argtypes = [C.c_void_p, C.c_int64, C.c_double]
    L.emobase_rows.restype = C.c_int64
    L.emobase_rows.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p]
    return L


def hamming_consts(N):
    """cIntensity::setupNamesForField (intensity.cpp:91-112): the window's first two values and its sum in index order, in double"""
    w = [0.54 - 0.46 * np.cos((2.0 * np.pi * float(i)) / (float(N) - 1.0)) for i in range(N)]
    s = 0.0
    for v in w:
        s += v
    return w[0], w[1], s


def geometry(fs):
    """samples per 25 ms frame, per 40 ms frame and per 10 ms step (lround, as the framers take them)"""
    return int(np.floor(0.025 * fs + 0.5)), int(np.floor(0.04 * fs + 0.5)), int(np.floor(0.01 * fs + 0.5))


def frames_of(n, N, H):
    return 0 if n < N else (n - N) // H + 1


def gold_pcm(gold, k):
    idx, n, fs = (int(v) for v in gold["inputs"][k])
    return (synth.utterance(idx, n) if n else np.zeros(0, np.int16)), fs


def as_f32(pcm):
    return (np.asarray(pcm).astype(np.float32) / np.float32(32767.0)).astype(np.float32)


def level25(gold, k, sfx=""):
    return np.ascontiguousarray(np.concatenate([gold["%s_%s%d" % (lv, sfx, k)] for lv in LEVELS25], axis=1), np.float32)


def host_rows(L, a25, p3, W=1):
    a25, p3 = np.ascontiguousarray(a25, np.float32), np.ascontiguousarray(p3, np.float32).reshape(-1, 3)
    n25 = a25.shape[1]
    out = np.zeros((len(p3) + W + 1, 2 * (n25 + 3)), np.float32)
    rows = L.emobase_rows(a25.ctypes.data, len(a25), p3.ctypes.data, len(p3), n25, W, out.ctypes.data)
    return out[:rows]


def host_frames25(L, pcm, fs, p=8):
    """(intens, mzcr, lpc, lsp) of every 25 ms frame from the samples"""
    N, _, H = geometry(fs)
    x = np.ascontiguousarray(pcm if np.asarray(pcm).dtype == np.float32 else as_f32(pcm))
    T = frames_of(len(x), N, H)
    o = np.zeros((max(T, 1), 3 + 2 * p), np.float32)
    w0, w1, ws = hamming_consts(N)
    L.emobase_frames25(x.ctypes.data, T, N, H, 0.97, w0, w1, ws, p, o.ctypes.data)
    o = o[:T]
    return o[:, :2], o[:, 2:3], o[:, 3:3 + p], o[:, 3 + p:]


def host_pitch(L, voice_prob, f0raw, cutoff=0.55):
    T = len(voice_prob)
    p3 = np.ascontiguousarray(np.concatenate([voice_prob.reshape(-1, 1), f0raw.reshape(-1, 1), np.zeros((T, 1), np.float32)], axis=1), np.float32)
    L.emobase_pitch_level(p3.ctypes.data, T, cutoff)
    return p3


# ------------------------------------------------------------------------------------------------ preset, ABI, geometry
def test_preset_values_and_export(capi):
    for sym in ("smilehip_config_emobase", "smilehip_batch_emobase_taps", "smilehip_plan_set_lpc_order", "smilehip_plan_get_lpc_order",
                "smilehip_plan_emobase_frame40"):
        assert sym in capi.SYMBOLS
    hdr = open(os.path.join(ROOT, "include", "smilehip.h")).read()
    assert re.search(r"void\s+smilehip_config_emobase\s*\(", hdr) and re.search(r"#define\s+SMILEHIP_CHAIN_EMOBASE\s+13\b", hdr)
    assert re.search(r"int\s+smilehip_batch_emobase_taps\s*\(", hdr) and re.search(r"int\s+smilehip_plan_set_lpc_order\s*\(", hdr)
    c = capi.emobase_config()
    assert c.chain_kind == 13 == capi.CHAIN_EMOBASE
    assert c.struct_size == 280 == capi.is09_lld_config().struct_size          # SMILEHIP_LLD_CONFIG_SIZE_V1, what every V1 preset reports
    assert (c.frame_size_sec, c.frame_step_sec) == (0.025, 0.010)
    assert (c.preemph, c.preemph_de, c.zero_pad_symmetric, c.win_gain, c.win_offset) == (1, 0, 0, 1.0, 0.0) and abs(c.preemph_k - 0.97) < 1e-7
    assert (c.n_bands, c.lofreq, c.hifreq, c.use_power, c.mel_htk_compatible) == (26, 0.0, 8000.0, 1, 1)
    assert (c.first_mfcc, c.last_mfcc, c.cep_lifter, c.mfcc_htk_compatible) == (1, 12, 22.0, 1)
    assert (c.n_delta, c.delta_win, c.pitch_max, c.voicing_cutoff, c.sma_win) == (1, 2, 500.0, 0.55, 3)
    # the existing presets report the sizes they reported before
    assert capi.prosody_acf_config().struct_size == 280 and capi.chroma_fft_config().struct_size == 312
    assert capi.chroma_filt_config().struct_size == 352 and C.sizeof(capi.LldConfig) == 280


def test_geometry_rows_and_refusals(capi, ops):
    L = capi.load()
    want = {8000: (200, 80, 256, 320, 512), 11025: (276, 110, 512, 441, 512), 16000: (400, 160, 512, 640, 1024), 22050: (551, 221, 1024, 882, 1024),
            32000: (800, 320, 1024, 1280, 2048), 44100: (1103, 441, 2048, 1764, 2048), 48000: (1200, 480, 2048, 1920, 2048)}
    for fs, (N25, H, F25, N40, F40) in want.items():
        p = capi.Plan(None, capi.emobase_config(fs))
        g = p.geometry
        assert (g.frame_size, g.frame_step, g.fft_size, g.n_static, g.n_out) == (N25, H, F25, 26, 52)
        assert p.emobase_frame40() == (N40, F40) and (N25, N40, H) == geometry(fs)
        assert p.lpc_order() == 8
        for T25, T40 in ((1, 0), (2, 1), (3, 1), (3, 2), (4, 2), (11, 10)):
            for sw in (3, 5, 9):
                W = sw // 2
                rows = ops.emobase_rows_of(T25, T40, W)
                assert rows == (T40 + W if T40 else 0)
                if sw == 3:
                    for r in range(rows):
                        assert L.smilehip_row_time(p._h, T25, r) == L.smilehip_frame_time(p._h, ops.emobase_row_time_frame(T25, T40, W, r))
        p.set_lpc_order(10)
        assert p.lpc_order() == 10 and (p.geometry.n_static, p.geometry.n_out) == (28, 56)
        for bad in (0, 1, 7, 18, -2):
            assert L.smilehip_plan_set_lpc_order(p._h, bad) != 0 and b"cLpc p" in L.smilehip_last_error()
        p.close()
    other = capi.Plan(None, capi.is09_lld_config())
    assert L.smilehip_plan_set_lpc_order(other._h, 8) != 0 and b"not an emobase plan" in L.smilehip_last_error()
    other.close()
    h = C.c_void_p()
    for field, value, word in (("sma_win", 4, b"sma_win"), ("sma_win", 11, b"sma_win"), ("sma_win", 1, b"sma_win"), ("n_delta", 2, b"n_delta"),
                               ("delta_win", 3, b"delta_win"), ("preemph", 0, b"preemph"), ("zero_pad_symmetric", 1, b"zero_pad_symmetric"),
                               ("last_mfcc", 10, b"12 coefficients"), ("append_log_energy", 1, b"append_log_energy"), ("cms", 1, b"cms"),
                               ("frame_size_sec", 0.05, b"0.040"), ("frame_size_sec", 0.001, b"mel bank")):
        c = capi.emobase_config()
        setattr(c, field, value)
        assert L.smilehip_plan_create_host_only(C.byref(c), C.byref(h)) != 0 and word in L.smilehip_last_error(), (field, L.smilehip_last_error())


def test_rows_of_is_the_measured_rule(ops, gold):
    """what the binary writes: T40 + smaWin / 2 rows for T40 >= 1 frames of 40 ms, none for T40 = 0 -- whatever the number of 25 ms frames
    (the 400, 560 and 639 sample inputs have one or two and no row); row n carries the time of frame n for n < smaWin / 2, of frame
    min(n, T25 - 1) otherwise"""
    seen = set()
    for k, (idx, n, fs) in enumerate(gold["inputs"]):
        N25, N40, H = geometry(int(fs))
        T25, T40 = frames_of(int(n), N25, H), frames_of(int(n), N40, H)
        seen.add((T25, T40))
        for lv in LEVELS25 + ("lpc",):
            assert len(gold["%s_%d" % (lv, k)]) == T25, (lv, k)
        assert len(gold["pitch_%d" % k]) == len(gold["f0raw_%d" % k]) == T40
        rows = ops.emobase_rows_of(T25, T40, 1)
        assert gold["lld_%d" % k].shape == (rows, 52), (k, n, fs)
        want = [ops.emobase_row_time_frame(T25, T40, 1, r) * H / float(fs) for r in range(rows)]
        assert np.allclose(gold["times_%d" % k], want, rtol=0, atol=6e-7), (k, gold["times_%d" % k][-3:], want[-3:])   # (the CSV has six decimals)
    assert {(0, 0), (1, 0), (2, 0), (2, 1), (3, 1), (3, 2), (4, 2), (11, 10), (98, 97), (298, 297)} <= seen
    assert (28, 26) in seen                                # 22.05 kHz: two steps without a 40 ms frame
    assert sorted(set(int(fs) for _, _, fs in gold["inputs"])) == [8000, 11025, 16000, 22050, 32000, 44100, 48000]
    n_w = 0
    for sw in (5, 7, 9):
        W = sw // 2
        for k in (3, 4, 5, 6, 7, 8, 9, 10):
            T25, T40 = len(gold["intens_%d" % k]), len(gold["pitch_%d" % k])
            rows = ops.emobase_rows_of(T25, T40, W)
            assert len(gold["lld_w%d_%d" % (sw, k)]) == rows
            fs = 16000
            want = [ops.emobase_row_time_frame(T25, T40, W, r) * 160 / float(fs) for r in range(rows)]
            assert np.allclose(gold["times_w%d_%d" % (sw, k)], want, rtol=0, atol=6e-7), (sw, k, gold["times_w%d_%d" % (sw, k)], want)
            n_w += 1
    assert n_w == 24
    for k in (11, 12):                                     # both branches of F0 in the inputs of a second or more
        f0 = gold["lld_%d" % k][:, 24]
        assert (f0 > 0).any() and (f0 == 0).any()


# ------------------------------------------------------------------------------------------------ step 1: levels -> lld | lld_de
def test_host_rows_equal_the_binary_bit_for_bit(ops, gold):
    from tolerance import assert_bits_equal
    n_rows = 0
    for k, (idx, n, fs) in enumerate(gold["inputs"]):
        out = host_rows(ops, level25(gold, k), gold["pitch_%d" % k])
        assert out.shape == gold["lld_%d" % k].shape, (k, out.shape)
        if len(out):
            assert_bits_equal(out, gold["lld_%d" % k], "lld | lld_de, input %d (%d samples at %d Hz)" % (k, n, fs))
        n_rows += len(out)
    assert n_rows > 500


def test_host_rows_wider_windows(ops, gold):
    """smaWin 5, 7 and 9 on the short inputs, where every edge rule of both components shows"""
    from tolerance import assert_bits_equal
    seen = 0
    for key in gold.files:
        m = re.match(r"lld_w(\d)_(\d+)$", key)
        if not m:
            continue
        sw, k = int(m.group(1)), int(m.group(2))
        out = host_rows(ops, level25(gold, k), gold["pitch_%d" % k], W=sw // 2)
        assert out.shape == gold[key].shape
        if len(out):
            assert_bits_equal(out, gold[key], key)
        seen += 1
    assert seen == 24


def test_host_rows_with_edited_parameters(ops, gold):
    from tolerance import assert_bits_equal
    for tag, ncol in (("mp300", 52), ("p10", 56)):
        for k in (10, 11):
            out = host_rows(ops, level25(gold, k, tag + "_"), gold["pitch_%s_%d" % (tag, k)])
            assert out.shape == gold["lld_%s_%d" % (tag, k)].shape and out.shape[1] == ncol
            assert_bits_equal(out, gold["lld_%s_%d" % (tag, k)], "%s, input %d" % (tag, k))
        assert gold["lld_%s_11" % tag].shape != gold["lld_11"].shape or gold["lld_%s_11" % tag].tobytes() != gold["lld_11"].tobytes()


# ------------------------------------------------------------------------------------------------ step 2: samples -> levels
def test_host_frame_recipes_equal_the_binary_bit_for_bit(ops, gold):
    """cIntensity, cMZcr, cVectorPreemphasis + cLpc + cLsp from the samples (what the frame kernel's lane 0 and lld_emobase_lsp run),
    and the level pitch from the binary's voiceProb and F0raw (cut-off, contour, F0env: lld_emobase_contour)"""
    from tolerance import assert_bits_equal
    n_lsp, n_contour = 0, 0
    for k, (idx, n, fs) in enumerate(gold["inputs"]):
        pcm, fs = gold_pcm(gold, k)
        what = "input %d (%d samples at %d Hz)" % (k, n, fs)
        if len(gold["intens_%d" % k]):
            intens, zcr, lpc, lsp = host_frames25(ops, pcm, fs)
            assert_bits_equal(intens, gold["intens_%d" % k], "level intens, " + what)
            assert_bits_equal(zcr, gold["mzcr_%d" % k], "level mzcr, " + what)
            assert_bits_equal(lpc, gold["lpc_%d" % k], "level lpc, " + what)
            assert_bits_equal(lsp, gold["lsp_%d" % k], "level lsp, " + what)
            n_lsp += len(lsp)
        pitch, raw = gold["pitch_%d" % k], gold["f0raw_%d" % k]
        if len(pitch):
            lv = host_pitch(ops, pitch[:, 0], raw[:, 0])
            assert_bits_equal(lv, pitch, "level pitch, " + what)
            n_contour += int((lv[:, 1] != np.where(pitch[:, 0] < 0.55, 0, raw[:, 0])).sum())
    assert n_lsp > 500 and n_contour > 100                 # the contour did change the candidates: the test is not vacuous
    for k in (10, 11):                                     # the edited copies: p = 10, and maxPitch 300 with voicingCutoff 0.7
        pcm, fs = gold_pcm(gold, k)
        intens, zcr, lpc, lsp = host_frames25(ops, pcm, fs, p=10)
        assert_bits_equal(lpc, gold["lpc_p10_%d" % k], "p = 10, level lpc, input %d" % k)
        assert_bits_equal(lsp, gold["lsp_p10_%d" % k], "p = 10, level lsp, input %d" % k)
        pitch, raw = gold["pitch_mp300_%d" % k], gold["f0raw_mp300_%d" % k]
        assert_bits_equal(host_pitch(ops, pitch[:, 0], raw[:, 0], cutoff=0.7), pitch, "mp300, level pitch, input %d" % k)
    assert (gold["pitch_mp300_11"][:, 0] != gold["pitch_11"][:, 0]).any()


def test_hard_signal_fixture_shape(ops):
    h = np.load(os.path.join(GOLD, "hard_emobase.npz"))
    from helpers import hard_signals
    assert sorted(h.files) == sorted("lld_" + n for n in hard_signals.NAMES)
    N25, N40, H = geometry(16000)
    rows = ops.emobase_rows_of(frames_of(24000, N25, H), frames_of(24000, N40, H), 1)
    for n in hard_signals.NAMES:
        assert h["lld_" + n].shape == (rows, 52) == (148, 52)      # 1.5 s: T40 = 147 frames, T40 + 1 rows
    assert (h["lld_dc"][:, 1] > 0).all() and (h["lld_clicks_in_zeros"][:, 1] == 0).any()    # loudness through pow: DC and digital zero


# ------------------------------------------------------------------------------------------------ names, front end
def test_names_and_csv_header(gold):
    hdr = str(gold["csv_header"])
    assert hdr == "name;frameTime;" + ";".join(names())
    src = open(os.path.join(ROOT, "opensmile_amd", "host", "feature_names.cpp")).read()
    for n in ("pcm_intensity", "pcm_loudness", "lspFreq", "pcm_zcr", "voiceProb", "F0env", "_sma_de"):
        assert '"%s"' % n in src
    for stem in ("u2_8000", "u3_4000"):
        lines = open(os.path.join(GOLD, "files", "emobase_%s.csv" % stem)).read().splitlines()
        assert lines[0] == hdr and lines[1].startswith("'%s';0.000000;" % stem)


needs_exe = pytest.mark.skipif(not os.path.exists(EXE), reason="smilextract_hip not built")
needs_conf = pytest.mark.skipif(not os.path.isdir(CONF), reason="the reference's configuration files are not there (oracle/_ref not built)")

# a minimal configuration text of the same graph, not the shipped file: own wording, no includes, no functionals
MINIMAL = """
[componentInstances:cComponentManager]
instance[dataMemory].type=cDataMemory
instance[wave].type=cWaveSource
instance[fa].type=cFramer
instance[fb].type=cFramer
instance[wb].type=cWindower
instance[tb].type=cTransformFFT
instance[mb].type=cFFTmagphase
instance[ac].type=cAcf
instance[ce].type=cAcf
instance[p].type=cPitchACF
instance[pre].type=cVectorPreemphasis
instance[wa].type=cWindower
instance[ta].type=cTransformFFT
instance[ma].type=cFFTmagphase
instance[mel].type=cMelspec
instance[cc].type=cMfcc
instance[lp].type=cLpc
instance[ls].type=cLsp
instance[zc].type=cMZcr
instance[loud].type=cIntensity
instance[sm].type=cContourSmoother
instance[de].type=cDeltaRegression
instance[out].type=cCsvSink
[wave:cWaveSource]
writer.dmLevel=wave
filename=\\cm[inputfile(I){in.wav}:input]
[fb:cFramer]
reader.dmLevel=wave
writer.dmLevel=long
frameSize=0.04
frameStep=0.01
[wb:cWindower]
reader.dmLevel=long
writer.dmLevel=longw
winFunc=ham
[tb:cTransformFFT]
reader.dmLevel=longw
writer.dmLevel=longc
zeroPadSymmetric=0
[mb:cFFTmagphase]
reader.dmLevel=longc
writer.dmLevel=longm
[ac:cAcf]
reader.dmLevel=longm
writer.dmLevel=lags
usePower=1
acfCepsNormOutput=0
[ce:cAcf]
reader.dmLevel=longm
writer.dmLevel=quef
usePower=1
cepstrum=1
oldCompatCepstrum=1
[p:cPitchACF]
reader.dmLevel=lags;quef
writer.dmLevel=f0
processArrayFields=0
maxPitch=500
voicingCutoff=0.55
voiceProb=1
F0=1
F0env=1
[fa:cFramer]
reader.dmLevel=wave
writer.dmLevel=short
frameSize=0.025
frameStep=0.01
[pre:cVectorPreemphasis]
reader.dmLevel=short
writer.dmLevel=shortpe
k=0.97
[wa:cWindower]
reader.dmLevel=shortpe
writer.dmLevel=shortw
winFunc=ham
[ta:cTransformFFT]
reader.dmLevel=shortw
writer.dmLevel=shortc
zeroPadSymmetric=0
[ma:cFFTmagphase]
reader.dmLevel=shortc
writer.dmLevel=shortm
[mel:cMelspec]
reader.dmLevel=shortm
writer.dmLevel=bands
nBands=26
lofreq=0
hifreq=8000
usePower=1
[cc:cMfcc]
reader.dmLevel=bands
writer.dmLevel=ceps
firstMfcc=1
lastMfcc=12
[lp:cLpc]
reader.dmLevel=shortpe
writer.dmLevel=lpcoef
p=8
[ls:cLsp]
reader.dmLevel=lpcoef
writer.dmLevel=lsf
[loud:cIntensity]
reader.dmLevel=short
writer.dmLevel=loudness
intensity=1
loudness=1
[zc:cMZcr]
reader.dmLevel=short
writer.dmLevel=crossings
zcr=1
amax=0
mcr=0
maxmin=0
[sm:cContourSmoother]
reader.dmLevel=loudness;ceps;lsf;crossings;f0
writer.dmLevel=lld
smaWin=3
[de:cDeltaRegression]
reader.dmLevel=lld
writer.dmLevel=lld_de
deltawin=2
[out:cCsvSink]
reader.dmLevel=lld;lld_de
filename=\\cm[lldcsvoutput{?}:csv]
"""


def describe(path, *more):
    r = subprocess.run([EXE, "--set", "emobase", "-C", path, "--describe", *more], capture_output=True, text=True)
    kv = dict(l.split("=", 1) for l in r.stdout.split("\n") if "=" in l)
    return r.returncode, kv, r.stderr


def write_conf(tmp_path, text, name="e.conf"):
    p = tmp_path / name
    p.write_text(text)
    return str(p)


@needs_exe
def test_minimal_text_maps_to_the_set(tmp_path):
    rc, kv, err = describe(write_conf(tmp_path, MINIMAL))
    assert rc == 0 and kv["preset"] == "emobase", err
    got = {k[6:]: float(v) for k, v in kv.items() if k.startswith("param.")}
    assert got == {"pitch_max": 500, "voicing_cutoff": 0.55, "sma_win": 3, "lpc_order": 8}


@needs_exe
def test_each_parameter_edit_is_taken(tmp_path):
    for old, new, key, val in (("maxPitch=500", "maxPitch=300", "pitch_max", 300), ("voicingCutoff=0.55", "voicingCutoff=0.7", "voicing_cutoff", 0.7),
                               ("smaWin=3", "smaWin=7", "sma_win", 7), ("p=8", "p=10", "lpc_order", 10), ("p=8", "p=16", "lpc_order", 16),
                               ("voicingCutoff=0.55", "voicingCutoff=1.5", "voicing_cutoff", 1.0)):
        assert MINIMAL.count(old) == 1
        rc, kv, err = describe(write_conf(tmp_path, MINIMAL.replace(old, new)))
        assert rc == 0 and kv["preset"] == "emobase", err
        assert float(kv["param." + key]) == val, (key, kv)


REFUSED = [  # (text of the minimal configuration, its replacement, the option the message must name)
    ("winFunc=ham\n[tb", "winFunc=han\n[tb", "winFunc"),
    ("oldCompatCepstrum=1", "oldCompatCepstrum=0", "oldCompatCepstrum"),
    ("acfCepsNormOutput=0", "acfCepsNormOutput=1", "acfCepsNormOutput"),
    ("F0env=1", "F0env=0", "F0env"),
    ("k=0.97", "k=0.95", "cVectorPreemphasis] k ="),
    ("p=8", "p=7", "p = 7"),
    ("p=8", "p=18", "p = 18"),
    ("p=8", "p=8\nmethod=burg", "method"),
    ("p=8", "p=8\nlpGain=1", "lpGain"),
    ("smaWin=3", "smaWin=4", "smaWin"),
    ("deltawin=2", "deltawin=3", "deltawin"),
    ("frameSize=0.04", "frameSize=0.05", "frameSize"),
    ("lastMfcc=12", "lastMfcc=14", "lastMfcc"),
    ("nBands=26", "nBands=40", "nBands"),
    ("intensity=1", "intensity=0", "intensity"),
    ("mcr=0", "mcr=1", "mcr"),
    ("reader.dmLevel=loudness;ceps;lsf;crossings;f0", "reader.dmLevel=ceps;loudness;lsf;crossings;f0", "reader.dmLevel"),
    ("zeroPadSymmetric=0\n[ma", "zeroPadSymmetric=1\n[ma", "zeroPadSymmetric"),
]


@needs_exe
@pytest.mark.parametrize("old,new,option", REFUSED, ids=["%s:%s" % (r[2], r[1].split("\n")[0]) for r in REFUSED])
def test_refused_edit_names_the_option(tmp_path, old, new, option):
    assert MINIMAL.count(old) == 1
    rc, kv, err = describe(write_conf(tmp_path, MINIMAL.replace(old, new)))
    assert rc != 0 and "preset" not in kv
    assert option in err, err


@needs_exe
def test_functionals_outputs_are_refused_and_plain_conf_names_the_route(tmp_path):
    wav = os.path.join(GOLD, "files", "u2_8000.wav")
    for o in ("-O", "-csvoutput", "-htkoutput"):
        r = subprocess.run([EXE, "--set", "emobase", "-I", wav, o, str(tmp_path / "f.out")], capture_output=True, text=True)
        assert r.returncode != 0 and "functionals level" in r.stderr and "not built" in r.stderr and not (tmp_path / "f.out").exists()
    r = subprocess.run([EXE, "--set", "emobase"], capture_output=True, text=True)        # the set name is known: what is missing is the input
    assert r.returncode != 0 and "no input" in r.stderr and "--set must be" not in r.stderr
    r = subprocess.run([EXE, "-C", write_conf(tmp_path, MINIMAL), "--describe"], capture_output=True, text=True)      # plain -C: refused, with the way to run it
    assert r.returncode != 0 and "cannot run on the fused path" in r.stderr and "--set emobase -C" in r.stderr
    r = subprocess.run([EXE, "--set", "prosody_acf", "-C", write_conf(tmp_path, MINIMAL), "--describe"], capture_output=True, text=True)
    assert r.returncode != 0 and "prosodyAcf.conf" in r.stderr


@needs_exe
@needs_conf
def test_shipped_file_is_recognised(tmp_path):
    path = os.path.join(CONF, "emobase", "emobase.conf")
    rc, kv, err = describe(path)
    assert rc == 0 and kv["preset"] == "emobase" and "every processing component and option identical" in err
    assert not [k for k in kv if k.startswith("param.")]
    r = subprocess.run([EXE, "-C", path, "--describe"], capture_output=True, text=True)
    assert r.returncode != 0 and "cannot run on the fused path" in r.stderr and "--set emobase -C" in r.stderr
    # the file's own functionals outputs stay refused with -C as well
    r = subprocess.run([EXE, "--set", "emobase", "-C", path, "-I", os.path.join(GOLD, "files", "u2_8000.wav"), "-O", str(tmp_path / "f.arff")],
                       capture_output=True, text=True)
    assert r.returncode != 0 and "functionals level" in r.stderr
    # edited copies of the shipped file: each parameter is taken
    text = open(path, encoding="latin-1").read().replace("\\{../shared/", "\\{" + os.path.join(CONF, "shared") + "/")
    for old, new, key, val in (("maxPitch = 500", "maxPitch = 300", "pitch_max", 300), ("\np = 8\n", "\np = 10\n", "lpc_order", 10),
                               ("smaWin = 3", "smaWin = 5", "sma_win", 5)):
        assert text.count(old) == 1
        p = tmp_path / "edited.conf"
        p.write_text(text.replace(old, new), encoding="latin-1")
        rc, kv, err = describe(str(p))
        assert rc == 0 and kv["preset"] == "emobase" and float(kv["param." + key]) == val, err
