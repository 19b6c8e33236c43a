"""config/prosody/prosodyAcf.conf as a fused batch set (SMILEHIP_CHAIN_PROSODY_ACF) on the device: lld_acf_pitch_frame in both of
its forms (a wave per frame at 8 / 11.025 / 16 kHz, a workgroup per frame above), the contour scan and the window chain's SMA
stage, held bit for bit to the real binary's lld, pitch and intens levels (tests/golden/make_golden_prosody_acf.py), to the chain
of the library's own per-component operators, across workgroup seams, on the hard-signal corpus and through the smilextract_hip
front end. Tolerance everywhere: identical bits."""
import os
import subprocess

import numpy as np
import pytest

from test_prosody_acf_host import GOLD, geometry, gold_pcm

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "opensmile_amd", "smilextract_hip")
CONF = os.path.join(ROOT, "oracle", "_ref", "config")
WAVE_FRAMES = 4                                            # frames per workgroup of the wave form (lld_prosody_acf.hip: kAcfWaves)


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLD, "prosody_acf_synth.npz"))


@pytest.fixture(scope="module")
def hip():
    from opensmile_amd import capi
    ctx = capi.Context(0)
    plan = capi.Plan(ctx, capi.prosody_acf_config())
    g = plan.geometry
    assert (g.frame_size, g.frame_step, g.fft_size, g.n_bins, g.n_out) == (800, 160, 1024, 513, 3)
    return capi, ctx, plan


def offsets(pcms):
    return np.concatenate([[0], np.cumsum([len(p) for p in pcms])]).astype(np.int64)


def as_f32(pcm):
    return (np.asarray(pcm).astype(np.float32) / np.float32(32767.0)).astype(np.float32)


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def check_against_gold(gold, ks, b, out, tap, suffix="%d", what=""):
    """rows, every cell and the tap (levels pitch and intens) of the batch's utterances against the binary's"""
    from tolerance import assert_bits_equal
    f0 = 0
    for i, k in enumerate(ks):
        ref, pitch, intens = (gold[n + "_" + suffix % k] for n in ("lld", "pitch", "intens"))
        T = len(pitch)
        assert b.frame_offsets[i + 1] - b.frame_offsets[i] == len(ref), (k, T)
        if T:
            assert_bits_equal(tap[f0:f0 + T, :2], pitch, "%slevel pitch, input %d" % (what, k))
            assert_bits_equal(tap[f0:f0 + T, 2:], intens, "%slevel intens, input %d" % (what, k))
            assert_bits_equal(out[b.frame_offsets[i]:b.frame_offsets[i + 1]], ref, "%slld, input %d" % (what, k))
        f0 += T
    assert f0 == b.total_frames == len(tap)


# ---------------------------------------------------------------------------------------------- 1. golden, ragged batch
def test_golden_ragged_batch(hip, gold):
    capi, ctx, plan = hip
    # the 0-frame and 1-frame utterances between long ones, inside one workgroup's frames: 96 = 24 x 4 frames of the 1 s input,
    # then 799 samples (no frame), 800 (one), 0, 960 (two), the 3 s input, 100 (none), 1120, 1280, 2080
    ks = [8, 2, 3, 0, 4, 9, 1, 5, 6, 7]
    assert all(int(gold["inputs"][k][2]) == 16000 for k in ks) and sorted(ks) == list(range(10))
    assert sum(1 for _, _, fs in gold["inputs"] if fs == 16000) == 10
    pcms = [gold_pcm(gold, k)[0] for k in ks]
    b = capi.Batch(plan, offsets(pcms))
    out, tap = b.prosody_acf_run_host(np.concatenate(pcms))
    check_against_gold(gold, ks, b, out, tap)
    b.close()


def test_golden_other_rates(gold):
    """int16 at the six other rates: the wave form with M = 256 (8 kHz) and M = 512 (11.025 kHz), the workgroup form at 2048 and
    4096 points; two of them with 50 ms no whole number of samples"""
    from opensmile_amd import capi
    ctx = capi.Context(0)
    seen = {}
    for k, (idx, n, fs) in enumerate(gold["inputs"]):
        if fs == 16000:
            continue
        cfg = capi.prosody_acf_config()
        cfg.sample_rate = float(fs)
        plan = capi.Plan(ctx, cfg)
        assert (plan.geometry.frame_size, plan.geometry.frame_step) == geometry(int(fs))
        pcm, _ = gold_pcm(gold, k)
        b = capi.Batch(plan, np.array([0, len(pcm)], np.int64))
        out, tap = b.prosody_acf_run_host(pcm)
        check_against_gold(gold, [k], b, out, tap, what="%d Hz: " % fs)
        b.close()
        seen[int(fs)] = plan.geometry.fft_size
        plan.close()
    assert seen == {8000: 512, 11025: 1024, 22050: 2048, 32000: 2048, 44100: 4096, 48000: 4096}


def test_float_input_equals_int16(hip, gold):
    capi, ctx, plan = hip
    pcm, _ = gold_pcm(gold, 8)                             # the 1 s input
    b = capi.Batch(plan, np.array([0, len(pcm)], np.int64))
    out, tap = b.prosody_acf_run_host(pcm)
    out32, tap32 = b.prosody_acf_run_host(as_f32(pcm))
    assert bits_equal(out32, out) and bits_equal(tap32, tap) and bits_equal(out, gold["lld_8"])
    b.close()
    # ... and through the workgroup form
    cfg = capi.prosody_acf_config()
    cfg.sample_rate = 44100.0
    p44 = capi.Plan(ctx, cfg)
    k = [i for i, (_, _, fs) in enumerate(gold["inputs"]) if fs == 44100][0]
    pcm, _ = gold_pcm(gold, k)
    b = capi.Batch(p44, np.array([0, len(pcm)], np.int64))
    out32, _ = b.prosody_acf_run_host(as_f32(pcm))
    assert bits_equal(out32, gold["lld_%d" % k])
    b.close()
    p44.close()


# ---------------------------------------------------------------------------------------------- 2. fused = per-component
def per_component(capi, ctx, plan, pcm, cutoff=0.55, max_pitch=500.0, W=1):
    """the chain out of the existing operators, one launch each over all frames of one utterance: (lld rows, level before the smoother)"""
    import torch
    import ctypes as C
    L = capi.load()
    g = plan.geometry
    N, H, K, Nfft = g.frame_size, g.frame_step, g.n_bins, g.fft_size
    M = Nfft // 2
    T = (len(pcm) - N) // H + 1
    x = as_f32(pcm)
    d_fr = torch.from_numpy(np.stack([x[t * H:t * H + N] for t in range(T)])).cuda()
    d_w, d_c, d_m = torch.zeros((T, N), device="cuda"), torch.zeros((T, Nfft), device="cuda"), torch.zeros((T, K), device="cuda")
    capi.window_frames(plan, d_fr.data_ptr(), N, d_w.data_ptr(), N, T)
    capi.rfft_frames(plan, d_w.data_ptr(), N, d_c.data_ptr(), Nfft, T)
    capi.fftmag_frames(plan, d_c.data_ptr(), Nfft, d_m.data_ptr(), K, T)
    d_ac = torch.zeros((T, 2 * M), device="cuda")          # [acf(M) | cepstrum(M)] per frame
    capi._check(L.smilehip_acf_frames(plan._h, d_m.data_ptr(), K, d_ac.data_ptr(), 2 * M, M, T, 1, 0, 1, 0, None))
    capi._check(L.smilehip_acf_frames(plan._h, d_m.data_ptr(), K, d_ac.data_ptr() + 4 * M, 2 * M, M, T, 0, 1, 1, 0, None))
    d_v = torch.zeros(T, dtype=torch.float64, device="cuda")
    d_i = torch.zeros(T, dtype=torch.int32, device="cuda")
    fs_sec = float(np.float32(g.fft_frame_size_sec))       # cPitchACF keeps the level's frameSizeSec as a float
    capi._check(L.smilehip_pitchacf_frames(ctx._h, d_ac.data_ptr(), 2 * M, M, T, fs_sec, max_pitch, d_v.data_ptr(), d_i.data_ptr(), None))
    d_state = torch.zeros(8, device="cuda")
    d_o4 = torch.zeros((T, 4), device="cuda")
    capi._check(L.smilehip_pitchacf_contour_frames(ctx._h, d_v.data_ptr(), d_i.data_ptr(), fs_sec / Nfft, cutoff, d_state.data_ptr(),
                                                   d_o4.data_ptr(), T, None))
    d_l = torch.zeros((T, 1), device="cuda")
    capi._check(L.smilehip_intensity_frames(ctx._h, d_fr.data_ptr(), N, N, 2, d_l.data_ptr(), 1, T, None))
    torch.cuda.synchronize()
    level = np.stack([d_v.cpu().numpy().astype(np.float32), d_o4.cpu().numpy()[:, 0], d_l.cpu().numpy()[:, 0]], axis=1)
    # cContourSmoother: the row operator on each column, the block as getMatrix hands it over (T > 2 W: first and last frame replicated)
    assert T > 2 * W
    rows = T + W
    cols = []
    for c in range(3):
        padded = np.concatenate([np.repeat(level[:1, c], W), level[:, c], np.repeat(level[-1:, c], 2 * W)]).astype(np.float32)
        d_x = torch.from_numpy(padded).cuda()
        d_y = torch.zeros(rows, device="cuda")
        capi._check(L.smilehip_window_op_row(ctx._h, d_x.data_ptr() + 4 * W, d_y.data_ptr(), rows, 1, W, None))
        torch.cuda.synchronize()
        cols.append(d_y.cpu().numpy())
    return np.stack(cols, axis=1), level


@pytest.mark.parametrize("fs", [16000, 44100])
def test_fused_equals_per_component_operators(fs):
    """a seeded 2 s signal on which no fixture exists, once per kernel form"""
    from tolerance import assert_bits_equal
    from opensmile_amd import capi, synth
    ctx = capi.Context(0)
    cfg = capi.prosody_acf_config()
    cfg.sample_rate = float(fs)
    plan = capi.Plan(ctx, cfg)
    pcm = synth.utterance(31, 2 * fs)
    b = capi.Batch(plan, np.array([0, len(pcm)], np.int64))
    fused, tap = b.prosody_acf_run_host(pcm)
    b.close()
    ref, level = per_component(capi, ctx, plan, pcm)
    assert (level[:, 1] > 0).any() and (level[:, 1] == 0).any()
    assert_bits_equal(tap, level, "levels in front of the smoother at %d Hz" % fs)
    assert_bits_equal(fused, ref, "lld at %d Hz" % fs)
    plan.close()


# ---------------------------------------------------------------------------------------------- 3. workgroup seams
def test_workgroup_seams(hip):
    """batches whose total frame count is 1, then one short of, equal to and one past a multiple of the wave form's frames per
    workgroup: each utterance's rows equal its rows when run alone"""
    from opensmile_amd import synth
    capi, ctx, plan = hip
    frames = {1: 800, 2: 960, 3: 1120, 4: 1280, 5: 1440}
    alone = {}
    for T, n in frames.items():
        pcm = synth.utterance(50 + T, n)
        b = capi.Batch(plan, np.array([0, n], np.int64))
        assert b.total_frames == T
        alone[T] = (pcm,) + b.prosody_acf_run_host(pcm)
        b.close()
    for Ts in ([1], [3, 4], [3, 5], [3, 5, 1], [4, 4, 3], [5, 5, 2, 4], [2, 5, 5, 5]):
        total = sum(Ts)
        pcms = [alone[T][0] for T in Ts]
        b = capi.Batch(plan, offsets(pcms))
        assert b.total_frames == total
        out, tap = b.prosody_acf_run_host(np.concatenate(pcms))
        f0 = 0
        for i, T in enumerate(Ts):
            assert bits_equal(out[b.frame_offsets[i]:b.frame_offsets[i + 1]], alone[T][1]), (Ts, i)
            assert bits_equal(tap[f0:f0 + T], alone[T][2]), (Ts, i)
            f0 += T
        b.close()
    assert {sum(t) % WAVE_FRAMES for t in ([3, 4], [3, 5], [3, 5, 1])} == {WAVE_FRAMES - 1, 0, 1}


# ---------------------------------------------------------------------------------------------- 4. re-run, empty batch, ld_out
def test_rerun_empty_and_ld_out(hip):
    import torch
    from opensmile_amd import synth
    capi, ctx, plan = hip
    L = capi.load()
    pcm = np.concatenate([synth.utterance(3, 32000), synth.utterance(4, 1000), synth.utterance(5, 16000)])
    b = capi.Batch(plan, np.array([0, 32000, 33000, 49000], np.int64))
    a, tap_a = b.prosody_acf_run_host(pcm)
    c, tap_c = b.prosody_acf_run_host(pcm, runs=2)         # the contour runs in place on the scratch: a second run starts from fresh candidates
    assert a.shape == (197 + 3 + 97, 3) and bits_equal(a, c) and bits_equal(tap_a, tap_c)
    wide, _ = b.prosody_acf_run_host(pcm, ld_out=7, fill=-7.5)
    assert bits_equal(wide[:, :3], a) and (wide[:, 3:] == np.float32(-7.5)).all()       # the pads keep what they held
    d_pcm = torch.from_numpy(pcm).cuda()
    d_out = torch.zeros((b.total_rows, 3), device="cuda")
    rc = L.smilehip_lld_run(plan._h, b._h, d_pcm.data_ptr(), d_out.data_ptr(), 2, None)
    assert rc == -1 and b"ld_out" in L.smilehip_last_error()            # SMILEHIP_ERR_INVALID, by name
    torch.cuda.synchronize()
    assert float(d_out.abs().max()) == 0.0
    b.close()
    e = capi.Batch(plan, np.array([0, 0, 100, 899], np.int64))          # nothing, 100 samples, 799 samples: no frame anywhere
    assert e.total_frames == 0 and e.total_rows == 0 and list(e.frame_offsets) == [0, 0, 0, 0]
    out, tap = e.prosody_acf_run_host(np.zeros(899, np.int16))
    assert out.shape == (0, 3) and tap.shape == (0, 3)
    e.close()
    f0b = capi.Batch(capi.Plan(ctx, capi.prosody_shs_config()), np.array([0, 16000], np.int64))
    assert L.smilehip_batch_prosody_acf_taps(f0b._h, None, None) == -1 and b"not a prosodyAcf chain batch" in L.smilehip_last_error()
    f0b.close()


# ---------------------------------------------------------------------------------------------- 5. hard signals
def test_hard_signals(hip):
    from tolerance import assert_bits_equal
    from helpers import hard_signals
    capi, ctx, plan = hip
    ref = np.load(os.path.join(GOLD, "hard_prosody_acf.npz"))
    pcm = np.load(os.path.join(GOLD, "hard_pcm.npz"))
    sig = [np.ascontiguousarray(pcm[n], np.int16) for n in hard_signals.NAMES]
    b = capi.Batch(plan, offsets(sig))
    out, _ = b.prosody_acf_run_host(np.concatenate(sig))
    for i, n in enumerate(hard_signals.NAMES):
        assert_bits_equal(out[b.frame_offsets[i]:b.frame_offsets[i + 1]], ref["lld_" + n], n)
    b.close()


# ---------------------------------------------------------------------------------------------- 6. parameters of the chain
@pytest.mark.parametrize("sma_win", [5, 7, 9])
def test_wider_smoothing_windows_equal_the_binary(hip, gold, sma_win):
    """sma_win is a field of the config struct: the short inputs, where the smoother's edge rules show, against what the binary
    wrote for a copy of the file with smaWin edited"""
    capi, ctx, _ = hip
    cfg = capi.prosody_acf_config()
    cfg.sma_win = sma_win
    plan = capi.Plan(ctx, cfg)
    ks = [4, 5, 6, 7, 8]
    pcms = [gold_pcm(gold, k)[0] for k in ks]
    b = capi.Batch(plan, offsets(pcms))
    out, tap = b.prosody_acf_run_host(np.concatenate(pcms))
    for i, k in enumerate(ks):
        assert bits_equal(out[b.frame_offsets[i]:b.frame_offsets[i + 1]], gold["lld_w%d_%d" % (sma_win, k)]), (sma_win, k)
    b.close()
    plan.close()


EDITED = {"mp300": dict(pitch_max=300.0, voicing_cutoff=0.7), "vc15": dict(voicing_cutoff=1.5)}


@pytest.mark.parametrize("tag", sorted(EDITED))
def test_edited_parameters_equal_the_binary(hip, gold, tag):
    """maxPitch and voicingCutoff as fields of the config struct (1.5 is clamped to 1 as cPitchACF does), against what the binary
    wrote for a copy of the file with the same options edited: both levels and the three columns, bit for bit"""
    capi, ctx, _ = hip
    cfg = capi.prosody_acf_config()
    for f, v in EDITED[tag].items():
        setattr(cfg, f, v)
    plan = capi.Plan(ctx, cfg)
    ks = [7, 8]
    pcms = [gold_pcm(gold, k)[0] for k in ks]
    b = capi.Batch(plan, offsets(pcms))
    out, tap = b.prosody_acf_run_host(np.concatenate(pcms))
    check_against_gold(gold, ks, b, out, tap, suffix=tag + "_%d", what=tag + ": ")
    b.close()
    plan.close()


# ---------------------------------------------------------------------------------------------- 7. front end
def run_exe(*args):
    p = subprocess.run([EXE, *args], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]


def same_file(path, name):
    return open(path, "rb").read() == open(os.path.join(GOLD, "files", name), "rb").read()


@pytest.mark.parametrize("stem", ["u2_8000", "u3_4000"])
def test_front_end_set_writes_the_binary_s_files(tmp_path, stem):
    wav = os.path.join(GOLD, "files", stem + ".wav")
    htk, csv = str(tmp_path / "o.htk"), str(tmp_path / "o.csv")
    run_exe("--set", "prosody_acf", "-I", wav, "-O", htk, "-csvoutput", csv, "-instname", stem)
    assert same_file(htk, "prosody_acf_%s.htk" % stem) and same_file(csv, "prosody_acf_%s.csv" % stem)


def test_front_end_filelist(tmp_path):
    lst = tmp_path / "list.txt"
    lst.write_text("".join(os.path.join(GOLD, "files", s + ".wav") + "\n" for s in ("u2_8000", "u3_4000")))
    out = tmp_path / "out"
    out.mkdir()
    run_exe("--set", "prosody_acf", "-filelist", str(lst), "-outdir", str(out), "-O", "x", "-csvoutput", "x")
    for s in ("u2_8000", "u3_4000"):
        assert same_file(out / (s + ".htk"), "prosody_acf_%s.htk" % s) and same_file(out / (s + ".csv"), "prosody_acf_%s.csv" % s)


def test_front_end_serve(tmp_path):
    """--serve: two lists on one process (context and plan kept); every file equals the binary's"""
    lines = ""
    for tag in ("a", "b"):
        (tmp_path / tag).mkdir()
        lst = tmp_path / (tag + ".txt")
        lst.write_text("".join(os.path.join(GOLD, "files", s + ".wav") + "\n" for s in ("u2_8000", "u3_4000")))
        lines += "-filelist %s -outdir %s\n" % (lst, tmp_path / tag)
    r = subprocess.run([EXE, "--set", "prosody_acf", "-O", "1", "-csvoutput", "1", "--serve"], input=lines + "quit\n", capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-1500:]
    done = [l.split() for l in r.stdout.splitlines() if l.startswith("done ")]
    assert len(done) == 2 and all(d[1] == "0" for d in done), r.stdout
    for tag in ("a", "b"):
        for s in ("u2_8000", "u3_4000"):
            for ext in ("htk", "csv"):
                assert same_file(tmp_path / tag / (s + "." + ext), "prosody_acf_%s.%s" % (s, ext))


needs_conf = pytest.mark.skipif(not os.path.isdir(CONF), reason="the reference's configuration files are not there (oracle/_ref not built)")


@needs_conf
def test_front_end_conf_file(tmp_path):
    conf = os.path.join(CONF, "prosody", "prosodyAcf.conf")
    for stem in ("u2_8000", "u3_4000"):
        htk, csv = str(tmp_path / (stem + ".htk")), str(tmp_path / (stem + ".csv"))
        run_exe("--set", "prosody_acf", "-C", conf, "-I", os.path.join(GOLD, "files", stem + ".wav"), "-O", htk, "-csvoutput", csv, "-instname", stem)
        assert same_file(htk, "prosody_acf_%s.htk" % stem) and same_file(csv, "prosody_acf_%s.csv" % stem)


@needs_conf
@pytest.mark.parametrize("tag,edits", [("mp300", {"maxPitch = 500": "maxPitch = 300", "voicingCutoff = 0.550000": "voicingCutoff = 0.700000"}),
                                       ("vc15", {"voicingCutoff = 0.550000": "voicingCutoff = 1.500000"}),
                                       ("w5", {"smaWin = 3": "smaWin = 5"})])
def test_front_end_edited_conf_equals_the_binary(gold, tmp_path, tag, edits):
    """--set prosody_acf -C edited.conf on the 1 s input: the rows the binary wrote for the same edited copy"""
    from oracle import lldo
    text = open(os.path.join(CONF, "prosody", "prosodyAcf.conf")).read().replace("\\{../shared/", "\\{" + os.path.join(CONF, "shared") + "/")
    for a, b in edits.items():
        assert text.count(a) == 1
        text = text.replace(a, b)
    conf = tmp_path / "edited.conf"
    conf.write_text(text)
    pcm, fs = gold_pcm(gold, 8)
    wav, htk = str(tmp_path / "in.wav"), str(tmp_path / "e.htk")
    lldo.write_wav(wav, pcm, fs)
    run_exe("--set", "prosody_acf", "-C", str(conf), "-I", wav, "-O", htk)
    ref = gold["lld_w5_8"] if tag == "w5" else gold["lld_%s_8" % tag]
    assert bits_equal(lldo.read_htk(htk)[0].reshape(-1, 3), ref)
    assert not bits_equal(ref, gold["lld_8"])
