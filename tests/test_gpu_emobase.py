"""config/emobase/emobase.conf, levels lld and lld_de, as a fused batch set (SMILEHIP_CHAIN_EMOBASE) on the device: lld_emobase_frame in
both of its forms (a wave per step at 8 / 11.025 / 16 kHz, a workgroup per step above and where SMILEHIP_EMOBASE=block asks for it),
the cLpc / cLsp row kernel, the contour scan and the row kernel of the smoother and the regression, held bit for bit to the real
binary's 52 columns and to its levels intens, mfcc1, lsp, mzcr and pitch (tests/golden/make_golden_emobase.py), across workgroup
seams, on the hard-signal corpus and through the smilextract_hip front end. Tolerance everywhere: identical bits."""
import os
import subprocess

import numpy as np
import pytest

from test_emobase_host import CONF, GOLD, LEVELS25, as_f32, frames_of, geometry, gold_pcm, level25

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "opensmile_amd", "smilextract_hip")
WAVE_STEPS = 6                                             # steps per workgroup of the wave form (lld_emobase.hip: kEmoWaves)


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLD, "emobase_synth.npz"))


@pytest.fixture(scope="module")
def hip():
    from opensmile_amd import capi
    ctx = capi.Context(0)
    plan = capi.Plan(ctx, capi.emobase_config())
    g = plan.geometry
    assert (g.frame_size, g.frame_step, g.fft_size, g.n_bins, g.n_out) == (400, 160, 512, 257, 52) and plan.emobase_frame40() == (640, 1024)
    return capi, ctx, plan


def offsets(pcms):
    return np.concatenate([[0], np.cumsum([len(p) for p in pcms])]).astype(np.int64)


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def check_against_gold(gold, ks, b, out, tap25, tap3, sfx="", what=""):
    """rows, every cell and the taps (the five levels in front of the smoother) of the batch's utterances against the binary's"""
    from tolerance import assert_bits_equal
    f0 = 0
    for i, k in enumerate(ks):
        ref, pitch, a25 = gold["lld_%s%d" % (sfx, k)], gold["pitch_%s%d" % (sfx, k)], level25(gold, k, sfx)
        T25, T40 = len(a25), len(pitch)
        assert b.frame_offsets[i + 1] - b.frame_offsets[i] == len(ref), (k, T25, T40)
        if T25:
            assert_bits_equal(tap25[f0:f0 + T25], a25, "%slevels intens | mfcc1 | lsp | mzcr, input %d" % (what, k))
        if T40:
            assert_bits_equal(tap3[f0:f0 + T40], pitch, "%slevel pitch, input %d" % (what, k))
            assert_bits_equal(out[b.frame_offsets[i]:b.frame_offsets[i + 1]], ref, "%slld | lld_de, input %d" % (what, k))
        f0 += T25
    assert f0 == b.total_frames == len(tap25) == len(tap3)


# ---------------------------------------------------------------------------------------------- 1. golden, ragged batch
def test_golden_ragged_batch(hip, gold):
    capi, ctx, plan = hip
    # 98 = 16 x 6 + 2 steps of the 1 s input, then, inside one workgroup's run of steps: 399 samples (no frame), 400 (one 25 ms frame, no
    # 40 ms frame), 0, 640 (two steps, one 40 ms frame), the 3 s input, 100 (none), 560, 639 (T40 = 0), 720, 800, 880, 2080
    ks = [11, 2, 3, 0, 6, 12, 1, 4, 5, 7, 8, 9, 10]
    assert all(int(gold["inputs"][k][2]) == 16000 for k in ks) and sorted(ks) == list(range(13))
    assert sum(1 for _, _, fs in gold["inputs"] if fs == 16000) == 13
    pcms = [gold_pcm(gold, k)[0] for k in ks]
    b = capi.Batch(plan, offsets(pcms))
    out, tap25, tap3 = b.emobase_run_host(np.concatenate(pcms))
    check_against_gold(gold, ks, b, out, tap25, tap3)
    b.close()


def test_golden_other_rates(gold):
    """int16 at the six other rates: the wave form at 8 kHz (256 / 512 points: the 25 ms transform in LDS, the 40 ms one in registers) and
    11.025 kHz (512 / 512), the workgroup form at 1024 and 2048 points; three of them with frames of no whole number of milliseconds"""
    from opensmile_amd import capi
    ctx = capi.Context(0)
    seen = {}
    for k, (idx, n, fs) in enumerate(gold["inputs"]):
        if fs == 16000:
            continue
        plan = capi.Plan(ctx, capi.emobase_config(float(fs)))
        N25, N40, H = geometry(int(fs))
        assert (plan.geometry.frame_size, plan.geometry.frame_step, plan.emobase_frame40()[0]) == (N25, H, N40)
        pcm, _ = gold_pcm(gold, k)
        b = capi.Batch(plan, np.array([0, len(pcm)], np.int64))
        out, tap25, tap3 = b.emobase_run_host(pcm)
        check_against_gold(gold, [k], b, out, tap25, tap3, what="%d Hz: " % fs)
        b.close()
        seen[int(fs)] = (plan.geometry.fft_size, plan.emobase_frame40()[1])
        plan.close()
    assert seen == {8000: (256, 512), 11025: (512, 512), 22050: (1024, 1024), 32000: (1024, 2048), 44100: (2048, 2048), 48000: (2048, 2048)}


def test_float_input_equals_int16(hip, gold):
    capi, ctx, plan = hip
    pcm, _ = gold_pcm(gold, 11)                            # the 1 s input
    b = capi.Batch(plan, np.array([0, len(pcm)], np.int64))
    a = b.emobase_run_host(pcm)
    f = b.emobase_run_host(as_f32(pcm))
    assert all(bits_equal(x, y) for x, y in zip(a, f)) and bits_equal(a[0], gold["lld_11"])
    b.close()
    # ... and through the workgroup form
    p44 = capi.Plan(ctx, capi.emobase_config(44100.0))
    k = [i for i, (_, _, fs) in enumerate(gold["inputs"]) if fs == 44100][0]
    pcm, _ = gold_pcm(gold, k)
    b = capi.Batch(p44, np.array([0, len(pcm)], np.int64))
    out32, _, _ = b.emobase_run_host(as_f32(pcm))
    assert bits_equal(out32, gold["lld_%d" % k])
    b.close()
    p44.close()


# ---------------------------------------------------------------------------------------------- 2. forced workgroup form
def test_forced_workgroup_form_equals_wave_form(hip, gold):
    """SMILEHIP_EMOBASE=block (read at every launch): the workgroup form at 16 kHz gives the wave form's bits, and the binary's"""
    capi, ctx, plan = hip
    ks = [11, 3, 6, 10]
    pcms = [gold_pcm(gold, k)[0] for k in ks]
    b = capi.Batch(plan, offsets(pcms))
    wave = b.emobase_run_host(np.concatenate(pcms))
    assert "SMILEHIP_EMOBASE" not in os.environ
    os.environ["SMILEHIP_EMOBASE"] = "block"
    try:
        block = b.emobase_run_host(np.concatenate(pcms))
    finally:
        del os.environ["SMILEHIP_EMOBASE"]
    assert all(bits_equal(x, y) for x, y in zip(wave, block))
    check_against_gold(gold, ks, b, *block, what="workgroup form: ")
    b.close()


# ---------------------------------------------------------------------------------------------- 3. workgroup seams
def test_workgroup_seams(hip):
    """batches whose total step count is 1, then one short of, equal to and one past a multiple of the wave form's steps per workgroup:
    each utterance's rows and levels equal those of the utterance run alone"""
    from opensmile_amd import synth
    capi, ctx, plan = hip
    samples = {1: 400, 2: 640, 3: 800, 4: 960, 5: 1120, 7: 1440}          # 25 ms frames: samples ((T40 = T25 - 1; none for 400)
    alone = {}
    for T, n in samples.items():
        pcm = synth.utterance(50 + T, n)
        b = capi.Batch(plan, np.array([0, n], np.int64))
        assert b.total_frames == T and b.total_rows == (T if T > 1 else 0)
        alone[T] = (pcm,) + b.emobase_run_host(pcm)
        b.close()
    sets = ([1], [2, 3], [2, 4], [3, 4], [5, 7], [7, 5, 1], [4, 7, 1, 5], [5, 5, 2, 7])
    for Ts in sets:
        pcms = [alone[T][0] for T in Ts]
        b = capi.Batch(plan, offsets(pcms))
        assert b.total_frames == sum(Ts)
        out, tap25, tap3 = b.emobase_run_host(np.concatenate(pcms))
        f0 = 0
        for i, T in enumerate(Ts):
            assert bits_equal(out[b.frame_offsets[i]:b.frame_offsets[i + 1]], alone[T][1]), (Ts, i)
            assert bits_equal(tap25[f0:f0 + T], alone[T][2]) and bits_equal(tap3[f0:f0 + T - 1], alone[T][3][:T - 1]), (Ts, i)
            f0 += T
        b.close()
    assert {sum(t) % WAVE_STEPS for t in ([2, 3], [2, 4], [3, 4])} == {WAVE_STEPS - 1, 0, 1}
    assert {sum(t) % WAVE_STEPS for t in ([4, 7, 1, 5], [5, 7], [7, 5, 1])} == {WAVE_STEPS - 1, 0, 1}


# ---------------------------------------------------------------------------------------------- 4. re-run, empty batch, ld_out
def test_rerun_empty_and_ld_out(hip):
    import torch
    from opensmile_amd import synth
    capi, ctx, plan = hip
    L = capi.load()
    pcm = np.concatenate([synth.utterance(3, 32000), synth.utterance(4, 500), synth.utterance(5, 16000)])
    b = capi.Batch(plan, np.array([0, 32000, 32500, 48500], np.int64))
    a = b.emobase_run_host(pcm)
    c = b.emobase_run_host(pcm, runs=2)                    # the contour runs in place on the scratch: a second run starts from fresh candidates
    assert a[0].shape == (198 + 0 + 98, 52) and all(bits_equal(x, y) for x, y in zip(a, c))
    wide = b.emobase_run_host(pcm, ld_out=57, fill=-7.5)[0]
    assert bits_equal(wide[:, :52], a[0]) and (wide[:, 52:] == np.float32(-7.5)).all()     # the pads keep what they held
    d_pcm = torch.from_numpy(pcm).cuda()
    d_out = torch.zeros((b.total_rows, 52), device="cuda")
    rc = L.smilehip_lld_run(plan._h, b._h, d_pcm.data_ptr(), d_out.data_ptr(), 51, None)
    assert rc == -1 and b"ld_out" in L.smilehip_last_error()            # SMILEHIP_ERR_INVALID, by name
    torch.cuda.synchronize()
    assert float(d_out.abs().max()) == 0.0
    b.close()
    e = capi.Batch(plan, np.array([0, 0, 100, 499], np.int64))          # nothing, 100 samples, 399 samples: no frame anywhere
    assert e.total_frames == 0 and e.total_rows == 0 and list(e.frame_offsets) == [0, 0, 0, 0]
    out, tap25, tap3 = e.emobase_run_host(np.zeros(499, np.int16))
    assert out.shape == (0, 52) and tap25.shape == (0, 23) and tap3.shape == (0, 3)
    e.close()
    e = capi.Batch(plan, np.array([0, 400, 1039], np.int64))            # 25 ms frames (one, two) and no 40 ms frame: levels, no row
    assert e.total_frames == 3 and e.total_rows == 0
    out, tap25, tap3 = e.emobase_run_host(synth.utterance(7, 1039))
    assert out.shape == (0, 52) and tap25.shape == (3, 23) and (tap25[:, 1] > 0).all() and not tap3.any()
    e.close()
    other = capi.Batch(capi.Plan(ctx, capi.prosody_acf_config()), np.array([0, 16000], np.int64))
    assert L.smilehip_batch_emobase_taps(other._h, None, None, None, None) == -1 and b"not an emobase chain batch" in L.smilehip_last_error()
    other.close()


# ---------------------------------------------------------------------------------------------- 5. hard signals
def test_hard_signals(hip):
    from tolerance import assert_bits_equal
    from helpers import hard_signals
    capi, ctx, plan = hip
    ref = np.load(os.path.join(GOLD, "hard_emobase.npz"))
    pcm = np.load(os.path.join(GOLD, "hard_pcm.npz"))
    sig = [np.ascontiguousarray(pcm[n], np.int16) for n in hard_signals.NAMES]
    b = capi.Batch(plan, offsets(sig))
    out = b.emobase_run_host(np.concatenate(sig))[0]
    for i, n in enumerate(hard_signals.NAMES):
        assert_bits_equal(out[b.frame_offsets[i]:b.frame_offsets[i + 1]], ref["lld_" + n], n)
    b.close()


# ---------------------------------------------------------------------------------------------- 6. parameters of the chain
@pytest.mark.parametrize("sma_win", [5, 7, 9])
def test_wider_smoothing_windows_equal_the_binary(hip, gold, sma_win):
    """sma_win is a field of the config struct: the short inputs, where the edge rules of the smoother and of the regression show,
    against what the binary wrote for a copy of the file with smaWin edited"""
    capi, ctx, _ = hip
    cfg = capi.emobase_config()
    cfg.sma_win = sma_win
    plan = capi.Plan(ctx, cfg)
    ks = [3, 4, 5, 6, 7, 8, 9, 10]
    pcms = [gold_pcm(gold, k)[0] for k in ks]
    b = capi.Batch(plan, offsets(pcms))
    out = b.emobase_run_host(np.concatenate(pcms))[0]
    for i, k in enumerate(ks):
        assert bits_equal(out[b.frame_offsets[i]:b.frame_offsets[i + 1]], gold["lld_w%d_%d" % (sma_win, k)]), (sma_win, k)
    b.close()
    plan.close()


@pytest.mark.parametrize("tag", ["mp300", "p10"])
def test_edited_parameters_equal_the_binary(hip, gold, tag):
    """maxPitch and voicingCutoff as fields of the config struct, cLpc's order through smilehip_plan_set_lpc_order, against what the
    binary wrote for a copy of the file with the same options edited: the levels and every column, bit for bit"""
    capi, ctx, _ = hip
    cfg = capi.emobase_config()
    if tag == "mp300":
        cfg.pitch_max, cfg.voicing_cutoff = 300.0, 0.7
    plan = capi.Plan(ctx, cfg)
    if tag == "p10":
        plan.set_lpc_order(10)
        assert plan.geometry.n_out == 56
    ks = [10, 11]
    pcms = [gold_pcm(gold, k)[0] for k in ks]
    b = capi.Batch(plan, offsets(pcms))
    out, tap25, tap3 = b.emobase_run_host(np.concatenate(pcms))
    check_against_gold(gold, ks, b, out, tap25, tap3, sfx=tag + "_", what=tag + ": ")
    if tag == "p10":                                       # a batch keeps the order it was laid out for
        import torch
        plan.set_lpc_order(8)
        d = torch.zeros(64, device="cuda")
        L = capi.load()
        assert L.smilehip_lld_run(plan._h, b._h, d.data_ptr(), d.data_ptr(), 52, None) == -1 and b"laid out for cLpc p = 10" in L.smilehip_last_error()
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
    run_exe("--set", "emobase", "-I", wav, "-lldhtkoutput", htk, "-lldcsvoutput", csv, "-instname", stem)
    assert same_file(htk, "emobase_%s.htk" % stem) and same_file(csv, "emobase_%s.csv" % stem)


def test_front_end_filelist(tmp_path):
    lst = tmp_path / "list.txt"
    lst.write_text("".join(os.path.join(GOLD, "files", s + ".wav") + "\n" for s in ("u2_8000", "u3_4000")))
    out = tmp_path / "out"
    out.mkdir()
    run_exe("--set", "emobase", "-filelist", str(lst), "-outdir", str(out), "-lldhtkoutput", "x", "-lldcsvoutput", "x")
    for s in ("u2_8000", "u3_4000"):
        assert same_file(out / (s + ".lld.htk"), "emobase_%s.htk" % s) and same_file(out / (s + ".lld.csv"), "emobase_%s.csv" % s)


needs_conf = pytest.mark.skipif(not os.path.isdir(CONF), reason="the reference's configuration files are not there (oracle/_ref not built)")


@needs_conf
def test_front_end_conf_file(tmp_path):
    conf = os.path.join(CONF, "emobase", "emobase.conf")
    for stem in ("u2_8000", "u3_4000"):
        htk, csv = str(tmp_path / (stem + ".htk")), str(tmp_path / (stem + ".csv"))
        run_exe("--set", "emobase", "-C", conf, "-I", os.path.join(GOLD, "files", stem + ".wav"), "-lldhtkoutput", htk, "-lldcsvoutput", csv, "-instname", stem)
        assert same_file(htk, "emobase_%s.htk" % stem) and same_file(csv, "emobase_%s.csv" % stem)


@needs_conf
@pytest.mark.parametrize("tag,edits", [("mp300", {"maxPitch = 500": "maxPitch = 300", "voicingCutoff = 0.550000": "voicingCutoff = 0.700000"}),
                                       ("p10", {"\np = 8\n": "\np = 10\n"}),
                                       ("w5", {"smaWin = 3": "smaWin = 5"})])
def test_front_end_edited_conf_equals_the_binary(gold, tmp_path, tag, edits):
    """--set emobase -C edited.conf on the 2080-sample input: the rows the binary wrote for the same edited copy"""
    from oracle import lldo
    text = open(os.path.join(CONF, "emobase", "emobase.conf"), encoding="latin-1").read().replace("\\{../shared/", "\\{" + os.path.join(CONF, "shared") + "/")
    for a, b in edits.items():
        assert text.count(a) == 1
        text = text.replace(a, b)
    conf = tmp_path / "edited.conf"
    conf.write_text(text, encoding="latin-1")
    pcm, fs = gold_pcm(gold, 10)
    wav, htk = str(tmp_path / "in.wav"), str(tmp_path / "e.htk")
    lldo.write_wav(wav, pcm, fs)
    run_exe("--set", "emobase", "-C", str(conf), "-I", wav, "-lldhtkoutput", htk)
    ref = gold["lld_w5_10"] if tag == "w5" else gold["lld_%s_10" % tag]
    assert bits_equal(lldo.read_htk(htk)[0].reshape(-1, ref.shape[1]), ref)
    assert ref.shape != gold["lld_10"].shape or not bits_equal(ref, gold["lld_10"])
