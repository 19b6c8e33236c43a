"""config/prosody/prosodyShs.conf as a fused batch set (SMILEHIP_CHAIN_PROSODY_SHS) on the device: the F0 front end's frame kernels
on 50 ms frames and the row-parallel tail kernel (lld_prosody.hip), held bit for bit to the real binary's lld level and cPitchShs
rows (tests/golden/make_golden_prosody_shs.py), to the chain of the library's own per-component operators, across chunk seams,
on the hard-signal corpus and through the smilextract_hip front end. Tolerance everywhere: identical bits."""
import os
import subprocess
import sys

import numpy as np
import pytest

from test_prosody_shs_host import GOLD, gold_pcm

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "opensmile_amd", "smilextract_hip")
CONF = os.path.join(ROOT, "oracle", "_ref", "config")


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLD, "prosody_shs_synth.npz"))


@pytest.fixture(scope="module")
def hip():
    from opensmile_amd import capi
    ctx = capi.Context(0)
    plan = capi.Plan(ctx, capi.prosody_shs_config())
    g = plan.geometry
    assert (g.frame_size, g.frame_step, g.fft_size, g.n_bins, g.n_out) == (800, 160, 1024, 513, 3)
    return capi, ctx, plan


def taps15(shs21):
    """the library's 21-value cPitchShs rows as the binary's level holds them with nCandidates = 4"""
    return np.concatenate([shs21[:, 0:1], shs21[:, 1:5], shs21[:, 7:11], shs21[:, 13:17], shs21[:, 19:21]], axis=1)


def run_f32(capi, plan, off, pcm_f32):
    import torch
    b = capi.Batch(plan, off)
    d_pcm = torch.from_numpy(np.ascontiguousarray(pcm_f32, np.float32)).cuda()
    d_out = torch.full((max(b.total_rows, 1), 3), -7.0, dtype=torch.float32, device="cuda")
    b.run_device_f32(d_pcm.data_ptr(), d_out.data_ptr(), 3)
    torch.cuda.synchronize()
    out, fo = d_out.cpu().numpy()[:b.total_rows], b.frame_offsets.copy()
    b.close()
    return out, fo


# ---------------------------------------------------------------------------------------------- 1. golden, ragged batch
def test_golden_ragged_batch(hip, gold):
    from tolerance import assert_bits_equal
    capi, ctx, plan = hip
    ks = [k for k, (idx, n, fs) in enumerate(gold["inputs"]) if fs == 16000]
    assert [int(gold["inputs"][k][1]) for k in ks] == [0, 100, 799, 800, 960, 1120, 1280, 2080, 16000, 48000]
    pcms = [gold_pcm(gold, k)[0] for k in ks]
    off = np.concatenate([[0], np.cumsum([len(p) for p in pcms])]).astype(np.int64)
    pcm = np.concatenate(pcms)
    b = capi.Batch(plan, off)
    np.testing.assert_array_equal(np.diff(b.frame_offsets), [len(gold["lld_%d" % k]) for k in ks])     # rows as the binary's
    assert b.total_frames == sum(len(gold["shs_%d" % k]) for k in ks)
    out, taps = b.prosody_shs_run_host(pcm, taps=True)
    b.close()
    f0 = 0
    for i, k in enumerate(ks):
        T = len(gold["shs_%d" % k])
        if T:
            assert_bits_equal(taps15(taps["shs"][f0:f0 + T]), gold["shs_%d" % k], "cPitchShs rows, input %d" % k)
        f0 += T
        assert_bits_equal(out[b.frame_offsets[i]:b.frame_offsets[i + 1]], gold["lld_%d" % k].reshape(-1, 3), "lld, input %d" % k)
    # the same samples as floats (smilehip_lld_run_f32)
    out32, fo = run_f32(capi, plan, off, (pcm.astype(np.float32) / np.float32(32767.0)).astype(np.float32))
    np.testing.assert_array_equal(fo, b.frame_offsets)
    assert_bits_equal(out32, out, "float input")


def test_golden_other_rates(gold):
    from tolerance import assert_bits_equal
    from opensmile_amd import capi
    ctx = capi.Context(0)
    seen = set()
    for k, (idx, n, fs) in enumerate(gold["inputs"]):
        if fs == 16000:
            continue
        cfg = capi.prosody_shs_config()
        cfg.sample_rate = float(fs)
        plan = capi.Plan(ctx, cfg)
        pcm, _ = gold_pcm(gold, k)
        b = capi.Batch(plan, np.array([0, len(pcm)], np.int64))
        out, taps = b.prosody_shs_run_host(pcm, taps=True)
        b.close()
        assert_bits_equal(taps15(taps["shs"]), gold["shs_%d" % k], "cPitchShs rows at %d Hz" % fs)
        assert_bits_equal(out, gold["lld_%d" % k], "lld at %d Hz" % fs)
        plan.close()
        seen.add(int(fs))
    assert seen == {8000, 44100, 48000}


# ---------------------------------------------------------------------------------------------- 2. fused = per-component
def sma_rows(x, rows, W=1):
    """cContourSmoother over one level of len(x) frames, `rows` rows: centre, -1, +1 in float; clamped positions, and in the
    left-padding rows a position beyond the last frame is an unwritten slot, zero (lld_prosody_ops.hpp)"""
    f = np.float32
    n = len(x)
    y = np.zeros(rows, f)
    for r in range(rows):
        val = lambda i: f(0) if (r - W < 0 and i > n - 1) else x[min(max(i, 0), n - 1)]
        acc = f(val(r))
        for k in range(1, W + 1):
            acc = f(acc + val(r - k))
            acc = f(acc + val(r + k))
        y[r] = f(acc / f(2 * W + 1))
    return y


def test_fused_equals_per_component_operators(hip):
    import torch
    from tolerance import assert_bits_equal
    from opensmile_amd import synth
    capi, ctx, plan = hip
    L = capi.load()
    lens = [16000, 100, 799, 800, 960, 1120, 1280, 2080, 2240, 0, 8000]
    pcms = [synth.utterance(20 + i, n) if n else np.zeros(0, np.int16) for i, n in enumerate(lens)]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    b = capi.Batch(plan, off)
    fused = b.run_host(np.concatenate(pcms))
    fo = b.frame_offsets.copy()
    b.close()
    N, H, K = 800, 160, 513
    for u, (n, pcm) in enumerate(zip(lens, pcms)):
        T = 0 if n < N else (n - N) // H + 1
        rows = T if T >= 2 else 0
        assert fo[u + 1] - fo[u] == rows, (n, T)
        if not rows:
            continue
        x = (pcm.astype(np.float32) / np.float32(32767.0)).astype(np.float32)
        frames = np.stack([x[t * H:t * H + N] for t in range(T)])
        d_fr = torch.from_numpy(frames).cuda()
        d_w, d_c = torch.zeros((T, N), device="cuda"), torch.zeros((T, 1024), device="cuda")
        d_m, d_h, d_s = torch.zeros((T, K), device="cuda"), torch.zeros((T, K), device="cuda"), torch.zeros((T, 21), device="cuda")
        capi.window_frames(plan, d_fr.data_ptr(), N, d_w.data_ptr(), N, T)
        capi.rfft_frames(plan, d_w.data_ptr(), N, d_c.data_ptr(), 1024, T)
        capi.fftmag_frames(plan, d_c.data_ptr(), 1024, d_m.data_ptr(), K, T)
        capi._check(L.smilehip_specscale_frames(plan._h, d_m.data_ptr(), K, d_h.data_ptr(), K, T, None))
        capi._check(L.smilehip_pitchshs_frames(plan._h, d_h.data_ptr(), K, d_s.data_ptr(), 21, T, None))
        # cPitchSmoother as the file runs it (postSmoothingMethod = simple), F0final | voicingFinalUnclipped: rows = [F0Cand | candVoicing | candScore]
        d_c18 = torch.cat([d_s[:, 1:7], d_s[:, 7:13], d_s[:, 13:19]], dim=1).contiguous()
        d_p = torch.zeros((T, 2), device="cuda")
        d_wr = torch.zeros(1, dtype=torch.int64, device="cuda")
        capi._check(L.smilehip_pitch_smoother_rows(ctx._h, 6, 0.7, 0, 1, 1 | 8, d_c18.data_ptr(), 18, None, 1, T, None, 0, d_p.data_ptr(), 2,
                                                   d_wr.data_ptr(), None))
        d_l = torch.zeros((T, 1), device="cuda")
        capi._check(L.smilehip_intensity_frames(ctx._h, d_fr.data_ptr(), N, N, 2, d_l.data_ptr(), 1, T, None))
        torch.cuda.synchronize()
        assert int(d_wr.item()) == T - 1
        p, l = d_p.cpu().numpy()[:T - 1], d_l.cpu().numpy()[:, 0]
        ref = np.stack([sma_rows(p[:, 0], rows), sma_rows(p[:, 1], rows), sma_rows(l, rows)], axis=1)
        assert_bits_equal(fused[fo[u]:fo[u + 1]], ref, "utterance %d (%d samples)" % (u, n))


# ---------------------------------------------------------------------------------------------- 3. chunk seams
SEAM_SCRIPT = r"""
import sys, numpy as np
sys.path.insert(0, %r)
from opensmile_amd import capi, synth
ctx = capi.Context(0)
plan = capi.Plan(ctx, capi.prosody_shs_config())
pcms = [synth.utterance(40 + i, 16000) for i in range(12)]
off = np.arange(13, dtype=np.int64) * 16000
b = capi.Batch(plan, off)
assert b.total_frames == 12 * 96
np.save(sys.argv[1], b.run_host(np.concatenate(pcms)))
""" % ROOT


def test_chunk_seams(hip, tmp_path):
    from opensmile_amd import synth
    capi, ctx, plan = hip
    pcms = [synth.utterance(40 + i, 16000) for i in range(12)]
    b = capi.Batch(plan, np.arange(13, dtype=np.int64) * 16000)
    assert b.total_frames == 12 * 96 > 2 * 64 * 8                       # 144 tiles of 8 frames: three chunks of 64 tiles
    whole = b.run_host(np.concatenate(pcms))
    b.close()
    path = str(tmp_path / "seams.npy")
    p = subprocess.run([sys.executable, "-c", SEAM_SCRIPT, path], env=dict(os.environ, SMILEHIP_F0_CHUNK_TILES="64"), capture_output=True,
                       text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    cut = np.load(path)
    assert cut.shape == whole.shape == (12 * 96, 3)
    assert np.array_equal(cut.view(np.uint32), whole.view(np.uint32))


# ---------------------------------------------------------------------------------------------- 4. re-run, empty batch, ld_out
def test_rerun_empty_and_ld_out(hip):
    import torch
    from opensmile_amd import synth
    capi, ctx, plan = hip
    L = capi.load()
    pcm = np.concatenate([synth.utterance(3, 32000), synth.utterance(4, 1000), synth.utterance(5, 16000)])
    b = capi.Batch(plan, np.array([0, 32000, 33000, 49000], np.int64))
    a = b.run_host(pcm)
    c = b.run_host(pcm)
    assert a.shape == (196 + 2 + 96, 3) and np.array_equal(a.view(np.uint32), c.view(np.uint32))
    d_pcm = torch.from_numpy(pcm).cuda()
    d_out = torch.zeros((b.total_rows, 3), device="cuda")
    rc = L.smilehip_lld_run(plan._h, b._h, d_pcm.data_ptr(), d_out.data_ptr(), 2, None)
    assert rc == -1 and b"ld_out" in L.smilehip_last_error()            # SMILEHIP_ERR_INVALID, by name
    torch.cuda.synchronize()
    assert float(d_out.abs().max()) == 0.0
    b.close()
    e = capi.Batch(plan, np.array([0, 0, 100, 899], np.int64))          # nothing, 100 samples, 799 samples: no frame anywhere
    assert e.total_frames == 0 and e.total_rows == 0 and list(e.frame_offsets) == [0, 0, 0, 0]
    assert e.run_host(np.zeros(899, np.int16)).shape == (0, 3)
    e.close()
    cfg = capi.prosody_shs_config()
    cfg.specscale_off = 1
    p2 = capi.Plan(ctx, cfg)
    b2 = capi.Batch(p2, np.array([0, 16000], np.int64))
    rc = L.smilehip_lld_run(p2._h, b2._h, d_pcm.data_ptr(), d_out.data_ptr(), 3, None)
    assert rc == -1 and b"specscale_off" in L.smilehip_last_error()
    b2.close()
    p2.close()


# ---------------------------------------------------------------------------------------------- 5. hard signals
def test_hard_signals(hip):
    from tolerance import assert_bits_equal
    from helpers import hard_signals
    capi, ctx, plan = hip
    ref = np.load(os.path.join(GOLD, "hard_prosody_shs.npz"))
    pcm = np.load(os.path.join(GOLD, "hard_pcm.npz"))
    sig = [np.ascontiguousarray(pcm[n], np.int16) for n in hard_signals.NAMES]
    off = np.concatenate([[0], np.cumsum([len(s) for s in sig])]).astype(np.int64)
    b = capi.Batch(plan, off)
    out = b.run_host(np.concatenate(sig))
    for i, n in enumerate(hard_signals.NAMES):
        assert_bits_equal(out[b.frame_offsets[i]:b.frame_offsets[i + 1]], ref["lld_" + n], n)
    b.close()


# ---------------------------------------------------------------------------------------------- 6. front end
def run_exe(*args):
    p = subprocess.run([EXE, *args], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]


@pytest.mark.parametrize("stem", ["u2_8000", "u3_4000"])
def test_front_end_set_writes_the_binary_s_files(tmp_path, stem):
    wav = os.path.join(GOLD, "files", stem + ".wav")
    htk, csv = str(tmp_path / "o.htk"), str(tmp_path / "o.csv")
    run_exe("--set", "prosody_shs", "-I", wav, "-O", htk, "-csvoutput", csv, "-instname", stem)
    assert open(htk, "rb").read() == open(os.path.join(GOLD, "files", "prosody_shs_%s.htk" % stem), "rb").read()
    assert open(csv, "rb").read() == open(os.path.join(GOLD, "files", "prosody_shs_%s.csv" % stem), "rb").read()


def test_front_end_filelist(tmp_path):
    lst = tmp_path / "list.txt"
    lst.write_text("".join(os.path.join(GOLD, "files", s + ".wav") + "\n" for s in ("u2_8000", "u3_4000")))
    out = tmp_path / "out"
    out.mkdir()
    run_exe("--set", "prosody_shs", "-filelist", str(lst), "-outdir", str(out), "-O", "x", "-csvoutput", "x")
    for s in ("u2_8000", "u3_4000"):
        assert open(out / (s + ".htk"), "rb").read() == open(os.path.join(GOLD, "files", "prosody_shs_%s.htk" % s), "rb").read()
        assert open(out / (s + ".csv"), "rb").read() == open(os.path.join(GOLD, "files", "prosody_shs_%s.csv" % s), "rb").read()


needs_conf = pytest.mark.skipif(not os.path.isdir(CONF), reason="the reference's configuration files are not there (oracle/_ref not built)")


@needs_conf
def test_front_end_conf_file(tmp_path):
    conf = os.path.join(CONF, "prosody", "prosodyShs.conf")
    for stem in ("u2_8000", "u3_4000"):
        htk, csv = str(tmp_path / (stem + ".htk")), str(tmp_path / (stem + ".csv"))
        run_exe("--set", "prosody_shs", "-C", conf, "-I", os.path.join(GOLD, "files", stem + ".wav"), "-O", htk, "-csvoutput", csv, "-instname", stem)
        assert open(htk, "rb").read() == open(os.path.join(GOLD, "files", "prosody_shs_%s.htk" % stem), "rb").read()
        assert open(csv, "rb").read() == open(os.path.join(GOLD, "files", "prosody_shs_%s.csv" % stem), "rb").read()


@needs_conf
def test_front_end_edited_conf_equals_the_c_abi(hip, tmp_path):
    import wave
    from oracle import lldo
    capi, ctx, _ = hip
    text = open(os.path.join(CONF, "prosody", "prosodyShs.conf")).read()
    assert text.count("maxPitch = 620") == 1
    text = text.replace("maxPitch = 620", "maxPitch = 400").replace("\\{../shared/", "\\{" + os.path.join(CONF, "shared") + "/")
    conf = tmp_path / "edited.conf"
    conf.write_text(text)
    wav = os.path.join(GOLD, "files", "u2_8000.wav")
    htk = str(tmp_path / "e.htk")
    run_exe("--set", "prosody_shs", "-C", str(conf), "-I", wav, "-O", htk)
    with wave.open(wav, "rb") as w:
        pcm = np.frombuffer(w.readframes(w.getnframes()), dtype="<i2")
    cfg = capi.prosody_shs_config()
    cfg.pitch_max = 400.0
    plan = capi.Plan(ctx, cfg)
    b = capi.Batch(plan, np.array([0, len(pcm)], np.int64))
    ref = b.run_host(pcm)
    b.close()
    plan.close()
    got = lldo.read_htk(htk)[0]
    assert got.shape == ref.shape and np.array_equal(got.view(np.uint32), ref.view(np.uint32))


# ---------------------------------------------------------------------------------------------- 7. a parameter of the chain: smaWin
@pytest.mark.parametrize("sma_win", [5, 7, 9])
def test_wider_smoothing_windows_equal_the_binary(hip, gold, sma_win):
    """sma_win is a field of the config struct: the short inputs, where the smoother's edge rules show, against what the binary
    wrote for a copy of the file with smaWin edited (lld_w5_<k>, lld_w7_<k> of the golden)"""
    from tolerance import assert_bits_equal
    capi, ctx, _ = hip
    cfg = capi.prosody_shs_config()
    cfg.sma_win = sma_win
    plan = capi.Plan(ctx, cfg)
    ks = [4, 5, 6, 7, 8]
    pcms = [gold_pcm(gold, k)[0] for k in ks]
    b = capi.Batch(plan, np.concatenate([[0], np.cumsum([len(p) for p in pcms])]).astype(np.int64))
    out = b.run_host(np.concatenate(pcms))
    for i, k in enumerate(ks):
        assert_bits_equal(out[b.frame_offsets[i]:b.frame_offsets[i + 1]], gold["lld_w%d_%d" % (sma_win, k)], "smaWin %d, input %d" % (sma_win, k))
    b.close()
    plan.close()


EDITED = {"maxpitch400": dict(pitch_max=400.0),
          "all": dict(pitch_max=400.0, pitch_min=60.0, shs_n_candidates=6, specscale_min_f=20.0, voicing_cutoff=0.6, shs_n_harmonics=12,
                      shs_compression=0.8)}


@pytest.mark.parametrize("tag", sorted(EDITED))
def test_edited_parameters_equal_the_binary(hip, gold, tag):
    """the chain's other parameters as fields of the config struct, against what the binary wrote for a copy of the file with the
    same options edited (make_golden_prosody_shs.EDITS): cPitchShs rows and the three columns, bit for bit"""
    from tolerance import assert_bits_equal
    capi, ctx, _ = hip
    cfg = capi.prosody_shs_config()
    for f, v in EDITED[tag].items():
        setattr(cfg, f, v)
    plan = capi.Plan(ctx, cfg)
    ks = [7, 8]
    pcms = [gold_pcm(gold, k)[0] for k in ks]
    b = capi.Batch(plan, np.concatenate([[0], np.cumsum([len(p) for p in pcms])]).astype(np.int64))
    out, taps = b.prosody_shs_run_host(np.concatenate(pcms), taps=True)
    f0 = 0
    for i, k in enumerate(ks):
        ref_shs = gold["shs_%s_%d" % (tag, k)]
        mine = taps["shs"][f0:f0 + len(ref_shs)]
        assert_bits_equal(mine if ref_shs.shape[1] == 21 else taps15(mine), ref_shs, "%s: cPitchShs rows, input %d" % (tag, k))
        f0 += len(ref_shs)
        assert_bits_equal(out[b.frame_offsets[i]:b.frame_offsets[i + 1]], gold["lld_%s_%d" % (tag, k)], "%s: lld, input %d" % (tag, k))
    b.close()
    plan.close()


def test_front_end_serve(tmp_path):
    """--serve: two lists on one process (context and plan kept); every file equals the binary's"""
    lines = ""
    for tag in ("a", "b"):
        (tmp_path / tag).mkdir()
        lst = tmp_path / (tag + ".txt")
        lst.write_text("".join(os.path.join(GOLD, "files", s + ".wav") + "\n" for s in ("u2_8000", "u3_4000")))
        lines += "-filelist %s -outdir %s\n" % (lst, tmp_path / tag)
    r = subprocess.run([EXE, "--set", "prosody_shs", "-O", "1", "-csvoutput", "1", "--serve"], input=lines + "quit\n", capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-1500:]
    done = [l.split() for l in r.stdout.splitlines() if l.startswith("done ")]
    assert len(done) == 2 and all(d[1] == "0" for d in done), r.stdout
    for tag in ("a", "b"):
        for s in ("u2_8000", "u3_4000"):
            for ext in ("htk", "csv"):
                assert open(tmp_path / tag / (s + "." + ext), "rb").read() == open(os.path.join(GOLD, "files", "prosody_shs_%s.%s" % (s, ext)), "rb").read()
