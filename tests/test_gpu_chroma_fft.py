"""config/chroma/chroma_fft.conf as a fused batch set (SMILEHIP_CHAIN_CHROMA_FFT) on the device: lld_chroma_frame in both of its
forms (a wave per frame at 8 / 11.025 / 16 kHz, a workgroup per frame above) and the two per-component operators, held bit for bit
to the real binary's tonespec and chroma levels (tests/golden/make_golden_chroma_fft.py), to the chain of the library's own
operators, across workgroup seams and the persistent grid's second trip, on the hard-signal corpus and through the smilextract_hip
front end. Tolerance everywhere: identical bits."""
import os
import subprocess
import sys

import numpy as np
import pytest

from test_chroma_fft_host import EDITED, GOLD, MINIMAL, geometry, gold_pcm

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "opensmile_amd", "smilextract_hip")
WAVE_FRAMES = 4                                            # frames per workgroup of the wave form (lld_chroma.hip: kChromaWaves)
WG_PER_CU_MAX = 4                                          # ... and its workgroups per CU at most (chroma_wave_grid_cap: 16 / kChromaWaves)
N16 = 8


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLD, "chroma_fft_synth.npz"))


@pytest.fixture(scope="module")
def hip():
    from opensmile_amd import capi
    ctx = capi.Context(0)
    plan = capi.Plan(ctx, capi.chroma_fft_config())
    g = plan.geometry
    assert (g.frame_size, g.frame_step, g.fft_size, g.n_bins, g.n_out) == (1024, 160, 1024, 513, 12)
    return capi, ctx, plan


def offsets(pcms):
    return np.concatenate([[0], np.cumsum([len(p) for p in pcms])]).astype(np.int64)


def as_f32(pcm):
    return (np.asarray(pcm).astype(np.float32) / np.float32(32767.0)).astype(np.float32)


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def check_against_gold(gold, ks, b, out, tap, suffix="%d", what=""):
    """rows, every cell and the tap (level tonespec) of the batch's utterances against the binary's"""
    from tolerance import assert_bits_equal
    f0 = 0
    for i, k in enumerate(ks):
        ref, ts = gold["chroma_" + suffix % k], gold["tonespec_" + suffix % k]
        T = len(ref)
        assert b.frame_offsets[i + 1] - b.frame_offsets[i] == T, (k, T)
        if T:
            assert_bits_equal(tap[f0:f0 + T], ts, "%slevel tonespec, input %d" % (what, k))
            assert_bits_equal(out[b.frame_offsets[i]:b.frame_offsets[i + 1]], ref, "%slevel chroma, input %d" % (what, k))
        f0 += T
    assert f0 == b.total_frames == len(tap)


# ---------------------------------------------------------------------------------------------- 1. golden
def test_golden_ragged_batch(hip, gold):
    """all 16 kHz inputs in one batch, the empty one and the one-sample-short one between long ones; the tap is the tonespec level"""
    capi, ctx, plan = hip
    ks = [6, 1, 2, 0, 3, 7, 4, 5]
    assert all(int(gold["inputs"][k][2]) == 16000 for k in ks) and sorted(ks) == list(range(N16))
    assert sum(1 for r in gold["inputs"] if r[2] == 16000) == N16
    pcms = [gold_pcm(gold, k)[0] for k in ks]
    b = capi.Batch(plan, offsets(pcms))
    out, tap = b.chroma_run_host(np.concatenate(pcms))
    check_against_gold(gold, ks, b, out, tap)
    nz = (out != 0).any(axis=1)
    assert nz.any() and (~nz).any()                        # both branches of the silence flag
    b.close()


def test_golden_other_rates(gold):
    """the six other rates: the wave form with M = 256 (8 kHz) and M = 512 (11.025 kHz, a zero-padded frame of 706 samples), the
    workgroup form at 2048 and 4096 points; int16 and float input"""
    from opensmile_amd import capi
    ctx = capi.Context(0)
    seen = {}
    for k, (idx, n, fs, div) in enumerate(gold["inputs"]):
        if fs == 16000:
            continue
        plan = capi.Plan(ctx, capi.chroma_fft_config(float(fs)))
        assert (plan.geometry.frame_size, plan.geometry.frame_step) == geometry(int(fs))
        pcm, _ = gold_pcm(gold, k)
        b = capi.Batch(plan, np.array([0, len(pcm)], np.int64))
        out, tap = b.chroma_run_host(pcm)
        check_against_gold(gold, [k], b, out, tap, what="%d Hz: " % fs)
        out32, tap32 = b.chroma_run_host(as_f32(pcm))
        assert bits_equal(out32, out) and bits_equal(tap32, tap)
        b.close()
        seen[int(fs)] = plan.geometry.fft_size
        plan.close()
    assert seen == {8000: 512, 11025: 1024, 22050: 2048, 32000: 2048, 44100: 4096, 48000: 4096}


def test_float_input_equals_int16(hip, gold):
    capi, ctx, plan = hip
    pcm, _ = gold_pcm(gold, 6)                             # the 1 s input
    b = capi.Batch(plan, np.array([0, len(pcm)], np.int64))
    out, tap = b.chroma_run_host(pcm)
    out32, tap32 = b.chroma_run_host(as_f32(pcm))
    assert bits_equal(out32, out) and bits_equal(tap32, tap) and bits_equal(out, gold["chroma_6"])
    assert bits_equal(b.run_host(pcm), out)                # smilehip_lld_run_host
    b.close()


CHILD = """
import sys
import numpy as np
sys.path.insert(0, %r)
sys.path.insert(0, %r)
from opensmile_amd import capi
from test_chroma_fft_host import GOLD, gold_pcm
from test_gpu_chroma_fft import check_against_gold, offsets
import os
gold = np.load(os.path.join(GOLD, "chroma_fft_synth.npz"))
ctx = capi.Context(0)
for fs, ks in ((16000, [6, 1, 2, 0, 3, 7, 4, 5]), (8000, [8]), (11025, [9])):
    plan = capi.Plan(ctx, capi.chroma_fft_config(float(fs)))
    pcms = [gold_pcm(gold, k)[0] for k in ks]
    b = capi.Batch(plan, offsets(pcms))
    out, tap = b.chroma_run_host(np.concatenate(pcms))
    check_against_gold(gold, ks, b, out, tap, what="workgroup form, %%d Hz: " %% fs)
    b.close()
    plan.close()
print("CHILD OK", os.environ.get("SMILEHIP_CHROMA"))
"""


def test_workgroup_form_equals_the_binary():
    """SMILEHIP_CHROMA=block: the workgroup-per-frame form where the wave form would run (512 / 1024 points), in a fresh process"""
    env = dict(os.environ, SMILEHIP_CHROMA="block")
    r = subprocess.run([sys.executable, "-c", CHILD % (ROOT, os.path.join(ROOT, "tests"))], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "CHILD OK block" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])


# ---------------------------------------------------------------------------------------------- 2. fused = per-component
def tonespec_op(capi, ctx, opts, n_src, fss):
    import ctypes as C
    op = C.c_void_p()
    capi._check(capi.load().smilehip_tonespec_op_create(ctx._h, C.byref(opts), n_src, fss, C.byref(op)))
    return op


def chroma_op(capi, ctx, opts, n_src):
    import ctypes as C
    op = C.c_void_p()
    capi._check(capi.load().smilehip_chroma_op_create(ctx._h, C.byref(opts), n_src, C.byref(op)))
    return op


def per_component(capi, ctx, plan, pcm):
    """the chain out of the operators, one launch each over all frames of one utterance: (chroma rows, tonespec rows)"""
    import torch
    L = capi.load()
    g = plan.geometry
    N, H, K, Nfft = g.frame_size, g.frame_step, g.n_bins, g.fft_size
    T = (len(pcm) - N) // H + 1
    x = as_f32(pcm)
    d_fr = torch.from_numpy(np.stack([x[t * H:t * H + N] for t in range(T)])).cuda()
    d_w, d_c, d_m = torch.zeros((T, N), device="cuda"), torch.zeros((T, Nfft), device="cuda"), torch.zeros((T, K), device="cuda")
    capi.window_frames(plan, d_fr.data_ptr(), N, d_w.data_ptr(), N, T)
    capi.rfft_frames(plan, d_w.data_ptr(), N, d_c.data_ptr(), Nfft, T)
    capi.fftmag_frames(plan, d_c.data_ptr(), Nfft, d_m.data_ptr(), K, T)
    top = tonespec_op(capi, ctx, capi.tonespec_opts(), K, g.fft_frame_size_sec)
    cop = chroma_op(capi, ctx, capi.chroma_opts(), 72)
    assert L.smilehip_tonespec_op_n_out(top) == 72
    d_ts, d_ch = torch.zeros((T, 72), device="cuda"), torch.zeros((T, 12), device="cuda")
    capi._check(L.smilehip_tonespec_op_frames(top, d_m.data_ptr(), K, d_ts.data_ptr(), 72, T, None))
    capi._check(L.smilehip_chroma_op_frames(cop, d_ts.data_ptr(), 72, d_ch.data_ptr(), 12, T, None))
    torch.cuda.synchronize()
    capi._check(L.smilehip_tonespec_op_destroy(top))
    capi._check(L.smilehip_chroma_op_destroy(cop))
    return d_ch.cpu().numpy(), d_ts.cpu().numpy()


@pytest.mark.parametrize("fs", [16000, 44100])
def test_fused_equals_per_component_operators(fs):
    """a seeded 2 s signal on which no fixture exists, once per kernel form: window, transform and magnitude operators feed the
    tonespec operator, which feeds the chroma operator"""
    from tolerance import assert_bits_equal
    from opensmile_amd import capi, synth
    ctx = capi.Context(0)
    plan = capi.Plan(ctx, capi.chroma_fft_config(float(fs)))
    pcm = (synth.utterance(31, 2 * fs).astype(np.int32) // 100).astype(np.int16)
    b = capi.Batch(plan, np.array([0, len(pcm)], np.int64))
    fused, tap = b.chroma_run_host(pcm)
    b.close()
    ref, ts = per_component(capi, ctx, plan, pcm)
    nz = (ref != 0).any(axis=1)
    assert nz.any() and (~nz).any()
    assert_bits_equal(tap, ts, "level tonespec at %d Hz" % fs)
    assert_bits_equal(fused, ref, "level chroma at %d Hz" % fs)
    plan.close()


def test_operators_on_strided_rows(gold):
    """ld larger than the row on both sides, the gaps poisoned: the rows are the binary's, the gaps keep the poison"""
    import torch
    from opensmile_amd import capi
    ctx = capi.Context(0)
    L = capi.load()
    mag, ts, ch = gold["fftmag_5"], gold["tonespec_5"], gold["chroma_5"]
    T, K = mag.shape
    poison = np.float32(-7.25)
    top = tonespec_op(capi, ctx, capi.tonespec_opts(), K, 0.064)
    cop = chroma_op(capi, ctx, capi.chroma_opts(), 72)
    src = np.full((T, K + 5), poison, np.float32)
    src[:, :K] = mag
    d_src = torch.from_numpy(src).cuda()
    d_ts = torch.full((T, 72 + 9), float(poison), device="cuda")
    d_ch = torch.full((T, 12 + 3), float(poison), device="cuda")
    capi._check(L.smilehip_tonespec_op_frames(top, d_src.data_ptr(), K + 5, d_ts.data_ptr(), 81, T, None))
    capi._check(L.smilehip_chroma_op_frames(cop, d_ts.data_ptr(), 81, d_ch.data_ptr(), 15, T, None))
    torch.cuda.synchronize()
    h_ts, h_ch = d_ts.cpu().numpy(), d_ch.cpu().numpy()
    assert bits_equal(h_ts[:, :72], ts) and (h_ts[:, 72:] == poison).all()
    assert bits_equal(h_ch[:, :12], ch) and (h_ch[:, 12:] == poison).all()
    assert bits_equal(d_src.cpu().numpy(), src)
    # refusals: a leading dimension below the row, null rows, an input that is no multiple of octaveSize
    assert L.smilehip_tonespec_op_frames(top, d_src.data_ptr(), K - 1, d_ts.data_ptr(), 81, T, None) == -1
    assert L.smilehip_tonespec_op_frames(top, d_src.data_ptr(), K + 5, d_ts.data_ptr(), 71, T, None) == -1
    assert L.smilehip_chroma_op_frames(cop, d_ts.data_ptr(), 81, d_ch.data_ptr(), 11, T, None) == -1
    assert L.smilehip_chroma_op_frames(cop, None, 81, None, 15, 0, None) == 0
    import ctypes as C
    bad = C.c_void_p()
    assert L.smilehip_chroma_op_create(ctx._h, C.byref(capi.chroma_opts()), 70, C.byref(bad)) == -1 and b"octaveSize" in L.smilehip_last_error()
    capi._check(L.smilehip_tonespec_op_destroy(top))
    capi._check(L.smilehip_chroma_op_destroy(cop))


# ---------------------------------------------------------------------------------------------- 3. workgroup seams
def test_workgroup_seams(hip):
    """batches of 3, 4, 5 and 9 frames in all (one short of, equal to, one past a workgroup's frames, and into a third workgroup):
    each utterance's rows equal its rows when run alone"""
    from opensmile_amd import synth
    capi, ctx, plan = hip
    alone = {}
    for T in (1, 2, 3, 4):
        n = 1024 + 160 * (T - 1)
        pcm = synth.utterance(50 + T, n)
        b = capi.Batch(plan, np.array([0, n], np.int64))
        assert b.total_frames == T
        alone[T] = (pcm,) + b.chroma_run_host(pcm)
        b.close()
    totals = set()
    for Ts in ([3], [1, 3], [2, 3], [4, 1, 4], [3, 2, 4]):
        pcms = [alone[T][0] for T in Ts]
        b = capi.Batch(plan, offsets(pcms))
        assert b.total_frames == sum(Ts)
        totals.add(sum(Ts))
        out, tap = b.chroma_run_host(np.concatenate(pcms))
        f0 = 0
        for i, T in enumerate(Ts):
            assert bits_equal(out[b.frame_offsets[i]:b.frame_offsets[i + 1]], alone[T][1]), (Ts, i)
            assert bits_equal(tap[f0:f0 + T], alone[T][2]), (Ts, i)
            f0 += T
        b.close()
    assert totals == {WAVE_FRAMES - 1, WAVE_FRAMES, WAVE_FRAMES + 1, 2 * WAVE_FRAMES + 1}


def test_persistent_wave_takes_a_second_frame(hip):
    """one utterance with more frames than the device's grid cap holds waves (CUs x WG_PER_CU_MAX workgroups x WAVE_FRAMES: the bound
    of chroma_wave_grid_cap whatever the LDS admits), so that the persistent loop runs again: its frames equal those of the same
    samples cut into utterances of at most 1000 frames, each a batch below the cap"""
    import torch
    from opensmile_amd import synth
    capi, ctx, plan = hip
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    frames = cus * WG_PER_CU_MAX * WAVE_FRAMES + 2 * WAVE_FRAMES + 1
    n = 1024 + 160 * (frames - 1)
    pcm = (synth.utterance(3, n).astype(np.int32) // 64).astype(np.int16)
    b = capi.Batch(plan, np.array([0, n], np.int64))
    assert b.total_frames == frames
    out, tap = b.chroma_run_host(pcm)
    b.close()
    nz = (out != 0).any(axis=1)
    assert nz.any() and (~nz).any()
    piece_frames = min(1000, cus * WAVE_FRAMES)
    for t0 in range(0, frames, piece_frames):
        T = min(piece_frames, frames - t0)
        piece = pcm[t0 * 160:t0 * 160 + 1024 + 160 * (T - 1)]
        pb = capi.Batch(plan, np.array([0, len(piece)], np.int64))
        assert pb.total_frames == T <= cus * WAVE_FRAMES
        o, tp = pb.chroma_run_host(piece)
        pb.close()
        assert bits_equal(out[t0:t0 + T], o) and bits_equal(tap[t0:t0 + T], tp), t0


# ---------------------------------------------------------------------------------------------- 4. re-run, empty batch, ld_out
def test_rerun_empty_and_ld_out(hip):
    import torch
    from opensmile_amd import synth
    capi, ctx, plan = hip
    L = capi.load()
    pcm = np.concatenate([synth.utterance(3, 32000), synth.utterance(4, 1000), synth.utterance(5, 16000)])
    b = capi.Batch(plan, np.array([0, 32000, 33000, 49000], np.int64))
    a, tap_a = b.chroma_run_host(pcm)
    c, tap_c = b.chroma_run_host(pcm, runs=2)
    assert a.shape == (194 + 0 + 94, 12) and bits_equal(a, c) and bits_equal(tap_a, tap_c)
    wide, _ = b.chroma_run_host(pcm, ld_out=17, fill=-7.5)
    assert bits_equal(wide[:, :12], a) and (wide[:, 12:] == np.float32(-7.5)).all()      # the pads keep what they held
    d_pcm = torch.from_numpy(pcm).cuda()
    d_out = torch.zeros((b.total_rows, 12), device="cuda")
    rc = L.smilehip_lld_run(plan._h, b._h, d_pcm.data_ptr(), d_out.data_ptr(), 11, None)
    assert rc == -1 and b"ld_out" in L.smilehip_last_error()            # SMILEHIP_ERR_INVALID, by name
    torch.cuda.synchronize()
    assert float(d_out.abs().max()) == 0.0
    b.close()
    e = capi.Batch(plan, np.array([0, 0, 100, 1123], np.int64))         # nothing, 100 samples, 1023 samples: no frame anywhere
    assert e.total_frames == 0 and e.total_rows == 0 and list(e.frame_offsets) == [0, 0, 0, 0]
    out, tap = e.chroma_run_host(np.zeros(1123, np.int16))
    assert out.shape == (0, 12) and tap.shape == (0, 72)
    e.close()
    other = capi.Batch(capi.Plan(ctx, capi.prosody_acf_config()), np.array([0, 16000], np.int64))
    assert L.smilehip_batch_chroma_taps(other._h, None, None) == -1 and b"not a chroma_fft chain batch" in L.smilehip_last_error()
    other.close()


# ---------------------------------------------------------------------------------------------- 5. hard signals
def test_hard_signals(hip):
    from tolerance import assert_bits_equal
    from helpers import hard_signals
    capi, ctx, plan = hip
    ref = np.load(os.path.join(GOLD, "hard_chroma_fft.npz"))
    pcm = np.load(os.path.join(GOLD, "hard_pcm.npz"))
    sig = [np.ascontiguousarray(pcm[n], np.int16) for n in hard_signals.NAMES]
    b = capi.Batch(plan, offsets(sig))
    out, _ = b.chroma_run_host(np.concatenate(sig))
    for i, n in enumerate(hard_signals.NAMES):
        assert_bits_equal(out[b.frame_offsets[i]:b.frame_offsets[i + 1]], ref["chroma_" + n], n)
    b.close()


# ---------------------------------------------------------------------------------------------- 6. parameters of the chain
@pytest.mark.parametrize("tag", sorted(EDITED))
def test_edited_parameters_equal_the_binary(hip, gold, tag):
    """nOctaves, firstNote, filterType, usePower, dbA, octaveSize and silThresh as fields of the config struct, against what the
    binary wrote for a copy of the file with the same options edited: both levels, bit for bit"""
    capi, ctx, _ = hip
    cfg = capi.chroma_fft_config()
    for f, v in EDITED[tag]["cfg"].items():
        setattr(cfg, f, v)
    plan = capi.Plan(ctx, cfg)
    ks = [5, 6]
    pcms = [gold_pcm(gold, k)[0] for k in ks]
    b = capi.Batch(plan, offsets(pcms))
    out, tap = b.chroma_run_host(np.concatenate(pcms))
    assert out.shape[1] == EDITED[tag]["octave_size"]
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
def test_front_end_set_writes_the_binary_s_file(tmp_path, stem):
    wav = os.path.join(GOLD, "files", stem + ".wav")
    csv = str(tmp_path / "o.csv")
    run_exe("--set", "chroma_fft", "-I", wav, "-O", csv)
    assert same_file(csv, "chroma_fft_%s.csv" % stem)


def test_front_end_csvoutput_has_header_and_time_stamps(tmp_path, gold):
    """-csvoutput: the other sets' CSV file (name, frameTime, header) with the same values"""
    wav = os.path.join(GOLD, "files", "u2_8000.wav")
    csv, plain = str(tmp_path / "o.csv"), str(tmp_path / "p.csv")
    run_exe("--set", "chroma_fft", "-I", wav, "-O", plain, "-csvoutput", csv, "-instname", "u2")
    assert same_file(plain, "chroma_fft_u2_8000.csv")
    lines = open(csv).read().splitlines()
    want = open(plain).read().splitlines()
    assert lines[0] == "name;frameTime;" + str(gold["csv_header"]) and len(lines) == len(want) + 1
    assert lines[1] == "'u2';0.000000;" + want[0] and lines[2].startswith("'u2';0.010000;")
    assert [ln.split(";", 2)[2] for ln in lines[1:]] == want


def test_front_end_filelist(tmp_path):
    lst = tmp_path / "list.txt"
    lst.write_text("".join(os.path.join(GOLD, "files", s + ".wav") + "\n" for s in ("u2_8000", "u3_4000")))
    out = tmp_path / "out"
    out.mkdir()
    run_exe("--set", "chroma_fft", "-filelist", str(lst), "-outdir", str(out), "-O", "x")
    for s in ("u2_8000", "u3_4000"):
        assert same_file(out / (s + ".csv"), "chroma_fft_%s.csv" % s)


def test_front_end_serve(tmp_path):
    """--serve: two lists on one process (context and plan kept); every file equals the binary's"""
    lines = ""
    for tag in ("a", "b"):
        (tmp_path / tag).mkdir()
        lst = tmp_path / (tag + ".txt")
        lst.write_text("".join(os.path.join(GOLD, "files", s + ".wav") + "\n" for s in ("u2_8000", "u3_4000")))
        lines += "-filelist %s -outdir %s\n" % (lst, tmp_path / tag)
    r = subprocess.run([EXE, "--set", "chroma_fft", "-O", "1", "--serve"], input=lines + "quit\n", capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-1500:]
    done = [l.split() for l in r.stdout.splitlines() if l.startswith("done ")]
    assert len(done) == 2 and all(d[1] == "0" for d in done), r.stdout
    for tag in ("a", "b"):
        for s in ("u2_8000", "u3_4000"):
            assert same_file(tmp_path / tag / (s + ".csv"), "chroma_fft_%s.csv" % s)


def test_front_end_conf_file(tmp_path):
    """--set chroma_fft -C: the graph in its own wording runs as the set and writes the binary's file"""
    conf = tmp_path / "c.conf"
    conf.write_text(MINIMAL)
    for stem in ("u2_8000", "u3_4000"):
        csv = str(tmp_path / (stem + ".csv"))
        run_exe("--set", "chroma_fft", "-C", str(conf), "-I", os.path.join(GOLD, "files", stem + ".wav"), "-O", csv)
        assert same_file(csv, "chroma_fft_%s.csv" % stem)


@pytest.mark.parametrize("tag", sorted(EDITED))
def test_front_end_edited_conf_equals_the_binary(gold, tmp_path, tag):
    """--set chroma_fft -C edited.conf on the 1 s input: the file the binary wrote for the same edits of its own file"""
    from oracle import lldo
    text = MINIMAL
    for a, b in EDITED[tag]["minimal"].items():
        assert text.count(a) == 1, a
        text = text.replace(a, b)
    conf = tmp_path / "edited.conf"
    conf.write_text(text)
    pcm, fs = gold_pcm(gold, 6)
    wav, csv = str(tmp_path / "in.wav"), str(tmp_path / "e.csv")
    lldo.write_wav(wav, pcm, fs)
    run_exe("--set", "chroma_fft", "-C", str(conf), "-I", wav, "-O", csv)
    assert open(csv).read() == str(gold["csv_%s_6" % tag])
    assert str(gold["csv_%s_6" % tag]) != str(gold["csv_6"])
