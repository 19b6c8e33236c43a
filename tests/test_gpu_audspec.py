"""config/audspec/audspec.conf as SMILEHIP_CHAIN_AUDSPEC on the device: every cell and every row count equal the real binary's
(tests/golden/audspec_synth.npz, hard_audspec.npz, files/audspec_*), in both forms of lld_audspec_frame, for int16 and float samples,
through the plan, against the library's own per-component operators and through the front end."""
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import audspec_host as AH

pytestmark = pytest.mark.gpu
ROOT = AH.ROOT
GOLD = AH.GOLDEN
EXE = os.path.join(ROOT, "opensmile_amd", "smilextract_hip")
REF_CONF = os.path.join(ROOT, "oracle", "_ref", "config", "audspec")
WAVE_FRAMES = 4                                            # frames per workgroup of the wave form (lld_audspec.hip: kAudWaves)
WG_PER_CU_MAX = 4                                          # ... and its workgroups per CU at most (audspec_wave_grid_cap: 16 / kAudWaves)
# the ragged 16 kHz batch (fixture inputs): one second, 0 samples, T = 128, 399 samples, T = 1, T = 257, T = 2, 3, T = 129, T = 5, 16, 17, one second
RAGGED = [13, 0, 10, 1, 2, 12, 4, 5, 11, 6, 7, 8, 13]


@pytest.fixture(scope="module")
def gold():
    return AH.fixture()


@pytest.fixture(scope="module")
def hip():
    from opensmile_amd import capi
    ctx = capi.Context(0)
    plan = capi.Plan(ctx, capi.audspec_config())
    g = plan.geometry
    assert (g.frame_size, g.frame_step, g.fft_size, g.n_bins, g.n_static, g.n_out) == (400, 160, 512, 257, 26, 78)
    return capi, ctx, plan


def offsets(pcms):
    return np.concatenate([[0], np.cumsum([len(p) for p in pcms])]).astype(np.int64)


def as_f32(pcm):
    return (np.asarray(pcm).astype(np.float32) / np.float32(32767.0)).astype(np.float32)


def check_batch(gold, ks, b, out, suffix="%d", what=""):
    """rows and every cell of the batch's utterances against the binary's"""
    from tolerance import assert_bits_equal
    for i, k in enumerate(ks):
        ref = gold["lld_" + suffix % k]
        assert b.frame_offsets[i + 1] - b.frame_offsets[i] == len(ref), (k, len(ref))
        if len(ref):
            assert_bits_equal(out[b.frame_offsets[i]:b.frame_offsets[i + 1]], ref, "%slevel lld, input %d" % (what, k))
    assert b.total_rows == sum(len(gold["lld_" + suffix % k]) for k in ks)


def run_inputs(capi, ctx, cfg, gold, ks, suffix="%d", f32=False, what=""):
    plan = capi.Plan(ctx, cfg)
    pcms = [AH.input_pcm(k)[0] for k in ks]
    b = capi.Batch(plan, offsets(pcms))
    x = np.concatenate(pcms)
    out = b.audspec_run_host(as_f32(x) if f32 else x, fill=np.nan)
    check_batch(gold, ks, b, out, suffix, what)
    n_fft = plan.geometry.fft_size
    plan.close()
    return n_fft


# ---------------------------------------------------------------------------------------------- 1. golden
def test_golden_ragged_batch(hip, gold):
    capi, ctx, plan = hip
    assert [len(gold["lld_%d" % k]) for k in RAGGED] == [98, 0, 128, 0, 1, 257, 2, 3, 129, 5, 16, 17, 98]
    pcms = [AH.input_pcm(k)[0] for k in RAGGED]
    b = capi.Batch(plan, offsets(pcms))
    x = np.concatenate(pcms)
    out = b.run_host(x)                                     # smilehip_lld_run_host serves the chain
    check_batch(gold, RAGGED, b, out)
    for f32 in (False, True):                               # poisoned output, twice over: every cell is written by every run
        o2 = b.audspec_run_host(as_f32(x) if f32 else x, fill=np.nan, runs=2)
        check_batch(gold, RAGGED, b, o2, what="float input, " if f32 else "")
    o3 = b.audspec_run_host(x, ld_out=83, fill=-7.0)        # a wider matrix: the columns behind the 78 keep what they held
    check_batch(gold, RAGGED, b, o3[:, :78])
    assert (o3[:, 78:] == -7.0).all()


@pytest.mark.parametrize("fs", [8000, 11025, 22050, 32000, 44100, 48000])
@pytest.mark.parametrize("f32", [False, True])
def test_golden_other_rates(gold, fs, f32):
    from opensmile_amd import capi
    ctx = capi.Context(0)
    ks = [k for k, r in enumerate(gold["inputs"]) if int(r[2]) == fs]
    assert run_inputs(capi, ctx, capi.audspec_config(fs), gold, ks, f32=f32) == AH.NFFT[fs]
    assert run_inputs(capi, ctx, capi.audspec_config(fs, compat=True), gold, ks, "compat_%d", f32=f32) == AH.NFFT[fs]


def test_compat_at_16k(hip, gold):
    capi, ctx, _ = hip
    ks = [5, 6, 7, 8, 9, 13]
    for f32 in (False, True):
        assert run_inputs(capi, ctx, capi.audspec_config(16000.0, compat=True), gold, ks, "compat_%d", f32=f32) == 512


CHILD = r"""
import os, sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import numpy as np
import test_gpu_audspec as T
from helpers import audspec_host as AH
from opensmile_amd import capi
gold = AH.fixture()
ctx = capi.Context(0)
T.run_inputs(capi, ctx, capi.audspec_config(), gold, T.RAGGED)
T.run_inputs(capi, ctx, capi.audspec_config(), gold, T.RAGGED, f32=True)
T.run_inputs(capi, ctx, capi.audspec_config(16000.0, compat=True), gold, [5, 6, 7, 8, 9, 13], "compat_%%d")
T.run_inputs(capi, ctx, capi.audspec_config(32000.0), gold, [19])
print("CHILD OK", os.environ.get("SMILEHIP_AUDSPEC"))
"""


def test_workgroup_form_equals_the_binary():
    """SMILEHIP_AUDSPEC=block: the workgroup-per-frame form where the wave form would run (512 / 1024 points), in a fresh process"""
    env = dict(os.environ, SMILEHIP_AUDSPEC="block")
    r = subprocess.run([sys.executable, "-c", CHILD % (ROOT, os.path.join(ROOT, "tests"))], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "CHILD OK block" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


@pytest.mark.parametrize("tag", sorted(AH.EDITS))
def test_edited_parameters_equal_the_binary(hip, gold, tag):
    capi, ctx, _ = hip
    for f32 in (False, True):
        run_inputs(capi, ctx, AH.config(16000.0, **AH.EDITS[tag]), gold, list(AH.EDIT_INPUTS), tag + "_%d", f32=f32, what=tag + ": ")


# ---------------------------------------------------------------------------------------------- 2. seams, the grid's second trip
def test_persistent_grid_takes_a_second_trip(hip, gold):
    """more frames than the wave form's grid holds at once (its cap times four frames): copies of the one-second input with short ones
    between; every copy's rows equal the single-utterance run's, which equal the binary's"""
    import torch
    from tolerance import assert_bits_equal
    capi, ctx, plan = hip
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    at_once = cus * WG_PER_CU_MAX * WAVE_FRAMES
    one, two, five = AH.input_pcm(13)[0], AH.input_pcm(4)[0], AH.input_pcm(6)[0]
    copies = at_once // 98 + 8
    pcms = []
    for i in range(copies):
        pcms += [one, (two, five, np.zeros(0, np.int16))[i % 3]]
    b = capi.Batch(plan, offsets(pcms))
    assert b.total_frames > at_once + 98
    out = b.audspec_run_host(np.concatenate(pcms), fill=np.nan)
    refs = {98: gold["lld_13"], 2: gold["lld_4"], 5: gold["lld_6"]}
    for i in range(len(pcms)):
        o = out[b.frame_offsets[i]:b.frame_offsets[i + 1]]
        if len(o):
            assert_bits_equal(o, refs[len(o)], "utterance %d of the long batch" % i)
    assert [int(b.frame_offsets[i + 1] - b.frame_offsets[i]) for i in range(6)] == [98, 2, 98, 5, 98, 0]


# ---------------------------------------------------------------------------------------------- 3. the library's own operators
def per_component(capi, ctx, plan, cfg, pcm):
    """the chain out of the operators, one launch each over all frames of one utterance"""
    import torch
    g = plan.geometry
    N, H, K, Nfft, nb = g.frame_size, g.frame_step, g.n_bins, g.fft_size, g.n_static
    T = (len(pcm) - N) // H + 1
    x = as_f32(pcm)
    d_fr = torch.from_numpy(np.stack([x[t * H:t * H + N] for t in range(T)])).cuda()
    d_pe, d_w = torch.zeros((T, N), device="cuda"), torch.zeros((T, N), device="cuda")
    d_c, d_m = torch.zeros((T, Nfft), device="cuda"), torch.zeros((T, K), device="cuda")
    d_mel, d_aud = torch.zeros((T, nb), device="cuda"), torch.zeros((T, nb), device="cuda")
    capi.preemphasis_frames(ctx, d_fr.data_ptr(), N, d_pe.data_ptr(), N, T, N, float(cfg.preemph_k), int(cfg.preemph_de))
    capi.window_frames(plan, d_pe.data_ptr(), N, d_w.data_ptr(), N, T)
    capi.rfft_frames(plan, d_w.data_ptr(), N, d_c.data_ptr(), Nfft, T)
    capi.fftmag_frames(plan, d_c.data_ptr(), Nfft, d_m.data_ptr(), K, T)
    capi.melspec_frames(plan, d_m.data_ptr(), K, d_mel.data_ptr(), nb, T)
    d_eql = torch.from_numpy(AH.geometry(cfg)[5]).cuda()
    capi._check(capi.load().smilehip_plp_audspec_frames(ctx._h, d_mel.data_ptr(), nb, nb, d_eql.data_ptr(), 1.0, float(cfg.plp_compression), 0, None, None,
                                                        d_aud.data_ptr(), nb, T, None))
    d_io = torch.zeros((T, 3 * nb), device="cuda")
    d_io[:, :nb] = d_aud
    b = capi.Batch(plan, np.array([0, len(pcm)], np.int64))
    capi.delta_chain(plan, b, d_io.data_ptr(), 3 * nb, nb, int(cfg.delta_win), 2)
    torch.cuda.synchronize()
    return d_io.cpu().numpy()


@pytest.mark.parametrize("fs", [16000, 44100])
def test_fused_equals_per_component_operators(fs):
    """a seeded signal on which no fixture exists, once per kernel form"""
    from tolerance import assert_bits_equal
    from opensmile_amd import capi, synth
    ctx = capi.Context(0)
    cfg = capi.audspec_config(float(fs))
    plan = capi.Plan(ctx, cfg)
    pcm = (synth.utterance(31, fs).astype(np.int32) // 3).astype(np.int16)
    b = capi.Batch(plan, np.array([0, len(pcm)], np.int64))
    fused = b.audspec_run_host(pcm, fill=np.nan)
    ref = per_component(capi, ctx, plan, cfg, pcm)
    assert np.isfinite(ref).all() and (ref[:, :26] > 0).all()
    assert_bits_equal(fused, ref, "level lld at %d Hz" % fs)
    plan.close()


# ---------------------------------------------------------------------------------------------- 4. hard signals
def test_hard_signals(hip):
    from tolerance import assert_bits_equal
    from helpers import hard_signals
    capi, ctx, plan = hip
    ref = AH.fixture("hard_audspec.npz")
    pcm = hard_signals.signals()
    sig = [np.ascontiguousarray(pcm[n], np.int16) for n in hard_signals.NAMES]
    b = capi.Batch(plan, offsets(sig))
    out = b.audspec_run_host(np.concatenate(sig), fill=np.nan)
    for i, n in enumerate(hard_signals.NAMES):
        assert_bits_equal(out[b.frame_offsets[i]:b.frame_offsets[i + 1]], ref["lld_" + n], "hard signal " + n)


# ---------------------------------------------------------------------------------------------- 5. the front end
needs_exe = pytest.mark.skipif(not os.path.exists(EXE), reason="smilextract_hip not built")


def smilextract(*args):
    p = subprocess.run([EXE, *args], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    return p


def read(path):
    with open(path, "rb") as f:
        return f.read()


@needs_exe
@pytest.mark.parametrize("stem", ["u2_8000", "u3_4000"])
def test_front_end_sets_write_the_binarys_files(tmp_path, stem):
    wav = os.path.join(GOLD, "files", stem + ".wav")
    htk, csv = str(tmp_path / "o.htk"), str(tmp_path / "o.csv")
    smilextract("--set", "audspec", "-I", wav, "-O", htk, "-csvoutput", csv)
    assert read(htk) == read(os.path.join(GOLD, "files", "audspec_%s.htk" % stem))
    assert read(csv) == read(os.path.join(GOLD, "files", "audspec_%s.csv" % stem))
    htk2 = str(tmp_path / "c.htk")
    smilextract("--set", "audspec_compat", "-I", wav, "-O", htk2)
    assert read(htk2) == read(os.path.join(GOLD, "files", "audspec_compat_%s.htk" % stem)) and read(htk2) != read(htk)


@needs_exe
@pytest.mark.skipif(not os.path.isdir(REF_CONF), reason="the reference's configuration files are not here")
@pytest.mark.parametrize("name", ["audspec", "audspec_compat"])
def test_front_end_shipped_conf_files(tmp_path, name):
    for stem in ("u2_8000", "u3_4000"):
        wav = os.path.join(GOLD, "files", stem + ".wav")
        htk, csv = str(tmp_path / (stem + ".htk")), str(tmp_path / (stem + ".csv"))
        smilextract("--set", name, "-C", os.path.join(REF_CONF, name + ".conf"), "-I", wav, "-O", htk, "-csvoutput", csv)
        assert read(htk) == read(os.path.join(GOLD, "files", "%s_%s.htk" % (name, stem)))
        if name == "audspec":
            assert read(csv) == read(os.path.join(GOLD, "files", "audspec_%s.csv" % stem))


@needs_exe
def test_front_end_minimal_text_and_an_edit(tmp_path, gold):
    """the project's own configuration text, as it is and with nBands = 20: the HTK file's rows are the binary's"""
    from oracle import lldo
    for tag, edits in (("", None), ("nb20", AH.TEXT_EDITS["nb20"])):
        conf = tmp_path / ("m%s.conf" % tag)
        conf.write_text(AH.minimal_text(edits))
        pcm, fs = AH.input_pcm(9)
        wav, htk = str(tmp_path / "in.wav"), str(tmp_path / ("o%s.htk" % tag))
        lldo.write_wav(wav, pcm, fs)
        smilextract("--set", "audspec", "-C", str(conf), "-I", wav, "-O", htk)
        rows, period, kind = lldo.read_htk(htk)
        ref = gold["lld_%s9" % (tag + "_" if tag else "")]
        assert (period, kind) == (100000, 9) and rows.shape == ref.shape and rows.tobytes() == ref.tobytes()
