"""config/chroma/chroma_filt.conf as a fused batch set (SMILEHIP_CHAIN_CHROMA_FILT) on the device: lld_tonefilt_scan (a lane per
(utterance, note) chain) and lld_chroma_rows behind it, and cTonefilt as a stream operator, held bit for bit to the real binary's
tonespec and chroma levels (tests/golden/make_golden_chroma_filt.py) one utterance at a time and as ragged batches, on the
hard-signal corpus and through the smilextract_hip front end. Tolerance for the two float levels everywhere: identical bits. The
double states are the device's own sine and cosine's: they are held to the host's within 4 D, D being what moving every libm result
by one ulp changes (measured by the fixture generator on the reference side; the factor 4 covers errors that are one-signed where the
perturbation's sign was random)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from helpers import tonefilt_host as H
from test_chroma_filt_host import EDITED, EDIT_INPUTS, GOLD, LONG, MINIMAL, N16, gold_pcm, kept_rows

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "opensmile_amd", "smilextract_hip")


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLD, "chroma_filt_synth.npz"))


@pytest.fixture(scope="module")
def hip():
    from opensmile_amd import capi
    ctx = capi.Context(0)
    plan = capi.Plan(ctx, capi.chroma_filt_config())
    g = plan.geometry
    assert (g.frame_size, g.frame_step, g.n_out) == (160, 160, 12)
    return capi, ctx, plan


def offsets(pcms):
    return np.concatenate([[0], np.cumsum([len(p) for p in pcms])]).astype(np.int64)


def check_against_gold(gold, ks, b, out, tap, suffix="%d", what=""):
    """rows, every cell and the tap (level tonespec) of the batch's utterances against the binary's"""
    from tolerance import assert_bits_equal
    f0 = 0
    for i, k in enumerate(ks):
        ref, ts = gold["chroma_" + suffix % k], gold["tonespec_" + suffix % k]
        T = int(gold["n_rows_" + suffix % k])
        assert b.frame_offsets[i + 1] - b.frame_offsets[i] == T, (k, T)
        if T:
            keep = kept_rows(gold, k, T)
            assert_bits_equal(tap[f0:f0 + T][keep], ts, "%slevel tonespec, input %d" % (what, k))
            assert_bits_equal(out[b.frame_offsets[i]:b.frame_offsets[i + 1]][keep], ref, "%slevel chroma, input %d" % (what, k))
        f0 += T
    assert f0 == b.total_frames == len(tap)


# ---------------------------------------------------------------------------------------------- 1. golden
@pytest.mark.parametrize("k", range(14))
def test_golden_one_utterance_at_a_time(hip, gold, k):
    """every input alone, at its own rate; the 60 s input (two waves, 480 000 steps each) is the one with large arguments"""
    capi, ctx, _ = hip
    pcm, fs = gold_pcm(gold, k)
    plan = capi.Plan(ctx, capi.chroma_filt_config(fs))
    b = capi.Batch(plan, offsets([pcm]))
    out, tap = b.chroma_run_host(pcm)
    check_against_gold(gold, [k], b, out, tap)
    b.close()


@pytest.mark.parametrize("ks", [[6, 1, 2, 0, 3, 5, 4], [0, 4, 3, 6, 1, 5, 2, 6, 0]], ids=["order-a", "order-b"])
def test_golden_ragged_batch(hip, gold, ks):
    """all 16 kHz inputs in ONE batch, the empty one and the P - 1 sample one between long ones: 72 chains per utterance put every
    utterance seam inside a wave, and the lanes of the short ones finish 100 blocks before their neighbours"""
    capi, ctx, plan = hip
    assert all(int(gold["inputs"][k][2]) == 16000 for k in ks) and sorted(set(ks)) == list(range(N16))
    assert sum(1 for r in gold["inputs"] if r[2] == 16000) == N16
    pcms = [gold_pcm(gold, k)[0] for k in ks]
    b = capi.Batch(plan, offsets(pcms))
    out, tap = b.chroma_run_host(np.concatenate(pcms))
    check_against_gold(gold, ks, b, out, tap)
    nz = (out != 0).any(axis=1)
    assert nz.any() and (~nz).any()                        # both branches of the silence flag
    b.close()


def test_float_input_rerun_and_ld_out(hip, gold):
    """smilehip_lld_run_f32 on the converted samples, twice over, into a wider matrix: the same rows, the padding untouched"""
    capi, ctx, plan = hip
    ks = [5, 6, 1, 3]
    pcms = [gold_pcm(gold, k)[0] for k in ks]
    b = capi.Batch(plan, offsets(pcms))
    out, tap = b.chroma_run_host(H.pcm_float(np.concatenate(pcms)), ld_out=16, fill=7.0, runs=2)
    assert (out[:, 12:] == 7.0).all()
    check_against_gold(gold, ks, b, out[:, :12], tap, what="float input: ")
    b.close()
    e = capi.Batch(plan, offsets([np.zeros(0, np.int16)] * 3))      # nothing but empty utterances
    out, tap = e.chroma_run_host(np.zeros(0, np.int16))
    assert out.shape == (0, 12) and e.total_frames == 0
    e.close()


@pytest.mark.parametrize("tag", sorted(EDITED))
def test_edited_parameters_equal_the_binary(hip, gold, tag):
    capi, ctx, _ = hip
    cfg = capi.chroma_filt_config()
    for f, v in EDITED[tag]["cfg"].items():
        setattr(cfg, f, v)
    plan = capi.Plan(ctx, cfg)
    ks = list(EDIT_INPUTS)
    pcms = [gold_pcm(gold, k)[0] for k in ks]
    b = capi.Batch(plan, offsets(pcms))
    out, tap = b.chroma_run_host(np.concatenate(pcms))
    check_against_gold(gold, ks, b, out, tap, suffix=tag + "_%d", what=tag + ": ")
    b.close()


def test_hard_signals(hip):
    from helpers import hard_signals
    from tolerance import assert_bits_equal
    capi, ctx, plan = hip
    h = np.load(os.path.join(GOLD, "hard_chroma_filt.npz"))
    sig = hard_signals.signals()
    names = list(sig)
    b = capi.Batch(plan, offsets([sig[n] for n in names]))
    out, tap = b.chroma_run_host(np.concatenate([sig[n] for n in names]))
    for i, n in enumerate(names):
        r0, r1 = b.frame_offsets[i], b.frame_offsets[i + 1]
        assert_bits_equal(tap[r0:r1], h["tonespec_" + n], "hard signal %s, level tonespec" % n)
        assert_bits_equal(out[r0:r1], h["chroma_" + n], "hard signal %s, level chroma" % n)
    b.close()


# ---------------------------------------------------------------------------------------------- 2. the operator
def op_rows(capi, ctx, x, fs, opts=None, per_call=None):
    """the operator on float samples x (a whole number of blocks): rows, and the state behind them"""
    op = capi.TonefiltOp(ctx, capi.tonefilt_opts(**dict(H.SHIPPED, **(opts or {}))), fs, len(x))
    P = op.block_len
    step = len(x) if per_call is None else per_call * P
    rows = [op.blocks_host(x[i:i + step]) for i in range(0, len(x), max(step, 1))]
    st = op.state()
    return (np.concatenate(rows) if rows else np.zeros((0, op.n_out), np.float32)), st, op


def test_operator_equals_the_chain_and_the_binary(hip, gold):
    """pcm16_to_float, tonefilt_op, chroma_op on an input's samples (the last block completed as the reader completes it): the chain's rows"""
    from tolerance import assert_bits_equal
    capi, ctx, plan = hip
    for k in (3, 6, 9):
        pcm, fs = gold_pcm(gold, k)
        x = H.pcm_float(H.padded(pcm, fs))
        ts, (pos, s, c), op = op_rows(capi, ctx, x, fs)
        assert pos == len(x) and op.n_out == 72 and op.block_len == H.block_len(fs)
        assert_bits_equal(ts, gold["tonespec_%d" % k], "operator, level tonespec, input %d" % k)
        op.close()


def test_operator_block_by_block_equals_all_at_once(hip, gold):
    """one block per call and everything in one call: the same rows and the same doubles; _reset gives a fresh operator's state"""
    capi, ctx, plan = hip
    pcm, fs = gold_pcm(gold, 6)
    x = H.pcm_float(pcm[:160 * 12])
    all_rows, (pos_a, s_a, c_a), op_a = op_rows(capi, ctx, x, fs)
    one_rows, (pos_b, s_b, c_b), op_b = op_rows(capi, ctx, x, fs, per_call=1)
    assert pos_a == pos_b == len(x) and all_rows.tobytes() == one_rows.tobytes()
    assert s_a.tobytes() == s_b.tobytes() and c_a.tobytes() == c_b.tobytes() and np.abs(s_a).max() > 0
    op_b.reset()
    pos, s, c = op_b.state()
    assert pos == 0 and not s.any() and not c.any()
    again = op_b.blocks_host(x)
    assert again.tobytes() == all_rows.tobytes() and op_b.state()[1].tobytes() == s_a.tobytes()
    L = capi.load()                                        # the stream may not run past what the operator was created for
    d = C.c_void_p(1)
    assert L.smilehip_tonefilt_op_blocks(op_b._h, d, 1, d, None) != 0 and b"sincos_d" in L.smilehip_last_error()
    op_a.close()
    op_b.close()


@pytest.mark.parametrize("k", [1, 2, 5, 6, 7, 8, 9, 10, 11, 12, LONG])
def test_device_states_within_4_D_of_the_host_s(hip, gold, k):
    """the device's double states against the g++ build's (libm): relative difference at most 4 D of that fixture; the count of
    states that differ at all is printed and recorded, not asserted"""
    from tolerance import record
    capi, ctx, plan = hip
    pcm, fs = gold_pcm(gold, k)
    x = H.pcm_float(H.padded(pcm, fs))
    ts, (pos, s, c), op = op_rows(capi, ctx, x, fs)
    op.close()
    dev, host = np.concatenate([s, c]), np.concatenate([gold["state_s_%d" % k], gold["state_c_%d" % k]])
    D = float(gold["D_%d" % k])
    nz = host != 0
    rel = np.abs(dev[nz] - host[nz]) / np.abs(host[nz])
    differing = int((dev != host).sum())
    print("input %d: %d of %d states differ from the host's, largest relative difference %.3g, D %.3g" % (k, differing, len(host), rel.max(), D))
    record("chroma_filt_states", input=k, differing=differing, states=len(host), rel_max=float(rel.max()), D=D)
    assert (dev[~nz] == 0).all() and D > 0
    assert rel.max() <= 4 * D, (k, rel.max(), D)


def test_domain_overrun_is_refused(hip):
    """an utterance (a stream) long enough to carry 2 pi freq[71] t past 2^30: SMILEHIP_ERR_INVALID naming sincos_d's domain"""
    capi, ctx, plan = hip
    L = capi.load()
    w = H.tables(16000)["w"][-1]
    n_ok = int(2.0 ** 30 / w * 16000) // 160 * 160 - 160
    n_bad = n_ok + 2 * 160
    h = C.c_void_p()
    off = (C.c_int64 * 3)(0, 100, 100 + n_bad)
    rc = L.smilehip_batch_create(plan._h, off, 2, C.byref(h))
    assert rc == -1                                        # SMILEHIP_ERR_INVALID
    assert b"domain of sincos_d" in L.smilehip_last_error() and str(n_bad).encode() in L.smilehip_last_error()
    o = capi.tonefilt_opts()
    assert L.smilehip_tonefilt_op_create(ctx._h, C.byref(o), 16000.0, n_bad, C.byref(h)) != 0 and b"domain of sincos_d" in L.smilehip_last_error()
    op = capi.TonefiltOp(ctx, o, 16000.0, n_ok)            # the longest stream inside the domain is accepted
    op.close()
    o = capi.tonefilt_opts(first_note=55.0 * 2 ** 20)      # ... and a higher firstNote shortens it
    assert L.smilehip_tonefilt_op_create(ctx._h, C.byref(o), 16000.0, n_ok // 1000, C.byref(h)) != 0 and b"domain of sincos_d" in L.smilehip_last_error()


# ---------------------------------------------------------------------------------------------- 3. chroma_fft is what it was
@pytest.mark.parametrize("size", ["V2", "full"])
def test_chroma_fft_chain_through_both_struct_sizes(size):
    """SMILEHIP_CHAIN_CHROMA_FFT batches give the bits they gave, through the V2-sized struct its preset fills and through a full-sized one"""
    from opensmile_amd import capi
    from tolerance import assert_bits_equal
    import test_chroma_fft_host as F
    g = np.load(os.path.join(GOLD, "chroma_fft_synth.npz"))
    ctx = capi.Context(0)
    if size == "V2":
        cfg = capi.chroma_fft_config()
        assert cfg.struct_size == capi.LLD_CONFIG_SIZE_V2
    else:
        cfg = capi.LldConfigChromaFilt()
        capi.load().smilehip_config_chroma_fft(C.cast(C.byref(cfg), C.POINTER(capi.LldConfigChroma)), 16000.0)
        cfg.struct_size = C.sizeof(cfg)
    plan = capi.Plan(ctx, cfg)
    ks = [5, 6]
    pcms = [F.gold_pcm(g, k)[0] for k in ks]
    b = capi.Batch(plan, offsets(pcms))
    out, tap = b.chroma_run_host(np.concatenate(pcms))
    f0 = 0
    for i, k in enumerate(ks):
        T = len(g["chroma_%d" % k])
        assert_bits_equal(tap[f0:f0 + T], g["tonespec_%d" % k], "chroma_fft, %s struct, level tonespec, input %d" % (size, k))
        assert_bits_equal(out[b.frame_offsets[i]:b.frame_offsets[i + 1]], g["chroma_%d" % k], "chroma_fft, %s struct, level chroma, input %d" % (size, k))
        f0 += T
    b.close()


# ---------------------------------------------------------------------------------------------- 4. the front end
def run_exe(*args):
    p = subprocess.run([EXE, *args], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]


def same_file(path, name):
    return open(path, "rb").read() == open(os.path.join(GOLD, "files", name), "rb").read()


@pytest.mark.parametrize("stem", ["u2_8000", "u3_4000"])
def test_front_end_set_writes_the_binary_s_file(tmp_path, stem):
    wav = os.path.join(GOLD, "files", stem + ".wav")
    csv = str(tmp_path / "o.csv")
    run_exe("--set", "chroma_filt", "-I", wav, "-O", csv)
    assert same_file(csv, "chroma_filt_%s.csv" % stem)


def test_front_end_csvoutput_has_header_and_time_stamps(tmp_path, gold):
    """-csvoutput: the other sets' CSV file (name, frameTime, header) with the same values, names and times as a header-printing copy"""
    wav = os.path.join(GOLD, "files", "u2_8000.wav")
    csv, plain = str(tmp_path / "o.csv"), str(tmp_path / "p.csv")
    run_exe("--set", "chroma_filt", "-I", wav, "-O", plain, "-csvoutput", csv, "-instname", "u2")
    assert same_file(plain, "chroma_filt_u2_8000.csv")
    lines = open(csv).read().splitlines()
    want = open(plain).read().splitlines()
    copy = str(gold["csv_header_copy"]).splitlines()
    assert lines[0] == "name;" + copy[0] and len(lines) == len(want) + 1
    assert [ln.split(";")[1] for ln in lines[1:len(copy)]] == [ln.split(";")[0] for ln in copy[1:]]
    assert [ln.split(";", 2)[2] for ln in lines[1:]] == want


def test_front_end_conf_file_and_filelist(tmp_path):
    """--set chroma_filt -C: the graph in its own wording runs as the set and writes the binary's files, here through a file list"""
    conf = tmp_path / "c.conf"
    conf.write_text(MINIMAL)
    lst = tmp_path / "list.txt"
    lst.write_text("".join(os.path.join(GOLD, "files", s + ".wav") + "\n" for s in ("u2_8000", "u3_4000")))
    out = tmp_path / "out"
    out.mkdir()
    run_exe("--set", "chroma_filt", "-C", str(conf), "-filelist", str(lst), "-outdir", str(out), "-O", "x")
    for s in ("u2_8000", "u3_4000"):
        assert same_file(out / (s + ".csv"), "chroma_filt_%s.csv" % s)


@pytest.mark.parametrize("tag", sorted(EDITED))
def test_front_end_edited_conf_equals_the_binary(gold, tmp_path, tag):
    """--set chroma_filt -C edited.conf on the 1 s input: the file the binary wrote for the same edits of its own file"""
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
    run_exe("--set", "chroma_filt", "-C", str(conf), "-I", wav, "-O", csv)
    assert open(csv).read() == str(gold["csv_%s_6" % tag])
    assert str(gold["csv_%s_6" % tag]) != str(gold["csv_6"])
