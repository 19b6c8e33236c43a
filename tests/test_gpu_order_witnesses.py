"""cSpectral on the spectra of tests/golden/order_witnesses.npz, where the ORDER of the double additions decides a float of the
output (built by tests/golden/make_golden_order_witnesses.py, held on the host by tests/test_order_witnesses_host.py).

Through the C ABI, at most 64 frames with K <= 513 per call (the flux state carried from call to call as
tests/helpers/op_layouts.py does): smilehip_spectral_frames at K = 257 (the block form, spectral_frame), 129 and 513
(spectral_frame_wave<2> / <8>, the fused ComParE wave kernel's template), smilehip_spectral_gemaps_frames (gemaps_spectral_wave)
and smilehip_spectral_op_frames with the ComParE option set (one thread per frame, the reference's chains).

Two classes of columns:
  sequence-decided   roll-off x 4, centroid, skewness, slope, sharpness, harmonicity; the GeMAPS slopes, alpha ratio, Hammarberg
                     index: a cancellation, a threshold or a float chain -- another order moves them by more than rounding, so the
                     kernels add in the reference's order and must equal the oracle bit for bit on EVERY row
  one-signed         band energies, flux, entropy, variance, kurtosis, GeMAPS flux: double sums of non-negative terms kept as trees.
                     Tree and chain differ by at most K 2^-53 relative (each of the < K additions of either order rounds by at most
                     2^-53 of a partial sum that is at most the total), far below the float's 2^-24: the two floats are equal or
                     adjacent. Bit-equal on the plain rows, within one float ulp everywhere, and -- the arithmetic-only ones -- equal
                     to the kernel-order model's bits, which shows that the whole deviation is the documented order."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_golden_order_witnesses as gen                     # noqa: E402

so = gen.so
f32 = np.float32
SHARPNESS, HARMONICITY, ENTROPY = 13, 14, 8
SEQUENCE_COLUMNS = [so.COLUMN_INDEX[c] for c in so.SEQUENCE_DECIDED] + [SHARPNESS, HARMONICITY]
ONE_SIGNED_COLUMNS = [so.COLUMN_INDEX[c] for c in so.ONE_SIGNED] + [ENTROPY]
NAMES = {v: k for k, v in so.COLUMN_INDEX.items()} | {SHARPNESS: "sharpness", HARMONICITY: "harmonicity", ENTROPY: "entropy"}
CALL = 64                                                    # frames per call


@pytest.fixture(scope="module")
def env():
    from helpers import op_layouts as OL
    return OL.Env()


@pytest.fixture(scope="module")
def corpus():
    return np.load(gen.OUT)


def run_stream(env, fn, plan, rows, n_out):
    """the rows of one stream through fn in calls of at most CALL frames; NaN behind every row's outputs must stay"""
    torch, L = env.torch, env.L
    n, K = rows.shape
    d_src = env.dev(rows)
    d_dst = torch.full((n, n_out + 1), float("nan"), dtype=torch.float32, device="cuda")
    d_state = torch.full((K,), float("nan"), dtype=torch.float32, device="cuda")
    for t in range(0, n, CALL):
        m = min(CALL, n - t)
        env.check(getattr(L, fn)(env.plan(plan)._h, d_src[t:].data_ptr(), K, d_state.data_ptr(), 1 if t == 0 else 0,
                                 d_dst[t:].data_ptr(), n_out + 1, m, None))
    env.sync()
    got = d_dst.cpu().numpy()
    assert np.isnan(got[:, n_out]).all()
    return np.ascontiguousarray(got[:, :n_out])


def run_op(env, rows, fss):
    """smilehip_spectral_op_* with the ComParE option set"""
    import ctypes as C
    from helpers import op_layouts as OL
    torch, L, capi = env.torch, env.L, env.capi
    n, K = rows.shape
    o = capi.spectral_opts(list(OL.COMPARE_BANDS), so.ROLLOFF, [], **OL.COMPARE_FLAGS)
    op = C.c_void_p()
    capi._check(L.smilehip_spectral_op_create(env.h, C.byref(o), K, fss, C.byref(op)))
    try:
        assert L.smilehip_spectral_op_n_out(op) == 15
        d_src = env.dev(rows)
        d_dst = torch.full((n, 16), float("nan"), dtype=torch.float32, device="cuda")
        d_state = torch.full((K,), float("nan"), dtype=torch.float32, device="cuda")
        for t in range(0, n, CALL):
            env.check(L.smilehip_spectral_op_frames(op, d_src[t:].data_ptr(), K, d_state.data_ptr(), 1 if t == 0 else 0,
                                                    d_dst[t:].data_ptr(), 16, min(CALL, n - t), None))
        env.sync()
        got = d_dst.cpu().numpy()
    finally:
        capi._check(L.smilehip_spectral_op_destroy(op))
    assert np.isnan(got[:, 15]).all()
    return np.ascontiguousarray(got[:, :15])


_kept = {}


def compare_case(env, corpus, K):
    """(rows, family, oracle rows, device rows) of one K, computed once for the module"""
    if K not in _kept:
        from helpers import op_layouts as OL
        rows = corpus[f"rows_{K}"]
        ref = OL.ref_spectral_compare(rows, gen.fss_of(K))
        ref.setflags(write=False)
        got = run_stream(env, "smilehip_spectral_frames", f"spectral{K}", rows, 15)
        _kept[K] = (rows, corpus[f"family_{K}"], ref, got)
    return _kept[K]


def gemaps_case(env, corpus, oracle):
    if "gemaps" not in _kept:
        rows = corpus["gemaps_rows"]
        ref = oracle.egemaps_spectral_rows(rows)
        ref.setflags(write=False)
        _kept["gemaps"] = (rows, corpus["gemaps_family"], ref, run_stream(env, "smilehip_spectral_gemaps_frames", "egemaps", rows, 5))
    return _kept["gemaps"]


def misses(got, ref, columns, names):
    """{column name: rows that differ} over `columns`"""
    d = so.differ(got, ref)
    return {names[c]: np.flatnonzero(d[:, c]).tolist() for c in columns if d[:, c].any()}


def ulps(a, b):
    """distance in float steps (finite values of one sign, or zeros)"""
    a, b = np.ascontiguousarray(a, f32), np.ascontiguousarray(b, f32)
    assert np.isfinite(a).all() and np.isfinite(b).all() and ((a >= 0) == (b >= 0)).all()
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64)) * ~((a == 0) & (b == 0))


@pytest.mark.parametrize("K", gen.KS)
def test_sequence_decided_columns_equal_the_oracle(env, corpus, oracle, K):
    rows, fam, ref, got = compare_case(env, corpus, K)
    bad = misses(got, ref, SEQUENCE_COLUMNS, NAMES)
    print(f"K={K}: {len(rows)} rows, cells off the oracle per sequence-decided column: { {k: len(v) for k, v in bad.items()} }")
    assert not bad, f"K={K}: rows off the oracle, per column: {bad}"


@pytest.mark.parametrize("K", gen.KS)
def test_one_signed_columns(env, corpus, oracle, K):
    rows, fam, ref, got = compare_case(env, corpus, K)
    bad = misses(got[fam == gen.PLAIN], ref[fam == gen.PLAIN], ONE_SIGNED_COLUMNS, NAMES)
    assert not bad, f"K={K}: plain rows off the oracle: {bad}"
    u = ulps(got[:, ONE_SIGNED_COLUMNS], ref[:, ONE_SIGNED_COLUMNS])
    print(f"K={K}: one-signed cells one ulp off the oracle, per column: "
          f"{ {NAMES[c]: int((u[:, i] == 1).sum()) for i, c in enumerate(ONE_SIGNED_COLUMNS)} }, largest distance {int(u.max())} ulp")
    assert u.max() <= 1, f"K={K}: {np.argwhere(u > 1)[:6].tolist()}"
    # the arithmetic-only ones ARE the documented order: the kernels' tree on the reference's centroid and frame sum
    model, _ = so.stream_columns(rows, gen.fss_of(K), so.device_order(K), chains=True)
    arith = [c for c in so.ONE_SIGNED]
    d = so.differ(got[:, [so.COLUMN_INDEX[c] for c in arith]], model[:, [gen.COL[c] for c in arith]])
    assert not d.any(), f"K={K}: off the kernel-order model: { {arith[c]: np.flatnonzero(d[:, c]).tolist() for c in range(len(arith)) if d[:, c].any()} }"
    # ... and the corpus bites: on the rows steered for a column the tree's float is NOT the oracle's
    for c in arith:
        tgt = corpus[f"target_{K}"] == gen.COL[c]
        assert so.differ(got[tgt, so.COLUMN_INDEX[c]], ref[tgt, so.COLUMN_INDEX[c]]).sum() >= 4, c


def test_gemaps_operator(env, corpus, oracle):
    rows, fam, ref, got = gemaps_case(env, corpus, oracle)
    names = {0: "slope0-500", 1: "slope500-1500", 2: "alphaRatio", 3: "hammarbergIndex", 4: "flux"}
    bad = misses(got, ref, [0, 1, 2, 3], names)
    print(f"GeMAPS: {len(rows)} rows, cells off the oracle per sequence-decided column: { {k: len(v) for k, v in bad.items()} }")
    assert not bad, f"rows off the oracle, per column: {bad}"
    assert not so.differ(got[fam == gen.PLAIN, 4], ref[fam == gen.PLAIN, 4]).any()
    assert ulps(got[:, 4], ref[:, 4]).max() <= 1


@pytest.mark.parametrize("K", gen.KS)
def test_operator_with_the_references_chains_equals_the_oracle(env, corpus, oracle, K):
    """smilehip_spectral_op_frames, one thread per frame, every sum the reference's chain: all fifteen columns bit for bit (entropy
    too, as tests/test_gpu_spectral_axis.py holds it) -- and no fused multiply-add, which these rows would show"""
    rows, fam, ref, _ = compare_case(env, corpus, K)
    got = run_op(env, rows, gen.fss_of(K))
    bad = misses(got, ref, range(15), NAMES | {i: f"col{i}" for i in range(15) if i not in NAMES})
    assert not bad, f"K={K}: rows off the oracle, per column: {bad}"
