"""tests/golden/order_witnesses.npz on the host: the file is what its generator writes, the sequential model of
tests/helpers/sum_orders.py IS the oracle's arithmetic on every committed row (bit for bit -- the oracle is pinned on the real
binary, so the model's term formation is too), every column has its witnesses, and the witnesses pin the kernels' OWN tree:
another tree (neighbours first) gives other floats on them."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_golden_order_witnesses as gen                     # noqa: E402

so = gen.so
f32 = np.float32
COL = gen.COL
CANCELLING_COLUMNS = ("ro25", "ro50", "ro75", "ro90", "slope")
STEERED_COLUMNS = ("band0", "band1", "flux", "centroid", "variance", "kurtosis")


@pytest.fixture(scope="module")
def corpus():
    return np.load(gen.OUT)


def witness_matrix(rows, K):
    """[n x columns] bool: the tree order smilehip_spectral_frames runs at K against the reference's, frame by frame of the stream;
    sequence-decided columns with every sum in the tree (what the kernels did before they followed the reference there), one-signed
    columns with the kernels as they stand"""
    fss = gen.fss_of(K)
    seq, _ = so.stream_columns(rows, fss, "seq")
    tree, amb = so.stream_columns(rows, fss, so.device_order(K), chains=False)
    mixed, _ = so.stream_columns(rows, fss, so.device_order(K), chains=True)
    w = so.differ(tree, seq)
    for c in so.ONE_SIGNED:
        w[:, COL[c]] = so.differ(mixed, seq)[:, COL[c]]
    return w, amb


def test_file_is_small_and_holds_magnitudes_only(corpus):
    assert os.path.getsize(gen.OUT) < 512 * 1024
    for K in gen.KS:
        r = corpus[f"rows_{K}"]
        assert r.dtype == f32 and r.shape[1] == K and np.isfinite(r).all() and (r >= 0).all()
        assert len(r) == len(corpus[f"family_{K}"]) == len(corpus[f"target_{K}"])
    assert corpus["gemaps_rows"].shape[1] == gen.GK


def test_regenerating_a_subset_reproduces_the_committed_bytes(corpus):
    """all of K = 129: every ComParE set, numpy only (the GeMAPS rows are steered through the C library's logf: `--check` of the
    generator compares the whole file)"""
    a = gen.build(ks=(129,), gemaps=False)
    for k, v in a.items():
        assert v.dtype == corpus[k].dtype and v.tobytes() == corpus[k].tobytes(), k


@pytest.mark.parametrize("K", gen.KS)
def test_sequential_model_is_the_oracle(corpus, oracle, K):
    from helpers import op_layouts as OL
    rows = corpus[f"rows_{K}"]
    ref = OL.ref_spectral_compare(rows, gen.fss_of(K))
    got, amb = so.stream_columns(rows, gen.fss_of(K), "seq")
    assert not amb.any()
    d = so.differ(got, ref[:, so.MODELLED])
    assert not d.any(), f"K={K}: columns {[so.COLUMNS[c] for c in sorted(set(np.argwhere(d)[:, 1]))]} rows {sorted(set(np.argwhere(d)[:, 0]))[:8]}"


def test_sequential_gemaps_model_is_the_oracle(corpus, oracle):
    rows = corpus["gemaps_rows"]
    ref = oracle.egemaps_spectral_rows(rows)
    got = so.gemaps_slopes(gen.log_spectrum(rows), gen.GFSS, "seq")
    assert not so.differ(got, ref[:, :2]).any()


@pytest.mark.parametrize("K", gen.KS)
def test_witness_counts(corpus, K):
    rows, fam, tgt = corpus[f"rows_{K}"], corpus[f"family_{K}"], corpus[f"target_{K}"]
    w, amb = witness_matrix(rows, K)
    assert not amb[fam == gen.CANCELLING].any(), "a cancelling row whose tree prefix names two roll-off bins"
    counts = {}
    for c in CANCELLING_COLUMNS:
        counts[c] = int(w[fam == gen.CANCELLING, COL[c]].sum())
        assert counts[c] >= 8, (K, c, counts[c])
    for c in STEERED_COLUMNS:
        counts[c] = int(w[(fam == gen.STEERED) & (tgt == COL[c]), COL[c]].sum())
        assert counts[c] >= 4, (K, c, counts[c])
    # skewness moves with the centroid: the centroid's witnesses are its own
    sk = w[(fam == gen.STEERED) & (tgt == COL["centroid"]), COL["skewness"]].sum()
    assert sk >= 4, (K, "skewness", int(sk))
    # controls: on the plain rows no order matters
    assert not w[fam == gen.PLAIN].any(), np.argwhere(w & (fam == gen.PLAIN)[:, None])[:6]
    print(f"K={K}: witnesses {counts}, skewness {int(sk)}")


def test_gemaps_witness_counts(corpus):
    rows, fam, tgt = corpus["gemaps_rows"], corpus["gemaps_family"], corpus["gemaps_target"]
    lg = gen.log_spectrum(rows)
    w = so.differ(so.gemaps_slopes(lg, gen.GFSS, "waveg"), so.gemaps_slopes(lg, gen.GFSS, "seq"))
    for b in (0, 1):
        assert int(w[(fam == gen.CANCELLING) & (tgt == b), b].sum()) >= 8, (b, w[:, b].sum())
        # ... and they cancel: Nind sumA - Sf sumB is at most 2^-26 of Nind sumA
        for r in rows[(fam == gen.CANCELLING) & (tgt == b)]:
            ctx = {}
            V, _ = gen.gemaps_numerator(b, r, ctx)
            assert abs(V) * 2 ** 26 <= ctx["scale"]
    assert not w[fam == gen.PLAIN].any()


@pytest.mark.parametrize("K", gen.KS)
def test_another_tree_is_told_apart(corpus, K):
    """the corpus pins THE tree, not "some tree": on at least one witness of every column the pairwise tree (neighbours first, and
    a prefix scanned in groups of 32) gives another float than the kernels' tree"""
    rows, fam = corpus[f"rows_{K}"], corpus[f"family_{K}"]
    fss = gen.fss_of(K)
    w, _ = witness_matrix(rows, K)
    for chains, cols in ((False, so.SEQUENCE_DECIDED), (True, so.ONE_SIGNED)):
        if chains is False:
            cols = [c for c in cols if c != "skewness"]          # (its sum has been the reference's chain all along)
        kernel, _ = so.stream_columns(rows, fss, so.device_order(K), chains=chains)
        other, _ = so.stream_columns(rows, fss, "pairwise", chains=chains)
        d = so.differ(kernel, other)
        for c in cols:
            assert (d[:, COL[c]] & w[:, COL[c]]).any(), (K, c)


def test_another_tree_is_told_apart_gemaps(corpus):
    rows, fam = corpus["gemaps_rows"], corpus["gemaps_family"]
    lg = gen.log_spectrum(rows)

    def pairwise(x):
        pad = np.zeros(x.shape[:-1] + (64,))
        pad[..., :x.shape[-1]] = x
        return so.pairwise_sum(pad)
    kernel, other, seq = (so.gemaps_slopes(lg, gen.GFSS, o) for o in ("waveg", pairwise, "seq"))
    for b in (0, 1):
        assert (so.differ(kernel, other)[:, b] & so.differ(kernel, seq)[:, b]).any(), b


def test_order_primitives():
    """the restated primitives on values whose sums are exact (every order agrees) and on a case worked by hand"""
    x = np.arange(1.0, 257.0)
    for fn in (so.seq_sum, so.block_tree, so.wave_sumw(4), so.pairwise_sum):
        assert fn(x) == 256 * 257 / 2
    assert so.waveg_sum(x[:64]) == 64 * 65 / 2 and so.quad_sum(x[:16]) == 16 * 17 / 2
    assert np.array_equal(so.tree_prefix(x), np.cumsum(x)) and np.array_equal(so.pairwise_prefix(x), np.cumsum(x))
    # 1 + 2^-53 + 2^-53: one after the other the two halves of an ulp are lost, paired first they survive
    t = np.zeros(64)
    t[0], t[1], t[33] = 1.0, 2.0 ** -53, 2.0 ** -53
    assert so.seq_sum(t) == 1.0 and so.waveg_sum(t) == 1.0 + 2.0 ** -52          # lanes 1 and 33 meet at offset 32, before lane 0
    t = np.zeros(16)
    t[0], t[3], t[11] = 1.0, 2.0 ** -53, 2.0 ** -53
    assert so.quad_sum(t) == 1.0 + 2.0 ** -52                                      # lanes 3 and 11 meet at rotation 8
