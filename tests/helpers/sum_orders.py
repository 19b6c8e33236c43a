"""The orders in which cSpectral's double sums are added -- the reference's and the kernels' -- restated on the host (numpy and
fractions only), and the arithmetic-only columns of the ComParE option set and the two GeMAPS band slopes formed on top of any
of them. tests/golden/make_golden_order_witnesses.py uses the models to build spectra on which two orders give different
floats (witnesses); tests/test_order_witnesses_host.py holds the sequential model to the oracle bit for bit;
tests/test_gpu_order_witnesses.py holds the kernels to the models.

The reference (spectral.cpp) adds bin after bin: seq_sum / seq_prefix. The kernels' orders, from csrc as it stands:

  block_tree        lld_blocks_compare.hpp block_sum_n: thread i owns bin i + 1; a shuffle-down tree inside each wave of 64
                    (offsets 32, 16, .. 1), then ((r0 + r1) + r2) + r3 over the four waves
  wave_sumw(W)      lld_blocks_compare.hpp wave_sumw<W>: lane l owns bins l + 64 w + 1; its W terms first, w = 0 .. W - 1 in
                    order, then one shuffle-down tree over the 64 lanes
  waveg_sum         lld_blocks.hpp WaveG::sum: the shuffle-down tree over 64 lane values
  quad_sum          lld_blocks.hpp QuadG::sum: a butterfly of row rotations 8, 4, 2, 1 over 16 lane values
  tree_prefix       the inclusive prefix of the kernels' former roll-off scan (block and wave form alike): a Hillis-Steele scan
                    (offsets 1, 2, .. 32) inside each group of 64 bins, then + the totals of the earlier groups, one after the other

Which sum of the ComParE set takes which order (`compare_columns(.., order, chains=...)`):

  chains=True   the kernels as they stand: frameSum (= sumB), the centroid numerator sumA and the roll-off prefix are the
                reference's sequential chains (one lane walks the bins), the third moment as well; band energies, flux, second and
                fourth moment keep the tree `order`. Sequence-decided columns equal the reference whatever the spectrum; the
                one-signed ones are within one float ulp.
  chains=False  the kernels before that change: every sum but the third moment in the tree `order`, the prefix by tree_prefix.
                The witness generator uses this to build the rows on which centroid, slope and roll-off used to differ.

The terms are formed as the kernels and the oracle form them: p = float(m * m), fj = F0 * j in double, the centroid rounded to
float before the moments; numpy's float64 operations are IEEE double operations, one rounding each, nothing fused. Entropy goes
through log() and is not modelled."""
from fractions import Fraction

import numpy as np

f32, f64 = np.float32, np.float64

ROLLOFF = (0.25, 0.5, 0.75, 0.9)
COMPARE_BANDS = ((250, 650), (1000, 4000))
# the modelled columns and where the ComParE option set writes them (15 values per frame; 8 = entropy, 13 = sharpness, 14 = harmonicity)
COLUMNS = ("band0", "band1", "ro25", "ro50", "ro75", "ro90", "flux", "centroid", "variance", "skewness", "kurtosis", "slope")
COLUMN_INDEX = dict(band0=0, band1=1, ro25=2, ro50=3, ro75=4, ro90=5, flux=6, centroid=7, variance=9, skewness=10, kurtosis=11, slope=12)
MODELLED = [COLUMN_INDEX[c] for c in COLUMNS]
# columns whose value the order of the additions can move by more than an ulp (cancellation, a threshold, or a sum that feeds one):
# the kernels follow the reference's order there
SEQUENCE_DECIDED = ("ro25", "ro50", "ro75", "ro90", "centroid", "skewness", "slope")
ONE_SIGNED = ("band0", "band1", "flux", "variance", "kurtosis")


# ------------------------------------------------------------------------------------------------ sums along the last axis
def seq_sum(x):
    """one addition after the other, index order (np.add.accumulate is the recurrence out[i] = out[i - 1] + x[i])"""
    return np.add.accumulate(np.asarray(x, f64), axis=-1)[..., -1]


def seq_prefix(x):
    return np.add.accumulate(np.asarray(x, f64), axis=-1)


def _down_tree(x):
    """lane 0 of `for off in 32, 16, .. 1: x += shfl_down(x, off)` over 64 lanes"""
    assert x.shape[-1] == 64
    for off in (32, 16, 8, 4, 2, 1):
        x = x[..., :off] + x[..., off:2 * off]
    return x[..., 0]


def waveg_sum(x):
    return _down_tree(np.asarray(x, f64))


def block_tree(x):
    x = np.asarray(x, f64)
    assert x.shape[-1] == 256
    r = _down_tree(x.reshape(x.shape[:-1] + (4, 64)))
    return ((r[..., 0] + r[..., 1]) + r[..., 2]) + r[..., 3]


def wave_sumw(W):
    def fn(x):
        x = np.asarray(x, f64)
        assert x.shape[-1] == 64 * W
        g = x.reshape(x.shape[:-1] + (W, 64))
        t = g[..., 0, :]
        for w in range(1, W):
            t = t + g[..., w, :]
        return _down_tree(t)
    fn.__name__ = f"wave_sumw{W}"
    return fn


def quad_sum(x):
    """every lane of the row ends with the same value (the butterfly is symmetric and IEEE addition commutes)"""
    x = np.asarray(x, f64)
    assert x.shape[-1] == 16
    for r in (8, 4, 2, 1):
        x = x + np.roll(x, r, axis=-1)
    return x[..., 0]


def pairwise_sum(x):
    """NOT a kernel's order: neighbours first, (x0 + x1) + (x2 + x3) .. -- the deliberately re-associated tree of the host test"""
    x = np.asarray(x, f64)
    while x.shape[-1] > 1:
        assert x.shape[-1] % 2 == 0
        x = x[..., 0::2] + x[..., 1::2]
    return x[..., 0]


def _group_prefix(x, G):
    x = np.asarray(x, f64)
    n = x.shape[-1]
    assert n % G == 0
    c = x.reshape(x.shape[:-1] + (n // G, G)).copy()
    off = 1
    while off < G:                                           # Hillis-Steele: every lane adds the value `off` lanes below, at once
        y = c.copy()
        y[..., off:] = c[..., off:] + c[..., :-off]
        c = y
        off *= 2
    red = c[..., G - 1].copy()
    for w in range(1, n // G):
        for w2 in range(w):
            c[..., w, :] = c[..., w, :] + red[..., w2, None]
    return c.reshape(x.shape)


def tree_prefix(x):
    return _group_prefix(x, 64)


def pairwise_prefix(x):
    """NOT a kernel's order: the same scan over groups of 32"""
    return _group_prefix(x, 32)


def orders_for(K):
    """name -> (sum, prefix) for the spectra of K = 64 W + 1 bins: the orders the kernels of that size use, and 'pairwise'"""
    W = (K - 1) // 64
    assert K == 64 * W + 1 and W in (2, 4, 8)
    o = {"seq": (seq_sum, seq_prefix), f"wave{W}": (wave_sumw(W), tree_prefix), "pairwise": (pairwise_sum, pairwise_prefix)}
    if W == 4:
        o["block"] = (block_tree, tree_prefix)
    return o


def device_order(K):
    """the order smilehip_spectral_frames runs at this K: the block form at 257, spectral_frame_wave<W> at 129 and 513"""
    return "block" if K == 257 else f"wave{(K - 1) // 64}"


# ------------------------------------------------------------------------------------------------ the ComParE columns
def band_edges(frq, lo, hi):
    """spectral.cpp:779-826 with a frequency axis: (iL, iR, wL, wR)"""
    n = len(frq)
    ii = next((i for i in range(n) if frq[i] > float(lo)), n)
    wl = (frq[ii] - float(lo)) / (frq[ii] - frq[ii - 1]) if 0 < ii < n else 1.0
    il = min(max(float(ii) - 1.0, 0.0), float(n))
    if wl == 0.0:
        wl = 1.0
    ii = next((i for i in range(n) if frq[i] >= float(f32(hi))), n)
    wr = (float(hi) - frq[ii - 1]) / (frq[ii] - frq[ii - 1]) if 0 < ii < n else 1.0
    ir = float(ii) if ii < n and frq[ii] == float(f32(hi)) else float(ii) - 1.0
    ir = min(ir, float(n - 1))
    if wr == 0.0:
        wr = 1.0
    il, ir = int(np.floor(il)), int(np.floor(ir))
    if il >= n:
        il = ir = n - 1
        wl = wr = 0.0
    return max(il, 0), max(ir, 0), wl, wr


def axis(K, fss):
    return (1.0 / fss) * np.arange(K, dtype=f64)


def compare_terms(mag, prev, fss):
    """the per-bin double terms of bins 1 .. K - 1, as rows: p, fj p, flux, band 0, band 1 (and fj)"""
    mag = np.ascontiguousarray(mag, f32)
    K = mag.shape[-1]
    frq = axis(K, fss)
    pw = (mag * mag).astype(f32)                              # squareInput, a float product (:676-683)
    p = pw[..., 1:].astype(f64)
    fj = frq[1:]
    d = mag[..., 1:].astype(f64) - np.ascontiguousarray(prev, f32)[..., 1:].astype(f64)
    bands = []
    for lo, hi in COMPARE_BANDS:
        il, ir, wl, wr = band_edges(frq, lo, hi)
        assert il >= 1, "bin 0 inside a band: not modelled"
        t = np.zeros(mag.shape, f64)
        t[..., il] = t[..., il] + pw[..., il].astype(f64) * wl
        t[..., il + 1:ir] = pw[..., il + 1:ir].astype(f64)
        t[..., ir] = t[..., ir] + pw[..., ir].astype(f64) * wr
        bands.append(t[..., 1:])
    return dict(p=p, fj=fj, fp=fj * p, flux=d * d, band0=bands[0], band1=bands[1])


def moment_terms(p, fj, ctr):
    t1 = fj - np.asarray(ctr, f32).astype(f64)[..., None]
    m2 = t1 * t1 * p
    m3 = m2 * t1
    return m2, m3, m3 * t1


def rolloff_bins(c, th, first_crossing):
    """index (0-based bin - 1) of the reported bin; first_crossing: the kernels' test (c[j] >= th and not c[j - 1] >= th), which
    names more than one bin where a tree prefix is not monotone -- `ambiguous` then"""
    m = c >= th[..., None]
    if not first_crossing:
        return np.argmax(m, axis=-1), ~m.any(axis=-1)
    cand = m.copy()
    cand[..., 1:] &= ~m[..., :-1]
    return np.argmax(cand, axis=-1), cand.sum(axis=-1) != 1


def compare_columns(mag, prev, first, fss, order, chains=True):
    """(values [R x len(COLUMNS)] float32, ambiguous [R] bool) for R magnitude rows, each with its previous frame's magnitudes and
    a `first` flag (flux 0). order: a key of orders_for(K), or a (sum, prefix) pair."""
    mag = np.atleast_2d(np.ascontiguousarray(mag, f32))
    prev = np.atleast_2d(np.ascontiguousarray(prev, f32))
    first = np.atleast_1d(np.asarray(first, bool))
    R, K = mag.shape
    n = K - 1
    tsum, tprefix = orders_for(K)[order] if isinstance(order, str) else order
    csum, cprefix = (seq_sum, seq_prefix) if chains else (tsum, tprefix)
    T = compare_terms(mag, prev, fss)
    p, fj = T["p"], T["fj"]
    out = np.zeros((R, len(COLUMNS)), f32)
    col = {c: i for i, c in enumerate(COLUMNS)}
    with np.errstate(all="ignore"):
        sB, sA = csum(p), csum(T["fp"])
        for b in (0, 1):
            out[:, col[f"band{b}"]] = (tsum(T[f"band{b}"]) / f64(n)).astype(f32)
        c = cprefix(p)
        amb = np.zeros(R, bool)
        frq = axis(K, fss)
        for i, share in enumerate(ROLLOFF):
            idx, a = rolloff_bins(c, f64(share) * sB, first_crossing=not (csum is seq_sum))
            amb |= a
            out[:, col["ro25"] + i] = frq[idx + 1].astype(f32)
        fl = tsum(T["flux"]) / f64(n)
        out[:, col["flux"]] = np.where(~first & (fl > 0.0), np.sqrt(fl), 0.0).astype(f32)
        ctr = np.where(sB != 0.0, sA / sB, 0.0).astype(f32)
        out[:, col["centroid"]] = ctr
        m2t, m3t, m4t = moment_terms(p, fj, ctr)
        m2, m3, m4 = tsum(m2t), seq_sum(m3t), tsum(m4t)
        s2 = np.where(sB != 0.0, m2 / sB, 0.0)
        out[:, col["variance"]] = s2.astype(f32)
        out[:, col["skewness"]] = np.where(s2 <= 0.0, 0.0, m3 / (sB * s2 * np.sqrt(s2))).astype(f32)
        out[:, col["kurtosis"]] = np.where(s2 == 0.0, 0.0, m4 / (sB * s2 * s2)).astype(f32)
        Sf, S2f = seq_sum(fj), seq_sum(fj * fj)
        deno = f64(n) * S2f - Sf * Sf
        slope = (f64(n) * sA - Sf * sB) / deno if deno != 0.0 else np.zeros(R)
        out[:, col["slope"]] = (slope * (f64(n) - 1.0)).astype(f32)
    return out, amb


def stream_columns(rows, fss, order, chains=True):
    """compare_columns over the frames of one stream: frame t's previous frame is row t - 1, the first frame's flux is 0"""
    rows = np.ascontiguousarray(rows, f32)
    prev = np.concatenate([np.zeros((1, rows.shape[1]), f32), rows[:-1]])
    first = np.arange(len(rows)) == 0
    return compare_columns(rows, prev, first, fss, order, chains)


def differ(a, b):
    """cells whose bits differ (both-zero counts as equal)"""
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    return (a.view(np.uint32) != b.view(np.uint32)) & ~((a == 0) & (b == 0))


# ------------------------------------------------------------------------------------------------ the GeMAPS band slopes
GEMAPS_SLOPES = ((0, 500), (500, 1500))


def gemaps_slopes(lg, fss, order, K=None):
    """the two band slopes of the log spectrum (spectral.cpp:872-992, oldSlopeScale = 0; csrc/lld_gemaps.hip:84-106) from rows of
    the log power spectrum `lg` (float32, K columns: what the oracle forms with the C library's logf). order: 'seq' (the
    reference's four chains; the kernel's, one lane walking the band's bins) or 'waveg' (the former form: lane l holds bin iL + l,
    zeros behind the band, WaveG::sum) or a sum function over the band's bins."""
    lg = np.atleast_2d(np.ascontiguousarray(lg, f32))
    K = lg.shape[1] if K is None else K
    frq = axis(K, fss)
    out = np.zeros((lg.shape[0], 2), f32)
    for b, (lo, hi) in enumerate(GEMAPS_SLOPES):
        il, ir, wl, wr, nind = slope_edges(frq, lo, hi)
        f = frq[il:ir + 1].copy()
        w = np.ones(ir - il + 1)
        w[0], w[-1] = wl, wr
        fw = f * w
        l = lg[:, il:ir + 1].astype(f64)
        f2 = np.concatenate([[fw[0] * fw[0]], f[1:-1] * f[1:-1], [f[-1] * wr * f[-1] * wr]])      # (:944-962: Sf * Sf left, ((f w) f) w right)
        terms = [np.broadcast_to(fw, l.shape), np.broadcast_to(f2, l.shape), fw * l, w * l]               # Sf, S2f, sumA, sumB
        if order == "seq":
            fn = seq_sum
        elif order == "waveg":
            def fn(x):
                pad = np.zeros(x.shape[:-1] + (64,), f64)
                pad[..., :x.shape[-1]] = x
                return waveg_sum(pad)
        else:
            fn = order
        Sf, S2f, sA, sB = (fn(t) for t in terms)
        with np.errstate(all="ignore"):
            deno = nind * S2f - Sf * Sf
            out[:, b] = np.where(deno != 0.0, (nind * sA - Sf * sB) / deno, 0.0).astype(f32)
    return out


def slope_edges(frq, lo, hi):
    """spectral.cpp:886-942: (iL, iR, wL, wR, Nind)"""
    n = len(frq)
    ii = next((i for i in range(n) if frq[i] > float(lo)), n)
    wl = (frq[ii] - float(lo)) / (frq[ii] - frq[ii - 1]) if 0 < ii < n else 1.0
    idl = min(max(float(ii) - 1.0, 0.0), float(n))
    if wl == 0.0:
        wl = 1.0
    ii = next((i for i in range(n) if frq[i] >= float(f32(hi))), n)
    wr = (float(hi) - frq[ii - 1]) / (frq[ii] - frq[ii - 1]) if 0 < ii < n else 1.0
    idr = float(ii) if ii < n and frq[ii] == float(f32(hi)) else float(ii) - 1.0
    idr = min(idr, float(n - 1))
    if wr == 0.0:
        wr = 1.0
    il, ir = int(np.floor(idl)), int(np.floor(idr))
    assert il < n and ir < n and ir - il >= 2
    return il, ir, wl, wr, idr - idl


# ------------------------------------------------------------------------------------------------ exact values (steering)
def exact_sum(x):
    """the exact sum of a vector of doubles"""
    m, e = np.frexp(np.asarray(x, f64).ravel())
    mi = (m * 9007199254740992.0).astype(np.int64)            # 2^53: exact
    emin = int(e.min())
    tot = 0
    for a, b in zip(mi.tolist(), (e - emin).tolist()):
        tot += a << b
    return Fraction(tot) * Fraction(2) ** (emin - 53)
