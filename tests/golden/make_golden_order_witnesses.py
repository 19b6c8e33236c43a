#!/usr/bin/env python3
"""Writes tests/golden/order_witnesses.npz: magnitude spectra on which the ORDER of cSpectral's double additions decides a float
of the output -- the rows tests/test_order_witnesses_host.py and tests/test_gpu_order_witnesses.py run. Seeded and deterministic;
numpy and fractions only (tests/helpers/sum_orders.py holds the models of the orders). Run from anywhere:

    python tests/golden/make_golden_order_witnesses.py            # rewrites the file
    python tests/golden/make_golden_order_witnesses.py --check    # regenerates and compares with the committed bytes

A row is a WITNESS for a column when the model of the tree order and the model of the reference's sequential order give
different floats (a different roll-off bin). Per spectrum size K = 129, 257, 513 (frames of 16 / 32 / 64 ms at 16 kHz; the tree is
the one smilehip_spectral_frames runs at that K: spectral_frame_wave<2>, the block form, spectral_frame_wave<8>) three families:

  cancelling (1)   slope: the power spectrum mirrored about the middle of bins 1 .. K - 1, powers over 2^-30 .. 1 -- the true
                   slope is 0 and the numerator N sumA - Sf sumB is rounding noise;
                   roll-off .25 / .5 / .75: four quarters (two halves), each a permutation of the same magnitudes, powers over
                   2^-45 .. 1 -- the exact prefix at a quarter's end IS the share of the total, rounding decides `c >= th`;
                   roll-off .9: the exact prefix at the crossing bin steered onto 0.9 x the total
  steered (2)      one set per one-signed column -- both band energies, flux (a pair of rows: the previous frame, then the steered
                   one), centroid, variance, kurtosis: small-magnitude bins moved by whole float steps until the exact value
                   (fractions, on the rounded double terms both orders add) lies within 2^-56 of a float rounding midpoint, where
                   the few ulps of the double by which two orders differ pick different floats
  plain (0)        the same generators' rows before mirroring / permuting / steering: controls, every column must match

and, for the GeMAPS operator at K = 257, rows for its two band slopes of the log spectrum (`gemaps_rows`; see gemaps_candidate).

Which tree decides a witness: centroid, slope and roll-off are compared between the all-tree form the kernels had (chains=False)
and the reference; bands, flux, variance and kurtosis between the kernels as they stand (chains=True: reference centroid and
frame sum, tree sums of the one-signed terms) and the reference. Skewness has no set of its own: its sum is the reference's chain
already, it moves with the centroid (d m3 / d ctr = -3 m2), so every centroid witness is one for it.

Arrays: rows_K [n x K] float32 (one stream per K: frame t's previous frame is row t - 1), family_K [n] (0 / 1 / 2), target_K [n]
(index into sum_orders.COLUMNS of the column the row was built for, -1: none); gemaps_rows, gemaps_family, gemaps_target (0 / 1:
the band)."""
import os
import sys
from fractions import Fraction

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "helpers"))
import sum_orders as so                                      # noqa: E402

f32, f64 = np.float32, np.float64
OUT = os.path.join(HERE, "order_witnesses.npz")
SEED = 20240611
KS = (129, 257, 513)
CANDIDATES = 64                  # per mirrored / permuted set (yields: slope ~70 %, roll-off ~50 %)
STEER_CANDIDATES = 2000          # at most, per steered set; a set ends when it has its rows (yields 20 .. 90 %; the seven-bin band of K = 129: ~4 %)
KEEP_CANCELLING, KEEP_STEERED, KEEP_PLAIN = 9, 5, 2
PLAIN, CANCELLING, STEERED = 0, 1, 2
COL = {c: i for i, c in enumerate(so.COLUMNS)}


def fss_of(K):
    return (K - 1) * 2 / 16000.0


def rng_for(*key):
    return np.random.default_rng([SEED, *[int(k) for k in key]])


def ladder(rng, n, octaves):
    """n magnitudes 2^-octaves .. 1, their exponents evenly spread and shuffled, random mantissas (ldexp: no libm in the bytes)"""
    e = np.floor(-octaves * rng.permutation(n) / n).astype(np.int32)
    return np.ldexp(0.5 + 0.5 * rng.random(n), e).astype(f32)


def step(m, k):
    """the float k representable steps above m (positive floats: their bit patterns are in order)"""
    b = np.array([m], f32).view(np.int32)[0] + int(k)
    assert 0x00800000 <= b < 0x7f000000
    return np.array([b], np.int32).view(f32)[0]


# ------------------------------------------------------------------------------------------------ exact values of a row
def exact_value(column, row, prev, K, ctx=None):
    """(V, weight): the exact value (Fraction) whose rounding to float decides `column` -- on the double terms the kernels and the
    reference add, which are themselves rounded -- and per bin 1 .. K - 1 an estimate of |dV / V| for one float step of its magnitude"""
    fss = fss_of(K)
    if column.startswith("gslope"):
        return gemaps_numerator(int(column[-1]), row, ctx)
    T = so.compare_terms(row, prev, fss)
    p, fj = T["p"], T["fj"]
    n = K - 1
    ulp = 2.0 ** -22
    if column in ("band0", "band1"):
        t = T[column]
        S = so.exact_sum(t)
        il, ir, _, _ = so.band_edges(so.axis(K, fss), *so.COMPARE_BANDS[int(column[-1])])
        w = np.zeros(n)
        w[il - 1:ir] = p[il - 1:ir] * ulp / float(S)           # bins il .. ir (index = bin - 1)
        return S / n, w
    if column == "flux":
        S = so.exact_sum(T["flux"])
        d = np.sqrt(T["flux"])
        return S / n, 2.0 * d * row[1:].astype(f64) * 2.0 ** -23 / float(S)
    B, A = so.exact_sum(p), so.exact_sum(T["fp"])
    if column == "centroid":
        V = A / B
        return V, p * ulp / float(B) * np.abs(fj - float(V)) / float(V)
    if column.startswith("ro9"):
        j = ctx["j"]                                           # the crossing bin's index, fixed while the row is steered
        C = so.exact_sum(p[:j + 1])
        return C / B, p * ulp / float(B) * np.where(np.arange(n) <= j, 0.1, 0.9)
    ctr = (so.seq_sum(T["fp"]) / so.seq_sum(p)).astype(f32)                 # the reference's centroid (chains=True)
    m2t, _, m4t = so.moment_terms(p, fj, ctr)
    m2 = so.exact_sum(m2t)
    t = fj - float(ctr)
    if column == "variance":
        return m2 / B, p * ulp * np.abs(t * t / float(m2) - 1.0 / float(B))
    m4 = so.exact_sum(m4t)
    assert column == "kurtosis"
    return m4 * B / (m2 * m2), p * ulp * np.abs((t * t) * (t * t) / float(m4) - 2.0 * t * t / float(m2) + 1.0 / float(B))


def midpoint(V, through=lambda x: x):
    """the float rounding midpoint nearest to through(V), as a Fraction"""
    x = through(float(V))
    f = f32(x)
    g = np.nextafter(f, f32(np.inf) if Fraction(float(f)) <= Fraction(x) else f32(-np.inf))
    return (Fraction(float(f)) + Fraction(float(g))) / 2


def target_of(column, V):
    if column.startswith("gslope"):
        return Fraction(0)
    if column.startswith("ro9"):
        return Fraction(0.9)                                   # the double the share is given as
    if column == "flux":
        m = midpoint(V, np.sqrt)                               # sqrt(S / n) crosses the midpoint where S / n crosses its square
        return m * m
    return midpoint(V)


def crossing(row):
    """index (bin - 1) of the bin at which the reference's prefix reaches 0.9 x the total"""
    c = so.seq_prefix((row * row).astype(f32)[1:].astype(f64))
    return int(np.argmax(c >= 0.9 * c[-1]))


def steer(column, row, prev, K, tol=2.0 ** -56, rounds=14):
    """moves bins of `row` by whole float steps until the exact value lies within tol (relative) of its target -- well inside the
    few 2^-53 by which two orders of a sum differ; (row, reached)"""
    row = row.copy()
    ctx = {}
    if column == "ro90":                                       # the bins behind the crossing scaled so that the prefix is ~0.9 x the total
        j = ctx["j"] = crossing(row)
        p = (row * row).astype(f32)[1:].astype(f64)
        if j + 2 >= K:
            return row, False
        row[j + 2:] = (row[j + 2:] * f32(np.sqrt(so.seq_sum(p[:j + 1]) / 9.0 / so.seq_sum(p[j + 1:])))).astype(f32)
    V, w = exact_value(column, row, prev, K, ctx)
    M = target_of(column, V)
    scale = ctx.get("scale", abs(M))
    used = set()
    rel = abs(float((V - M) / scale))
    for _ in range(rounds):
        if rel < tol:
            break
        # the bin whose single step is ~2^-10 of the gap: ~1000 steps close it to a thousandth
        e_rel = int(np.frexp(rel)[1])
        cand = [(abs(int(np.frexp(w[i])[1]) - e_rel + 10), i) for i in range(len(w)) if w[i] > 0.0 and i not in used]
        if not cand:
            break
        j = min(cand)[1] + 1
        used.add(j - 1)
        probe = row.copy()
        h = 64
        probe[j] = step(row[j], h)
        V2, _ = exact_value(column, probe, prev, K, ctx)
        if V2 == V:
            continue
        k = int(round(float((M - V) / ((V2 - V) / h))))
        k = max(-(1 << 20), min(1 << 20, k))
        best = (rel, row, V)
        for kk in (k - 1, k, k + 1):
            trial = row.copy()
            trial[j] = step(row[j], kk)
            Vt, _ = exact_value(column, trial, prev, K, ctx)
            r = abs(float((Vt - M) / scale))
            if r < best[0]:
                best = (r, trial, Vt)
        rel, row, V = best
        w = exact_value(column, row, prev, K, ctx)[1]
    return row, rel < tol


# ------------------------------------------------------------------------------------------------ the GeMAPS band slopes
GK, GFSS = 257, 512 / 16000.0
_libm = None


def log_spectrum(mag):
    """the log power spectrum cSpectral forms with useLogSpectrum (spectral.cpp:689-716) as the oracle does: squareInput as a float
    product, factor 10 / ln 10 as a float, the C library's logf, the floor at specFloor^2"""
    global _libm
    if _libm is None:
        import ctypes
        _libm = ctypes.CDLL("libm.so.6")
        _libm.logf.restype, _libm.logf.argtypes = ctypes.c_float, [ctypes.c_float]
    mag = np.ascontiguousarray(mag, f32)
    p = (mag * mag).astype(f32)
    floor = f32(f32(0.0000001) * f32(0.0000001))
    fac = f32(10.0 / np.log(10.0))
    lg = np.array([_libm.logf(float(v)) if v > floor else 0.0 for v in p.ravel()], f32).reshape(p.shape)
    log_floor = f32(10.0 * float(f32(_libm.logf(float(floor)))) / np.log(10.0))
    return np.where(p <= floor, log_floor, (fac * lg).astype(f32)).astype(f32)


def gemaps_numerator(b, row, ctx):
    """(V, weight) for band b: V = Nind sumA - Sf sumB exactly (the terms f l are exact doubles at F0 = 31.25 Hz, both weights 1);
    scale (ctx): Nind |sumA|, so that the relative gap is the depth of the cancellation. One float step of a magnitude moves l by
    ~(10 / ln 10) 2^-22, V by that times the bin's coefficient Nind f - Sf."""
    frq = so.axis(GK, GFSS)
    il, ir, wl, wr, nind = so.slope_edges(frq, *so.GEMAPS_SLOPES[b])
    assert wl == 1.0 and wr == 1.0
    f = frq[il:ir + 1]
    l = log_spectrum(row[il:ir + 1]).astype(f64)
    Sf = so.exact_sum(f)
    V = Fraction(nind) * so.exact_sum(f * l) - Sf * so.exact_sum(l)
    ctx["scale"] = abs(Fraction(nind) * so.exact_sum(f * l))
    w = np.zeros(GK - 1)
    if il == 0:                                                # (weights are indexed by bin - 1: bin 0 is not steered)
        w[il:ir] = np.abs(nind * f[1:] - float(Sf)) * 4.34 * 2.0 ** -22 / float(ctx["scale"])
    else:
        w[il - 1:ir] = np.abs(nind * f - float(Sf)) * 4.34 * 2.0 ** -22 / float(ctx["scale"])
    return V, w


def gemaps_candidate(rng):
    """(plain row, candidate): K = 257 magnitudes. Plain: powers 2^-40 .. 1. Candidate: bins 0 .. 48 in pairs mirrored about each
    band's mean frequency (bin 8.5 of 0 .. 16, bin 33 of 16 .. 48) so that the numerator Nind sumA - Sf sumB nearly cancels; the
    unpaired bins 0, 1, 16, 17, 33 and half of the pairs lie within 2^-10 .. 2^-21 of magnitude 1 -- log values of 1e-2 .. 1e-5 dB
    beside the others' -30 .. -120 dB, the spread at which the double sums of the exact products round at all"""
    plain = spectrum(rng, GK)
    row = plain.copy()

    def near_one():
        return f32(1.0 + (1.0 if rng.random() < 0.5 else -1.0) * float(np.ldexp(0.5 + 0.5 * rng.random(), -int(rng.integers(9, 21)))))

    def far():
        return f32(np.ldexp(0.5 + 0.5 * rng.random(), -int(rng.integers(5, 20))))

    for j in (0, 1, 16, 17, 33):
        row[j] = near_one()
    for a, b in [(j, 17 - j) for j in range(2, 9)] + [(j, 66 - j) for j in range(18, 33)]:
        row[a] = row[b] = near_one() if rng.random() < 0.5 else far()
    return plain, row


def gemaps_witness(b, row):
    lg = log_spectrum(row)
    return bool(so.differ(so.gemaps_slopes(lg, GFSS, "waveg"), so.gemaps_slopes(lg, GFSS, "seq"))[0, b])


def gemaps_sets():
    out = []
    for b in (0, 1):
        kept, plain = [], []
        for c in range(STEER_CANDIDATES):
            if len(kept) >= KEEP_CANCELLING:
                break
            base, row = gemaps_candidate(rng_for(GK, 4, b, c))
            if len(plain) < KEEP_PLAIN:
                plain.append(base)
            row, ok = steer(f"gslope{b}", row, None, GK, tol=2.0 ** -26, rounds=8)
            if ok and gemaps_witness(b, row):
                kept.append(row)
        out += [(PLAIN, -1, np.array(plain)), (CANCELLING, b, np.array(kept))]
    return out


# ------------------------------------------------------------------------------------------------ candidates
def is_witness(column, row, prev, K, first=False):
    """the tree order against the reference's on one row (see the module's text for which tree)"""
    chains = column in so.ONE_SIGNED
    dev, amb = so.compare_columns(row, prev, first, fss_of(K), so.device_order(K), chains=chains)
    seq, _ = so.compare_columns(row, prev, first, fss_of(K), "seq")
    return bool(so.differ(dev, seq)[0, COL[column]]) and not bool(amb[0])


def tells_trees_apart(column, row, prev, K):
    """a witness on which ANOTHER tree (neighbours first) gives another float than the kernels' tree: two trees are both closer to
    the exact sum than the chain is and mostly agree, so every set keeps a place for one row that separates them"""
    chains = column in so.ONE_SIGNED
    dev, _ = so.compare_columns(row, prev, False, fss_of(K), so.device_order(K), chains=chains)
    other, _ = so.compare_columns(row, prev, False, fss_of(K), "pairwise", chains=chains)
    return bool(so.differ(dev, other)[0, COL[column]])


def spectrum(rng, K, octaves=20.0):
    return np.concatenate([[f32(rng.random())], ladder(rng, K - 1, octaves)]).astype(f32)


def densify(rng, row, lo, hi):
    """two bins of three of row[lo:hi] raised to 0.25 .. 1: many terms of one size with full mantissas, whose sum no two trees round
    alike (on a pure ladder every tree returns the correctly rounded sum and only the chain stands apart); the rest stays a ladder
    to steer with"""
    n = hi - lo
    pick = rng.permutation(n)[:2 * n // 3] + lo
    row[pick] = (0.25 + 0.75 * rng.random(len(pick))).astype(f32)
    return row


def mirrored(rng, K):
    base = spectrum(rng, K, 15.0)
    row = base.copy()
    row[1:] = np.concatenate([base[1:(K - 1) // 2 + 1], base[1:(K - 1) // 2 + 1][::-1]])
    return base, row


def permuted(rng, K, parts):
    base = spectrum(rng, K, 22.5)
    row = base.copy()
    q = (K - 1) // parts
    row[1:] = np.concatenate([rng.permutation(base[1:q + 1]) for _ in range(parts)])
    return base, row


def compare_sets(K, only=None):
    """[(family, target column index, rows [r x K])] for one K, in the file's order; only: restrict to these sets (the host test
    regenerates a subset)"""
    zero = np.zeros(K, f32)
    out = []

    def want(name):
        return only is None or name in only

    if want("slope"):
        kept, plain = [], []
        for c in range(CANDIDATES):
            base, row = mirrored(rng_for(K, 1, c), K)
            if len(plain) < KEEP_PLAIN:
                plain.append(base)
            if len(kept) < KEEP_CANCELLING and is_witness("slope", row, zero, K):
                kept.append(row)
        out += [(PLAIN, -1, np.array(plain)), (CANCELLING, COL["slope"], np.array(kept))]
    for parts, cols, tag in ((4, ("ro25", "ro50", "ro75"), "quarters"), (2, ("ro50",), "halves")):
        if not want(tag):
            continue
        kept, plain, have = [], [], {c: 0 for c in cols}
        need = KEEP_CANCELLING if parts == 4 else 3
        for c in range(CANDIDATES):
            base, row = permuted(rng_for(K, 2, parts, c), K, parts)
            if len(plain) < KEEP_PLAIN:
                plain.append(base)
            hit = [col for col in cols if is_witness(col, row, zero, K)]
            if hit and any(have[col] < need for col in hit):
                kept.append(row)
                for col in hit:
                    have[col] += 1
        out += [(PLAIN, -1, np.array(plain)), (CANCELLING, COL[cols[-1]] if parts == 2 else COL["ro25"], np.array(kept))]
    for column in ("ro90", "band0", "band1", "centroid", "variance", "kurtosis", "flux"):
        if not want(column):
            continue
        family = CANCELLING if column == "ro90" else STEERED
        keep = KEEP_CANCELLING if column == "ro90" else KEEP_STEERED
        kept, plain, told = [], [], False
        for c in range(STEER_CANDIDATES):
            if len(kept) >= keep * (2 if column == "flux" else 1):
                break
            rng = rng_for(K, 3, COL[column], c)
            base = spectrum(rng, K)
            lo, hi = 1, K
            if column.startswith("band"):                      # few bins inside a band: they get a ladder of their own
                il, ir, _, _ = so.band_edges(so.axis(K, fss_of(K)), *so.COMPARE_BANDS[int(column[-1])])
                base[il:ir + 1] = ladder(rng, ir - il + 1, 22.0)
                lo, hi = il, ir + 1
            if c % 2 and hi - lo >= 24:                        # every other candidate: a dense spectrum
                densify(rng, base, lo, hi)
            prev = spectrum(rng, K) if column == "flux" else zero
            if len(plain) < KEEP_PLAIN:
                plain.append(base)
            row, ok = steer(column, base, prev, K)
            if ok and is_witness(column, row, prev, K):
                t = tells_trees_apart(column, row, prev, K)
                if not (t or told) and len(kept) >= (keep - 1) * (2 if column == "flux" else 1):
                    continue                                   # the last place waits for a row that tells two trees apart
                told |= t
                kept += [prev, row] if column == "flux" else [row]
        out.append((PLAIN, -1, np.array(plain)))
        if column == "flux":                                   # the partner rows are plain spectra; the steered one follows its partner
            fam = np.tile([PLAIN, STEERED], len(kept) // 2)
            tgt = np.tile([-1, COL["flux"]], len(kept) // 2)
            out.append((fam, tgt, np.array(kept)))
        else:
            out.append((family, COL[column], np.array(kept)))
    return out


def assemble(sets, K):
    rows = np.concatenate([r.reshape(-1, K) for _, _, r in sets]).astype(f32)
    fam = np.concatenate([np.broadcast_to(np.asarray(f, np.int8), (len(r.reshape(-1, K)),)) for f, _, r in sets]).astype(np.int8)
    tgt = np.concatenate([np.broadcast_to(np.asarray(t, np.int8), (len(r.reshape(-1, K)),)) for _, t, r in sets]).astype(np.int8)
    return rows, fam, tgt


def build(ks=KS, only=None, gemaps=True):
    arrays = {}
    for K in ks:
        arrays[f"rows_{K}"], arrays[f"family_{K}"], arrays[f"target_{K}"] = assemble(compare_sets(K, only), K)
    if gemaps:
        arrays["gemaps_rows"], arrays["gemaps_family"], arrays["gemaps_target"] = assemble(gemaps_sets(), GK)
    return arrays


def main():
    arrays = build()
    if "--check" in sys.argv:
        have = np.load(OUT)
        bad = [k for k in arrays if not (k in have.files and np.array_equal(have[k].view(np.uint8), arrays[k].view(np.uint8)))]
        print("identical" if not bad else f"DIFFERENT: {bad}")
        return 1 if bad else 0
    np.savez_compressed(OUT, **arrays)
    for K in KS:
        fam = arrays[f"family_{K}"]
        print(f"K = {K}: {len(fam)} rows, plain {int((fam == 0).sum())}, cancelling {int((fam == 1).sum())}, steered {int((fam == 2).sum())}")
    fam = arrays["gemaps_family"]
    print(f"GeMAPS: {len(fam)} rows, plain {int((fam == 0).sum())}, cancelling {int((fam == 1).sum())}")
    print(f"{OUT}: {os.path.getsize(OUT)} bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main())
