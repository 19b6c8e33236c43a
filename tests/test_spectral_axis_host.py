"""cSpectral on any spectrum, host side: a numpy restatement of cSpectral::processVector (src/lldcore/spectral.cpp:586-1555) with the
options the older general operator fixes -- squareInput, useLogSpectrum / specFloor, normBandEnergies, alphaRatio, hammarbergIndex,
freqRange, oldSlopeScale, buggyRollOff -- and the level's own frequency axis (or none) lives here: float32 / float64 elementwise IEEE
operations, every sum a strictly sequential np.add.accumulate in the reference's order, the C library's logf / expf / log / pow
through ctypes and math. It is held bit-equal to what the real binary wrote (tests/golden/spectral_axis_synth.npz, made by
tests/golden/make_golden_spectral_axis.py from tests/conf/spectral_axis.conf), and the library's table builder
(smilehip_spectral_axis_tables) is held bit-equal to the restatement's setup, refusals included.
tests/test_gpu_spectral_axis.py runs the device operator against the same restatement."""
import ctypes as C
import ctypes.util
import math
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIN, LOG, BARK, MEL, SEM, BAO = 0, 1, 2, 3, 4, 7            # SPECTSCALE_* (src/include/smileutil/smileUtil.h:330-337)
f32, f64 = np.float32, np.float64

_libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.logf.restype = C.c_float
_libm.logf.argtypes = [C.c_float]
_libm.expf.restype = C.c_float
_libm.expf.argtypes = [C.c_float]


def logf(x):
    return f32(_libm.logf(float(x)))


def expf(x):
    return f32(_libm.expf(float(x)))


def logf_v(x):
    with np.errstate(all="ignore"):
        return np.array([_libm.logf(float(v)) for v in x], f32)


class Refused(Exception):
    """the reference's own setup is undefined for these options"""


def seq(x, dtype=f64, start=None):
    """x[0] + x[1] + ... one after the other in dtype (np.sum adds pairwise); start: the accumulator's value before x[0]"""
    x = np.asarray(x, dtype)
    if start is not None:
        x = np.concatenate([np.array([start], dtype), x])
    if x.size == 0:
        return dtype(0.0)
    with np.errstate(all="ignore"):
        return np.add.accumulate(x, dtype=dtype)[-1]


def fwd(x, scale, param):
    """smileDsp_specScaleTransfFwd (smileUtil.c:1097-1147)"""
    if scale == LOG:
        return math.log(x) / math.log(param) if x > 0 else 0.0
    if scale == SEM:
        return 12.0 * (math.log(x / param) / math.log(2.0)) if x / param > 1.0 else 0.0
    if scale == BAO:
        return (26.81 / (1.0 + 1960.0 / x)) - 0.53 if x > 0 else 0.0
    if scale == BARK:
        if x > 0:
            zz = (26.81 / (1.0 + 1960.0 / x)) - 0.53
            if zz < 2:
                return 0.85 * zz + 0.3
            if zz > 20.1:
                return 1.22 * zz - 0.22 * 20.1
            return zz
        return 0.0
    if scale == MEL:
        return 1127.0 * math.log(1.0 + x / 700.0) if x > 0.0 else 0.0
    return x


def inv(x, scale, param):
    """smileDsp_specScaleTransfInv (smileUtil.c:1158-1199)"""
    if scale == LOG:
        return math.exp(x * math.log(param))
    if scale == SEM:
        return param * math.pow(2.0, x / 12.0)
    if scale == BAO:
        z0 = (x + 0.53) / 26.81
        return (1960.0 * z0) / (1.0 - z0) if z0 != 1.0 else 0.0
    if scale == BARK:
        zz = x
        if x > 20.1:
            zz = (x + 0.22 * 20.1) / 1.22
        elif x < 2:
            zz = (x - 0.3) / 0.85
        z0 = 26.81 / (zz + 0.53)
        return 1960.0 / (z0 - 1.0) if z0 != 1.0 else 0.0
    if scale == MEL:
        return 700.0 * (math.exp(x / 1127.0) - 1.0)
    return x


def sharp_weight(bark):
    """f * smileDsp_getSharpnessWeightG(f, SPECTSCALE_BARK, 0.0) (smileUtil.c:1064-1078)"""
    g = 1.0 if bark <= 16.0 else math.pow((bark - 16.0) / 4.0, 1.5849625) + 1.0
    return bark * g


# the options: cSpectral's names in the spelling of capi.spectral_axis_opts, with the component's defaults where the tests do not care
DEFAULTS = dict(bands=(), slopes=(), rolloff=(), square_input=1, use_log_spectrum=0, norm_band_energies=0, alpha_ratio=0,
                hammarberg_index=0, old_slope_scale=1, buggy_roll_off=0, tonality=0, spec_floor=0.0000001, freq_range=(0, 0), frq_scale=LIN,
                frq_scale_param=0.0, spec_diff=0, spec_pos_diff=0, flux=0, flux_centroid=0, flux_at_flux_centroid=0, centroid=0, max_pos=0,
                min_pos=0, entropy=0, standard_deviation=0, variance=0, skewness=0, kurtosis=0, slope=0, sharpness=0, harmonicity=0,
                flatness=0, log_flatness=0)
FLUX_FAMILY = ("spec_diff", "spec_pos_diff", "flux", "flux_centroid", "flux_at_flux_centroid")
SINGLE = FLUX_FAMILY + ("centroid", "max_pos", "min_pos", "entropy", "standard_deviation", "variance", "skewness", "kurtosis", "slope",
                        "sharpness", "harmonicity", "flatness")


def opts(**kw):
    o = dict(DEFAULTS)
    for k in kw:
        assert k in o, k
    o.update(kw)
    return o


def n_out(o):
    return len(o["bands"]) + len(o["slopes"]) + len(o["rolloff"]) + bool(o["alpha_ratio"]) + bool(o["hammarberg_index"]) + sum(bool(o[k]) for k in SINGLE)


def ref_setup(o, K, fs_sec, frq=None):
    """what processVector derives from the options and the axis before it looks at a spectrum; frq: K doubles or None"""
    if not 4 <= K <= 1 << 20 or not fs_sec > 0.0 or o["tonality"]:
        raise Refused("K / frame size / tonality")
    if len(o["bands"]) > 16 or len(o["slopes"]) > 16 or len(o["rolloff"]) > 16 or n_out(o) < 1:
        raise Refused("counts")
    if any(not 0.0 <= r <= 1.0 for r in o["rolloff"]):
        raise Refused("rollOff")
    axis = frq is not None
    if axis:
        frq = np.asarray(frq, f64)
        if frq.size < K:
            raise Refused("n_scale")
        frq = frq[:K]                                        # nScale = MIN(nScale, Nsrc) (:606-609)
        if not np.all(np.isfinite(frq)) or not np.all(frq[1:] > frq[:-1]):
            raise Refused("frq")
    F0 = 1.0 / fs_sec
    S = dict(K=K, axis=axis, F0=F0)
    # :85-91, :228-237
    if o["use_log_spectrum"]:
        sf = f32(o["spec_floor"])
        if not (sf > 0) or not np.isfinite(sf):
            raise Refused("specFloor")
        sf = f32(sf * sf)
        if not sf > 0:
            raise Refused("specFloor")
    else:
        sf = f32(0.0000001 * 0.0000001)
    S["spec_floor"] = sf
    S["log_spec_floor"] = f32(10.0 * float(logf(sf)) / math.log(10.0))
    S["log_spec_factor"] = f32(10.0 / math.log(10.0))
    # :625-647
    rl, ru = o["freq_range"]
    if rl < 0 or ru < rl:
        raise Refused("freqRange")
    if rl == 0 and ru == 0:
        lo, hi = 1, K - 1
    else:
        if not axis:
            raise Refused("freqRange without an axis")
        lo = hi = -1
        for i in range(K):
            if float(rl) >= frq[i]:
                lo = i
            if float(ru) > frq[i]:
                hi = i
        if hi == -1 or hi >= K:
            hi = K - 1
        if lo < 0:
            lo = 0
        if hi < lo:
            raise Refused("freqRange selects no bin")
    S["lo"], S["hi"] = lo, hi
    nBins = hi - lo + 1
    # :771-840, :873-946
    edges = []
    for (bl, bh) in tuple(o["bands"]) + tuple(o["slopes"]):
        if bl < 0 or bh <= bl:
            raise Refused("band")
        if not axis:
            idxL = float(bl) / F0
            wL = math.ceil(idxL) - idxL
            idxR = float(bh) / F0
            wR = idxR - math.floor(idxR)
        else:
            ii = 0
            while ii < K and not frq[ii] > float(bl):
                ii += 1
            wL = (frq[ii] - float(bl)) / (frq[ii] - frq[ii - 1]) if 0 < ii < K else 1.0
            idxL = float(ii) - 1.0
            if idxL < 0:
                idxL = 0.0
            if idxL >= K:
                idxL = float(K)
            bhf = float(f32(bh))                              # `frq[ii] >= (FLOAT_DMEM)bandsH[iii]`
            ii = 0
            while ii < K and not frq[ii] >= bhf:
                ii += 1
            wR = (float(bh) - frq[ii - 1]) / (frq[ii] - frq[ii - 1]) if 0 < ii < K else 1.0
            idxR = float(ii) if (ii < K and frq[ii] == bhf) else float(ii) - 1.0
            if idxR >= K:
                idxR = float(K - 1)
        if wL == 0.0:
            wL = 1.0
        if wR == 0.0:
            wR = 1.0
        iL, iR = int(math.floor(idxL)), int(math.floor(idxR))
        if iL >= K:
            iL = iR = K - 1
            wR = wL = 0.0
        if iR >= K:
            iR = K - 1
            wR = 1.0
        iL, iR = max(iL, 0), max(iR, 0)
        if iR < iL:
            raise Refused("a band between two bins")
        edges.append((iL, iR, float(wL), float(wR), float(idxR - idxL)))
    S["edges"] = edges
    # :995-1089
    f, n1a, n1h, j = 0.0, -1, -1, 0
    while j < K:
        fj = frq[j] if axis else f
        if fj > 5000.0:
            break
        if not fj < 1000.0 and n1a < 0:
            n1a = j
        if not fj < 2000.0 and n1h < 0:
            n1h = j
        f += F0
        j += 1
    S["ar"] = (j if n1a < 0 else n1a, j)
    S["hb"] = (j if n1h < 0 else n1h, j)
    # the axes
    ctr_group = any(o[k] for k in ("centroid", "standard_deviation", "variance", "skewness", "kurtosis", "slope"))
    f = 0.0                                                   # :1261
    if axis:
        S["ax_m"] = S["ax_c"] = S["ax_s"] = frq.copy()
        S["ax_ro"] = frq.astype(f32)
    else:
        S["ax_m"] = np.arange(K, dtype=f64) * F0
        S["ax_ro"] = np.arange(K, dtype=f32) * f32(F0)
        S["ax_s"] = np.arange(K, dtype=f64)
        ax_c = np.zeros(K)
        if ctr_group:
            for j in range(lo, hi + 1):                       # :1291-1294
                ax_c[j] = f
                f += F0
        S["ax_c"] = ax_c
    # :1400-1418
    if axis:
        S["slope_S2f"] = seq(frq[lo:hi + 1] * frq[lo:hi + 1])
        S["slope_Sf"] = seq(frq[lo:hi + 1])
    else:
        Nind = float(nBins)
        NNm1 = Nind * (Nind - 1.0)
        S["slope_Sf"] = f64(NNm1 / 2.0 * F0)
        S["slope_S2f"] = f64(NNm1 * (2.0 * Nind - 1.0) / 6.0 * F0 * F0)
    # :1438-1468
    sharp = np.zeros(nBins)
    if o["sharpness"]:
        for j in range(lo, hi + 1):
            if axis:
                fb = float(frq[j])
                if o["frq_scale"] != BARK:
                    fb = fwd(inv(fb, o["frq_scale"], o["frq_scale_param"]), BARK, 0.0)
            else:
                fb = fwd(f, BARK, 0.0)
                f += F0
            sharp[j - lo] = sharp_weight(fb)
        if not np.all(np.isfinite(sharp)):
            raise Refused("sharpness weights")
    S["sharp"] = sharp
    return S


def ref_row(S, o, src, prev):
    """one frame; prev: the frame before (as it came in) or None on a stream's first frame"""
    K, lo, hi, axis, F0 = S["K"], S["lo"], S["hi"], S["axis"], S["F0"]
    nBins = hi - lo + 1
    use_log = bool(o["use_log_spectrum"])
    src = np.asarray(src, f32)
    with np.errstate(all="ignore"):
        def mag(x):                                           # :661-676
            if o["square_input"]:
                return x
            return np.where(x > 0, np.sqrt(np.where(x > 0, x, f32(0))), f32(0)).astype(f32)
        srcM = mag(src)
        srcP = (src * src).astype(f32) if o["square_input"] else src
        if use_log:                                           # :689-716
            srcL = np.where(srcP <= S["spec_floor"], S["log_spec_floor"], (S["log_spec_factor"] * logf_v(np.where(srcP <= S["spec_floor"], f32(1), srcP))).astype(f32)).astype(f32)
            srcLP = srcL
        else:
            srcLP = srcP
        P, LP = srcP.astype(f64), srcLP.astype(f64)
        out = []
        frameSum = seq(P[lo:hi + 1])
        nb = len(o["bands"])
        for (iL, iR, wL, wR, _) in S["edges"][:nb]:           # :843-868
            s = seq(np.concatenate([[P[iL] * wL], P[iL + 1:iR], [P[iR] * wR]]))
            if o["norm_band_energies"]:
                out.append(f32(s / frameSum) if frameSum > 0.0 else f32(0))
            elif use_log:
                q = s / float(nBins)
                out.append(f32(10.0 * (math.log(q) if q > 0 else (-math.inf if q == 0 else math.nan)) / math.log(10.0)))
            else:
                out.append(f32(s / float(nBins)))
        a = S["ax_s"]
        for (iL, iR, wL, wR, Nind) in S["edges"][nb:]:        # :942-991
            mid = slice(iL + 1, iR) if axis else slice(0, 0)
            Sf0 = a[iL] * wL
            Sf = seq(np.concatenate([[Sf0], a[mid], [a[iR] * wR]]))
            S2f = seq(np.concatenate([[Sf0 * Sf0], a[mid] * a[mid], [a[iR] * wR * a[iR] * wR]]))
            sA = seq(np.concatenate([[a[iL] * wL * LP[iL]], a[mid] * LP[mid], [a[iR] * wR * LP[iR]]]))
            sB = seq(np.concatenate([[wL * LP[iL]], LP[mid], [wR * LP[iR]]]))
            if not axis:
                S2f, Sf, sA = S2f * (F0 * F0), Sf * F0, sA * F0
            deno = Nind * S2f - Sf * Sf
            slope = (Nind * sA - Sf * sB) / deno if deno != 0.0 else 0.0
            out.append(f32(slope * (Nind - 1.0)) if o["old_slope_scale"] else f32(slope))
        sfl = S["spec_floor"]
        if o["alpha_ratio"]:                                  # :995-1037
            n1, n2 = S["ar"]
            s01, s15 = seq(srcP[:n1], f32), seq(srcP[n1:n2], f32)
            if s01 > 0:
                if not use_log:
                    out.append(f32(s15 / s01))
                elif s15 > sfl:
                    out.append(f32(10.0 * float(logf(f32(s15 / s01))) / math.log(10.0)))
                else:
                    out.append(f32(10.0 * float(f32(logf(sfl) - logf(s01))) / math.log(10.0)))
            else:
                out.append(f32(0))
        if o["hammarberg_index"]:                             # :1039-1089
            n1, n2 = S["hb"]
            m02 = max(f32(0), srcP[:n1].max()) if n1 > 0 else f32(0)
            m25 = max(f32(0), srcP[n1:n2].max()) if n2 > n1 else f32(0)
            if m25 > 0:
                if not use_log:
                    out.append(f32(m02 / m25))
                elif m02 > sfl:
                    out.append(f32(10.0 * float(logf(f32(m02 / m25))) / math.log(10.0)))
                else:
                    out.append(f32(10.0 * float(f32(logf(sfl) - logf(m25))) / math.log(10.0)))
            else:
                out.append(f32(0))
        sumB = frameSum if (o["norm_band_energies"] and not use_log) else seq(LP[lo:hi + 1])   # :1092-1099
        nro = len(o["rolloff"])
        if nro:                                               # :1102-1122
            rep = nro if o["buggy_roll_off"] == 1 else 1
            acc = np.add.accumulate(np.repeat(P[lo:hi + 1], rep)).reshape(nBins, rep)
            for i, r in enumerate(o["rolloff"]):
                hit = acc[:, i if rep > 1 else 0] >= r * frameSum
                val = S["ax_ro"][lo:hi + 1][hit]
                nz = val[val != 0]
                out.append(f32(nz[0]) if nz.size else f32(0))
        if any(o[k] for k in FLUX_FAMILY):                    # :1124-1254
            if prev is None:
                out.append(f32(0))
            else:
                magP = mag(np.asarray(prev, f32))
                dM = srcM[lo:hi + 1].astype(f64) - magP[lo:hi + 1].astype(f64)
                dF = (srcM[lo:hi + 1] - magP[lo:hi + 1]).astype(f32).astype(f64)
                if o["spec_diff"]:
                    d = seq(dF * dF) / float(nBins)
                    out.append(f32(math.sqrt(d)) if d > 0.0 else f32(0))
                if o["spec_pos_diff"]:
                    d = seq(np.where(dF > 0, dF * dF, 0.0)) / float(nBins)
                    out.append(f32(math.sqrt(d)) if d > 0.0 else f32(0))
                myA = seq(dM * dM) if (o["flux"] or o["flux_centroid"]) else f64(0)
                myAf = seq(dM * dM * S["ax_m"][lo:hi + 1]) if o["flux_centroid"] else f64(0)
                if o["flux"]:
                    fl = myA / float(nBins)
                    out.append(f32(math.sqrt(fl)) if fl > 0.0 else f32(0))
                if o["flux_centroid"] or o["flux_at_flux_centroid"]:
                    fc = myAf / myA if myA > 0.0 else 0.0
                    if o["flux_centroid"]:
                        out.append(f32(fc))
                    if o["flux_at_flux_centroid"]:
                        ge = np.nonzero(S["ax_m"][lo:hi + 1] >= fc)[0]
                        b = lo + int(ge[0]) if ge.size else hi
                        st, en = max(b - 2, lo), min(b + 2, hi)
                        dd = srcM[st:en + 1].astype(f64) - magP[st:en + 1].astype(f64)
                        out.append(f32(seq(dd * dd) / float(en - st + 1)))
        ctr = f32(0)
        sumA = f64(0)
        if any(o[k] for k in ("centroid", "standard_deviation", "variance", "skewness", "kurtosis", "slope")):   # :1256-1312
            sumA = seq(S["ax_c"][lo:hi + 1] * LP[lo:hi + 1])
            if sumB != 0.0:
                ctr = f32(sumA / sumB)
            if o["centroid"]:
                out.append(ctr)
        if o["max_pos"] or o["min_pos"]:                      # :1314-1330
            w = srcLP[lo:max(hi, lo + 1)]
            if o["max_pos"]:
                out.append(f32(S["ax_m"][lo + int(np.argmax(w))]))
            if o["min_pos"]:
                out.append(f32(S["ax_m"][lo + int(np.argmin(w))]))
        if o["entropy"]:                                      # smileStat_entropy (smileUtil.c:2079-2124)
            vals = srcLP[lo:hi + 1]
            V = vals.astype(f64)
            dn = seq(V)
            mn = min(f32(0), vals.min())
            if mn < 0:
                mf = 0.0000001 + float(mn)
                steps = np.empty(2 * V.size)
                steps[0::2] = np.where(V <= mf, mf - V, 0.0)
                steps[1::2] = -float(mn)
                dn = seq(steps, start=dn)
            else:
                mn = f32(0)
            if dn < float(f32(0.0000001)):
                dn = float(f32(0.0000001))
            v = (vals - mn).astype(f32).astype(f64)
            v = np.where(v <= 0.0000001, 0.0000001, v)
            ln = v / dn
            l2 = math.log(2.0)
            e = seq(np.array([x * math.log(x) / l2 for x in ln if x > 0.0]))
            out.append(f32(-e))
        if any(o[k] for k in ("standard_deviation", "variance", "skewness", "kurtosis")):   # :1338-1397
            t1 = S["ax_m"][lo:hi + 1] - float(ctr)
            m = t1 * t1 * LP[lo:hi + 1]
            m2 = seq(m)
            m = m * t1
            m3 = seq(m)
            m4 = seq(m * t1)
            sigma2 = m2 / sumB if sumB != 0.0 else 0.0
            if o["standard_deviation"]:
                out.append(f32(math.sqrt(sigma2)) if sigma2 > 0.0 else f32(0))
            if o["variance"]:
                out.append(f32(sigma2))
            if o["skewness"]:
                out.append(f32(0) if sigma2 <= 0.0 else f32(m3 / (sumB * sigma2 * math.sqrt(sigma2))))
            if o["kurtosis"]:
                out.append(f32(0) if sigma2 == 0.0 else f32(m4 / (sumB * sigma2 * sigma2)))
        if o["slope"]:                                        # :1399-1427
            Nind = float(nBins)
            deno = Nind * S["slope_S2f"] - S["slope_Sf"] * S["slope_Sf"]
            slope = (Nind * sumA - S["slope_Sf"] * sumB) / deno if deno != 0.0 else 0.0
            out.append(f32(slope * (Nind - 1.0)) if o["old_slope_scale"] else f32(slope))
        if o["sharpness"]:                                    # :1429-1478
            sumAA = seq((S["sharp"] * P[lo:hi + 1]).astype(f32), f32)
            c2 = f32(float(sumAA) / frameSum) if frameSum != 0.0 else f32(0)
            out.append(f32(0.11 * float(c2)))
        if o["harmonicity"]:                                  # :1484-1513
            x = srcLP
            peaks = []
            for j in range(lo + 2, hi - 1):
                if (x[j - 2] < x[j] and x[j - 1] < x[j] and x[j] > x[j + 1] and x[j] > x[j + 2]) or \
                   (x[j - 2] > x[j] and x[j - 1] > x[j] and x[j] < x[j + 1] and x[j] < x[j + 2]):
                    peaks.append(x[j])
            peaks = np.array(peaks, f32)
            ptp = seq(np.abs(peaks[1:] - peaks[:-1]).astype(f32), f32) if peaks.size > 1 else f32(0)
            ptp = f32(float(ptp) / 2.0)
            if o["norm_band_energies"] and sumB != 0.0:
                ptp = f32(ptp / f32(abs(sumB))) if use_log else f32(ptp / f32(frameSum))
            else:
                ptp = f32(ptp / f32(nBins))
            out.append(ptp)
        if o["flatness"]:                                     # :1515-1543
            sf = f32(0)
            if sumB != 0.0:
                nzv = srcLP[lo:hi + 1]
                nzv = nzv[nzv != 0]
                g = seq(logf_v(np.abs(nzv)), f32)
                if nzv.size > 0:
                    g = f32(g / f32(nzv.size))
                g = expf(g)
                sf = f32(g / f32(abs(sumB / float(nBins))))
            if o["log_flatness"]:
                out.append(logf(sf) if sf > 0 else f32(0))
            else:
                out.append(sf)
    res = np.zeros(n_out(o), f32)                             # (a first frame with more of the flux family on than one: the vector's
    res[:len(out)] = np.array(out, f32)                       # last slots keep their zeros)
    return res


def ref_rows(S, o, rows, prev=None):
    """the frames of one stream in order; prev: the stream's last frame before rows[0], or None"""
    res = np.zeros((len(rows), n_out(o)), f32)
    for t in range(len(rows)):
        res[t] = ref_row(S, o, rows[t], prev)
        prev = rows[t]
    return res


def bits_equal(a, b):
    a = np.ascontiguousarray(a, np.float32)
    b = np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | ((a == 0) & (b == 0))))


# ---- the instances of tests/conf/spectral_axis.conf, in the order of the HTK file's levels: name -> (reader level, options)
_MOM = dict(centroid=1, max_pos=1, min_pos=1, entropy=1, standard_deviation=1, variance=1, skewness=1, kurtosis=1, slope=1, harmonicity=1,
            flatness=1)
_B2 = ((250, 650), (1000, 4000))
CONF = {
    "logA": ("mag", opts(bands=_B2, slopes=((0, 500), (500, 1500), (1500, 3000)), freq_range=(0, 5000), use_log_spectrum=1, alpha_ratio=1,
                         hammarberg_index=1, **_MOM)),
    "logB": ("mag", opts(bands=_B2, slopes=((0, 500), (500, 1500), (1500, 3000)), freq_range=(300, 3400), use_log_spectrum=1, alpha_ratio=1,
                         hammarberg_index=1, **_MOM)),
    "norm": ("mag", opts(bands=_B2, rolloff=(0.5,), norm_band_energies=1, alpha_ratio=1, hammarberg_index=1, harmonicity=1, flux=1)),
    "newslope": ("mag", opts(slopes=((0, 1000),), old_slope_scale=0, slope=1, centroid=1)),
    "buggy": ("mag", opts(rolloff=(0.25, 0.5, 0.9), buggy_roll_off=1)),
    "power": ("mag", opts(bands=((250, 650),), rolloff=(0.9,), square_input=0, flux=1, spec_diff=1, centroid=1, entropy=1, flux_centroid=1)),
    "sbark": ("bark", opts(bands=_B2, rolloff=(0.5, 0.9), sharpness=1, centroid=1)),
    "smel": ("mel", opts(bands=_B2, rolloff=(0.5, 0.9), sharpness=1, centroid=1)),
    "gemaps": ("mag", opts(slopes=((0, 500), (500, 1500)), freq_range=(0, 5000), use_log_spectrum=1, norm_band_energies=1, alpha_ratio=1,
                           hammarberg_index=1, old_slope_scale=0)),
}
CONF_ORDER = tuple(CONF)
SCALED = {"bark": (BARK, 26), "mel": (MEL, 40)}              # the two cSpecScale levels: scale, nPointsTarget
GOLDEN_KEYS = ("u3_6400", "u10_4800", "u3_6400_44k")


def split_levels(y, K):
    """the columns of the conf's HTK file: the magnitude level, the two scaled levels, then one level per cSpectral instance"""
    out, c = {"mag": y[:, :K]}, K
    for name, (_, w) in SCALED.items():
        out[name] = y[:, c:c + w]
        c += w
    for name in CONF_ORDER:
        w = n_out(CONF[name][1])
        out[name] = y[:, c:c + w]
        c += w
    assert c == y.shape[1]
    return out


def level_axis(level, K, fs_sec):
    """the axis a level of the conf carries, as many points as cSpectral reads of it: cTransformFFT's F0 i (transformFft.cpp:102-117);
    cSpecScale copies ITS READER's axis through the forward transform (specScale.cpp:232-239: the source bins' frequencies on the
    target scale, not the target points), of which cSpectral reads the first Nsrc (:606-609)"""
    F0 = 1.0 / fs_sec
    if level == "mag":
        return np.arange(K, dtype=f64) * F0
    scale, n = SCALED[level]
    return np.array([fwd(F0 * float(i), scale, 0.0) for i in range(n)], f64)


def golden_case(golden, key, name):
    """(options, setup, input rows, the binary's output rows) of one instance in one golden run"""
    y = golden["out_" + key]
    K = int(golden["K_" + key])
    fs = float(golden["frame_size_sec_" + key])
    lv = split_levels(y, K)
    level, o = CONF[name]
    rows = lv[level]
    # frqScale comes from the WRITER level's meta data (:614-623), which cSpectral's own output level never has: linear
    S = ref_setup(o, rows.shape[1], fs, level_axis(level, K, fs))
    return o, S, rows, lv[name]


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "spectral_axis_synth.npz"))


@pytest.mark.parametrize("key", GOLDEN_KEYS)
@pytest.mark.parametrize("name", CONF_ORDER)
def test_restatement_equals_the_real_binary(golden, name, key):
    """the restatement on the binary's own input level gives the binary's cSpectral level, bit for bit"""
    o, S, rows, want = golden_case(golden, key, name)
    assert 2 <= rows.shape[0] <= 40
    got = ref_rows(S, o, rows)
    d = (got.view(np.uint32) != want.view(np.uint32)) & ~((got == 0) & (want == 0))
    assert not d.any(), f"{name} {key}: {d.sum()} cells, first {np.argwhere(d)[:5].tolist()}: {got[d][:5]} vs {want[d][:5]}"


# ---- the library's table builder against the restatement's setup
def lib_tables(o, K, fs_sec, frq=None, n_scale=None):
    """smilehip_spectral_axis_tables; raises Refused with the library's message"""
    from opensmile_amd import capi
    L = capi.load()
    kw = {k: v for k, v in o.items() if k not in ("bands", "slopes", "rolloff")}
    co = capi.spectral_axis_opts(o["bands"], o["rolloff"], o["slopes"], **kw)
    geo, edges, sums, sharp = np.zeros(12, np.int32), np.zeros((32, 5)), np.zeros(2), np.zeros(max(K, 4))
    fa = None if frq is None else np.ascontiguousarray(frq, f64)
    ns = (0 if fa is None else fa.size) if n_scale is None else n_scale
    rc = L.smilehip_spectral_axis_tables(C.byref(co), K, fs_sec, None if fa is None else fa.ctypes.data, ns, geo.ctypes.data, edges.ctypes.data,
                                         sums.ctypes.data, sharp.ctypes.data)
    if rc < 0:
        assert rc == -1                                      # SMILEHIP_ERR_INVALID
        raise Refused(L.smilehip_last_error().decode())
    assert rc == n_out(o) == L.smilehip_spectral_axis_opts_count(C.byref(co))
    return geo, edges, sums, sharp


def same_tables(o, K, fs_sec, frq=None):
    S = ref_setup(o, K, fs_sec, frq)
    geo, edges, sums, sharp = lib_tables(o, K, fs_sec, frq)
    assert geo[:7].tolist() == [S["lo"], S["hi"], int(S["axis"]), S["ar"][0], S["ar"][1], S["hb"][0], S["hb"][1]]
    ne = len(S["edges"])
    want = np.array(S["edges"], f64).reshape(ne, 5)
    assert np.array_equal(edges[:ne].view(np.uint64), want.view(np.uint64)), (edges[:ne], want)
    assert np.array_equal(sums.view(np.uint64), np.array([S["slope_Sf"], S["slope_S2f"]], f64).view(np.uint64))
    nb = S["hi"] - S["lo"] + 1
    assert np.array_equal(sharp[:nb].view(np.uint64), S["sharp"].view(np.uint64))


@pytest.mark.parametrize("K,fs", [(257, 0.032), (1025, 0.025 * 2048 / 1103), (513, 0.064)])
@pytest.mark.parametrize("name", CONF_ORDER)
def test_table_builder_on_the_conf_instances(name, K, fs):
    level, o = CONF[name]
    frq = level_axis(level, K, fs)
    same_tables(o, frq.size, fs, frq)


AXIS_FREE = opts(bands=((250, 650), (0, 90), (7000, 9000)), slopes=((0, 500), (500, 1500), (100, 130)), rolloff=(0.5,), alpha_ratio=1,
                 hammarberg_index=1, centroid=1, slope=1, sharpness=1, variance=1)


@pytest.mark.parametrize("K", [4, 9, 26, 257, 1025, 8193, 16385])
@pytest.mark.parametrize("ctr", [0, 1])
def test_table_builder_without_an_axis(K, ctr):
    """the index-based branches; the sharpness weights continue the centroid's running f (spectral.cpp:1261, :1291-1294, :1464-1466)"""
    o = dict(AXIS_FREE, centroid=ctr, slope=ctr, variance=ctr)
    same_tables(o, K, 0.032)


@pytest.mark.parametrize("scale,param", [(LIN, 0.0), (LOG, 2.0), (BARK, 0.0), (MEL, 0.0), (SEM, 27.5), (BAO, 0.0)])
def test_table_builder_sharpness_scales(scale, param):
    """the weights through the inverse-then-bark transforms for every scale a level's meta data can name"""
    fs = 0.032
    frq = np.array([fwd(float(i) / fs, scale, param) for i in range(1, 65)], f64)
    same_tables(opts(sharpness=1, frq_scale=scale, frq_scale_param=param, freq_range=(0, 0)), 64, fs, frq)


def test_table_builder_ranges():
    frq = np.arange(257, dtype=f64) / 0.032
    for rng in ((0, 5000), (300, 3400), (30, 31), (0, 100000), (4000, 100000), (31, 63)):
        same_tables(opts(flux=1, freq_range=rng), 257, 0.032, frq)
    S = ref_setup(opts(flux=1, freq_range=(30, 31)), 257, 0.032, frq)
    assert S["lo"] == S["hi"] == 0                             # 30 >= frq[0] = 0 and 31 > frq[0] only (frq[1] = 31.25): one bin
    S = ref_setup(opts(flux=1, freq_range=(0, 100000)), 257, 0.032, frq)
    assert (S["lo"], S["hi"]) == (0, 256)


REFUSALS = {
    "frq": dict(o=opts(flux=1), K=16, frq=np.array([0.0, 1, 2, 3, 3, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15])),
    "n_scale": dict(o=opts(flux=1), K=16, frq=np.arange(15.0)),
    "freqRange": dict(o=opts(flux=1, freq_range=(62, 62)), K=16, frq=np.arange(16.0) * 31.0),   # both edges ON bin 2: lower bin 2, upper bin 1
    "tonality": dict(o=opts(flux=1, tonality=1), K=16, frq=None),
    "specFloor": dict(o=opts(flux=1, use_log_spectrum=1, spec_floor=0.0), K=16, frq=None),
    "bands": dict(o=opts(bands=((650, 250),)), K=16, frq=None),
    "K": dict(o=opts(flux=1), K=3, frq=None),
    "K:": dict(o=opts(flux=1), K=(1 << 20) + 1, frq=None),
}


@pytest.mark.parametrize("what", list(REFUSALS))
def test_table_builder_refusals(what):
    """where the restatement refuses, the library refuses with SMILEHIP_ERR_INVALID and names the option"""
    c = REFUSALS[what]
    with pytest.raises(Refused):
        ref_setup(c["o"], c["K"], 0.032, c["frq"])
    with pytest.raises(Refused, match=what):
        lib_tables(c["o"], c["K"], 0.032, c["frq"])
