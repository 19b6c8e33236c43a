"""The per-component operators of include/smilehip.h ("frame-major with leading dimensions") as a registry, and a checker for
the strided-row contract -- what tests/test_gpu_operator_layouts.py runs on the device and tests/test_operator_layouts_host.py
checks without one.

One entry (Op) per entry point and option set:
  make(rng, n)       the input of n frames, a float32 matrix (n + halo rows; the columns [0, w_src) go to the device matrix the
                     leading dimension belongs to, anything behind them is a second input the entry's run uploads itself), at the
                     smallest product-relevant width: 400-sample frames, FFT 512, K = 257, 26 bands, 13 cepstra, p = 8 / 11
  run(env, x, ld_src, ld_dst, d_src, d_dst, n, state)
                     ONE call through capi.load() with these leading dimensions and device pointers; returns a dict of further
                     outputs (host arrays, n rows each) or None
  widths             (w_src, w_dst) in 32-bit words (a double is two)
  reference(x)       a plain CPU reference on the packed rows: the oracle's function where it has one, else a float32 / float64
                     numpy restatement of the reference lines the header cites
and how the result is held to the reference (`compare`): "bits" (both-zero counts as equal, as in the operators' own tests) or the
name of the documented allowance of the operator's existing test, imported from there.

The checker (padded, first_row_offset, unpadded, check_layout) is numpy only."""
import ctypes as C
import math
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
f32, f64 = np.float32, np.float64

# a NaN no kernel produces: quiet, negative, with a payload
SENTINEL = np.uint32(0xFFC5A5A5)

# entry points whose leading dimensions are held to this standard elsewhere, or that are no row operators
EXEMPT = {
    "smilehip_spectral_axis_op_frames": "tests/test_gpu_spectral_axis.py::run_op pads source and destination with NaN and asserts the "
                                        "destination's pad; pieces with carried state in the same file",
    "smilehip_spectral_op_frames": "tests/test_gpu_spectral_general.py pads the destination with NaN, asserts it and runs uneven pieces; "
                                   "the operator is the any-axis one (same kernel)",
    "smilehip_functionals_matrix": "not a row operator: one output vector per matrix, no destination stride; its source stride is held by "
                                   "tests/test_gpu_operator_layouts.py::test_functionals_matrix_strided_source",
    "smilehip_funcspec_matrix": "not a row operator: one output vector per matrix, no destination stride; its source stride is held by "
                                "tests/test_gpu_operator_layouts.py::test_functionals_matrix_strided_source",
}


# ------------------------------------------------------------------------------------------------ the checker (numpy only)
def _fill(poison):
    """the 32-bit pattern of a poison value given as a float or as a bit pattern (any integer type)"""
    if isinstance(poison, (int, np.integer)):
        return np.uint32(poison)
    return np.array([poison], f32).view(np.uint32)[0]


def _lead(ld, lead):
    """words in front of the first guard row: by default as many (1 .. 4) as put row 0 one float past a 16-byte boundary of an
    aligned allocation, so that no row of a packed matrix is aligned and the rows of an odd stride take every alignment"""
    return 1 + (-ld) % 4 if lead is None else lead


def padded(x, ld, poison, lead=None):
    """(buffer, view): the rows of x at stride ld with one guard row in front and one behind; row 0 starts one float past a
    16-byte boundary (lead = 0: no such shift, for destinations of doubles); pad, guards and lead hold `poison`. The buffer is
    float32, the view its rows x.shape[0] x ld."""
    x = np.ascontiguousarray(x)
    assert x.ndim == 2 and x.dtype.itemsize == 4 and ld >= x.shape[1]
    n, w = x.shape
    lead = _lead(ld, lead)
    buf = np.full(lead + (n + 2) * ld, _fill(poison), np.uint32)
    view = buf[lead + ld:lead + (n + 1) * ld].reshape(n, ld)
    view[:, :w] = x.view(np.uint32)
    buf = buf.view(f32)
    return buf, buf[lead + ld:lead + (n + 1) * ld].reshape(n, ld)


def first_row_offset(ld, lead=None):
    """words from the allocation's start to row 0 of a padded() buffer"""
    return _lead(ld, lead) + ld


def unpadded(buffer, ld, w, n, lead=None):
    """the in-width cells of a padded() buffer as uint32 [n, w]"""
    lead = _lead(ld, lead)
    b = np.ascontiguousarray(buffer).view(np.uint32)
    return b[lead + ld:lead + (n + 1) * ld].reshape(n, ld)[:, :w].copy()


def check_layout(dst_buffer, ld_dst, w_dst, n, packed, sentinel=SENTINEL, lead=None, rows_written=None):
    """A destination buffer that started as padded(.., sentinel) after a call with leading dimension ld_dst: every in-width cell
    equals `packed` (the packed call's rows) as uint32, every pad cell, both guard rows and the lead still hold the sentinel, no
    in-width cell does. rows_written < n (smilehip_pitch_smoother_rows writes written[u] rows per stream): the rows behind them
    hold the sentinel everywhere. Raises AssertionError."""
    b = np.ascontiguousarray(dst_buffer).view(np.uint32)
    s = np.uint32(sentinel)
    lead = _lead(ld_dst, lead)
    assert b.size == lead + (n + 2) * ld_dst, f"buffer of {b.size} words for {n} rows at stride {ld_dst}"
    m = n if rows_written is None else int(rows_written)
    want = np.ascontiguousarray(packed).view(np.uint32).reshape(m, w_dst)
    assert (b[:lead + ld_dst] == s).all(), "the guard row in front of the rows was written"
    assert (b[lead + (n + 1) * ld_dst:] == s).all(), "the guard row behind the rows was written"
    rows = b[lead + ld_dst:lead + (n + 1) * ld_dst].reshape(n, ld_dst)
    bad = np.argwhere(rows[:, w_dst:] != s)
    assert not len(bad), f"pad cells written, first at row {bad[0][0]} column {w_dst + bad[0][1]}"
    assert (rows[m:] == s).all(), f"rows behind the {m} written ones were touched"
    left = np.argwhere(rows[:m, :w_dst] == s)
    assert not len(left), f"{len(left)} in-width cells left unwritten, first at row {left[0][0]} column {left[0][1]}"
    diff = np.argwhere(rows[:m, :w_dst] != want)
    assert not len(diff), (f"{len(diff)} of {want.size} in-width cells differ from the packed call, first at row {diff[0][0]} "
                           f"column {diff[0][1]}: {rows[diff[0][0], diff[0][1]]:#010x} vs {want[diff[0][0], diff[0][1]]:#010x}")


# ------------------------------------------------------------------------------------------------ seeded rows
def special_rows(x, zero_fill=0.0):
    """the rows where kernels go wrong, written into a seeded matrix: all zero, exact zeros interleaved, constant"""
    n = x.shape[0]
    if n > 1:
        x[1] = zero_fill
    if n > 2:
        x[2, ::2] = zero_fill
    if n > 3:
        x[3] = x[3, 0] if x[3, 0] != 0 else 0.25
    return x


def noise(rng, n, w, scale=0.1):
    return special_rows((rng.standard_normal((n, w)) * scale).astype(f32))


def magnitudes(rng, n, K, period=16.0):
    """magnitude spectra with harmonic structure (a clear pitch peak), plus the special rows"""
    mag = np.abs(rng.standard_normal((n, K))).astype(f32) + f32(0.01)
    mag += (2.0 + 2.0 * np.cos(2 * np.pi * np.arange(K) / period)).astype(f32)
    return special_rows(mag)


def packed_spectra(rng, n, nfft):
    return special_rows((rng.standard_normal((n, nfft)) * 0.3).astype(f32))


def mel_rows(rng, n, nb, scale=3.0e8):
    """mel-band energies as the HTK-scaled power bank gives them"""
    return special_rows((np.abs(rng.standard_normal((n, nb))) * scale).astype(f32))


# ------------------------------------------------------------------------------------------------ the oracle's stage functions
def _orc():
    from oracle import lldo
    return lldo


class _Mel(C.Structure):
    _fields_ = [("K", C.c_long), ("n_bands", C.c_int), ("nLo", C.c_long), ("nHi", C.c_long), ("coef", C.POINTER(C.c_float)),
                ("chan_map", C.POINTER(C.c_long)), ("cfs", C.POINTER(C.c_float)), ("use_power", C.c_int), ("htk", C.c_int)]


class _Dct(C.Structure):
    _fields_ = [("n_bands", C.c_int), ("first", C.c_int), ("last", C.c_int), ("n_mfcc", C.c_int), ("htk", C.c_int),
                ("melfloor", C.c_float), ("costable", C.POINTER(C.c_float)), ("sintable", C.POINTER(C.c_float))]


class _Plp(C.Structure):
    _fields_ = [("n_bands", C.c_int), ("new_rasta", C.c_int), ("init", C.c_int), ("melfloor", C.c_float), ("compression", C.c_float),
                ("rasta_iir", C.c_float), ("rasta_fir", C.c_float * 5), ("eql", C.POINTER(C.c_float)), ("buf", C.POINTER(C.c_float))]


class _PitchState(C.Structure):
    _fields_ = [("lastPitch", C.c_float), ("lastlastPitch", C.c_float), ("glMeanPitch", C.c_float), ("onsFlag", C.c_int),
                ("pitchEnv", C.c_float)]


FSS_512 = 512 / 16000.0           # frameSizeSec of the 512-point spectrum level at 16 kHz
_mel_cache = {}


def mel_bank(K=257, fss=FSS_512):
    """the oracle's cMelspec bank of MFCC12_0_D_A.conf on a K-bin spectrum (kept for the process)"""
    key = (K, fss)
    if key not in _mel_cache:
        lldo = _orc()
        L, c = lldo.lib(), lldo.default_cfg()
        m = _Mel()
        L.lldo_mel_init.restype = C.c_int
        L.lldo_mel_init.argtypes = [C.c_void_p, C.c_long, C.c_double, C.c_int, C.c_float, C.c_float, C.c_int, C.c_int]
        assert L.lldo_mel_init(C.byref(m), K, fss, c.n_bands, c.lofreq, c.hifreq, c.use_power, c.mel_htk_compatible) == 1
        _mel_cache[key] = (m, c)
    return _mel_cache[key]


def band_hz(K=257, fss=FSS_512):
    """the band-centre metadata cMelspec writes (melspec.cpp:408-412), as oracle/lld_oracle_compare.c::lldo_plp_chain forms it"""
    m, c = mel_bank(K, fss)
    return np.array([700.0 * (math.exp(float(m.cfs[b]) / 1127.0) - 1.0) for b in range(1, c.n_bands + 1)], f64)


def _rows(fn, x, w_out, dtype=f32):
    x = np.ascontiguousarray(x, f32)
    out = np.zeros((x.shape[0], w_out), dtype)
    for i in range(x.shape[0]):
        fn(x[i], out[i])
    return out


def ref_preemphasis(x, k, de):
    L = _orc().lib()
    L.lldo_preemphasis.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.c_float, C.c_int]
    return _rows(lambda a, o: L.lldo_preemphasis(a.ctypes.data, o.ctypes.data, a.size, float(k), de), x, x.shape[1])


def ref_window(x):
    lldo = _orc()
    L, c = lldo.lib(), lldo.default_cfg()
    N = x.shape[1]
    w = np.zeros(N, f64)
    L.lldo_window_table(c.win_func, N, c.win_sigma, c.win_gain, w.ctypes.data)
    L.lldo_window_apply.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.c_void_p, C.c_double]
    return _rows(lambda a, o: L.lldo_window_apply(a.ctypes.data, o.ctypes.data, N, w.ctypes.data, c.win_offset), x, N)


def ref_rdft(x, isgn):
    """the reference's rdft network row by row (oracle/lld_oracle_fft.c, pinned on the real rdft by tests/test_ooura_fft.py)"""
    L = _orc().lib()
    out = np.ascontiguousarray(x, f32).copy()
    fp = C.POINTER(C.c_float)
    for r in range(out.shape[0]):
        assert L.lldo_ooura_rdft(C.c_int(out.shape[1]), C.c_int(isgn), out[r].ctypes.data_as(fp)) == 0
    return out


def ref_rfft(x, nfft, sym):
    pad = (nfft - x.shape[1]) // 2 if sym else 0
    p = np.zeros((x.shape[0], nfft), f32)
    p[:, pad:pad + x.shape[1]] = x
    return ref_rdft(p, 1)


def ref_irfft(x):
    nfft = x.shape[1]
    return ref_rdft(x, -1) * (f32(2.0) / f32(nfft))          # transformFft.cpp:196-216


def ref_fftmag(x):
    L = _orc().lib()
    L.lldo_fftmag.argtypes = [C.c_void_p, C.c_long, C.c_void_p]
    return _rows(lambda a, o: L.lldo_fftmag(a.ctypes.data, a.size, o.ctypes.data), x, x.shape[1] // 2 + 1)


def ref_melspec(x):
    L = _orc().lib()
    m, c = mel_bank(x.shape[1])
    L.lldo_melspec.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    return _rows(lambda a, o: L.lldo_melspec(C.byref(m), a.ctypes.data, o.ctypes.data), x, c.n_bands)


def dense_bank(K=257, nb=26):
    """a bank in the dense form (HFCC / custom bandwidths, melspec.cpp:240-389): overlapping triangles of seeded widths;
    (coef [nb x K], first / last bin of each band [2 nb])"""
    rng = np.random.default_rng(77)
    coef = np.zeros((nb, K), f32)
    rng_bins = np.zeros(2 * nb, np.int32)
    centres = np.linspace(4, K - 6, nb)
    for b in range(nb):
        half = int(rng.integers(3, 14))
        lo, hi = max(0, int(centres[b]) - half), min(K - 1, int(centres[b]) + half)
        n = np.arange(lo, hi + 1)
        coef[b, lo:hi + 1] = (1.0 - np.abs(n - centres[b]) / (half + 1.0)).astype(f32)
        rng_bins[2 * b], rng_bins[2 * b + 1] = lo, hi
    return coef, rng_bins


def ref_melspec_dense(x, n_lo=2, n_hi=250):
    """melspec.cpp:519-570 with a dense bank, power spectrum, HTK scaling: the float sum of (float)((double)p (double)coef), bin
    after bin (rows side by side)"""
    coef, rb = dense_bank(x.shape[1])
    p = (x * x).astype(f32)
    out = np.zeros((x.shape[0], coef.shape[0]), f32)
    for b in range(coef.shape[0]):
        acc = np.zeros(x.shape[0], f32)
        for n in range(max(int(rb[2 * b]), n_lo), min(int(rb[2 * b + 1]) + 1, n_hi)):
            acc = (acc + (p[:, n].astype(f64) * f64(coef[b, n])).astype(f32)).astype(f32)
        out[:, b] = acc * f32(32767.0 * 32767.0)
    return out


def ref_mfcc(x):
    lldo = _orc()
    L, c = lldo.lib(), lldo.default_cfg()
    d = _Dct()
    L.lldo_mfcc_init.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, C.c_float]
    L.lldo_mfcc_init(C.byref(d), c.n_bands, c.first_mfcc, c.last_mfcc, c.cep_lifter, c.mfcc_htk_compatible, c.melfloor)
    L.lldo_mfcc.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    out = _rows(lambda a, o: L.lldo_mfcc(C.byref(d), a.ctypes.data, o.ctypes.data), x, c.last_mfcc - c.first_mfcc + 1)
    L.lldo_mfcc_free.argtypes = [C.c_void_p]
    L.lldo_mfcc_free(C.byref(d))
    return out


def ref_mfcc_inverse(x, do_log):
    lldo = _orc()
    c = lldo.default_cfg()
    return lldo.mfcc_inverse_rows(x, c.first_mfcc, c.last_mfcc, c.n_bands, c.cep_lifter, c.mfcc_htk_compatible, do_log)


def ref_sumsq(x):
    """energy.cpp:152-161: the float product added to a double, sample after sample"""
    out = np.zeros((x.shape[0], 1), f64)
    sq = (x * x).astype(f32).astype(f64)
    for i in range(x.shape[1]):
        out[:, 0] += sq[:, i]
    return out


def ref_zcr_count(x):
    """mzcr.cpp:117-124"""
    a, b, c = x[:, :-2], x[:, 1:-1], x[:, 2:]
    return ((((a * c <= 0) & (b == 0)) | (a * b < 0)).sum(axis=1)).astype(np.int32).reshape(-1, 1)


def ref_acf(x, cepstrum):
    L = _orc().lib()
    K = x.shape[1]
    L.lldo_acf.restype = None
    L.lldo_acf.argtypes = [C.c_void_p, C.c_long, C.c_int, C.c_void_p]
    return _rows(lambda a, o: L.lldo_acf(a.ctypes.data, K, cepstrum, o.ctypes.data), x, K - 1)


PITCH_FS_SEC, PITCH_MAX = float(f32(0.032)), 500.0      # fsSec is a float in cPitchACF (pitchACF.hpp)


def ref_pitchacf(x):
    """pitchACF.cpp:137-192 per row, a fresh contour state each (the per-frame analysis has none): voicing probability and F0raw"""
    L = _orc().lib()
    n = x.shape[1] // 2
    L.lldo_pitch_acf.restype = None
    L.lldo_pitch_acf.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.c_float, C.c_double, C.c_double, C.POINTER(_PitchState),
                                 C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float)]
    L.lldo_pitch_state_init.argtypes = [C.POINTER(_PitchState)]
    voicing, raw = np.zeros((x.shape[0], 1), f64), np.zeros(x.shape[0], f32)
    x = np.ascontiguousarray(x, f32)
    for f in range(x.shape[0]):
        st = _PitchState()
        L.lldo_pitch_state_init(C.byref(st))
        vp, f0, r = C.c_float(), C.c_float(), C.c_float()
        L.lldo_pitch_acf(x[f].ctypes.data, x[f, n:].ctypes.data, n, PITCH_FS_SEC, PITCH_MAX, 0.0, C.byref(st), C.byref(vp), C.byref(f0),
                         C.byref(r))
        voicing[f, 0], raw[f] = vp.value, r.value
    return voicing, {"f0raw": raw}


def ref_pitchacf_zcr(x):
    """the second result of voicingProb (pitchACF.cpp:249-283): the zero- or mean-crossing rate of the ACF"""
    n = x.shape[1]
    skip = int(1.0 / (PITCH_MAX * (PITCH_FS_SEC / (2 * n))))
    out = np.zeros((x.shape[0], 1), f64)
    for f, a in enumerate(x):
        zcr = int((a[:-1] * a[1:] < 0).sum())
        mean = f64(a[skip])
        for i in range(max(skip, 1), n):
            mean += f64(a[i])
        mean /= f64(n - skip + 1)
        d = a.astype(f64) - mean
        mcr = int((d[:-1] * d[1:] < 0).sum())
        out[f, 0] = (f64(mcr) if mcr > zcr else f64(zcr)) / f64(n)
    return out


def ref_valbased(x, idx, threshold, invert, allow_equal, zero_vec, remove_idx, output_val):
    """valbasedSelector.cpp:139-247, fixed threshold"""
    N = x.shape[1]
    i = min(idx, N - 1)
    v = x[:, i]
    copy = ((v < threshold) if invert else (v > threshold)) | ((v == threshold) if allow_equal else False)
    rows = np.delete(x, i, axis=1) if remove_idx else x.copy()
    rows[~copy] = f32(output_val)
    return rows, {"keep": np.where(copy, 1, 2 if zero_vec else 0).astype(np.int32)}


COMPARE_BANDS = ((250, 650), (1000, 4000))
COMPARE_FLAGS = dict(flux=1, centroid=1, entropy=1, variance=1, skewness=1, kurtosis=1, slope=1, sharpness=1, harmonicity=1)


def ref_spectral_compare(x, fss):
    return _orc().spectral_general_rows(x, fss, COMPARE_BANDS, (0.25, 0.5, 0.75, 0.9), **COMPARE_FLAGS)


def _libm():
    m = C.CDLL("libm.so.6")
    for name in ("logf", "expf", "sinf"):
        fn = getattr(m, name)
        fn.restype, fn.argtypes = C.c_float, [C.c_float]
    return m


def _map_f32(fn, a):
    return np.array([fn(float(v)) for v in np.asarray(a, f32).ravel()], f32).reshape(np.shape(a))


def plp_setup(rasta):
    """cPlp::initTables for the auditory spectrum (plp.cpp:335-402) from the oracle: (eql [26], rasta_coef [6], melfloor, compression)"""
    L = _orc().lib()
    hz = band_hz()
    p = _Plp()
    L.lldo_plp_init.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_double]
    L.lldo_plp_init(C.byref(p), len(hz), hz.ctypes.data, 1 if rasta else 0, 0.01)
    eql = np.array([p.eql[i] for i in range(len(hz))], f32)
    coef = np.array([p.rasta_iir] + list(p.rasta_fir), f32)
    return p, eql, coef, float(p.melfloor), float(p.compression)


def ref_plp_audspec(x, rasta):
    """rasta 0 / 1: the oracle's lldo_plp_audspec over the rows of one stream. rasta 2, the older RASTA form the oracle does not
    hold: plp.cpp:434-517 restated in float32 -- the five-frame ring, the IIR on the previous output, zeros for the first five
    frames -- with the C library's own logf / expf"""
    L = _orc().lib()
    p, eql, coef, melfloor, compression = plp_setup(rasta)
    if rasta != 2:
        L.lldo_plp_audspec.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        out = _rows(lambda a, o: L.lldo_plp_audspec(C.byref(p), a.ctypes.data, o.ctypes.data), x, x.shape[1])
    else:
        m = _libm()
        n, nb = x.shape
        ring, iir, init, ptr = np.zeros((nb, 5), f32), np.zeros(nb, f32), 0, 0
        out = np.zeros((n, nb), f32)
        fl = f32(melfloor)
        for t in range(n):
            s = _map_f32(m.logf, np.where(x[t] < fl, fl, x[t]))
            ring[:, ptr] = s
            acc = (coef[1] * s).astype(f32)
            for k in range(1, 5):
                acc = (acc + (coef[1 + k] * ring[:, (5 - k + ptr) % 5]).astype(f32)).astype(f32)
            acc = (acc + (coef[0] * iir).astype(f32)).astype(f32)
            iir = acc
            s = acc if init >= 5 else np.zeros(nb, f32)
            if init < 5:
                init += 1
            ptr = (ptr + 1) % 5
            s = ((s + eql).astype(f32) * f32(compression)).astype(f32)
            out[t] = _map_f32(m.expf, s)
    L.lldo_plp_free.argtypes = [C.c_void_p]
    L.lldo_plp_free(C.byref(p))
    return out


PLP_ORDER, PLP_COMPRESSION, PLP_LIFTER = 8, float(f32(0.33)), 22


def plp_cc_tables(nb=26, lp_order=PLP_ORDER, lifter=PLP_LIFTER):
    """cPlp::initTables for the HTK cepstral mode (plp.cpp:288-334; smileDsp_equalLoudnessWeight_htk, smileUtil.c:1056-1062):
    (eql [nb], cos [(lp_order + 1) x (nb + 2)], lifter [lp_order + 1])"""
    hz = band_hz()
    f2 = hz * hz
    fs = f2 / (f2 + 1.6e5)
    eql = (fs * fs * ((f2 + 1.44e6) / (f2 + 9.61e6))).astype(f32)
    n_freq, n_auto = nb + 2, lp_order + 1
    a = float(f32(math.pi) / f32(n_freq - 1))
    cos = np.zeros((n_auto, n_freq), f32)
    for i in range(n_auto):
        cos[i, 0] = 1.0
        for m in range(1, n_freq - 1):
            cos[i, m] = f32(2.0 * math.cos(a * float(i) * float(m)))
        cos[i, n_freq - 1] = f32(math.cos(a * float(i) * float(n_freq - 1)))
    lm = _libm()
    Lf = f32(lifter)
    sin = np.array([f32(1.0) + Lf / f32(2.0) * f32(lm.sinf(float(f32(math.pi) * f32(i) / Lf))) for i in range(n_auto)], f32)
    return eql, cos, sin


def ref_plp_stage(x, stage):
    return _orc().plp_stage_rows(x, band_hz(), PLP_ORDER, PLP_COMPRESSION, stage, PLP_LIFTER)


def _delta_ref():
    from test_gpu_option_sets import _delta_ref as fn         # cDeltaRegression::processBuffer in float32 (deltaRegression.cpp:104-170)
    return fn


def delta_norm(W):
    return f32(2.0) * f32(sum(i * i for i in range(1, W + 1)))


def ref_window_op_block(x, op, W, flags=0):
    """a cWindowProcessor block, element row by element row (windowProcessor.cpp:171-236): x holds max(W, 1) frames before frame 0
    and W behind the last one. op 0: deltaRegression.cpp:104-170, op 1: contourSmoother.cpp:106-114, op 2: :91-104 (noZeroSma)"""
    pre = max(W, 1)
    n = x.shape[0] - pre - W
    out = np.zeros((n, x.shape[1]), f32)
    for c in range(x.shape[1]):
        col = np.ascontiguousarray(x[:, c])
        if op == 0:
            out[:, c], _ = _delta_ref()(col, pre, n, W, flags, delta_norm(W) if W > 0 else f32(1.0))
            continue
        for t in range(n):
            k = pre + t
            if op == 2 and col[k] == 0.0:
                continue
            v, cnt = col[k], 1
            for w in range(1, W + 1):
                for u in (col[k - w], col[k + w]):
                    if op == 1 or u != 0.0:
                        v = f32(v + u)
                        cnt += 1
            out[t, c] = f32(v / f32(2 * W + 1 if op == 1 else cnt))
    return out


def ref_delta_segments(x, W, flags=0):
    """onlyInSegments (deltaRegression.cpp:121-137) over a block of one-frame ticks: the divisor grows with every pair used, tick
    after tick, element after element; it starts at 2 sum i^2 (:77-79)"""
    pre = max(W, 1)
    n = x.shape[0] - pre - W
    out = np.zeros((n, x.shape[1]), f32)
    norm = delta_norm(W)
    cols = [np.ascontiguousarray(x[:, c]) for c in range(x.shape[1])]
    for t in range(n):
        for c, col in enumerate(cols):
            y, norm = _delta_ref()(col, pre + t, 1, W, flags | 8, norm)
            out[t, c] = y[0]
    return out


F0_K, F0_FSS = 513, 1024 / 16000.0     # the spectrum of ComParE_2016's 60 ms frames


def ref_specscale(x):
    return _orc().specscale_shs_rows(x, F0_FSS)[0]


def ref_pitchshs(x):
    """cPitchShs on octave-scale rows (the oracle's lldo_pitch_shs with ComParE_2016's options)"""
    lldo = _orc()
    L = lldo.lib()
    s, h = lldo._SpecScale(), lldo._Shs()
    L.lldo_specscale_init.restype = C.c_int
    L.lldo_specscale_init.argtypes = [C.c_void_p, C.c_long, C.c_double]
    assert L.lldo_specscale_init(C.byref(s), x.shape[1], F0_FSS) == 1
    L.lldo_shs_init.restype = None
    L.lldo_shs_init.argtypes = [C.c_void_p, C.c_void_p]
    L.lldo_shs_init(C.byref(h), C.byref(s))
    L.lldo_pitch_shs.restype = None
    L.lldo_pitch_shs.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    out = _rows(lambda a, o: L.lldo_pitch_shs(C.byref(h), a.ctypes.data, o.ctypes.data, None), x, 21)
    L.lldo_specscale_free.argtypes = [C.c_void_p]
    L.lldo_specscale_free(C.byref(s))
    return out


SPECSCALE_OPS = {            # scale, param, min_f, max_f, n_points_target, enhance, smooth, weighting (tests/test_specscale_general_host.py)
    "log2": ("log", 2.0, 25.0, -1.0, 0, 1, 1, 1),
    "mel": ("mel", 0.0, 25.0, -1.0, 0, 1, 1, 0),
}


def ref_specscale_op(x, which):
    from test_specscale_general_host import SCALES, ref_rows, ref_tables
    scale, param, min_f, max_f, npt, enh, smo, wgt = SPECSCALE_OPS[which]
    T = ref_tables(SCALES[scale], param, min_f, max_f, npt, x.shape[1], FSS_512, wgt)
    return ref_rows(T, x, enh, smo)


RESAMPLE = dict(n_in=512, fs_sec=512 / 16000.0, last=320 / 16000.0, bp=1.0 / 16000.0, target=11000.0)     # 20 ms frames at 16 kHz -> 220 samples at 11 kHz


def ref_specresample_table(x):
    r = RESAMPLE
    return _orc().specresample_rows(x, r["fs_sec"], r["last"], r["bp"], r["target"])


def stable_lpc(rng, n, p):
    """LP coefficient sets from random reflection coefficients (stable), a few arbitrary ones (roots missing), the special rows"""
    rows = []
    for _ in range(n):
        k = rng.uniform(-0.95, 0.95, p)
        a = np.zeros(0)
        for m in range(p):
            a = np.concatenate([a + k[m] * a[::-1], [k[m]]])
        rows.append(a)
    x = np.array(rows, f32)
    if n > 4:
        x[4] = (rng.standard_normal(p) * 2).astype(f32)
    return special_rows(x)


def golden_rows(prefix, width, n, start=0):
    g = np.load(os.path.join(ROOT, "tests", "golden", "egemaps_lld_synth.npz"))
    rows = np.concatenate([g[k].reshape(-1, width) for k in sorted(g.files) if k.startswith(prefix) and g[k].size], axis=0)
    assert start + n <= len(rows)
    return np.ascontiguousarray(rows[start:start + n], f32)


def formant_lpc_rows(rng, n):
    """the real binary's LP rows of the golden eGeMAPS cases (silence -- all-zero rows -- included: the first rows), with a NaN row
    and a NaN coefficient, which make the QR iteration give up (the root carry). Finite or NaN only: +-inf would not end."""
    x = golden_rows("lpc_", 11, n, start=96)
    assert (x[0] == 0).all() or n < 2
    if n > 4:
        x[n // 2] = np.nan
        x[n - 2, 5] = np.nan
    assert (np.isfinite(x) | np.isnan(x)).all()
    return x


def harmonics_rows(rng, n):
    """[formants (10) | F0 (1) | magnitudes of the 60 ms frame (513)]: voiced and unvoiced frames, the binary's formant rows"""
    fm = golden_rows("formants_", 10, n, start=300)
    f0 = rng.uniform(80.0, 400.0, (n, 1)).astype(f32)
    f0[rng.random(n) < 0.3] = 0.0
    mag = magnitudes(rng, n, F0_K, period=13.0)
    if n > 1:
        f0[1] = 150.0                                     # a voiced frame on the all-zero spectrum
    return np.ascontiguousarray(np.concatenate([fm, f0, mag], axis=1), f32)


def ref_harmonics(x):
    return _orc().egemaps_harmonics_rows(x[:, 10], x[:, :10], x[:, 11:])


VOP_ELEMENTWISE = (("add", 0.37), ("mul", -2.5), ("log", 1.0), ("lgA", 10.0), ("sqr", 1.0), ("ee", 1.0), ("abs", 1.0), ("dBp", 1.0), ("dBv", 1.0))
VOP_REDUCE = ("sum", "ssm", "ll1", "ll2")


def vecop_rows_in(rng, n, w=26):
    x = (rng.standard_normal((n, w)) * 3).astype(f32)
    x[0, :7] = [0.0, -0.0, 1e-13, 1e-12, 1e-30, 88.0, -104.0]
    return special_rows(x)


def smoother_cands(rng, n, c=6):
    from test_is10_ops_host import random_cands
    return random_cands(rng, n, c)


# ------------------------------------------------------------------------------------------------ the device side
class Env:
    """what a run needs: torch, capi, the library, one context, and the plans / operators / tables the entries share"""

    def __init__(self):
        import torch
        from opensmile_amd import capi
        self.torch, self.capi, self.L = torch, capi, capi.load()
        self.ctx = capi.Context(0)
        self.h = self.ctx._h
        self._kept = {}

    def keep(self, key, make):
        if key not in self._kept:
            self._kept[key] = make()
        return self._kept[key]

    def dev(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a)).cuda()

    def plan(self, kind):
        capi = self.capi

        def make():
            if kind == "mfcc":
                return capi.Plan(self.ctx)
            if kind == "egemaps":
                return capi.Plan(self.ctx, capi.egemapsv02_config())
            if kind == "f0":
                return capi.Plan(self.ctx, capi.compare16_f0_config())
            cfg = capi.mfcc12_0_d_a_config()
            cfg.n_delta = 0
            if kind.startswith("fft"):                        # a transform-only plan of this frame = FFT length
                cfg.force_frame_size = int(kind[3:])
                cfg.stage_mask = capi.STAGE_FFT
            elif kind.startswith("spectral"):                 # what the plugin's cSpectral override builds for a K-bin level
                K = int(kind[8:])
                cfg.force_frame_size = (K - 1) * 2
                cfg.stage_mask = 16                           # SMILEHIP_STAGE_SPECTRAL
                cfg.force_fft_frame_size_sec = (K - 1) * 2 / 16000.0
            else:
                raise KeyError(kind)
            return capi.Plan(self.ctx, cfg)
        return self.keep(("plan", kind), make)

    def check(self, rc):
        if rc == -3:                                          # SMILEHIP_ERR_HIP: nothing more is started on a device that reported an error
            import pytest
            pytest.exit("HIP error: " + self.L.smilehip_last_error().decode(), returncode=3)
        self.capi._check(rc)

    def sync(self):
        try:
            self.torch.cuda.synchronize()
        except RuntimeError as e:
            import pytest
            pytest.exit(f"HIP error at synchronize: {e}", returncode=3)


class Op:
    def __init__(self, name, fn, make, run, widths, reference, compare="bits", stateful=False, new_state=None, halo=(0, 0),
                 dst_dtype=f32, dst_fixed=False, rows_written=None, src_flat=False, take=None, base_rows=129, quirk=None, kind=None):
        self.name, self.fn, self.make, self.run, self.widths, self.reference = name, fn, make, run, widths, reference
        self.compare, self.stateful, self.new_state, self.halo = compare, stateful, new_state, halo
        self.dst_dtype, self.dst_fixed, self.rows_written, self.src_flat = dst_dtype, dst_fixed, rows_written, src_flat
        self.take = take or (lambda x, m: x[:m + halo[0] + halo[1]])
        self.base_rows, self.quirk = base_rows, quirk
        self.kind = kind or ("restatement" if reference.__name__.startswith("ref_") and reference.__module__ == __name__ else "oracle")

    def __repr__(self):
        return self.name


REGISTRY = []


def op(name, fn, make, run, widths, reference, **kw):
    REGISTRY.append(Op(name, "smilehip_" + fn, make, run, widths, reference, **kw))


def _simple(fn_name, handle, pre=(), post=()):
    """run() of the common shape fn(handle, *pre, d_src, ld_src, d_dst, ld_dst, n, *post, stream)"""
    def run(env, x, ld_src, ld_dst, d_src, d_dst, n, state):
        h = handle(env)
        env.check(getattr(env.L, "smilehip_" + fn_name)(h, *pre, d_src, ld_src, d_dst, ld_dst, n, *post, None))
    return run


def _plan(kind):
    return lambda env: env.plan(kind)._h


N, NFFT, K, NB, NC = 400, 512, 257, 26, 13

# ---- R1 framing: the source is ONE row of samples, not a matrix (no ld_src)
def _run_frame_rows(env, x, ld_src, ld_dst, d_src, d_dst, n, state):
    env.check(env.L.smilehip_frame_rows(env.h, d_src, N, 160, n, d_dst, ld_dst, None))


def ref_frame_rows(x):
    """winToVecProcessor.cpp:1037-1052: frame f = samples [f step, f step + size)"""
    s = x.ravel()
    n = (s.size - N) // 160 + 1
    return np.stack([s[f * 160:f * 160 + N] for f in range(n)])


def _make_samples(rng, n):
    s = (rng.standard_normal((1, (n - 1) * 160 + N)) * 0.1).astype(f32)
    s[0, 160:320] = 0.0
    return s


op("frame_rows", "frame_rows", _make_samples, _run_frame_rows, (1, N), ref_frame_rows, src_flat=True,
   take=lambda x, m: x[:, :(m - 1) * 160 + N])

# ---- R2, R3
for de in (0, 1):
    op(f"preemphasis_de{de}", "preemphasis_frames", lambda rng, n: noise(rng, n, N),
       (lambda de: lambda env, x, ls, ld, s, d, n, st: env.check(env.L.smilehip_preemphasis_frames(env.h, s, ls, d, ld, n, N, float(f32(0.97)), de, None)))(de),
       (N, N), (lambda de: lambda x: ref_preemphasis(x, f32(0.97), de))(de), kind="oracle")
op("window", "window_frames", lambda rng, n: noise(rng, n, N), _simple("window_frames", _plan("mfcc")), (N, N), ref_window, kind="oracle")

# ---- R4: 512 points from 400 samples (one wave per frame), 256 points (the block form)
op("rfft_512", "rfft_frames", lambda rng, n: noise(rng, n, N), _simple("rfft_frames", _plan("mfcc")), (N, NFFT),
   lambda x: ref_rfft(x, NFFT, _orc().default_cfg().zero_pad_symmetric), kind="oracle")
op("rfft_256", "rfft_frames", lambda rng, n: noise(rng, n, 256), _simple("rfft_frames", _plan("fft256")), (256, 256),
   lambda x: ref_rfft(x, 256, 0), kind="oracle")
op("irfft_512", "irfft_frames", lambda rng, n: packed_spectra(rng, n, NFFT), _simple("irfft_frames", _plan("fft512")), (NFFT, NFFT), ref_irfft,
   kind="oracle")
op("irfft_256", "irfft_frames", lambda rng, n: packed_spectra(rng, n, 256), _simple("irfft_frames", _plan("fft256")), (256, 256), ref_irfft,
   kind="oracle")

# ---- R5
op("fftmag", "fftmag_frames", lambda rng, n: packed_spectra(rng, n, NFFT), _simple("fftmag_frames", _plan("mfcc")), (NFFT, K), ref_fftmag,
   kind="oracle")


def _ref_magphase(flags):
    def ref(x):
        from test_gpu_option_sets import ref_magphase
        return ref_magphase(x, flags, 90.302, -29.698)
    return ref


for mode, flags in (("magnitude", 1), ("phase", 2), ("magnitude_phase", 3), ("power_dbpsd", 1 | 8 | 16)):
    w = (K if flags & 1 else 0) + (K if flags & 2 else 0)
    op(f"fftmagphase_{mode}", "fftmagphase_frames", lambda rng, n: packed_spectra(rng, n, NFFT),
       (lambda flags: lambda env, x, ls, ld, s, d, n, st: env.check(env.L.smilehip_fftmagphase_frames(env.h, s, ls, NFFT, flags, 90.302, -29.698, d, ld, n, None)))(flags),
       (NFFT, w), _ref_magphase(flags), compare=("bits" if flags == 1 else ("magphase", flags)), kind="restatement")

# ---- R6
op("melspec", "melspec_frames", lambda rng, n: magnitudes(rng, n, K), _simple("melspec_frames", _plan("mfcc")), (K, NB), ref_melspec, kind="oracle")


def _run_melspec_table(dense):
    def run(env, x, ls, ld, s, d, n, st):
        def tables():
            if dense:
                coef, chan = dense_bank(K)
                return env.dev(coef), env.dev(chan), 2, 250
            m, c = mel_bank(K)
            assert c.use_power == 1 and c.mel_htk_compatible == 1
            coef = np.array([m.coef[i] for i in range(K)], f32)
            chan = np.array([m.chan_map[i] for i in range(K)], np.int32)
            return env.dev(coef), env.dev(chan), int(m.nLo), int(m.nHi)
        d_coef, d_chan, n_lo, n_hi = env.keep(("meltab", dense), tables)
        env.check(env.L.smilehip_melspec_table_frames(env.h, s, ls, K, NB, dense, d_coef.data_ptr(), d_chan.data_ptr(), n_lo, n_hi, 1,
                                                      float(f32(32767.0 * 32767.0)), d, ld, n, None))
    return run


op("melspec_table_standard", "melspec_table_frames", lambda rng, n: magnitudes(rng, n, K), _run_melspec_table(0), (K, NB), ref_melspec, kind="oracle")
op("melspec_table_dense", "melspec_table_frames", lambda rng, n: magnitudes(rng, n, K), _run_melspec_table(1), (K, NB), ref_melspec_dense)


def _melinv_tables():
    return _orc().melspec_inverse_rows(np.zeros((1, NB), f32), K, FSS_512, 0.0, 8000.0, 1, 1, tables=True)[1]


def _run_melinv(env, x, ls, ld, s, d, n, st):
    def tables():
        n_lo, n_hi, coef, chan = _melinv_tables()
        return env.dev(coef), env.dev(chan), n_lo, n_hi
    d_coef, d_chan, n_lo, n_hi = env.keep("melinv", tables)
    env.check(env.L.smilehip_melspec_inverse_table_frames(env.h, s, ls, NB, K, d_coef.data_ptr(), d_chan.data_ptr(), n_lo, n_hi, 1,
                                                          float(f32(32767.0 * 32767.0)), d, ld, n, None))


def _make_melinv(rng, n):
    x = (rng.standard_normal((n, NB)) * 3.0e8).astype(f32)
    x[:max(n - 2, 1)] = np.abs(x[:max(n - 2, 1)])            # the last rows keep negative bands: the square root's other branch
    return special_rows(x)


op("melspec_inverse_table", "melspec_inverse_table_frames", _make_melinv, _run_melinv, (NB, K),
   lambda x: _orc().melspec_inverse_rows(x, K, FSS_512, 0.0, 8000.0, 1, 1), kind="oracle")

# ---- R7
op("mfcc", "mfcc_frames", lambda rng, n: mel_rows(rng, n, NB), _simple("mfcc_frames", _plan("mfcc")), (NB, NC), ref_mfcc, compare="mfcc_log",
   kind="oracle")
for do_log in (1, 0):
    op(f"mfcc_inverse_log{do_log}", "mfcc_inverse_frames", lambda rng, n: special_rows((rng.standard_normal((n, NC)) * 4).astype(f32)),
       _simple("mfcc_inverse_frames", _plan("mfcc"), post=(do_log,)), (NC, NB), (lambda dl: lambda x: ref_mfcc_inverse(x, dl))(do_log), kind="oracle")

# ---- R12: one double / one int per frame, no destination stride
op("sumsq", "sumsq_frames", lambda rng, n: noise(rng, n, N),
   lambda env, x, ls, ld, s, d, n, st: env.check(env.L.smilehip_sumsq_frames(env.h, s, ls, N, n, d, None)),
   (N, 2), ref_sumsq, dst_dtype=f64, dst_fixed=True, compare="sumsq")
op("zcr_count", "zcr_count_frames", lambda rng, n: noise(rng, n, N),
   lambda env, x, ls, ld, s, d, n, st: env.check(env.L.smilehip_zcr_count_frames(env.h, s, ls, N, n, d, None)),
   (N, 1), ref_zcr_count, dst_dtype=np.int32, dst_fixed=True)


def _ref_mzcr(x):
    from test_gpu_option_sets import ref_mzcr
    return ref_mzcr(x, 31)


_ref_mzcr.__name__ = "ref_mzcr"
op("mzcr_all", "mzcr_frames", lambda rng, n: noise(rng, n, N),
   lambda env, x, ls, ld, s, d, n, st: env.check(env.L.smilehip_mzcr_frames(env.h, s, ls, N, n, 31, d, ld, None)),
   (N, 6), _ref_mzcr, kind="restatement")

# ---- R9: K = 257 (one wave per frame) and K = 129 (the block form), ACF and cepstrum
for Kacf in (257, 129):
    for cep in (0, 1):
        op(f"acf_K{Kacf}_{'cepstrum' if cep else 'acf'}", "acf_frames", (lambda Kacf: lambda rng, n: magnitudes(rng, n, Kacf))(Kacf),
           (lambda Kacf, cep: lambda env, x, ls, ld, s, d, n, st: env.check(
               env.L.smilehip_acf_frames(env.plan(f"fft{2 * (Kacf - 1)}")._h, s, ls, d, ld, Kacf - 1, n, 1, cep, 1, 0, None)))(Kacf, cep),
           (Kacf, Kacf - 1), (lambda cep: lambda x: ref_acf(x, cep))(cep), compare="acf", kind="oracle")


# ---- R10
def _make_acf_ceps(rng, n):
    mag = magnitudes(rng, n, K)
    return np.ascontiguousarray(np.concatenate([ref_acf(mag, 0), ref_acf(mag, 1)], axis=1))


def _run_pitchacf(env, x, ls, ld, s, d, n, st):
    idx = env.torch.full((n + 2,), -77, dtype=env.torch.int32, device="cuda")
    env.check(env.L.smilehip_pitchacf_frames(env.h, s, ls, K - 1, n, PITCH_FS_SEC, PITCH_MAX, d, idx.data_ptr() + 4, None))
    env.sync()
    i = idx.cpu().numpy()
    assert i[0] == -77 and i[-1] == -77, "smilehip_pitchacf_frames wrote outside its n peak indices"
    return {"max_idx": i[1:-1].copy()}


op("pitchacf", "pitchacf_frames", _make_acf_ceps, _run_pitchacf, (2 * (K - 1), 2), ref_pitchacf, dst_dtype=f64, dst_fixed=True,
   compare="pitchacf", kind="oracle")
op("pitchacf_zcr", "pitchacf_zcr_frames", lambda rng, n: np.ascontiguousarray(_make_acf_ceps(rng, n)[:, :K - 1]),
   lambda env, x, ls, ld, s, d, n, st: env.check(env.L.smilehip_pitchacf_zcr_frames(env.h, s, ls, K - 1, n, PITCH_FS_SEC, PITCH_MAX, d, None)),
   (K - 1, 2), ref_pitchacf_zcr, dst_dtype=f64, dst_fixed=True)


# ---- cValbasedSelector: N <= 128 (64 threads) and N > 128 (256), with and without removeIdx; zeroVec = 1 so that every row is defined
def _valbased(Nv, remove):
    args = dict(idx=3, threshold=0.05, invert=0, allow_equal=1, zero_vec=1, remove_idx=remove, output_val=-2.5)

    def make(rng, n):
        x = noise(rng, n, Nv)
        if n > 4:
            x[4, 3] = f32(0.05)                               # the == side of allowEqual
        return x

    def run(env, x, ls, ld, s, d, n, st):
        keep = env.torch.full((n + 2,), -77, dtype=env.torch.int32, device="cuda")
        env.check(env.L.smilehip_valbased_select_frames(env.h, s, ls, Nv, n, args["idx"], args["threshold"], args["invert"], args["allow_equal"],
                                                        args["zero_vec"], remove, args["output_val"], d, ld, keep.data_ptr() + 4, None))
        env.sync()
        k = keep.cpu().numpy()
        assert k[0] == -77 and k[-1] == -77, "smilehip_valbased_select_frames wrote outside its n decisions"
        return {"keep": k[1:-1].copy()}

    def ref_valbased_rows(x):
        return ref_valbased(x, **{**args, "threshold": f32(args["threshold"])})
    ref_valbased_rows.__name__ = "ref_valbased"
    op(f"valbased_N{Nv}{'_remove' if remove else ''}", "valbased_select_frames", make, run, (Nv, Nv - remove), ref_valbased_rows,
       kind="restatement")


for Nv in (21, 257):
    for remove in (0, 1):
        _valbased(Nv, remove)


# ---- R11 with carried state: d_state = K floats, not read when first != 0
def _spectral_state(Ks):
    return lambda env: {"buf": env.torch.full((Ks,), float("nan"), dtype=env.torch.float32, device="cuda"), "first": 1}


def _run_spectral(fn, plan):
    def run(env, x, ls, ld, s, d, n, st):
        env.check(getattr(env.L, fn)(env.plan(plan)._h, s, ls, st["buf"].data_ptr(), st["first"], d, ld, n, None))
        st["first"] = 0
    return run


for Ks in (129, 257, 513):
    op(f"spectral_K{Ks}", "spectral_frames", (lambda Ks: lambda rng, n: magnitudes(rng, n, Ks))(Ks),
       _run_spectral("smilehip_spectral_frames", f"spectral{Ks}"), (Ks, 15),
       (lambda Ks: lambda x: ref_spectral_compare(x, (Ks - 1) * 2 / 16000.0))(Ks), stateful=True, new_state=_spectral_state(Ks), kind="oracle")
op("spectral_gemaps", "spectral_gemaps_frames", lambda rng, n: magnitudes(rng, n, K), _run_spectral("smilehip_spectral_gemaps_frames", "egemaps"),
   (K, 5), lambda x: _orc().egemaps_spectral_rows(x), stateful=True, new_state=_spectral_state(K), compare="egemaps_stage", kind="oracle")


# ---- R8
def _run_plp_audspec(rasta):
    def run(env, x, ls, ld, s, d, n, st):
        _, eql, coef, melfloor, compression = plp_setup(rasta)
        d_eql = env.keep(("plp_eql", rasta), lambda: env.dev(eql))
        rc = np.ascontiguousarray(coef, f32)
        env.check(env.L.smilehip_plp_audspec_frames(env.h, s, ls, NB, d_eql.data_ptr(), melfloor, compression, rasta,
                                                    rc.ctypes.data if rasta else None, st["buf"].data_ptr() if rasta else None, d, ld, n, None))
    return run


def _plp_state(rasta):
    # zeroed before a stream's first frame (the filter taps and the frame counter); 6 n_bands + 2 floats serve both forms
    return lambda env: {"buf": env.torch.zeros(6 * NB + 2, dtype=env.torch.float32, device="cuda")}


for rasta in (0, 1, 2):
    op(f"plp_audspec_rasta{rasta}", "plp_audspec_frames", lambda rng, n: mel_rows(rng, n, NB, 40.0), _run_plp_audspec(rasta), (NB, NB),
       (lambda r: lambda x: ref_plp_audspec(x, r))(rasta), stateful=rasta != 0, new_state=_plp_state(rasta) if rasta else None,
       kind="oracle" if rasta != 2 else "restatement")


def _plp_cc_dev(env):
    def make():
        eql, cos, sin = plp_cc_tables()
        return env.dev(eql), env.dev(cos), env.dev(sin)
    return env.keep("plp_cc", make)


def _run_plp_cc(env, x, ls, ld, s, d, n, st):
    e, c, sn = _plp_cc_dev(env)
    env.check(env.L.smilehip_plp_cc_frames(env.h, s, ls, NB, e.data_ptr(), 1.0, PLP_COMPRESSION, PLP_ORDER, c.data_ptr(), sn.data_ptr(), d, ld, n, None))


def _run_plp_stage(stage):
    def run(env, x, ls, ld, s, d, n, st):
        e, c, _ = _plp_cc_dev(env)
        env.check(env.L.smilehip_plp_stage_frames(env.h, s, ls, NB, e.data_ptr(), 1.0, PLP_COMPRESSION, PLP_ORDER, c.data_ptr(), stage, d, ld, n, None))
    return run


op("plp_cc", "plp_cc_frames", lambda rng, n: mel_rows(rng, n, NB), _run_plp_cc, (NB, PLP_ORDER + 1), lambda x: ref_plp_stage(x, 3), kind="oracle")
op("plp_stage1", "plp_stage_frames", lambda rng, n: mel_rows(rng, n, NB), _run_plp_stage(1), (NB, PLP_ORDER + 1), lambda x: ref_plp_stage(x, 1),
   kind="oracle")
op("plp_stage2", "plp_stage_frames", lambda rng, n: mel_rows(rng, n, NB), _run_plp_stage(2), (NB, PLP_ORDER), lambda x: ref_plp_stage(x, 2),
   kind="oracle")


# ---- R13 on blocks: the block holds max(W, 1) frames before frame 0 and W behind the last one
def _contour(rng, n, w=5):
    x = (rng.standard_normal((n, w)) * 0.5).astype(f32)
    x[rng.random((n, w)) < 0.25] = 0.0                        # "no value" stretches (unvoiced frames of an F0 contour)
    x[:, 1] = 0.0
    x[:, 2] = 0.75
    return x


for wop, W in ((0, 2), (1, 1), (2, 1)):
    pre = max(W, 1)
    op(f"window_op_block_op{wop}", "window_op_block", (lambda pre, W: lambda rng, n: _contour(rng, n + pre + W))(pre, W),
       (lambda wop, W: lambda env, x, ls, ld, s, d, n, st: env.check(env.L.smilehip_window_op_block(env.h, s, ls, d, ld, n, 5, wop, W, 0, None)))(wop, W),
       (5, 5), (lambda wop, W: lambda x: ref_window_op_block(x, wop, W))(wop, W), halo=(pre, W), kind="restatement")


def _run_delta_segments(env, x, ls, ld, s, d, n, st):
    env.check(env.L.smilehip_delta_segments_block(env.h, s, ls, d, ld, n, 1, 5, 2, 0, st["buf"].data_ptr(), None))


op("delta_segments_block", "delta_segments_block", lambda rng, n: _contour(rng, n + 4), _run_delta_segments, (5, 5),
   lambda x: ref_delta_segments(x, 2), halo=(2, 2), stateful=True, kind="restatement",
   new_state=lambda env: {"buf": env.torch.tensor([float(delta_norm(2))], dtype=env.torch.float32, device="cuda")})

# ---- the F0 group, per component (ComParE_2016's plan: 513 bins)
op("specscale", "specscale_frames", lambda rng, n: magnitudes(rng, n, F0_K, 13.0), _simple("specscale_frames", _plan("f0")), (F0_K, F0_K),
   ref_specscale, kind="oracle")
op("pitchshs", "pitchshs_frames", lambda rng, n: ref_specscale(magnitudes(rng, n, F0_K, 13.0)), _simple("pitchshs_frames", _plan("f0")), (F0_K, 21),
   ref_pitchshs, compare="pitchshs", kind="oracle")


def _run_specscale_op(which):
    def run(env, x, ls, ld, s, d, n, st):
        def make():
            from test_specscale_general_host import SCALES
            scale, param, min_f, max_f, npt, enh, smo, wgt = SPECSCALE_OPS[which]
            o = env.capi.specscale_opts(SCALES[scale], param, min_f, max_f, npt, enh, smo, wgt)
            h = C.c_void_p()
            env.check(env.L.smilehip_specscale_op_create(env.h, C.byref(o), K, FSS_512, C.byref(h)))
            assert env.L.smilehip_specscale_op_n_out(h) == K
            return h
        env.check(env.L.smilehip_specscale_op_frames(env.keep(("specscale_op", which), make), s, ls, d, ld, n, None))
    return run


for which in SPECSCALE_OPS:
    op(f"specscale_op_{which}", "specscale_op_frames", lambda rng, n: magnitudes(rng, n, K, 13.0), _run_specscale_op(which), (K, K),
       (lambda w: lambda x: ref_specscale_op(x, w))(which), kind="restatement")

# ---- GeMAPS components (an eGeMAPS plan) and their any-geometry forms
op("specresample", "specresample_frames", lambda rng, n: packed_spectra(rng, n, NFFT), _simple("specresample_frames", _plan("egemaps")), (NFFT, 220),
   lambda x: _orc().egemaps_specresample_rows(x), kind="oracle")


def _run_specresample_table(env, x, ls, ld, s, d, n, st):
    def make():
        r = RESAMPLE
        n_out, k_max, nd = C.c_int64(0), C.c_int64(0), C.c_double(0.0)
        env.check(env.L.smilehip_specresample_geometry(r["n_in"], r["fs_sec"], r["last"], r["bp"], r["target"], C.byref(n_out), C.byref(k_max),
                                                       C.byref(nd)))
        assert n_out.value == 220
        h = k_max.value // 2
        ct, st_ = np.zeros(h * n_out.value, f32), np.zeros(h * n_out.value, f32)
        env.check(env.L.smilehip_specresample_tables(r["n_in"], n_out.value, k_max.value, nd.value, ct.ctypes.data, st_.ctypes.data))
        return env.dev(ct), env.dev(st_), k_max.value
    d_ct, d_st, k_max = env.keep("specresample_table", make)
    env.check(env.L.smilehip_specresample_table_frames(env.h, s, ls, NFFT, 220, k_max, d_ct.data_ptr(), d_st.data_ptr(), d, ld, n, None))


op("specresample_table", "specresample_table_frames", lambda rng, n: packed_spectra(rng, n, NFFT), _run_specresample_table, (NFFT, 220),
   ref_specresample_table, kind="oracle")
op("lpc_p11", "lpc_frames", lambda rng, n: noise(rng, n, 220), _simple("lpc_frames", _plan("egemaps")), (220, 11),
   lambda x: _orc().egemaps_lpc_rows(x, 11), kind="oracle")
op("lpc_acf_p8", "lpc_acf_frames", lambda rng, n: noise(rng, n, 220),
   lambda env, x, ls, ld, s, d, n, st: env.check(env.L.smilehip_lpc_acf_frames(env.h, s, ls, 220, 8, d, ld, n, None)),
   (220, 8), lambda x: _orc().egemaps_lpc_rows(x, 8), kind="oracle")
op("lsp_p8", "lsp_frames", lambda rng, n: stable_lpc(rng, n, 8),
   lambda env, x, ls, ld, s, d, n, st: env.check(env.L.smilehip_lsp_frames(env.h, s, ls, 8, d, ld, n, None)),
   (8, 8), lambda x: _orc().lsp_rows(x), kind="oracle")
for flags in (1, 2, 3):
    # intensity.cpp:134: the Hamming-weighted sum runs over MIN(N, number of outputs) samples -- one or two; the oracle's
    # lldo_intensity_frame restates that line, so the quirk is in the reference
    op(f"intensity_flags{flags}", "intensity_frames", lambda rng, n: noise(rng, n, N, 0.2),
       (lambda flags: lambda env, x, ls, ld, s, d, n, st: env.check(env.L.smilehip_intensity_frames(env.h, s, ls, N, flags, d, ld, n, None)))(flags),
       (N, bin(flags).count("1")), (lambda flags: lambda x: _orc().intensity_rows(x, flags & 1, (flags >> 1) & 1))(flags), kind="oracle",
       quirk="reads min(N, n_out) samples (intensity.cpp:134), restated by the oracle")
for vop, p1 in VOP_ELEMENTWISE:
    op(f"vecop_{vop}", "vecop_frames", vecop_rows_in,
       (lambda vop, p1: lambda env, x, ls, ld, s, d, n, st: env.check(
           env.L.smilehip_vecop_frames(env.h, _orc().VOP[vop], p1, 0.0, s, ls, NB, d, ld, n, None)))(vop, p1),
       (NB, NB), (lambda vop, p1: lambda x: _orc().vecop_rows(x, vop, p1))(vop, p1), kind="oracle")
for vop in VOP_REDUCE:
    op(f"vecop_{vop}", "vecop_frames", vecop_rows_in,
       (lambda vop: lambda env, x, ls, ld, s, d, n, st: env.check(
           env.L.smilehip_vecop_frames(env.h, _orc().VOP[vop], 1.0, 0.0, s, ls, NB, d, ld, n, None)))(vop),
       (NB, 1), (lambda vop: lambda x: _orc().vecop_reduce_rows(x, vop).reshape(-1, 1))(vop), kind="oracle")


# ---- cPitchSmoother: one stream; the state (32 bytes) is not read when resume = 0
def _smoother(octc, simple, flags):
    w = bin(flags).count("1")
    skips = 1 if (simple and flags & 3) else 0               # the first frame yields no row (pitchSmoother.cpp:331)

    def run(env, x, ls, ld, s, d, n, st):
        wr = env.torch.full((3,), -77, dtype=env.torch.int64, device="cuda")
        env.check(env.L.smilehip_pitch_smoother_rows(env.h, 6, 0.7, octc, simple, flags, s, ls, None, 1, n, st["buf"].data_ptr(), st["resume"], d, ld,
                                                     wr.data_ptr() + 8, None))
        env.sync()
        wrote = wr.cpu().numpy()
        assert wrote[0] == -77 and wrote[2] == -77
        want = n - (skips if not st["resume"] else 0)
        assert wrote[1] == want, f"written = {wrote[1]} for {n} rows (resume {st['resume']}), expected {want}"
        st["resume"] = 1

    op(f"pitch_smoother_oct{octc}_simple{simple}_flags{flags}", "pitch_smoother_rows", smoother_cands, run, (18, w),
       lambda x: _orc().pitch_smoother_rows(x, 6, 0.7, octc, simple, flags), stateful=True, kind="oracle",
       new_state=lambda env: {"buf": env.torch.full((8,), float("nan"), dtype=env.torch.float32, device="cuda"), "resume": 0},
       rows_written=lambda n, first: n - (skips if first else 0))


_smoother(1, 1, 15)
_smoother(0, 0, 4 | 8)

# ---- cFormantLpc, cHarmonics
FORMANT_STATE_BYTES = 176
op("formantlpc_frames", "formantlpc_frames", formant_lpc_rows, _simple("formantlpc_frames", _plan("egemaps")), (11, 10),
   lambda x: _orc().egemaps_formant_rows(x), compare="bits_strict", kind="oracle")


def _run_formant_rows(env, x, ls, ld, s, d, n, st):
    env.check(env.L.smilehip_formantlpc_rows(env.plan("egemaps")._h, s, ls, d, ld, n, st["buf"].data_ptr(), st["resume"], None))
    st["resume"] = 1


op("formantlpc_rows", "formantlpc_rows", formant_lpc_rows, _run_formant_rows, (11, 10), lambda x: _orc().egemaps_formant_rows(x),
   compare="bits_strict", stateful=True, kind="oracle",
   new_state=lambda env: {"buf": env.torch.full((FORMANT_STATE_BYTES // 4,), float("nan"), dtype=env.torch.float32, device="cuda"), "resume": 0})


def _run_harmonics(env, x, ls, ld, s, d, n, st):
    """ld_formants is the padded one; the magnitudes get the same pad behind their 513 bins, F0 is one value per frame"""
    pad = ls - 10
    mag, _ = padded(x[:, 11:], F0_K + pad, float("nan"))
    d_mag, d_f0 = env.dev(mag), env.dev(x[:, 10])
    env.check(env.L.smilehip_harmonics_frames(env.plan("egemaps")._h, d_f0.data_ptr(), s, ls, d_mag.data_ptr() + 4 * first_row_offset(F0_K + pad),
                                              F0_K + pad, d, ld, n, None))
    env.sync()                              # d_mag / d_f0 live until the kernel has run


op("harmonics", "harmonics_frames", harmonics_rows, _run_harmonics, (10, 6), ref_harmonics, compare="egemaps_stage", kind="oracle")


# ------------------------------------------------------------------------------------------------ holding a result to its reference
def as_words(a, dtype):
    return np.ascontiguousarray(a, dtype).reshape(len(a), -1).view(np.uint32)


def compare(entry, got_words, ref, got_extra=None, ref_extra=None):
    """got_words: the packed call's rows as uint32 [n, w_dst]; ref: reference(x) (its rows, or (rows, further outputs)). Raises."""
    got = np.ascontiguousarray(got_words).view(entry.dst_dtype)
    ref = np.ascontiguousarray(ref, entry.dst_dtype).reshape(got.shape)
    how = entry.compare
    gw, rw = got_words, as_words(ref, entry.dst_dtype)

    def cells(mask):
        at = np.argwhere(~mask)
        return f"{entry.name}: {len(at)} of {mask.size} cells differ from the reference, first at {at[0].tolist()}: {got[tuple(at[0])]!r} vs {ref[tuple(at[0])]!r}"
    if how == "bits_strict":
        same = gw == rw
        assert same.all(), cells(same if gw.shape == got.shape else same.reshape(len(got), -1, 2).all(axis=2))
    elif how == "bits":                                       # both-zero counts as equal, as in the operators' own tests
        same = gw == rw
        if entry.dst_dtype == f64:
            same = same.reshape(len(got), -1, 2).all(axis=2)
        assert (same | ((got == 0) & (ref == 0))).all(), cells(same | ((got == 0) & (ref == 0)))
    elif isinstance(how, tuple) and how[0] == "magphase":
        from test_gpu_option_sets import check_magphase
        check_magphase(got, ref, how[1], K)
    elif how == "mfcc_log":                                   # libm's logf against the kernel's once-rounded double log
        from test_gpu_stages import MFCC_LOG_FRAME_ERR, MFCC_LOG_SAME_MIN
        same = (gw == rw).mean()
        scale = np.abs(ref).max(axis=1, keepdims=True)
        err = (np.abs(got.astype(f64) - ref) / np.maximum(scale, 1e-30)).max()
        print(f"{entry.name}: {same * 100:.2f}% bit-identical, worst per-frame-scaled error {err:.2e}")
        assert same > MFCC_LOG_SAME_MIN and err < MFCC_LOG_FRAME_ERR
    elif how == "sumsq":                                      # as tests/test_gpu_stages.py: the rms against the oracle's
        from test_gpu_stages import SUMSQ_RMS_TOL
        rms_g = np.sqrt(got[:, 0] / f32(N)).astype(f32).astype(f64)
        rms_r = np.sqrt(ref[:, 0] / f32(N)).astype(f32).astype(f64)
        assert (np.abs(rms_g - rms_r) <= SUMSQ_RMS_TOL * np.maximum(rms_g, 1e-30)).all()
    elif how == "acf":
        from test_gpu_stages import ACF_ROW_MAX_TOL
        assert np.abs(got - ref).max() <= ACF_ROW_MAX_TOL * np.abs(ref).max()
    elif how == "pitchacf":
        from test_gpu_stages import VOICING_PROB_TOL
        assert (np.abs(got[:, 0].astype(f32) - ref[:, 0].astype(f32)) <= VOICING_PROB_TOL).all()
        idx, raw = got_extra["max_idx"], ref_extra["f0raw"]
        t_samp = f32(PITCH_FS_SEC / (2 * (K - 1)))
        with np.errstate(divide="ignore"):
            mine = np.where(idx > 0, f32(1.0) / (idx.astype(f32) * t_samp), f32(0.0)).astype(f32)
        assert np.array_equal(mine, raw), np.argwhere(mine != raw)[:5]
        return
    elif how == "pitchshs":
        from test_gpu_stages import PITCHSHS_EXP_TOL, PITCHSHS_ROWS_SAME_MIN
        same = (gw == rw).all(axis=1)
        assert same.mean() >= PITCHSHS_ROWS_SAME_MIN, f"{int((~same).sum())} of {len(same)} rows differ"
        assert np.abs(got - ref).max() <= PITCHSHS_EXP_TOL * max(np.abs(ref).max(), 1.0)
    elif how == "egemaps_stage":
        from test_gpu_egemaps import STAGE_SCALED_TOL, scaled_err
        assert scaled_err(got, ref).max() <= STAGE_SCALED_TOL
    else:
        raise KeyError(how)
    if ref_extra:
        for k, v in ref_extra.items():
            assert np.array_equal(got_extra[k], v), f"{entry.name}: output {k} differs from the reference at {np.argwhere(got_extra[k] != v)[:5].ravel()}"
