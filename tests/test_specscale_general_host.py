"""cSpecScale on every target scale, host side: a float64 restatement of the reference's setup (cSpecScale::myFetchConfig /
setupNewNames / dataProcessorCustomFinalise, src/dsp/specScale.cpp:100-321; smileMath_cspline_init / smileMath_csplint_init,
src/smileutil/smileUtilSpline.c:138-153, 295-342) and of its per-row arithmetic (processVector, specScale.cpp:326-377;
smileDsp_specEnhanceSHS / smileDsp_specSmoothSHS, src/smileutil/smileUtil.c:1965-2014; smileMath_cspline / smileMath_csplint,
smileUtilSpline.c:155-211, 344-357) lives here: scalar libm calls (math.log / math.atan: the C library's), elementwise IEEE
double operations in the reference's order, the recurrences as Python loops. It is held bit-equal to what the real binary wrote
(tests/golden/specscale_general_synth.npz), and the library's table builder (smilehip_specscale_tables) is held bit-equal to it,
refusals included. tests/test_gpu_specscale_general.py runs the device operator against the same restatement."""
import ctypes as C
import math
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIN, LOG, BARK, MEL, SEM, BAO = 0, 1, 2, 3, 4, 7            # SPECTSCALE_* (src/include/smileutil/smileUtil.h:330-337)
SCALES = {"lin": LIN, "log": LOG, "bark": BARK, "mel": MEL, "sem": SEM, "bao": BAO}


class Refused(Exception):
    """the reference's own setup is undefined for this geometry"""


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


def ref_tables(scale, param, min_f, max_f, n_points_target, n_src, frame_size_sec, weighting=0):
    """the reference's tables for one instance; raises Refused where its setup is undefined"""
    if scale == LOG and (param <= 0.0 or param == 1.0):
        param = 2.0
    if not (scale == LOG and param == 2.0):
        weighting = 0
    n_tgt = n_src if n_points_target <= 0 else n_points_target
    if n_tgt == 1:
        raise Refused("nPointsTarget 1")
    delta_f = 1.0 / float(np.float32(frame_size_sec))
    if min_f < 1.0:
        min_f = 1.0
    sampl_f = delta_f * float(n_src - 1)
    if max_f <= min_f or max_f > sampl_f:
        max_f = sampl_f
    fmin_t, fmax_t = fwd(min_f, scale, param), fwd(max_f, scale, param)
    delta_f_t = (fmax_t - fmin_t) / (n_tgt - 1)
    f_t = [0.0] * n_src
    for i in range(1 if scale == LOG else 0, n_src):
        f_t[i] = fwd(float(i) * delta_f, scale, param)
    if scale == LOG:
        f_t[0] = 2.0 * f_t[1] - f_t[2]
    if not all(f_t[i] > f_t[i - 1] for i in range(1, n_src)):
        raise Refused("source axis not increasing")
    x = np.array(f_t)
    spline = np.zeros((n_src, 5))
    y2 = 0.0
    for i in range(1, n_src - 1):
        sigma = (f_t[i] - f_t[i - 1]) / (f_t[i + 1] - f_t[i - 1])
        d1 = (f_t[i + 1] - f_t[i]) * (f_t[i + 1] - f_t[i - 1])
        d2 = (f_t[i] - f_t[i - 1]) * (f_t[i + 1] - f_t[i - 1])
        p = 1.0 / (sigma * y2 + 2.0)                       # smileMath_cspline's forward sweep: y2 does not depend on the data
        y2 = (sigma - 1.0) * p
        spline[i] = (sigma, d1, d2, p, y2)
    xt = [fmin_t + float(i) * delta_f_t for i in range(n_tgt)]
    if xt[0] < f_t[0] or xt[-1] > f_t[-1]:
        raise Refused("csplint_init: x out of range")
    k = np.zeros(n_tgt, np.int32)
    rec = np.ones((n_tgt, 4))
    kupper = 1
    for i in range(n_tgt):
        while kupper < n_src and f_t[kupper] < xt[i]:
            kupper += 1
        if kupper == n_src:
            raise Refused("csplint_init: x out of range")
        klower = kupper - 1
        rng = f_t[kupper] - f_t[klower]
        if rng == 0.0:
            raise Refused("csplint_init: range 0")
        a = (f_t[kupper] - xt[i]) / rng
        b = 1.0 - a
        r2 = rng * rng / 6.0
        k[i] = klower
        rec[i, :3] = (a, (a * a * a - a) * r2, (b * b * b - b) * r2)
    if weighting:
        n_oct = math.log(max_f / min_f) / math.log(2.0)
        ppo = n_tgt / n_oct
        atan_s = ppo * (math.log(65.0 / 50.0) / math.log(2.0)) - 1.0
        for i in range(n_tgt):
            rec[i, 3] = 0.5 + math.atan(3.0 * (i + 1 - atan_s) / ppo) / math.pi
    return dict(n_src=n_src, n_tgt=n_tgt, f_t=x, spline=spline, k=k, rec=rec, weighting=weighting)


def ref_rows(T, mag, enhance, smooth):
    """cSpecScale::processVector on the rows of mag (float32 [rows, n_src]) -> float32 [rows, n_tgt]"""
    n = T["n_src"]
    y = np.ascontiguousarray(mag, np.float32).astype(np.float64)
    assert y.shape[1] == n
    if enhance:                                              # smileDsp_specEnhanceSHS, row by row as the reference walks it
        for a in y:
            pk = np.zeros(n, bool)
            pk[0] = a[0] > a[1]
            pk[1:-1] = (a[1:-1] > a[:-2]) & (a[1:-1] >= a[2:])
            pk[-1] = a[-1] > a[-2]
            posmax = np.flatnonzero(pk)
            if len(posmax) == 1:                             # posmax[1] of the calloc'd list is 0
                a[0 + 3:] = 0
            else:
                for i in range(1, len(posmax)):
                    lo, hi = posmax[i - 1] + 3, posmax[i] - 3
                    if hi >= lo:
                        a[lo:hi + 1] = 0
    if smooth:                                               # smileDsp_specSmoothSHS: the old left neighbour, the last bin untouched
        left = np.concatenate([np.zeros((y.shape[0], 1)), y[:, :-2]], axis=1)
        y[:, :-1] = (left + 2.0 * y[:, :-1] + y[:, 1:]) / 4.0
    sp = T["spline"]
    u = np.zeros_like(y)
    y2 = np.zeros_like(y)
    with np.errstate(all="ignore"):
        for i in range(1, n - 1):                            # smileMath_cspline, natural boundaries (y1p = ynp = 1e30)
            sigma, d1, d2, p, _ = sp[i]
            ut = (y[:, i + 1] - y[:, i]) / d1 - (y[:, i] - y[:, i - 1]) / d2
            u[:, i] = p * (6.0 * ut - sigma * u[:, i - 1])
            y2[:, i] = sp[i, 4]
        y2[:, n - 1] = (0.0 - 0.0 * u[:, n - 2]) / (0.0 * y2[:, n - 2] + 1.0)
        for j in range(n - 2, -1, -1):
            y2[:, j] = y2[:, j] * y2[:, j + 1] + u[:, j]
        k, rec = T["k"], T["rec"]
        a, c, d = rec[:, 0], rec[:, 1], rec[:, 2]
        b = 1.0 - a
        out = a * y[:, k] + b * y[:, k + 1] + c * y2[:, k] + d * y2[:, k + 1]      # smileMath_csplint
        dst = out.astype(np.float32)
        if T["weighting"]:
            w = (dst.astype(np.float64) * rec[:, 3]).astype(np.float32)
            dst = np.where(dst > 0.0, w, np.float32(0.0))
    return dst


def bits_equal(a, b):
    a = np.ascontiguousarray(a, np.float32)
    b = np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | ((a == 0) & (b == 0))))


# ---- the instances of tests/conf/specscale_general.conf: name -> (scale, param, minF, maxF, nPointsTarget, enhance, smooth, weighting)
CONF = {
    "mel": (MEL, 0.0, 25.0, -1.0, 0, 1, 1, 0),
    "bark": (BARK, 0.0, 50.0, 7000.0, 64, 0, 0, 0),
    "lin": (LIN, 0.0, 100.0, 4000.0, 0, 1, 0, 0),
    "log": (LOG, 10.0, 25.0, -1.0, 0, 0, 1, 0),
    "sem": (SEM, 10.0, 50.0, 7000.0, 64, 1, 1, 0),
    "oct": (LOG, 2.0, 25.0, 7000.0, 100, 1, 1, 1),
}
CONF_ORDER = ("mel", "bark", "lin", "log", "sem", "oct")
GOLDEN_KEYS = ("u3_6400", "u10_4800")

# ---- seeded geometries the device test runs (and this file checks the table builder on): every scale with every source size; the
# target sizes {2, 7, n_src, 3 n_src}, the row counts and the switches go round so that each meets each source size and scale.
# 25 ms levels (40 Hz bins: the widest of bao's and bark's limits), minF 50 (the log axes start at half a bin, bao is negative
# below 39.5 Hz), an explicit maxF inside the spectrum (the top itself can fail the reference's range check by one rounding).
N_SRC = (5, 33, 200, 257, 513, 4097)
SEEDED = []
for _i, _n in enumerate(N_SRC):
    for _j, (_name, _param) in enumerate((("lin", 0.0), ("log", 10.0), ("log", 2.0), ("bark", 0.0), ("mel", 0.0), ("sem", 10.0), ("bao", 0.0))):
        _nt = (2, 7, 0, 3 * _n)[(_i + _j) % 4]
        _rows = (1, 63, 65, 130)[(_i + 2 * _j + _j // 2) % 4]
        _sw = (_i + 3 * _j) % 8                              # bit 0 enhance, 1 smooth, 2 weighting (kept on log base 2 only); 3 j: apart from the
                                                             # target-size index, so that each switch meets each target size
        SEEDED.append(dict(scale=_name, param=_param, min_f=50.0, max_f=0.9 * 40.0 * (_n - 1), n_tgt=_nt, n_src=_n, fs=0.025,
                           rows=_rows, enhance=_sw & 1, smooth=(_sw >> 1) & 1, weighting=(_sw >> 2) & 1))


def seeded_id(c):
    return f"{c['scale']}{c['param']:g}-n{c['n_src']}-t{c['n_tgt']}-r{c['rows']}-s{c['enhance']}{c['smooth']}{c['weighting']}"


def lib_tables(scale, param, min_f, max_f, n_points_target, n_src, frame_size_sec, weighting=0):
    """smilehip_specscale_tables: the tables the operator uploads; raises Refused with the library's message"""
    from opensmile_amd import capi
    L = capi.load()
    o = capi.specscale_opts(scale, param, min_f, max_f, n_points_target, 0, 0, weighting)
    n_tgt = n_src if n_points_target <= 0 else n_points_target
    f_t, spline = np.zeros(n_src), np.zeros((n_src, 5))
    k, rec = np.zeros(max(n_tgt, 1), np.int32), np.zeros((max(n_tgt, 1), 4))
    rc = L.smilehip_specscale_tables(C.byref(o), n_src, frame_size_sec, f_t.ctypes.data, spline.ctypes.data, k.ctypes.data, rec.ctypes.data)
    if rc < 0:
        assert rc == -1                                      # SMILEHIP_ERR_INVALID
        raise Refused(L.smilehip_last_error().decode())
    assert rc == n_tgt
    return dict(n_src=n_src, n_tgt=n_tgt, f_t=f_t, spline=spline, k=k, rec=rec)


def same_tables(A, B):
    for key in ("f_t", "spline", "rec"):
        assert np.array_equal(A[key].view(np.uint64), B[key].view(np.uint64)), key
    assert np.array_equal(A["k"], B["k"])


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "specscale_general_synth.npz"))


def split_levels(y):
    """the columns of the conf's HTK file: the magnitude level, then the six scaled levels"""
    out, c = {"mag": y[:, :257]}, 257
    for name in CONF_ORDER:
        w = CONF[name][4] if CONF[name][4] > 0 else 257
        out[name] = y[:, c:c + w]
        c += w
    assert c == y.shape[1] == 1256
    return out


@pytest.mark.parametrize("name", CONF_ORDER)
def test_restatement_equals_the_real_binary(golden, name):
    """the restatement on the binary's own magnitude level gives the binary's scaled level, bit for bit"""
    scale, param, min_f, max_f, npt, enh, smo, wgt = CONF[name]
    T = ref_tables(scale, param, min_f, max_f, npt, 257, float(golden["frame_size_sec"]), wgt)
    for key in GOLDEN_KEYS:
        lv = split_levels(golden["out_" + key])
        assert 2 <= lv["mag"].shape[0] <= 40
        got = ref_rows(T, lv["mag"], enh, smo)
        assert bits_equal(got, lv[name]), f"{name} {key}: {np.argwhere(got.view(np.uint32) != lv[name].view(np.uint32))[:5]}"


@pytest.mark.parametrize("name", CONF_ORDER)
@pytest.mark.parametrize("fs", [0.025, 0.032, 0.06, 0.064])
def test_table_builder_on_the_conf_instances(name, fs):
    scale, param, min_f, max_f, npt, _, _, wgt = CONF[name]
    same_tables(lib_tables(scale, param, min_f, max_f, npt, 257, fs, wgt), ref_tables(scale, param, min_f, max_f, npt, 257, fs, wgt))


@pytest.mark.parametrize("c", SEEDED, ids=seeded_id)
def test_table_builder_on_the_seeded_geometries(c):
    args = (SCALES[c["scale"]], c["param"], c["min_f"], c["max_f"], c["n_tgt"], c["n_src"], c["fs"], c["weighting"])
    same_tables(lib_tables(*args), ref_tables(*args))


def test_table_builder_option_resets():
    """logScaleBase <= 0 or == 1 becomes 2; the weighting table exists on log base 2 only; minF < 1 becomes 1; maxF above the
    spectrum's top or not above minF becomes the top (specScale.cpp:104-108, 164-177, 254-258)"""
    base = lib_tables(LOG, 2.0, 25.0, -1.0, 0, 257, 0.032, 1)
    assert (base["rec"][:, 3] != 1.0).all()
    for bad in (0.0, -3.0, 1.0):
        same_tables(lib_tables(LOG, bad, 25.0, -1.0, 0, 257, 0.032, 1), base)
    same_tables(lib_tables(LOG, 2.0, 25.0, 1e9, 0, 257, 0.032, 1), base)
    same_tables(lib_tables(LOG, 2.0, 25.0, 20.0, 0, 257, 0.032, 1), base)
    for scale, param in ((LOG, 10.0), (MEL, 0.0), (LIN, 0.0), (BARK, 0.0), (SEM, 10.0)):
        assert (lib_tables(scale, param, 50.0, 7000.0, 64, 257, 0.032, 1)["rec"][:, 3] == 1.0).all()
    same_tables(lib_tables(MEL, 0.0, 0.25, 4000.0, 50, 257, 0.032), ref_tables(MEL, 0.0, 1.0, 4000.0, 50, 257, 0.032))
    same_tables(lib_tables(MEL, 0.0, -5.0, 4000.0, 50, 257, 0.032), lib_tables(MEL, 0.0, 1.0, 4000.0, 50, 257, 0.032))


REFUSALS = {
    "sem firstNote at the bin spacing": ((SEM, 31.25, 50.0, 7000.0, 64, 257, 0.032), "increase"),
    "sem firstNote above the bin spacing": ((SEM, 55.0, 50.0, 7000.0, 64, 257, 0.032), "increase"),
    "bao at 31.25 Hz bins": ((BAO, 0.0, 100.0, 4000.0, 0, 257, 0.032), "increase"),
    "log base 10, minF 20, 100 points, 60 ms level: the range check by one rounding": ((LOG, 10.0, 20.0, -1.0, 100, 513, 0.06), "csplint_init"),
    "log minF below the axis' first point": ((LOG, 2.0, 5.0, -1.0, 0, 257, 0.032), "csplint_init"),
    "nPointsTarget 1": ((MEL, 0.0, 25.0, -1.0, 1, 257, 0.032), "nPointsTarget"),
    "three source bins": ((MEL, 0.0, 25.0, -1.0, 0, 3, 0.032), "source bins"),
    "8194 source bins": ((MEL, 0.0, 25.0, -1.0, 0, 8194, 0.032), "source bins"),
    "16385 target points": ((MEL, 0.0, 25.0, -1.0, 16385, 257, 0.032), "target points"),
    "unknown scale": ((5, 0.0, 25.0, -1.0, 0, 257, 0.032), "scale"),
    "minF not a number on the linear scale (the other scales map it to 0)": ((LIN, 0.0, float("nan"), -1.0, 0, 257, 0.032), "not finite"),
    "maxF not a number on the linear scale": ((LIN, 0.0, 25.0, float("nan"), 0, 257, 0.032), "not finite"),
    "log base not a number": ((LOG, float("nan"), 25.0, -1.0, 0, 257, 0.032), "increase"),
    "minF at the spectrum's top with the weighting on: zero octaves": ((LOG, 2.0, 1.0 / float(np.float32(0.032)) * 256.0, -1.0, 0, 257, 0.032, 1), "weighting"),
}
# Not in the list because no argument reaches them once the source axis has been found strictly increasing: smileMath_csplint_init's
# "range == 0" (the width of an interval between two bins of that axis), and the builder's guard against a spline interval whose
# width product underflows or overflows (frameSizeSec passes through a float: the bin spacing lies in 3e-39 .. 7e44 Hz, the
# products of two axis distances far inside the doubles; log-type axes are closer to 1 still). Both stay in the builder as guards.


@pytest.mark.parametrize("what", list(REFUSALS))
def test_table_builder_refusals(what):
    """where the reference's own setup is undefined the builder refuses with a message that names the cause -- and the
    restatement, which follows the reference's checks, refuses the same geometries (the size limits are the library's own)"""
    args, word = REFUSALS[what]
    with pytest.raises(Refused) as e:
        lib_tables(*args)
    assert word in str(e.value) and "cSpecScale" in str(e.value), str(e.value)
    if word in ("increase", "csplint_init", "nPointsTarget"):
        with pytest.raises(Refused):
            ref_tables(*args)


def test_sizes_at_the_limits():
    """4 and 8193 source bins, 2 and 16384 target points, sizes that are not 2^k + 1"""
    for n_src, n_tgt in ((4, 2), (8193, 16384), (300, 77), (6, 16384)):
        args = (MEL, 0.0, 25.0, 0.9 * 40.0 * (n_src - 1), n_tgt, n_src, 0.025)
        same_tables(lib_tables(*args), ref_tables(*args))
