"""The arithmetic sequences every bit-exact chain rests on, run ON THE DEVICE from the product's own headers and swept over their
arguments (tests/helpers/testkernels.hip includes opensmile_amd/csrc/lld_device.hpp and glibc_float.hpp; nothing is restated):

 - glibc_logf / expf / log10f / atanf / acosf: all 2^32 arguments of each against the real libm of this machine; glibc_atan2f on
   the pseudo-random pairs of tests/test_glibc_float.py (same generator, seed and count as its full run);
 - sqrt_rn_batch<16>: all 2^32 bit patterns against the host's IEEE sqrtf, arranged so that whole waves provably take the lean
   branch, and again with one value per wave that must send the wave to the library's;
 - div_markstein (float) behind its two guards, as the kernels call it: all 2^23 significands at every normal exponent, both signs,
   for the divisors the chains use, against the device's a / b -- which a sample of 2^26 triples pins to numpy's float32 division;
   and waves with one lane of every special class;
 - div_markstein (double): 2^30 seeded numerators per divisor of the F0 sweep's table (with its stored reciprocals) and of ComParE's
   frame kernel, against the device's a / b, itself checked against numpy float64 on a sample.

The default is the full sweep (13 - 15 s on an MI355X with 16 host threads, against 46 s for the slowest other test file:
profiles/r08_device_math_sweep.json); GLIBC_FLOAT_FULL=0 runs the strided and
complete-binade ranges of tests/test_glibc_float.py and every 61st significand chunk instead (for a quick local look).
Launches are short: at most 2^26 arguments each. All GPU work happens in this one process."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tolerance import record

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HELPERS = os.path.join(ROOT, "tests", "helpers")
CHUNK = 1 << 26
FULL = os.environ.get("GLIBC_FLOAT_FULL", "1") != "0"

u64, u32p = C.c_ulonglong, C.POINTER(C.c_uint)


@pytest.fixture(scope="module")
def dev():
    p = os.path.join(HELPERS, "libsmilehip_testkernels.so")
    if not os.path.exists(p):
        pytest.skip("tests/helpers/libsmilehip_testkernels.so not built (python __graft_entry__.py)")
    L = C.CDLL(p)
    L.smilehip_debug_sweep_open.argtypes = [C.c_size_t]
    L.smilehip_debug_sweep_host.restype = C.c_void_p
    L.smilehip_debug_sweep_host.argtypes = [C.c_int]
    L.smilehip_debug_glibc_launch.argtypes = [C.c_int, C.c_uint, C.c_uint, C.c_int]
    L.smilehip_debug_glibc_atan2f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    L.smilehip_debug_sqrt_launch.argtypes = [C.c_int, u64, C.c_uint, C.c_int]
    L.smilehip_debug_sweep_counters.argtypes = [C.POINTER(u64)]
    L.smilehip_debug_div_f32_sweep.argtypes = [C.c_int, C.c_float, C.c_int, C.POINTER(u64)]
    L.smilehip_debug_div_f32.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_float, C.c_void_p, C.c_void_p]
    L.smilehip_debug_div_f32_sample.argtypes = [C.c_void_p, C.c_int, C.c_uint, C.c_void_p, C.c_void_p, C.c_void_p]
    L.smilehip_debug_div_f64_sweep.argtypes = [u64, C.c_int, C.c_double, C.c_double, u64, C.POINTER(u64)]
    L.smilehip_debug_div_f64_sample.argtypes = [u64, C.c_int, C.c_void_p, C.c_int, C.c_uint, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.smilehip_debug_f0_sw_rec.argtypes = [C.c_longlong, C.c_double, C.c_int, C.c_float, C.c_double, C.c_void_p]
    assert L.smilehip_debug_sweep_open(CHUNK * 4) == 0
    yield L
    L.smilehip_debug_sweep_close()


@pytest.fixture(scope="module")
def host():
    """tests/helpers/device_math_check.cpp: the threaded comparison with the real libm (same compiler flags as the host sweep of
    tests/test_glibc_float.py, so that its build of the header is the one that test proves equal to libm)"""
    src = os.path.join(HELPERS, "device_math_check.cpp")
    so = os.path.join(HELPERS, "_device_math_check.so")
    deps = [src, os.path.join(HELPERS, "device_math_args.h"), os.path.join(ROOT, "opensmile_amd", "csrc", "glibc_float.hpp")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in deps):
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-pthread", "-ffp-contract=off", "-mfma", "-fno-builtin-logf",
                        "-fno-builtin-expf", "-fno-builtin-log10f", "-fno-builtin-atanf", "-fno-builtin-atan2f", "-fno-builtin-acosf",
                        "-o", so, src, "-lm"], check=True)
    L = C.CDLL(so)
    for f in ("device_math_check_libm", "device_math_check_header"):
        getattr(L, f).restype = C.c_longlong
        getattr(L, f).argtypes = [C.c_int, C.c_uint, u64, C.c_void_p, u32p]
    L.device_math_check_sqrt.restype = C.c_longlong
    L.device_math_check_sqrt.argtypes = [C.c_int, u64, u64, C.c_void_p, u32p]
    L.device_math_sqrt_odd_waves.restype = C.c_longlong
    L.device_math_sqrt_odd_waves.argtypes = [C.c_int, u64, u64]
    L.device_math_atan2f_pairs.restype = None
    L.device_math_atan2f_pairs.argtypes = [C.POINTER(u64), u64, u64, C.c_void_p, C.c_void_p]
    L.device_math_check_atan2f.restype = C.c_longlong
    L.device_math_check_atan2f.argtypes = [u64, C.c_void_p, C.c_void_p, C.c_void_p, u32p]
    return L


def _pipeline(dev, chunks, launch, check):
    """chunks through the two staging slots: chunk k + 1 is launched before the host looks at chunk k"""
    if not chunks:
        return
    assert launch(chunks[0], 0) == 0
    for k, ch in enumerate(chunks):
        assert dev.smilehip_debug_sweep_wait() == 0
        if k + 1 < len(chunks):
            assert launch(chunks[k + 1], (k + 1) & 1) == 0
        check(ch, dev.smilehip_debug_sweep_host(k & 1))


def _libm_chunks():
    if FULL:
        return [(lo, CHUNK) for lo in range(0, 1 << 32, CHUNK)]
    # every 61st chunk of 2^20 over the whole range, the complete binades around +-1, the subnormals and the first normal binade
    ch = [(lo, 1 << 20) for lo in range(0, 1 << 32, 61 << 20)]
    for lo, hi in ((0x3e800000, 0x40800000), (0xbe800000, 0xc0800000), (0, 0x01000000)):
        ch += [(a, min(CHUNK, hi - a)) for a in range(lo, hi, CHUNK)]
    return ch


@pytest.mark.parametrize("which,name", [(0, "logf"), (1, "expf"), (2, "log10f"), (3, "atanf"), (4, "acosf")])
def test_device_glibc_float_equals_libm(dev, host, which, name):
    """The gfx950 build of glibc_float.hpp against the libm of the machine running the test (which tests/test_glibc_float.py
    shows to be what the header's host build computes). A mismatch names the argument, the device's bits, libm's bits and the host
    build's bits: device != host build is a device code-generation difference; device == host build != libm is a libm that is not
    the one the tables were read from."""
    if "fma" not in open("/proc/cpuinfo").read():
        pytest.skip("CPU without FMA: the dynamic linker selects glibc's non-FMA build of logf / expf")
    fb = (C.c_uint * 4)()
    tot = {"n": 0, "bad": 0, "msg": ""}

    def check(ch, ptr):
        bad = host.device_math_check_libm(which, ch[0], ch[1], ptr, fb)
        tot["n"] += ch[1]
        if bad and not tot["bad"]:
            tot["msg"] = (f"{name}({fb[0]:#010x}): device {fb[1]:#010x}, libm {fb[2]:#010x}, host build of glibc_float.hpp {fb[3]:#010x}")
        tot["bad"] += bad

    _pipeline(dev, _libm_chunks(), lambda ch, slot: dev.smilehip_debug_glibc_launch(which, ch[0], ch[1], slot), check)
    record(f"device_math_glibc_{name}", arguments=tot["n"], mismatches=tot["bad"], threads=host.device_math_threads())
    assert tot["bad"] == 0, f"{tot['bad']} of {tot['n']} arguments differ, first: {tot['msg']}"
    assert not FULL or tot["n"] == 1 << 32


def test_device_glibc_atan2f_pairs_equal_libm(dev, host):
    """glibc_atan2f on the device, on the pairs glibc_float_check.cpp's generator produces for seed 12345 (3e8 in the full run, the
    count of its GLIBC_FLOAT_FULL sweep; 2e7 otherwise)."""
    n_total = 300_000_000 if FULL else 20_000_000
    step = 1 << 25
    state = (u64 * 2)(0, 0)
    ys, xs, out = (np.empty(step, np.float32) for _ in range(3))
    fb = (C.c_uint * 5)()
    done = bad_total = 0
    msg = ""
    while done < n_total:
        n = min(step, n_total - done)
        host.device_math_atan2f_pairs(state, 12345, n, ys.ctypes.data, xs.ctypes.data)
        assert dev.smilehip_debug_glibc_atan2f(ys.ctypes.data, xs.ctypes.data, out.ctypes.data, n) == 0
        bad = host.device_math_check_atan2f(n, ys.ctypes.data, xs.ctypes.data, out.ctypes.data, fb)
        if bad and not bad_total:
            msg = f"atan2f(y {fb[0]:#010x}, x {fb[1]:#010x}): device {fb[2]:#010x}, libm {fb[3]:#010x}, host build of glibc_float.hpp {fb[4]:#010x}"
        bad_total += bad
        done += n
    record("device_math_glibc_atan2f", arguments=done, mismatches=bad_total)
    assert bad_total == 0, f"{bad_total} of {done} pairs differ, first: {msg}"


LEAN, REST = 0x70000000, 0x90000000


def test_device_sqrt_rn_batch_every_bit_pattern(dev, host):
    """sqrt_rn_batch<16> over all 2^32 patterns against the host's sqrtf (IEEE 754: correctly rounded). Arrangement 0 fills waves from
    [2^-96, inf) alone: every wave must report the lean branch, or the lean form is not what is being tested. Arrangement 1 is the
    same waves with one value replaced by +0, -0, a subnormal, 2^-97, +inf, a NaN or a negative number in turn: every wave must
    report the library branch, and every lane must still be right. Arrangement 2 is the rest of the 2^32 patterns."""
    fb = (C.c_uint * 3)()
    cnt = (u64 * 3)()
    stride = 1 if FULL else 61
    res = {}
    for arr, total in ((0, LEAN), (1, LEAN), (2, REST)):
        chunks = [(lo, CHUNK) for lo in range(0, total, CHUNK)][::stride]
        assert dev.smilehip_debug_sweep_counters(cnt) == 0            # (reset)
        tot = {"n": 0, "bad": 0, "msg": ""}

        def check(ch, ptr):
            bad = host.device_math_check_sqrt(arr, ch[0], ch[1], ptr, fb)
            tot["n"] += ch[1]
            if bad and not tot["bad"]:
                tot["msg"] = f"arrangement {arr}: sqrt({fb[0]:#010x}): device {fb[1]:#010x}, host sqrtf {fb[2]:#010x}"
            tot["bad"] += bad

        _pipeline(dev, chunks, lambda ch, slot: dev.smilehip_debug_sqrt_launch(arr, ch[0], ch[1], slot), check)
        assert dev.smilehip_debug_sweep_counters(cnt) == 0
        res[arr] = (tot["n"], tot["bad"], int(cnt[0]), int(cnt[1]), tot["msg"])
        record(f"device_math_sqrt_arrangement{arr}", arguments=tot["n"], mismatches=tot["bad"], lean_waves=int(cnt[0]), library_waves=int(cnt[1]))
    for arr, (n, bad, lean, libw, msg) in res.items():
        assert bad == 0, f"{bad} of {n} values differ, first: {msg}"
        assert lean + libw == n // 1024
    assert res[0][3] == 0 and res[0][2] == res[0][0] // 1024, f"arrangement 0: {res[0][3]} waves left the lean branch"
    assert res[1][2] == 0 and res[1][3] == res[1][0] // 1024, f"arrangement 1: {res[1][2]} waves took the lean branch past a value it is not valid for"
    assert res[2][2] == 0
    if FULL:
        assert res[0][0] + res[2][0] == 1 << 32 and res[1][0] == LEAN
    # the arrangement is what it says (host side): one odd value in every wave of arrangement 1
    assert host.device_math_sqrt_odd_waves(1, 0, 1 << 22) == 1 << 12 and host.device_math_sqrt_odd_waves(0, 0, 1 << 22) == 0


# the divisors the chains divide by this way: nHarmonics 1 .. 32 (f0_shs), the delta regression's 10, cAcf's bin counts, and the hostile
# set of tests/test_exact_sum_claims.py
DIVISORS = [float(b) for b in range(1, 33)] + [10.0, 129.0, 257.0, 513.0, 1025.0, 2049.0, 3.0, 16777215.0, 1.9999999, 1.0000001]
KINDS = {0: "any_sign", 1: "nonneg"}            # div_needs_division / div_needs_division_nonneg


def _bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    ai, bi = (a.view(np.uint32), b.view(np.uint32)) if a.dtype == np.float32 else (a.view(np.uint64), b.view(np.uint64))
    return (ai == bi) | (np.isnan(a) & np.isnan(b))


@pytest.mark.parametrize("kind", [0, 1])
def test_device_float_quotient_every_significand_and_exponent(dev, kind):
    """div_markstein behind its guard, as the kernels call it (a lane ORs the guard over its 16 values, the wave takes the sequence
    when div_wave_is_safe): every float with a normal exponent (254 x 2^23), both signs, every divisor above, against a / b on the
    device. The guards send part of the range to the division itself (any-sign: |a| outside (2^-60, 2^60); never-negative:
    (0, 2^-100) and everything with the sign bit) -- the share of waves that took the sequence is recorded and must be what the
    guard's range says."""
    res = (u64 * 5)()
    checked = bad = fast = waves = 0
    first = None
    for b in DIVISORS:
        for neg in (0, 1):
            assert dev.smilehip_debug_div_f32_sweep(kind, b, neg, res) == 0
            checked += res[0]; bad += res[1]; fast += res[2]; waves += res[3]
            if res[1] and first is None:
                first = f"a = {int(res[4]) | (0x80000000 if neg else 0):#010x}, b = {b!r}"
    record(f"device_math_div_f32_{KINDS[kind]}", arguments=checked, mismatches=bad, divisors=len(DIVISORS), fast_waves=fast, waves=waves)
    assert bad == 0, f"{bad} of {checked} quotients differ from a / b, first: {first}"
    assert checked == len(DIVISORS) * 2 * 254 * (1 << 23)
    # exponents -59 .. 59 of both signs (any-sign; the wave holding 2^-60 itself takes the division), -100 .. 127 of the positive ones
    per_exp = (1 << 23) // 1024
    expect = len(DIVISORS) * (2 * (120 * per_exp - 1) if kind == 0 else 228 * per_exp)
    assert fast == expect, (fast, expect)


def test_device_float_division_is_ieee(dev):
    """2^26 (a, b, a / b) triples of the device's own division -- a walks every class of bit pattern, b the divisors above -- against
    numpy's float32 division: what the sweep above compares with is the correctly rounded quotient."""
    n = CHUNK
    divs = np.asarray(DIVISORS, np.float32)
    a, b, q = (np.empty(n, np.float32) for _ in range(3))
    assert dev.smilehip_debug_div_f32_sample(divs.ctypes.data, len(divs), n, a.ctypes.data, b.ctypes.data, q.ctypes.data) == 0
    assert np.array_equal(b, divs[np.arange(n) % len(divs)])
    assert len(np.unique(a.view(np.uint32) >> 23)) == 512            # every sign and exponent field occurs
    with np.errstate(all="ignore"):
        ok = _same(q, a / b)
    record("device_math_div_f32_device_division_vs_numpy", arguments=n, mismatches=int((~ok).sum()))
    i = int(np.argmin(ok))
    assert ok.all(), f"{(~ok).sum()} differ, first: {_bits(a)[i]:#010x} / {b[i]!r}: device {_bits(q)[i]:#010x}"


def _f(bits):
    return np.array([bits], np.uint32).view(np.float32)[0]


_UP, _DN = (lambda x: np.nextafter(np.float32(x), np.float32(np.inf))), (lambda x: np.nextafter(np.float32(x), np.float32(-np.inf)))
CLASSES_NONNEG = {
    "+0": _f(0), "min_subnormal": _f(1), "max_subnormal": _f(0x007fffff), "below_2^-100": _DN(2.0 ** -100), "2^-100": np.float32(2.0 ** -100),
    "above_2^-100": _UP(2.0 ** -100), "below_2^-60": _DN(2.0 ** -60), "2^-60": np.float32(2.0 ** -60), "above_2^-60": _UP(2.0 ** -60),
    "below_2^60": _DN(2.0 ** 60), "2^60": np.float32(2.0 ** 60), "above_2^60": _UP(2.0 ** 60), "max_normal": _f(0x7f7fffff),
    "+inf": np.float32(np.inf), "nan": np.float32(np.nan),
}
CLASSES = dict(CLASSES_NONNEG)
CLASSES.update({"-" + k.lstrip("+"): -v for k, v in CLASSES_NONNEG.items() if k != "nan"})


@pytest.mark.parametrize("kind,cls", [(0, c) for c in CLASSES] + [(1, c) for c in CLASSES_NONNEG])
def test_device_float_quotient_special_lane(dev, kind, cls):
    """Waves of ordinary values with ONE lane holding a special value: +-0, the smallest and largest subnormal, the values either side
    of each guard bound (2^-100; 2^-60, 2^60), +-inf, NaN. Every lane of the wave -- the special one and the 63 others -- must carry
    the division's bits (NaN as a class), for both guards; the never-negative guard (f0_shs) is given the non-negative classes, its
    domain. (Before the guard of f0_shs tested for non-finite values, +inf failed here: fma(-inf, nh, inf) is NaN, inf / nh is inf.)"""
    rng = np.random.default_rng(11)
    special = CLASSES[cls]
    for b in (15.0, 10.0, 257.0, 3.0, 1.0, 32.0):
        lanes = (0, 1, 31, 32, 62, 63)
        a = np.exp(rng.uniform(-20, 20, (len(lanes), 64))).astype(np.float32)
        if kind == 0:
            a *= rng.choice(np.array([-1.0, 1.0], np.float32), a.shape)
        for w, lane in enumerate(lanes):
            a[w, lane] = special
        got, div = np.empty_like(a), np.empty_like(a)
        assert dev.smilehip_debug_div_f32(kind, a.ctypes.data, a.size, b, got.ctypes.data, div.ctypes.data) == 0
        with np.errstate(all="ignore"):
            ref = a / np.float32(b)
        assert _same(div, ref).all(), f"the device's division differs from numpy's for b = {b}"
        ok = _same(got, div)
        w, lane = np.unravel_index(int(np.argmin(ok)), ok.shape)
        assert ok.all(), (f"{KINDS[kind]} guard, class {cls}, b = {b}: lane {lane} of a wave whose lane {lanes[w]} holds {special!r}: a = {_bits(a)[w, lane]:#010x}, "
                          f"helper {_bits(got)[w, lane]:#010x}, a / b {_bits(div)[w, lane]:#010x}")
    record(f"device_math_div_f32_class_{KINDS[kind]}_{cls}", arguments=6 * 6 * 64, mismatches=0)


def _f64_divisors(dev):
    """(b, y) pairs: d1 and d2 of every bin of the default ComParE plan's F0 sweep table with the reciprocals stored beside them;
    ComParE's frame-kernel divisors: log 2 with its compile-time reciprocal, and frame power sums over their whole range (floor
    1e-7 .. 2.7e7), whose reciprocal the kernel forms on the device (y = NaN asks the test kernel to do the same)."""
    from opensmile_amd import capi
    ctx = capi.Context(0)
    plan = capi.Plan(ctx, capi.compare16_f0_config())
    g = plan.geometry
    cfg = capi.compare16_f0_config()
    K = int(g.n_bins)
    rec = np.zeros((K, 8), np.float64)
    assert dev.smilehip_debug_f0_sw_rec(K, g.fft_frame_size_sec, cfg.shs_n_harmonics, cfg.shs_compression,
                                        cfg.specscale_min_f if cfg.specscale_min_f > 0 else 25.0, rec.ctypes.data) == 0
    inner = rec[1:K - 1]
    pairs = [(b, y) for b, y in zip(inner[:, 3], inner[:, 4])] + [(b, y) for b, y in zip(inner[:, 5], inner[:, 6])]
    assert len(pairs) == 2 * (K - 2) and all(b > 0 and y == 1.0 / b for b, y in pairs)
    log2 = 0.693147180559945286226764
    pairs.append((log2, 1.0 / log2))
    rng = np.random.default_rng(5)
    dn = np.concatenate([[np.float64(np.float32(0.0000001)), 2.7e7], np.exp(rng.uniform(np.log(1e-7), np.log(2.7e7), 14))])
    pairs += [(float(b), float("nan")) for b in dn]
    return pairs


def test_device_double_quotient(dev):
    """div_markstein (double) against the device's a / b: per divisor 2^29 seeded numerators of magnitude 2^-17 .. 2 (what the F0
    sweep and the ComParE frame kernel divide) and 2^29 across exponents -900 .. 900 (the domain the helper's comment claims), random
    signs. And the device's double division against numpy float64 on 2^22 + 2^22 sampled triples."""
    pairs = _f64_divisors(dev)
    per_mode = 1 << 29 if FULL else 1 << 20
    res = (u64 * 3)()
    checked = bad = 0
    first = None
    for k, (b, y) in enumerate(pairs):
        for mode in (0, 1):
            assert dev.smilehip_debug_div_f64_sweep(1000 + k, mode, b, y, per_mode, res) == 0
            checked += res[0]; bad += res[1]
            if res[1] and first is None:
                first = f"divisor {b!r} (reciprocal {y!r}), mode {mode}, seed {1000 + k}, numerator index {int(res[2])}"
    record("device_math_div_f64", arguments=checked, mismatches=bad, divisors=len(pairs), numerators_per_divisor=2 * per_mode)
    assert bad == 0, f"{bad} of {checked} quotients differ from a / b, first: {first}"
    n = 1 << 22
    divs = np.array([p[0] for p in pairs], np.float64)
    for mode in (0, 1):
        a, b, q, qm = (np.empty(n, np.float64) for _ in range(4))
        assert dev.smilehip_debug_div_f64_sample(77, mode, divs.ctypes.data, len(divs), n, a.ctypes.data, b.ctypes.data, q.ctypes.data, qm.ctypes.data) == 0
        assert np.array_equal(b, divs[np.arange(n) % len(divs)])
        lo, hi = (2.0 ** -17, 2.0) if mode == 0 else (2.0 ** -900, 2.0 ** 901)
        assert (np.abs(a) >= lo).all() and (np.abs(a) < hi).all() and (a < 0).any() and (a > 0).any()
        ok = _same(q, a / b)
        record(f"device_math_div_f64_device_division_vs_numpy_mode{mode}", arguments=n, mismatches=int((~ok).sum()))
        i = int(np.argmin(ok))
        assert ok.all(), f"device a / b differs from numpy float64: {a[i]!r} / {b[i]!r} = {q[i]!r}"
        assert _same(qm, q).all()
