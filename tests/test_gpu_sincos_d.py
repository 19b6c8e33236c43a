"""sincos_d (opensmile_amd/csrc/lld_sincos_d.hpp), the device's double sine and cosine behind cTonefilt's recursion, against sinl / cosl
of a g++ helper (tests/helpers/tonefilt_check.cpp), the way tests/test_gpu_fft.py measures log_d. The bound is the function's stated
one, 1 ulp over its stated domain |x| <= 2^30; the measured maxima are recorded."""
import numpy as np
import pytest

from helpers import tonefilt_host as H

pytestmark = pytest.mark.gpu
DOMAIN = 2.0 ** 30


@pytest.fixture(scope="module")
def dev():
    from opensmile_amd import capi
    ctx = capi.Context(0)
    return capi, ctx


def measure(dev, x, what):
    from tolerance import record
    capi, ctx = dev
    x = np.ascontiguousarray(x, np.float64)
    s, c = capi.sincos_d_host(ctx, x)
    err, at = H.sincos_err(x, s, c)
    print("sincos_d, %s: %d arguments, largest error %.4f ulp (sin, at %.17g), %.4f ulp (cos, at %.17g)" % (what, len(x), err[0], at[0], err[1], at[1]))
    record("sincos_d_ulp", what=what, n=len(x), sin_ulp=float(err[0]), cos_ulp=float(err[1]))
    assert err.max() <= 1.0, (what, err, at)
    return s, c


def test_the_chain_s_own_arguments(dev):
    """2 pi freq[t] k / rate as the recursion forms it -- w[t] * ((double)k * period) --, every note, seven rates, windows of k from the
    start of an input up to the end of the stated domain"""
    assert H.load().tonefilt_domain() == DOMAIN
    xs = []
    for fs in H.RATES:
        w = H.tables(fs)["w"]
        period = 1.0 / fs
        k_max = int(DOMAIN / (w[-1] * period)) - 1
        for k0 in (0, 10 ** 4, 10 ** 6, k_max // 2, k_max - 256):
            t = np.arange(k0, k0 + 256).astype(np.float64) * period
            xs.append((w[:, None] * t[None, :]).ravel())
    x = np.concatenate(xs)
    assert x.max() <= DOMAIN and x.max() > 0.99 * DOMAIN and len(x) == 7 * 5 * 72 * 256
    measure(dev, x, "the chain's arguments")


def test_seeded_arguments_over_the_domain(dev):
    rng = np.random.default_rng(20)
    measure(dev, rng.uniform(-DOMAIN, DOMAIN, 1 << 22), "2^22 uniform over the domain")


def test_next_to_multiples_of_half_pi_zero_and_tiny(dev):
    k = np.concatenate([np.arange(1, 1 << 15), (1 << np.arange(15, 29)), (1 << np.arange(15, 29)) + 1, [683565275, 683565274]]).astype(np.float64)
    m = k * (np.pi / 2)                                    # the doubles next to k pi/2, both signs
    assert np.abs(m).max() <= DOMAIN
    x = np.concatenate([m, np.nextafter(m, 0.0), np.nextafter(m, 1e300), -m])
    measure(dev, x, "next to multiples of pi/2")
    tiny = np.array([0.0, -0.0, 5e-324, -5e-324, 1e-310, 2.2250738585072014e-308, 1e-300, -1e-300, 1e-160, 1e-20, -1e-9, 2.0 ** -27, 2.0 ** -26,
                     1e-5, -1e-5, DOMAIN, -DOMAIN])
    s, c = measure(dev, tiny, "zero, tiny arguments and the domain's ends")
    assert (s[:2] == 0).all() and (c[:2] == 1).all() and (s[2:9] == tiny[2:9]).all() and (c[2:9] == 1).all()


def test_the_host_build_is_the_same_arithmetic(dev):
    """the g++ build of the header (explicit fma for fma): the device's bits"""
    capi, ctx = dev
    rng = np.random.default_rng(21)
    x = rng.uniform(-DOMAIN, DOMAIN, 1 << 16)
    s, c = capi.sincos_d_host(ctx, x)
    hs, hc, _, _ = H.sincos_check(x)
    assert (s == hs).all() and (c == hc).all()
