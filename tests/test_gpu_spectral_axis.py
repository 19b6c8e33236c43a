"""cSpectral on any spectrum on the device (smilehip_spectral_axis_op_*, csrc/lld_spectral_axis.hip): against the real binary's levels
(tests/golden/spectral_axis_synth.npz), against the numpy restatement of tests/test_spectral_axis_host.py (which that file holds
bit-equal to the same goldens), against the oracle's cSpectral for the linear option sets, and against the GeMAPS operator on
the option sets the two share. The kernel's operations are the
reference's correctly rounded operations in its order and the tables come from the same C library: everything is compared bit for
bit (both-zero counts as equal)."""
import ctypes as C
import os

import numpy as np
import pytest

from test_spectral_axis_host import BARK, CONF, CONF_ORDER, GOLDEN_KEYS, bits_equal, fwd, golden_case, n_out, opts, ref_rows, ref_setup

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, f64 = np.float32, np.float64


@pytest.fixture(scope="module")
def env():
    import torch
    from opensmile_amd import capi
    return torch, capi, capi.Context(0)


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "spectral_axis_synth.npz"))


def c_opts(capi, o):
    kw = {k: v for k, v in o.items() if k not in ("bands", "slopes", "rolloff")}
    return capi.spectral_axis_opts(o["bands"], o["rolloff"], o["slopes"], **kw)


def create(env, o, K, fs, frq):
    torch, capi, ctx = env
    L = capi.load()
    co = c_opts(capi, o)
    op = C.c_void_p()
    fa = None if frq is None else np.ascontiguousarray(frq, f64)
    rc = L.smilehip_spectral_axis_op_create(ctx._h, C.byref(co), K, fs, None if fa is None else fa.ctypes.data, 0 if fa is None else fa.size,
                                            C.byref(op))
    return rc, op


def run_op(env, o, rows, fs, frq, pieces=None, pad_src=3, pad_dst=2):
    """the operator on the rows of one stream, launched piece by piece (default: one launch); rows of K + pad_src floats in and
    n_out + pad_dst out, both pads NaN: the output's must stay NaN"""
    torch, capi, ctx = env
    L = capi.load()
    n, K = rows.shape
    rc, op = create(env, o, K, fs, frq)
    capi._check(rc)
    try:
        no = L.smilehip_spectral_axis_op_n_out(op)
        assert no == n_out(o)
        src = np.full((n, K + pad_src), np.nan, f32)
        src[:, :K] = rows
        d_src = torch.from_numpy(src).cuda()
        d_dst = torch.full((n, no + pad_dst), float("nan"), dtype=torch.float32, device="cuda")
        d_state = torch.full((K,), float("nan"), dtype=torch.float32, device="cuda")
        t = 0
        for m in (pieces or [n]):
            capi._check(L.smilehip_spectral_axis_op_frames(op, d_src[t:].data_ptr(), K + pad_src, d_state.data_ptr(), 1 if t == 0 else 0,
                                                           d_dst[t:].data_ptr(), no + pad_dst, m, None))
            t += m
        assert t == n
        torch.cuda.synchronize()
        got = d_dst.cpu().numpy()
    finally:
        capi._check(L.smilehip_spectral_axis_op_destroy(op))
    assert np.isnan(got[:, no:]).all(), "the operator wrote past a row's outputs"
    return got[:, :no]


def assert_bits(got, ref, what):
    if not bits_equal(got, ref):
        d = (got.view(np.uint32) != ref.view(np.uint32)) & ~((got == 0) & (ref == 0))
        at = np.argwhere(d)
        raise AssertionError(f"{what}: {d.sum()} of {d.size} cells differ, first {at[:4].tolist()}: {got[d][:4]} vs {ref[d][:4]}")


@pytest.mark.parametrize("key", GOLDEN_KEYS)
@pytest.mark.parametrize("name", CONF_ORDER)
def test_goldens(env, golden, name, key):
    """the operator on the real binary's input level gives the real binary's cSpectral level"""
    o, S, rows, want = golden_case(golden, key, name)
    frq = S["ax_m"]
    assert_bits(run_op(env, o, rows, 1.0 / S["F0"], frq), want, f"{name} {key}")


# ---- synthetic spectra against the restatement
EVERY = dict(centroid=1, max_pos=1, min_pos=1, entropy=1, standard_deviation=1, variance=1, skewness=1, kurtosis=1, slope=1, sharpness=1,
             harmonicity=1, flatness=1, spec_diff=1, spec_pos_diff=1, flux=1, flux_centroid=1, flux_at_flux_centroid=1, alpha_ratio=1,
             hammarberg_index=1)
BANDS = ((250, 650), (0, 90), (1000, 4000), (900, 200000))
SLOPES = ((0, 500), (500, 1500), (100, 130))
SETS = {
    "log": opts(bands=BANDS, slopes=SLOPES, rolloff=(0.25, 0.9), use_log_spectrum=1, old_slope_scale=0, spec_floor=1e-5, **EVERY),
    "lognorm": opts(bands=BANDS, slopes=SLOPES, rolloff=(0.5,), use_log_spectrum=1, norm_band_energies=1, log_flatness=1, **EVERY),
    "lin": opts(bands=BANDS, slopes=SLOPES, rolloff=(0.25, 0.5, 0.9), norm_band_energies=1, buggy_roll_off=1, old_slope_scale=0, **EVERY),
    "power": opts(bands=BANDS, slopes=SLOPES, rolloff=(0.9,), square_input=0, log_flatness=1, **EVERY),
}
# (K, rows): every K of the issue; 1, 63, 64, 65 and 130 rows around the 64 frames of a workgroup; 26, 32 and 33 bins around the
# 32-bin tile of the LDS-staged variant that was measured against this kernel (narrower, as wide, one bin wider), 257 and up many
# tiles wide. The large sizes take the small row counts: the restatement is a Python loop per row.
SHAPES = ((4, 130), (9, 64), (26, 65), (32, 65), (33, 64), (257, 63), (257, 130), (1025, 65), (8193, 1), (16385, 1))


def spectra(K, rows, seed, power=False):
    rng = np.random.default_rng(seed)
    x = (rng.random((rows, K)) ** 4 * (10.0 ** rng.uniform(-3, 0, (rows, 1)))).astype(f32)
    return (x * x).astype(f32) if power else x


@pytest.mark.parametrize("axis", [0, 1], ids=["index", "axis"])
@pytest.mark.parametrize("which", list(SETS))
@pytest.mark.parametrize("K,rows", SHAPES)
def test_restatement(env, K, rows, which, axis):
    o = SETS[which]
    fs = 2.0 * (K - 1) / 16000.0 if K > 33 else 0.004       # (a few wide bins for the small K: the bands still meet them)
    frq = np.arange(K, dtype=f64) / fs if axis else None
    x = spectra(K, rows, 1000 * K + rows, which == "power")
    assert_bits(run_op(env, o, x, fs, frq), ref_rows(ref_setup(o, K, fs, frq), o, x), f"{which} K={K} rows={rows} axis={axis}")


@pytest.mark.parametrize("which", list(SETS))
@pytest.mark.parametrize("rng", [(30, 31), (0, 1000000), (125, 1000000), (300, 3400)], ids=["one-bin", "all-bins", "beyond-the-top", "inside"])
def test_freq_range(env, rng, which):
    """freqRange selecting one bin (bin 0), every bin, an upper edge beyond the last bin, and a range inside the spectrum"""
    K, fs = 257, 0.032
    frq = np.arange(K, dtype=f64) / fs
    o = dict(SETS[which], freq_range=rng)
    S = ref_setup(o, K, fs, frq)
    assert (S["lo"], S["hi"]) == {(30, 31): (0, 0), (0, 1000000): (0, 256), (125, 1000000): (4, 256), (300, 3400): (9, 108)}[rng]
    x = spectra(K, 9, 77, which == "power")
    assert_bits(run_op(env, o, x, fs, frq), ref_rows(S, o, x), f"{which} {rng}")


@pytest.mark.parametrize("which", list(SETS))
@pytest.mark.parametrize("K", [26, 257])
def test_edge_rows(env, K, which):
    """all zero, constant, every value below the floor, one non-zero bin, a denormal among the powers; between ordinary rows"""
    o = SETS[which]
    fs = 0.032 if K == 257 else 0.004
    frq = np.arange(K, dtype=f64) / fs
    x = spectra(K, 12, 5, which == "power")
    x[1] = 0.0
    x[3] = 0.25
    x[4] = 0.25
    x[6] = 1e-8 if which != "power" else 1e-16              # specFloor^2 is 1e-10 ("log") / 1e-14 (default) on the powers
    x[8] = 0.0
    x[8, K // 2] = 0.5
    x[10, 3] = 1e-20 if which != "power" else 1e-40          # its power is a denormal float
    assert_bits(run_op(env, o, x, fs, frq), ref_rows(ref_setup(o, K, fs, frq), o, x), f"{which} K={K}")


def test_bark_axis_sharpness(env):
    """an axis that is not linear, with the scale the sharpness weights have to undo named (bark: nothing to undo) and not named
    (what the reference does behind cSpecScale: its own writer level has no SCALED_SPEC meta data, spectral.cpp:614-623)"""
    K, fs = 64, 0.032
    frq = np.array([fwd(float(i) / fs, BARK, 0.0) for i in range(1, K + 1)], f64)
    x = spectra(K, 65, 9)
    for scale in (0, BARK):
        o = opts(bands=((2, 5),), rolloff=(0.5,), sharpness=1, centroid=1, variance=1, frq_scale=scale)
        assert_bits(run_op(env, o, x, fs, frq), ref_rows(ref_setup(o, K, fs, frq), o, x), f"frq_scale {scale}")


@pytest.mark.parametrize("which", ["log", "power"])
def test_stream_carry(env, which):
    """the flux family across launches: the whole stream in one launch = frame by frame = in uneven pieces"""
    K, fs, n = 257, 0.032, 24
    frq = np.arange(K, dtype=f64) / fs
    o = dict(SETS[which], freq_range=(300, 3400))
    x = spectra(K, n, 31, which == "power")
    ref = ref_rows(ref_setup(o, K, fs, frq), o, x)
    assert_bits(run_op(env, o, x, fs, frq), ref, "one launch")
    assert_bits(run_op(env, o, x, fs, frq, pieces=[1] * n), ref, "frame by frame")
    assert_bits(run_op(env, o, x, fs, frq, pieces=[1, 1, 5, 2, 15]), ref, "pieces")


# ---- consistency with the oracle of the linear sets and with the GeMAPS operator
OLD_SETS = {
    "mediaeval": ([(40, 150), (250, 650), (1000, 4000), (5000, 15000)], (0.25, 0.5, 0.75, 0.9), (),
                  dict(flux=1, centroid=1, entropy=1, variance=1, skewness=1, kurtosis=1, slope=1, harmonicity=1, sharpness=1)),
    "all": ([(0, 100), (100, 8000), (7999, 8000), (300, 301)], (0.9,), ((0, 500), (500, 1500)),
            dict(flux=1, centroid=1, max_pos=1, min_pos=1, entropy=1, variance=1, skewness=1, kurtosis=1, slope=1, sharpness=1, harmonicity=1,
                 flatness=1, spec_diff=1, spec_pos_diff=1, flux_centroid=1, flux_at_flux_centroid=1, standard_deviation=1)),
}


@pytest.mark.parametrize("K", [129, 257])
@pytest.mark.parametrize("name", list(OLD_SETS))
def test_equals_the_general_oracle(env, name, K, oracle):
    """linear options: the same bits as the oracle's lldo_spectral_general, which tests/test_oracle_pin_spectral_sets.py pins on the
    real binary. That is cSpectral on an FFT magnitude level, whose axis cTransformFFT attaches (frq[i] = i / frameSizeSec,
    transformFft.cpp:102-117), so that axis is what the operator gets here (without one the reference takes its index-based
    branches: another roll-off rounding, a running-sum centroid axis)."""
    bands, rolloff, slopes, flags = OLD_SETS[name]
    fs = 2.0 * (K - 1) / 16000.0
    x = spectra(K, 70, 3)
    want = oracle.spectral_general_rows(x, fs, bands, rolloff, slopes=slopes, **flags)
    o = opts(bands=tuple(bands), rolloff=rolloff, slopes=tuple(slopes), **flags)
    assert_bits(run_op(env, o, x, fs, np.arange(K, dtype=f64) / fs), want, name)


def test_equals_the_gemaps_operator(env, golden):
    """the two GeMAPS sets at 257 bins (smilehip_spectral_gemaps_frames: slopes 0-500 / 500-1500 of the log spectrum, alphaRatioDB,
    hammarbergIndexDB; flux over 0-5000 Hz) on the real binary's magnitude rows"""
    torch, capi, ctx = env
    plan = capi.Plan(ctx, capi.egemapsv02_config())
    try:
        fs = 0.032
        frq = np.arange(257, dtype=f64) / fs
        for key in ("u3_6400", "u10_4800"):
            x = np.ascontiguousarray(golden["out_" + key][:, :257])
            old = capi.spectral_gemaps_host(plan, x)
            four = run_op(env, CONF["gemaps"][1], x, fs, frq)
            flux = run_op(env, opts(flux=1, freq_range=(0, 5000), use_log_spectrum=1, norm_band_energies=1, old_slope_scale=0), x, fs, frq)
            new = np.concatenate([four, flux], axis=1)
            assert_bits(new, old, key)
    finally:
        plan.close()


REFUSALS = {
    "frq": (opts(flux=1), 16, np.array([0.0, 1, 2, 3, 3, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15])),
    "n_scale": (opts(flux=1), 16, np.arange(15.0)),
    "freqRange": (opts(flux=1, freq_range=(62, 62)), 16, np.arange(16.0) * 31.0),
    "tonality": (opts(flux=1, tonality=1), 16, None),
    "specFloor": (opts(flux=1, use_log_spectrum=1, spec_floor=-1.0), 16, None),
    "bands": (opts(bands=((650, 250),)), 16, None),
    "slopes": (opts(slopes=((5, 5),)), 16, None),
    "rollOff": (opts(rolloff=(1.5,)), 16, None),
    "K": (opts(flux=1), (1 << 20) + 1, None),
}


@pytest.mark.parametrize("what", list(REFUSALS))
def test_argument_checks(env, what):
    torch, capi, ctx = env
    L = capi.load()
    o, K, frq = REFUSALS[what]
    rc, op = create(env, o, K, 0.032, frq)
    assert rc == -1 and not op.value                         # SMILEHIP_ERR_INVALID
    assert what in L.smilehip_last_error().decode()


def test_frames_argument_checks(env):
    torch, capi, ctx = env
    L = capi.load()
    rc, op = create(env, opts(flux=1, centroid=1), 16, 0.032, None)
    capi._check(rc)
    d = torch.zeros(64, dtype=torch.float32, device="cuda")
    assert L.smilehip_spectral_axis_op_frames(op, d.data_ptr(), 16, None, 1, d.data_ptr(), 2, 1, None) == -1      # flux without a state buffer
    assert L.smilehip_spectral_axis_op_frames(op, d.data_ptr(), 15, d.data_ptr(), 1, d.data_ptr(), 2, 1, None) == -1   # ld_src < K
    assert L.smilehip_spectral_axis_op_frames(op, d.data_ptr(), 16, d.data_ptr(), 1, d.data_ptr(), 1, 1, None) == -1   # ld_dst < n_out
    assert L.smilehip_spectral_axis_op_frames(op, d.data_ptr(), 16, d.data_ptr(), 1, d.data_ptr(), 2, 0, None) == 0    # no frames: nothing to do
    capi._check(L.smilehip_spectral_axis_op_destroy(op))
