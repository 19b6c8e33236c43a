"""lld_mfcc512 deals the columns of the second DFT16 to the lanes by the map kc = 0 .. 7, 9 .. 15, 8, so that the untangle partner of
lanes 1 .. 14 sits opposite under row_mirror (one DPP move per value), lane 15 (column 8) is its own partner in the same register
and lane 0 (column 0) one register up. No arithmetic expression, operand or summation order changes: every output cell is the
parent commit's, bit for bit.

What only this change can break is the pairing itself: the two self-paired columns 0 and 8 (bins 16 q and 8 + 16 q, with DC,
Nyquist and bin 128 among them) and every lane's partner. So beside seeded noise the signals put their energy where one wrong pair
shows: all zeros, a constant (DC only), +-A alternating (Nyquist only), single tones at the bin centres k x 31.25 Hz for k = 8, 16,
120, 128, 136, 248 (the self-paired columns, low, middle and high) and one tone per lane column, k = 1 .. 15. Every signal as
utterances of 1, 4, 5 and 17 frames: one pass, a ragged pass, several passes.

Instances: the bench's own, magnitude instead of power, zero_pad_symmetric (the padded kernel), a 32 ms frame (MP = 16: sixteen
sample pairs per lane) with the regression stages and without, 24 bands (UC = 8: eight mel units per lane) and the PLP chain.

The fixture tests/golden/mfcc512_untangle_parent_bits.npz was recorded on the GPU from the parent commit's library by
tools/dev/gen_mfcc512_untangle_parent_bits.py (which runs `run_case` below; the commit's hash is stored in the file as 40 hex
digits)."""
import os

import numpy as np
import pytest

from tolerance import assert_bits_equal

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "mfcc512_untangle_parent_bits.npz")
FRAMES = (1, 4, 5, 17)
SEED0 = 1300
AMP = 8000.0
TONES = (8, 16, 120, 128, 136, 248) + tuple(range(1, 16))          # bin centres k x 31.25 Hz at 16 kHz
SIGNALS = ("noise", "zeros", "dc", "nyquist") + tuple("tone%d" % k for k in TONES)

# name -> (what the case changes in the MFCC12_0_D_A (plp: PLP_0_D_A) configuration, the fast kernel that has to run)
CASES = {
    "bench": (dict(), "lld_mfcc512"),
    "magnitude": (dict(use_power=0, n_delta=0), "lld_mfcc512"),
    "symmetric": (dict(zero_pad_symmetric=1, n_delta=0), "lld_mfcc512_padded"),
    "mp16_delta": (dict(frame_size_sec=0.032), "lld_mfcc512"),
    "mp16_static": (dict(frame_size_sec=0.032, n_delta=0), "lld_mfcc512"),
    "uc8": (dict(n_bands=24), "lld_mfcc512"),
    "plp": (dict(plp=True), "lld_mfcc512"),
}


def make_config(capi, name):
    changes = CASES[name][0]
    cfg = capi.plp_0_d_a_config() if changes.get("plp") else capi.mfcc12_0_d_a_config()
    for k, v in changes.items():
        if k != "plp":
            setattr(cfg, k, v)
    return cfg


def signal(kind, seed, n):
    """n int16 samples of one utterance"""
    from opensmile_amd import synth
    t = np.arange(n, dtype=np.float64)
    if kind == "noise":
        return synth.utterance(seed, n)
    if kind == "zeros":
        return np.zeros(n, np.int16)
    if kind == "dc":
        return np.full(n, 5000, np.int16)
    if kind == "nyquist":
        return np.where(np.arange(n) & 1, -AMP, AMP).astype(np.int16)
    k = int(kind[4:])
    return np.round(AMP * np.cos(2.0 * np.pi * k * t / 512.0 + 0.3)).astype(np.int16)


def run_case(capi, ctx, name):
    """The output matrix of the batch (all rows, float32) and the names of the kernels that ran."""
    plan = capi.Plan(ctx, make_config(capi, name))
    g = plan.geometry
    assert g.frame_size == (512 if "mp16" in name else 400)
    pcms, want = [], []
    for s, kind in enumerate(SIGNALS):
        for i, t in enumerate(FRAMES):
            pcms.append(signal(kind, SEED0 + 4 * s + i, int(g.frame_size + (t - 1) * g.frame_step)))
            want.append(t)
    off = np.concatenate([[0], np.cumsum([len(p) for p in pcms])]).astype(np.int64)
    b = capi.Batch(plan, off)
    assert [int(n) for n in np.diff(b.frame_offsets)] == want
    capi.kernel_timing(True)
    try:
        out = b.run_host(np.concatenate(pcms))
        ran = {k.strip("( ") for k in capi.kernel_timing_report()}
    finally:
        capi.kernel_timing(False)
    b.close()
    plan.close()
    return out, ran


@pytest.fixture(scope="module")
def hip():
    from opensmile_amd import capi
    ctx = capi.Context(0)
    assert "gfx950" in ctx.name()
    return capi, ctx


@pytest.fixture(scope="module")
def parent():
    z = np.load(GOLDEN)
    assert all(z[k].dtype == np.float32 for k in z.files)
    return z


@pytest.mark.parametrize("name", list(CASES))
def test_bits_equal_parent(hip, parent, name):
    capi, ctx = hip
    out, ran = run_case(capi, ctx, name)
    want = CASES[name][1]
    other = "lld_mfcc512" if want == "lld_mfcc512_padded" else "lld_mfcc512_padded"
    assert want in ran and other not in ran and "lld_mfcc_generic" not in ran, ran
    assert np.isfinite(out).all()
    assert out.shape == parent[name].shape and out.shape[0] == len(SIGNALS) * sum(FRAMES)
    assert_bits_equal(out, parent[name], what=f"lld_mfcc512 instance '{name}' against the parent commit")
