"""lld_mfcc512 moves the 16 x 16 transposition between its two DFT16 through a split-complex buffer: a plane of real and a plane of
imaginary parts, each row 64 consecutive floats (one per lane), written by two address-free stores per index (the address is M0 +
an immediate + 4 x lane) and read back sixteen floats at a time (ds_read_b128). The first DFT16 of the MP = 13 instances also drops
six additions of a literal zero. No arithmetic expression, operand or summation order that reaches the output changes: every output
cell is the parent commit's, bit for bit. Instances that keep the interleaved buffer (split_transpose() in the kernel source) are
in the fixture too: the rule must not change them.

What only this change can break is the way of one value through the buffer: writer lane (g, j) puts index k1 into row k1 of its
plane, reader lane (g, kc) takes columns 0 .. 15 of row kc. So beside seeded noise, zeros and a constant the signals put their
energy into ONE sample pair: an impulse at pair j for j = 0 .. 15 (one writer lane each, all sixteen rows; in a frame of several the
hop of 80 pairs = 5 x 16 keeps it in that lane) and an impulse at pair 16 m for m = 0 .. 12 (every input index of the first DFT16
of lane 0, the three literal zeros of MP = 13 behind them). Noise, zeros and the constant as utterances of 1, 4, 5 and 17 frames
(one pass, a ragged pass, several passes), the impulses as 1 and 5 frames: 70 utterances per batch, so that all eight waves of a
block -- eight regions of the buffer -- work.

Instances: the bench's own, magnitude instead of power, zero_pad_symmetric (the padded kernel), a 32 ms frame (MP = 16: sixteen
sample pairs per lane) with the regression stages and without, 24 bands (UC = 8: eight mel units per lane) and the PLP chain.

The fixture tests/golden/mfcc512_split_transpose_parent_bits.npz was recorded on the GPU from the parent commit's library by
tools/dev/gen_mfcc512_split_transpose_parent_bits.py (which runs `run_case` below; the commit's hash is stored in the file as 40
hex digits)."""
import os

import numpy as np
import pytest

from tolerance import assert_bits_equal

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "mfcc512_split_transpose_parent_bits.npz")
FRAMES = (1, 4, 5, 17)
FRAMES_IMPULSE = (1, 5)
SEED0 = 1700
HOP = 160                                                          # samples between frames (10 ms at 16 kHz)
# (signal, frames per utterance)
SIGNALS = tuple((s, FRAMES) for s in ("noise", "zeros", "dc")) \
    + tuple(("pair%d" % n, FRAMES_IMPULSE) for n in range(16)) \
    + tuple(("pair%d" % (16 * m), FRAMES_IMPULSE) for m in range(1, 13))
UTTERANCES = tuple((s, t) for s, ts in SIGNALS for t in ts)

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
    if kind == "noise":
        return synth.utterance(seed, n)
    if kind == "zeros":
        return np.zeros(n, np.int16)
    if kind == "dc":
        return np.full(n, 5000, np.int16)
    # pair p of every frame: the even sample (real part) and, smaller and negative, the odd one (imaginary part)
    p = int(kind[4:])
    x = np.zeros(n, np.int16)
    x[2 * p::HOP] = 20000
    x[2 * p + 1::HOP] = -12000
    return x


def run_case(capi, ctx, name):
    """The output matrix of the batch (all rows, float32) and the names of the kernels that ran."""
    plan = capi.Plan(ctx, make_config(capi, name))
    g = plan.geometry
    assert g.frame_size == (512 if "mp16" in name else 400) and g.frame_step == HOP
    pcms = [signal(kind, SEED0 + i, int(g.frame_size + (t - 1) * g.frame_step)) for i, (kind, t) in enumerate(UTTERANCES)]
    off = np.concatenate([[0], np.cumsum([len(p) for p in pcms])]).astype(np.int64)
    b = capi.Batch(plan, off)
    assert [int(n) for n in np.diff(b.frame_offsets)] == [t for _, t in UTTERANCES]
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


def test_batch_reaches_every_wave_region():
    assert len(UTTERANCES) >= 16
    assert {s for s, _ in SIGNALS} >= {"pair%d" % n for n in range(16)} | {"pair%d" % (16 * m) for m in range(13)}


@pytest.mark.parametrize("name", list(CASES))
def test_bits_equal_parent(hip, parent, name):
    capi, ctx = hip
    out, ran = run_case(capi, ctx, name)
    want = CASES[name][1]
    other = "lld_mfcc512" if want == "lld_mfcc512_padded" else "lld_mfcc512_padded"
    assert want in ran and other not in ran and "lld_mfcc_generic" not in ran, ran
    assert np.isfinite(out).all()
    assert out.shape == parent[name].shape and out.shape[0] == sum(t for _, t in UTTERANCES)
    assert_bits_equal(out, parent[name], what=f"lld_mfcc512 instance '{name}' against the parent commit")
