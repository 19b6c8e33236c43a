"""Changes of lld_mfcc512's LDS layout -- the band vectors 68 floats apart instead of 64; the loop-invariant tables (window, tw256,
tw512) in another order or read at another width -- change no arithmetic expression, operand or summation order: every output cell is
the parent commit's, bit for bit.

tests/golden/mfcc512_parent_bits.npz (tests/test_gpu_mfcc512_bits_r8.py) has no instance with MP = 16 (sixteen sample pairs per
lane: the largest window table) and none with UC = 8 (eight mel units per lane: the largest shared region in front of the per-wave
ones). Those are recorded here: a 32 ms frame (N = 512) gives MP = 16, and 24 mel bands give eight units per lane
(fast512_build_host: 80 units on 12 lanes; 26 bands give six) -- with the regression stages fused (integer sample loads at MP = 16)
and without (typed loads), and the PLP chain, whose vectors share the band vector's 68 floats, at MP = 16 with the regression stages
fused.

The fixture tests/golden/mfcc512_tables_parent_bits.npz was recorded on the GPU from the parent commit's library by
tools/dev/gen_mfcc512_tables_parent_bits.py (which runs `run_case` below; the commit's hash is stored in the file as 40 hex digits).

One batch for every instance: utterances of 1, 4, 5, 17 and 253 frames -- one pass, a ragged pass, and a tile cut with its halo."""
import os

import numpy as np
import pytest

from tolerance import assert_bits_equal

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "mfcc512_tables_parent_bits.npz")
FRAMES = (1, 4, 5, 17, 253)
SEED0 = 900

# name -> what the case changes in the MFCC12_0_D_A (plp: PLP_0_D_A) configuration
CASES = {
    "mp16_uc8_delta": dict(frame_size_sec=0.032, n_bands=24),
    "mp16_uc8_static": dict(frame_size_sec=0.032, n_bands=24, n_delta=0),
    "mp13_uc8_delta": dict(n_bands=24),
    "mp16_uc6_delta": dict(frame_size_sec=0.032),
    "plp_mp16_delta": dict(plp=True, frame_size_sec=0.032),
}


def make_config(capi, name):
    changes = CASES[name]
    cfg = capi.plp_0_d_a_config() if changes.get("plp") else capi.mfcc12_0_d_a_config()
    for k, v in changes.items():
        if k != "plp":
            setattr(cfg, k, v)
    return cfg


def run_case(capi, ctx, name):
    """The output matrix of the batch (all rows, float32) and the names of the kernels that ran."""
    from opensmile_amd import synth
    plan = capi.Plan(ctx, make_config(capi, name))
    g = plan.geometry
    assert g.frame_size == (512 if "mp16" in name else 400)
    pcms = [synth.utterance(SEED0 + i, int(g.frame_size + (t - 1) * g.frame_step)) for i, t in enumerate(FRAMES)]
    off = np.concatenate([[0], np.cumsum([len(p) for p in pcms])]).astype(np.int64)
    b = capi.Batch(plan, off)
    assert [int(n) for n in np.diff(b.frame_offsets)] == list(FRAMES)
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
    assert "lld_mfcc512" in ran and "lld_mfcc512_padded" not in ran and "lld_mfcc_generic" not in ran, ran
    assert np.isfinite(out).all()
    assert out.shape == parent[name].shape and out.shape[0] == sum(FRAMES)
    assert_bits_equal(out, parent[name], what=f"lld_mfcc512 instance '{name}' against the parent commit")
