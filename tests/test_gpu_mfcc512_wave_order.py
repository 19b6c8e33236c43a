"""lld_mfcc512's waves set their issue priority per pass and may start a fixed delay apart: that changes WHEN an instruction issues,
never what it computes -- every output cell is the parent commit's, bit for bit.

The bench instance (MFCC12_0_D_A with the fused regression stages, lld_mfcc512<13, true, true, true, false, 6, true>) on the two
batches in which the waves of one SIMD are furthest from running in step:

  ragged   eight seeded utterances of 17, 18, 20, 21, 24, 33, 61 and 253 frames: one block whose waves run pass counts that differ
           by more than tenfold, side by side on the same SIMDs.
  tiled    eight distinct 17-frame utterances tiled to 4 104 copies (25 MB of PCM): more tiles than the 4 096 wave slots of the
           resident grid, so some waves move on to a second tile and their pass count -- and with it the priority -- runs across
           a tile change. Every copy's rows equal the rows of its original.

The fixture tests/golden/mfcc512_wave_order_parent_bits.npz was recorded on the GPU from the parent commit's library by
tools/dev/gen_mfcc512_wave_order_parent_bits.py (which runs `run_case` below; the commit's hash is stored in the file as 40 hex
digits). For `tiled` it holds the rows of the eight originals (on the parent every copy gave them: the generator checks it)."""
import os

import numpy as np
import pytest

from tolerance import assert_bits_equal

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "mfcc512_wave_order_parent_bits.npz")
RAGGED_FRAMES = (17, 18, 20, 21, 24, 33, 61, 253)
TILED_FRAMES, TILED_UNIQUE, TILED_COPIES = 17, 8, 4104
WAVE_SLOTS = 4096                       # 256 CUs x 2 blocks x 8 waves
SEED0 = 1300

CASES = ("ragged", "tiled")


def case_frames(name):
    return list(RAGGED_FRAMES) if name == "ragged" else [TILED_FRAMES] * TILED_COPIES


def run_case(capi, ctx, name):
    """The output matrix of the batch (all rows, float32) and the names of the kernels that ran."""
    from opensmile_amd import synth
    plan = capi.Plan(ctx)                   # MFCC12_0_D_A
    g = plan.geometry
    assert g.frame_size == 400 and g.n_out == 39
    frames = case_frames(name)
    n_unique = len(frames) if name == "ragged" else TILED_UNIQUE
    unique = [synth.utterance(SEED0 + i, int(g.frame_size + (frames[i] - 1) * g.frame_step)) for i in range(n_unique)]
    pcms = [unique[i % n_unique] for i in range(len(frames))]
    off = np.concatenate([[0], np.cumsum([len(p) for p in pcms])]).astype(np.int64)
    b = capi.Batch(plan, off)
    assert [int(n) for n in np.diff(b.frame_offsets)] == frames
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


def check_ran(out, ran, name):
    assert "lld_mfcc512" in ran and "lld_mfcc512_padded" not in ran and "lld_mfcc_generic" not in ran, ran
    assert "lld_chain_tiled" not in ran, ran          # the regression stages are the fused ones
    assert np.isfinite(out).all()
    assert out.shape == (sum(case_frames(name)), 39)


def test_ragged_bits_equal_parent(hip, parent):
    capi, ctx = hip
    out, ran = run_case(capi, ctx, "ragged")
    check_ran(out, ran, "ragged")
    assert_bits_equal(out, parent["ragged"], what="lld_mfcc512, ragged batch, against the parent commit")


def test_tiled_bits_equal_parent_across_tile_change(hip, parent):
    capi, ctx = hip
    assert TILED_COPIES > WAVE_SLOTS
    out, ran = run_case(capi, ctx, "tiled")
    check_ran(out, ran, "tiled")
    gold = parent["tiled"]
    assert gold.shape == (TILED_UNIQUE * TILED_FRAMES, 39)
    expect = np.tile(gold.reshape(1, TILED_UNIQUE * TILED_FRAMES, 39), (TILED_COPIES // TILED_UNIQUE, 1, 1)).reshape(-1, 39)
    assert expect.shape == out.shape
    assert_bits_equal(out, expect, what="lld_mfcc512, 4 104 tiled copies, every copy against the parent commit's rows of its original")
