"""Round 9 lets the buffer unit convert the int16 samples of lld_mfcc512 to float (typed buffer loads, format 16_16 / 16 with
SSCALED numbers) where the parent loaded integers and converted them on the vector ALU. (float)x is exact for every int16 x, so
every later operation sees the parent's operands and every output cell is the parent commit's, bit for bit -- provided the
device's typed load really returns (float)int16 for EVERY value, in both components. That is what this test pins.

Input: one utterance, a seeded permutation of all 65 536 int16 values, one zero, the same permutation again (now on the other
parity) and zeros up to a whole number of frames: every value, -32768 included, passes through the even (.x) and through the odd
(.y) sample of a pair, and every sample lies inside a frame. 131 120 samples = 818 frames of 25 ms every 10 ms, 39 columns.

Cases: the bench's own instance (aligned input: one tbuffer_load_format_xy per pair), the same batch starting at an odd sample
(unaligned input: two tbuffer_load_format_x per pair, the separate window chain) and the forced padded kernel.

The fixture tests/golden/mfcc512_allvalues_parent_bits.npz was recorded on the GPU from the PARENT commit's library by
tools/dev/gen_mfcc512_allvalues_parent_bits.py (which runs `run_case` below; the commit's hash is stored in the file as 40 hex
digits) -- never from the code under test. A wrong destination select or an unsupported format would show here as zeros or NaNs:
a failed comparison, not a fault."""
import os

import numpy as np
import pytest

from tolerance import assert_bits_equal

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "mfcc512_allvalues_parent_bits.npz")
SEED = 909

# name -> (first sample offset of the batch, environment knobs, the fast kernel that has to run)
CASES = {
    "bench": (0, {}, "lld_mfcc512"),
    "unaligned": (1, {}, "lld_mfcc512"),
    "force_padded": (0, {"SMILEHIP_MFCC512_FORCE_PADDED": "1"}, "lld_mfcc512_padded"),
}


def all_values_utterance(frame_size, frame_step):
    """permutation | 0 | permutation | zeros up to the end of the last frame that holds a permuted sample"""
    perm = (np.random.default_rng(SEED).permutation(65536) - 32768).astype(np.int16)
    assert np.array_equal(np.sort(perm), np.arange(-32768, 32768, dtype=np.int16))
    body = np.concatenate([perm, np.zeros(1, np.int16), perm])
    n_frames = -(-(len(body) - frame_size) // frame_step) + 1
    pcm = np.zeros(frame_size + (n_frames - 1) * frame_step, np.int16)
    pcm[:len(body)] = body
    return pcm, n_frames


def run_case(capi, ctx, name):
    """The output matrix of the one-utterance batch (all rows, float32) and the names of the kernels that ran."""
    first, env, _ = CASES[name]
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        plan = capi.Plan(ctx, capi.mfcc12_0_d_a_config())
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    g = plan.geometry
    utt, n_frames = all_values_utterance(int(g.frame_size), int(g.frame_step))
    # both parities of every value
    for parity in (0, 1):
        assert len(np.unique(utt[parity::2])) == 65536
    off = np.array([first, first + len(utt)], np.int64)
    pcm = np.concatenate([np.zeros(first, np.int16), utt])
    b = capi.Batch(plan, off)
    assert [int(n) for n in np.diff(b.frame_offsets)] == [n_frames]
    capi.kernel_timing(True)
    try:
        out = b.run_host(pcm)
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
def test_all_int16_values_bits_equal_parent(hip, parent, name):
    capi, ctx = hip
    out, ran = run_case(capi, ctx, name)
    want = CASES[name][2]
    other = "lld_mfcc512" if want == "lld_mfcc512_padded" else "lld_mfcc512_padded"
    assert want in ran and other not in ran and "lld_mfcc_generic" not in ran, ran
    if name == "unaligned":
        assert "lld_chain_tiled" in ran, ran          # the separate window chain, not the fused regression stages
    assert out.shape == (818, 39)
    assert np.isfinite(out).all()
    assert_bits_equal(out, parent[name], what=f"lld_mfcc512 '{name}' on all int16 values against the parent commit")
