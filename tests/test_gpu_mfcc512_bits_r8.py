"""Round 8 reorders LDS traffic inside lld_mfcc512_body (the transposition stores behind the first DFT's last layer; behind
switches the order of the transposition loads and the mirror step as a DPP operand) and changes no arithmetic expression: every
output cell of every instance is the parent commit's, bit for bit.

The fixture tests/golden/mfcc512_parent_bits.npz was recorded on the GPU from the parent commit by
tools/dev/gen_mfcc512_parent_bits.py (which runs `run_case` below; the commit's hash is stored in the file as 40 hex digits).

One batch for every instance: utterances of 1, 3, 4, 5, 16, 17, 40, 253 and 1030 frames (synth.utterance seeds) -- the
lld_chain_short boundary, one pass and two passes, a length that is no multiple of 4, a tile cut with its halo passes, a wave
that walks on to a second tile.

The fixture has to stay below 1 MiB and 1369 frames x 39 columns are 214 KB, so four instances are recorded with their delta
and acceleration columns (the bench's own with the regression stages fused, the unaligned one with the separate window chain,
the forced padded kernel and the PLP chain -- 18 columns -- with the regression stages fused) and the other three with
nDelta = 0 (13 static columns, the instances without the fused stages): DELTA on and off are both covered, and every cell of
every recorded matrix is compared."""
import os

import numpy as np
import pytest

from tolerance import assert_bits_equal

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "mfcc512_parent_bits.npz")
FRAMES = (1, 3, 4, 5, 16, 17, 40, 253, 1030)
SEED0 = 800

# name -> (what the case changes in the MFCC12_0_D_A configuration, first sample offset of the batch, environment knobs,
#          the fast kernel that has to run)
CASES = {
    "bench": (dict(), 0, {}, "lld_mfcc512"),
    "unaligned": (dict(), 1, {}, "lld_mfcc512"),
    "force_padded": (dict(), 0, {"SMILEHIP_MFCC512_FORCE_PADDED": "1"}, "lld_mfcc512_padded"),
    "symmetric": (dict(zero_pad_symmetric=1, n_delta=0), 0, {}, "lld_mfcc512_padded"),
    "magnitude": (dict(use_power=0, n_delta=0), 0, {}, "lld_mfcc512"),
    "plp": (dict(plp=True), 0, {}, "lld_mfcc512"),
    "bands27": (dict(n_bands=27, n_delta=0), 0, {}, "lld_mfcc512"),
}


def make_config(capi, name):
    changes = CASES[name][0]
    cfg = capi.plp_0_d_a_config() if changes.get("plp") else capi.mfcc12_0_d_a_config()
    for k, v in changes.items():
        if k != "plp":
            setattr(cfg, k, v)
    return cfg


def run_case(capi, ctx, name):
    """The output matrix of the batch (all rows, float32) and the names of the kernels that ran."""
    from opensmile_amd import synth
    _, first, env, _ = CASES[name]
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        plan = capi.Plan(ctx, make_config(capi, name))
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    g = plan.geometry
    pcms = [synth.utterance(SEED0 + i, int(g.frame_size + (t - 1) * g.frame_step)) for i, t in enumerate(FRAMES)]
    off = (first + np.concatenate([[0], np.cumsum([len(p) for p in pcms])])).astype(np.int64)
    pcm = np.concatenate([np.zeros(first, np.int16)] + pcms)
    b = capi.Batch(plan, off)
    assert [int(n) for n in np.diff(b.frame_offsets)] == list(FRAMES)
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
def test_bits_equal_parent(hip, parent, name):
    capi, ctx = hip
    out, ran = run_case(capi, ctx, name)
    want = CASES[name][3]
    other = "lld_mfcc512" if want == "lld_mfcc512_padded" else "lld_mfcc512_padded"
    assert want in ran and other not in ran and "lld_mfcc_generic" not in ran, ran
    if name == "unaligned":
        assert "lld_chain_tiled" in ran, ran          # the separate window chain, not the fused regression stages
    assert np.isfinite(out).all()
    assert_bits_equal(out, parent[name], what=f"lld_mfcc512 instance '{name}' against the parent commit")
