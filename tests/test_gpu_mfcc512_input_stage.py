"""The fast Nfft = 512 kernel's input stage (conversion, pre-emphasis, window) at the places it treats specially:
the frame's first sample y[0] = (1-k) x[0] (lane 0, register 0 without zero padding -- lld_mfcc512 -- and a runtime
lane / register under symmetric zero padding -- lld_mfcc512_padded), the predecessor sample of every lane and register
(the neighbour lane's odd sample; lane 0 takes lane 15's of the register one pair down), and utterances whose first
frame starts at the buffer's first sample or whose last frame ends at its last one. Each case against the CPU oracle
at the gate and against the reference-order kernel on the same input."""
import os

import numpy as np
import pytest

from tolerance import assert_parity

pytestmark = pytest.mark.gpu

N, H = 400, 160          # 25 ms / 10 ms at 16 kHz


@pytest.fixture(scope="module")
def hip():
    from opensmile_amd import capi
    ctx = capi.Context(0)
    assert "gfx950" in ctx.name()
    return capi, ctx


def _plan(capi, ctx, cfg, env):
    """A plan made with the given environment knobs set (and the caller's values put back afterwards)."""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return capi.Plan(ctx, cfg)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _run(capi, ctx, cfg, pcms, generic, padded=False):
    """Rows per utterance, and the names of the kernels that ran (template arguments stripped)."""
    plan = _plan(capi, ctx, cfg, {"SMILEHIP_FORCE_GENERIC": "1" if generic else "0",
                                  "SMILEHIP_MFCC512_FORCE_PADDED": "1" if padded else "0"})
    off = np.concatenate([[0], np.cumsum([len(p) for p in pcms])]).astype(np.int64)
    b = capi.Batch(plan, off)
    capi.kernel_timing(True)
    try:
        out = b.run_host(np.concatenate(pcms))
        ran = {k.strip("( ") for k in capi.kernel_timing_report()}
    finally:
        capi.kernel_timing(False)
    rows = [out[b.frame_offsets[i]:b.frame_offsets[i + 1]].copy() for i in range(len(pcms))]
    b.close()
    plan.close()
    return rows, ran


def _fast(ran, padded):
    """Exactly one of the two fast kernels ran: lld_mfcc512_padded if `padded`, else lld_mfcc512."""
    want, other = ("lld_mfcc512_padded", "lld_mfcc512") if padded else ("lld_mfcc512", "lld_mfcc512_padded")
    return want in ran and other not in ran


def _impulse_utterances():
    """Low-level noise with a full-scale impulse at sample p of frame 1 for every pair position: p = 2 (j + 16 m) and
    p = 2 (j + 16 m) + 1 walk all 16 lanes and all 13 registers, so every predecessor x[2n - 1] (the lane 0 ones from the
    register one pair down included) and the first sample itself carry a value that dominates the frame."""
    rng = np.random.default_rng(7)
    pcms = []
    for p in list(range(0, 34)) + [2 * (j + 16 * m) + o for m in (1, 5, 12) for j in (0, 1, 15) for o in (0, 1)] + [398, 399]:
        x = rng.integers(-40, 41, size=H + N + 3 * H).astype(np.int16)
        x[H + p] = 32767 if p % 3 else -32768
        pcms.append(x)
    return pcms


def _cfg(capi, oracle, sym):
    cfg = capi.mfcc12_0_d_a_config()
    oc = oracle.default_cfg()
    cfg.zero_pad_symmetric = oc.zero_pad_symmetric = sym
    return cfg, oc


@pytest.mark.parametrize("sym", [False, True], ids=["pad0", "symmetric"])
def test_first_and_predecessor_samples_vs_oracle(hip, oracle, sym):
    capi, ctx = hip
    cfg, oc = _cfg(capi, oracle, sym)
    pcms = _impulse_utterances()
    fast, ran = _run(capi, ctx, cfg, pcms, generic=False)
    assert _fast(ran, padded=sym), ran
    gen, ran = _run(capi, ctx, cfg, pcms, generic=True)
    assert "lld_mfcc512" not in ran and "lld_mfcc512_padded" not in ran, ran
    for i, p in enumerate(pcms):
        ref = oracle.mfcc_chain(oc, p)
        assert fast[i].shape == ref.shape == gen[i].shape
        assert_parity(fast[i], ref, block=13, what=f"fast, impulse utterance {i}, sym={sym}")
        assert_parity(fast[i], gen[i], block=13, what=f"fast vs reference-order kernel, impulse utterance {i}, sym={sym}")


@pytest.mark.parametrize("sym", [False, True], ids=["pad0", "symmetric"])
def test_buffer_start_and_end(hip, oracle, sym):
    """The batch's first utterance starts at the buffer's first sample (its first frame's predecessor and, under
    symmetric padding, its left padding lie in front of the buffer) and the last one's last frame ends at the
    buffer's last sample; a one-frame utterance sits between them."""
    from opensmile_amd import synth
    capi, ctx = hip
    cfg, oc = _cfg(capi, oracle, sym)
    pcms = [synth.utterance(70, N + 37 * H), synth.utterance(71, N), synth.utterance(72, N + 12 * H)]
    for p in (pcms[0], pcms[-1]):
        p[0] = 30000
        p[-1] = -30000
    fast, ran = _run(capi, ctx, cfg, pcms, generic=False)
    assert _fast(ran, padded=sym), ran
    gen, _ = _run(capi, ctx, cfg, pcms, generic=True)
    for i, p in enumerate(pcms):
        ref = oracle.mfcc_chain(oc, p)
        assert fast[i].shape == ref.shape == gen[i].shape
        assert_parity(fast[i], ref, block=13, what=f"fast, utterance {i}, sym={sym}")
        assert_parity(fast[i], gen[i], block=13, what=f"fast vs reference-order kernel, utterance {i}, sym={sym}")


def test_pad0_kernel_equals_padded_kernel(hip, oracle):
    """At pad_left = 0 the specialised kernel (the fix-up at lane 0, register 0, fixed at compile time) and the general one (the
    same position as a runtime value) compute the same thing: the same operations on the same values, so the same bits -- on
    the impulse utterances (every lane and register) and on utterances that start and end at the buffer's ends."""
    from opensmile_amd import synth
    capi, ctx = hip
    cfg, _ = _cfg(capi, oracle, False)
    pcms = _impulse_utterances() + [synth.utterance(73, N + 40 * H), synth.utterance(74, N + 3 * H)]
    spec, ran_s = _run(capi, ctx, cfg, pcms, generic=False, padded=False)
    gen, ran_g = _run(capi, ctx, cfg, pcms, generic=False, padded=True)
    assert _fast(ran_s, padded=False), ran_s
    assert _fast(ran_g, padded=True), ran_g
    for i in range(len(pcms)):
        np.testing.assert_array_equal(spec[i], gen[i], err_msg=f"utterance {i}")
