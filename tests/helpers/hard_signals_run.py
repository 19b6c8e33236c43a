"""Runs the hard-signal corpus (hard_signals.py) as ONE ragged batch through the C ABI, for tests/test_gpu_hard_signals.py: in the
test's own process, or -- for a switch the library reads once per process (SMILEHIP_COMPARE_BLOCK) -- as a child process:

    python tests/helpers/hard_signals_run.py <set> <order> <out.npz>        (switches in the environment)

Sets: mfcc, plp (MFCC12_0_D_A / PLP_0_D_A), is09, compare16, egemaps. Orders: "forward" = the fifteen signals; "mixed" = the same
in reverse order with an empty utterance and a 100-sample utterance in between."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)

from helpers import hard_signals  # noqa: E402

SWITCHES = ("SMILEHIP_FORCE_GENERIC", "SMILEHIP_IS09", "SMILEHIP_COMPARE_WAVE", "SMILEHIP_COMPARE_BLOCK", "SMILEHIP_GEMAPS_WAVE")


def batch_of(order):
    """[(signal name or None, samples)] of a batch order."""
    sig = hard_signals.signals()
    if order == "forward":
        return [(n, sig[n]) for n in hard_signals.NAMES]
    assert order == "mixed"
    utts = [(n, sig[n]) for n in reversed(hard_signals.NAMES)]
    utts.insert(5, (None, np.zeros(0, np.int16)))
    utts.insert(11, (None, sig["full_range_noise"][:100].copy()))
    return utts


def run(set_name, order, switches=None):
    """{lld: all rows, rows: row offsets per utterance, func: n_utt x F or absent, b_extra (compare16), ran: kernel names}; every
    switch of SWITCHES is removed from the environment for the run unless `switches` sets it (SMILEHIP_COMPARE_BLOCK only counts
    at the process's first ComParE launch: give it to a child process)."""
    from opensmile_amd import capi
    saved = {k: os.environ.pop(k, None) for k in SWITCHES}
    os.environ.update(switches or {})
    ctx = capi.Context(0)
    cfg = {"mfcc": capi.mfcc12_0_d_a_config, "plp": capi.plp_0_d_a_config, "is09": capi.is09_lld_config,
           "compare16": capi.compare16_config, "egemaps": capi.egemapsv02_config}[set_name]()
    try:
        plan = capi.Plan(ctx, cfg)
        utts = batch_of(order)
        off = np.concatenate([[0], np.cumsum([len(p) for _, p in utts])]).astype(np.int64)
        pcm = np.concatenate([p for _, p in utts])
        b = capi.Batch(plan, off)
        capi.kernel_timing(True)
        try:
            res = {}
            if set_name in ("mfcc", "plp"):
                res["lld"] = b.run_host(pcm)
            elif set_name == "is09":
                res["lld"] = b.run_host(pcm)
                res["func"] = b.functionals_host(res["lld"])
            elif set_name == "compare16":
                res["lld"], res["func"], res["b_extra"] = b.run_host_with_functionals16(pcm)
            else:
                res["lld"], res["func"] = b.run_host_egemaps(pcm)
            res["ran"] = np.array(sorted(k.strip("( ") for k in capi.kernel_timing_report()))
        finally:
            capi.kernel_timing(False)
        res["rows"] = b.frame_offsets.copy()
        b.close()
        plan.close()
    finally:
        ctx.close()
        for k in SWITCHES:
            os.environ.pop(k, None)
            if saved[k] is not None:
                os.environ[k] = saved[k]
    return res


if __name__ == "__main__":
    try:
        import torch  # noqa: F401  (first, so that the library binds to the HIP runtime torch brings: tests/conftest.py)
    except Exception:
        pass
    np.savez(sys.argv[3], **run(sys.argv[1], sys.argv[2], {k: os.environ[k] for k in SWITCHES if k in os.environ}))
