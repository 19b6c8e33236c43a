"""Timing of the cSpectral operator (smilehip_spectral_axis_op_*) on seven linear option sets of tests/test_gpu_spectral_general.py
(on the FFT axis arange(K) / frameSizeSec), on a log-spectrum set (the GeMAPS options plus a third slope) and on a bark axis. HIP
events around one call, 3 warm-up calls, 20 timed calls per repeat, five repeats: the median of a repeat, and the spread of the
five medians. Prints the figures and writes them to the file given as the first argument (default: spectral_axis_timing.json in
the working directory); a second argument names the tree that was timed and is recorded as it is.
profiles/spectral_one_operator_timing.json is a run of this tool's earlier form, which timed the linear-set kernel that has since
been removed (smilehip_spectral_op_*, now a wrapper over this operator) against this one on the same rows in the same process,
the two alternating."""
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from opensmile_amd import capi  # noqa: E402
from test_gpu_spectral_general import SETS, SLOPES  # noqa: E402

L = capi.load()
ctx = capi.Context(0)
ROWS = 65536
LINEAR = ("avec2011", "avec2013", "emo_large", "mediaeval", "r6_all", "sixteen", "flux_only")
res = {"device": ctx.name(), "rows": ROWS, "tree": sys.argv[2] if len(sys.argv) > 2 else "",
       "method": "HIP events around one call; per repeat 3 warm-up calls and the median of 20; five repeats", "sizes": []}


def repeat(fn):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(20):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms)


def figures(meds):
    return {"median_ms": statistics.median(meds), "min_ms": min(meds), "max_ms": max(meds), "spread_ms": max(meds) - min(meds), "repeats_ms": meds}


def bark(x):
    if x <= 0:
        return 0.0
    zz = (26.81 / (1.0 + 1960.0 / x)) - 0.53
    return 0.85 * zz + 0.3 if zz < 2 else (1.22 * zz - 0.22 * 20.1 if zz > 20.1 else zz)


for K in (257, 1025):
    fs = (K - 1) * 2 / 16000.0
    torch.manual_seed(K)
    d_m = torch.rand((ROWS, K), dtype=torch.float32, device="cuda") ** 4
    frq = np.arange(K, dtype=np.float64) / fs

    def new_op(o, axis):
        op = C.c_void_p()
        capi._check(L.smilehip_spectral_axis_op_create(ctx._h, C.byref(o), K, fs, axis.ctypes.data, K, C.byref(op)))
        n = L.smilehip_spectral_axis_op_n_out(op)
        d_o = torch.zeros((ROWS, n), dtype=torch.float32, device="cuda")
        d_s = torch.zeros((K,), dtype=torch.float32, device="cuda")
        return op, d_o, (lambda: capi._check(L.smilehip_spectral_axis_op_frames(op, d_m.data_ptr(), K, d_s.data_ptr(), 1, d_o.data_ptr(), n, ROWS, None)))

    entry = {"K": K, "linear_sets": {}}
    for name in LINEAR:
        bands, flags = SETS[name]
        slopes = SLOPES.get(name, [])
        rolloff = (0.25, 0.5, 0.75, 0.9) if name != "flux_only" else ()
        new, _, run_new = new_op(capi.spectral_axis_opts(bands, rolloff, slopes, **flags), frq)
        entry["linear_sets"][name] = {"bands": len(bands), "slopes": len(slopes), "rolloff_points": len(rolloff), "descriptors": sorted(flags),
                                      "axis_operator": figures([repeat(run_new) for _ in range(5)])}
        print(json.dumps({"K": K, "set": name, **{k: v for k, v in entry["linear_sets"][name].items() if k != "descriptors"}}), flush=True)
        capi._check(L.smilehip_spectral_axis_op_destroy(new))
    log3, _, run_log = new_op(capi.spectral_axis_opts((), (), ((0, 500), (500, 1500), (1500, 3000)), use_log_spectrum=1, norm_band_energies=1,
                                                      alpha_ratio=1, hammarberg_index=1, old_slope_scale=0, freq_range=(0, 5000)), frq)
    bk, _, run_bark = new_op(capi.spectral_axis_opts(((2, 5), (8, 15)), (0.5, 0.9), (), sharpness=1, centroid=1),
                             np.array([bark(f) for f in frq[1:]] + [bark(frq[-1] + 1.0 / fs)]))
    m_log, m_bark = [], []
    for _ in range(5):
        m_log.append(repeat(run_log))
        m_bark.append(repeat(run_bark))
    entry["axis_operator_log_three_slopes"] = figures(m_log)
    entry["axis_operator_bark_axis"] = figures(m_bark)
    res["sizes"].append(entry)
    print(json.dumps({k: v for k, v in entry.items() if k != "linear_sets"}), flush=True)
    for op in (log3, bk):
        capi._check(L.smilehip_spectral_axis_op_destroy(op))
    del d_m
    torch.cuda.empty_cache()
json.dump(res, open(sys.argv[1] if len(sys.argv) > 1 else "spectral_axis_timing.json", "w"), indent=1)
