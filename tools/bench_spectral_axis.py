"""Timing of the cSpectral operator for any option set (smilehip_spectral_axis_op_*) against the older general
operator (smilehip_spectral_op_*) on the option set both serve (the `mediaeval` set of
tests/test_gpu_spectral_general.py), on the same rows, in the same process; and of the new operator alone on a log-spectrum set (the
GeMAPS options plus a third slope) and on a bark axis. HIP events around one call, 3 warm-up calls, 20 timed calls per repeat, five
repeats: the median of a repeat, and the spread of the five medians. Prints the figures and writes them to the file given as the
first argument (default: spectral_axis_timing.json in the working directory); profiles/spectral_axis_timing.json is one run of it."""
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from opensmile_amd import capi  # noqa: E402

L = capi.load()
ctx = capi.Context(0)
ROWS = 65536
res = {"device": ctx.name(), "rows": ROWS,
       "method": "HIP events around one call; per repeat 3 warm-up calls and the median of 20; five repeats, old and new alternating", "sizes": []}


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


BANDS = [(40, 150), (250, 650), (1000, 4000), (5000, 15000)]
ROLLOFF = (0.25, 0.5, 0.75, 0.9)
FLAGS = dict(flux=1, centroid=1, entropy=1, variance=1, skewness=1, kurtosis=1, slope=1, harmonicity=1, sharpness=1)

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

    oo = capi.spectral_opts(BANDS, ROLLOFF, (), **FLAGS)
    old = C.c_void_p()
    capi._check(L.smilehip_spectral_op_create(ctx._h, C.byref(oo), K, fs, C.byref(old)))
    n_old = L.smilehip_spectral_op_n_out(old)
    d_a = torch.zeros((ROWS, n_old), dtype=torch.float32, device="cuda")
    d_sa = torch.zeros((K,), dtype=torch.float32, device="cuda")
    run_old = lambda: capi._check(L.smilehip_spectral_op_frames(old, d_m.data_ptr(), K, d_sa.data_ptr(), 1, d_a.data_ptr(), n_old, ROWS, None))  # noqa: E731
    shared, d_b, run_shared = new_op(capi.spectral_axis_opts(BANDS, ROLLOFF, (), **FLAGS), frq)
    log3, _, run_log = new_op(capi.spectral_axis_opts((), (), ((0, 500), (500, 1500), (1500, 3000)), use_log_spectrum=1, norm_band_energies=1,
                                                      alpha_ratio=1, hammarberg_index=1, old_slope_scale=0, freq_range=(0, 5000)), frq)
    bk, _, run_bark = new_op(capi.spectral_axis_opts(((2, 5), (8, 15)), (0.5, 0.9), (), sharpness=1, centroid=1),
                             np.array([bark(f) for f in frq[1:]] + [bark(frq[-1] + 1.0 / fs)]))
    m_old, m_new, m_log, m_bark = [], [], [], []
    for _ in range(5):
        m_old.append(repeat(run_old))
        m_new.append(repeat(run_shared))
        m_log.append(repeat(run_log))
        m_bark.append(repeat(run_bark))
    eq = bool(((d_a.view(torch.int32) == d_b.view(torch.int32)) | ((d_a == 0) & (d_b == 0))).all())
    entry = {"K": K, "shared_set": "mediaeval (4 bands, 4 roll-off points, 9 descriptors)", "general_operator": figures(m_old),
             "axis_operator": figures(m_new), "axis_over_general": statistics.median(m_new) / statistics.median(m_old), "rows_bit_equal": eq,
             "axis_operator_log_three_slopes": figures(m_log), "axis_operator_bark_axis": figures(m_bark)}
    res["sizes"].append(entry)
    print(json.dumps(entry), flush=True)
    capi._check(L.smilehip_spectral_op_destroy(old))
    for op in (shared, log3, bk):
        capi._check(L.smilehip_spectral_axis_op_destroy(op))
    del d_m, d_a, d_b
    torch.cuda.empty_cache()
json.dump(res, open(sys.argv[1] if len(sys.argv) > 1 else "spectral_axis_timing.json", "w"), indent=1)
