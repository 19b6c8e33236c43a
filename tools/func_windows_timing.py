"""Timing of the functionals over fixed windows: HIP events, warm, median of 20. IS09's spec on 32 columns of seeded data, windows of
200 rows every 50, in two shapes -- (a) one utterance of 60 000 rows through smilehip_funcspec_matrix_windows, (b) 8 000 utterances of
1 000 rows through smilehip_batch_funcspec_windows -- each against the only route there was before: a host loop of
smilehip_funcspec_matrix over the same slices, timed in the same process (where one pass of that loop takes seconds, the loop is timed
as the median of 3 and the file says so). Writes the file given as the first argument (default: profiles/func_windows_timing.json);
--no-baseline leaves the loop out."""
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

SIZE, STEP, COLS = 200, 50, 32


def timed(fn, reps=20, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out_path = args[0] if args else os.path.join(ROOT, "profiles", "func_windows_timing.json")
    baseline = "--no-baseline" not in sys.argv
    L = capi.load()
    ctx = capi.Context(0)
    spec = capi.funcspec_is09()
    per = capi.funcspec_count(spec)
    res = {"device": ctx.name(), "spec": "IS09_emotion (12 values per column)", "cols": COLS, "size_rows": SIZE, "step_rows": STEP,
           "method": "HIP events around one call (or one pass of the loop), 3 warm-up calls, median of 20", "shapes": []}
    plan = capi.Plan(ctx, capi.is09_lld_config())
    for name, n_utt, rows in (("one utterance of 60000 rows", 1, 60000), ("8000 utterances of 1000 rows", 8000, 1000)):
        torch.manual_seed(rows)
        d_x = torch.randn((n_utt * rows, COLS), dtype=torch.float32, device="cuda")
        n_win = n_utt * ((rows - SIZE) // STEP + 1)
        d_f = torch.zeros((n_win, COLS * per), dtype=torch.float32, device="cuda")
        d_g = torch.zeros((n_win, COLS * per), dtype=torch.float32, device="cuda")
        if n_utt == 1:
            def windows():
                capi._check(L.smilehip_funcspec_matrix_windows(ctx._h, C.byref(spec), d_x.data_ptr(), COLS, rows, COLS, SIZE, STEP,
                                                               d_f.data_ptr(), COLS * per, None))
            batch = None
        else:
            # an IS09 batch whose utterances have `rows` LLD rows each (25 ms frames every 10 ms, one row more than frames)
            n_samp = 400 + 160 * (rows - 2)
            batch = capi.Batch(plan, np.arange(n_utt + 1, dtype=np.int64) * n_samp)
            assert batch.total_rows == n_utt * rows and int(batch.func_windows(SIZE, STEP)[-1]) == n_win

            def windows():
                capi._check(L.smilehip_batch_funcspec_windows(plan._h, batch._h, C.byref(spec), d_x.data_ptr(), COLS, 0, COLS, 0,
                                                              SIZE, STEP, d_f.data_ptr(), COLS * per, None))
        med, lo, hi = timed(windows)
        entry = {"shape": name, "windows": n_win, "windows_ms": med, "windows_min_ms": lo, "windows_max_ms": hi,
                 "windows_per_s": n_win / (med * 1e-3)}
        if baseline:
            starts = [u * rows + k * STEP for u in range(n_utt) for k in range((rows - SIZE) // STEP + 1)]
            x0, g0, fn = d_x.data_ptr(), d_g.data_ptr(), L.smilehip_funcspec_matrix
            sref, h = C.byref(spec), ctx._h

            def loop():
                for i, r in enumerate(starts):
                    rc = fn(h, sref, x0 + r * COLS * 4, COLS, SIZE, COLS, g0 + i * COLS * per * 4, None)
                    if rc:
                        capi._check(rc)
            loop()
            torch.cuda.synchronize()
            assert torch.equal(d_f.view(torch.int32), d_g.view(torch.int32)), "the windows differ from the loop over their slices"
            one = timed(loop, reps=1, warm=0)[0]
            reps = 20 if one < 2000.0 else 3
            bmed, blo, bhi = timed(loop, reps=reps, warm=1 if reps == 3 else 3)
            entry.update({"loop_ms": bmed, "loop_min_ms": blo, "loop_max_ms": bhi, "loop_median_of": reps,
                          "loop_over_windows": bmed / med, "bit_equal": True})
        res["shapes"].append(entry)
        print(json.dumps(entry))
        if batch is not None:
            batch.close()
        del d_x, d_f, d_g
    if baseline:
        assert all(e["loop_over_windows"] > 1.0 for e in res["shapes"]), "the batched call must be faster than the loop"
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
