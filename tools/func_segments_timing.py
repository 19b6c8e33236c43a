"""Timing of the functionals over listed segments: HIP events, warm, median of 20. IS09's spec on 32 columns of seeded data through
smilehip_batch_funcspec_segments on two lists -- (a) skewed: 100 000 segments over 2 000 utterances of 3 000 rows, lengths
log-uniform in 3 .. 3 000 rows, in random list order; (b) uniform: the 136 000 windows of 200 rows every 50 of 8 000 utterances of
1 000 rows as a list (the shape tools/func_windows_timing.py measures, whose windows it is compared with bit for bit) -- each against
the only route there was before: a host loop of smilehip_funcspec_matrix over the same slices, timed in the same process on a seeded
subsample of LOOP_SAMPLE segments (stated in the output) and scaled to the list. Writes the file given as the first argument
(default: profiles/func_segments_timing.json); --no-baseline leaves the loop out.

--ab-env NAME=VALUE times the call a second time with that environment variable set, in ROUNDS interleaved rounds, and checks the
rows bit for bit: for a build that reads a schedule switch at every call (how the caller-order schedule was measured against the
length-sorted one before it was removed)."""
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

COLS, LOOP_SAMPLE, ROUNDS = 32, 2000, 3


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


def skewed_list(n_utt, rows, n_seg, rng):
    """lengths log-uniform in 3 .. rows, a random utterance and a random start each, in that (random) order grouped by utterance"""
    length = np.minimum(rows, np.floor(np.exp(rng.uniform(np.log(3.0), np.log(rows + 1.0), n_seg)))).astype(np.int64)
    utt = np.sort(rng.integers(0, n_utt, n_seg))
    first = (rng.random(n_seg) * (rows - length + 1)).astype(np.int64)
    seg_off = np.searchsorted(utt, np.arange(n_utt + 1)).astype(np.int64)
    return seg_off, first, length


def uniform_list(n_utt, rows, size, step):
    per = (rows - size) // step + 1
    first = np.tile(np.arange(per, dtype=np.int64) * step, n_utt)
    return np.arange(n_utt + 1, dtype=np.int64) * per, first, np.full(n_utt * per, size, np.int64)


def main():
    args, ab = [], None
    it = iter(sys.argv[1:])
    for a in it:
        if a == "--ab-env":
            ab = next(it).split("=", 1)
        elif not a.startswith("--"):
            args.append(a)
    out_path = args[0] if args else os.path.join(ROOT, "profiles", "func_segments_timing.json")
    baseline = "--no-baseline" not in sys.argv
    L = capi.load()
    ctx = capi.Context(0)
    spec = capi.funcspec_is09()
    per = capi.funcspec_count(spec)
    res = {"device": ctx.name(), "spec": "IS09_emotion (12 values per column)", "cols": COLS,
           "method": "HIP events around one call (or one pass of the loop), 3 warm-up calls, median of 20", "lists": []}
    plan = capi.Plan(ctx, capi.is09_lld_config())
    rng = np.random.default_rng(20261020)
    shapes = (("skewed: 100000 segments of 3 .. 3000 rows (log-uniform) over 2000 utterances of 3000 rows", 2000, 3000, None),
              ("uniform: 136000 segments of 200 rows every 50 over 8000 utterances of 1000 rows", 8000, 1000, (200, 50)))
    for name, n_utt, rows, win in shapes:
        seg_off, first, length = skewed_list(n_utt, rows, 100000, rng) if win is None else uniform_list(n_utt, rows, *win)
        n_seg = len(first)
        torch.manual_seed(rows)
        d_x = torch.randn((n_utt * rows, COLS), dtype=torch.float32, device="cuda")
        d_f = torch.zeros((n_seg, COLS * per), dtype=torch.float32, device="cuda")
        # an IS09 batch whose utterances have `rows` LLD rows each (25 ms frames every 10 ms, one row more than frames)
        batch = capi.Batch(plan, np.arange(n_utt + 1, dtype=np.int64) * (400 + 160 * (rows - 2)))
        assert batch.total_rows == n_utt * rows

        def segments(out=d_f):
            capi._check(L.smilehip_batch_funcspec_segments(plan._h, batch._h, C.byref(spec), d_x.data_ptr(), COLS, 0, COLS, 0,
                                                           seg_off.ctypes.data, first.ctypes.data, length.ctypes.data, out.data_ptr(),
                                                           COLS * per, None))
        entry = {"list": name, "segments": n_seg, "rows_in_segments": int(length.sum())}
        if ab is None:
            med, lo, hi = timed(segments)
            entry.update({"segments_ms": med, "segments_min_ms": lo, "segments_max_ms": hi})
        else:
            d_h = torch.zeros_like(d_f)
            rounds = {"tree": [], "ab": []}
            for _ in range(ROUNDS):                        # interleaved: tree, switch, tree, switch, ...
                os.environ.pop(ab[0], None)
                rounds["tree"].append(timed(segments))
                os.environ[ab[0]] = ab[1]
                rounds["ab"].append(timed(lambda: segments(d_h)))
                os.environ.pop(ab[0], None)
            torch.cuda.synchronize()
            assert torch.equal(d_f.view(torch.int32), d_h.view(torch.int32)), "the two schedules' rows differ"
            for k, label in (("tree", "segments"), ("ab", "ab")):
                meds = [r[0] for r in rounds[k]]
                entry.update({f"{label}_ms": statistics.median(meds), f"{label}_round_medians_ms": meds,
                              f"{label}_min_ms": min(r[1] for r in rounds[k]), f"{label}_max_ms": max(r[2] for r in rounds[k])})
            entry.update({"ab_env": "=".join(ab), "ab_over_segments": entry["ab_ms"] / entry["segments_ms"], "ab_bit_equal": True})
            del d_h
        entry["segments_per_s"] = n_seg / (entry["segments_ms"] * 1e-3)
        if win is not None:                                # the same rows as the fixed windows
            d_w = torch.zeros_like(d_f)
            capi._check(L.smilehip_batch_funcspec_windows(plan._h, batch._h, C.byref(spec), d_x.data_ptr(), COLS, 0, COLS, 0, win[0], win[1],
                                                          d_w.data_ptr(), COLS * per, None))
            torch.cuda.synchronize()
            assert torch.equal(d_f.view(torch.int32), d_w.view(torch.int32)), "the segments differ from the windows"
            wmed, wlo, whi = timed(lambda: capi._check(L.smilehip_batch_funcspec_windows(
                plan._h, batch._h, C.byref(spec), d_x.data_ptr(), COLS, 0, COLS, 0, win[0], win[1], d_w.data_ptr(), COLS * per, None)))
            entry.update({"windows_ms": wmed, "windows_min_ms": wlo, "windows_max_ms": whi, "windows_bit_equal": True})
            del d_w
        if baseline:
            pick = np.sort(np.random.default_rng(7).choice(n_seg, LOOP_SAMPLE, replace=False))
            utt = np.searchsorted(seg_off, pick, side="right") - 1
            starts = (utt * rows + first[pick]).tolist()
            lens = length[pick].tolist()
            d_g = torch.zeros((LOOP_SAMPLE, COLS * per), dtype=torch.float32, device="cuda")
            x0, g0, fn = d_x.data_ptr(), d_g.data_ptr(), L.smilehip_funcspec_matrix
            sref, h = C.byref(spec), ctx._h

            def loop():
                for i, (r, n) in enumerate(zip(starts, lens)):
                    rc = fn(h, sref, x0 + r * COLS * 4, COLS, n, COLS, g0 + i * COLS * per * 4, None)
                    if rc:
                        capi._check(rc)
            loop()
            torch.cuda.synchronize()
            idx = torch.as_tensor(pick, device="cuda")
            assert torch.equal(d_f[idx].view(torch.int32), d_g.view(torch.int32)), "the segments differ from the loop over their slices"
            bmed, blo, bhi = timed(loop, reps=5, warm=1)
            scale = float(length.sum()) / float(length[pick].sum())
            entry.update({"loop_sample": LOOP_SAMPLE, "loop_sample_rows": int(length[pick].sum()), "loop_sample_ms": bmed,
                          "loop_sample_min_ms": blo, "loop_sample_max_ms": bhi, "loop_median_of": 5,
                          "loop_scaled_by_segments_ms": bmed * n_seg / LOOP_SAMPLE, "loop_scaled_by_rows_ms": bmed * scale,
                          "loop_over_segments": bmed * n_seg / LOOP_SAMPLE / entry["segments_ms"], "bit_equal": True})
            del d_g
        res["lists"].append(entry)
        print(json.dumps(entry), flush=True)
        batch.close()
        del d_x, d_f
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
