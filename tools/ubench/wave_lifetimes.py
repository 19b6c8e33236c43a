#!/usr/bin/env python3
"""Per-wave lifetimes of the fused MFCC kernel (instrumented build: tools/ubench/variant.sh lifetimes -DSMILEHIP_PHASE_TIMING=2;
opensmile_amd/csrc/wave_lifetimes.hpp).

usage (GPU): tools/ubench/wave_lifetimes.py [--per-simd] [out.json]      SMILEHIP_LIB=<library> overrides tools/ubench/build/libsmilehip_lifetimes.so

Runs the bench instance (MFCC12_0_D_A, 1000 x 10 s) warm, records ONE launch and prints / stores
  - the distribution of lifetime / longest lifetime,
  - per SIMD (XCC, SE, SH, CU, SIMD decoded from HW_ID and XCC_ID) the finish order against the start order,
  - the time-integral of resident waves per SIMD (what rocprofv3's SQ_WAVE_CYCLES x 4 / 1024 / GRBM_GUI_ACTIVE gives: waves_per_simd
    of tools/pmc_counters_json.py; the record covers the pass loop only, not a wave's table copy in front of it),
  - which waves (block, wave number, hardware wave slot) share a SIMD.
s_memtime counters of different CUs need not share a zero: lifetimes (end - begin) are compared across the chip, absolute times only
within a CU. `analyse` and the decoders need no GPU (tests/test_wave_lifetimes_tool.py)."""
import collections
import json
import os
import sys

import numpy as np

WORDS = 6            # begin | end | HW_ID + (XCC_ID << 32) | block + (wave << 32) | passes | written   (wave_lifetimes.hpp)
N_SIMDS = 1024       # 256 CUs x 4: the divisor of the counters' waves_per_simd


def decode_hw_id(hw):
    """Fields of HW_REG_HW_ID (gfx9 layout): the wave slot on its SIMD, the SIMD, and the CU's place in its XCC."""
    hw = int(hw)
    return {"wave_id": hw & 0xf, "simd": (hw >> 4) & 3, "pipe": (hw >> 6) & 3, "cu": (hw >> 8) & 0xf, "sh": (hw >> 12) & 1,
            "se": (hw >> 13) & 7, "tg": (hw >> 16) & 0xf, "vm": (hw >> 20) & 0xf, "queue": (hw >> 24) & 7, "state": (hw >> 27) & 7,
            "me": (hw >> 30) & 3}


def decode_xcc_id(x):
    return int(x) & 0xf


def decode_records(raw):
    """raw: uint64 [n, WORDS] -> list of dicts of the records that were written."""
    raw = np.asarray(raw, dtype=np.uint64).reshape(-1, WORDS)
    out = []
    for r in raw:
        if int(r[5]) != 1:
            continue
        f = decode_hw_id(int(r[2]) & 0xffffffff)
        xcc = decode_xcc_id(int(r[2]) >> 32)
        out.append({"t0": int(r[0]), "t1": int(r[1]), "xcc": xcc, "se": f["se"], "sh": f["sh"], "cu": f["cu"], "simd": f["simd"],
                    "wave_id": f["wave_id"], "block": int(r[3]) & 0xffffffff, "wave": int(r[3]) >> 32, "passes": int(r[4])})
    return out


def _ranks(values):
    order = sorted(range(len(values)), key=lambda i: (values[i], i))
    rk = [0] * len(values)
    for pos, i in enumerate(order):
        rk[i] = pos
    return rk


def analyse(recs, n_simds=N_SIMDS):
    """recs: decode_records' list. Returns a dict of plain numbers and lists (JSON-ready)."""
    if not recs:
        raise ValueError("no wave record was written")
    life = np.array([r["t1"] - r["t0"] for r in recs], dtype=np.float64)
    longest = float(life.max())
    ratio = life / longest
    hist, _ = np.histogram(ratio, bins=np.linspace(0.0, 1.0, 11))
    simds = collections.defaultdict(list)
    for i, r in enumerate(recs):
        simds[(r["xcc"], r["se"], r["sh"], r["cu"], r["simd"])].append(i)
    cus = collections.defaultdict(list)
    for i, r in enumerate(recs):
        cus[(r["xcc"], r["se"], r["sh"], r["cu"])].append(i)
    # the launch on one CU: first entry to last exit of its waves (one clock); the launch: the longest of them
    cu_span = {k: max(recs[i]["t1"] for i in v) - min(recs[i]["t0"] for i in v) for k, v in cus.items()}
    span = float(max(cu_span.values()))
    per_simd, same_order, rho_sum, rho_n = [], 0, 0.0, 0
    by_start_rank = collections.defaultdict(list)
    spread = []
    shares_wave, shares_slot, n_blocks, slot_distinct = collections.Counter(), collections.Counter(), collections.Counter(), 0
    for key in sorted(simds):
        idx = simds[key]
        s_rk = _ranks([recs[i]["t0"] for i in idx])
        f_rk = _ranks([recs[i]["t1"] for i in idx])
        n = len(idx)
        same_order += int(s_rk == f_rk)
        if n > 1:
            d2 = sum((a - b) ** 2 for a, b in zip(s_rk, f_rk))
            rho_sum += 1.0 - 6.0 * d2 / (n * (n * n - 1))
            rho_n += 1
        lr = [float(ratio[i]) for i in idx]
        spread.append(max(lr) - min(lr))
        for i, rk in zip(idx, s_rk):
            by_start_rank[rk].append(float(ratio[i]))
        t_first = min(recs[i]["t0"] for i in idx)
        resident = float(sum(life[i] for i in idx))
        shares_wave[tuple(sorted(recs[i]["wave"] for i in idx))] += 1
        shares_slot[tuple(sorted(recs[i]["wave_id"] for i in idx))] += 1
        n_blocks[len({recs[i]["block"] for i in idx})] += 1
        slot_distinct += int(len({recs[i]["wave_id"] & 3 for i in idx}) == n)
        per_simd.append({"xcc": key[0], "se": key[1], "sh": key[2], "cu": key[3], "simd": key[4],
                         "resident_over_launch": resident / span,
                         # block, wave, hardware wave slot, begin and end relative to the SIMD's first entry, passes
                         "waves": [[recs[i]["block"], recs[i]["wave"], recs[i]["wave_id"], recs[i]["t0"] - t_first, recs[i]["t1"] - t_first,
                                    recs[i]["passes"]] for i in sorted(idx, key=lambda i: recs[i]["t0"])]})
    q = [0, 5, 25, 50, 75, 95, 100]
    return {
        "n_waves": len(recs), "n_simds_used": len(simds), "n_cus_used": len(cus), "n_simds": n_simds,
        "longest_lifetime_ticks": longest, "launch_span_ticks": span,
        "cu_span_over_launch": {"min": min(cu_span.values()) / span, "mean": float(np.mean(list(cu_span.values()))) / span},
        "lifetime_over_longest": {"mean": float(ratio.mean()), "percentiles": {str(p): float(np.percentile(ratio, p)) for p in q},
                                  "histogram_tenths": [int(h) for h in hist]},
        "lifetime_over_launch_mean": float(life.mean()) / span,
        # the counters' figure: wave-ticks of the whole chip over (SIMDs x launch)
        "resident_waves_per_simd": float(life.sum()) / (n_simds * span),
        "resident_waves_per_used_simd": float(life.sum()) / (len(simds) * span),
        "finish_order": {"simds_finishing_in_start_order": same_order, "of": len(simds),
                         "mean_rank_correlation": rho_sum / rho_n if rho_n else None,
                         "mean_lifetime_over_longest_by_start_rank": {str(k): float(np.mean(v)) for k, v in sorted(by_start_rank.items())},
                         "lifetime_spread_within_simd": {"mean": float(np.mean(spread)), "max": float(np.max(spread))}},
        "sharing": {"wave_numbers_on_a_simd": {str(list(k)): v for k, v in shares_wave.most_common(8)},
                    "hw_wave_slots_on_a_simd": {str(list(k)): v for k, v in shares_slot.most_common(8)},
                    "blocks_on_a_simd": {str(k): v for k, v in sorted(n_blocks.items())},
                    "simds_with_distinct_slot_mod_4": slot_distinct},
        "passes": {"min": min(r["passes"] for r in recs), "max": max(r["passes"] for r in recs)},
        "per_simd": per_simd,
    }


def report(a):
    lo = a["lifetime_over_longest"]
    fo = a["finish_order"]
    lines = [
        f"waves {a['n_waves']} on {a['n_simds_used']} SIMDs of {a['n_cus_used']} CUs; passes per wave {a['passes']['min']} .. {a['passes']['max']}",
        f"launch (longest CU, first entry to last exit) {a['launch_span_ticks']:.0f} ticks; shortest CU {a['cu_span_over_launch']['min']:.3f}, "
        f"mean CU {a['cu_span_over_launch']['mean']:.3f} of it",
        f"lifetime / longest: mean {lo['mean']:.3f}; percentiles " + "  ".join(f"p{k} {v:.3f}" for k, v in lo["percentiles"].items()),
        "  tenths 0.0 .. 1.0: " + " ".join(str(h) for h in lo["histogram_tenths"]),
        f"lifetime / launch: mean {a['lifetime_over_launch_mean']:.3f}",
        f"resident waves per SIMD (time integral): {a['resident_waves_per_simd']:.3f} over {a['n_simds']} SIMDs, "
        f"{a['resident_waves_per_used_simd']:.3f} over the SIMDs used",
        f"finish order = start order on {fo['simds_finishing_in_start_order']} of {fo['of']} SIMDs; mean rank correlation "
        f"{fo['mean_rank_correlation']:.3f}" if fo["mean_rank_correlation"] is not None else "finish order: one wave per SIMD",
        "  mean lifetime / longest by start rank on the SIMD: " + "  ".join(f"{k}: {v:.3f}" for k, v in fo["mean_lifetime_over_longest_by_start_rank"].items()),
        f"  spread of lifetime / longest within a SIMD: mean {fo['lifetime_spread_within_simd']['mean']:.3f}, max {fo['lifetime_spread_within_simd']['max']:.3f}",
        f"wave numbers sharing a SIMD: {a['sharing']['wave_numbers_on_a_simd']}",
        f"hardware wave slots on a SIMD: {a['sharing']['hw_wave_slots_on_a_simd']}",
        f"blocks on a SIMD: {a['sharing']['blocks_on_a_simd']}; SIMDs whose waves differ in slot & 3: {a['sharing']['simds_with_distinct_slot_mod_4']}",
    ]
    return "\n".join(lines)


def record_bench_instance():
    """One warm launch of the bench instance with the instrumented library; returns the raw records."""
    import ctypes as C
    root = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    sys.path.insert(0, root)
    os.environ.setdefault("SMILEHIP_LIB", os.path.join(root, "tools", "ubench", "build", "libsmilehip_lifetimes.so"))
    import torch
    from opensmile_amd import capi, synth
    ctx = capi.Context(0)
    plan = capi.Plan(ctx)
    pcm, off = synth.corpus_tiled(1000, 160000, n_unique=32)
    b = capi.Batch(plan, off)
    d_pcm = torch.from_numpy(pcm).cuda()
    d_out = torch.empty((b.total_frames, 39), dtype=torch.float32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    dbg = capi.load().smilehip_debug_wave_life
    dbg.restype = C.c_int
    dbg.argtypes = [C.POINTER(C.c_uint64), C.c_int, C.c_int]
    for _ in range(100):                       # warm: clocks and caches as in the bench's timed region
        b.run_device(d_pcm.data_ptr(), d_out.data_ptr(), 39, st)
    torch.cuda.synchronize()
    n_slots = dbg(None, 0, 1)
    if n_slots <= 0:
        raise SystemExit("smilehip_debug_wave_life failed")
    b.run_device(d_pcm.data_ptr(), d_out.data_ptr(), 39, st)
    torch.cuda.synchronize()
    buf = (C.c_uint64 * (n_slots * WORDS))()
    if dbg(buf, n_slots, 0) <= 0:
        raise SystemExit("smilehip_debug_wave_life failed")
    return np.frombuffer(buf, dtype=np.uint64).reshape(n_slots, WORDS).copy(), os.environ["SMILEHIP_LIB"]


def main():
    raw, lib = record_bench_instance()
    a = analyse(decode_records(raw))
    a["library"] = os.path.basename(lib)
    print(report(a))
    args = [x for x in sys.argv[1:] if x != "--per-simd"]
    if args:
        if "--per-simd" not in sys.argv:          # the table of every SIMD's waves (190 KB) only on request
            a.pop("per_simd")
        with open(args[0], "w") as f:
            json.dump(a, f, indent=1)
            f.write("\n")
        print(args[0], os.path.getsize(args[0]), "bytes")


if __name__ == "__main__":
    main()
