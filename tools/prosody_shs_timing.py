"""Timing of the prosodyShs chain (SMILEHIP_CHAIN_PROSODY_SHS) on the flagship batch shape: 12 500 utterances of 10 s at 16 kHz,
PCM resident on the device, host clock around smilehip_lld_run + stream synchronise, warm. Writes the file given as the first
argument (default: profiles/prosody_shs_timing.json):

  (a) the new chain: ms per step and frames/s -- median of ROUNDS rounds, each a fresh process
  (b) SMILEHIP_CHAIN_COMPARE_F0 on the same PCM (the same front end on 60 ms frames + the Viterbi pass), on the library given by
      --parent-lib (a build of the parent commit; without it: this tree's library, and the output says so) -- the rounds of (a)
      and (b) alternate, so both see the same box; (b)'s own spread over the rounds is what (a) - (b) is read against
  (c) the per-component route of tests/test_gpu_prosody_shs.py (frame rows, window, rfft, fftmag, specscale, pitchshs,
      pitch_smoother_rows, intensity; the moving average on the host is NOT timed) on C_UTTS utterances, scaled per frame
  and the tail kernel's own time and share of the step, from the library's kernel timing (every launch between HIP events).

The children bind only the symbols they call, so a parent library that lacks the new preset loads."""
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_UTT, SECONDS, RATE, ROUNDS, STEPS, WARM, DISTINCT, C_UTTS = 12500, 10, 16000, 5, 5, 2, 25, 200
CHAIN_F0, CHAIN_PROSODY = 4, 7


def block_pcm():
    from opensmile_amd import synth
    return np.concatenate([synth.utterance(2 + i, SECONDS * RATE) for i in range(DISTINCT)])


def child_chain(lib_path, chain, n_utt):
    """one process: plan + batch of n_utt utterances, WARM + STEPS runs; prints {"ms": [...], "frames": n, "rows": n}"""
    from opensmile_amd.capi import LldConfig, Geometry
    L = C.CDLL(lib_path)
    vp = C.c_void_p
    L.smilehip_last_error.restype = C.c_char_p

    def ck(rc):
        if rc != 0:
            raise RuntimeError(L.smilehip_last_error().decode())
    for name, args in (("smilehip_init", [C.c_int, C.POINTER(vp)]), ("smilehip_plan_create", [vp, C.POINTER(LldConfig), C.POINTER(vp)]),
                       ("smilehip_batch_create", [vp, vp, C.c_int32, C.POINTER(vp)]), ("smilehip_alloc", [vp, C.c_uint64, C.POINTER(vp)]),
                       ("smilehip_copy_to_device", [vp, vp, vp, C.c_uint64, vp]), ("smilehip_lld_run", [vp, vp, vp, vp, C.c_int64, vp]),
                       ("smilehip_stream_synchronize", [vp, vp]), ("smilehip_plan_geometry", [vp, C.POINTER(Geometry)])):
        getattr(L, name).argtypes = args
    for name in ("smilehip_batch_total_frames", "smilehip_batch_total_rows"):
        getattr(L, name).restype, getattr(L, name).argtypes = C.c_int64, [vp]
    cfg = LldConfig()
    if chain == CHAIN_PROSODY:
        L.smilehip_config_prosody_shs(C.byref(cfg))
    else:
        L.smilehip_config_compare16_f0(C.byref(cfg))
    ctx, plan, batch, d_pcm, d_out = vp(), vp(), vp(), vp(), vp()
    ck(L.smilehip_init(0, C.byref(ctx)))
    ck(L.smilehip_plan_create(ctx, C.byref(cfg), C.byref(plan)))
    g = Geometry()
    ck(L.smilehip_plan_geometry(plan, C.byref(g)))
    n = SECONDS * RATE
    off = np.arange(n_utt + 1, dtype=np.int64) * n
    ck(L.smilehip_batch_create(plan, off.ctypes.data, n_utt, C.byref(batch)))
    frames, rows = L.smilehip_batch_total_frames(batch), L.smilehip_batch_total_rows(batch)
    blk = block_pcm()
    ck(L.smilehip_alloc(ctx, int(off[-1]) * 2, C.byref(d_pcm)))
    ck(L.smilehip_alloc(ctx, max(rows, 1) * g.n_out * 4, C.byref(d_out)))
    for u0 in range(0, n_utt, DISTINCT):
        k = min(DISTINCT, n_utt - u0)
        ck(L.smilehip_copy_to_device(ctx, d_pcm.value + u0 * n * 2, blk.ctypes.data, k * n * 2, None))
    ck(L.smilehip_stream_synchronize(ctx, None))
    ms = []
    for i in range(WARM + STEPS):
        t0 = time.perf_counter()
        ck(L.smilehip_lld_run(plan, batch, d_pcm, d_out, g.n_out, None))
        ck(L.smilehip_stream_synchronize(ctx, None))
        if i >= WARM:
            ms.append((time.perf_counter() - t0) * 1e3)
    print(json.dumps({"ms": ms, "frames": frames, "rows": rows}))


def child_kernels():
    """this tree's library: the chain's kernels one by one (HIP events around every launch), 3 steps"""
    import torch  # noqa: F401  (first: one HIP runtime in the process)
    from opensmile_amd import capi
    ctx = capi.Context(0)
    plan = capi.Plan(ctx, capi.prosody_shs_config())
    n = SECONDS * RATE
    b = capi.Batch(plan, np.arange(N_UTT + 1, dtype=np.int64) * n)
    d_pcm = torch.from_numpy(block_pcm()).cuda().repeat(N_UTT // DISTINCT)
    d_out = torch.zeros((b.total_rows, 3), device="cuda")
    b.run_device(d_pcm.data_ptr(), d_out.data_ptr(), 3)
    torch.cuda.synchronize()
    capi.kernel_timing(True)
    for _ in range(3):
        b.run_device(d_pcm.data_ptr(), d_out.data_ptr(), 3)
    torch.cuda.synchronize()
    rep = capi.kernel_timing_report()
    capi.kernel_timing(False)
    print(json.dumps({k: [v[0], v[1] / 3.0] for k, v in rep.items()}))


def child_components():
    """the per-component route on C_UTTS utterances: every operator of the chain as its own launch over all frames"""
    import torch
    from opensmile_amd import capi
    L = capi.load()
    ctx = capi.Context(0)
    plan = capi.Plan(ctx, capi.prosody_shs_config())
    n, N, H, K = SECONDS * RATE, 800, 160, 513
    T = (n - N) // H + 1
    nF = C_UTTS * T
    pcm = torch.from_numpy(block_pcm()).cuda().repeat(C_UTTS // DISTINCT)
    x = torch.zeros(C_UTTS * n, device="cuda")
    fr, w, c = torch.zeros((nF, N), device="cuda"), torch.zeros((nF, N), device="cuda"), torch.zeros((nF, 1024), device="cuda")
    m, h, s = torch.zeros((nF, K), device="cuda"), torch.zeros((nF, K), device="cuda"), torch.zeros((nF, 21), device="cuda")
    c18, p, l = torch.zeros((nF, 18), device="cuda"), torch.zeros((nF, 2), device="cuda"), torch.zeros((nF, 1), device="cuda")
    roff = (torch.arange(C_UTTS + 1, dtype=torch.int64) * T).cuda()
    wr = torch.zeros(C_UTTS, dtype=torch.int64, device="cuda")

    def step():
        capi.pcm16_to_float(ctx, pcm.data_ptr(), C_UTTS * n, x.data_ptr())
        for u in range(C_UTTS):
            capi._check(L.smilehip_frame_rows(ctx._h, x.data_ptr() + 4 * u * n, N, H, T, fr.data_ptr() + 4 * u * T * N, N, None))
        capi.window_frames(plan, fr.data_ptr(), N, w.data_ptr(), N, nF)
        capi.rfft_frames(plan, w.data_ptr(), N, c.data_ptr(), 1024, nF)
        capi.fftmag_frames(plan, c.data_ptr(), 1024, m.data_ptr(), K, nF)
        capi._check(L.smilehip_specscale_frames(plan._h, m.data_ptr(), K, h.data_ptr(), K, nF, None))
        capi._check(L.smilehip_pitchshs_frames(plan._h, h.data_ptr(), K, s.data_ptr(), 21, nF, None))
        c18.copy_(s[:, 1:19])
        capi._check(L.smilehip_pitch_smoother_rows(ctx._h, 6, 0.7, 0, 1, 9, c18.data_ptr(), 18, roff.data_ptr(), C_UTTS, 0, None, 0, p.data_ptr(), 2,
                                                   wr.data_ptr(), None))
        capi._check(L.smilehip_intensity_frames(ctx._h, fr.data_ptr(), N, N, 2, l.data_ptr(), 1, nF, None))
        torch.cuda.synchronize()
    ms = []
    for i in range(WARM + STEPS):
        t0 = time.perf_counter()
        step()
        if i >= WARM:
            ms.append((time.perf_counter() - t0) * 1e3)
    print(json.dumps({"ms": ms, "frames": nF}))


def spawn(*args):
    p = subprocess.run([sys.executable, os.path.abspath(__file__), *args], capture_output=True, text=True, timeout=900)
    if p.returncode != 0:
        raise SystemExit("child %r failed (%d): %s" % (args, p.returncode, p.stderr[-2000:]))
    return json.loads(p.stdout.strip().splitlines()[-1])


def main():
    if sys.argv[1:2] == ["--child-chain"]:
        return child_chain(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]))
    if sys.argv[1:2] == ["--child-kernels"]:
        return child_kernels()
    if sys.argv[1:2] == ["--child-components"]:
        return child_components()
    args, parent_lib = [], None
    it = iter(sys.argv[1:])
    for a in it:
        if a == "--parent-lib":
            parent_lib = os.path.abspath(next(it))
        else:
            args.append(a)
    out_path = args[0] if args else os.path.join(ROOT, "profiles", "prosody_shs_timing.json")
    tree_lib = os.path.join(ROOT, "opensmile_amd", "libsmilehip.so")
    a_rounds, b_rounds = [], []
    for r in range(ROUNDS):                                # alternating: (a), (b), (a), (b), ...
        a_rounds.append(spawn("--child-chain", tree_lib, str(CHAIN_PROSODY), str(N_UTT)))
        b_rounds.append(spawn("--child-chain", parent_lib or tree_lib, str(CHAIN_F0), str(N_UTT)))
        print("round", r, "a", statistics.median(a_rounds[-1]["ms"]), "b", statistics.median(b_rounds[-1]["ms"]), flush=True)
    a_ms = [statistics.median(x["ms"]) for x in a_rounds]
    b_ms = [statistics.median(x["ms"]) for x in b_rounds]
    kern = spawn("--child-kernels")
    comp = spawn("--child-components")
    a_med, b_med = statistics.median(a_ms), statistics.median(b_ms)
    step_kernels = sum(v[1] for v in kern.values())
    tail = kern.get("lld_prosody_tail", kern.get("smilehip::lld_prosody_tail", [0, 0.0]))
    c_med = statistics.median(comp["ms"])
    res = {
        "workload": "%d x %d s at %d Hz, int16 PCM resident; host clock around smilehip_lld_run + synchronise; %d warm + %d timed steps "
                    "per process, %d alternating rounds of fresh processes" % (N_UTT, SECONDS, RATE, WARM, STEPS, ROUNDS),
        "a_prosody_shs": {"ms_per_step_median": a_med, "ms_rounds": a_ms, "frames": a_rounds[0]["frames"], "rows": a_rounds[0]["rows"],
                          "frames_per_s": a_rounds[0]["frames"] / (a_med * 1e-3)},
        "b_compare_f0": {"library": "parent commit's build" if parent_lib else "THIS tree's build (no --parent-lib given)",
                         "ms_per_step_median": b_med, "ms_rounds": b_ms, "spread_ms": max(b_ms) - min(b_ms), "frames": b_rounds[0]["frames"],
                         "frames_per_s": b_rounds[0]["frames"] / (b_med * 1e-3)},
        "a_minus_b_ms": a_med - b_med,
        "c_per_component": {"utterances": C_UTTS, "frames": comp["frames"], "ms_per_step_median": c_med, "ms": comp["ms"],
                            "frames_per_s": comp["frames"] / (c_med * 1e-3), "note": "the moving average (host) is not timed"},
        "kernels_ms_per_step": {k: v[1] for k, v in sorted(kern.items())},
        "tail_kernel": {"ms_per_step": tail[1], "share_of_kernel_time": tail[1] / step_kernels if step_kernels else None},
    }
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
