"""Timing of the audspec chain (SMILEHIP_CHAIN_AUDSPEC) on the flagship batch shape: 12 500 utterances of 10 s at 16 kHz, PCM resident
on the device, host clock around smilehip_lld_run + stream synchronise, warm. Writes the file given as the first argument (default:
profiles/audspec_timing.json):

  (a) the new chain: ms per step and frames/s -- median of ROUNDS rounds, each a fresh process; and its kernels (HIP events around
      every launch: the library's kernel timing): lld_audspec_frame in the wave form, the window chain
  (b) SMILEHIP_CHAIN_PLP (plp_0_d_a) with SMILEHIP_FORCE_GENERIC=1 on the same PCM, on the library given by --parent-lib (a build of
      the parent commit; without it: this tree's library, and the output says so): lld_mfcc_generic, the only reference-order kernel
      that covered the same front end before
  (c) the new chain with SMILEHIP_AUDSPEC=block: the workgroup-per-frame form of the frame kernel where the wave form runs
  (m) the headline chain (mfcc12_0_d_a, the fast kernel) on this tree's library and on the parent's: it must not have moved
      the rounds of (a), (b), (c) and (m) alternate, so all see the same box; the spread over the rounds is what differences are read against
  (d) the operators route of tests/test_gpu_audspec.py (pcm16_to_float, frame rows, pre-emphasis, window, rfft, fftmag, melspec,
      plp_audspec, delta chain) on C_UTTS utterances, scaled per frame
  (r) the roofline line: bytes moved per frame (samples read once, the static row written and read, the output row written) against
      the measured time

Every child process runs under its own `timeout -k 10`; the first one that fails ends the run, nothing is retried. The children bind
only the symbols they call, so a parent library that lacks the new preset loads."""
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

N_UTT, SECONDS, RATE, ROUNDS, STEPS, WARM, DISTINCT, C_UTTS = 12500, 10, 16000, 3, 5, 2, 25, 200
CHILD_LIMIT_S = 180
vp = C.c_void_p


def block_pcm(rate):
    from opensmile_amd import synth
    return np.concatenate([synth.utterance(2 + i, SECONDS * rate) for i in range(DISTINCT)])


def bind(lib_path, names):
    from opensmile_amd.capi import SYMBOLS
    L = C.CDLL(lib_path)
    L.smilehip_last_error.restype = C.c_char_p
    for n in names:
        f = getattr(L, n)
        f.restype, f.argtypes = SYMBOLS[n]
    return L


def checker(L):
    def ck(rc):
        if rc != 0:
            raise RuntimeError(L.smilehip_last_error().decode())
    return ck


def config_for(L, kind, rate):
    """kind "audspec": the new preset; "plp": plp_0_d_a; "mfcc": mfcc12_0_d_a (what the parent's library runs as well)"""
    from opensmile_amd.capi import SYMBOLS, LldConfig
    name = {"audspec": "smilehip_config_audspec", "plp": "smilehip_config_plp_0_d_a", "mfcc": "smilehip_config_mfcc12_0_d_a"}[kind]
    cfg = LldConfig()
    f = getattr(L, name)
    f.restype, f.argtypes = SYMBOLS[name]
    f(C.byref(cfg))
    cfg.sample_rate = float(rate)
    return cfg


def kernel_report(L):
    n = 1 << 16
    while True:
        buf = C.create_string_buffer(n)
        got = L.smilehip_kernel_timing_report(buf, n)
        if got >= 0:
            break
        n = -got + 1
    out = {}
    for line in buf.value.decode().splitlines():
        name, launches, ms = line.split("\t")
        name = name.split("<")[0].strip().strip("(")
        a = out.get(name, [0, 0.0])
        out[name] = [a[0] + int(launches), a[1] + float(ms)]
    return out


def child_chain(lib_path, kind, n_utt, rate):
    """one process: plan + batch of n_utt utterances, WARM + STEPS timed runs, then 3 runs with HIP events around every launch"""
    from opensmile_amd.capi import Geometry
    L = bind(lib_path, ["smilehip_init", "smilehip_plan_create", "smilehip_batch_create", "smilehip_alloc", "smilehip_copy_to_device",
                        "smilehip_lld_run", "smilehip_stream_synchronize", "smilehip_plan_geometry", "smilehip_batch_total_frames",
                        "smilehip_batch_total_rows", "smilehip_kernel_timing", "smilehip_kernel_timing_report"])
    ck = checker(L)
    cfg = config_for(L, kind, rate)
    ctx, plan, batch, d_pcm, d_out = vp(), vp(), vp(), vp(), vp()
    ck(L.smilehip_init(0, C.byref(ctx)))
    ck(L.smilehip_plan_create(ctx, C.byref(cfg), C.byref(plan)))
    g = Geometry()
    ck(L.smilehip_plan_geometry(plan, C.byref(g)))
    n = SECONDS * rate
    off = np.arange(n_utt + 1, dtype=np.int64) * n
    ck(L.smilehip_batch_create(plan, off.ctypes.data, n_utt, C.byref(batch)))
    frames, rows = L.smilehip_batch_total_frames(batch), L.smilehip_batch_total_rows(batch)
    blk = block_pcm(rate)
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
    ck(L.smilehip_kernel_timing(1))
    for _ in range(3):
        ck(L.smilehip_lld_run(plan, batch, d_pcm, d_out, g.n_out, None))
    ck(L.smilehip_stream_synchronize(ctx, None))
    kern = {k: [v[0], v[1] / 3.0] for k, v in kernel_report(L).items()}
    ck(L.smilehip_kernel_timing(0))
    print(json.dumps({"ms": ms, "frames": frames, "rows": rows, "fft_size": g.fft_size, "kernels": kern}))


def child_components(lib_path):
    """the operators route on C_UTTS utterances: every operator of the chain as its own launch over all frames"""
    import torch
    L = bind(lib_path, ["smilehip_init", "smilehip_plan_create", "smilehip_batch_create", "smilehip_stream_synchronize", "smilehip_pcm16_to_float",
                        "smilehip_frame_rows", "smilehip_preemphasis_frames", "smilehip_window_frames", "smilehip_rfft_frames", "smilehip_fftmag_frames",
                        "smilehip_melspec_frames", "smilehip_plp_audspec_frames", "smilehip_delta_chain"])
    ck = checker(L)
    ctx, plan, batch = vp(), vp(), vp()
    ck(L.smilehip_init(0, C.byref(ctx)))
    cfg = config_for(L, "audspec", RATE)
    ck(L.smilehip_plan_create(ctx, C.byref(cfg), C.byref(plan)))
    n, N, H, K, Nfft, NB = SECONDS * RATE, 400, 160, 257, 512, 26
    T = (n - N) // H + 1
    nF = C_UTTS * T
    off = np.arange(C_UTTS + 1, dtype=np.int64) * n
    ck(L.smilehip_batch_create(plan, off.ctypes.data, C_UTTS, C.byref(batch)))
    dev = "cuda"
    pcm = torch.from_numpy(block_pcm(RATE)).to(dev).repeat(C_UTTS // DISTINCT)
    x = torch.zeros(C_UTTS * n, device=dev)
    fr, pe, w = torch.zeros((nF, N), device=dev), torch.zeros((nF, N), device=dev), torch.zeros((nF, N), device=dev)
    c, m = torch.zeros((nF, Nfft), device=dev), torch.zeros((nF, K), device=dev)
    mel, io = torch.zeros((nF, NB), device=dev), torch.zeros((nF, 3 * NB), device=dev)
    eql = torch.ones(NB, device=dev)                        # (the weights' values do not change the time)

    def step():
        ck(L.smilehip_pcm16_to_float(ctx, pcm.data_ptr(), C_UTTS * n, x.data_ptr(), None))
        for u in range(C_UTTS):
            ck(L.smilehip_frame_rows(ctx, x.data_ptr() + 4 * u * n, N, H, T, fr.data_ptr() + 4 * u * T * N, N, None))
        ck(L.smilehip_preemphasis_frames(ctx, fr.data_ptr(), N, pe.data_ptr(), N, nF, N, 0.97, 0, None))
        ck(L.smilehip_window_frames(plan, pe.data_ptr(), N, w.data_ptr(), N, nF, None))
        ck(L.smilehip_rfft_frames(plan, w.data_ptr(), N, c.data_ptr(), Nfft, nF, None))
        ck(L.smilehip_fftmag_frames(plan, c.data_ptr(), Nfft, m.data_ptr(), K, nF, None))
        ck(L.smilehip_melspec_frames(plan, m.data_ptr(), K, mel.data_ptr(), NB, nF, None))
        ck(L.smilehip_plp_audspec_frames(ctx, mel.data_ptr(), NB, NB, eql.data_ptr(), 1.0, 0.33, 0, None, None, io.data_ptr(), 3 * NB, nF, None))
        ck(L.smilehip_delta_chain(plan, batch, io.data_ptr(), 3 * NB, NB, 2, 2, None))
        torch.cuda.synchronize()
    ms = []
    for i in range(WARM + STEPS):
        t0 = time.perf_counter()
        step()
        if i >= WARM:
            ms.append((time.perf_counter() - t0) * 1e3)
    print(json.dumps({"ms": ms, "frames": nF}))


def spawn(*args, env=None):
    """a child process under its own time limit; a failure ends the whole run (no retry)"""
    cmd = ["timeout", "-k", "10", str(CHILD_LIMIT_S), sys.executable, os.path.abspath(__file__), *args]
    p = subprocess.run(cmd, capture_output=True, text=True, env=dict(os.environ, **(env or {})))
    if p.returncode != 0:
        raise SystemExit("child %r failed (%d), stopping: %s" % (args, p.returncode, p.stderr[-2000:]))
    return json.loads(p.stdout.strip().splitlines()[-1])


def summary(rounds):
    ms = [statistics.median(x["ms"]) for x in rounds]
    med = statistics.median(ms)
    return {"ms_per_step_median": med, "ms_rounds": ms, "spread_ms": max(ms) - min(ms), "frames": rounds[0]["frames"], "rows": rounds[0]["rows"],
            "frames_per_s": rounds[0]["frames"] / (med * 1e-3), "fft_size": rounds[0]["fft_size"],
            "kernels_ms_per_step": {k: statistics.median(r["kernels"].get(k, [0, 0.0])[1] for r in rounds) for k in sorted(rounds[0]["kernels"])}}


def main():
    if sys.argv[1:2] == ["--child-chain"]:
        return child_chain(sys.argv[2], sys.argv[3], int(sys.argv[4]), int(sys.argv[5]))
    if sys.argv[1:2] == ["--child-components"]:
        return child_components(sys.argv[2])
    args, parent_lib = [], None
    it = iter(sys.argv[1:])
    for a in it:
        if a == "--parent-lib":
            parent_lib = os.path.abspath(next(it))
        else:
            args.append(a)
    out_path = args[0] if args else os.path.join(ROOT, "profiles", "audspec_timing.json")
    tree_lib = os.path.join(ROOT, "opensmile_amd", "libsmilehip.so")
    a_rounds, b_rounds, c_rounds, mt_rounds, mp_rounds = [], [], [], [], []
    for r in range(ROUNDS):                                # alternating: (a), (b), (c), (m) tree, (m) parent, (a), ...
        a_rounds.append(spawn("--child-chain", tree_lib, "audspec", str(N_UTT), str(RATE)))
        b_rounds.append(spawn("--child-chain", parent_lib or tree_lib, "plp", str(N_UTT), str(RATE), env={"SMILEHIP_FORCE_GENERIC": "1"}))
        c_rounds.append(spawn("--child-chain", tree_lib, "audspec", str(N_UTT), str(RATE), env={"SMILEHIP_AUDSPEC": "block"}))
        mt_rounds.append(spawn("--child-chain", tree_lib, "mfcc", str(N_UTT), str(RATE)))
        mp_rounds.append(spawn("--child-chain", parent_lib or tree_lib, "mfcc", str(N_UTT), str(RATE)))
        print("round", r, "a", statistics.median(a_rounds[-1]["ms"]), "b", statistics.median(b_rounds[-1]["ms"]), "c",
              statistics.median(c_rounds[-1]["ms"]), "m tree", statistics.median(mt_rounds[-1]["ms"]), "m parent",
              statistics.median(mp_rounds[-1]["ms"]), flush=True)
    comp = spawn("--child-components", tree_lib)
    a, b, c, mt, mp = summary(a_rounds), summary(b_rounds), summary(c_rounds), summary(mt_rounds), summary(mp_rounds)
    which = "parent commit's build" if parent_lib else "THIS tree's build (no --parent-lib given)"
    b["library"] = mp["library"] = which
    ka, kb, kc = a["kernels_ms_per_step"], b["kernels_ms_per_step"], c["kernels_ms_per_step"]
    frame_a = sum(v for k, v in ka.items() if "lld_audspec_frame" in k)
    frame_b = sum(v for k, v in kb.items() if "lld_mfcc_generic" in k)
    frame_c = sum(v for k, v in kc.items() if "lld_audspec_frame" in k)
    comp_med = statistics.median(comp["ms"])
    # bytes per frame: H int16 samples read once (the frames overlap: the rest comes from cache), the static row written by the frame
    # kernel and read by the window chain, the output row written
    H, NB = 160, 26
    bytes_per_frame = 2 * H + 2 * 4 * NB + 4 * 3 * NB
    res = {
        "workload": "%d x %d s at %d Hz, int16 PCM resident; host clock around smilehip_lld_run + synchronise; %d warm + %d timed steps "
                    "per process, %d alternating rounds of fresh processes; kernels: HIP events around every launch, 3 further steps"
                    % (N_UTT, SECONDS, RATE, WARM, STEPS, ROUNDS),
        "a_audspec": a,
        "b_plp_0_d_a_force_generic": b,
        "c_audspec_workgroup_form": c,
        "m_headline_mfcc_chain": {"this_tree": mt, "parent": mp},
        "frame_kernel_ms": {"a_wave_form": frame_a, "b_lld_mfcc_generic": frame_b, "c_workgroup_form": frame_c},
        "frame_kernel_ns_per_frame": {"a_wave_form": 1e6 * frame_a / a["frames"], "b_lld_mfcc_generic": 1e6 * frame_b / b["frames"],
                                      "c_workgroup_form": 1e6 * frame_c / c["frames"]},
        "a_minus_c_ms": a["ms_per_step_median"] - c["ms_per_step_median"],
        "d_operators_route": {"library": "this tree's build", "utterances": C_UTTS, "frames": comp["frames"], "ms_per_step_median": comp_med,
                              "ms": comp["ms"], "frames_per_s": comp["frames"] / (comp_med * 1e-3),
                              "factor_against_a_per_frame": (comp_med / comp["frames"]) / (a["ms_per_step_median"] / a["frames"])},
        "r_roofline": {"bytes_per_frame": bytes_per_frame, "gbytes_per_step": bytes_per_frame * a["frames"] * 1e-9,
                       "gbytes_per_s_at_the_measured_step": bytes_per_frame * a["frames"] * 1e-9 / (a["ms_per_step_median"] * 1e-3),
                       "note": "against 8 TB/s of HBM3E peak: the step's share of the memory roofline is this figure / 8000"},
    }
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
