"""Timing of the chroma_fft chain (SMILEHIP_CHAIN_CHROMA_FFT) on the flagship batch shape: 12 500 utterances of 10 s at 16 kHz, PCM
resident on the device, host clock around smilehip_lld_run + stream synchronise, warm. Writes the file given as the first argument
(default: profiles/chroma_fft_timing.json):

  (a) the new chain: ms per step and frames/s -- median of ROUNDS rounds, each a fresh process; and its one kernel (HIP events around
      the launch: the library's kernel timing)
  (b) SMILEHIP_CHAIN_PROSODY_ACF on the same PCM, on the library given by --parent-lib (a build of the parent commit; without it:
      this tree's library, and the output says so): the whole step and its frame kernel lld_acf_pitch_frame -- the yardstick: the same
      1024-point transform at 16 kHz three times per frame (50 ms frames) where lld_chroma_frame transforms once (64 ms frames)
  (c) the new chain with SMILEHIP_CHROMA=block: the workgroup-per-frame form of the frame kernel where the wave form runs
      the rounds of (a), (b) and (c) alternate, so all see the same box; the spread over the rounds is what differences are read against
  (d) the operators route of tests/test_gpu_chroma_fft.py (pcm16_to_float, frame rows, window, rfft, fftmag, tonespec_op, chroma_op) on
      C_UTTS utterances, scaled per frame
  (e) the new chain at 44.1 kHz (the workgroup form), the batch scaled to the same number of samples: one process
  (f) the real binary on config/chroma/chroma_fft.conf, one 10 s file, frames per second of wall time -- if oracle/_ref is there

Every child process runs under its own `timeout -k 10`; the first one that fails ends the run, nothing is retried. The children bind
only the symbols they call, so a parent library that lacks the new preset loads."""
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_UTT, SECONDS, RATE, ROUNDS, STEPS, WARM, DISTINCT, C_UTTS = 12500, 10, 16000, 5, 5, 2, 25, 200
CHILD_LIMIT_S = 240
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
    """kind "chroma": the new preset; "acf": prosodyAcf.conf's (what the parent's library runs)"""
    from opensmile_amd.capi import SYMBOLS, LldConfig, LldConfigChroma
    if kind == "chroma":
        cfg = LldConfigChroma()
        L.smilehip_config_chroma_fft.restype, L.smilehip_config_chroma_fft.argtypes = SYMBOLS["smilehip_config_chroma_fft"]
        L.smilehip_config_chroma_fft(C.byref(cfg), float(rate))
    else:
        cfg = LldConfig()
        L.smilehip_config_prosody_acf.restype, L.smilehip_config_prosody_acf.argtypes = SYMBOLS["smilehip_config_prosody_acf"]
        L.smilehip_config_prosody_acf(C.byref(cfg))
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
    from opensmile_amd import capi
    L = bind(lib_path, ["smilehip_init", "smilehip_plan_create", "smilehip_stream_synchronize", "smilehip_pcm16_to_float", "smilehip_frame_rows",
                        "smilehip_window_frames", "smilehip_rfft_frames", "smilehip_fftmag_frames", "smilehip_tonespec_op_create",
                        "smilehip_tonespec_op_frames", "smilehip_chroma_op_create", "smilehip_chroma_op_frames"])
    ck = checker(L)
    ctx, plan, top, cop = vp(), vp(), vp(), vp()
    ck(L.smilehip_init(0, C.byref(ctx)))
    cfg = config_for(L, "chroma", RATE)
    ck(L.smilehip_plan_create(ctx, C.byref(cfg), C.byref(plan)))
    n, N, H, K, Nfft = SECONDS * RATE, 1024, 160, 513, 1024
    ck(L.smilehip_tonespec_op_create(ctx, C.byref(capi.tonespec_opts()), K, 0.064, C.byref(top)))
    ck(L.smilehip_chroma_op_create(ctx, C.byref(capi.chroma_opts()), 72, C.byref(cop)))
    T = (n - N) // H + 1
    nF = C_UTTS * T
    dev = "cuda"
    pcm = torch.from_numpy(block_pcm(RATE)).to(dev).repeat(C_UTTS // DISTINCT)
    x = torch.zeros(C_UTTS * n, device=dev)
    fr, w, c = torch.zeros((nF, N), device=dev), torch.zeros((nF, N), device=dev), torch.zeros((nF, Nfft), device=dev)
    m, ts, ch = torch.zeros((nF, K), device=dev), torch.zeros((nF, 72), device=dev), torch.zeros((nF, 12), device=dev)

    def step():
        ck(L.smilehip_pcm16_to_float(ctx, pcm.data_ptr(), C_UTTS * n, x.data_ptr(), None))
        for u in range(C_UTTS):
            ck(L.smilehip_frame_rows(ctx, x.data_ptr() + 4 * u * n, N, H, T, fr.data_ptr() + 4 * u * T * N, N, None))
        ck(L.smilehip_window_frames(plan, fr.data_ptr(), N, w.data_ptr(), N, nF, None))
        ck(L.smilehip_rfft_frames(plan, w.data_ptr(), N, c.data_ptr(), Nfft, nF, None))
        ck(L.smilehip_fftmag_frames(plan, c.data_ptr(), Nfft, m.data_ptr(), K, nF, None))
        ck(L.smilehip_tonespec_op_frames(top, m.data_ptr(), K, ts.data_ptr(), 72, nF, None))
        ck(L.smilehip_chroma_op_frames(cop, ts.data_ptr(), 72, ch.data_ptr(), 12, nF, None))
        torch.cuda.synchronize()
    ms = []
    for i in range(WARM + STEPS):
        t0 = time.perf_counter()
        step()
        if i >= WARM:
            ms.append((time.perf_counter() - t0) * 1e3)
    print(json.dumps({"ms": ms, "frames": nF}))


def reference_binary():
    """the real binary on the shipped file, one 10 s file: frames per second of wall time (best of three); None if it is not built"""
    from oracle import lldo
    exe = os.path.join(ROOT, "oracle", "_ref", "SMILExtract")
    conf = os.path.join(ROOT, "oracle", "_ref", "config", "chroma", "chroma_fft.conf")
    if not (os.path.exists(exe) and os.path.exists(conf)):
        return None
    from opensmile_amd import synth
    with tempfile.TemporaryDirectory() as td:
        wav, csv = os.path.join(td, "in.wav"), os.path.join(td, "out.csv")
        lldo.write_wav(wav, synth.utterance(2, SECONDS * RATE), RATE)
        best = None
        for _ in range(3):
            t0 = time.perf_counter()
            subprocess.run(["timeout", "-k", "10", "60", exe, "-C", conf, "-I", wav, "-O", csv, "-l", "0"], check=True, stdout=subprocess.DEVNULL,
                           stderr=subprocess.DEVNULL)
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
        rows = len(open(csv).read().splitlines())
    return {"seconds_of_audio": SECONDS, "frames": rows, "wall_s_best_of_3": best, "frames_per_s": rows / best, "note": "one process per file, start-up included"}


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
    out_path = args[0] if args else os.path.join(ROOT, "profiles", "chroma_fft_timing.json")
    tree_lib = os.path.join(ROOT, "opensmile_amd", "libsmilehip.so")
    a_rounds, b_rounds, c_rounds = [], [], []
    for r in range(ROUNDS):                                # alternating: (a), (b), (c), (a), (b), (c), ...
        a_rounds.append(spawn("--child-chain", tree_lib, "chroma", str(N_UTT), str(RATE)))
        b_rounds.append(spawn("--child-chain", parent_lib or tree_lib, "acf", str(N_UTT), str(RATE)))
        c_rounds.append(spawn("--child-chain", tree_lib, "chroma", str(N_UTT), str(RATE), env={"SMILEHIP_CHROMA": "block"}))
        print("round", r, "a", statistics.median(a_rounds[-1]["ms"]), "b", statistics.median(b_rounds[-1]["ms"]), "c",
              statistics.median(c_rounds[-1]["ms"]), flush=True)
    comp = spawn("--child-components", tree_lib)
    n441 = N_UTT * RATE // 44100
    e = spawn("--child-chain", tree_lib, "chroma", str(n441), "44100")
    a, b, c = summary(a_rounds), summary(b_rounds), summary(c_rounds)
    b["library"] = "parent commit's build" if parent_lib else "THIS tree's build (no --parent-lib given)"
    ka, kb, kc = a["kernels_ms_per_step"], b["kernels_ms_per_step"], c["kernels_ms_per_step"]
    frame_a = sum(v for k, v in ka.items() if "lld_chroma_frame" in k)
    frame_b = sum(v for k, v in kb.items() if "lld_acf_pitch_frame" in k)
    frame_c = sum(v for k, v in kc.items() if "lld_chroma_frame" in k)
    comp_med = statistics.median(comp["ms"])
    res = {
        "workload": "%d x %d s at %d Hz, int16 PCM resident; host clock around smilehip_lld_run + synchronise; %d warm + %d timed steps "
                    "per process, %d alternating rounds of fresh processes; kernels: HIP events around every launch, 3 further steps"
                    % (N_UTT, SECONDS, RATE, WARM, STEPS, ROUNDS),
        "a_chroma_fft": a,
        "b_prosody_acf_chain": b,
        "c_chroma_fft_workgroup_form": c,
        "frame_kernel_ms": {"a_wave_form": frame_a, "b_lld_acf_pitch_frame": frame_b, "c_workgroup_form": frame_c},
        "frame_kernel_ns_per_frame": {"a_wave_form": 1e6 * frame_a / a["frames"], "b_lld_acf_pitch_frame": 1e6 * frame_b / b["frames"],
                                      "c_workgroup_form": 1e6 * frame_c / c["frames"]},
        "a_minus_c_ms": a["ms_per_step_median"] - c["ms_per_step_median"],
        "d_operators_route": {"library": "this tree's build", "utterances": C_UTTS, "frames": comp["frames"], "ms_per_step_median": comp_med,
                              "ms": comp["ms"], "frames_per_s": comp["frames"] / (comp_med * 1e-3),
                              "factor_against_a_per_frame": (comp_med / comp["frames"]) / (a["ms_per_step_median"] / a["frames"])},
        "e_44100_hz": {"utterances": n441, "ms_per_step_median": statistics.median(e["ms"]), "ms": e["ms"], "frames": e["frames"],
                       "fft_size": e["fft_size"], "frames_per_s": e["frames"] / (statistics.median(e["ms"]) * 1e-3),
                       "kernels_ms_per_step": {k: v[1] for k, v in sorted(e["kernels"].items())}, "rounds": 1},
        "f_reference_binary": reference_binary(),
    }
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
