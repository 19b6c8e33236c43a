"""Timing of the spectrogram chain (SMILEHIP_CHAIN_SPECTROGRAM) on the flagship batch shape: 12 500 utterances of 10 s at 16 kHz, PCM
resident on the device, host clock around smilehip_lld_run + stream synchronise, warm. 12 475 000 rows x 257 columns = 3.2e9 cells,
12.8 GB of output: cell indices pass 2^31. Writes the file given as the first argument (default: profiles/spectrogram_timing.json):

  (a) the new chain, plain magnitude: ms per step and frames/s -- median of ROUNDS rounds, each a fresh process; and its kernel (HIP
      events around every launch: the library's kernel timing): lld_spectrogram_frame in the wave form
  (b) the same in the dB form: one glibc_log10f per bin more
  (c) the magnitude form with SMILEHIP_SPECTROGRAM=block: the workgroup-per-frame form of the frame kernel where the wave form runs
  (p) SMILEHIP_CHAIN_AUDSPEC on the same PCM, on the library given by --parent-lib (a build of the parent commit; without it: this
      tree's library, and the output says so): the yardstick of a kernel with the same transform and a narrow row
  (m) the headline chain (mfcc12_0_d_a, the fast kernel) on this tree's library and on the parent's: it must not have moved
      the rounds of (a), (b), (c), (p) and (m) alternate, so all see the same box; the spread over the rounds is what differences are
      read against
  (d) the operators route (pcm16_to_float, frame rows, window, rfft, fftmagphase) on C_UTTS utterances, scaled per frame
  (l) the large batch: the last utterance's rows of one run of (a)'s batch equal the same utterance run alone (cells past 2^31)
  (r) the roofline line: bytes moved per frame (H int16 samples read once, K floats written) against the measured time

Every child process runs under its own `timeout -k 10`; the first one that fails ends the run, nothing is retried. The children bind
only the symbols they call, so a parent library that lacks the new chain loads."""
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
HBM_ACHIEVABLE_TBS = 6.3
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
    """kind "spectrogram" / "spectrogram_db": the new preset; "audspec", "mfcc": what the parent's library runs as well"""
    from opensmile_amd.capi import SYMBOLS, LldConfig
    name = {"spectrogram": "smilehip_config_spectrogram", "spectrogram_db": "smilehip_config_spectrogram", "audspec": "smilehip_config_audspec",
            "mfcc": "smilehip_config_mfcc12_0_d_a"}[kind]
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


def child_chain(lib_path, kind, n_utt, rate, check_last):
    """one process: plan + batch of n_utt utterances, WARM + STEPS timed runs, then 3 runs with HIP events around every launch;
    check_last: the last utterance's rows against the same utterance run alone in a batch of its own"""
    from opensmile_amd.capi import Geometry
    names = ["smilehip_init", "smilehip_plan_create", "smilehip_batch_create", "smilehip_alloc", "smilehip_copy_to_device", "smilehip_copy_to_host",
             "smilehip_lld_run", "smilehip_stream_synchronize", "smilehip_plan_geometry", "smilehip_batch_total_frames",
             "smilehip_batch_total_rows", "smilehip_kernel_timing", "smilehip_kernel_timing_report"]
    if kind == "spectrogram_db":
        names.append("smilehip_plan_set_spectrum_form")
    L = bind(lib_path, names)
    ck = checker(L)
    cfg = config_for(L, kind, rate)
    ctx, plan, batch, d_pcm, d_out = vp(), vp(), vp(), vp(), vp()
    ck(L.smilehip_init(0, C.byref(ctx)))
    ck(L.smilehip_plan_create(ctx, C.byref(cfg), C.byref(plan)))
    if kind == "spectrogram_db":
        ck(L.smilehip_plan_set_spectrum_form(plan, 1 | 16, 90.302, -102.0))
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
    res = {"ms": ms, "frames": frames, "rows": rows, "fft_size": g.fft_size, "n_out": g.n_out, "cells": rows * g.n_out}
    if check_last:
        T = rows // n_utt
        last = np.zeros((T, g.n_out), np.float32)
        ck(L.smilehip_copy_to_host(ctx, last.ctypes.data, d_out.value + (rows - T) * g.n_out * 4, last.nbytes, None))
        ck(L.smilehip_stream_synchronize(ctx, None))
        b1, d1 = vp(), vp()
        one = np.array([0, n], np.int64)
        ck(L.smilehip_batch_create(plan, one.ctypes.data, 1, C.byref(b1)))
        ck(L.smilehip_alloc(ctx, last.nbytes, C.byref(d1)))
        ck(L.smilehip_lld_run(plan, b1, d_pcm.value + (n_utt - 1) * n * 2, d1, g.n_out, None))
        alone = np.zeros_like(last)
        ck(L.smilehip_copy_to_host(ctx, alone.ctypes.data, d1, alone.nbytes, None))
        ck(L.smilehip_stream_synchronize(ctx, None))
        res["last_utterance"] = {"first_cell_index": int((rows - T) * g.n_out), "past_2_31": bool((rows - T) * g.n_out > 2 ** 31),
                                 "rows": int(T), "cells_differing_from_the_run_alone": int((last.view(np.uint32) != alone.view(np.uint32)).sum()),
                                 "finite": bool(np.isfinite(last).all())}
    ck(L.smilehip_kernel_timing(1))
    for _ in range(3):
        ck(L.smilehip_lld_run(plan, batch, d_pcm, d_out, g.n_out, None))
    ck(L.smilehip_stream_synchronize(ctx, None))
    res["kernels"] = {k: [v[0], v[1] / 3.0] for k, v in kernel_report(L).items()}
    ck(L.smilehip_kernel_timing(0))
    print(json.dumps(res))


def child_components(lib_path):
    """the operators route on C_UTTS utterances: every operator of the chain as its own launch over all frames"""
    import torch
    L = bind(lib_path, ["smilehip_init", "smilehip_plan_create", "smilehip_stream_synchronize", "smilehip_pcm16_to_float", "smilehip_frame_rows",
                        "smilehip_window_frames", "smilehip_rfft_frames", "smilehip_fftmagphase_frames"])
    ck = checker(L)
    ctx, plan = vp(), vp()
    ck(L.smilehip_init(0, C.byref(ctx)))
    cfg = config_for(L, "spectrogram", RATE)
    ck(L.smilehip_plan_create(ctx, C.byref(cfg), C.byref(plan)))
    n, N, H, K, Nfft = SECONDS * RATE, 400, 160, 257, 512
    T = (n - N) // H + 1
    nF = C_UTTS * T
    dev = "cuda"
    pcm = torch.from_numpy(block_pcm(RATE)).to(dev).repeat(C_UTTS // DISTINCT)
    x = torch.zeros(C_UTTS * n, device=dev)
    fr, w = torch.zeros((nF, N), device=dev), torch.zeros((nF, N), device=dev)
    c, m = torch.zeros((nF, Nfft), device=dev), torch.zeros((nF, K), device=dev)

    def step():
        ck(L.smilehip_pcm16_to_float(ctx, pcm.data_ptr(), C_UTTS * n, x.data_ptr(), None))
        for u in range(C_UTTS):
            ck(L.smilehip_frame_rows(ctx, x.data_ptr() + 4 * u * n, N, H, T, fr.data_ptr() + 4 * u * T * N, N, None))
        ck(L.smilehip_window_frames(plan, fr.data_ptr(), N, w.data_ptr(), N, nF, None))
        ck(L.smilehip_rfft_frames(plan, w.data_ptr(), N, c.data_ptr(), Nfft, nF, None))
        ck(L.smilehip_fftmagphase_frames(ctx, c.data_ptr(), Nfft, Nfft, 1, 90.302, -102.0, m.data_ptr(), K, nF, None))
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
            "frames_per_s": rounds[0]["frames"] / (med * 1e-3), "fft_size": rounds[0]["fft_size"], "n_out": rounds[0]["n_out"],
            "kernels_ms_per_step": {k: statistics.median(r["kernels"].get(k, [0, 0.0])[1] for r in rounds) for k in sorted(rounds[0]["kernels"])}}


def main():
    if sys.argv[1:2] == ["--child-chain"]:
        return child_chain(sys.argv[2], sys.argv[3], int(sys.argv[4]), int(sys.argv[5]), sys.argv[6] == "1")
    if sys.argv[1:2] == ["--child-components"]:
        return child_components(sys.argv[2])
    args, parent_lib = [], None
    it = iter(sys.argv[1:])
    for a in it:
        if a == "--parent-lib":
            parent_lib = os.path.abspath(next(it))
        else:
            args.append(a)
    out_path = args[0] if args else os.path.join(ROOT, "profiles", "spectrogram_timing.json")
    tree_lib = os.path.join(ROOT, "opensmile_amd", "libsmilehip.so")
    a_rounds, b_rounds, c_rounds, p_rounds, mt_rounds, mp_rounds = [], [], [], [], [], []
    for r in range(ROUNDS):                                # alternating: (a), (b), (c), (p), (m) tree, (m) parent, (a), ...
        a_rounds.append(spawn("--child-chain", tree_lib, "spectrogram", str(N_UTT), str(RATE), "1" if r == 0 else "0"))
        b_rounds.append(spawn("--child-chain", tree_lib, "spectrogram_db", str(N_UTT), str(RATE), "0"))
        c_rounds.append(spawn("--child-chain", tree_lib, "spectrogram", str(N_UTT), str(RATE), "0", env={"SMILEHIP_SPECTROGRAM": "block"}))
        p_rounds.append(spawn("--child-chain", parent_lib or tree_lib, "audspec", str(N_UTT), str(RATE), "0"))
        mt_rounds.append(spawn("--child-chain", tree_lib, "mfcc", str(N_UTT), str(RATE), "0"))
        mp_rounds.append(spawn("--child-chain", parent_lib or tree_lib, "mfcc", str(N_UTT), str(RATE), "0"))
        print("round", r, "a", statistics.median(a_rounds[-1]["ms"]), "b", statistics.median(b_rounds[-1]["ms"]), "c",
              statistics.median(c_rounds[-1]["ms"]), "p", statistics.median(p_rounds[-1]["ms"]), "m tree", statistics.median(mt_rounds[-1]["ms"]),
              "m parent", statistics.median(mp_rounds[-1]["ms"]), flush=True)
    comp = spawn("--child-components", tree_lib)
    a, b, c, p, mt, mp = (summary(x) for x in (a_rounds, b_rounds, c_rounds, p_rounds, mt_rounds, mp_rounds))
    which = "parent commit's build" if parent_lib else "THIS tree's build (no --parent-lib given)"
    p["library"] = mp["library"] = which

    def frame_ms(s, word):
        return sum(v for k, v in s["kernels_ms_per_step"].items() if word in k)
    fa, fb, fc, fp = frame_ms(a, "lld_spectrogram_frame"), frame_ms(b, "lld_spectrogram_frame"), frame_ms(c, "lld_spectrogram_frame"), frame_ms(p, "lld_audspec_frame")
    comp_med = statistics.median(comp["ms"])
    H, K = 160, a["n_out"]
    bytes_per_frame = 2 * H + 4 * K                        # H int16 samples read once (the frames overlap: the rest comes from cache), K floats written
    gb = bytes_per_frame * a["frames"] * 1e-9
    res = {
        "workload": "%d x %d s at %d Hz, int16 PCM resident; host clock around smilehip_lld_run + synchronise; %d warm + %d timed steps "
                    "per process, %d alternating rounds of fresh processes; kernels: HIP events around every launch, 3 further steps"
                    % (N_UTT, SECONDS, RATE, WARM, STEPS, ROUNDS),
        "a_spectrogram_magnitude": a,
        "b_spectrogram_db": b,
        "c_spectrogram_workgroup_form": c,
        "p_audspec_chain": p,
        "m_headline_mfcc_chain": {"this_tree": mt, "parent": mp},
        "frame_kernel_ms": {"a_wave_form_magnitude": fa, "b_wave_form_db": fb, "c_workgroup_form": fc, "p_lld_audspec_frame": fp},
        "frame_kernel_ns_per_frame": {"a_wave_form_magnitude": 1e6 * fa / a["frames"], "b_wave_form_db": 1e6 * fb / b["frames"],
                                      "c_workgroup_form": 1e6 * fc / c["frames"], "p_lld_audspec_frame": 1e6 * fp / p["frames"]},
        "b_minus_a_ms": {"step": b["ms_per_step_median"] - a["ms_per_step_median"], "frame_kernel": fb - fa},
        "a_minus_p_ms": {"step": a["ms_per_step_median"] - p["ms_per_step_median"], "frame_kernel": fa - fp},
        "d_operators_route": {"library": "this tree's build", "utterances": C_UTTS, "frames": comp["frames"], "ms_per_step_median": comp_med,
                              "ms": comp["ms"], "frames_per_s": comp["frames"] / (comp_med * 1e-3),
                              "factor_against_a_per_frame": (comp_med / comp["frames"]) / (a["ms_per_step_median"] / a["frames"])},
        "l_large_batch": dict(a_rounds[0]["last_utterance"], cells=a_rounds[0]["cells"]),
        "r_roofline": {"bytes_per_frame": bytes_per_frame, "gbytes_per_step": gb,
                       "ms_at_%.1f_tbytes_per_s" % HBM_ACHIEVABLE_TBS: gb / HBM_ACHIEVABLE_TBS,
                       "gbytes_per_s_at_the_measured_step": gb / (a["ms_per_step_median"] * 1e-3),
                       "gbytes_per_s_in_the_frame_kernel": gb / (fa * 1e-3) if fa else None},
    }
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
