"""Timing of the emobase chain (SMILEHIP_CHAIN_EMOBASE) on the flagship batch shape: 12 500 utterances of 10 s at 16 kHz, PCM resident on
the device, host clock around smilehip_lld_run + stream synchronise, warm. Writes the file given as the first argument (default:
profiles/emobase_timing.json):

  (a) the new chain: ms per step and steps/s -- median of ROUNDS rounds, each a fresh process; and its kernels one by one (HIP events
      around every launch: the library's kernel timing)
  (b) SMILEHIP_CHAIN_IS09 (25 ms frames: MFCC, ZCR, energy, ACF pitch, SMA, delta) on the same PCM, on the library given by
      --parent-lib (a build of the parent commit; without it: this tree's library, and the output says so)
  (p) SMILEHIP_CHAIN_PROSODY_ACF (50 ms frames: ACF / cepstrum pitch, loudness, SMA) on the same PCM and library as (b)
      -- emobase does the work of both and more: a_over_b_plus_p is the new chain's step over the sum of the two
  (c) the new chain with SMILEHIP_EMOBASE=block: the workgroup-per-step form of the frame kernel where the wave form runs
      the rounds of (a), (b), (p) and (c) alternate, so all see the same box; the spread over the rounds is what differences are read against
  (d) the per-component operators route (pcm16_to_float, frame rows twice, intensity, mzcr, preemphasis, lpc_acf, lsp, window, rfft,
      fftmag, melspec, mfcc; window, rfft, fftmag, acf twice, pitchacf, contour per utterance; window_op_block twice) on C_UTTS
      utterances on the library of (b), scaled per step

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
    """kind "emobase": the new preset; "is09" / "acf": the parent's presets as they are; "is09_40": IS09's plan on 40 ms frames
    without pre-emphasis (window and transform of the second framer, for the operators route)"""
    from opensmile_amd.capi import LldConfig, SYMBOLS
    cfg = LldConfig()
    name = {"emobase": "smilehip_config_emobase", "acf": "smilehip_config_prosody_acf"}.get(kind, "smilehip_config_is09_lld")
    f = getattr(L, name)
    f.restype, f.argtypes = SYMBOLS[name]
    f(C.byref(cfg))
    if kind == "is09_25":
        cfg.use_power = 1                                  # [mspec:cMelspec] usePower = 1
    if kind == "is09_40":
        cfg.frame_size_sec, cfg.preemph = 0.040, 0
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
    print(json.dumps({"ms": ms, "frames": frames, "rows": rows, "fft_size": g.fft_size, "n_out": g.n_out, "kernels": kern}))


def child_components(lib_path):
    """the per-component route on C_UTTS utterances: every operator of the file as its own launch over all frames"""
    import torch
    L = bind(lib_path, ["smilehip_init", "smilehip_plan_create", "smilehip_stream_synchronize", "smilehip_pcm16_to_float", "smilehip_frame_rows",
                        "smilehip_window_frames", "smilehip_rfft_frames", "smilehip_fftmag_frames", "smilehip_acf_frames", "smilehip_pitchacf_frames",
                        "smilehip_pitchacf_contour_frames", "smilehip_intensity_frames", "smilehip_mzcr_frames", "smilehip_preemphasis_frames",
                        "smilehip_lpc_acf_frames", "smilehip_lsp_frames", "smilehip_melspec_frames", "smilehip_mfcc_frames", "smilehip_window_op_block"])
    ck = checker(L)
    ctx, plan25, plan40 = vp(), vp(), vp()
    ck(L.smilehip_init(0, C.byref(ctx)))
    c25, c40 = config_for(L, "is09_25", RATE), config_for(L, "is09_40", RATE)
    ck(L.smilehip_plan_create(ctx, C.byref(c25), C.byref(plan25)))
    ck(L.smilehip_plan_create(ctx, C.byref(c40), C.byref(plan40)))
    n, H = SECONDS * RATE, 160
    N25, K25, F25, N40, K40, F40, M40 = 400, 257, 512, 640, 513, 1024, 512
    T25, T40 = (n - N25) // H + 1, (n - N40) // H + 1
    n25, n40 = C_UTTS * T25, C_UTTS * T40
    dev = "cuda"
    z = lambda *s, **k: torch.zeros(s, device=dev, **k)    # noqa: E731
    pcm = torch.from_numpy(block_pcm(RATE)).to(dev).repeat(C_UTTS // DISTINCT)
    x = z(C_UTTS * n)
    fr25, pe, w25, c25b, m25, mel, cc = z(n25, N25), z(n25, N25), z(n25, N25), z(n25, F25), z(n25, K25), z(n25, 26), z(n25, 12)
    it, zc, lpc, lsp = z(n25, 2), z(n25, 1), z(n25, 8), z(n25, 8)
    fr40, w40, c40b, m40, ac = z(n40, N40), z(n40, N40), z(n40, F40), z(n40, K40), z(n40, 2 * M40)
    v, idx = z(n40, dtype=torch.float64), z(n40, dtype=torch.int32)
    state, o4 = z(C_UTTS, 8), z(n40, 4)
    lvl, lld, de = z(n25 + 4, 26), z(n25 + 4, 26), z(n25 + 4, 26)
    fs_sec = float(np.float32(0.04 * F40 / N40))

    def step():
        ck(L.smilehip_pcm16_to_float(ctx, pcm.data_ptr(), C_UTTS * n, x.data_ptr(), None))
        for u in range(C_UTTS):
            ck(L.smilehip_frame_rows(ctx, x.data_ptr() + 4 * u * n, N25, H, T25, fr25.data_ptr() + 4 * u * T25 * N25, N25, None))
            ck(L.smilehip_frame_rows(ctx, x.data_ptr() + 4 * u * n, N40, H, T40, fr40.data_ptr() + 4 * u * T40 * N40, N40, None))
        ck(L.smilehip_intensity_frames(ctx, fr25.data_ptr(), N25, N25, 3, it.data_ptr(), 2, n25, None))
        ck(L.smilehip_mzcr_frames(ctx, fr25.data_ptr(), N25, N25, n25, 1, zc.data_ptr(), 1, None))
        ck(L.smilehip_preemphasis_frames(ctx, fr25.data_ptr(), N25, pe.data_ptr(), N25, n25, N25, 0.97, 0, None))
        ck(L.smilehip_lpc_acf_frames(ctx, pe.data_ptr(), N25, N25, 8, lpc.data_ptr(), 8, n25, None))
        ck(L.smilehip_lsp_frames(ctx, lpc.data_ptr(), 8, 8, lsp.data_ptr(), 8, n25, None))
        ck(L.smilehip_window_frames(plan25, pe.data_ptr(), N25, w25.data_ptr(), N25, n25, None))
        ck(L.smilehip_rfft_frames(plan25, w25.data_ptr(), N25, c25b.data_ptr(), F25, n25, None))
        ck(L.smilehip_fftmag_frames(plan25, c25b.data_ptr(), F25, m25.data_ptr(), K25, n25, None))
        ck(L.smilehip_melspec_frames(plan25, m25.data_ptr(), K25, mel.data_ptr(), 26, n25, None))
        ck(L.smilehip_mfcc_frames(plan25, mel.data_ptr(), 26, cc.data_ptr(), 12, n25, None))
        ck(L.smilehip_window_frames(plan40, fr40.data_ptr(), N40, w40.data_ptr(), N40, n40, None))
        ck(L.smilehip_rfft_frames(plan40, w40.data_ptr(), N40, c40b.data_ptr(), F40, n40, None))
        ck(L.smilehip_fftmag_frames(plan40, c40b.data_ptr(), F40, m40.data_ptr(), K40, n40, None))
        ck(L.smilehip_acf_frames(plan40, m40.data_ptr(), K40, ac.data_ptr(), 2 * M40, M40, n40, 1, 0, 0, 0, None))
        ck(L.smilehip_acf_frames(plan40, m40.data_ptr(), K40, ac.data_ptr() + 4 * M40, 2 * M40, M40, n40, 1, 2, 0, 1, None))
        ck(L.smilehip_pitchacf_frames(ctx, ac.data_ptr(), 2 * M40, M40, n40, fs_sec, 500.0, v.data_ptr(), idx.data_ptr(), None))
        state.zero_()
        for u in range(C_UTTS):
            ck(L.smilehip_pitchacf_contour_frames(ctx, v.data_ptr() + 8 * u * T40, idx.data_ptr() + 4 * u * T40, fs_sec / F40, 0.55,
                                                  state.data_ptr() + 32 * u, o4.data_ptr() + 16 * u * T40, T40, None))
        lvl[2:2 + n25, 0:2] = it
        lvl[2:2 + n25, 2:14] = cc
        lvl[2:2 + n25, 14:22] = lsp
        lvl[2:2 + n25, 22:23] = zc
        lvl[2:2 + n40, 23] = v.float()
        lvl[2:2 + n40, 24] = o4[:, 0]
        lvl[2:2 + n40, 25] = o4[:, 2]
        for u in range(C_UTTS):                            # (the block's edge frames are its neighbours here: timing only, the tests check values)
            ck(L.smilehip_window_op_block(ctx, lvl.data_ptr() + 104 * (2 + u * T40), 26, lld.data_ptr() + 104 * (2 + u * T40), 26, T40, 26, 1, 1, 0, None))
        for u in range(C_UTTS):
            ck(L.smilehip_window_op_block(ctx, lld.data_ptr() + 104 * (2 + u * T40), 26, de.data_ptr() + 104 * (2 + u * T40), 26, T40, 26, 0, 2, 0, None))
        torch.cuda.synchronize()
    ms = []
    for i in range(WARM + STEPS):
        t0 = time.perf_counter()
        step()
        if i >= WARM:
            ms.append((time.perf_counter() - t0) * 1e3)
    print(json.dumps({"ms": ms, "frames": n25}))


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
    out_path = args[0] if args else os.path.join(ROOT, "profiles", "emobase_timing.json")
    tree_lib = os.path.join(ROOT, "opensmile_amd", "libsmilehip.so")
    other = parent_lib or tree_lib
    a_rounds, b_rounds, p_rounds, c_rounds = [], [], [], []
    for r in range(ROUNDS):                                # alternating: (a), (b), (p), (c), (a), ...
        a_rounds.append(spawn("--child-chain", tree_lib, "emobase", str(N_UTT), str(RATE)))
        b_rounds.append(spawn("--child-chain", other, "is09", str(N_UTT), str(RATE)))
        p_rounds.append(spawn("--child-chain", other, "acf", str(N_UTT), str(RATE)))
        c_rounds.append(spawn("--child-chain", tree_lib, "emobase", str(N_UTT), str(RATE), env={"SMILEHIP_EMOBASE": "block"}))
        print("round", r, "a", statistics.median(a_rounds[-1]["ms"]), "b", statistics.median(b_rounds[-1]["ms"]), "p",
              statistics.median(p_rounds[-1]["ms"]), "c", statistics.median(c_rounds[-1]["ms"]), flush=True)
    comp = spawn("--child-components", other)
    a, b, p, c = summary(a_rounds), summary(b_rounds), summary(p_rounds), summary(c_rounds)
    which = "parent commit's build" if parent_lib else "THIS tree's build (no --parent-lib given)"
    b["library"] = p["library"] = which
    ka, kc = a["kernels_ms_per_step"], c["kernels_ms_per_step"]
    total_a = sum(ka.values())
    frame_a = sum(v for k, v in ka.items() if "lld_emobase_frame" in k)
    lsp_a = sum(v for k, v in ka.items() if "lld_emobase_lsp" in k)
    frame_c = sum(v for k, v in kc.items() if "lld_emobase_frame" in k)
    comp_med = statistics.median(comp["ms"])
    res = {
        "workload": "%d x %d s at %d Hz, int16 PCM resident; host clock around smilehip_lld_run + synchronise; %d warm + %d timed steps "
                    "per process, %d alternating rounds of fresh processes; kernels: HIP events around every launch, 3 further steps"
                    % (N_UTT, SECONDS, RATE, WARM, STEPS, ROUNDS),
        "a_emobase": a,
        "b_is09_chain": b,
        "p_prosody_acf_chain": p,
        "c_emobase_workgroup_form": c,
        "a_over_b_plus_p": a["ms_per_step_median"] / (b["ms_per_step_median"] + p["ms_per_step_median"]),
        "kernels_of_a_ms": {"frame_kernel_wave_form": frame_a, "lsp_row_kernel": lsp_a,
                            "contour_scan": sum(v for k, v in ka.items() if "lld_emobase_contour" in k),
                            "tail_row_kernel": sum(v for k, v in ka.items() if "lld_emobase_tail" in k), "all": total_a,
                            "frame_kernel_share": frame_a / total_a if total_a else None, "lsp_row_kernel_share": lsp_a / total_a if total_a else None,
                            "c_frame_kernel_workgroup_form": frame_c, "workgroup_over_wave": frame_c / frame_a if frame_a else None},
        "a_minus_c_ms": a["ms_per_step_median"] - c["ms_per_step_median"],
        "d_per_component": {"library": which, "utterances": C_UTTS, "frames": comp["frames"], "ms_per_step_median": comp_med, "ms": comp["ms"],
                            "frames_per_s": comp["frames"] / (comp_med * 1e-3),
                            "factor_against_a_per_frame": (comp_med / comp["frames"]) / (a["ms_per_step_median"] / a["frames"])},
    }
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
