"""Timing of the chroma_filt chain (SMILEHIP_CHAIN_CHROMA_FILT) on the flagship batch shape: 12 500 utterances of 10 s at 16 kHz, PCM
resident on the device, host clock around smilehip_lld_run + stream synchronise, warm. Writes the file given as the first argument
(default: profiles/chroma_filt_timing.json):

  (a) the new chain: ms per step and rows/s -- median of ROUNDS rounds, each a fresh process; and its kernels (HIP events around every
      launch: the library's kernel timing)
  (b) SMILEHIP_CHAIN_CHROMA_FFT on the same PCM, on the library given by --parent-lib (a build of the parent commit; without it: this
      tree's library, and the output says so): the 64 ms FFT route to the same twelve columns
      the rounds of (a) and (b) alternate, so both see the same box; the spread over the rounds is what differences are read against
  (c) the operators route (pcm16_to_float, tonefilt_op, chroma_op) on C_UTTS utterances, one stream after the other (the operator is
      one stream: 72 lanes), scaled per row
  (d) the real binary on config/chroma/chroma_filt.conf, one 10 s file, rows per second of wall time -- if oracle/_ref is there
  (e) the scan kernel's time against 4 cycles x its counted FP64 instructions per step (profiles/chroma_filt_kernel_resources_tree.txt):
      waves per SIMD x steps x FP64_PER_STEP x 4 cycles at the device's clock

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

N_UTT, SECONDS, RATE, ROUNDS, STEPS, WARM, DISTINCT, C_UTTS = 12500, 10, 16000, 3, 3, 1, 25, 2
FP64_PER_STEP = 63                                         # counted in the assembly: profiles/chroma_filt_kernel_resources_tree.txt
NOMINAL_CLOCK_HZ = 2.4e9                                   # MI355X: 2400 MHz maximum
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
    """kind "filt": the new preset; "fft": chroma_fft.conf's (what the parent's library runs; the larger struct holds either)"""
    from opensmile_amd.capi import SYMBOLS, LldConfigChromaFilt
    cfg = LldConfigChromaFilt()
    name = "smilehip_config_chroma_filt" if kind == "filt" else "smilehip_config_chroma_fft"
    f = getattr(L, name)
    f.restype, f.argtypes = SYMBOLS[name][0], [vp, C.c_double]
    f(C.byref(cfg), float(rate))
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
    """one process: plan + batch of n_utt utterances, WARM + STEPS timed runs, then one run with HIP events around every launch"""
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
    ck(L.smilehip_lld_run(plan, batch, d_pcm, d_out, g.n_out, None))
    ck(L.smilehip_stream_synchronize(ctx, None))
    kern = {k: [v[0], v[1]] for k, v in kernel_report(L).items()}
    ck(L.smilehip_kernel_timing(0))
    print(json.dumps({"ms": ms, "frames": frames, "rows": rows, "frame_size": g.frame_size, "kernels": kern}))


def child_components(lib_path):
    """the operators route on C_UTTS utterances: pcm16_to_float over all samples, one tonefilt operator per stream, chroma_op over all rows"""
    import torch
    from opensmile_amd import capi
    L = bind(lib_path, ["smilehip_init", "smilehip_stream_synchronize", "smilehip_pcm16_to_float", "smilehip_tonefilt_op_create",
                        "smilehip_tonefilt_op_blocks", "smilehip_tonefilt_op_reset", "smilehip_chroma_op_create", "smilehip_chroma_op_frames"])
    ck = checker(L)
    ctx, cop = vp(), vp()
    ck(L.smilehip_init(0, C.byref(ctx)))
    n, P = SECONDS * RATE, 160
    T = n // P
    ops = [vp() for _ in range(C_UTTS)]
    for o in ops:
        ck(L.smilehip_tonefilt_op_create(ctx, C.byref(capi.tonefilt_opts()), float(RATE), n, C.byref(o)))
    ck(L.smilehip_chroma_op_create(ctx, C.byref(capi.chroma_opts()), 72, C.byref(cop)))
    dev = "cuda"
    pcm = torch.from_numpy(block_pcm(RATE)[:C_UTTS * n].copy()).to(dev)
    x = torch.zeros(C_UTTS * n, device=dev)
    ts, ch = torch.zeros((C_UTTS * T, 72), device=dev), torch.zeros((C_UTTS * T, 12), device=dev)
    props = torch.cuda.get_device_properties(0)

    def step():
        ck(L.smilehip_pcm16_to_float(ctx, pcm.data_ptr(), C_UTTS * n, x.data_ptr(), None))
        for u, o in enumerate(ops):
            ck(L.smilehip_tonefilt_op_reset(o))
            ck(L.smilehip_tonefilt_op_blocks(o, x.data_ptr() + 4 * u * n, T, ts.data_ptr() + 4 * u * T * 72, None))
        ck(L.smilehip_chroma_op_frames(cop, ts.data_ptr(), 72, ch.data_ptr(), 12, C_UTTS * T, None))
        torch.cuda.synchronize()
    ms = []
    for i in range(WARM + STEPS):
        t0 = time.perf_counter()
        step()
        if i >= WARM:
            ms.append((time.perf_counter() - t0) * 1e3)
    print(json.dumps({"ms": ms, "rows": C_UTTS * T, "cus": props.multi_processor_count, "clock_khz": getattr(props, "clock_rate", 0)}))


def reference_binary():
    """the real binary on the shipped file, one 10 s file: rows per second of wall time (best of three); None if it is not built"""
    from oracle import lldo
    exe = os.path.join(ROOT, "oracle", "_ref", "SMILExtract")
    conf = os.path.join(ROOT, "oracle", "_ref", "config", "chroma", "chroma_filt.conf")
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
    return {"seconds_of_audio": SECONDS, "rows": rows, "wall_s_best_of_3": best, "rows_per_s": rows / best, "note": "one process per file, start-up included"}


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
    return {"ms_per_step_median": med, "ms_rounds": ms, "spread_ms": max(ms) - min(ms), "rows": rounds[0]["rows"],
            "rows_per_s": rounds[0]["rows"] / (med * 1e-3), "frame_size": rounds[0]["frame_size"],
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
    out_path = args[0] if args else os.path.join(ROOT, "profiles", "chroma_filt_timing.json")
    tree_lib = os.path.join(ROOT, "opensmile_amd", "libsmilehip.so")
    a_rounds, b_rounds = [], []
    for r in range(ROUNDS):                                # alternating: (a), (b), (a), (b), ...
        a_rounds.append(spawn("--child-chain", tree_lib, "filt", str(N_UTT), str(RATE)))
        b_rounds.append(spawn("--child-chain", parent_lib or tree_lib, "fft", str(N_UTT), str(RATE)))
        print("round", r, "a", statistics.median(a_rounds[-1]["ms"]), "b", statistics.median(b_rounds[-1]["ms"]), flush=True)
    comp = spawn("--child-components", tree_lib)
    a, b = summary(a_rounds), summary(b_rounds)
    b["library"] = "parent commit's build" if parent_lib else "THIS tree's build (no --parent-lib given)"
    scan_ms = sum(v for k, v in a["kernels_ms_per_step"].items() if "lld_tonefilt_scan" in k)
    comp_med = statistics.median(comp["ms"])
    waves = (N_UTT * 72 + 63) // 64
    simds = 4 * comp["cus"]
    # the clock: what the runtime reports, else the part's nominal maximum (the clock held under this load is not measured either way)
    clock_hz = comp["clock_khz"] * 1e3 if comp["clock_khz"] else NOMINAL_CLOCK_HZ
    clock_source = "reported by the runtime" if comp["clock_khz"] else "nominal maximum of the part; the runtime reported none"
    steps = SECONDS * RATE
    model_ms = (waves / simds) * steps * FP64_PER_STEP * 4 / clock_hz * 1e3
    res = {
        "workload": "%d x %d s at %d Hz, int16 PCM resident; host clock around smilehip_lld_run + synchronise; %d warm + %d timed steps "
                    "per process, %d alternating rounds of fresh processes; kernels: HIP events around every launch, 1 further step"
                    % (N_UTT, SECONDS, RATE, WARM, STEPS, ROUNDS),
        "a_chroma_filt": a,
        "b_chroma_fft_chain": b,
        "a_over_b": a["ms_per_step_median"] / b["ms_per_step_median"],
        "c_operators_route": {"library": "this tree's build", "utterances": C_UTTS, "rows": comp["rows"], "ms_per_step_median": comp_med,
                              "ms": comp["ms"], "rows_per_s": comp["rows"] / (comp_med * 1e-3),
                              "factor_against_a_per_row": (comp_med / comp["rows"]) / (a["ms_per_step_median"] / a["rows"]),
                              "note": "one operator is one stream: 72 lanes walk 160 000 samples; the streams run one after the other"},
        "d_reference_binary": reference_binary() or "not measured",
        "e_scan_kernel_against_its_fp64_issue": {
            "scan_kernel_ms": scan_ms, "fp64_instructions_per_step": FP64_PER_STEP, "cycles_per_fp64_instruction_assumed": 4,
            "waves": waves, "simds": simds, "clock_hz": clock_hz, "clock_source": clock_source, "held_clock": "not measured",
            "steps_per_wave": steps, "model_ms": model_ms, "measured_over_model": scan_ms / model_ms,
            "ns_per_step_and_chain": 1e6 * scan_ms / (N_UTT * 72 * steps)},
    }
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
