"""Timing of the general cSpecScale operator: HIP events, warm, median of 20; the octave operator of the F0 chains on the same rows;
the plugin's wall time on tests/conf/specscale_general.conf against the plain binary. Prints the figures and writes them to the file
given as the first argument (default: specscale_general_timing.json in the working directory); profiles/specscale_general_timing.json
is one run of it."""
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from opensmile_amd import capi, synth  # noqa: E402
from oracle import lldo  # noqa: E402

L = capi.load()
ctx = capi.Context(0)
ROWS = 65536
res = {"device": ctx.name(), "rows": ROWS, "method": "HIP events around one call, 3 warm-up calls, median of 20", "operators": []}


def timed(fn):
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
    return statistics.median(ms), min(ms), max(ms)


for K in (513, 2049, 4097):
    fs = (K - 1) * 2 / 16000.0
    torch.manual_seed(K)
    d_m = torch.rand((ROWS, K), dtype=torch.float32, device="cuda")
    d_m[:, ::5] *= 30.0
    d_a = torch.zeros((ROWS, K), dtype=torch.float32, device="cuda")
    o = capi.specscale_opts("log", 2.0, 25.0, -1.0, 0, 1, 1, 1)
    op = C.c_void_p()
    capi._check(L.smilehip_specscale_op_create(ctx._h, C.byref(o), K, fs, C.byref(op)))
    med, lo, hi = timed(lambda: capi._check(L.smilehip_specscale_op_frames(op, d_m.data_ptr(), K, d_a.data_ptr(), K, ROWS, None)))
    entry = {"n_src": K, "n_tgt": K, "general_ms": med, "general_min_ms": lo, "general_max_ms": hi,
             "general_rows_per_s": ROWS / (med * 1e-3)}
    capi._check(L.smilehip_specscale_op_destroy(op))
    if K <= 2049:                                           # the octave operator's plans: 512 .. 4096-point transforms
        cfg = capi.compare16_f0_config()
        cfg.force_fft_frame_size_sec = fs
        cfg.force_frame_size = 2 * (K - 1)
        plan = capi.Plan(ctx, cfg)
        d_b = torch.zeros((ROWS, K), dtype=torch.float32, device="cuda")
        med2, lo2, hi2 = timed(lambda: capi._check(L.smilehip_specscale_frames(plan._h, d_m.data_ptr(), K, d_b.data_ptr(), K, ROWS, None)))
        entry.update({"octave_operator_ms": med2, "octave_operator_min_ms": lo2, "octave_operator_max_ms": hi2,
                      "general_over_octave": med / med2, "rows_bit_equal": bool(torch.equal(d_a.view(torch.int32), d_b.view(torch.int32)) or
                                                                               bool(((d_a.view(torch.int32) == d_b.view(torch.int32)) | ((d_a == 0) & (d_b == 0))).all()))})
        del plan, d_b
    res["operators"].append(entry)
    print(entry, flush=True)
    del d_m, d_a
    torch.cuda.empty_cache()

# the plugin inside the unmodified binary: wall time of the whole process, 60 s of audio
exe = os.path.join(lldo.REF_DIR, "SMILExtract")
plugdir = os.path.join(ROOT, "opensmile_amd", "plugin")
conf = os.path.join(ROOT, "tests", "conf", "specscale_general.conf")
pcm = synth.utterance(5, 16000 * 60)
with tempfile.TemporaryDirectory() as td:
    wav, out = os.path.join(td, "in.wav"), os.path.join(td, "out.htk")
    lldo.write_wav(wav, pcm, 16000)
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = os.pathsep.join([os.path.join(ROOT, "opensmile_amd"), lldo.REF_DIR, env.get("LD_LIBRARY_PATH", "")])
    wall = {}
    outs = {}
    for name, extra in (("plain", {"SMILEHIP_PLUGIN_COMPONENTS": "none"}), ("plugin", {})):
        e = dict(env)
        e.update(extra)
        ts = []
        for _ in range(3):
            t0 = time.perf_counter()
            r = subprocess.run([exe, "-C", conf, "-I", wav, "-O", out, "-l", "1"], cwd=plugdir, env=e, capture_output=True, text=True, timeout=120)
            ts.append(time.perf_counter() - t0)
            assert r.returncode == 0, r.stderr[-1000:]
        wall[name] = statistics.median(ts)
        outs[name] = open(out, "rb").read()
    res["plugin_conf"] = {"conf": "tests/conf/specscale_general.conf", "audio_s": 60, "runs": 3, "plain_wall_s": wall["plain"],
                          "plugin_wall_s": wall["plugin"], "plugin_over_plain": wall["plugin"] / wall["plain"],
                          "files_identical": outs["plain"] == outs["plugin"]}
print(res["plugin_conf"], flush=True)
json.dump(res, open(sys.argv[1] if len(sys.argv) > 1 else "specscale_general_timing.json", "w"), indent=1)
