"""bench.py's plain line and --dump-outputs: the plain run times exactly --steps steps and carries none of --full's extras;
the dumped arrays are the timed path's own output (checked against the oracle) and repeat bit for bit from run to run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, timeout=600):
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=timeout)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_bench_plain_line_dumps_the_timed_output(tmp_path, oracle):
    from opensmile_amd import synth
    from tolerance import assert_parity
    r = _run(["--gpus", "1", "--utts", "96", "--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path)])
    assert r["steps"] == 3 and r["ms_per_step"] > 0 and r["value"] > 0 and r["dtype"] == "f32"
    for k in ("accuracy", "cpu_baseline", "configs", "h2d_inclusive", "file_to_file"):
        assert k not in r, k
    lld, utt = np.load(tmp_path / "lld.npy"), np.load(tmp_path / "utterances.npy")
    assert lld.dtype == np.float32 and lld.shape == (96 * 998, 39)
    assert np.array_equal(utt, np.arange(96))
    for u in (0, 95):          # the corpus tiles 32 seeded utterances
        ref = oracle.mfcc_chain(oracle.default_cfg(), synth.utterance(u % 32, 160000))
        assert_parity(lld[u * 998:(u + 1) * 998], ref, block=13, what=f"dumped utterance {u}")


@pytest.mark.gpu
def test_bench_dump_outputs_repeat_config5(tmp_path):
    runs = []
    for i in range(2):
        d = tmp_path / f"run{i}"
        r = _run(["--config", "5", "--utts", "64", "--steps", "2", "--warmup", "1", "--dump-outputs", str(d)])
        assert r["steps"] == 2 and r["ms_per_step"] > 0 and "accuracy" not in r
        runs.append({n: np.load(d / f"{n}.npy") for n in ("lld", "functionals", "utterances")})
    a, b = runs
    assert a["functionals"].shape == (64, 88) and a["lld"].shape[1] == 25 and np.array_equal(a["utterances"], np.arange(64))
    for n in a:
        assert a[n].dtype in (np.float32, np.float64)
        assert np.array_equal(a[n].view(np.uint8), b[n].view(np.uint8)), n
