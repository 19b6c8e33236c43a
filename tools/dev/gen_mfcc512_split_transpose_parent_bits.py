#!/usr/bin/env python3
"""usage (GPU box, on the PARENT commit's build): tools/dev/gen_mfcc512_split_transpose_parent_bits.py <commit hash> <out.npz>
Records the output of every case of tests/test_gpu_mfcc512_split_transpose_bits.py (its CASES and run_case) as float32 matrices; the
commit hash goes into the file as 40 hex digits (float32 array `parent_commit_hex`). The result is
tests/golden/mfcc512_split_transpose_parent_bits.npz. SMILEHIP_LIB names the library to record from when it is not the tree's own
(opensmile_amd/capi.py)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
try:
    import torch  # noqa: F401  (first, as tests/conftest.py does: one HIP runtime in the process)
except Exception:
    pass
from opensmile_amd import capi  # noqa: E402
import test_gpu_mfcc512_split_transpose_bits as cases  # noqa: E402


def main():
    commit, path = sys.argv[1], sys.argv[2]
    assert len(commit) == 40 and int(commit, 16) >= 0
    ctx = capi.Context(0)
    arrays = {"parent_commit_hex": np.array([int(c, 16) for c in commit], np.float32)}
    for name in cases.CASES:
        out, ran = cases.run_case(capi, ctx, name)
        assert cases.CASES[name][1] in ran and "lld_mfcc_generic" not in ran and np.isfinite(out).all(), (name, ran)
        arrays[name] = np.ascontiguousarray(out, np.float32)
        print(name, out.shape, sorted(ran))
    np.savez_compressed(path, **arrays)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()
