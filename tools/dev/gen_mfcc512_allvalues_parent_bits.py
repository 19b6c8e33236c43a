#!/usr/bin/env python3
"""usage (GPU box, on the PARENT commit's build, or with SMILEHIP_LIB=<a copy of the parent commit's libsmilehip.so>):
    tools/dev/gen_mfcc512_allvalues_parent_bits.py <commit hash> <out.npz>
Records the output of every case of tests/test_gpu_mfcc512_typed_loads.py (its CASES and run_case: all 65 536 int16 values through
both samples of a pair) as float32 matrices; the commit hash goes into the file as 40 hex digits (float32 array
`parent_commit_hex`). The result is tests/golden/mfcc512_allvalues_parent_bits.npz.

The input and the cases are the TEST MODULE's (imported below), so that fixture and test cannot drift apart -- which also means
that an edit of the test's CASES, SEED, all_values_utterance or run_case changes what a later run of this script records. The
committed fixture was recorded with the test module as it stands in the commit that added it, from the library of the commit
whose hash it stores (that commit's parent); after such an edit the fixture has to be recorded again from that same parent."""
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
import test_gpu_mfcc512_typed_loads as cases  # noqa: E402


def main():
    commit, path = sys.argv[1], sys.argv[2]
    assert len(commit) == 40 and int(commit, 16) >= 0
    ctx = capi.Context(0)
    arrays = {"parent_commit_hex": np.array([int(c, 16) for c in commit], np.float32)}
    for name, (_, _, want) in cases.CASES.items():
        out, ran = cases.run_case(capi, ctx, name)
        assert want in ran and np.isfinite(out).all(), (name, ran)
        arrays[name] = np.ascontiguousarray(out, np.float32)
        print(name, out.shape, sorted(ran))
    np.savez_compressed(path, **arrays)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()
