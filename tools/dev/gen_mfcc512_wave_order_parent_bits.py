#!/usr/bin/env python3
"""usage (GPU box, on the PARENT commit's build): tools/dev/gen_mfcc512_wave_order_parent_bits.py <commit hash> <out.npz>
(SMILEHIP_LIB=<the parent's library> where the tree's own is a later one.)
Records the output of the cases of tests/test_gpu_mfcc512_wave_order.py (its run_case) as float32 matrices; the commit hash goes into
the file as 40 hex digits (float32 array `parent_commit_hex`). `ragged`: all rows. `tiled`: the rows of the eight original utterances,
after checking that every one of the 4 104 copies gave exactly those. The result is tests/golden/mfcc512_wave_order_parent_bits.npz."""
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
import test_gpu_mfcc512_wave_order as cases  # noqa: E402


def main():
    commit, path = sys.argv[1], sys.argv[2]
    assert len(commit) == 40 and int(commit, 16) >= 0
    ctx = capi.Context(0)
    arrays = {"parent_commit_hex": np.array([int(c, 16) for c in commit], np.float32)}
    for name in cases.CASES:
        out, ran = cases.run_case(capi, ctx, name)
        assert "lld_mfcc512" in ran and "lld_chain_tiled" not in ran and np.isfinite(out).all(), (name, ran)
        out = np.ascontiguousarray(out, np.float32)
        if name == "tiled":
            rows = cases.TILED_UNIQUE * cases.TILED_FRAMES
            copies = out.reshape(-1, rows, out.shape[1])
            assert copies.shape[0] == cases.TILED_COPIES // cases.TILED_UNIQUE
            assert (copies.view(np.uint32) == copies[:1].view(np.uint32)).all(), "the copies differ on the parent"
            out = np.ascontiguousarray(copies[0])
        arrays[name] = out
        print(name, out.shape, sorted(ran))
    np.savez_compressed(path, **arrays)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()
