#!/usr/bin/env python3
"""Generate the hard-signal fixtures under tests/golden/ by running the REAL reference binary (oracle/_ref/SMILExtract, built by
oracle/Makefile) on the fifteen signals of tests/helpers/hard_signals.py:

    hard_pcm.npz        the sample arrays themselves (the tests assert that the generator reproduces them)
    hard_mfcc_plp.npz   mfcc/MFCC12_0_D_A.conf (T x 39) and plp/PLP_0_D_A.conf (T x 18)
    hard_is09.npz       is09-13/IS09_emotion.conf: LLD level (T + 1 x 32) and the 384 functionals
    hard_compare16.npz  compare16/ComParE_2016.conf: LLD level (T60 + 1 x 130), the 6373 functionals and their names; for the
                        signals of hard_signals.TAPPED also the levels the six cFunctionals instances read (lldo.FUNC_TAPS)
    hard_egemaps.npz    egemaps/v02/eGeMAPSv02.conf: the 25 LLDs and the 88 functionals

Run from the repo root where the reference is built:
    python tests/golden/make_golden_hard.py
The .npz files are committed; the GPU box only reads them."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import lldo  # noqa: E402
from helpers import hard_signals  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))


def reference_sets(name, pcm):
    """What the binary gives for one signal: {fixture file stem: {key: array}} (also what the pin test compares a fresh run with)."""
    r = {"hard_mfcc_plp": {"mfcc_" + name: lldo.run_reference("mfcc/MFCC12_0_D_A.conf", pcm),
                           "plp_" + name: lldo.run_reference("plp/PLP_0_D_A.conf", pcm)}}
    f, x = lldo.run_reference_func("is09-13/IS09_emotion.conf", pcm)
    r["hard_is09"] = {"lld_" + name: x, "func_" + name: f}
    t = lldo.run_reference_func_taps(pcm)
    r["hard_compare16"] = {"lld_" + name: t["lld"], "func_" + name: t["func"]}
    if name in hard_signals.TAPPED:
        for k in lldo.FUNC_TAPS:
            r["hard_compare16"][k + "_" + name] = t[k]
    r["names"] = t["names"]
    e = lldo.run_reference_egemaps(pcm)
    r["hard_egemaps"] = {"lld_" + name: e["lld"], "func_" + name: e["func"]}
    return r


def main():
    lldo.build()
    assert lldo.have_ref(), "oracle/_ref/SMILExtract missing (the reference is not built)"
    sig = hard_signals.signals()
    files = {"hard_pcm": dict(sig), "hard_mfcc_plp": {}, "hard_is09": {}, "hard_compare16": {}, "hard_egemaps": {}}
    names = None
    for name, pcm in sig.items():
        r = reference_sets(name, pcm)
        names = names or r["names"]
        assert names == r["names"]
        for stem in files:
            if stem != "hard_pcm":
                files[stem].update(r[stem])
        print(name, {k: v.shape for stem in r if stem != "names" for k, v in r[stem].items()})
    files["hard_compare16"]["names"] = np.array(names)
    for stem, d in files.items():
        path = os.path.join(OUT, stem + ".npz")
        np.savez_compressed(path, **d)
        print(stem, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
