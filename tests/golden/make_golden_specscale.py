#!/usr/bin/env python3
"""Generate tests/golden/specscale_general_synth.npz: the levels of tests/conf/specscale_general.conf (the magnitude level and one
cSpecScale instance per target scale, in one HTK file of 1256 columns) as the REAL reference binary (oracle/_ref/SMILExtract, built
from the reference sources by oracle/Makefile) writes them for two short utterances of the synthetic-corpus contract
(opensmile_amd/synth.py). Data only; run from the repository root where the reference build exists:
    python tests/golden/make_golden_specscale.py
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import lldo  # noqa: E402
from opensmile_amd import synth  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
CONF = os.path.join(ROOT, "tests", "conf", "specscale_general.conf")


def main():
    ref = {}
    for key, (u, n) in {"u3_6400": (3, 6400), "u10_4800": (10, 4800)}.items():
        pcm = synth.utterance(u, n)
        with tempfile.TemporaryDirectory() as td:
            wav, out = os.path.join(td, "in.wav"), os.path.join(td, "out.htk")
            lldo.write_wav(wav, pcm, 16000)
            subprocess.run([os.path.join(lldo.REF_DIR, "SMILExtract"), "-C", CONF, "-I", wav, "-O", out, "-l", "0"], check=True, cwd=td,
                           stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
            y = lldo.read_htk(out)[0]
        assert y.shape[1] == 1256 and 2 <= y.shape[0] <= 40, y.shape
        ref["pcm_" + key] = pcm
        ref["out_" + key] = y
        print(key, y.shape)
    # the magnitude level's frameSizeSec: 400 samples at 16 kHz, zero-padded to 512 by cTransformFFT (transformFft.cpp:79-83)
    ref["frame_size_sec"] = np.float64(0.025 * (512.0 / 400.0))
    np.savez_compressed(os.path.join(OUT, "specscale_general_synth.npz"), **ref)


if __name__ == "__main__":
    main()
