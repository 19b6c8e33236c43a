#!/usr/bin/env python3
"""Generate tests/golden/spectral_axis_synth.npz: the levels of tests/conf/spectral_axis.conf (the magnitude level, a bark and a mel
cSpecScale level and one cSpectral instance per option set, in one HTK file) as the REAL reference binary (oracle/_ref/SMILExtract,
built from the reference sources by oracle/Makefile) writes them for two short utterances of the synthetic-corpus contract
(opensmile_amd/synth.py) at 16 kHz (257 bins) and for the first of them played at 44.1 kHz (1025 bins). Data only; run from the
repository root where the reference build exists:
    python tests/golden/make_golden_spectral_axis.py
"""
import math
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
CONF = os.path.join(ROOT, "tests", "conf", "spectral_axis.conf")
N_SPECTRAL = 26 + 40 + 18 + 18 + 7 + 3 + 3 + 7 + 6 + 6 + 4     # the columns behind the magnitude level


def main():
    ref = {}
    for key, (u, n, rate) in {"u3_6400": (3, 6400, 16000), "u10_4800": (10, 4800, 16000), "u3_6400_44k": (3, 6400, 44100)}.items():
        pcm = synth.utterance(u, n)
        with tempfile.TemporaryDirectory() as td:
            wav, out = os.path.join(td, "in.wav"), os.path.join(td, "out.htk")
            lldo.write_wav(wav, pcm, rate)
            subprocess.run([os.path.join(lldo.REF_DIR, "SMILExtract"), "-C", CONF, "-I", wav, "-O", out, "-l", "0"], check=True, cwd=td,
                           stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
            y = lldo.read_htk(out)[0]
        # 25 ms frames: round(0.025 rate) samples (winToVecProcessor.cpp:435-456), zero-padded to the next power of two by
        # cTransformFFT, which scales the level's frameSizeSec with it (transformFft.cpp:79-83)
        N = int(math.floor(0.025 / (1.0 / rate) + 0.5))     # C's round(): half away from zero
        nfft = 1 << (N - 1).bit_length()
        K = nfft // 2 + 1
        assert y.shape[1] == K + N_SPECTRAL and 2 <= y.shape[0] <= 40, y.shape
        ref["out_" + key] = y
        ref["K_" + key] = np.int32(K)
        ref["frame_size_sec_" + key] = np.float64(0.025 * (float(nfft) / float(N)))
        print(key, y.shape, K)
    np.savez_compressed(os.path.join(OUT, "spectral_axis_synth.npz"), **ref)


if __name__ == "__main__":
    main()
