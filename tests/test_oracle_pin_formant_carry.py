"""cFormantLpc when the QR root solver gives up, pinned on the real binary (oracle/_ref/SMILExtract).

The reference keeps `roots` as a member of cFormantLpc (src/lld/formantLpc.cpp:196), malloc'ed once and never cleared.
zerosolveQRhelper writes a root only when it finds one and stops after 70 iterations without a deflation
(src/smileutil/zerosolve.cpp:166-168, 337-341); the return value is ignored (formantLpc.cpp:270). A frame whose iteration
gives up therefore works on the previous frame's roots, already folded into the unit circle by the in-place
smileMath_complexIntoUnitCircle, and the log gets "zerosolve: the QR-method for root solving did not converge!" once.

What makes it give up: a NaN in any LP coefficient. A float WAV with NaN samples reaches cLpc unchanged (cWaveSource passes
floats through) and gives NaN coefficients. The oracle (oracle/lld_oracle_gemaps.c: lldo_formant_lpc with a caller-owned
roots array that oracle/lldo.py::egemaps_formant_rows carries from row to row) must give the binary's rows bit for bit; the
device (tests/test_gpu_formant_carry.py) is then held to the oracle.

Finite coefficients never gave up in a seeded host search with the oracle's solver: 117 990 LP rows of the oracle's own chain
(framer, Hamming window, FFT, cSpecResample to 11 kHz, cLpc p = 11) at 8, 11.025, 16, 22.05, 32, 44.1 and 48 kHz, from pure
tones at five amplitudes down to 1 LSB, sums of 2-5 tones, square and clipped waves, DC, impulse trains and near-silence
(+-1, +-2 LSB noise, isolated 1-2 LSB clicks) -- none of them left a root slot unwritten. So no frame is known that gives up
after finding some roots: the device's rule for that case (re-solve on top of the carried roots) follows the reference but is
not exercised by a test. +-inf coefficients are never fed anywhere: the balancing loop of zerosolveBalanceCmatrix does not end
on them, in the reference as on the device."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tolerance import assert_bits_equal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONF = os.path.join(ROOT, "tests", "conf", "formant_chain.conf")
NOT_CONVERGED = "the QR-method for root solving did not converge!"
# NaN bursts of the test signal (sample ranges at 16 kHz): one sample, ~30 ms, ~120 ms; the first one after 17 converged frames
# (the reference's first frame would read uninitialised memory if it gave up)
BURSTS = ((3000, 3001), (9600, 10080), (19000, 20920))


def write_f32_wav(path, x, fs=16000):
    """Mono 32-bit IEEE float WAV (format tag 3); x must be finite or NaN, never +-inf."""
    x = np.ascontiguousarray(x, dtype="<f4")
    assert (np.isfinite(x) | np.isnan(x)).all(), "+-inf samples would hang the root solver"
    data = x.tobytes()
    fmt = struct.pack("<HHIIHH", 3, 1, fs, fs * 4, 4, 32)
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", 4 + 8 + len(fmt) + 8 + len(data)) + b"WAVE")
        f.write(b"fmt " + struct.pack("<I", len(fmt)) + fmt)
        f.write(b"data" + struct.pack("<I", len(data)) + data)


def nan_burst_signal(n=32000):
    """synth.utterance in [-1, 1) as float32 with the NaN bursts of BURSTS."""
    from opensmile_amd import synth
    x = (synth.utterance(3, n).astype(np.float64) / 32768.0).astype(np.float32)
    for a, b in BURSTS:
        x[a:b] = np.nan
    return x


def run_formant_chain(exe, wav, td, env=None, cwd=None):
    """SMILExtract on tests/conf/formant_chain.conf -> (lpc rows, formant rows, log text). -l 1 shows SMILE_ERR."""
    r = subprocess.run([exe, "-C", CONF, "-I", wav, "-T", td, "-l", "1"], capture_output=True, text=True, timeout=120, env=env,
                       cwd=cwd or td)
    log = r.stdout + r.stderr
    assert r.returncode == 0, log[-2000:]
    from oracle import lldo
    return lldo.read_htk(os.path.join(td, "tap_lpc.htk"))[0], lldo.read_htk(os.path.join(td, "tap_formants.htk"))[0], log


@pytest.mark.skipif(not __import__("oracle.lldo", fromlist=["x"]).have_ref(), reason="oracle/_ref not built")
def test_nan_lpc_frames_carry_the_roots_like_the_binary(oracle, tmp_path):
    x = nan_burst_signal()
    wav = str(tmp_path / "nan.wav")
    write_f32_wav(wav, x)
    lpc, fm, log = run_formant_chain(os.path.join(oracle.REF_DIR, "SMILExtract"), wav, str(tmp_path))
    assert lpc.shape == (199, 11) and fm.shape == (199, 10)
    assert not np.isinf(lpc).any()
    nan_rows = np.flatnonzero(np.isnan(lpc).any(axis=1))
    # a 320-sample frame every 160 samples: 2 frames see the single sample, 4 the 30 ms burst, 14 the 120 ms one
    assert len(nan_rows) == 2 + 4 + 14 and nan_rows[0] == 17, nan_rows
    # the path was taken: one message per NaN-LP frame
    assert log.count(NOT_CONVERGED) == len(nan_rows), log[-2000:]
    # the oracle carries its roots like the binary's member
    assert_bits_equal(oracle.egemaps_formant_rows(lpc), fm, "oracle vs binary, NaN LP rows")
    # no root found: the frame repeats the last converged frame's row (not zeros)
    for i in nan_rows:
        assert np.array_equal(fm[i].view(np.uint32), fm[i - 1].view(np.uint32)), i
    assert (fm[nan_rows, 0] > 0).all()
