"""The g++ build of opensmile_amd/csrc/lld_spectrogram_ops.hpp (tests/helpers/spectrogram_check.cpp, a stand-alone program), the
reference of the spectrogram tests, and what they share: the fixtures, their cases, the samples of each input, the form of each case
as the C ABI takes it."""
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FORMS = ("mag", "db", "norm", "pow", "normpow")
# SMILEHIP_MAGPHASE_* bits of each form (1 magnitude, 4 normalise, 8 power, 16 dBpsd), the form index of lld_spectrogram_ops.hpp, and
# the field name cFFTmagphase gives the level (fftmagphase.cpp:141-155)
FLAGS = {"mag": 1, "norm": 1 | 4, "pow": 1 | 8, "normpow": 1 | 4 | 8, "db": 1 | 16}
FORM_INDEX = {"mag": 0, "norm": 1, "pow": 2, "normpow": 3, "db": 4}
FIELD = {"mag": "pcm_fftMag", "norm": "pcm_fftMag_SpecDens", "pow": "pcm_fftMag_PowSpec", "normpow": "pcm_fftMag_PowSpecDens",
         "db": "pcm_fftMag_dBsplPSD"}
DBP_NORM, MIN_DBP = 90.302, -102.0                          # the component's defaults
_exe = None
_fix = {}


def exe():
    """path of the built program (rebuilt when a source is newer)"""
    global _exe
    if _exe is not None:
        return _exe
    csrc = os.path.join(ROOT, "opensmile_amd", "csrc")
    src = os.path.join(ROOT, "tests", "helpers", "spectrogram_check.cpp")
    out = os.path.join(ROOT, "tests", "helpers", "_spectrogram_check")
    deps = [src] + [os.path.join(csrc, h) for h in ("lld_spectrogram_ops.hpp", "glibc_float.hpp")]
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(p) for p in deps):
        tmp = out + ".%d.new" % os.getpid()
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-o", tmp, src, "-lm"], check=True)
        os.replace(tmp, out)
    _exe = out
    return out


def rows_of(n, N, H):
    return int(subprocess.run([exe(), "rows", str(n), str(N), str(H)], check=True, capture_output=True, text=True).stdout)


def clamp_bits(dbp_norm, min_dbp):
    return int(subprocess.run([exe(), "clamp", repr(float(dbp_norm)), repr(float(min_dbp))], check=True, capture_output=True, text=True).stdout, 16)


def form_of_flags(flags):
    return int(subprocess.run([exe(), "form", str(flags)], check=True, capture_output=True, text=True).stdout)


def spectrum_rows(fft, form, dbp_norm=DBP_NORM, min_dbp=MIN_DBP):
    """rows of the level fft [T x Nfft] -> rows of the level lld [T x Nfft / 2 + 1] in `form`, by the host build of the row functions"""
    fft = np.ascontiguousarray(fft, np.float32)
    T, nfft = fft.shape
    with tempfile.TemporaryDirectory() as td:
        a, b = os.path.join(td, "in.f32"), os.path.join(td, "out.f32")
        fft.tofile(a)
        subprocess.run([exe(), "spectrum", str(FORM_INDEX[form]), str(nfft), repr(float(dbp_norm)), repr(float(min_dbp)), a, b], check=True)
        return np.fromfile(b, np.float32).reshape(T, nfft // 2 + 1)


def fixture(name="spectrogram_synth.npz"):
    if name not in _fix:
        _fix[name] = np.load(os.path.join(GOLDEN, name))
    return _fix[name]


def cases(name="spectrogram_synth.npz"):
    """[(key, idx, n, fs, form, zps, frame_size, frame_step)] of a fixture (make_golden_spectrogram.py)"""
    return [(str(c[0]), int(c[1]), int(c[2]), int(c[3]), str(c[4]), int(c[5]), float(c[6]), float(c[7])) for c in fixture(name)["cases"]]


def fft_of(name, key):
    """the tapped fft level of a case: stored once per input, under the key without its form; None where the fixture keeps none"""
    f = fixture(name)
    k = "fft_" + key.split("_", 1)[1]
    return f[k] if k in f.files else None


def cut(idx, n):
    """the samples of a fixture input (make_golden_spectrogram.py: cut)"""
    from opensmile_amd import synth
    return synth.utterance(int(idx), int(n)).astype(np.int16) if n else np.zeros(0, np.int16)


def config(fs, zps=1, frame_size=0.025, frame_step=0.010):
    from opensmile_amd import capi
    c = capi.spectrogram_config(fs, frame_size, frame_step)
    c.zero_pad_symmetric = int(zps)
    return c


# the project's own text of the graph (the reference's file includes shared files; this one stands alone): cWaveSource, the four
# components, the file's three command-line options, an HTK and a CSV sink on lld
MINIMAL = """[componentInstances:cComponentManager]
instance[dataMemory].type = cDataMemory
instance[src].type = cWaveSource
instance[fr].type = cFramer
instance[win].type = cWindower
instance[fft].type = cTransformFFT
instance[mag].type = cFFTmagphase
instance[out].type = cHtkSink
instance[csv].type = cCsvSink
[src:cWaveSource]
writer.dmLevel = wave
filename = \\cm[inputfile(I){in.wav}:input]
monoMixdown = 1
[fr:cFramer]
reader.dmLevel = wave
writer.dmLevel = frames
frameSize = \\cm[frameSize{0.0250}:frame size in seconds]
frameStep = \\cm[frameStep{0.010}:frame step in seconds]
frameMode = fixed
frameCenterSpecial = left
[win:cWindower]
reader.dmLevel = frames
writer.dmLevel = winframes
winFunc = ham
gain = 1.0
offset = 0
[fft:cTransformFFT]
reader.dmLevel = winframes
writer.dmLevel = fft
[mag:cFFTmagphase]
reader.dmLevel = fft
writer.dmLevel = lld
dBpsd = \\cm[dB{0}:dB power spectral density]
[out:cHtkSink]
reader.dmLevel = lld
filename = \\cm[output(O){?}:output]
parmKind = 9
[csv:cCsvSink]
reader.dmLevel = lld
filename = \\cm[csvoutput{?}:CSV output]
instanceName = \\cm[instname(N){unknown}:instance name]
timestamp = 1
number = 0
printHeader = 1
"""
# edits of the text: {text: replacement}; the first five are the fixture's forms and its zeroPadSymmetric = 0 copy
TEXT_EDITS = {"norm": {"writer.dmLevel = lld\n": "writer.dmLevel = lld\nnormalise = 1\n"},
              "pow": {"writer.dmLevel = lld\n": "writer.dmLevel = lld\npower = 1\n"},
              "normpow": {"writer.dmLevel = lld\n": "writer.dmLevel = lld\nnormalise = 1\npower = 1\n"},
              "zps0": {"writer.dmLevel = fft\n": "writer.dmLevel = fft\nzeroPadSymmetric = 0\n"}}


def minimal_text(edits=None):
    text = MINIMAL
    for a, b in (edits or {}).items():
        assert text.count(a) == 1, a
        text = text.replace(a, b)
    return text
