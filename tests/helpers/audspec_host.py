"""The g++ build of opensmile_amd/csrc/lld_audspec_ops.hpp (tests/helpers/audspec_check.cpp, linked to the library for its table
builders), loaded through ctypes:
cMelspec's rows and cPlp's auditory-spectrum rows on the host, the reference of the audspec tests, and what they share: the fixture,
its inputs, the minimal configuration text of the edited copies and the config struct of each."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
GOLDEN = os.path.join(ROOT, "tests", "golden")
RATES = (8000, 11025, 16000, 22050, 32000, 44100, 48000)
NFFT = {8000: 256, 11025: 512, 16000: 512, 22050: 1024, 32000: 1024, 44100: 2048, 48000: 2048}   # 25 ms frames zero-padded to a power of two
_lib = None
_fix = {}


def load():
    global _lib
    if _lib is not None:
        return _lib
    csrc = os.path.join(ROOT, "opensmile_amd", "csrc")
    src = [os.path.join(ROOT, "tests", "helpers", "audspec_check.cpp")]
    pkg = os.path.join(ROOT, "opensmile_amd")              # make_geometry / make_mel: the library's own (tables.cpp), found beside the package
    so = os.path.join(ROOT, "tests", "helpers", "_audspec_check.so")
    deps = src + [os.path.join(csrc, h) for h in ("lld_audspec_ops.hpp", "tables.hpp", "glibc_float.hpp")] + [os.path.join(ROOT, "include", "smilehip.h"),
                                                                                                                     os.path.join(pkg, "libsmilehip.so")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(p) for p in deps):
        tmp = so + ".%d.new" % os.getpid()
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-o", tmp] + src +
                       ["-L" + pkg, "-lsmilehip", "-Wl,-rpath," + pkg, "-lm"], check=True)
        os.replace(tmp, so)
    L = C.CDLL(so)
    L.audspec_rows_of.restype = C.c_int64
    L.audspec_rows_of.argtypes = [C.c_int64, C.c_int64, C.c_int64]
    L.audspec_geometry.restype = C.c_int
    L.audspec_geometry.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.audspec_mel_rows.restype = C.c_int
    L.audspec_mel_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p]
    L.audspec_aud_rows.restype = C.c_int
    L.audspec_aud_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    L.audspec_frame_samples.restype = None
    L.audspec_frame_samples.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_float, C.c_float, C.c_void_p]
    _lib = L
    return L


def fixture(name="audspec_synth.npz"):
    if name not in _fix:
        _fix[name] = np.load(os.path.join(GOLDEN, name))
    return _fix[name]


def cut(idx, n, div=1):
    """the samples of a fixture input (make_golden_audspec.py: cut)"""
    from opensmile_amd import synth
    if not n:
        return np.zeros(0, np.int16)
    if idx < 0:
        return np.zeros(n, np.int16)
    return (synth.utterance(int(idx), int(n)).astype(np.int32) // int(div)).astype(np.int16)


def input_pcm(k):
    idx, n, fs, div = (int(v) for v in fixture()["inputs"][k])
    return cut(idx, n, div), fs


# the edited copies of the fixture as changes of the config struct (what the walker must make of the edited text) ...
EDITS = {"nb20": dict(n_bands=20), "nb40": dict(n_bands=40), "lohi": dict(lofreq=100.0, hifreq=4000.0), "comp05": dict(plp_compression=0.5),
         "dw3": dict(delta_win=3), "d1": dict(n_delta=1), "d0": dict(n_delta=0), "fs32": dict(frame_size_sec=0.032),
         "han": dict(win_func=1), "inert": dict(plp_lp_order=8, first_mfcc=1, cep_lifter=0.0)}
# ... and of the minimal text below: {text: replacement}
TEXT_EDITS = {"nb20": {"nBands = 26": "nBands = 20"}, "nb40": {"nBands = 26": "nBands = 40"},
              "lohi": {"lofreq = 0": "lofreq = 100", "hifreq = 8000": "hifreq = 4000"}, "comp05": {"compression = 0.33": "compression = 0.5"},
              "dw3": {"deltawin = 2": "deltawin = 3"}, "d1": {"reader.dmLevel = plp;plpde;plpdede": "reader.dmLevel = plp;plpde"},
              "d0": {"reader.dmLevel = plp;plpde;plpdede": "reader.dmLevel = plp"}, "fs32": {"frameSize = 0.025": "frameSize = 0.032"},
              "han": {"winFunc = ham": "winFunc = han"},
              "inert": {"lpOrder = 5": "lpOrder = 8", "firstCC = 0": "firstCC = 1", "cepLifter = 22": "cepLifter = 0"}}
EDIT_INPUTS = (6, 9)                                       # T = 5 (with fftmag) and T = 20

# a configuration text of the project's own with the graph of config/audspec/audspec.conf (no text of the reference's file)
MINIMAL = """[componentInstances:cComponentManager]
instance[dataMemory].type = cDataMemory
instance[src].type = cWaveSource
instance[fr].type = cFramer
instance[pe].type = cVectorPreemphasis
instance[win].type = cWindower
instance[fft].type = cTransformFFT
instance[mag].type = cFFTmagphase
instance[mel].type = cMelspec
instance[aud].type = cPlp
instance[de].type = cDeltaRegression
instance[dede].type = cDeltaRegression
instance[cat].type = cVectorConcat
instance[out].type = cHtkSink
[src:cWaveSource]
writer.dmLevel = wave
filename = \\cm[inputfile(I){in.wav}:input]
monoMixdown = 1
[fr:cFramer]
reader.dmLevel = wave
writer.dmLevel = frames
frameSize = 0.025
frameStep = 0.010
frameCenterSpecial = left
[pe:cVectorPreemphasis]
reader.dmLevel = frames
writer.dmLevel = framespe
k = 0.97
de = 0
[win:cWindower]
reader.dmLevel = framespe
writer.dmLevel = winframes
winFunc = ham
gain = 1.0
offset = 0
[fft:cTransformFFT]
reader.dmLevel = winframes
writer.dmLevel = fft
[mag:cFFTmagphase]
reader.dmLevel = fft
writer.dmLevel = fftmag
[mel:cMelspec]
reader.dmLevel = fftmag
writer.dmLevel = melspec
htkcompatible = 1
nBands = 26
usePower = 1
lofreq = 0
hifreq = 8000
[aud:cPlp]
reader.dmLevel = melspec
writer.dmLevel = plp
firstCC = 0
lpOrder = 5
cepLifter = 22
compression = 0.33
htkcompatible = 1
doIDFT = 0
doLpToCeps = 0
doLP = 0
doInvLog = 0
doAud = 1
doLog = 0
[de:cDeltaRegression]
reader.dmLevel = plp
writer.dmLevel = plpde
deltawin = 2
[dede:cDeltaRegression]
reader.dmLevel = plpde
writer.dmLevel = plpdede
deltawin = 2
[cat:cVectorConcat]
reader.dmLevel = plp;plpde;plpdede
writer.dmLevel = lld
[out:cHtkSink]
reader.dmLevel = lld
filename = \\cm[output(O){out.htk}:output]
parmKind = 9
"""


def minimal_text(edits=None):
    text = MINIMAL
    for a, b in (edits or {}).items():
        assert text.count(a) >= 1, a
        text = text.replace(a, b)
    return text


def config(fs=16000.0, compat=False, **fields):
    from opensmile_amd import capi
    c = capi.audspec_config(fs, compat)
    for k, v in fields.items():
        setattr(c, k, v)
    return c


def geometry(cfg):
    """(N, H, Nfft, K, n_bands, eql[n_bands]) of this build's tables"""
    L = load()
    geo = np.zeros(4, np.int64)
    eql = np.zeros(64, np.float32)
    nb = L.audspec_geometry(C.addressof(cfg), geo.ctypes.data, eql.ctypes.data)
    assert nb > 0, nb
    return int(geo[0]), int(geo[1]), int(geo[2]), int(geo[3]), nb, eql[:nb].copy()


def mel_rows(cfg, mag):
    """rows of magnitudes -> rows of mel bands (audspec::mel_row on this build's tables)"""
    L = load()
    mag = np.ascontiguousarray(mag, np.float32)
    out = np.zeros((len(mag), cfg.n_bands), np.float32)
    assert L.audspec_mel_rows(C.addressof(cfg), mag.ctypes.data, len(mag), mag.shape[1], out.ctypes.data) == cfg.n_bands
    return out


def aud_rows(cfg, mel):
    """rows of mel bands -> rows of the auditory spectrum (audspec::aud_row)"""
    L = load()
    mel = np.ascontiguousarray(mel, np.float32)
    out = np.zeros_like(mel)
    assert L.audspec_aud_rows(C.addressof(cfg), mel.ctypes.data, len(mel), out.ctypes.data) == mel.shape[1]
    return out


def lld_rows(aud, n_delta, delta_win):
    """static | de | de_de from the static level: the oracle's tick-accurate regression chain (lldo.delta_chain)"""
    from oracle import lldo
    aud = np.ascontiguousarray(aud, np.float32)
    if n_delta == 0 or len(aud) == 0:
        return aud
    y = lldo.delta_chain(aud, delta_win, n_delta)
    return np.concatenate([aud] + [y[i] for i in range(n_delta)], axis=1)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)
