"""The g++ build of opensmile_amd/csrc/lld_chroma_ops.hpp and chroma_tables.cpp (tests/helpers/chroma_check.cpp), loaded through
ctypes: cTonespec's tables and rows and cChroma's rows on the host, the reference the chroma tests and the operator registry share."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
FILTER = {"gau": 0, "tri": 1, "trp": 2, "rec": 3}
SHIPPED = dict(n_octaves=6, first_note=55.0, filter_type="gau", use_power=1, dba=1)     # [tonespec:cTonespec] of chroma_fft.conf
_lib = None


def load():
    global _lib
    if _lib is not None:
        return _lib
    csrc = os.path.join(ROOT, "opensmile_amd", "csrc")
    src = [os.path.join(ROOT, "tests", "helpers", "chroma_check.cpp"), os.path.join(csrc, "chroma_tables.cpp")]
    so = os.path.join(ROOT, "tests", "helpers", "_chroma_check.so")
    deps = src + [os.path.join(csrc, h) for h in ("lld_chroma_ops.hpp", "chroma_tables.hpp", "glibc_float.hpp")] + [os.path.join(ROOT, "include", "smilehip.h")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(p) for p in deps):
        tmp = so + ".%d.new" % os.getpid()
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-o", tmp] + src + ["-lm"], check=True)
        os.replace(tmp, so)
    L = C.CDLL(so)
    L.chroma_rows_of.restype = C.c_int64
    L.chroma_rows_of.argtypes = [C.c_int64, C.c_int64, C.c_int64]
    opts = [C.c_int, C.c_float, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_double]
    L.chroma_tables.restype = C.c_int
    L.chroma_tables.argtypes = opts + [C.c_void_p] * 6
    L.chroma_tonespec_rows.restype = C.c_int
    L.chroma_tonespec_rows.argtypes = opts + [C.c_void_p, C.c_int64, C.c_void_p]
    L.chroma_chroma_rows.restype = None
    L.chroma_chroma_rows.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_float, C.c_void_p]
    _lib = L
    return L


def _opts(o):
    o = dict(SHIPPED, **(o or {}))
    ft = o["filter_type"]
    return [int(o["n_octaves"]), float(o["first_note"]), FILTER[ft] if isinstance(ft, str) else int(ft), int(o["use_power"]), int(o["dba"])]


def frame_size_sec(fs, frame_sec=0.064):
    """frameSizeSec of the magnitude level: cTransformFFT scales the framer's by Nfft / N in double (transformFft.cpp:68-94)"""
    N = int(np.floor(frame_sec * fs + 0.5))
    nfft = 1 << (N - 1).bit_length()
    return frame_sec * (float(nfft) / float(N)) if nfft != N else frame_sec


def tables(n_src, fss, opts=None):
    L = load()
    o = _opts(opts)
    n = L.chroma_tables(*o, n_src, fss, None, None, None, None, None, None)
    assert n > 0, n
    t = dict(pitch_class_freq=np.zeros(n + 2, np.float32), bin_key=np.zeros(n_src, np.int32), nbins=np.zeros(n + 2, np.int32),
             filter_map=np.zeros(n_src, np.float32), note_rec=np.zeros((n, 4), np.int32), first_last=np.zeros(2, np.int32))
    assert L.chroma_tables(*o, n_src, fss, *(t[k].ctypes.data for k in ("pitch_class_freq", "bin_key", "nbins", "filter_map", "note_rec",
                                                                            "first_last"))) == n
    return t


def tonespec_rows(mag, fss, opts=None):
    """rows of magnitudes -> rows of notes (chroma::tonespec_row on this build's tables)"""
    L = load()
    mag = np.ascontiguousarray(mag, np.float32)
    o = _opts(opts)
    out = np.zeros((len(mag), 12 * o[0]), np.float32)
    assert L.chroma_tonespec_rows(*o, mag.shape[1], fss, mag.ctypes.data, len(mag), out.ctypes.data) == out.shape[1]
    return out


def chroma_rows(ts, octave_size=12, sil_thresh=0.001):
    """rows of notes -> rows of classes (chroma::chroma_row)"""
    L = load()
    ts = np.ascontiguousarray(ts, np.float32)
    out = np.zeros((len(ts), octave_size), np.float32)
    L.chroma_chroma_rows(ts.ctypes.data, len(ts), ts.shape[1], octave_size, sil_thresh, out.ctypes.data)
    return out
