"""The g++ build of opensmile_amd/csrc/lld_tonefilt_ops.hpp, lld_sincos_d.hpp and tonefilt_tables.cpp
(tests/helpers/tonefilt_check.cpp), loaded through ctypes: cTonefilt's tables and rows on the host with the C library's sin / cos,
the reference the chroma_filt tests and the fixture generator share."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
SHIPPED = dict(n_notes=72, first_note=55.0, decay_f0=0.9999, decay_fn=0.999, output_period=0.01)     # [tonefilt:cTonefilt] of chroma_filt.conf
RATES = (8000, 11025, 16000, 22050, 32000, 44100, 48000)
_lib = None


def load():
    global _lib
    if _lib is not None:
        return _lib
    csrc = os.path.join(ROOT, "opensmile_amd", "csrc")
    src = [os.path.join(ROOT, "tests", "helpers", "tonefilt_check.cpp"), os.path.join(csrc, "tonefilt_tables.cpp")]
    so = os.path.join(ROOT, "tests", "helpers", "_tonefilt_check.so")
    deps = src + [os.path.join(csrc, h) for h in ("lld_tonefilt_ops.hpp", "lld_sincos_d.hpp", "tonefilt_tables.hpp", "glibc_float.hpp")]
    deps.append(os.path.join(ROOT, "include", "smilehip.h"))
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(p) for p in deps):
        tmp = so + ".%d.new" % os.getpid()
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-o", tmp] + src + ["-lm"], check=True)
        os.replace(tmp, so)
    L = C.CDLL(so)
    L.tonefilt_block_len.restype = C.c_int64
    L.tonefilt_block_len.argtypes = [C.c_double, C.c_double]
    L.tonefilt_rows_of.restype = C.c_int64
    L.tonefilt_rows_of.argtypes = [C.c_int64, C.c_int64]
    L.tonefilt_domain.restype = C.c_double
    opts = [C.c_int, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double]
    L.tonefilt_tables.restype = C.c_int
    L.tonefilt_tables.argtypes = opts + [C.c_void_p] * 4
    L.tonefilt_blocks.restype = C.c_int
    L.tonefilt_blocks.argtypes = opts + [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_uint64]
    L.tonefilt_sincos_check.restype = None
    L.tonefilt_sincos_check.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.tonefilt_sincos_err.restype = None
    L.tonefilt_sincos_err.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    _lib = L
    return L


def _opts(o, fs):
    o = dict(SHIPPED, **(o or {}))
    return [int(o["n_notes"]), float(o["first_note"]), float(o["decay_f0"]), float(o["decay_fn"]), float(o["output_period"]), float(fs)]


def block_len(fs, output_period=0.01):
    return int(load().tonefilt_block_len(float(fs), float(output_period)))


def tables(fs, opts=None):
    L = load()
    o = _opts(opts, fs)
    n = L.tonefilt_tables(*o, None, None, None, None)
    assert n > 0, n
    P = C.c_int64()
    t = dict(freq=np.zeros(n), decay=np.zeros(n), w=np.zeros(n))
    assert L.tonefilt_tables(*o, C.addressof(P), t["freq"].ctypes.data, t["decay"].ctypes.data, t["w"].ctypes.data) == n
    t["P"] = int(P.value)
    return t


def pcm_float(pcm):
    """smilePcm_convertSamples for 16-bit input: (float)s / 32767.0f"""
    pcm = np.asarray(pcm)
    return pcm.astype(np.float32) if pcm.dtype == np.float32 else (pcm.astype(np.float32) / np.float32(32767.0)).astype(np.float32)


def rows_of(n, P):
    return int(load().tonefilt_rows_of(int(n), int(P)))


def padded(pcm, fs, opts=None):
    """the samples cTonefilt filters: the input, and its last sample repeated up to a whole number of blocks (the reader's padding of
    the last block at the end of input)"""
    pcm = np.asarray(pcm)
    P = tables(fs, opts)["P"]
    r = (-len(pcm)) % P
    return np.concatenate([pcm, np.full(r, pcm[-1], pcm.dtype)]) if len(pcm) and r else pcm


def tonespec_rows(pcm, fs, opts=None, mode=0, seed=1, state=None, pos=0):
    """samples -> (rows of notes, s, c): whole blocks only; mode 0 libm, 1 libm moved one ulp with seeded signs, 2 sincos_d"""
    L = load()
    o = _opts(opts, fs)
    P = tables(fs, opts)["P"]
    x = np.ascontiguousarray(pcm_float(pcm))
    nb = len(x) // P
    n = max(o[0], 1)
    s, c = (np.zeros(n), np.zeros(n)) if state is None else (np.array(state[0], np.float64), np.array(state[1], np.float64))
    ts = np.zeros((nb, n), np.float32)
    assert L.tonefilt_blocks(*o, x.ctypes.data, nb, pos, s.ctypes.data, c.ctypes.data, ts.ctypes.data, mode, seed) == n
    return ts, s, c


def sincos_check(x):
    """sincos_d of the host build on x: (s, c, largest ulp errors (sin, cos) against sinl / cosl, where)"""
    L = load()
    x = np.ascontiguousarray(x, np.float64)
    s, c, err, at = np.zeros(len(x)), np.zeros(len(x)), np.zeros(2), np.zeros(2)
    L.tonefilt_sincos_check(x.ctypes.data, len(x), s.ctypes.data, c.ctypes.data, err.ctypes.data, at.ctypes.data)
    return s, c, err, at


def sincos_err(x, s, c):
    """largest ulp errors (sin, cos) of given values against sinl / cosl, and where"""
    L = load()
    x, s, c = (np.ascontiguousarray(a, np.float64) for a in (x, s, c))
    err, at = np.zeros(2), np.zeros(2)
    L.tonefilt_sincos_err(x.ctypes.data, s.ctypes.data, c.ctypes.data, len(x), err.ctypes.data, at.ctypes.data)
    return err, at
