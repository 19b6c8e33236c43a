"""Registry entries (helpers/op_layouts.py) of the two operators of config/chroma/chroma_fft.conf, smilehip_tonespec_op_frames and
smilehip_chroma_op_frames, with the file's own options on the 257-bin level. The reference is the g++ build of the operators' own row
functions and tables (helpers/chroma_host.py), which tests/test_chroma_fft_host.py holds to the real binary's levels bit for bit.
The package's __init__ imports this module behind op_layouts, so whoever reads the registry finds the entries in it."""
import ctypes as C

from . import chroma_host
from . import op_layouts as OL


def _run(which):
    def run(env, x, ls, ld, s, d, n, st):
        def make():
            h = C.c_void_p()
            if which == "tonespec":
                env.check(env.L.smilehip_tonespec_op_create(env.h, C.byref(env.capi.tonespec_opts()), OL.K, OL.FSS_512, C.byref(h)))
                assert env.L.smilehip_tonespec_op_n_out(h) == 72
            else:
                env.check(env.L.smilehip_chroma_op_create(env.h, C.byref(env.capi.chroma_opts()), 72, C.byref(h)))
            return h
        fn = env.L.smilehip_tonespec_op_frames if which == "tonespec" else env.L.smilehip_chroma_op_frames
        env.check(fn(env.keep(("chroma_ops", which), make), s, ls, d, ld, n, None))
    return run


def ref_tonespec_op(x):
    return chroma_host.tonespec_rows(x, OL.FSS_512)


def ref_chroma_op(x):
    return chroma_host.chroma_rows(x)


OL.op("tonespec_op", "tonespec_op_frames", lambda rng, n: OL.magnitudes(rng, n, OL.K, 13.0), _run("tonespec"), (OL.K, 72), ref_tonespec_op,
      kind="restatement")
OL.op("chroma_op", "chroma_op_frames", lambda rng, n: ref_tonespec_op(OL.magnitudes(rng, n, OL.K, 13.0)), _run("chroma"), (72, 12), ref_chroma_op,
      kind="restatement")
