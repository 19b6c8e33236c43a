"""Every per-component operator of include/smilehip.h (tests/helpers/op_layouts.py holds one entry per entry point and option set)
held to its strided-row contract, on the device:

  test_strided_equals_packed                 odd leading dimensions with poisoned pads (NaN, then 1e30) give the packed call's bits,
                                             nothing outside a row's width is written and no cell inside it is left out
  test_row_does_not_depend_on_frame_count    a call with the first n frames gives rows [0, n) of the largest call -- n around the
                                             1 - 3 / >= 4 frames per block, 64-frame workgroup and wave forms; the operators that
                                             carry state: uneven pieces with the state carried against one call
  test_packed_equals_reference               the largest call against the entry's CPU reference, bit for bit except where the
                                             operator's own test documents an allowance (imported from there)

Source and destination are padded() buffers: a guard row either side, row 0 one float past a 16-byte boundary, the destination
pre-filled with a NaN no kernel produces. Every call stays inside them."""
import zlib

import numpy as np
import pytest

from helpers import op_layouts as OL

pytestmark = pytest.mark.gpu

N_STRIDED = 37
COUNTS = (1, 2, 3, 4, 5, 63, 64, 65)
PIECES = (1, 3, 60, 64, 1)


@pytest.fixture(scope="module")
def env():
    return OL.Env()


def rows_in(entry, n):
    return entry.make(np.random.default_rng(zlib.crc32(entry.name.encode())), n)


_base = {}


def base_call(env, entry):
    """the largest packed call of an entry, made once for the two tests that need it"""
    if entry.name not in _base:
        x = rows_in(entry, entry.base_rows)
        _base[entry.name] = (x,) + call(env, entry, x, entry.base_rows, *entry.widths)
    return _base[entry.name]


def call(env, entry, x, n, ld_src, ld_dst, src_poison=float("nan"), pieces=None):
    """n frames of x through the operator in one call (or piece by piece with the state carried) with these leading dimensions;
    (rows as uint32 [written, w_dst], the destination buffer, rows written, further outputs)"""
    w_src, w_dst = entry.widths
    pre = entry.halo[0]
    if entry.dst_fixed:
        ld_dst = w_dst
    lead_d = 0 if entry.dst_fixed else None
    if entry.src_flat:                                        # one row of samples between two guard rows, no stride
        ld_src = x.shape[1]
        src, _ = OL.padded(x, ld_src, src_poison)
    else:
        src, _ = OL.padded(x[:, :w_src], ld_src, src_poison)
    dst, _ = OL.padded(np.zeros((n, 0), np.float32), ld_dst, OL.SENTINEL, lead=lead_d)
    d_src, d_dst = env.dev(src), env.dev(dst)
    s_ptr = d_src.data_ptr() + 4 * (OL.first_row_offset(ld_src) + pre * ld_src)
    d_ptr = d_dst.data_ptr() + 4 * OL.first_row_offset(ld_dst, lead_d)
    state = entry.new_state(env) if entry.new_state else None
    extras, t_src, t_dst = {}, 0, 0
    for m in (pieces or [n]):
        more = entry.run(env, entry.take(x[t_src:], m), ld_src, ld_dst, s_ptr + 4 * t_src * ld_src, d_ptr + 4 * t_dst * ld_dst, m, state)
        for k, v in (more or {}).items():
            extras[k] = np.concatenate([extras[k], v]) if k in extras else v
        t_dst += entry.rows_written(m, t_src == 0) if entry.rows_written else m
        t_src += m
    assert t_src == n
    env.sync()
    out = d_dst.cpu().numpy()
    assert np.array_equal(d_src.cpu().numpy().view(np.uint32), src.view(np.uint32)), f"{entry.name} wrote into its source"
    return OL.unpadded(out, ld_dst, w_dst, n, lead=lead_d)[:t_dst], out, t_dst, extras


def same_extras(a, b, rows, what):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(a[k][:rows], b[k][:rows]), f"{what}: output {k} differs"


@pytest.mark.parametrize("entry", OL.REGISTRY, ids=lambda e: e.name)
def test_strided_equals_packed(env, entry):
    w_src, w_dst = entry.widths
    n = N_STRIDED
    x = rows_in(entry, n)
    packed, buf, wrote, ex = call(env, entry, x, n, w_src, w_dst)
    lead = 0 if entry.dst_fixed else None
    OL.check_layout(buf, w_dst, w_dst, n, packed, OL.SENTINEL, lead=lead, rows_written=wrote)
    for poison in (float("nan"), 1e30):
        ld_dst = w_dst if entry.dst_fixed else w_dst + 5
        got, buf, wrote2, ex2 = call(env, entry, x, n, w_src + 3, ld_dst, poison)
        assert wrote2 == wrote
        OL.check_layout(buf, ld_dst, w_dst, n, packed, OL.SENTINEL, lead=lead, rows_written=wrote)
        assert np.array_equal(got, packed)
        same_extras(ex, ex2, n, f"source pad {poison}")


@pytest.mark.parametrize("entry", OL.REGISTRY, ids=lambda e: e.name)
def test_row_does_not_depend_on_frame_count(env, entry):
    w_src, w_dst = entry.widths
    x, base, _, wrote, ex = base_call(env, entry)
    assert wrote == (entry.rows_written(entry.base_rows, True) if entry.rows_written else entry.base_rows)
    if entry.stateful:
        assert sum(PIECES) == entry.base_rows
        got, _, wrote2, ex2 = call(env, entry, x, entry.base_rows, w_src, w_dst, pieces=PIECES)
        assert wrote2 == wrote
        diff = np.argwhere(got != base)
        assert not len(diff), f"pieces {PIECES} with the state carried: {len(diff)} cells differ from one call, first at {diff[0].tolist()}"
        same_extras(ex, ex2, entry.base_rows, f"pieces {PIECES}")
        return
    for n in COUNTS:
        got, _, wrote_n, ex_n = call(env, entry, entry.take(x, n), n, w_src, w_dst)
        diff = np.argwhere(got != base[:wrote_n])
        assert not len(diff), f"a call of {n} frames: {len(diff)} cells differ from the rows of the {entry.base_rows}-frame call, first at {diff[0].tolist()}"
        same_extras(ex_n, ex, n, f"a call of {n} frames")


@pytest.mark.parametrize("entry", OL.REGISTRY, ids=lambda e: e.name)
def test_packed_equals_reference(env, entry, oracle):
    x, base, _, wrote, ex = base_call(env, entry)
    ref = entry.reference(x)
    ref_extra = None
    if isinstance(ref, tuple):
        ref, ref_extra = ref
    assert len(ref) == wrote
    OL.compare(entry, base, ref, ex, ref_extra)


# (entries whose entry point checks both leading dimensions against the widths the registry declares)
REFUSED = ("preemphasis_de0", "rfft_512", "fftmag", "melspec", "mfcc", "plp_cc", "spectral_K257", "window_op_block_op1", "specresample",
           "lsp_p8", "vecop_add", "formantlpc_frames")


@pytest.mark.parametrize("entry", [e for e in OL.REGISTRY if e.name in REFUSED], ids=lambda e: e.name)
def test_leading_dimension_below_the_width_is_refused(env, entry):
    """SMILEHIP_ERR_INVALID before any launch: the destination keeps its sentinel"""
    w_src, w_dst = entry.widths
    x = rows_in(entry, 4)
    for ld_src, ld_dst in ((w_src - 1, w_dst), (w_src, w_dst - 1)):
        if min(ld_src, ld_dst) < 1:
            continue
        src, _ = OL.padded(x[:, :w_src], w_src, float("nan"))
        dst, _ = OL.padded(np.zeros((4, 0), np.float32), w_dst, OL.SENTINEL)
        d_src, d_dst = env.dev(src), env.dev(dst)
        state = entry.new_state(env) if entry.new_state else None
        with pytest.raises(env.capi.SmileHipError, match="error -1"):
            entry.run(env, x, ld_src, ld_dst, d_src.data_ptr() + 4 * (OL.first_row_offset(w_src) + entry.halo[0] * w_src),
                      d_dst.data_ptr() + 4 * OL.first_row_offset(w_dst), 4, state)
        env.sync()
        assert (d_dst.cpu().numpy().view(np.uint32) == OL.SENTINEL).all()


def test_functionals_matrix_strided_source(env):
    """The two matrix entry points of the functionals engine take a leading dimension on the source only (one output vector per
    matrix): a padded matrix (NaN, then 1e30 behind every row) gives the packed matrix's bits, and the output's guards stay."""
    import ctypes as C
    L, capi = env.L, env.capi
    rows, cols = 129, 5
    x = (np.random.default_rng(41).standard_normal((rows, cols)) * 2).astype(np.float32)
    x[:, 1] = 0.0
    x[:, 2] = np.round(x[:, 2])
    spec = capi.funcspec_compare16("A")
    per16, per = L.smilehip_functionals_count(0x1ffff), capi.funcspec_count(spec)
    assert per16 == 17 and per > 17

    def both(ld, poison):
        src, _ = OL.padded(x, ld, poison)
        d_src = env.dev(src)
        ptr = d_src.data_ptr() + 4 * OL.first_row_offset(ld)
        outs = []
        for n_out, fn in ((cols * per16, lambda d: L.smilehip_functionals_matrix(env.h, ptr, ld, rows, cols, 0x1ffff, d, None)),
                          (cols * per, lambda d: L.smilehip_funcspec_matrix(env.h, C.byref(spec), ptr, ld, rows, cols, d, None))):
            dst, _ = OL.padded(np.zeros((1, 0), np.float32), n_out, OL.SENTINEL, lead=0)
            d_dst = env.dev(dst)
            env.check(fn(d_dst.data_ptr() + 4 * n_out))
            env.sync()
            out = d_dst.cpu().numpy()
            OL.check_layout(out, n_out, n_out, 1, OL.unpadded(out, n_out, n_out, 1, lead=0), OL.SENTINEL, lead=0)
            outs.append(OL.unpadded(out, n_out, n_out, 1, lead=0))
        return outs
    packed = both(cols, float("nan"))
    assert all(np.unique(p).size > cols for p in packed)
    for poison in (float("nan"), 1e30):
        for a, b in zip(both(cols + 3, poison), packed):
            assert np.array_equal(a, b), f"source pad {poison}"


def test_carried_state_of_the_operators_without_a_leading_dimension(env):
    """smilehip_pitchacf_contour_frames (8 words of state, zeroed before the first frame) and smilehip_window_op_row_ex kind 3
    (onlyInSegments: the divisor in d_norm_io) take one value per frame, so they are not in the registry: their frames in the
    pieces of the registry's stateful operators give one call's bits, kind 3 also the restatement's."""
    L, torch = env.L, env.torch
    n = sum(PIECES)
    rng = np.random.default_rng(43)
    voicing = np.where(rng.random(n) < 0.3, rng.uniform(0.0, 0.5, n), rng.uniform(0.55, 1.0, n))
    idx = np.where(rng.random(n) < 0.2, 0, rng.integers(20, 200, n)).astype(np.int32)
    d_v, d_i = env.dev(voicing), env.dev(idx)

    def contour(pieces):
        state = torch.zeros(8, dtype=torch.float32, device="cuda")
        out = env.dev(OL.padded(np.zeros((n, 0), np.float32), 4, OL.SENTINEL, lead=0)[0])
        t = 0
        for m in pieces:
            env.check(L.smilehip_pitchacf_contour_frames(env.h, d_v.data_ptr() + 8 * t, d_i.data_ptr() + 4 * t, OL.PITCH_FS_SEC / 512.0, 0.55,
                                                         state.data_ptr(), out.data_ptr() + 16 * (1 + t), m, None))
            t += m
        env.sync()
        return out.cpu().numpy()
    one = contour([n])
    rows = OL.unpadded(one, 4, 4, n, lead=0)
    OL.check_layout(one, 4, 4, n, rows, OL.SENTINEL, lead=0)
    assert np.unique(rows[:, 0]).size > 10
    assert np.array_equal(contour(PIECES).view(np.uint32), one.view(np.uint32))

    W, pre = 2, 2
    x = (rng.standard_normal(n + pre + W) * 0.5).astype(np.float32)
    x[rng.random(len(x)) < 0.25] = 0.0
    d_x = env.dev(x)

    def delta_segments(pieces):
        norm = torch.tensor([float(OL.delta_norm(W))], dtype=torch.float32, device="cuda")
        out = env.dev(OL.padded(np.zeros((1, 0), np.float32), n, OL.SENTINEL, lead=0)[0])
        t = 0
        for m in pieces:
            env.check(L.smilehip_window_op_row_ex(env.h, d_x.data_ptr() + 4 * (pre + t), out.data_ptr() + 4 * (n + t), m, 3, W, norm.data_ptr(), None))
            t += m
        env.sync()
        return out.cpu().numpy(), norm.cpu().numpy()
    one, norm1 = delta_segments([n])
    ref, norm_ref = OL._delta_ref()(x, pre, n, W, 8, OL.delta_norm(W))
    OL.check_layout(one, n, n, 1, ref.view(np.uint32), OL.SENTINEL, lead=0)
    assert norm1.view(np.uint32)[0] == np.array([norm_ref], np.float32).view(np.uint32)[0]
    more, norm2 = delta_segments(PIECES)
    assert np.array_equal(more.view(np.uint32), one.view(np.uint32)) and np.array_equal(norm2.view(np.uint32), norm1.view(np.uint32))
