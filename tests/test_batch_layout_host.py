"""opensmile_amd/csrc/batch_layout.hpp -- what a batch of packed utterances is, as host index arithmetic -- compiled for the HOST
(tests/helpers/batch_layout_check.cpp) and run on ragged offset lists for every chain kind: frames against smilehip_num_frames of a
host-only plan, the row rules of the chains, and every work list (tiles, delta tiles, runs, jitter items, the delta-fused fast
kernel's tiles) covering every frame / row of every utterance exactly once. No device: smilehip_batch_create uploads exactly
these vectors, and the GPU tests show what the kernels make of them."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from opensmile_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "opensmile_amd", "csrc")
NAMES = ("samp_off", "frame_off", "row_off", "fin_off", "short_utts", "scalars", "tile_utt", "tile_t0", "dtile_utt", "dtile_t0",
         "run_utt", "run_t0", "jit_utt", "jit_t0", "frame_utt", "tile_rec", "ftiles")
FAST_SLOTS = 256 * 8 * 8       # smilehip_batch_create passes max(1, blocks of the fast kernel) * 8; any positive value is a valid spec


def _constant(unit, name):
    """`constexpr int NAME = VALUE;` of a .hip unit: the constants smilehip_batch_create passes in are owned by the kernels' files"""
    m = re.search(r"constexpr int %s = (\d+);" % name, open(os.path.join(CSRC, unit)).read())
    assert m, (unit, name)
    return int(m.group(1))


SHORT_T = _constant("lld_kernels.hip", "kShortMaxT")           # chain_short_max(): utterances of <= 16 frames are lld_chain_short's
DTILE_ROWS = _constant("lld_kernels.hip", "kChainTile")        # chain_tile_rows(): rows per tile of the window chain
FAST_TILE = _constant("lld_mfcc512.hip", "kTileFrames")        # fast512_tile_frames(): frames per wave tile of the fast kernel
F0_TILE = _constant("lld_f0.hip", "kTileFrames")               # f0_tile_frames(): frames per work item of the F0 frame kernels
JIT_CHUNK = _constant("lld_jitter.hip", "kJitChunk")           # jitter_chunk_frames(): frames per cPitchJitter work item
NO_TILING = 1 << 40                                            # every other chain: one tile per utterance (smilehip_batch_create)

CHAINS = {   # chain kind -> (config, fast kernel and fused deltas as smilehip_batch_create would find them on a device)
    "mfcc": (capi.mfcc12_0_d_a_config, True),
    "mfcc_generic": (capi.mfcc12_0_d_a_config, False),
    "plp": (capi.plp_0_d_a_config, True),
    "is09": (capi.is09_lld_config, False),
    "compare_ab": (capi.compare16_ab_config, False),
    "compare_f0": (capi.compare16_f0_config, False),
    "compare": (capi.compare16_config, False),
    "egemaps": (capi.egemapsv02_config, False),
}
KIND_IS09, KIND_F0, KIND_EGEMAPS = 1, 4, 6                     # include/smilehip.h: SMILEHIP_CHAIN_IS09 / _COMPARE_F0 / _EGEMAPS
COMPARE_LIKE = (2, 5)                                          # SMILEHIP_CHAIN_COMPARE_AB / _COMPARE: the ComParE row rule


@pytest.fixture(scope="module")
def lib():
    src = os.path.join(ROOT, "tests", "helpers", "batch_layout_check.cpp")
    so = os.path.join(ROOT, "tests", "helpers", "_batch_layout_check.so")
    hdrs = [os.path.join(CSRC, h) for h in ("batch_layout.hpp", "lld_tile_rec.hpp")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(p) for p in [src] + hdrs):
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, src], check=True)
    L = C.CDLL(so)
    L.blc_run.restype = C.c_void_p
    L.blc_run.argtypes = [C.c_void_p, C.c_double, C.c_void_p, C.c_int32]
    L.blc_rc.argtypes = [C.c_void_p]
    L.blc_size.restype = C.c_int64
    L.blc_size.argtypes = [C.c_void_p, C.c_char_p]
    L.blc_copy.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p]
    L.blc_free.argtypes = [C.c_void_p]
    L.blc_compare_run_frames.argtypes = [C.c_int64]
    return L


class Chain:
    """A host-only plan of one chain kind and the spec smilehip_batch_create would fill from it."""

    def __init__(self, name):
        factory, fast = CHAINS[name]
        self.plan = capi.Plan(None, factory())
        cfg, g = self.plan.cfg, self.plan.geometry
        self.kind, self.fast = int(cfg.chain_kind), fast
        self.N, self.H = int(g.frame_size), int(g.frame_step)
        self.period = g.frame_period / g.frame_step
        self.N60 = int(round(0.060 / self.period))
        self.row_extra = int(cfg.sma_win) // 2 if self.kind == KIND_IS09 else 0     # plan_row_extra (smilehip_plan.cpp)
        self.tile_frames = FAST_TILE if fast else (F0_TILE if self.kind == KIND_F0 else NO_TILING)

    def layout(self, lib, off, run_frames_override=0):
        off = np.ascontiguousarray(off, np.int64)
        n_utt = max(len(off) - 1, 0)
        spec = np.array([self.kind, self.N, self.H, self.row_extra, int(self.fast), FAST_SLOTS, self.tile_frames, DTILE_ROWS,
                         SHORT_T, JIT_CHUNK, run_frames_override], np.int64)
        h = lib.blc_run(spec.ctypes.data, self.period, off.ctypes.data if n_utt else None, n_utt)
        try:
            rc = lib.blc_rc(h)
            out = {}
            for name in NAMES if rc == 0 else ():
                a = np.zeros(lib.blc_size(h, name.encode()), np.int64)
                lib.blc_copy(h, name.encode(), a.ctypes.data)
                out[name] = a
        finally:
            lib.blc_free(h)
        return rc, out

    def lengths(self):
        """Every length class the issue names, in samples: zero, shorter than a frame, exactly one frame, T == short_T and
        short_T + 1, a frame count that is not a multiple of four, around the 60 ms framer's first and fourth frame, and long."""
        N, H, N60 = self.N, self.H, self.N60
        T = lambda t, extra=0: N + (t - 1) * H + extra
        return [0, N - 1, N, T(SHORT_T), T(SHORT_T + 1, H - 1), T(37, 3), T(40), T(998), N60 - 1, N60, N60 + 2 * H, N60 + 3 * H, 1, T(2),
                T(2 * JIT_CHUNK + 5), T(DTILE_ROWS + 1)]


def offsets(lens, start=0):
    return np.concatenate([[start], start + np.cumsum(lens)]).astype(np.int64)


def cases(chain):
    """name -> offset list"""
    L = chain.lengths()
    rng = np.random.default_rng(20161016 + chain.kind)
    T = lambda t: chain.N + (t - 1) * chain.H
    return {
        "empty": np.zeros(0, np.int64),
        "one_empty_utt": offsets([0]),
        "classes": offsets(L),
        "classes_reversed_even": offsets([n & ~1 for n in L[::-1]]),
        "classes_odd_start": offsets(L, start=7),
        "odd_offsets_only_where_no_frames": offsets([3, 5, T(20) + 2, 1, 1, T(50)]),    # odd starts fall on frameless utterances
        "odd_offset_on_a_frame": offsets([T(20), 3, T(20)]),
        "short_T_and_next": offsets([T(SHORT_T), T(SHORT_T + 1), T(1), T(SHORT_T + 1), T(SHORT_T)]),
        "one_long": offsets([T(200003)]),
        "many_equal": offsets([T(998)] * 300),
        "random_even": offsets((rng.integers(0, 40000, 200) & ~1)),
        "random": offsets(rng.integers(0, 40000, 200), start=int(rng.integers(0, 1000))),
    }


def covers_once(utt, t0, count_of, step, what):
    """items (utt, t0) of `step` elements each: every element of every utterance exactly once, utterances and starts ascending"""
    seen = {}
    for u, t in zip(utt.tolist(), t0.tolist()):
        assert t % step == 0 and 0 <= t < count_of[u], (what, u, t)
        seen.setdefault(u, []).append(t)
    for u, n in enumerate(count_of.tolist()):
        assert seen.get(u, []) == list(range(0, n, step)), (what, u)
    assert np.all(np.diff(utt) >= 0), what


@pytest.mark.parametrize("name", list(CHAINS))
def test_layout_of_ragged_batches(lib, name):
    chain = Chain(name)
    for case, off in cases(chain).items():
        rc, L = chain.layout(lib, off)
        what = (name, case)
        assert rc == 0, what
        n_utt = max(len(off) - 1, 0)
        lens = np.diff(off) if n_utt else np.zeros(0, np.int64)
        starts = off[:-1] if n_utt else lens
        np.testing.assert_array_equal(L["samp_off"], off if n_utt else [0], err_msg=str(what))
        # frames: smilehip_num_frames of the host-only plan
        T = np.array([chain.plan.num_frames(int(n)) for n in lens], np.int64)
        np.testing.assert_array_equal(np.diff(L["frame_off"]), T, err_msg=str(what))
        assert L["frame_off"][0] == 0 and L["row_off"][0] == 0 and len(L["frame_off"]) == len(L["row_off"]) == n_utt + 1
        # rows: tests/test_gpu_compare.py (T60 + 1 rows, none below four 60 ms frames), tests/test_gpu_egemaps.py
        # test_row_counts_and_offsets (T60 + 1, 0 without a 60 ms frame), capi.py Batch.run_egemaps (fin_off: T20 + 1 where T60 >= 1)
        T60 = np.where(lens >= chain.N60, (lens - chain.N60) // chain.H + 1, 0)
        if chain.kind in COMPARE_LIKE:
            rows = np.where(T60 >= 4, T60 + 1, 0)
        elif chain.kind == KIND_EGEMAPS:
            rows = np.where(T60 >= 1, T60 + 1, 0)
        else:
            rows = np.where(T > 0, T + chain.row_extra, 0)
        np.testing.assert_array_equal(np.diff(L["row_off"]), rows, err_msg=str(what))
        if chain.kind == KIND_EGEMAPS:
            np.testing.assert_array_equal(np.diff(L["fin_off"]), np.where(T60 >= 1, T + 1, 0), err_msg=str(what))
            assert L["fin_off"][0] == 0 and len(L["fin_off"]) == n_utt + 1
        else:
            assert len(L["fin_off"]) == 0, what
        all_even, total_frames, total_rows, run_frames = L["scalars"].tolist()
        assert (total_frames, total_rows) == (T.sum(), rows.sum()), what
        np.testing.assert_array_equal(L["short_utts"], np.flatnonzero((T > 0) & (T <= SHORT_T)), err_msg=str(what))
        assert bool(all_even) == (not np.any((T > 0) & (starts % 2 == 1))), what
        # frame tiles and their resolved records
        covers_once(L["tile_utt"], L["tile_t0"], T, chain.tile_frames, what + ("tiles",))
        rec = L["tile_rec"].reshape(-1, 4)
        np.testing.assert_array_equal(rec[:, 0], off[L["tile_utt"]] + L["tile_t0"] * chain.H if n_utt else [], err_msg=str(what))
        np.testing.assert_array_equal(rec[:, 1], L["frame_off"][L["tile_utt"]] + L["tile_t0"], err_msg=str(what))
        np.testing.assert_array_equal(rec[:, 2], np.minimum(chain.tile_frames, T[L["tile_utt"]] - L["tile_t0"]), err_msg=str(what))
        assert not rec[:, 3].any(), what
        covers_once(L["dtile_utt"], L["dtile_t0"], rows, DTILE_ROWS, what + ("dtiles",))
        # 20 ms runs: the chains with a 20 ms frame kernel only
        if chain.kind in COMPARE_LIKE or chain.kind == KIND_EGEMAPS:
            assert run_frames == lib.blc_compare_run_frames(int(T.sum())), what
            covers_once(L["run_utt"], L["run_t0"], T, run_frames, what + ("runs",))
        else:
            assert len(L["run_utt"]) == len(L["run_t0"]) == 0, what
        # cPitchJitter's items: all first chunks, then all second chunks, ...
        if chain.kind == KIND_F0:
            want = [(u, t0) for t0 in range(0, int(T.max()) if n_utt else 0, JIT_CHUNK) for u in range(n_utt) if t0 < T[u]]
            assert list(zip(L["jit_utt"].tolist(), L["jit_t0"].tolist())) == want, what
        else:
            assert len(L["jit_utt"]) == len(L["jit_t0"]) == 0, what
        if chain.kind == KIND_IS09:
            np.testing.assert_array_equal(L["frame_utt"], np.repeat(np.arange(n_utt), T), err_msg=str(what))
        else:
            assert len(L["frame_utt"]) == 0, what
        check_fused_tiles(chain, L, off, T, bool(all_even), what)


def check_fused_tiles(chain, L, off, T, all_even, what):
    ft = L["ftiles"].reshape(-1, 8)
    if not (chain.fast and all_even and T.sum() > 0):
        assert len(ft) == 0, what
        return
    samp0, row0, n_frames, live_n, e0, e1, lo, delta_on = ft.T
    assert np.all(n_frames % 4 == 0) and np.all(n_frames > 0), what
    assert np.all(np.diff(n_frames) <= 0), what                      # longest first ...
    utt = np.searchsorted(L["frame_off"], row0, side="right") - 1   # (row0 = frame_off[u] + p0 lies inside utterance u)
    p0 = -lo
    np.testing.assert_array_equal(row0, L["frame_off"][utt] + p0, err_msg=str(what))
    np.testing.assert_array_equal(samp0, off[utt] + p0 * chain.H, err_msg=str(what))
    np.testing.assert_array_equal(live_n, T[utt] - p0, err_msg=str(what))
    np.testing.assert_array_equal(delta_on, (T[utt] > SHORT_T).astype(np.int64), err_msg=str(what))
    t0, t1 = p0 + e0, p0 + e1
    assert np.all(np.where(t0 > 0, e0 == 4, e0 == 0)), what         # four frames early inside an utterance, at 0 at its start
    assert np.all(p0 % 4 == 0) and np.all(t0 % 4 == 0), what        # a frame's lane group is its index mod 4
    np.testing.assert_array_equal(n_frames, ((t1 + 3) & ~3) - p0 + 4, err_msg=str(what))   # ... and the pass behind the last row
    # ... and stable: tiles of equal length in utterance order, an utterance's in frame order
    for n in np.unique(n_frames):
        sel = n_frames == n
        key = utt[sel] * (1 << 32) + t0[sel]
        assert np.all(np.diff(key) > 0), what
    for u in range(len(T)):                                          # [t0, t1) partition [0, T)
        sel = np.flatnonzero(utt == u)
        if T[u] == 0:
            assert len(sel) == 0, what
            continue
        order = sel[np.argsort(t0[sel])]
        assert t0[order[0]] == 0 and t1[order[-1]] == T[u] and np.array_equal(t0[order[1:]], t1[order[:-1]]), (what, u)
        if T[u] <= SHORT_T:
            assert len(sel) == 1, (what, u)


@pytest.mark.parametrize("name", list(CHAINS))
def test_decreasing_offsets_are_refused(lib, name):
    chain = Chain(name)
    rc, _ = chain.layout(lib, np.array([0, 16000, 15999, 40000], np.int64))
    assert rc == 2                                                   # utterance 1, counted from one
    rc, _ = chain.layout(lib, np.array([10, 9], np.int64))
    assert rc == 1


def test_run_frames_override_and_growth(lib):
    """SMILEHIP_RUN_FRAMES reaches the layout as run_frames_override; without it the runs double while >= 65 536 of them remain"""
    chain = Chain("compare_ab")
    off = offsets([chain.N + 99 * chain.H] * 5)
    rc, L = chain.layout(lib, off, run_frames_override=24)
    assert rc == 0 and L["scalars"][3] == 24
    covers_once(L["run_utt"], L["run_t0"], np.full(5, 100), 24, "override")
    assert [lib.blc_compare_run_frames(n) for n in (0, 16 * 65536 - 1, 16 * 65536, 32 * 65536, 64 * 65536, 1 << 40)] == [8, 8, 16, 32, 64, 64]
