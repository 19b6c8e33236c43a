"""Functionals over fixed windows (cWinToVecProcessor frameMode = fixed), the part that needs no device: the window geometry of
smilehip_func_window_geometry against what the real binary was measured to do (the tables below, and the fixture
tests/golden/func_windows_is09.npz that tests/golden/make_golden_func_windows.py records from oracle/_ref/SMILExtract), and the
refusals (a batch needs a device: its window prefix is checked in test_gpu_func_windows.py)."""
import ctypes as C
import os

import numpy as np
import pytest

from opensmile_amd import capi

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "func_windows_is09.npz")
PERIOD = 0.01

# IS09_emotion.conf on 16 kHz noise files, frameSize 0.1, frameStep 0.01: (LLD rows L, windows)
NOISE_FILES = ((8, 0), (12, 3), (29, 20), (99, 90), (122, 113), (369, 360), (1199, 1190), (2500, 2491))
# the reference's opensmile.wav, L = 203: (frameSize, frameStep, windows, last frameTime or None)
EXAMPLE_FILE = ((1.0, 0.5, 3, 1.0), (1.0, 0.01, 104, 1.03), (0.5, 0.01, 154, None), (0.03, 0.02, 101, 2.00))


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def test_geometry_of_the_measured_noise_files():
    for rows, n in NOISE_FILES:
        assert capi.func_window_geometry(PERIOD, 0.1, 0.01, rows) == (10, 1, n), rows


def test_geometry_of_the_measured_example_file():
    for size, step, n, last in EXAMPLE_FILE:
        sr, st, got = capi.func_window_geometry(PERIOD, size, step, 203)
        assert got == n, (size, step, got)
        if last is not None:                               # frameTime of a window = the time of its first row
            assert abs((n - 1) * st * PERIOD - last) < 1e-9, (size, step, st)
    assert capi.func_window_geometry(PERIOD, 1.0, 0.5, 203)[:2] == (100, 50)


def test_geometry_against_the_binary(golden):
    """Sizes of 12.5 and 13.5 rows are in the set for the round(); every count, and every frameTime the CSV sink printed."""
    files = golden["files"]
    assert [int(golden[f"rows_{f}"]) for f in range(len(files))] == [8, 12, 29, 99, 369]
    assert [tuple(g) for g in golden["geometries"]] == [(0.1, 0.01), (0.125, 0.05), (0.135, 0.135), (0.03, 0.02), (1.0, 0.5)]
    for g, (size, step) in enumerate(golden["geometries"]):
        for f in range(len(files)):
            rows = int(golden[f"rows_{f}"])
            sr, st, n = capi.func_window_geometry(PERIOD, float(size), float(step), rows)
            assert (sr, st) == (int(golden[f"size_{g}"]), int(golden[f"step_{g}"])), (size, step)
            assert n == int(golden[f"n_{f}_{g}"]) == golden[f"func_{f}_{g}"].shape[0], (size, step, rows)
            assert golden[f"func_{f}_{g}"].shape[1] == 384
            t = golden[f"time_{f}_{g}"]
            assert np.allclose(t, np.arange(n) * st * PERIOD, rtol=0, atol=5e-7), (size, step, rows)
    assert os.path.getsize(GOLDEN) <= 1 << 20


def test_zero_step_rows_becomes_the_size():
    assert capi.func_window_geometry(PERIOD, 0.05, 0.004, 20) == (5, 5, 4)
    assert capi.func_window_geometry(0.02, 0.1, 0.1, 4) == (5, 5, 0)
    assert capi.func_window_geometry(PERIOD, 0.1, 0.01, 0) == (10, 1, 0)


def test_geometry_refusals():
    with pytest.raises(capi.SmileHipError, match="frameSize"):
        capi.func_window_geometry(PERIOD, 0.004, 0.01, 100)            # rounds to 0 rows
    with pytest.raises(capi.SmileHipError, match="frameSize"):
        capi.func_window_geometry(PERIOD, 0.0, 0.01, 100)
    with pytest.raises(capi.SmileHipError, match="frameStep = 0.*full"):
        capi.func_window_geometry(PERIOD, 1.0, 0.0, 100)
    with pytest.raises(capi.SmileHipError, match="period"):
        capi.func_window_geometry(0.0, 1.0, 0.5, 100)
    # output pointers are optional
    assert capi.load().smilehip_func_window_geometry(PERIOD, 0.1, 0.01, 50, None, None, None) == 0


def modulation_spec():
    s = capi.FuncSpec()
    s.n_fam, s.period = 2, PERIOD
    s.fam[0], s.fam[1] = 14, 0
    s.ext_mask, s.ext_norm = 0x07, 2
    s.mod_win_frames, s.mod_step_frames, s.mod_n_bins, s.mod_win_func = 100, 50, 8, 1
    s.mod_min_freq, s.mod_max_freq = 0.5, 20.0
    return s


def test_modulation_below_34_rows_is_refused_by_name():
    """... before the entry points look at the device: the refusal needs none."""
    L = capi.load()
    s = modulation_spec()
    assert capi.funcspec_count(s) == 11
    rc = L.smilehip_funcspec_matrix_windows(None, C.byref(s), None, 4, 100, 4, 33, 1, None, 44, None)
    assert rc == -1 and b"Modulation" in L.smilehip_last_error() and b"34" in L.smilehip_last_error()
    rc = L.smilehip_funcspec_matrix_windows(None, C.byref(s), None, 4, 100, 4, 34, 1, None, 44, None)
    assert rc == -2, L.smilehip_last_error()                           # accepted up to the missing device
    s09 = capi.funcspec_is09()
    for size, step in ((0, 1), (5, 0)):
        rc = L.smilehip_funcspec_matrix_windows(None, C.byref(s09), None, 32, 100, 32, size, step, None, 384, None)
        assert rc == -1 and b"size_rows and step_rows" in L.smilehip_last_error()


def test_is09_spec():
    """IS09_emotion_core.func.conf.inc: Extremes max min range maxpos minpos amean (norm = frame); Regression linregc1 linregc2
    linregerrQ with oldBuggyQerr and no ratio limits; Moments stddev skewness kurtosis; period 0.01."""
    s = capi.funcspec_is09()
    assert capi.funcspec_count(s) == 12 and s.period == 0.01
    assert [s.fam[i] for i in range(s.n_fam)] == [0, 3, 2]
    assert (s.ext_mask, s.ext_norm) == (0x3f, 2)
    assert (s.reg_mask, s.reg_old_buggy_qerr, s.reg_ratio_limit, s.reg_centroid_limit, s.reg_norm_inputs, s.reg_norm_coeff) == (0b1011, 1, 0, 0, 0, 0)
    assert (s.mom_mask, s.mom_ratio_limit, s.non_zero_functs) == (0b1110, 0, 0)
