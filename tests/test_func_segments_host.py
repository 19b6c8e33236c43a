"""Functionals over listed segments (cWinToVecProcessor frameMode = list), the part that needs no device: the list parser
smilehip_func_list_parse and the fit rule smilehip_func_list_fit against what the real binary was measured to do (the table below,
and the fixture tests/golden/func_segments_is09.npz that tests/golden/make_golden_func_segments.py records from
oracle/_ref/SMILExtract), the clamps, and the refusals."""
import ctypes as C
import os

import numpy as np
import pytest

from opensmile_amd import capi

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "func_segments_is09.npz")
PERIOD = 0.01

# IS09_emotion.conf on a 16 kHz file of 99 LLD rows: frameList -> the (first row, rows) of the vectors the binary wrote
MEASURED = (
    ("10-50", [(10, 41)]),
    ("0.3s-0.9s", [(30, 61)]),
    ("20,30,10", [(0, 20), (20, 30), (50, 10)]),
    ("0.2s,0.3s", [(0, 21), (20, 31)]),
    ("0.105s-0.2049s", [(10, 12)]),
    ("0.5s-0.98s", [(50, 49)]),
    ("0.29s-0.57s,0.07s-0.14s", [(28, 30), (7, 9)]),      # 0.29 / 0.01 floors to 28, 0.14 / 0.01 ceils to 15
    ("3-3", [(3, 4)]),                                       # "too short": end = start + 3
    ("5-6", [(5, 4)]),
    ("0-98", [(0, 99)]),
    ("0-99", []),
    ("0.3s-0.9s,0.1s-0.5s", [(30, 61), (10, 41)]),          # list order, not time order
    ("0.1s-0.5s,0.1s-0.5s", [(10, 41), (10, 41)]),
    ("0.0s-0.5s,0.2s-5.0s,0.1s-0.3s", [(0, 51)]),           # the second does not fit and blocks the third
    ("0.5s-0.97s,0.5s-0.98s,0.5s-0.99s,0.5s-1.0s", [(50, 48), (50, 49)]),
)
ROWS = 99


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def emitted(frame_list, rows, period=PERIOD):
    first, n_rows = capi.func_list_parse(frame_list, period)
    n = capi.func_list_fit(first, n_rows, rows)
    return list(zip(first[:n].tolist(), n_rows[:n].tolist()))


@pytest.mark.parametrize("frame_list,want", MEASURED)
def test_parser_against_the_measured_table(frame_list, want):
    assert emitted(frame_list, ROWS) == want


def test_parser_against_the_binary(golden):
    """Every list of the fixture on every file: the count, the rows behind every vector, the frameTime the CSV sink printed."""
    files, lists = golden["files"], [str(s) for s in golden["lists"]]
    assert [int(golden[f"rows_{f}"]) for f in range(len(files))] == [12, 29, 99, 369]
    assert lists[:len(MEASURED)] == [m[0] for m in MEASURED] and len(lists) == len(MEASURED) + 1
    seen = 0
    for f in range(len(files)):
        rows = int(golden[f"rows_{f}"])
        for li, fl in enumerate(lists):
            if f"n_{f}_{li}" not in golden:
                assert li == int(golden["big"]) and rows != 369
                continue
            got = emitted(fl, rows)
            assert len(got) == int(golden[f"n_{f}_{li}"]) == golden[f"func_{f}_{li}"].shape[0], (rows, fl)
            assert got == list(zip(golden[f"first_{f}_{li}"].tolist(), golden[f"len_{f}_{li}"].tolist())), (rows, fl)
            assert np.allclose(golden[f"time_{f}_{li}"], np.array([a for a, _ in got], np.float64) * PERIOD, rtol=0, atol=5e-7), (rows, fl)
            assert golden[f"func_{f}_{li}"].shape[1] == 384
            seen += len(got)
    big = emitted(lists[-1], 369)
    assert len(big) == 40 and {2, 3, 64, 65, 300} <= {r for _, r in big} and len(set(big)) < 40      # short, around a wave, long, a repeat
    assert seen == 92                                      # 2 + 5 + 20 + 25 vectors of the table's lists, 40 of the long one
    assert os.path.getsize(GOLDEN) <= 1 << 20


def test_fit_rule_on_the_blocked_lists():
    """A segment whose last row is not in the level is never emitted and blocks every segment after it."""
    first, n_rows = capi.func_list_parse("0.0s-0.5s,0.2s-5.0s,0.1s-0.3s", PERIOD)
    assert list(zip(first.tolist(), n_rows.tolist())) == [(0, 51), (20, 481), (10, 21)]
    assert capi.func_list_fit(first, n_rows, ROWS) == 1
    assert capi.func_list_fit(first, n_rows, 501) == 3 and capi.func_list_fit(first, n_rows, 500) == 1
    first, n_rows = capi.func_list_parse("0.5s-0.97s,0.5s-0.98s,0.5s-0.99s,0.5s-1.0s", PERIOD)
    assert list(zip(first.tolist(), n_rows.tolist())) == [(50, 48), (50, 49), (50, 50), (50, 51)]
    assert [capi.func_list_fit(first, n_rows, r) for r in (97, 98, 99, 100, 101)] == [0, 1, 2, 3, 4]
    assert capi.func_list_fit(np.zeros(0, np.int64), np.zeros(0, np.int64), 10) == 0
    # last row = rows - 1 fits, last row = rows does not
    assert capi.func_list_fit([0], [99], 99) == 1 and capi.func_list_fit([1], [99], 99) == 0


def test_the_two_clamps():
    """Rows: end - start < 3 -> end = start + 3. Seconds: end - start < 0.01 -> end = start + 0.01."""
    assert emitted("3-3", 99) == [(3, 4)] and emitted("5-6", 99) == [(5, 4)] and emitted("5-7", 99) == [(5, 4)]
    assert emitted("5-8", 99) == [(5, 4)] and emitted("5-9", 99) == [(5, 5)]
    assert emitted("50-10", 99) == [(50, 4)]                           # a negative length is "too short" as well
    # seconds: [0.2, 0.2] becomes [0.2, 0.21]: floor(0.2 / 0.01) = 20, ceil(0.21 / 0.01) = 21 -> rows 20 .. 21
    first, n_rows = capi.func_list_parse("0.2s-0.2s", PERIOD)
    want_end = int(np.ceil((0.2 + 0.01) / PERIOD))
    assert first.tolist() == [20] and n_rows.tolist() == [want_end - 20 + 1]
    first, n_rows = capi.func_list_parse("0.2s-0.205s", PERIOD)
    assert first.tolist() == [20] and n_rows.tolist() == [want_end - 20 + 1]
    # a length in rows below 3 is 3 rows (the reference logs an error and sets it)
    assert emitted("1,2,5", 99) == [(0, 3), (3, 3), (6, 5)]


def test_token_forms():
    assert emitted(" 10 - 50 , 60-70 ", 99) == [(10, 41), (60, 11)]   # blanks around values
    assert emitted("0.3S-0.9S", 99) == [(30, 61)]                      # the capital suffix
    assert emitted("0.3s-0.9s", 99, period=0.0) == [(0, 2)]            # period 0 is taken as 1: floor(0.3), ceil(0.9)
    assert emitted("1e1-5e1", 99) == [(10, 41)]                        # what strtod reads


@pytest.mark.parametrize("frame_list,token", [
    ("10-E", "10-E"),                                                  # to the end of the input: the binary emits nothing
    ("10-50,60-E", "60-E"),
    ("0.1s-0.5s,10-50", "10-50"),                                      # seconds and rows
    ("10-0.5s", "10-0.5s"),
    ("10-50,30", "30"),                                                # intervals and lengths
    ("0.2s,0.1s-0.3s", "0.1s-0.3s"),
    ("0.2s,0.005s", "0.005s"),                                         # a length in seconds below 0.01
    ("10-50,,60-70", "empty"),
    ("", "empty"),
    ("10-50,", "empty"),
    ("-50", "-50"),                                                    # an empty value
    ("10x-50", "10x-50"),                                              # not consumed whole by strtod
    ("10-50-60", "10-50-60"),
    ("1 0-50", "1 0-50"),
    ("abc", "abc"),
    ("0.3 s-0.9s", "0.3 s-0.9s"),
])
def test_refusals_name_the_token(frame_list, token):
    with pytest.raises(capi.SmileHipError) as e:
        capi.func_list_parse(frame_list, PERIOD)
    assert "error -1" in str(e.value) and token in str(e.value), str(e.value)


def test_cap_zero_counts():
    L = capi.load()
    n = C.c_int32(-1)
    assert L.smilehip_func_list_parse(b"20,30,10", PERIOD, None, None, 0, C.byref(n)) == 0 and n.value == 3
    first, rows = np.full(4, -7, np.int64), np.full(4, -7, np.int64)
    assert L.smilehip_func_list_parse(b"20,30,10", PERIOD, first.ctypes.data, rows.ctypes.data, 4, C.byref(n)) == 0 and n.value == 3
    assert first.tolist() == [0, 20, 50, -7] and rows.tolist() == [20, 30, 10, -7]
    assert L.smilehip_func_list_parse(b"20,30,10", PERIOD, first.ctypes.data, rows.ctypes.data, 2, C.byref(n)) == -1
    assert b"cap" in L.smilehip_last_error()
    assert L.smilehip_func_list_parse(b"20,30,10", PERIOD, None, None, 3, C.byref(n)) == -1      # cap without arrays


def test_compute_refusals_need_no_device():
    """What the matrix entry point refuses, it refuses before it looks for a device: Modulation below 34 rows, a segment of no
    row, a negative first row, a last row beyond the matrix -- each naming utterance and segment."""
    from test_func_windows_host import modulation_spec
    L = capi.load()
    s = modulation_spec()

    def call(spec, first, rows, total=100, cols=4, per=11):
        first, rows = np.array(first, np.int64), np.array(rows, np.int64)
        rc = L.smilehip_funcspec_matrix_segments(None, C.byref(spec), None, cols, total, cols, len(first), first.ctypes.data, rows.ctypes.data,
                                                 None, cols * per, None)
        return rc, L.smilehip_last_error()
    rc, msg = call(s, [0, 10], [40, 33])
    assert rc == -1 and b"Modulation" in msg and b"34" in msg and b"utterance 0, segment 1" in msg
    assert call(s, [0, 10], [40, 34])[0] == -2                         # accepted up to the missing device
    s09 = capi.funcspec_is09()
    rc, msg = call(s09, [0, 5], [10, 0], cols=32, per=12)
    assert rc == -1 and b"utterance 0, segment 1" in msg and b"0 rows" in msg
    rc, msg = call(s09, [-1], [10], cols=32, per=12)
    assert rc == -1 and b"utterance 0, segment 0" in msg and b"negative" in msg
    rc, msg = call(s09, [0, 0, 91], [100, 3, 10], cols=32, per=12)
    assert rc == -1 and b"utterance 0, segment 2" in msg and b"[91, 100]" in msg
    assert call(s09, [0, 90], [100, 10], cols=32, per=12)[0] == -2
    with pytest.raises(capi.SmileHipError, match="Modulation"):
        capi.funcspec_matrix_segments_host(None, s, np.zeros((100, 4), np.float32), [0], [20])
