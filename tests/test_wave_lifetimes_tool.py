"""tools/ubench/wave_lifetimes.py on a synthetic record with known answers (no GPU): the decoding of HW_ID / XCC_ID, which waves
share a SIMD, the finish order against the start order, and the time integral of resident waves per SIMD."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools", "ubench"))
import wave_lifetimes as wl  # noqa: E402


def hw_id(wave_id, simd, cu, sh, se):
    return wave_id | (simd << 4) | (cu << 8) | (sh << 12) | (se << 13) | (0x5 << 16) | (0x2 << 24)     # (tg and queue bits set: ignored)


def rec(t0, t1, xcc, se, sh, cu, simd, wave_id, block, wave, passes):
    return [t0, t1, hw_id(wave_id, simd, cu, sh, se) | (xcc << 32), block | (wave << 32), passes, 1]


# SIMD A (XCC 1, SE 2, SH 0, CU 3, SIMD 1): a staircase -- four waves start 1 tick apart and leave at 40, 60, 85, 100.
# SIMD B (XCC 7, SE 5, SH 1, CU 15, SIMD 3), a CU whose clock has another zero: two waves that finish in REVERSE order, 50 ticks.
RAW = np.array([
    rec(1000, 1040, 1, 2, 0, 3, 1, 0, 5, 1, 10),
    rec(1001, 1060, 1, 2, 0, 3, 1, 1, 5, 5, 10),
    rec(1002, 1085, 1, 2, 0, 3, 1, 2, 9, 1, 12),
    rec(1003, 1100, 1, 2, 0, 3, 1, 3, 9, 5, 10),
    [7, 7, 7, 7, 7, 0],                                  # never written: skipped
    rec(9000000, 9000050, 7, 5, 1, 15, 3, 4, 2, 3, 3),
    rec(9000010, 9000040, 7, 5, 1, 15, 3, 1, 2, 7, 3),
], dtype=np.uint64)


def test_decode():
    f = wl.decode_hw_id(hw_id(9, 2, 11, 1, 6))
    assert (f["wave_id"], f["simd"], f["cu"], f["sh"], f["se"]) == (9, 2, 11, 1, 6)
    assert wl.decode_xcc_id(0xabc7) == 7
    recs = wl.decode_records(RAW)
    assert len(recs) == 6
    assert recs[2] == {"t0": 1002, "t1": 1085, "xcc": 1, "se": 2, "sh": 0, "cu": 3, "simd": 1, "wave_id": 2, "block": 9, "wave": 1,
                       "passes": 12}
    assert (recs[5]["xcc"], recs[5]["se"], recs[5]["sh"], recs[5]["cu"], recs[5]["simd"], recs[5]["wave_id"]) == (7, 5, 1, 15, 3, 1)


def test_analysis_known_answers():
    a = wl.analyse(wl.decode_records(RAW), n_simds=2)
    assert (a["n_waves"], a["n_simds_used"], a["n_cus_used"]) == (6, 2, 2)
    assert a["longest_lifetime_ticks"] == 97.0            # 1100 - 1003
    assert a["launch_span_ticks"] == 100.0                # CU A: 1000 .. 1100; CU B's 50 ticks on its own clock
    assert a["cu_span_over_launch"]["min"] == pytest.approx(0.5)
    lives = [40, 59, 83, 97, 50, 30]
    assert a["lifetime_over_longest"]["mean"] == pytest.approx(np.mean(lives) / 97.0)
    assert a["lifetime_over_launch_mean"] == pytest.approx(np.mean(lives) / 100.0)
    # the integral: wave-ticks over SIMDs x launch
    assert a["resident_waves_per_simd"] == pytest.approx(sum(lives) / (2 * 100.0))
    sa, sb = a["per_simd"]                                # sorted by (xcc, se, sh, cu, simd)
    assert (sa["xcc"], sa["se"], sa["sh"], sa["cu"], sa["simd"]) == (1, 2, 0, 3, 1)
    assert sa["resident_over_launch"] == pytest.approx(2.79)
    assert sb["resident_over_launch"] == pytest.approx(0.80)
    assert sa["waves"][0] == [5, 1, 0, 0, 40, 10] and sa["waves"][3] == [9, 5, 3, 3, 100, 10]
    fo = a["finish_order"]
    assert fo["simds_finishing_in_start_order"] == 1 and fo["of"] == 2
    assert fo["mean_rank_correlation"] == pytest.approx(0.0)          # +1 on A, -1 on B
    assert fo["mean_lifetime_over_longest_by_start_rank"]["3"] == pytest.approx(1.0)
    assert fo["mean_lifetime_over_longest_by_start_rank"]["0"] == pytest.approx((40 / 97 + 50 / 97) / 2)
    assert fo["lifetime_spread_within_simd"]["max"] == pytest.approx(57 / 97)
    sh = a["sharing"]
    assert sh["wave_numbers_on_a_simd"] == {"[1, 1, 5, 5]": 1, "[3, 7]": 1}
    assert sh["hw_wave_slots_on_a_simd"] == {"[0, 1, 2, 3]": 1, "[1, 4]": 1}
    assert sh["blocks_on_a_simd"] == {"1": 1, "2": 1}
    assert sh["simds_with_distinct_slot_mod_4"] == 2      # B: slots 4 and 1 -> 0 and 1
    assert a["passes"] == {"min": 3, "max": 12}
    assert "resident waves per SIMD" in wl.report(a)


def test_no_record_is_an_error():
    with pytest.raises(ValueError):
        wl.analyse(wl.decode_records(np.zeros((4, wl.WORDS), np.uint64)))
