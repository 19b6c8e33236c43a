"""The registry and the checker of tests/helpers/op_layouts.py without a device: every entry point of include/smilehip.h that takes
a leading dimension is in the registry (or exempt, with the reason), the checker raises for each defect it exists to find, and
every entry's reference is a real one (declared width, finite, not constant)."""
import os
import re
import zlib

import numpy as np
import pytest

from helpers import op_layouts as OL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD_NAMES = ("ld_src", "ld_dst", "ld_x", "ld_y", "ld_formants")


def header_functions():
    """{name: parameter list} of every function include/smilehip.h declares"""
    text = open(os.path.join(ROOT, "include", "smilehip.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"^\s*#.*$", " ", text, flags=re.M)
    return {m.group(1): m.group(2) for m in re.finditer(r"\b(smilehip_\w+)\s*\(([^;{}()]*)\)\s*;", text)}


def test_every_entry_point_with_a_leading_dimension_is_covered():
    fns = header_functions()
    assert len(fns) > 100 and "smilehip_harmonics_frames" in fns
    with_ld = {n for n, params in fns.items() if re.search(r"\b(%s)\b" % "|".join(LD_NAMES), params)}
    covered = {e.fn for e in OL.REGISTRY}
    missing = sorted(with_ld - covered - set(OL.EXEMPT))
    assert not missing, f"entry points with a leading dimension and no entry in tests/helpers/op_layouts.py: {missing}"
    assert not (covered & set(OL.EXEMPT)), "an exempt entry point is in the registry"
    unknown = sorted((covered | set(OL.EXEMPT)) - set(fns))
    assert not unknown, f"not in include/smilehip.h: {unknown}"
    stale = sorted(set(OL.EXEMPT) - with_ld)
    assert not stale, f"exempt without a leading dimension: {stale}"
    assert all(len(r) > 20 for r in OL.EXEMPT.values())
    names = [e.name for e in OL.REGISTRY]
    assert len(names) == len(set(names))


# the option sets each entry point is to be run with (entries per entry point)
VARIANTS = {"preemphasis_frames": 2, "rfft_frames": 2, "fftmagphase_frames": 4, "melspec_table_frames": 2, "acf_frames": 4,
            "valbased_select_frames": 4, "spectral_frames": 3, "plp_audspec_frames": 3, "plp_stage_frames": 2, "window_op_block": 3,
            "specscale_op_frames": 2, "intensity_frames": 3, "vecop_frames": 13}


def test_option_sets():
    count = {}
    for e in OL.REGISTRY:
        count[e.fn] = count.get(e.fn, 0) + 1
    for fn, n in VARIANTS.items():
        assert count.get("smilehip_" + fn, 0) >= n, fn
    assert {e.name for e in OL.REGISTRY} >= {"rfft_512", "rfft_256", "acf_K257_acf", "acf_K129_cepstrum", "valbased_N21", "valbased_N257_remove",
                                            "spectral_K129", "spectral_K513", "plp_audspec_rasta2", "mzcr_all", "melspec_table_dense"}
    stateful = {e.fn for e in OL.REGISTRY if e.stateful}
    assert stateful >= {"smilehip_spectral_frames", "smilehip_spectral_gemaps_frames", "smilehip_plp_audspec_frames",
                        "smilehip_delta_segments_block", "smilehip_pitch_smoother_rows", "smilehip_formantlpc_rows"}


# ---- the checker
N, W, LD = 6, 4, 9


def good():
    rng = np.random.default_rng(3)
    packed = rng.standard_normal((N, W)).astype(np.float32)
    buf, view = OL.padded(np.zeros((N, 0), np.float32), LD, OL.SENTINEL)
    view[:, :W] = packed
    return buf, view, packed


def test_padded_layout():
    x = np.arange(12, dtype=np.float32).reshape(3, 4)
    buf, view = OL.padded(x, 7, float("nan"))
    assert buf.size == 2 + 5 * 7 and view.shape == (3, 7) and np.shares_memory(buf, view)
    assert view.ctypes.data - buf.ctypes.data == 4 * OL.first_row_offset(7)
    for ld in range(4, 12):                                # row 0 is one float past a 16-byte boundary, whatever the stride
        assert OL.first_row_offset(ld) % 4 == 1 and ld < OL.first_row_offset(ld) <= ld + 4
    assert np.array_equal(view[:, :4], x) and np.isnan(view[:, 4:]).all() and np.isnan(buf[:9]).all() and np.isnan(buf[-7:]).all()
    assert np.array_equal(OL.unpadded(buf, 7, 4, 3), x.view(np.uint32))
    b2, _ = OL.padded(x, 4, OL.SENTINEL)
    assert (b2.view(np.uint32)[:5] == OL.SENTINEL).all() and np.isnan(b2[0]) and b2.size == 1 + 5 * 4
    b3, v3 = OL.padded(x, 7, 1e30, lead=0)
    assert b3.size == 5 * 7 and v3[0, 6] == np.float32(1e30)


def test_checker_passes_a_correct_buffer():
    buf, view, packed = good()
    OL.check_layout(buf, LD, W, N, packed, OL.SENTINEL)
    # fewer rows written than the call had (smilehip_pitch_smoother_rows): the rest holds the sentinel
    view[N - 1] = np.array([OL.SENTINEL], np.uint32).view(np.float32)[0]
    OL.check_layout(buf, LD, W, N, packed[:N - 1], OL.SENTINEL, rows_written=N - 1)


def defect_pad(buf, view, packed):
    view[2, W + 1] = 0.0


def defect_guard_front(buf, view, packed):
    buf[3] = 1.0


def defect_guard_behind(buf, view, packed):
    buf[-2] = 1.0


def defect_unwritten(buf, view, packed):
    view[4, 1] = np.array([OL.SENTINEL], np.uint32).view(np.float32)[0]


def defect_stride(buf, view, packed):
    """rows written at stride w_dst where the stride is ld_dst"""
    flat = buf[OL.first_row_offset(LD):]
    flat[:N * LD] = np.array([OL.SENTINEL], np.uint32).view(np.float32)[0]
    flat[:N * W] = packed.ravel()


def defect_ulp(buf, view, packed):
    view[3, 2] = np.nextafter(view[3, 2], np.float32(np.inf))


@pytest.mark.parametrize("defect", [defect_pad, defect_guard_front, defect_guard_behind, defect_unwritten, defect_stride, defect_ulp],
                         ids=lambda f: f.__name__[7:])
def test_checker_raises_for(defect):
    buf, view, packed = good()
    defect(buf, view, packed)
    with pytest.raises(AssertionError):
        OL.check_layout(buf, LD, W, N, packed, OL.SENTINEL)


def test_checker_raises_for_a_row_behind_the_written_ones():
    buf, view, packed = good()
    with pytest.raises(AssertionError):
        OL.check_layout(buf, LD, W, N, packed[:N - 1], OL.SENTINEL, rows_written=N - 1)


def test_sentinel_is_a_nan_with_a_payload():
    s = np.array([OL.SENTINEL], np.uint32)
    assert np.isnan(s.view(np.float32)[0]) and int(s[0]) != int(np.array([np.nan], np.float32).view(np.uint32)[0])
    # two of them as one double (the operators with one double per frame): about -3e307, no operator's output either
    assert np.array([OL.SENTINEL, OL.SENTINEL], np.uint32).view(np.float64)[0] < -1e300


# ---- the references
@pytest.mark.parametrize("entry", OL.REGISTRY, ids=lambda e: e.name)
def test_reference_is_not_vacuous(entry, oracle):
    rng = np.random.default_rng(zlib.crc32(entry.name.encode()))
    x = entry.make(rng, 5)
    assert x.dtype == np.float32 and x.ndim == 2
    if not entry.src_flat:
        assert x.shape[0] == 5 + sum(entry.halo) and x.shape[1] >= entry.widths[0]
    ref = entry.reference(x)
    if isinstance(ref, tuple):
        ref, extra = ref
        assert all(len(v) == 5 for v in extra.values())
    rows = 5 if entry.rows_written is None else entry.rows_written(5, True)
    words = OL.as_words(ref, entry.dst_dtype)
    assert words.shape == (rows, entry.widths[1]), (words.shape, entry.widths)
    ref = np.asarray(ref, np.float64)
    assert np.isfinite(ref).all(), f"{int((~np.isfinite(ref)).sum())} non-finite reference values"
    assert np.unique(ref).size > 1, "a constant reference"
    assert entry.kind in ("oracle", "restatement")


@pytest.mark.parametrize("entry", [e for e in OL.REGISTRY if e.compare != "pitchacf" and not isinstance(e.compare, tuple)], ids=lambda e: e.name)
def test_comparison_with_the_reference_is_not_vacuous(entry, oracle):
    """compare() takes the reference's own rows and refuses them with one cell changed: by one unit in the last place where the
    entry demands bits, by a thousandth of the largest value where it has an allowance (all of them are below 1e-5)"""
    rng = np.random.default_rng(zlib.crc32(entry.name.encode()))
    ref = entry.reference(entry.make(rng, 5))
    extra = None
    if isinstance(ref, tuple):
        ref, extra = ref
    ref = np.ascontiguousarray(ref, entry.dst_dtype).reshape(len(ref), -1)
    OL.compare(entry, OL.as_words(ref, entry.dst_dtype), ref, extra, extra)
    bad = ref.copy()
    at = np.unravel_index(np.argmax(np.abs(ref)), ref.shape)
    if entry.compare in ("bits", "bits_strict"):
        bad[at] = bad[at] + 1 if entry.dst_dtype == np.int32 else np.nextafter(bad[at], entry.dst_dtype(np.inf))
    else:
        bad[at] = bad[at] * entry.dst_dtype(1.001)
    assert OL.as_words(bad, entry.dst_dtype).tobytes() != OL.as_words(ref, entry.dst_dtype).tobytes()
    with pytest.raises(AssertionError):
        OL.compare(entry, OL.as_words(bad, entry.dst_dtype), ref, extra, extra)
