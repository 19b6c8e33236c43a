"""Pins the CPU oracle against the REAL binary on the hard-signal corpus (tests/helpers/hard_signals.py: full-scale and clipped
samples, DC, +-1 LSB noise, clicks inside digital zeros, zero gaps inside voiced speech, F0 outside / at the edge of the SHS range,
octave jumps, a glide, a missing fundamental) -- the inputs on which log floors, 0/0 in the spectral moments, voiced / unvoiced run
edges, noZeroSma / onlyInSegments and Viterbi transitions decide the result. tests/golden/hard_*.npz hold the binary's output
(tests/golden/make_golden_hard.py); where oracle/_ref is built the fixtures are also compared with a fresh run of the binary, so a
stale fixture cannot hide.

The last test checks the float64 restatement of MFCC12_0_D_A's tail (hard_signals.e_ref) that tests/test_gpu_hard_signals.py uses
to judge the fast kernel: e_ref(frame) is the reference's OWN transform rounding on that frame, seen through the tail. These signals
amplify it: at most 2.9e-7 on the synthetic corpus, up to 6.03e-6 here (glide_80_600)."""
import importlib.util
import os

import numpy as np
import pytest

from helpers import hard_signals
from test_oracle_pin_funcspec import func_rows, inputs, pending
from tolerance import assert_bits_equal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NAMES = hard_signals.NAMES
SETS = ("hard_mfcc_plp", "hard_is09", "hard_compare16", "hard_egemaps")
# (instance, first LLD column, columns) in the order [functionals] concatenates the six cFunctionals instances' values
PARTS = [("A", 6, 4), ("A", 71, 4), ("B", 10, 55), ("B", 75, 55), ("Nz", 0, 6), ("Nz", 65, 6), ("F0", 0, 1), ("LLD", 6, 59),
         ("Delta", 71, 59)]


def load(stem):
    return np.load(os.path.join(GOLDEN, stem + ".npz"))


def same_or_both_zero(a, b):
    """eGeMAPS: +0 and -0 count as equal (tests/test_gpu_egemaps.py::bits_equal)."""
    a = np.ascontiguousarray(a, np.float32)
    b = np.ascontiguousarray(b, np.float32)
    assert a.shape == b.shape, (a.shape, b.shape)
    return (a.view(np.uint32) == b.view(np.uint32)) | ((a == 0) & (b == 0))


def compare16_func_from_lld(oracle, lld, b_extra, T, P, spec_of=None):
    """The 6373 functionals from a 130-column LLD matrix (T + 1 rows) and row T + 1 of the group-B levels (110 values), with the
    row rules of tests/test_oracle_pin_funcspec.py. Returns (values [6373], value name per position)."""
    spec_of = spec_of or oracle.compare16_func_spec
    vals, names = [], []
    for inst, c0, nc in PARTS:
        spec = spec_of(inst)
        n = func_rows(inst, T, P)
        if inst == "B":
            half = slice(0, 55) if c0 == 10 else slice(55, 110)
            xi = np.concatenate([lld[:, c0:c0 + nc], np.asarray(b_extra, np.float32)[None, half]], axis=0)
            assert xi.shape[0] == n
        else:
            xi = lld[:n, c0:c0 + nc]
        vals.append(oracle.funcspec(np.ascontiguousarray(xi), spec).reshape(-1))
        names += oracle.funcspec_names(spec) * nc
    return np.concatenate(vals), names


@pytest.fixture(scope="module")
def sig():
    return hard_signals.signals()


@pytest.fixture(scope="module")
def golden():
    return {s: load(s) for s in SETS}


def test_generator_reproduces_the_committed_samples(sig):
    z = load("hard_pcm")
    assert tuple(sig) == NAMES and sorted(z.files) == sorted(NAMES)
    for k in NAMES:
        assert sig[k].dtype == np.int16 and sig[k].shape == (24000,) and np.array_equal(sig[k], z[k]), k
    assert sig["clip_sine"].max() == 32767 and sig["clip_sine"].min() == -32768 and not sig["clicks_in_zeros"][:700].any()


def test_fixture_shapes_and_no_nonfinite_value(golden):
    shapes = {"hard_mfcc_plp": {"mfcc": (148, 39), "plp": (148, 18)}, "hard_is09": {"lld": (149, 32), "func": (1, 384)},
              "hard_compare16": {"lld": (146, 130), "func": (6373,)}, "hard_egemaps": {"lld": (146, 25), "func": (1, 88)}}
    for s, d in shapes.items():
        for k, shp in d.items():
            for n in NAMES:
                a = golden[s][k + "_" + n]
                assert a.shape == shp and a.dtype == np.float32 and np.isfinite(a).all(), (s, k, n)
    for n in hard_signals.TAPPED:
        for k in ("a_smo", "a_de", "b_smo", "b_de", "nz_smo", "nz_de", "f0_smo"):
            assert np.isfinite(golden["hard_compare16"][k + "_" + n]).all()
    # the F0 group is exercised: seven signals without a voiced frame (F0final_sma > 0), four voiced throughout, four in between
    voiced = [int((golden["hard_compare16"]["lld_" + n][:, 0] > 0).sum()) for n in NAMES]
    assert sorted(voiced) == [0] * 7 + [76, 77, 121, 143] + [146] * 4
    for s in SETS:
        assert os.path.getsize(os.path.join(GOLDEN, s + ".npz")) <= 1024 * 1024, s


@pytest.mark.parametrize("name", NAMES)
def test_mfcc_plp_is09_bit_exact(oracle, golden, sig, name):
    oracle.use_reference_fft(False)
    g = golden["hard_mfcc_plp"]
    assert_bits_equal(oracle.mfcc_chain(oracle.default_cfg(), sig[name]), g["mfcc_" + name], "MFCC12_0_D_A " + name)
    assert_bits_equal(oracle.plp_chain(sig[name]), g["plp_" + name], "PLP_0_D_A " + name)
    g = golden["hard_is09"]
    lld = g["lld_" + name]
    assert_bits_equal(oracle.is09_chain(sig[name]), lld, "IS09_emotion LLD " + name)
    assert_bits_equal(oracle.functionals(lld[:max(1, lld.shape[0] - 3)]).reshape(1, -1), g["func_" + name], "IS09_emotion functionals " + name)


@pytest.mark.parametrize("name", NAMES)
def test_compare16_lld_and_functionals_bit_exact(oracle, golden, sig, name):
    """The 130-column LLD level; the 6373 functionals from the oracle's own LLD matrix (+ the extra group-B row) and -- for the
    signals whose level taps are in the fixture -- from exactly the rows the binary's cFunctionals instances read."""
    oracle.use_reference_fft(False)
    g = golden["hard_compare16"]
    lld = oracle.compare_lld_chain(sig[name])
    assert_bits_equal(lld, g["lld_" + name], "ComParE_2016 LLD " + name)
    T, P = pending(oracle, sig[name])
    assert lld.shape[0] == T + 1
    f, names = compare16_func_from_lld(oracle, lld, oracle.compare_b_extra(sig[name]), T, P)
    ref = g["func_" + name]
    d = f.view(np.uint32) != ref.view(np.uint32)
    assert not d.any(), f"{name} (T={T}, P={P}): {[(int(i), names[i]) for i in np.flatnonzero(d)[:8]]}"
    if name in hard_signals.TAPPED:
        check_func_from_taps(oracle, g, name, ref, T, P)


def check_func_from_taps(oracle, g, name, ref, T, P):
    X = inputs(g, name)
    pos = 0
    for inst in ("A", "B", "Nz", "F0", "LLD", "Delta"):
        spec = oracle.compare16_func_spec(inst)
        names = oracle.funcspec_names(spec)
        cols = X[inst].shape[1]
        r = ref[pos:pos + len(names) * cols].reshape(cols, len(names))
        pos += len(names) * cols
        out = oracle.funcspec(np.ascontiguousarray(X[inst][:func_rows(inst, T, P)]), spec)
        d = out.view(np.uint32) != r.view(np.uint32)
        assert not d.any(), f"{name}/{inst} from the binary's levels: {[(int(c), names[k]) for c, k in np.argwhere(d)[:5]]}"
    assert pos == 6373


@pytest.mark.parametrize("name", NAMES)
def test_egemaps_lld_and_functionals_bit_exact(oracle, golden, sig, name):
    oracle.use_reference_fft(False)
    g = golden["hard_egemaps"]
    d = ~same_or_both_zero(oracle.egemaps_lld_chain(sig[name]), g["lld_" + name])
    assert not d.any(), f"{name}: {int(d.sum())} LLD cells differ, columns {sorted(set(np.argwhere(d)[:, 1]))}, first frame {np.argwhere(d)[0, 0]}"
    d = ~same_or_both_zero(oracle.egemaps_func(sig[name]), g["func_" + name])
    assert not d.any(), f"{name}: functionals {np.flatnonzero(d)} differ"


def test_fixtures_equal_a_fresh_run_of_the_binary(oracle, golden, sig):
    if not oracle.have_ref():
        pytest.skip("oracle/_ref/SMILExtract not built")
    spec = importlib.util.spec_from_file_location("make_golden_hard", os.path.join(GOLDEN, "make_golden_hard.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    seen = {s: set() for s in SETS}
    for name in NAMES:
        r = mod.reference_sets(name, sig[name])
        assert r["names"] == [str(x) for x in golden["hard_compare16"]["names"]]
        for s in SETS:
            for k, a in r[s].items():
                f = golden[s][k]
                assert f.shape == a.shape and np.array_equal(f.view(np.uint32), a.view(np.uint32)), (s, k)
                seen[s].add(k)
    for s in SETS:
        assert seen[s] == set(golden[s].files) - {"names"}, s


def test_float64_restatement_and_the_references_own_rounding(oracle, sig):
    """(1) The float64 tail on the oracle's own magnitudes gives the oracle's static columns to 4e-7 (per-frame-scaled) on every
    frame whose mel energies are all above the floor: the restatement is the chain. (2) e_ref, the same tail on a float64 FFT
    against the tail on the oracle's magnitudes: at least 70 % of the non-zero frames <= 1e-6 (measured 77 - 81 %), maximum <= 1e-5
    (measured 6.03e-6, glide_80_600; octave_jumps 3.9e-6, f0_45 3.6e-6, gated_voiced 3.2e-6)."""
    oracle.use_reference_fft(False)
    es, worst = [], {}
    for name in NAMES:
        r = hard_signals.e_ref(oracle, sig[name])
        assert r["out"].shape == (148, 39)
        tail, _ = hard_signals.frame_scaled(r["c_mag"] - r["out"][:, :13], r["out"][:, :13])
        m = r["above"] & r["nz"]
        assert not m.any() or tail[m].max() <= 4e-7, (name, tail[m].max())
        es.append(r["e"][r["nz"]])
        worst[name] = float(r["e"].max())
    e = np.concatenate(es)
    print({k: f"{v:.3g}" for k, v in worst.items()}, f"{(e <= 1e-6).mean():.3f} of {len(e)} non-zero frames <= 1e-6")
    assert len(e) == 2011
    assert (e <= 1e-6).mean() >= 0.70
    assert e.max() <= 1e-5
