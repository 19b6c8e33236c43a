"""cFormantLpc's root carry on the device (lld_gemaps_formants + lld_gemaps_formants_fix) against the oracle, bit for bit.

A frame whose QR iteration gives up keeps the previous frame's folded roots wherever it found none
(tests/test_oracle_pin_formant_carry.py pins the rule on the real binary; a NaN LP coefficient is what makes it give up).
The rows start from the binary's own LP coefficients (tests/golden/egemaps_lld_synth.npz, as
test_gpu_egemaps.py::test_stage_formants_on_the_binarys_lpc) with rows or single coefficients set to NaN at the placements
where a per-frame kernel and its fix-up pass go wrong: the second and the last row, runs of 1 .. 70 rows, runs across a 64-row
workgroup and into the last partial one, a predecessor with roots outside the unit circle, and 10^5 rows with 1 % NaN. The
carry across calls goes through the state buffer of smilehip_formantlpc_rows.

Every matrix sent to the device is finite or NaN: +-inf coefficients make the balancing loop run forever (in the reference too).
No finite row is known that gives up after finding some roots (the search in test_oracle_pin_formant_carry.py's docstring), so
the partial re-solve of the fix-up pass is not exercised here."""
import os

import numpy as np
import pytest

from tolerance import assert_bits_equal

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def base_lpc():
    """The binary's LP rows of the golden eGeMAPS cases, cut to a length that leaves a partial last workgroup."""
    g = np.load(os.path.join(ROOT, "tests", "golden", "egemaps_lld_synth.npz"))
    rows = np.concatenate([g[k].reshape(-1, 11) for k in sorted(g.files) if k.startswith("lpc_") and g[k].size], axis=0)
    n = (len(rows) // 64) * 64 - 64 + 37
    assert n > 1000
    return np.ascontiguousarray(rows[:n], np.float32)


@pytest.fixture(scope="module")
def gm():
    from opensmile_amd import capi
    ctx = capi.Context(0)
    plan = capi.Plan(ctx, capi.egemapsv02_config())
    yield capi, plan
    plan.close()
    ctx.close()


def finite_or_nan(m):
    """Nothing that reaches the device may hold +-inf (the root solver's balancing would not end)."""
    m = np.ascontiguousarray(m, np.float32)
    assert (np.isfinite(m) | np.isnan(m)).all(), "+-inf in a matrix for the device"
    return m


def device(gm, lpc, cuts=None):
    capi, plan = gm
    return capi.formantlpc_host(plan, finite_or_nan(lpc), cuts)


def check(gm, oracle, lpc, what, cuts=None):
    ref = oracle.egemaps_formant_rows(lpc)
    out = device(gm, lpc, cuts)
    assert_bits_equal(out, ref, what)
    return out, ref


def with_nan(base, rows, cols=slice(None)):
    x = base.copy()
    for r in rows:
        x[r, cols] = np.nan
    return x


def test_nan_placements(gm, oracle, base_lpc):
    n = len(base_lpc)
    last_wg = (n // 64) * 64
    cases = {
        "one row": [100],
        "run of 2": range(200, 202),
        "run of 5": range(300, 305),
        "run of 70": range(400, 470),
        "second row": [1],
        "last row": [n - 1],
        "rows 63/64": range(62, 66),
        "workgroup boundary 575/576": [575, 576],
        "into the last partial workgroup": range(last_wg - 3, last_wg + 5),
        "last partial workgroup to the end": range(last_wg + 30, n),
        "two runs one row apart": [700, 701, 703, 704],
    }
    for what, rows in cases.items():
        out, ref = check(gm, oracle, with_nan(base_lpc, rows), what)
        r0 = list(rows)[0]
        # the carry happened: the first NaN row repeats its predecessor's row
        assert np.array_equal(out[r0].view(np.uint32), out[r0 - 1].view(np.uint32)), what


@pytest.mark.parametrize("cols", [[0], [5], [10], list(range(11))], ids=["coef0", "coef5", "coef10", "all11"])
def test_nan_in_some_coefficients(gm, oracle, base_lpc, cols):
    check(gm, oracle, with_nan(base_lpc, [150, 151, 640], cols), f"NaN in coefficients {cols}")


def test_first_row_gives_zeros(gm, oracle, base_lpc):
    """Nothing before the first row: the oracle's roots start at zero, so does the device (the reference would read
    uninitialised memory)."""
    out, _ = check(gm, oracle, with_nan(base_lpc, [0, 1, 2]), "first rows")
    assert not out[:3].any()


def test_carried_roots_are_the_folded_ones(gm, oracle, base_lpc):
    """A predecessor with roots outside the unit circle: what a NaN row carries is 1 / conj(root), not the root."""
    x = base_lpc.copy()
    # monic polynomial with one pair at radius 1.25 (formant angle ~ 700 Hz at 11 kHz) and the others inside
    ang = 2 * np.pi * np.array([700.0, 1500.0, 2500.0, 3500.0, 4500.0]) / 11000.0
    rad = np.array([1.25, 0.95, 0.9, 0.85, 0.8])
    z = np.concatenate([rad * np.exp(1j * ang), rad * np.exp(-1j * ang), [0.5]])
    poly = np.real(np.poly(z))                         # z^11 + c1 z^10 + ... ; lpc[k] = -c_{k+1}
    row = (-poly[1:]).astype(np.float32)
    assert np.isfinite(row).all()
    assert np.abs(np.roots(np.concatenate([[1.0], -row.astype(np.float64)]))).max() > 1.2
    x[800] = row
    x[801:804] = np.nan
    out, ref = check(gm, oracle, x, "predecessor with roots outside the unit circle")
    assert np.array_equal(out[801].view(np.uint32), out[800].view(np.uint32))
    # the folded pair gives the bandwidth of radius 1 / 1.25 (positive): the unfolded one would give a negative one
    assert (out[801, 5:] >= 0).all()


def test_hundred_thousand_rows_one_percent_nan(gm, oracle, base_lpc):
    rng = np.random.default_rng(7)
    reps = -(-100_003 // len(base_lpc))
    x = np.tile(base_lpc, (reps, 1))[:100_003].copy()
    n = len(x)
    nan_rows = 0
    while nan_rows < n // 100:
        a = int(rng.integers(1, n))
        k = int(min(rng.geometric(0.3), 40))
        cols = slice(None) if rng.random() < 0.7 else int(rng.integers(0, 11))
        x[a:a + k, cols] = np.nan
        nan_rows = int(np.isnan(x).any(axis=1).sum())
    out, _ = check(gm, oracle, x, "1e5 rows, 1 % NaN in random runs")
    # ... and split over calls, with cuts inside runs, at a run's first row and one row long
    runs = np.flatnonzero(np.isnan(x).any(axis=1))
    cuts = sorted({int(runs[10]) + 1, int(runs[500]), int(runs[500]) + 1, 64 * 700, 64 * 700 + 1, int(runs[-1])})
    out2 = device(gm, x, cuts)
    assert_bits_equal(out2, out, "1e5 rows in calls")


def test_carry_across_calls(gm, oracle, base_lpc):
    """Rows split over several calls of smilehip_formantlpc_rows give the single call's rows: the state buffer carries the roots
    of the last row into the next call, also when a whole call is NaN."""
    x = with_nan(base_lpc, list(range(400, 470)) + [63, 64, 65])
    single, _ = check(gm, oracle, x, "single call")
    for cuts in ([401], [64], [420, 421, 430], [400], [470], [10, 64, 128, 405, 460, 900]):
        assert_bits_equal(device(gm, x, cuts), single, f"calls split at {cuts}")


def test_finite_rows_unchanged_by_the_fix_pass(gm, oracle, base_lpc):
    """No NaN: every row converges, the fix-up pass has nothing to do; one call or many."""
    out, _ = check(gm, oracle, base_lpc, "finite rows")
    assert_bits_equal(device(gm, base_lpc, [1, 64, 65, 500]), out, "finite rows in calls")


@pytest.mark.parametrize("ticks", [{"SMILEHIP_PLUGIN_BLOCK": "0"}, {"SMILEHIP_PLUGIN_BLOCK_MIN": "2", "SMILEHIP_PLUGIN_BLOCK_MAX": "5"}, {}],
                         ids=["frame_per_tick", "blocks_of_2_to_5", "default_blocks"])
def test_plugin_carries_the_roots_between_ticks(oracle, tmp_path, ticks):
    """The unmodified binary with only cFormantLpc on the device (upstream components stay on the CPU, so NaN reaches this
    kernel alone) on tests/conf/formant_chain.conf and the NaN-burst float WAV: the formant rows of the plain binary, byte for
    byte, with one frame per tick, with blocks of 2-5 frames (the bursts cross ticks) and with the default blocks."""
    from test_oracle_pin_formant_carry import nan_burst_signal, run_formant_chain, write_f32_wav
    exe = os.path.join(oracle.REF_DIR, "SMILExtract")
    plugdir = os.path.join(ROOT, "opensmile_amd", "plugin")
    if not (os.path.exists(exe) and os.path.exists(os.path.join(plugdir, "plugins", "libsmilehip_plugin.so"))):
        pytest.skip("oracle/_ref/SMILExtract or the plugin .so not built (needs /root/reference at build time)")
    wav = str(tmp_path / "nan.wav")
    write_f32_wav(wav, nan_burst_signal())
    plain, dev = tmp_path / "plain", tmp_path / "dev"
    plain.mkdir()
    dev.mkdir()
    ref_lpc, ref_fm, _ = run_formant_chain(exe, wav, str(plain))
    assert np.isnan(ref_lpc).any(axis=1).sum() == 20
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = os.pathsep.join([os.path.join(ROOT, "opensmile_amd"), oracle.REF_DIR, env.get("LD_LIBRARY_PATH", "")])
    env.update({"SMILEHIP_PLUGIN_COMPONENTS": "cFormantLpc", "SMILEHIP_PLUGIN_FUSE": "0", "SMILEHIP_PLUGIN_TRACE": str(dev / "trace.txt")})
    env.update(ticks)
    lpc, fm, log = run_formant_chain(exe, wav, str(dev), env=env, cwd=plugdir)   # cwd: the directory that holds ./plugins
    tr = dict(l.split() for l in open(dev / "trace.txt").read().split("\n") if l.strip())
    assert int(tr["cFormantLpc"]) == len(ref_fm) and int(tr["cFormantLpc.cpu"]) == 0, tr
    assert np.array_equal(lpc.view(np.uint32), ref_lpc.view(np.uint32))
    assert fm.tobytes() == ref_fm.tobytes(), np.argwhere(fm.view(np.uint32) != ref_fm.view(np.uint32))[:10]
