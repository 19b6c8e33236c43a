"""Every fused chain on the hard-signal corpus (tests/helpers/hard_signals.py) against the REAL binary's output
(tests/golden/hard_*.npz, pinned on the CPU by tests/test_oracle_pin_hard_signals.py): fifteen 1.5 s signals as one ragged batch
through the C ABI -- samples at +32767 / -32768, clipped tops, DC, +-1 LSB noise, clicks inside digital zeros, zero gaps inside
voiced speech, F0 below / near the top of the SHS range, octave jumps, a glide, a missing fundamental.

  a. the reference-order chains in every form (quad / wave / block) equal the binary's fixture bit for bit;
  b. the functionals of the device's own LLD matrix equal the oracle's and the binary's (degenerate contours: an all-unvoiced F0,
     constant columns, columns with one non-zero row);
  c. an utterance's rows do not depend on the batch around it (reverse order, an empty and a 100-sample utterance in between);
  d. the fast kernels (lld_mfcc512): finite, exact zeros where the reference row is zero, the project's 1e-5 gate wherever the
     reference's own transform rounding e_ref is <= 1e-6, per signal <= max(1e-5, 8 x max e_ref), regression columns bit for bit;
  e. smilextract_hip and the plugin inside the unmodified binary write the binary's files byte for byte.

d's factor 8 is not measured on the kernel under test: the kernel's recorded error on the standard corpus (1.04e-6, README) over the
reference's own rounding there (2.9e-7) is 3.6; times 2 for the spread of a maximum over ~150 frames between two independent
transforms, rounded up. e_ref is computed by the test from the oracle (hard_signals.e_ref).

Measured on an MI355X (per-frame-scaled, all 39 columns on the scale of the frame's static block):
    signal                   max e_ref  lld_mfcc512  on its frames with e_ref <= 1e-6 (their number)
    clip_sine                 2.05e-08   2.55e-07   2.55e-07 (148)
    nyquist_then_min          1.07e-06   1.26e-06   7.62e-07 (75)
    dc                        7.38e-07   1.07e-06   1.07e-06 (148)
    lsb_noise                 4.03e-07   7.24e-07   7.24e-07 (148)
    clicks_in_zeros           1.16e-07   4.53e-07   4.53e-07 (34)
    gated_voiced              3.16e-06   8.33e-06   4.12e-06 (64)
    f0_45                     3.61e-06   3.05e-05   5.72e-06 (60)
    f0_650                    4.25e-07   7.46e-07   7.46e-07 (148)
    octave_jumps              3.94e-06   1.19e-05   6.87e-06 (89)
    glide_80_600              6.03e-06   1.65e-05   1.08e-05 (108)
    missing_fundamental        1.8e-06   3.49e-06    1.9e-06 (89)
    bin_tone_lsb_then_full    4.04e-07   7.14e-07   7.14e-07 (148)
    slow_ramp                 1.79e-06   4.64e-06   4.64e-06 (136)
    full_range_noise          2.23e-07   4.07e-07   4.07e-07 (148)
    zeros_voiced_zeros         1.4e-07    2.6e-07    2.6e-07 (77)
Two misses, kept as strict expected failures below: f0_45 misses (iii) (3.05e-5 > 2.89e-5) and glide_80_600 misses (ii) (1.08e-5 on a
frame whose e_ref is <= 1e-6); gated_voiced, octave_jumps and glide_80_600 pass (iii) only through its 8 x e_ref term.
Before the third central moment of lld_compare_frame* was added bin after bin, (a) failed on clicks_in_zeros in all three forms:
17 (block form: 14) of 284 700 cells, pcm_fftMag_spectralSkewness_sma and its delta, from frame 13 on (the first full-scale click).
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import hard_signals, hard_signals_run
from test_gpu_funcspec import LIBM, as_oracle_spec
from test_oracle_pin_funcspec import pending
from test_oracle_pin_hard_signals import compare16_func_from_lld, load, same_or_both_zero
from tolerance import RTOL, record

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = hard_signals.NAMES
# (set, form) -> the switches of that form; "fast" = lld_mfcc512 with its own transform order, everything else reference order
FORMS = {("mfcc", "generic"): {"SMILEHIP_FORCE_GENERIC": "1"}, ("plp", "generic"): {"SMILEHIP_FORCE_GENERIC": "1"},
         ("mfcc", "fast"): {}, ("plp", "fast"): {},
         ("is09", "default"): {}, ("is09", "block"): {"SMILEHIP_IS09": "block"},
         ("compare16", "default"): {}, ("compare16", "wave"): {"SMILEHIP_COMPARE_WAVE": "1"},
         ("compare16", "block"): {"SMILEHIP_COMPARE_BLOCK": "1"},
         ("egemaps", "default"): {}, ("egemaps", "wave"): {"SMILEHIP_GEMAPS_WAVE": "1"}}
REFERENCE_ORDER = [k for k in FORMS if k[1] != "fast"]
FIXTURE = {"mfcc": ("hard_mfcc_plp", "mfcc_"), "plp": ("hard_mfcc_plp", "plp_"), "is09": ("hard_is09", "lld_"),
           "compare16": ("hard_compare16", "lld_"), "egemaps": ("hard_egemaps", "lld_")}
_RUNS = {}


def run(set_name, form, order="forward"):
    """One batch run per (set, form, order) for the whole module (hard_signals_run.run); SMILEHIP_COMPARE_BLOCK is read once per
    process, so that form runs in a child."""
    key = (set_name, form, order)
    if key not in _RUNS:
        if "SMILEHIP_COMPARE_BLOCK" in FORMS[set_name, form]:
            import tempfile
            with tempfile.TemporaryDirectory() as td:
                out = os.path.join(td, "run.npz")
                env = dict(os.environ)
                env.update(FORMS[set_name, form])
                r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "helpers", "hard_signals_run.py"), set_name, order, out],
                                   env=env, capture_output=True, text=True, timeout=300)
                assert r.returncode == 0, r.stderr[-2000:]
                with np.load(out) as z:
                    _RUNS[key] = {k: z[k] for k in z.files}
        else:
            _RUNS[key] = hard_signals_run.run(set_name, order, FORMS[set_name, form])
        _RUNS[key]["ran"] = {str(k) for k in _RUNS[key]["ran"]}
    return _RUNS[key]


def rows_of(res, order="forward"):
    """{signal name: its rows} of a run."""
    utts = hard_signals_run.batch_of(order)
    return {n: res["lld"][res["rows"][i]:res["rows"][i + 1]] for i, (n, _) in enumerate(utts) if n}


def func_of(res, order="forward"):
    utts = hard_signals_run.batch_of(order)
    return {n: res["func"][i] for i, (n, _) in enumerate(utts) if n}


@pytest.fixture(scope="module")
def golden():
    return {s: load(s) for s in ("hard_mfcc_plp", "hard_is09", "hard_compare16", "hard_egemaps")}


@pytest.fixture(scope="module")
def sig():
    s = hard_signals.signals()
    z = load("hard_pcm")
    assert all(np.array_equal(s[n], z[n]) for n in NAMES)
    return s


def differing(same, name):
    d = np.argwhere(~same)
    return f"{name}: {len(d)} of {same.size} cells, columns {sorted(set(d[:, 1]))[:24]}, first differing frame {d[:, 0].min()}"


# ------------------------------------------------------------------ a. reference-order chains against the binary
@pytest.mark.parametrize("set_name,form", REFERENCE_ORDER)
def test_reference_order_chain_equals_binary(golden, set_name, form):
    res = run(set_name, form)
    assert np.isfinite(res["lld"]).all()
    if set_name in ("mfcc", "plp"):
        assert "lld_mfcc_generic" in res["ran"] and "lld_mfcc512" not in res["ran"], res["ran"]
    elif form != "default":
        assert res["ran"] != run(set_name, "default")["ran"], f"the switch of form '{form}' selected no other kernel: {res['ran']}"
    stem, prefix = FIXTURE[set_name]
    bad, cells, identical = [], 0, 0
    for name, got in rows_of(res).items():
        ref = golden[stem][prefix + name]
        assert got.shape == ref.shape, (name, got.shape, ref.shape)
        same = same_or_both_zero(got, ref) if set_name == "egemaps" else got.view(np.uint32) == ref.view(np.uint32)
        cells += same.size
        identical += int(same.sum())
        if not same.all():
            bad.append(differing(same, name))
    record("hard_signals_bits", what=f"{set_name}/{form}", cells=cells, identical=identical / cells)
    assert not bad, f"{set_name}/{form} differs from the binary: " + "; ".join(bad)


# ------------------------------------------------------------------ b. functionals
def check_func16(dev, ref, names, what):
    lib = np.array([n in LIBM for n in names])
    d = (dev.view(np.uint32) != ref.view(np.uint32)) & ~lib
    assert not d.any(), f"{what}: {[(int(i), names[i]) for i in np.flatnonzero(d)[:8]]} ({int(d.sum())} values)"
    err = np.abs(dev[lib].astype(np.float64) - ref[lib]) / np.maximum(np.abs(ref[lib]), 1e-6)
    assert err.max() <= 1e-6, f"{what}: libm-dependent value off by {err.max():.3g}"


@pytest.mark.parametrize("form", ["default", "wave", "block"])
def test_compare16_functionals_vs_oracle_and_binary(golden, oracle, sig, form):
    """The 6373 values from the device's own LLD matrix: oracle.funcspec on the same matrix with the row rules of
    test_oracle_pin_funcspec.py (bits outside LIBM, those 1e-6), and -- the LLD being the binary's (a) -- the binary's vector."""
    from opensmile_amd import capi
    res = run("compare16", form)
    lld, func = rows_of(res), func_of(res)
    assert res["func"].shape == (len(NAMES), 6373) and np.isfinite(res["func"]).all()
    degenerate = 0
    for i, name in enumerate(NAMES):
        T, P = pending(oracle, sig[name])
        assert lld[name].shape[0] == T + 1
        ref, names = compare16_func_from_lld(oracle, lld[name], res["b_extra"][i], T, P,
                                             spec_of=lambda inst: as_oracle_spec(oracle, capi.funcspec_compare16(inst)))
        check_func16(func[name], ref, names, f"{name} ({form}) against the oracle on the device's LLD")
        check_func16(func[name], golden["hard_compare16"]["func_" + name], names, f"{name} ({form}) against the binary")
        degenerate += int(not lld[name][:, 0].any())
    assert degenerate == 7                              # all-unvoiced F0 contours: what makes this corpus worth having


@pytest.mark.parametrize("form", ["default", "wave"])
def test_egemaps_functionals_vs_binary(golden, form):
    func = func_of(run("egemaps", form))
    for name in NAMES:
        ref = golden["hard_egemaps"]["func_" + name]
        same = same_or_both_zero(func[name][None, :], ref)
        assert same.all(), f"{name} ({form}): functionals {np.flatnonzero(~same[0])} differ from the binary's"


@pytest.mark.parametrize("form", ["default", "block"])
def test_is09_functionals_vs_binary(golden, form):
    """functionals_host on the device's LLD matrix (the binary's, a): the binary's 384 values bit for bit -- none of IS09's twelve
    functionals goes through libm (tests/test_gpu_func.py)."""
    func = func_of(run("is09", form))
    for name in NAMES:
        ref = golden["hard_is09"]["func_" + name][0]
        d = func[name].view(np.uint32) != ref.view(np.uint32)
        assert not d.any(), f"{name} ({form}): LLD column / functional {[(int(j) // 12, int(j) % 12) for j in np.flatnonzero(d)[:8]]}"


# ------------------------------------------------------------------ c. batch composition
@pytest.mark.parametrize("set_name,form", [("mfcc", "generic"), ("mfcc", "fast"), ("plp", "generic"), ("plp", "fast"), ("is09", "default"),
                                           ("compare16", "default"), ("egemaps", "default")])
def test_rows_do_not_depend_on_the_batch_around_them(set_name, form):
    a, b = run(set_name, form), run(set_name, form, "mixed")
    utts = hard_signals_run.batch_of("mixed")
    assert a["ran"] == b["ran"]
    for i, (n, p) in enumerate(utts):
        if n is None:
            assert b["rows"][i + 1] == b["rows"][i], f"an utterance of {len(p)} samples has rows"
            assert "func" not in b or not b["func"][i].any()
    ra, rb = rows_of(a), rows_of(b, "mixed")
    for n in NAMES:
        assert ra[n].shape == rb[n].shape and ra[n].shape[0] > 100
        same = ra[n].view(np.uint32) == rb[n].view(np.uint32)
        assert same.all(), f"{set_name}/{form} " + differing(same, n)
    if "func" in a:
        fa, fb = func_of(a), func_of(b, "mixed")
        for n in NAMES:
            d = fa[n].view(np.uint32) != fb[n].view(np.uint32)
            assert not d.any(), f"{set_name}/{form} {n}: functionals {np.flatnonzero(d)[:10]} depend on the batch"


# ------------------------------------------------------------------ d. the fast kernels
def per_frame_err(out, ref, block):
    """tolerance.frame_scaled_err per frame: max over ALL columns of |out - ref| on the scale of the frame's static block."""
    return hard_signals.frame_scaled(np.asarray(out, np.float64) - ref, ref[:, :block])


@pytest.fixture(scope="module")
def reference_rounding(oracle, sig):
    oracle.use_reference_fft(False)
    return {n: hard_signals.e_ref(oracle, sig[n]) for n in NAMES}


@pytest.mark.parametrize("set_name,block", [("mfcc", 13), ("plp", 6)])
def test_fast_kernel_ran_finite_zero_rows_and_regression_bits(golden, oracle, set_name, block):
    """(i) and (iv) for lld_mfcc512 in its MFCC and PLP instances."""
    res = run(set_name, "fast")
    assert "lld_mfcc512" in res["ran"] and "lld_mfcc_generic" not in res["ran"], res["ran"]
    assert np.isfinite(res["lld"]).all()
    for name, out in rows_of(res).items():
        ref = golden["hard_mfcc_plp"][FIXTURE[set_name][1] + name]
        assert out.shape == ref.shape
        zero = ~ref.any(axis=1)
        assert not out[zero].any(), f"{name}: {int(out[zero].any(axis=1).sum())} frames are not zero where the reference row is all zero"
        de = oracle.delta_chain(np.ascontiguousarray(out[:, :block]), 2, 2)
        for k in (0, 1):
            got = np.ascontiguousarray(out[:, block * (k + 1):block * (k + 2)])
            same = got.view(np.uint32) == de[k].view(np.uint32)
            assert same.all(), f"{set_name} regression order {k + 1} " + differing(same, name)


@pytest.fixture(scope="module")
def fast_mfcc_errors(golden, reference_rounding):
    """{signal: (max e_ref, largest error over the non-zero frames, largest error over those with e_ref <= 1e-6)} of lld_mfcc512."""
    res = run("mfcc", "fast")
    assert "lld_mfcc512" in res["ran"] and "lld_mfcc_generic" not in res["ran"], res["ran"]
    table = {}
    for name, out in rows_of(res).items():
        r = reference_rounding[name]
        assert np.array_equal(r["out"].view(np.uint32), golden["hard_mfcc_plp"]["mfcc_" + name].view(np.uint32))
        err, nz = per_frame_err(out, r["out"], 13)
        quiet = nz & (r["e"] <= 1e-6)
        table[name] = (float(r["e"].max()), float(err[nz].max()) if nz.any() else 0.0, float(err[quiet].max()) if quiet.any() else 0.0,
                       int(np.argmax(err)), int(np.argmax(np.where(quiet, err, 0.0))))
        print(f"{name:24s} max e_ref {table[name][0]:.3g}  lld_mfcc512 {table[name][1]:.3g}  on its {int(quiet.sum())} frames with e_ref <= 1e-6: {table[name][2]:.3g}")
        record("hard_signals_fast_mfcc", signal=name, max_e_ref=table[name][0], err=table[name][1], err_quiet_frames=table[name][2])
    return table


# A miss of (ii) or (iii) is a finding about the accuracy of lld_mfcc512's own transform on signals whose upper mel bands hold nothing
# but the transform's rounding; each stays a STRICT expected failure that names the signal and the measured error until the
# transform is more accurate (no bound, reference or case was changed to make room for it).
MISSES_II = {"glide_80_600": "lld_mfcc512 on glide_80_600: 1.08e-5 > 1e-5 on frame 84, whose e_ref is <= 1e-6"}
MISSES_III = {"f0_45": "lld_mfcc512 on f0_45: 3.05e-5 on frame 12 > max(1e-5, 8 x 3.61e-6) = 2.89e-5"}


def cases(misses):
    return [pytest.param(n, marks=pytest.mark.xfail(strict=True, reason=misses[n])) if n in misses else n for n in NAMES]


@pytest.mark.parametrize("name", cases(MISSES_II))
def test_fast_mfcc_holds_the_project_gate_where_the_reference_is_quiet(fast_mfcc_errors, name):
    """(ii) On the frames whose e_ref is <= 1e-6 the project's unchanged gate: per-frame-scaled error against the oracle <= 1e-5."""
    e_ref, err, err_quiet, _, frame = fast_mfcc_errors[name]
    assert err_quiet <= RTOL, f"{name}: {err_quiet:.3g} > 1e-5 on frame {frame}, whose e_ref is <= 1e-6"


@pytest.mark.parametrize("name", cases(MISSES_III))
def test_fast_mfcc_within_eight_times_the_references_own_rounding(fast_mfcc_errors, name):
    """(iii) Per signal the largest per-frame-scaled error over its non-zero frames <= max(1e-5, 8 x max e_ref)."""
    e_ref, err, _, frame, _ = fast_mfcc_errors[name]
    bound = max(RTOL, 8 * e_ref)
    assert err <= bound, f"{name}: {err:.3g} on frame {frame} > {bound:.3g} = max(1e-5, 8 x {e_ref:.3g})"


# ------------------------------------------------------------------ e. the two front doors
REF = os.path.join(ROOT, "oracle", "_ref", "SMILExtract")
REF_CONF = os.path.join(ROOT, "oracle", "_ref", "config")
EXE = os.path.join(ROOT, "opensmile_amd", "smilextract_hip")
PLUGDIR = os.path.join(ROOT, "opensmile_amd", "plugin")


@pytest.mark.parametrize("set_name,conf,opts", [
    ("mfcc12_0_d_a", "mfcc/MFCC12_0_D_A.conf", ["-O"]),
    ("is09_emotion", "is09-13/IS09_emotion.conf", ["-lldhtkoutput", "-htkoutput"]),
    ("compare16", "compare16/ComParE_2016.conf", ["-lldhtkoutput", "-htkoutput"]),
    ("egemapsv02", "egemaps/v02/eGeMAPSv02.conf", ["-lldhtkoutput", "-htkoutput"]),
])
def test_smilextract_hip_file_list_equals_binary(oracle, sig, tmp_path, set_name, conf, opts):
    """A file list of the fifteen WAVs: every HTK file smilextract_hip writes is the binary's, byte for byte."""
    if not (os.path.exists(REF) and os.path.exists(EXE) and os.path.isdir(REF_CONF)):
        pytest.skip("oracle/_ref/SMILExtract (+ config/) or smilextract_hip not built")
    wavs = []
    for name in NAMES:
        wavs.append(str(tmp_path / (name + ".wav")))
        oracle.write_wav(wavs[-1], sig[name])
        args = [REF, "-C", os.path.join(REF_CONF, conf), "-I", wavs[-1], "-l", "0"]
        for o in opts:
            args += [o, str(tmp_path / f"ref_{name}{o}.htk")]
        subprocess.run(args, check=True, cwd=str(tmp_path), stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=120)
    lst = tmp_path / "list.txt"
    lst.write_text("".join(w + "\n" for w in wavs))
    outdir = tmp_path / "own"
    outdir.mkdir()
    args = [EXE, "--set", set_name, "-filelist", str(lst), "-outdir", str(outdir)]
    for o in opts:
        args += [o, "on"]
    env = dict(os.environ)
    if opts == ["-O"]:
        env["SMILEHIP_FORCE_GENERIC"] = "1"             # byte identity is the reference-order kernel's property (tests/test_gpu_rates.py)
    r = subprocess.run(args, capture_output=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    ext = {"-O": ".htk", "-lldhtkoutput": ".lld.htk", "-htkoutput": ".func.htk"}
    bad = []
    for name in NAMES:
        for o in opts:
            ref = open(tmp_path / f"ref_{name}{o}.htk", "rb").read()
            own = open(outdir / (name + ext[o]), "rb").read()
            assert len(ref) > 12
            if own != ref:
                bad.append(f"{name} {o} ({len(own)} vs {len(ref)} bytes)")
    assert not bad, f"{set_name}: files differ from the binary's: {bad}"


@pytest.mark.parametrize("conf", ["compare16/ComParE_2016.conf", "egemaps/v02/eGeMAPSv02.conf"])
def test_plugin_on_the_concatenated_corpus_equals_binary(oracle, sig, tmp_path, conf):
    """The unmodified binary with the plugin on ONE 22.5 s WAV of the fifteen signals back to back (the seams between the signal
    classes are themselves hard): fused (the default, SMILEHIP_PLUGIN_FUSE removed) and with the components kept apart
    (SMILEHIP_PLUGIN_FUSE=0) the LLD and functionals files are the plain binary's byte for byte, no frame on the CPU code."""
    plug = os.path.join(PLUGDIR, "plugins", "libsmilehip_plugin.so")
    if not (os.path.exists(REF) and os.path.exists(plug)):
        pytest.skip("oracle/_ref/SMILExtract or the plugin .so not built")
    wav = str(tmp_path / "all.wav")
    oracle.write_wav(wav, np.concatenate([sig[n] for n in NAMES]))
    files = {}
    for tag, switches in (("cpu", {"SMILEHIP_PLUGIN_COMPONENTS": "none"}), ("fused", {}), ("apart", {"SMILEHIP_PLUGIN_FUSE": "0"})):
        env = dict(os.environ)
        env.pop("SMILEHIP_PLUGIN_FUSE", None)
        env["LD_LIBRARY_PATH"] = os.pathsep.join([os.path.join(ROOT, "opensmile_amd"), oracle.REF_DIR, env.get("LD_LIBRARY_PATH", "")])
        lld, func, trace = (str(tmp_path / f"{tag}.{e}") for e in ("lld.htk", "func.htk", "trace.txt"))
        env["SMILEHIP_PLUGIN_TRACE"] = trace
        env.update(switches)
        r = subprocess.run([REF, "-C", os.path.join(REF_CONF, conf), "-I", wav, "-lldhtkoutput", lld, "-htkoutput", func, "-l", "1"],
                           cwd=PLUGDIR, env=env, capture_output=True, text=True, errors="replace", timeout=300)
        assert r.returncode == 0 and os.path.exists(lld) and os.path.exists(func), (tag, r.stderr[-2000:])
        tr = {k: int(v) for k, v in (l.split() for l in open(trace) if len(l.split()) == 2)} if os.path.exists(trace) else {}
        files[tag] = (open(lld, "rb").read(), open(func, "rb").read(), tr)
    assert len(files["cpu"][0]) > 12 + 2200 * 25 * 4 and len(files["cpu"][1]) > 12 and not any(files["cpu"][2].values())
    for tag in ("fused", "apart"):
        lld, func, tr = files[tag]
        assert not [n for n, v in tr.items() if n.endswith(".cpu") and v], (tag, tr)
        assert (tr.get("fused.rows", 0) > 0) == (tag == "fused"), (tag, tr)
        assert tag == "fused" or tr.get("cTransformFFT", 0) > 0, tr
        assert lld == files["cpu"][0], f"{tag}: the LLD file differs from the plain binary's"
        assert func == files["cpu"][1], f"{tag}: the functionals file differs from the plain binary's"
