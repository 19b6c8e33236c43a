"""config/spectrum/spectrogram.conf without a GPU: the g++ build of the row functions (opensmile_amd/csrc/lld_spectrogram_ops.hpp through
tests/helpers/spectrogram_check.cpp) against the real binary's levels bit for bit in all five forms and at all rates, the measured
row rule and row times, the C ABI's new exports on host-only plans, and the front end's mapping, names and refusals."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from helpers import spectrogram_host as SH

ROOT = SH.ROOT
EXE = os.path.join(ROOT, "opensmile_amd", "smilextract_hip")
REF_CONF = os.path.join(ROOT, "oracle", "_ref", "config", "spectrum", "spectrogram.conf")
SYNTH, RATES = "spectrogram_synth.npz", "spectrogram_rates.npz"
# 25 ms / 10 ms at every rate: frame, step, transform (what the framer's rounding gives)
GEOMETRY = {8000: (200, 80, 256), 11025: (276, 110, 512), 16000: (400, 160, 512), 22050: (551, 221, 1024), 32000: (800, 320, 1024),
            44100: (1103, 441, 2048), 48000: (1200, 480, 2048)}
FLOOR = np.float32(-120.0) + np.float32(90.302)            # mindBp behind the clamp at the component's defaults


@pytest.fixture(scope="module")
def capi():
    from opensmile_amd import capi as m
    m.load()
    return m


def same(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and bool((a.view(np.uint32) == b.view(np.uint32)).all())


# ------------------------------------------------------------------------------------------------ the fixtures
def test_fixtures_hold_what_the_issue_lists():
    c16, cr = SH.cases(SYNTH), SH.cases(RATES)
    N, H = 400, 160
    for form in ("mag", "db"):
        lens = sorted(c[2] for c in c16 if c[4] == form and c[5] == 1)
        assert lens == sorted([0, N - 1, N, N + H - 1, N + H] + [N + H * (T - 1) for T in (3, 4, 5, 9, 17)])
    assert sorted(c[4] for c in c16 if c[2] == 1040 and c[5] == 1) == sorted(SH.FORMS)
    assert sorted(c[4] for c in c16 if c[5] == 0) == ["db", "mag"]
    assert sorted({c[3] for c in cr if c[6] == 0.025}) == [8000, 11025, 22050, 32000, 44100, 48000]
    assert sorted({(c[3], c[6], c[7]) for c in cr if c[6] != 0.025}) == [(8000, 0.008, 0.01), (16000, 0.0405, 0.004), (32000, 0.2, 0.01)]
    for name in (SYNTH, RATES):
        f = SH.fixture(name)
        for c in SH.cases(name):
            assert "lld_" + c[0] in f.files
    for name in (SYNTH, RATES, "hard_spectrogram.npz"):
        assert os.path.getsize(os.path.join(SH.GOLDEN, name)) < 1 << 20
    assert list(SH.fixture(SYNTH)["htk_header"][1:]) == [100000, 4 * 257, 9]


def test_hard_signal_fixture_sits_on_the_floor():
    from helpers import hard_signals
    h = SH.fixture("hard_spectrogram.npz")
    seg = {str(r[0]): (int(r[1]), int(r[2])) for r in h["segments"]}
    assert sorted(seg) == sorted(hard_signals.NAMES) and all(0 < n <= 4000 for _, n in seg.values())
    for n in hard_signals.NAMES:
        for form in ("mag", "db"):
            assert h["lld_%s_%s" % (form, n)].shape == ((seg[n][1] - 400) // 160 + 1, 257)
    # digital zeros and +-1 LSB noise land on the mindBp floor in the dB form
    for n in ("lsb_noise", "clicks_in_zeros", "zeros_voiced_zeros"):
        cells = int((h["lld_db_" + n] == FLOOR).sum())
        assert cells > 0 and cells == int(h["floor_cells"][hard_signals.NAMES.index(n)]), n
    assert not any(np.isnan(h["lld_db_" + n]).any() for n in hard_signals.NAMES)
    assert all((h["lld_db_" + n] >= FLOOR).all() for n in hard_signals.NAMES)


# ------------------------------------------------------------------------------------------------ the row functions against the binary
@pytest.mark.parametrize("name", [SYNTH, RATES])
def test_row_functions_equal_the_binarys_lld_level(name):
    """the binary's fft level (a cHtkSink tap) through the host build equals the binary's lld level, in all five forms, at all rates"""
    f = SH.fixture(name)
    seen = set()
    for key, idx, n, fs, form, zps, fsz, fst in SH.cases(name):
        lld, fft = f["lld_" + key], SH.fft_of(name, key)
        if not len(lld) or fft is None:
            continue
        assert fft.shape == (len(lld), 2 * (lld.shape[1] - 1))
        assert same(SH.spectrum_rows(fft, form), lld), key
        seen.add((fs, form, fft.shape[1]))
    if name == SYNTH:
        assert {s[1] for s in seen} == set(SH.FORMS)
    else:
        assert {s[0] for s in seen} == {8000, 11025, 16000, 22050, 32000, 44100, 48000} and {s[2] for s in seen} == {64, 256, 512, 1024, 2048, 8192}


def test_db_form_floor_nan_and_clamp():
    """MAX(mindBp, v) as the component orders it: zeros land on the floor, a NaN value passes through, the clamp is the component's"""
    fft = np.zeros((1, 64), np.float32)
    fft[0, 4] = np.nan
    fft[0, 1] = np.inf
    out = SH.spectrum_rows(fft, "db")
    assert out[0, 0] == FLOOR and out[0, 1] == FLOOR and np.isnan(out[0, 2]) and out[0, 32] == np.inf
    assert SH.spectrum_rows(fft, "db", 90.302, -20.0)[0, 0] == np.float32(-20.0)      # above dBpnorm - 120: kept
    assert SH.clamp_bits(90.302, -102.0) == int(np.array(FLOOR).view(np.uint32)) and SH.clamp_bits(0.0, -120.0) == int(np.float32(-120.0).view(np.uint32))
    assert SH.clamp_bits(90.302, -29.0) == int(np.float32(-29.0).view(np.uint32))
    assert [SH.form_of_flags(SH.FLAGS[f]) for f in ("mag", "norm", "pow", "normpow", "db")] == [0, 1, 2, 3, 4]
    assert SH.form_of_flags(1 | 4 | 8 | 16) == 4 and SH.form_of_flags(4) == -1 and SH.form_of_flags(3) == -1


# ------------------------------------------------------------------------------------------------ rows, times, preset, exports
def test_row_rule_and_times_are_the_measured_ones(capi):
    L = capi.load()
    for name in (SYNTH, RATES):
        f = SH.fixture(name)
        for key, idx, n, fs, form, zps, fsz, fst in SH.cases(name):
            p = capi.Plan(None, SH.config(fs, zps, fsz, fst))
            g = p.geometry
            rows = len(f["lld_" + key])
            assert rows == p.num_frames(n) == SH.rows_of(n, g.frame_size, g.frame_step), key
            if rows:
                assert f["lld_" + key].shape[1] == g.n_bins == g.n_static == g.n_out == g.fft_size // 2 + 1
            if "times_" + key in f.files:                   # the CSV sink's frameTime column (six decimals): t * H / fs
                want = f["times_" + key]
                got = [L.smilehip_row_time(p._h, rows, t) for t in range(rows)]
                assert len(want) == rows and np.allclose(got, want, atol=5.1e-7), key
                assert got == [t * g.frame_step / fs for t in range(rows)]
            p.close()
    p = capi.Plan(None, capi.spectrogram_config())
    for n, want in ((0, 0), (399, 0), (400, 1), (559, 1), (560, 2), (160000, 998)):
        assert p.num_frames(n) == want == SH.rows_of(n, 400, 160)


def test_preset_values_size_and_exports(capi):
    L = capi.load()
    assert capi.CHAIN_SPECTROGRAM == 12 and capi.LLD_CONFIG_SIZE_V1 == 280
    hdr = open(os.path.join(ROOT, "include", "smilehip.h")).read()
    assert "#define SMILEHIP_CHAIN_SPECTROGRAM 12" in hdr and "void smilehip_config_spectrogram(smilehip_lld_config *c);" in hdr
    assert "int smilehip_plan_set_spectrum_form(smilehip_plan *plan, int32_t flags, float dbp_norm, float min_dbp);" in hdr
    for sym in ("smilehip_config_spectrogram", "smilehip_plan_set_spectrum_form", "smilehip_plan_get_spectrum_form"):
        assert sym in capi.SYMBOLS and hasattr(L, sym)
    for k, v in (("MAGNITUDE", 1), ("PHASE", 2), ("NORMALISE", 4), ("POWER", 8), ("DBPSD", 16)):
        assert getattr(capi, "MAGPHASE_" + k) == v and re.search(r"#define SMILEHIP_MAGPHASE_%s %d\b" % (k, v), hdr)

    class Guarded(C.Structure):
        _fields_ = [("cfg", capi.LldConfig), ("guard", C.c_ubyte * 64)]
    g = Guarded()
    C.memset(C.byref(g), 0xA5, C.sizeof(g))
    L.smilehip_config_spectrogram(C.cast(C.byref(g), C.POINTER(capi.LldConfig)))
    c = g.cfg
    assert c.struct_size == 280 and bytes(g.guard) == b"\xa5" * 64            # exactly V1 bytes, nothing behind them
    assert (c.chain_kind, c.zero_pad_symmetric, c.n_delta, c.preemph, c.win_func) == (12, 1, 0, 0, 2)
    assert (c.frame_size_sec, c.frame_step_sec, c.win_gain, c.win_offset, c.append_log_energy, c.cms, c.stage_mask) == (0.025, 0.010, 1.0, 0.0, 0, 0, 0)
    c = capi.spectrogram_config(22050.0, 0.05, 0.02)
    assert (c.sample_rate, c.frame_size_sec, c.frame_step_sec) == (22050.0, 0.05, 0.02) and capi.spectrogram_config().sample_rate == 16000.0


@pytest.mark.parametrize("fs", sorted(GEOMETRY))
def test_geometry_at_every_rate(capi, fs):
    N, H, nfft = GEOMETRY[fs]
    g = capi.Plan(None, capi.spectrogram_config(fs)).geometry
    assert (g.frame_size, g.frame_step, g.fft_size, g.n_bins, g.n_static, g.n_out) == (N, H, nfft, nfft // 2 + 1, nfft // 2 + 1, nfft // 2 + 1)


def test_spectrum_form_on_a_host_only_plan(capi):
    p = capi.Plan(None, capi.spectrogram_config())
    assert p.spectrum_form() == (1, float(np.float32(90.302)), float(FLOOR))           # a fresh plan: plain magnitude, the defaults clamped
    for form in SH.FORMS:
        p.set_spectrum_form(SH.FLAGS[form])
        flags = p.spectrum_form()[0]
        assert flags & ~4 == SH.FLAGS[form] & ~4 and bool(flags & 4) == (form in ("norm", "normpow", "db"))
    p.set_spectrum_form(1 | 16, 0.0, -200.0)                # the mindBp clamp, as the component applies it
    assert p.spectrum_form() == (21, 0.0, -120.0)
    p.set_spectrum_form(1 | 16, 90.302, -29.0)
    assert p.spectrum_form()[2] == float(np.float32(-29.0))
    p.set_spectrum_form(1 | 4 | 8 | 16)                     # dBpsd wins over power
    assert p.spectrum_form()[0] == 21
    for flags, word in ((1 | 2, "PHASE"), (2, "PHASE"), (0, "MAGNITUDE"), (4 | 8, "MAGNITUDE"), (1 | 32, "flag bits")):
        with pytest.raises(RuntimeError, match=word):
            p.set_spectrum_form(flags)
    assert p.spectrum_form()[0] == 21                       # a refused call changes nothing
    with pytest.raises(RuntimeError, match="not a number"):
        p.set_spectrum_form(1 | 16, float("nan"))
    for other in (capi.audspec_config(), capi.mfcc12_0_d_a_config(), capi.chroma_fft_config()):
        q = capi.Plan(None, other)
        with pytest.raises(RuntimeError, match="not a spectrogram plan"):
            q.set_spectrum_form(1)
        with pytest.raises(RuntimeError, match="not a spectrogram plan"):
            q.spectrum_form()


def test_every_plan_refusal_names_its_parameter(capi):
    for field, value, word in (("stage_mask", 3, "stage_mask"), ("n_delta", 1, "n_delta"), ("preemph", 1, "preemph"),
                               ("append_log_energy", 1, "append_log_energy"), ("cms", 1, "cms")):
        c = capi.spectrogram_config()
        setattr(c, field, value)
        with pytest.raises(RuntimeError, match="spectrogram chain: " + word):
            capi.Plan(None, c)
    with pytest.raises(RuntimeError, match="64 .. 8192 points.*gives 32"):           # 2 ms at 16 kHz: 32 points
        capi.Plan(None, capi.spectrogram_config(16000.0, 0.002))
    with pytest.raises(RuntimeError, match="16384"):                                 # 0.6 s at 16 kHz
        capi.Plan(None, capi.spectrogram_config(16000.0, 0.6))
    assert capi.Plan(None, capi.spectrogram_config(8000.0, 0.008)).geometry.fft_size == 64
    assert capi.Plan(None, capi.spectrogram_config(32000.0, 0.2)).geometry.fft_size == 8192
    c = capi.spectrogram_config()                           # the struct sizes the library accepts have not changed
    c.struct_size = 284
    with pytest.raises(RuntimeError, match="struct_size"):
        capi.Plan(None, c)


def test_names_per_form_equal_the_binarys_headers():
    f = SH.fixture(SYNTH)
    for form in SH.FORMS:
        assert str(f["csv_header_" + form]).split(";") == ["name", "frameTime"] + ["%s[%d]" % (SH.FIELD[form], k) for k in range(257)]
    src = open(os.path.join(ROOT, "opensmile_amd", "host", "feature_names.cpp")).read()
    assert "lld_names_spectrogram" in src and all('"%s"' % SH.FIELD[form] in open(os.path.join(ROOT, "opensmile_amd", "host", "conf_plan.cpp")).read() for form in SH.FORMS)


# ------------------------------------------------------------------------------------------------ the front end (no device needed)
needs_exe = pytest.mark.skipif(not os.path.exists(EXE), reason="smilextract_hip not built")


def describe(*args):
    r = subprocess.run([EXE, "--set", "spectrogram", *args, "--describe"], capture_output=True, text=True)
    kv = dict(ln.split("=", 1) for ln in r.stdout.split("\n") if "=" in ln)
    return r.returncode, kv, r.stderr


def write_conf(tmp_path, text, name="s.conf"):
    p = tmp_path / name
    p.write_text(text)
    return str(p)


@needs_exe
def test_set_describes_its_form_and_geometry():
    rc, kv, err = describe()
    assert rc == 0, err
    assert (kv["preset"], kv["chain_kind"], kv["spectrum_flags"], kv["spectrum_field"], kv["parm_kind"]) == ("spectrogram", "12", "1", "pcm_fftMag", "9")
    assert (float(kv["frame_size_sec"]), float(kv["frame_step_sec"]), kv["zero_pad_symmetric"], kv["win_func"]) == (0.025, 0.010, "1", "2")
    rc, kv, err = describe("-dB", "1", "-frameSize", "0.0405", "-frameStep", "0.004")
    assert rc == 0, err
    assert (kv["spectrum_flags"], kv["spectrum_field"], float(kv["frame_size_sec"]), float(kv["frame_step_sec"])) == ("21", "pcm_fftMag_dBsplPSD", 0.0405, 0.004)
    assert float(kv["dbp_norm"]) == pytest.approx(90.302) and float(kv["min_dbp"]) == -102.0


@needs_exe
def test_minimal_text_and_its_options_map_to_the_chain(tmp_path):
    conf = write_conf(tmp_path, SH.MINIMAL)
    rc, kv, err = describe("-C", conf)
    assert rc == 0, err
    assert (kv["preset"], kv["chain_kind"], kv["spectrum_flags"], kv["names"], kv["parm_kind"]) == ("", "12", "1", "pcm_fftMag", "9")
    assert (float(kv["frame_size_sec"]), float(kv["frame_step_sec"]), kv["zero_pad_symmetric"], kv["win_func"], kv["preemph"], kv["n_delta"]) == \
        (0.025, 0.010, "1", "2", "0", "0")
    rc, kv, err = describe("-C", conf, "-dB", "1", "-frameSize", "0.2", "-frameStep", "0.02")    # the file's own \cm options
    assert rc == 0, err
    assert (kv["spectrum_flags"], kv["spectrum_field"], float(kv["frame_size_sec"]), float(kv["frame_step_sec"])) == ("21", "pcm_fftMag_dBsplPSD", 0.2, 0.02)


EDITS_OK = {
    "norm": (SH.TEXT_EDITS["norm"], dict(spectrum_flags="5", spectrum_field="pcm_fftMag_SpecDens")),
    "pow": (SH.TEXT_EDITS["pow"], dict(spectrum_flags="9", spectrum_field="pcm_fftMag_PowSpec")),
    "normpow": (SH.TEXT_EDITS["normpow"], dict(spectrum_flags="13", spectrum_field="pcm_fftMag_PowSpecDens")),
    "zps0": (SH.TEXT_EDITS["zps0"], dict(zero_pad_symmetric="0")),
    "db_in_file": ({"dBpsd = \\cm[dB{0}:dB power spectral density]": "dBpsd = 1\ndBpnorm = 80\nmindBp = -30"},
                   dict(spectrum_flags="21", dbp_norm="80", min_dbp="-30")),
    "han": ({"winFunc = ham": "winFunc = han"}, dict(win_func="1")),
    "gauss": ({"winFunc = ham": "winFunc = gauss\nsigma = 0.3"}, dict(win_func="3", win_sigma="0.29999999999999999")),
    "gain": ({"gain = 1.0": "gain = 0.5"}, dict(win_gain="0.5")),
    "sizes": ({"{0.0250}": "{0.032}", "{0.010}": "{0.008}"}, dict(frame_size_sec="0.032000000000000001", frame_step_sec="0.0080000000000000002")),
}


@needs_exe
@pytest.mark.parametrize("tag", sorted(EDITS_OK))
def test_each_allowed_edit_shows_up(tmp_path, tag):
    edits, want = EDITS_OK[tag]
    rc, kv, err = describe("-C", write_conf(tmp_path, SH.minimal_text(edits)))
    assert rc == 0, err
    assert kv["chain_kind"] == "12"
    for k, v in want.items():
        assert kv[k] == v, (k, kv[k], v)


MAG = "writer.dmLevel = lld\n"
REFUSED = [
    ({MAG: MAG + "magnitude = 0\n"}, ["cFFTmagphase", "magnitude"]),
    ({MAG: MAG + "phase = 1\n"}, ["cFFTmagphase", "phase"]),
    ({MAG: MAG + "joinMagphase = 1\n"}, ["cFFTmagphase", "joinMagphase"]),
    ({MAG: MAG + "inverse = 1\n"}, ["cFFTmagphase", "inverse"]),
    ({"writer.dmLevel = fft\n": "writer.dmLevel = fft\ninverse = 1\n"}, ["cTransformFFT", "inverse"]),
    ({"frameMode = fixed": "frameMode = full"}, ["cFramer", "frameMode"]),
    ({"frameCenterSpecial = left": "frameCenterSpecial = mid"}, ["cFramer", "frameCenterSpecial"]),
    ({"winFunc = ham": "winFunc = blackman"}, ["cWindower", "winFunc"]),
    ({"offset = 0": "offset = 0\nfade = 1"}, ["cWindower", "fade"]),
    ({"offset = 0": "offset = 0\nalphas = 3"}, ["cWindower", "alphas"]),
    ({"instance[mag].type = cFFTmagphase": "instance[mag].type = cFFTmagphase\ninstance[en].type = cEnergy",
      "[out:cHtkSink]": "[en:cEnergy]\nreader.dmLevel = frames\nwriter.dmLevel = en\n[out:cHtkSink]"}, ["cEnergy", "spectrogram.conf"]),
    ({"[mag:cFFTmagphase]\nreader.dmLevel = fft": "[mag:cFFTmagphase]\nreader.dmLevel = winframes"}, ["reader.dmLevel", "winframes"]),
]


@needs_exe
@pytest.mark.parametrize("edit,words", REFUSED, ids=[w[1][1] + "_" + w[1][0] for w in REFUSED])
def test_each_refused_edit_names_its_option(tmp_path, edit, words):
    rc, kv, err = describe("-C", write_conf(tmp_path, SH.minimal_text(edit)))
    assert rc != 0 and all(w in err for w in words), err


@needs_exe
def test_set_options_refused_by_name(tmp_path):
    conf = write_conf(tmp_path, SH.MINIMAL)
    wav = os.path.join(SH.GOLDEN, "files", "u3_4000.wav")
    r = subprocess.run([EXE, "--set", "spectrogram"], capture_output=True, text=True)     # the set name is known: what is missing is the input
    assert r.returncode != 0 and "no input" in r.stderr, r.stderr
    for args, words in ((["--set", "spectrogram", "-frameMode", "fixed", "-I", wav], ["-frameMode fixed", "no functionals level"]),
                        (["--set", "spectrogram", "-arffoutput", "x.arff", "-I", wav], ["-arffoutput", "ARFF"]),
                        (["--set", "spectrogram", "-dB", "2", "-I", wav], ["-dB 2"]),
                        (["--set", "spectrogram", "-frameSize", "0", "-I", wav], ["-frameSize 0"]),
                        (["--set", "mfcc12_0_d_a", "-dB", "1", "-I", wav], ["-dB", "--set spectrogram"]),
                        (["--set", "spectrogram", "-C", conf, "-frameMode", "fixed", "-I", wav], ["-frameMode"]),
                        (["-C", conf, "-I", wav], ["cannot run on the fused path", "--set spectrogram -C"]),      # plain -C keeps refusing, and names the route
                        (["--set", "audspec", "-C", conf, "-I", wav], ["cMelspec"])):
        r = subprocess.run([EXE, *args], capture_output=True, text=True, cwd=str(tmp_path))
        assert r.returncode != 0 and all(w in r.stderr for w in words), (args, r.stderr)
    assert not (tmp_path / "x.arff").exists()


@needs_exe
@pytest.mark.skipif(not os.path.exists(REF_CONF), reason="the reference's configuration files are not here")
def test_shipped_file_is_recognised_under_the_set_and_refused_without():
    rc, kv, err = describe("-C", REF_CONF)
    assert rc == 0, err
    assert (kv["chain_kind"], kv["spectrum_flags"], kv["zero_pad_symmetric"], kv["parm_kind"], kv["win_func"]) == ("12", "1", "1", "9", "2")
    rc, kv, err = describe("-C", REF_CONF, "-dB", "1")
    assert rc == 0 and kv["spectrum_flags"] == "21", err
    r = subprocess.run([EXE, "-C", REF_CONF, "--describe"], capture_output=True, text=True)
    assert r.returncode != 0 and "cannot run on the fused path" in r.stderr and "--set spectrogram -C" in r.stderr, r.stderr
    r = subprocess.run([EXE, "--set", "spectrogram", "-C", REF_CONF, "-arffoutput", "x.arff", "--describe"], capture_output=True, text=True)
    assert r.returncode != 0 and "-arffoutput" in r.stderr, r.stderr
