"""config/audspec/audspec.conf as SMILEHIP_CHAIN_AUDSPEC, without a GPU: the g++ build of the row functions both forms of lld_audspec_frame
call (opensmile_amd/csrc/lld_audspec_ops.hpp through tests/helpers/audspec_host.py) equals the real binary's `melspec`, `plp` and `lld`
levels bit for bit -- the mel bands from the binary's own `fftmag` rows, the auditory spectrum from its `melspec` rows, the regression
stages from that --; what the fixture holds, the row rule as measured, the presets and their size, the geometry at every rate, the plan's
refusals, the names, and the front end's walker (`--set audspec -C file`) on a configuration text of the project's own."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from helpers import audspec_host as AH

ROOT = AH.ROOT
GOLD = AH.GOLDEN
EXE = os.path.join(ROOT, "opensmile_amd", "smilextract_hip")
REF_CONF = os.path.join(ROOT, "oracle", "_ref", "config", "audspec")
NAMES = ["audSpec%s[%d]" % (s, i) for s in ("", "_de", "_de_de") for i in range(26)]
# 25 ms / 10 ms at every rate: frame, step, transform (make_geometry: what the framer's rounding gives)
GEOMETRY = {8000: (200, 80, 256), 11025: (276, 110, 512), 16000: (400, 160, 512), 22050: (551, 221, 1024), 32000: (800, 320, 1024),
            44100: (1103, 441, 2048), 48000: (1200, 480, 2048)}


@pytest.fixture(scope="module")
def capi():
    from opensmile_amd import capi as m
    m.load()
    return m


@pytest.fixture(scope="module")
def gold():
    return AH.fixture()


def same(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and bool((a.view(np.uint32) == b.view(np.uint32)).all())


def levels_from(cfg, gold, suffix):
    """the binary's levels of one fixture entry against the host build: returns what was compared"""
    lld = gold["lld_" + suffix]
    nb = cfg.n_bands
    seen = []
    mel = gold["melspec_" + suffix] if "melspec_" + suffix in gold.files else None
    if "fftmag_" + suffix in gold.files and len(lld):
        assert same(AH.mel_rows(cfg, gold["fftmag_" + suffix]), mel), "melspec " + suffix
        seen.append("melspec")
    if mel is not None and len(lld):
        assert mel.shape == (len(lld), nb)
        aud = AH.aud_rows(cfg, mel)
        assert same(aud, lld[:, :nb]), "plp " + suffix           # (the plp level is the lld level's first block: make_golden_audspec.store)
        assert same(AH.lld_rows(aud, cfg.n_delta, cfg.delta_win), lld), "lld " + suffix
        seen += ["plp", "lld"]
    return seen


# ------------------------------------------------------------------------------------------------ the fixture
def test_fixture_holds_what_it_says(gold):
    inputs = gold["inputs"]
    assert len(inputs) == 22 and sorted(set(int(r[2]) for r in inputs)) == sorted(AH.RATES)
    for k, (idx, n, fs, div) in enumerate(inputs):
        N, H, _ = GEOMETRY[int(fs)]
        T = (int(n) - N) // H + 1 if n >= N else 0
        lld = gold["lld_%d" % k]
        assert lld.shape == ((T, 78) if T else (0, 0)), (k, lld.shape)
        assert np.isfinite(lld).all()
    # both branches of cPlp's floor (plp.cpp:502): the silence input sits on it in every band, the quiet one in a few, most bands do not
    sil, quiet = gold["melspec_14"], gold["melspec_15"]
    assert len(sil) and (sil < 1.0).all() and 0 < (quiet < 1.0).sum() < quiet.size
    on = sum(int((gold[f] < 1.0).sum()) for f in gold.files if f.startswith("melspec_"))
    off = sum(int((gold[f] >= 1.0).sum()) for f in gold.files if f.startswith("melspec_"))
    assert on > 0 and off > 4 * on
    # on the floor the band is pow(1.0 * eql, compression): the same in every frame
    assert (gold["lld_14"][:, :26] == gold["lld_14"][0, :26]).all() and (gold["lld_14"][:, 26:] == 0).all()
    assert [int(v) for v in gold["htk_header"]][1:] == [100000, 312, 9]      # 10 ms in 100 ns units, 78 floats, parmKind 9
    # the compat file differs from audspec.conf wherever the frame is zero-padded (all seven rates)
    for k in (5, 6, 7, 8, 9, 13, 16, 17, 18, 19, 20, 21):
        assert gold["lld_compat_%d" % k].shape == gold["lld_%d" % k].shape and not same(gold["lld_compat_%d" % k], gold["lld_%d" % k])
    # the inert options: lpOrder 8, firstCC 1, cepLifter 0 give the same bytes
    for k in AH.EDIT_INPUTS:
        assert same(gold["lld_inert_%d" % k], gold["lld_%d" % k])
        for tag in AH.EDITS:
            if tag != "inert":
                assert not same(gold["lld_%s_%d" % (tag, k)], gold["lld_%d" % k]), tag


def test_hard_signal_fixture_shape():
    from helpers import hard_signals
    h = AH.fixture("hard_audspec.npz")
    assert sorted(h.files) == sorted("lld_" + n for n in hard_signals.NAMES)
    for n in hard_signals.NAMES:
        assert h["lld_" + n].shape == (148, 78) and np.isfinite(h["lld_" + n]).all()      # 1.5 s: (24000 - 400) / 160 + 1 frames


# ------------------------------------------------------------------------------------------------ the row functions against the binary
@pytest.mark.parametrize("fs", AH.RATES)
def test_levels_at_every_rate(gold, fs):
    done = set()
    for k, row in enumerate(gold["inputs"]):
        if int(row[2]) == fs:
            done.update(levels_from(AH.config(fs), gold, str(k)))
    assert done == {"melspec", "plp", "lld"}


def test_levels_of_the_compat_file(gold):
    done = set()
    for k in (5, 6, 7, 8, 9, 13, 16, 17, 18, 19, 20, 21):
        fs = int(gold["inputs"][k][2])
        done.update(levels_from(AH.config(fs, compat=True), gold, "compat_%d" % k))
    assert done == {"melspec", "plp", "lld"}


@pytest.mark.parametrize("tag", sorted(AH.EDITS))
def test_levels_of_the_edited_copies(gold, tag):
    done = set()
    for k in AH.EDIT_INPUTS:
        cfg = AH.config(16000.0, **AH.EDITS[tag])
        done.update(levels_from(cfg, gold, "%s_%d" % (tag, k)))
        assert gold["lld_%s_%d" % (tag, k)].shape[1] == cfg.n_bands * (1 + cfg.n_delta)
    assert done == {"melspec", "plp", "lld"}


def test_frame_samples_are_the_reference_expressions():
    """audspec::frame_sample (both kernel forms' R2 / R3) against the expressions of lld_mfcc_generic, written out in numpy float32"""
    L = AH.load()
    rng = np.random.default_rng(5)
    x = (rng.integers(-32768, 32768, 400).astype(np.float32) / np.float32(32767.0)).astype(np.float32)
    win = rng.random(400).astype(np.float32)
    k, off = np.float32(0.97), np.float32(0.25)
    for preemph, de in ((1, 0), (1, 1), (0, 0)):
        y = np.zeros(400, np.float32)
        L.audspec_frame_samples(x.ctypes.data, win.ctypes.data, 400, preemph, de, float(k), float(off), y.ctypes.data)
        want = x.copy()
        if preemph:
            kp = (k * x[:-1]).astype(np.float32)
            want[1:] = (x[1:] + kp) if de else (x[1:] - kp)
            want[0] = (np.float32(1) - k) * x[0]
        want = ((want * win).astype(np.float32) + off).astype(np.float32)
        assert same(y, want), (preemph, de)


# ------------------------------------------------------------------------------------------------ rows, presets, geometry, refusals
def test_row_rule_is_the_measured_one(capi, gold):
    L = capi.load()
    h = C.c_void_p()
    c = capi.audspec_config(16000.0)
    capi._check(L.smilehip_plan_create_host_only(C.byref(c), C.byref(h)))
    try:
        N, H = 400, 160
        for n, want in ((0, 0), (N - 1, 0), (N, 1), (N + H - 1, 1), (N + H, 2), (N + 2 * H, 3), (16000, 98), (160000, 998)):
            assert L.smilehip_num_frames(h, n) == want == AH.load().audspec_rows_of(n, N, H)
        for k in range(14):                                 # ... and it is what the binary wrote for the 16 kHz inputs
            n = int(gold["inputs"][k][1])
            assert len(gold["lld_%d" % k]) == L.smilehip_num_frames(h, n), k
        assert [round(L.smilehip_row_time(h, 9, r) / 0.01) for r in range(9)] == list(range(9))
    finally:
        L.smilehip_plan_destroy(h)


def test_presets_values_size_and_exports(capi):
    L = capi.load()
    assert capi.CHAIN_AUDSPEC == 11 and capi.LLD_CONFIG_SIZE_V1 == 280
    hdr = open(os.path.join(ROOT, "include", "smilehip.h")).read()
    assert "#define SMILEHIP_CHAIN_AUDSPEC 11" in hdr and "void smilehip_config_audspec(" in hdr and "void smilehip_config_audspec_compat(" in hdr

    class Guarded(C.Structure):
        _fields_ = [("cfg", capi.LldConfig), ("guard", C.c_ubyte * 64)]
    assert C.sizeof(capi.LldConfig) == 280
    for fn, zps in ((L.smilehip_config_audspec, 1), (L.smilehip_config_audspec_compat, 0)):
        g = Guarded()
        C.memset(C.byref(g), 0xA5, C.sizeof(g))
        fn(C.cast(C.byref(g), C.POINTER(capi.LldConfig)))
        c = g.cfg
        assert c.struct_size == 280 and bytes(g.guard) == b"\xa5" * 64        # exactly V1 bytes, nothing behind them
        assert (c.chain_kind, c.zero_pad_symmetric, c.n_bands, c.use_power, c.mel_htk_compatible, c.n_delta, c.delta_win) == (11, zps, 26, 1, 1, 2, 2)
        assert (c.frame_size_sec, c.frame_step_sec, c.preemph, c.preemph_de, c.win_func) == (0.025, 0.010, 1, 0, 2)
        assert c.preemph_k == np.float32(0.97) and c.plp_compression == np.float32(0.33) and (c.lofreq, c.hifreq) == (0.0, 8000.0)
        assert (c.win_gain, c.win_offset, c.append_log_energy, c.cms, c.stage_mask) == (1.0, 0.0, 0, 0, 0)
    c = capi.audspec_config(22050.0, compat=True)
    assert c.sample_rate == 22050.0 and c.zero_pad_symmetric == 0 and capi.audspec_config().sample_rate == 16000.0


@pytest.mark.parametrize("fs", AH.RATES)
def test_geometry_at_every_rate(capi, fs):
    L = capi.load()
    N, H, nfft = GEOMETRY[fs]
    assert AH.NFFT[fs] == nfft
    for compat in (False, True):
        c = capi.audspec_config(fs, compat)
        p = capi.Plan(None, c)
        g = p.geometry
        assert (g.frame_size, g.frame_step, g.fft_size, g.n_bins, g.n_static, g.n_out) == (N, H, nfft, nfft // 2 + 1, 26, 78)
        assert AH.geometry(c)[:5] == (N, H, nfft, nfft // 2 + 1, 26)
        p.close()
    for nd in (0, 1):
        c = capi.audspec_config(fs)
        c.n_delta, c.n_bands = nd, 40
        p = capi.Plan(None, c)
        assert (p.geometry.n_static, p.geometry.n_out) == (40, 40 * (1 + nd))
        p.close()


def test_every_plan_refusal_names_its_parameter(capi):
    L = capi.load()
    h = C.c_void_p()
    for field, value, word in (("stage_mask", 3, b"stage_mask"), ("use_power", 0, b"use_power"), ("mel_htk_compatible", 0, b"mel_htk_compatible"),
                               ("plp_compression", -0.5, b"plp_compression"), ("n_delta", 3, b"n_delta"), ("n_delta", -1, b"n_delta"),
                               ("delta_win", 0, b"delta_win"), ("delta_win", 5, b"delta_win"), ("n_bands", 0, b"n_bands"), ("n_bands", 65, b"n_bands"),
                               ("append_log_energy", 1, b"append_log_energy"), ("cms", 1, b"cms"), ("frame_size_sec", 0.001, b"no mel bank on 9 bins"),
                               ("frame_size_sec", 0.6, b"8192"), ("win_func", 99, b"window")):
        c = capi.audspec_config()
        setattr(c, field, value)
        assert L.smilehip_plan_create_host_only(C.byref(c), C.byref(h)) != 0 and word in L.smilehip_last_error(), (field, L.smilehip_last_error())
    c = capi.audspec_config()                               # few bands on a frame too short to transform: the transform length is named
    c.n_bands, c.frame_size_sec, c.frame_step_sec = 4, 0.001, 0.001
    assert L.smilehip_plan_create_host_only(C.byref(c), C.byref(h)) != 0 and b"transform length" in L.smilehip_last_error(), L.smilehip_last_error()
    for field, value in (("first_mfcc", 7), ("last_mfcc", 3), ("cep_lifter", 0.0), ("plp_lp_order", 99), ("melfloor", 123.0)):   # not read
        c = capi.audspec_config()
        setattr(c, field, value)
        capi._check(L.smilehip_plan_create_host_only(C.byref(c), C.byref(h)))
        L.smilehip_plan_destroy(h)


# ------------------------------------------------------------------------------------------------ names, files, front end
def test_names_equal_the_binarys_header(gold):
    assert str(gold["csv_header"]).split(";") == ["name", "frameTime"] + NAMES
    src = open(os.path.join(ROOT, "opensmile_amd", "host", "feature_names.cpp")).read()
    assert "lld_names_audspec" in src and '"audSpec"' in src
    for stem, rows in (("u2_8000", (8000 - 400) // 160 + 1), ("u3_4000", (4000 - 400) // 160 + 1)):      # 16 kHz files of 8000 / 4000 samples
        lines = open(os.path.join(GOLD, "files", "audspec_%s.csv" % stem)).read().splitlines()
        assert lines[0].split(";") == ["name", "frameTime"] + NAMES and len(lines) == rows + 1 and all(len(ln.split(";")) == 80 for ln in lines)
        for tag in ("audspec", "audspec_compat"):
            b = open(os.path.join(GOLD, "files", "%s_%s.htk" % (tag, stem)), "rb").read()
            assert struct.unpack(">IIHH", b[:12]) == (rows, 100000, 312, 9) and len(b) == 12 + rows * 312
        assert open(os.path.join(GOLD, "files", "audspec_%s.htk" % stem), "rb").read() != open(os.path.join(GOLD, "files", "audspec_compat_%s.htk" % stem), "rb").read()


needs_exe = pytest.mark.skipif(not os.path.exists(EXE), reason="smilextract_hip not built")


def describe(path, *more):
    r = subprocess.run([EXE, "--set", "audspec", "-C", path, "--describe", *more], capture_output=True, text=True)
    kv = dict(ln.split("=", 1) for ln in r.stdout.split("\n") if "=" in ln)
    return r.returncode, kv, r.stderr


def write_conf(tmp_path, text, name="c.conf"):
    p = tmp_path / name
    p.write_text(text)
    return str(p)


@needs_exe
def test_minimal_text_maps_to_the_chain(tmp_path):
    rc, kv, err = describe(write_conf(tmp_path, AH.MINIMAL))
    assert rc == 0, err
    assert kv["preset"] == "" and kv["chain_kind"] == "11" and kv["names"].split(";") == NAMES and kv["parm_kind"] == "9"
    assert (kv["n_bands"], kv["n_delta"], kv["delta_win"], kv["zero_pad_symmetric"], kv["use_power"], kv["mel_htk_compatible"]) == ("26", "2", "2", "1", "1", "1")
    assert (float(kv["frame_size_sec"]), float(kv["frame_step_sec"]), kv["preemph"], kv["win_func"]) == (0.025, 0.010, "1", "2")
    assert np.float32(kv["plp_compression"]) == np.float32(0.33) and np.float32(kv["preemph_k"]) == np.float32(0.97)
    assert "auditory-spectrum chain" in err and "accepted and ignored" in err
    rc, kv, err = describe(write_conf(tmp_path, AH.minimal_text({"writer.dmLevel = fft\n": "writer.dmLevel = fft\nzeroPadSymmetric = 0\n"})))
    assert rc == 0 and kv["zero_pad_symmetric"] == "0", err


WALKER_SHOWS = {"nb20": dict(n_bands="20"), "nb40": dict(n_bands="40"), "lohi": dict(lofreq="100", hifreq="4000"), "comp05": dict(plp_compression="0.5"),
                "dw3": dict(delta_win="3"), "d1": dict(n_delta="1"), "d0": dict(n_delta="0"), "fs32": dict(frame_size_sec="0.032"),
                "han": dict(win_func="1"), "inert": dict(plp_lp_order="8", first_mfcc="1", cep_lifter="0")}


@needs_exe
@pytest.mark.parametrize("tag", sorted(AH.TEXT_EDITS))
def test_each_allowed_edit_shows_up(tmp_path, tag):
    rc, kv, err = describe(write_conf(tmp_path, AH.minimal_text(AH.TEXT_EDITS[tag])))
    assert rc == 0, err
    assert kv["chain_kind"] == "11"
    for k, v in WALKER_SHOWS[tag].items():
        assert float(kv[k]) == float(v), (k, kv[k])
    nb, nd = int(kv["n_bands"]), int(kv["n_delta"])
    assert kv["names"].split(";") == ["audSpec%s[%d]" % (s, i) for s in ("", "_de", "_de_de")[:nd + 1] for i in range(nb)]
    if tag == "inert":
        assert "accepted and ignored" in err
    for k, v in (("k = 0.97", "k = 0.9"), ("de = 0", "de = 1"), ("gain = 1.0", "gain = 2.0"), ("offset = 0", "offset = 0.001"), ("frameStep = 0.010", "frameStep = 0.005")):
        rc2, kv2, err2 = describe(write_conf(tmp_path, AH.minimal_text({k: v}), "d.conf"))
        assert rc2 == 0 and kv2["chain_kind"] == "11", err2


@needs_exe
@pytest.mark.parametrize("edit,words", [
    ({"htkcompatible = 1\ndoIDFT": "htkcompatible = 0\ndoIDFT"}, ("aud:cPlp", "htkcompatible")),
    ({"doLog = 0": "doLog = 0\nRASTA = 1"}, ("aud:cPlp", "RASTA")),
    ({"doLog = 0": "doLog = 0\nnewRASTA = 1"}, ("aud:cPlp", "newRASTA")),
    ({"doIDFT = 0": "doIDFT = 1"}, ("aud:cPlp", "doIDFT = 1 with doLP = 0")),
    ({"doIDFT = 0": "doIDFT = 1", "doLP = 0": "doLP = 1"}, ("aud:cPlp", "doLP = 1 with doLpToCeps = 0")),
    ({"usePower = 1": "usePower = 0"}, ("mel:cMelspec", "usePower")),
    ({"instance[cat].type = cVectorConcat": "instance[cat].type = cVectorConcat\ninstance[en].type = cEnergy",
      "[cat:cVectorConcat]": "[en:cEnergy]\nreader.dmLevel = frames\nwriter.dmLevel = energy\nhtkcompatible = 1\n[cat:cVectorConcat]"}, ("en:cEnergy", "not built")),
    ({"instance[cat].type = cVectorConcat": "instance[cat].type = cVectorConcat\ninstance[cms].type = cFullinputMean",
      "[cat:cVectorConcat]": "[cms:cFullinputMean]\nreader.dmLevel = plp\nwriter.dmLevel = plpz\n[cat:cVectorConcat]"}, ("cms:cFullinputMean", "not built")),
])
def test_each_refused_edit_names_its_option(tmp_path, edit, words):
    rc, kv, err = describe(write_conf(tmp_path, AH.minimal_text(edit)))
    assert rc != 0 and all(w in err for w in words), err


@needs_exe
def test_set_names_and_refused_options(tmp_path):
    r = subprocess.run([EXE, "--set", "audspec"], capture_output=True, text=True)          # the set name is known: what is missing is the input
    assert r.returncode != 0 and "no input" in r.stderr, r.stderr
    r = subprocess.run([EXE, "--set", "audspec_compat"], capture_output=True, text=True)
    assert r.returncode != 0 and "no input" in r.stderr, r.stderr
    r = subprocess.run([EXE, "--set", "audspec_nope", "-I", "x.wav"], capture_output=True, text=True)
    assert r.returncode != 0 and "audspec or audspec_compat" in r.stderr
    r = subprocess.run([EXE, "--set", "audspec", "-I", "x.wav", "-arffoutput", "x.arff"], capture_output=True, text=True)
    assert r.returncode != 0 and "-arffoutput" in r.stderr, r.stderr
    conf = write_conf(tmp_path, AH.MINIMAL)
    r = subprocess.run([EXE, "-C", conf, "--describe"], capture_output=True, text=True)    # plain -C keeps to its files and names the route
    assert r.returncode != 0 and "aud:cPlp" in r.stderr and "--set audspec -C" in r.stderr, r.stderr
    r = subprocess.run([EXE, "--set", "audspec_compat", "-C", conf, "--describe"], capture_output=True, text=True)   # the file's own zero padding holds
    assert r.returncode == 0 and "zero_pad_symmetric=1" in r.stdout and "chain_kind=11" in r.stdout, r.stderr
    r = subprocess.run([EXE, "--set", "plp_0_d_a", "-C", conf, "--describe"], capture_output=True, text=True)
    assert r.returncode != 0 and "exclude each other" in r.stderr


@needs_exe
@pytest.mark.skipif(not os.path.isdir(REF_CONF), reason="the reference's configuration files are not here")
@pytest.mark.parametrize("name,zps", [("audspec.conf", "1"), ("audspec_compat.conf", "0")])
def test_shipped_files_are_recognised(name, zps):
    rc, kv, err = describe(os.path.join(REF_CONF, name))
    assert rc == 0, err
    assert kv["chain_kind"] == "11" and kv["zero_pad_symmetric"] == zps and kv["names"].split(";") == NAMES and kv["parm_kind"] == "9"
    assert (kv["n_bands"], kv["n_delta"], kv["delta_win"], kv["plp_lp_order"], kv["first_mfcc"]) == ("26", "2", "2", "5", "0")
    r = subprocess.run([EXE, "--set", "audspec", "-C", os.path.join(REF_CONF, name), "--describe", "-arffoutput", "x.arff"], capture_output=True, text=True)
    assert r.returncode != 0 and "-arffoutput" in r.stderr, r.stderr
    r = subprocess.run([EXE, "-C", os.path.join(REF_CONF, name), "--describe"], capture_output=True, text=True)
    assert r.returncode != 0 and "--set audspec -C" in r.stderr, r.stderr
    plp = os.path.join(REF_CONF, "..", "plp", "PLP_0_D_A.conf")                 # a cepstral file is not this set's
    r = subprocess.run([EXE, "--set", "audspec", "-C", plp, "--describe"], capture_output=True, text=True)
    assert r.returncode != 0 and "not an auditory-spectrum chain" in r.stderr, r.stderr
