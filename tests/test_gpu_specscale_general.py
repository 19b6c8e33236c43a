"""cSpecScale on every target scale on the device (smilehip_specscale_op_*, csrc/lld_specscale.hip): against the real binary's levels
(tests/golden/specscale_general_synth.npz), against the float64 restatement of tests/test_specscale_general_host.py (which that file
holds bit-equal to the same goldens), against the octave operator of the F0 chains on the geometry both serve, and inside the
unmodified binary through the plugin. The kernels' operations are the reference's correctly rounded double operations in its order
and the tables come from the same C library: everything is compared bit for bit (both-zero counts as equal)."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

from test_specscale_general_host import (CONF, CONF_ORDER, GOLDEN_KEYS, LIN, LOG, MEL, SCALES, SEEDED, bits_equal, ref_rows, ref_tables,
                                         seeded_id, split_levels)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLUGDIR = os.path.join(ROOT, "opensmile_amd", "plugin")
CONF_FILE = os.path.join(ROOT, "tests", "conf", "specscale_general.conf")


@pytest.fixture(scope="module")
def env():
    import torch
    from opensmile_amd import capi
    return torch, capi, capi.Context(0)


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "specscale_general_synth.npz"))


def run_op(env, mag, scale, param, min_f, max_f, n_points_target, fs, enhance, smooth, weighting, ld_src=None, pad_dst=0):
    """the operator on the rows of mag; rows of ld_src floats in (the tail filled with NaN), n_out + pad_dst out (the pad must stay)"""
    torch, capi, ctx = env
    L = capi.load()
    rows, n_src = mag.shape
    o = capi.specscale_opts(scale, param, min_f, max_f, n_points_target, enhance, smooth, weighting)
    op = C.c_void_p()
    capi._check(L.smilehip_specscale_op_create(ctx._h, C.byref(o), n_src, fs, C.byref(op)))
    try:
        n_out = L.smilehip_specscale_op_n_out(op)
        ld_src = ld_src or n_src
        src = np.full((rows, ld_src), np.nan, np.float32)
        src[:, :n_src] = mag
        d_src = torch.from_numpy(src).cuda()
        d_dst = torch.full((rows, n_out + pad_dst), -7.0, dtype=torch.float32, device="cuda")
        capi._check(L.smilehip_specscale_op_frames(op, d_src.data_ptr(), ld_src, d_dst.data_ptr(), n_out + pad_dst, rows, None))
        torch.cuda.synchronize()
        got = d_dst.cpu().numpy()
    finally:
        capi._check(L.smilehip_specscale_op_destroy(op))
    assert (got[:, n_out:] == -7.0).all(), "the operator wrote past a row's nPointsTarget values"
    return got[:, :n_out]


def assert_bits(got, ref, what):
    if not bits_equal(got, ref):
        d = (got.view(np.uint32) != ref.view(np.uint32)) & ~((got == 0) & (ref == 0))
        at = np.argwhere(d)
        raise AssertionError(f"{what}: {d.sum()} of {d.size} cells differ, first {at[:4].tolist()}: {got[d][:4]} vs {ref[d][:4]}")


@pytest.mark.parametrize("name", CONF_ORDER)
def test_goldens(env, golden, name):
    """the operator on the real binary's magnitude level gives the real binary's scaled level"""
    scale, param, min_f, max_f, npt, enh, smo, wgt = CONF[name]
    for key in GOLDEN_KEYS:
        lv = split_levels(golden["out_" + key])
        got = run_op(env, lv["mag"], scale, param, min_f, max_f, npt, float(golden["frame_size_sec"]), enh, smo, wgt)
        assert_bits(got, lv[name], f"{name} {key}")


def seeded_rows(rng, rows, n):
    """spectrum-like rows: magnitudes with a few strong peaks, so that the enhancement has gaps to zero and the spline overshoots"""
    mag = np.abs(rng.standard_normal((rows, n), dtype=np.float32))
    mag[:, ::5] *= 30.0
    if rows > 2:
        mag[1] = np.float32(np.round(mag[1] * 4.0) / 4.0)    # plateaus: the peak test's >= side
    return mag


@pytest.mark.parametrize("c", SEEDED, ids=seeded_id)
def test_seeded_rows(env, c):
    """every scale on every source size, the target sizes {2, 7, n_src, 3 n_src}, row counts around the 64-row tile, the switches on
    and off, rows longer than the spectrum in and out"""
    scale = SCALES[c["scale"]]
    T = ref_tables(scale, c["param"], c["min_f"], c["max_f"], c["n_tgt"], c["n_src"], c["fs"], c["weighting"])
    mag = seeded_rows(np.random.default_rng(1000 * c["n_src"] + c["rows"]), c["rows"], c["n_src"])
    ref = ref_rows(T, mag, c["enhance"], c["smooth"])
    got = run_op(env, mag, scale, c["param"], c["min_f"], c["max_f"], c["n_tgt"], c["fs"], c["enhance"], c["smooth"], c["weighting"],
                 ld_src=c["n_src"] + 3, pad_dst=5)
    assert_bits(got, ref, seeded_id(c))


def edge_rows(n):
    i = np.arange(n, dtype=np.float32)
    rows = {
        "all zero": np.zeros(n, np.float32),
        "constant": np.full(n, 2.5, np.float32),
        "a single peak": np.where(i <= n // 2, i, n // 2 - 0.5 * (i - n // 2)).astype(np.float32),      # one maximum: everything from bin 3 on is zeroed
        "strictly rising": (i * 0.37 + 1.0).astype(np.float32),                                       # its one maximum is the last bin
        "strictly falling": (n - i).astype(np.float32),                                               # ... the first bin
        "alternating": np.where(i % 2 == 0, 1.0, 3.0).astype(np.float32),
        "negative values": (np.sin(i * 0.7) * 3.0 - 1.0).astype(np.float32),
        "1e30": (np.abs(np.sin(i * 1.3)) * np.float32(1e30)).astype(np.float32),
    }
    return list(rows), np.stack(list(rows.values()))


@pytest.mark.parametrize("n_src", [33, 257])
@pytest.mark.parametrize("sw", [0, 1, 2, 3, 7])
def test_edge_rows(env, n_src, sw):
    """all-zero, constant, single-peak (the reference's nmax == 1 quirk), rising, falling, alternating and 1e30 rows; negative values
    pass through when the weighting is off and are floored by it when it is on"""
    names, mag = edge_rows(n_src)
    enh, smo, wgt = sw & 1, (sw >> 1) & 1, (sw >> 2) & 1
    for scale, param in ((LOG, 2.0), (MEL, 0.0), (LIN, 0.0)):
        args = (scale, param, 50.0, 0.9 * 40.0 * (n_src - 1), 0 if scale != MEL else 3 * n_src, n_src, 0.025, wgt)
        T = ref_tables(*args)
        ref = ref_rows(T, mag, enh, smo)
        got = run_op(env, mag, scale, param, args[2], args[3], args[4], 0.025, enh, smo, wgt)
        for r, nm in enumerate(names):
            assert_bits(got[r:r + 1], ref[r:r + 1], f"{nm}, scale {scale}, switches {sw}")
        neg = names.index("negative values")
        if T["weighting"]:
            assert (got[neg] >= 0).all()
        elif scale == LIN and not enh and not smo:
            assert (got[neg] < 0).any()


@pytest.mark.parametrize("K,min_f,off", [(513, 25.0, 0), (257, 20.0, 0), (2049, 25.0, 5), (513, 25.0, 7)])
def test_equals_the_octave_operator(env, K, min_f, off):
    """on the octave geometry of the F0 chains (log base 2, maxF -1, nPointsTarget 0) the general operator and
    smilehip_specscale_frames, which runs other kernels on other tables, give the same rows: independent of the restatement"""
    torch, capi, ctx = env
    fs = (K - 1) * 2 / 16000.0
    cfg = capi.compare16_f0_config()
    cfg.force_fft_frame_size_sec = fs
    cfg.force_frame_size = 2 * (K - 1)
    cfg.specscale_min_f = min_f
    cfg.specscale_off = off
    plan = capi.Plan(ctx, cfg)
    assert plan.geometry.n_bins == K
    mag = seeded_rows(np.random.default_rng(K + off), 70, K)
    mag[0] = 0.0
    mag[2] = 1.0
    d_m = torch.from_numpy(mag).cuda()
    d_h = torch.zeros((70, K), dtype=torch.float32, device="cuda")
    capi._check(capi.load().smilehip_specscale_frames(plan._h, d_m.data_ptr(), K, d_h.data_ptr(), K, 70, None))
    torch.cuda.synchronize()
    got = run_op(env, mag, LOG, 2.0, min_f, -1.0, 0, fs, not off & 1, not off & 2, not off & 4)
    assert_bits(got, d_h.cpu().numpy(), f"octave K={K} off={off}")


def test_more_rows_than_one_chunk_and_a_second_call(env):
    """a batch longer than the operator's scratch is walked in chunks; a later, longer call grows the scratch"""
    torch, capi, ctx = env
    L = capi.load()
    n_src, fs = 8193, 0.025                                  # 131 200 bytes of scratch per row: the 512 MiB limit holds 4 032 rows
    args = (MEL, 0.0, 50.0, 0.9 * 40.0 * (n_src - 1), 7, n_src, fs)
    T = ref_tables(*args)
    rng = np.random.default_rng(5)
    mag = seeded_rows(rng, 4032 + 65, n_src)
    pick = np.array([0, 63, 64, 4031, 4032, 4033, 4096])     # rows on both sides of the chunk boundary
    ref = ref_rows(T, mag[pick], 1, 1)
    o = capi.specscale_opts(MEL, 0.0, args[2], args[3], 7, 1, 1, 0)
    op = C.c_void_p()
    capi._check(L.smilehip_specscale_op_create(ctx._h, C.byref(o), n_src, fs, C.byref(op)))
    d_src = torch.from_numpy(mag).cuda()
    d_dst = torch.zeros((mag.shape[0], 7), dtype=torch.float32, device="cuda")
    capi._check(L.smilehip_specscale_op_frames(op, d_src.data_ptr(), n_src, d_dst.data_ptr(), 7, 3, None))       # a small first call
    capi._check(L.smilehip_specscale_op_frames(op, d_src.data_ptr(), n_src, d_dst.data_ptr(), 7, mag.shape[0], None))
    torch.cuda.synchronize()
    got = d_dst.cpu().numpy()[pick]
    # bad arguments are refused, not run
    assert L.smilehip_specscale_op_frames(op, d_src.data_ptr(), n_src - 1, d_dst.data_ptr(), 7, 3, None) != 0
    assert L.smilehip_specscale_op_frames(op, d_src.data_ptr(), n_src, d_dst.data_ptr(), 6, 3, None) != 0
    assert L.smilehip_specscale_op_frames(op, None, n_src, d_dst.data_ptr(), 7, 3, None) != 0
    capi._check(L.smilehip_specscale_op_frames(op, None, n_src, None, 7, 0, None))
    capi._check(L.smilehip_specscale_op_destroy(op))
    assert_bits(got, ref, "chunked batch")


def test_create_refuses_what_the_tables_refuse(env):
    torch, capi, ctx = env
    L = capi.load()
    op = C.c_void_p()
    bao = capi.specscale_opts("bao", 0.0, 100.0, 4000.0, 0)
    assert L.smilehip_specscale_op_create(ctx._h, C.byref(bao), 257, 0.032, C.byref(op)) == -1
    assert "increase" in L.smilehip_last_error().decode()
    assert L.smilehip_specscale_op_create(ctx._h, None, 257, 0.032, C.byref(op)) == -1
    assert L.smilehip_specscale_op_n_out(None) == -1


# ------------------------------------------------------------------ inside the unmodified binary
def _smilextract(oracle, pcm, conf, env_extra):
    exe = os.path.join(oracle.REF_DIR, "SMILExtract")
    plug = os.path.join(PLUGDIR, "plugins", "libsmilehip_plugin.so")
    if not (os.path.exists(exe) and os.path.exists(plug)):
        pytest.skip("oracle/_ref/SMILExtract or the plugin .so not built (needs the reference sources at build time)")
    with tempfile.TemporaryDirectory() as td:
        wav, out, trace = (os.path.join(td, n) for n in ("in.wav", "out.htk", "trace.txt"))
        oracle.write_wav(wav, pcm, 16000)
        e = dict(os.environ)
        e["LD_LIBRARY_PATH"] = os.pathsep.join([os.path.join(ROOT, "opensmile_amd"), oracle.REF_DIR, e.get("LD_LIBRARY_PATH", "")])
        e["SMILEHIP_PLUGIN_TRACE"] = trace
        e.update(env_extra or {})
        r = subprocess.run([exe, "-C", conf, "-I", wav, "-O", out, "-l", "1"], cwd=PLUGDIR, env=e, capture_output=True, text=True,
                           errors="replace", timeout=300)
        data = open(out, "rb").read() if os.path.exists(out) else b""
        tr = dict(l.split() for l in open(trace).read().split("\n") if l.strip()) if os.path.exists(trace) else {}
    return r, data, {k: int(v) for k, v in tr.items()}


def test_plugin_runs_every_scale(oracle, golden):
    """tests/conf/specscale_general.conf through the real binary, plain and with every override: the files are byte-identical, no
    component ran on the CPU, and cSpecScale counted its six instances' frames"""
    key = GOLDEN_KEYS[0]
    pcm = golden["pcm_" + key]
    r0, ref, _ = _smilextract(oracle, pcm, CONF_FILE, {"SMILEHIP_PLUGIN_COMPONENTS": "none"})
    assert r0.returncode == 0, r0.stderr[-2000:]
    r1, own, tr = _smilextract(oracle, pcm, CONF_FILE, None)
    assert r1.returncode == 0, r1.stderr[-2000:]
    assert not [k for k, v in tr.items() if k.endswith(".cpu") and v], tr
    n_frames = golden["out_" + key].shape[0]
    assert tr.get("cSpecScale", 0) == 6 * n_frames, tr
    assert len(ref) == 12 + 4 * 1256 * n_frames and own == ref


def test_plugin_refuses_bao_on_this_spectrum(oracle, golden, tmp_path):
    """'bao' on 31.25 Hz bins: the source axis goes down at bin 1, the reference's spline is undefined -- the run ends with the
    refusal that names it"""
    text = open(CONF_FILE).read()
    assert text.count("scale = lin") == 1
    conf = tmp_path / "specscale_bao.conf"
    conf.write_text(text.replace("scale = lin", "scale = bao"))
    r, _, tr = _smilextract(oracle, golden["pcm_" + GOLDEN_KEYS[1]], str(conf), None)
    said = r.stderr + r.stdout
    assert r.returncode != 0
    assert "cSpecScale" in said and "do not increase on the target axis" in said and "not built for the HIP path" in said, said[-2000:]


def test_plugin_octave_axis_on_other_spectrum_sizes(oracle, tmp_path):
    """the option set of the F0 chains (octave axis, maxF -1, nPointsTarget 0 -- the component's defaults) on spectra their plans are
    not built for: 129 bins (25 ms frames at 8 kHz) with nothing but the default options, 4097 bins (1 s frames) with the three
    switches on. Both go to the general operator; the files equal the plain binary's byte for byte and nothing ran on the CPU."""
    from opensmile_amd import synth
    exe = os.path.join(oracle.REF_DIR, "SMILExtract")
    plug = os.path.join(PLUGDIR, "plugins", "libsmilehip_plugin.so")
    if not (os.path.exists(exe) and os.path.exists(plug)):
        pytest.skip("oracle/_ref/SMILExtract or the plugin .so not built (needs the reference sources at build time)")
    conf = os.path.join(ROOT, "tests", "conf", "specscale_octave_sizes.conf")
    wav, trace = str(tmp_path / "in.wav"), str(tmp_path / "trace.txt")
    oracle.write_wav(wav, synth.utterance(3, 20000, 8000), 8000)
    files = {}
    for mode, extra in (("plain", {"SMILEHIP_PLUGIN_COMPONENTS": "none"}), ("plugin", {})):
        e = dict(os.environ)
        e["LD_LIBRARY_PATH"] = os.pathsep.join([os.path.join(ROOT, "opensmile_amd"), oracle.REF_DIR, e.get("LD_LIBRARY_PATH", "")])
        e["SMILEHIP_PLUGIN_TRACE"] = trace
        e.update(extra)
        outs = [str(tmp_path / f"{mode}_{n}.htk") for n in ("short", "long")]
        r = subprocess.run([exe, "-C", conf, "-I", wav, "-O", outs[0], "-P", outs[1], "-l", "1"], cwd=PLUGDIR, env=e, capture_output=True,
                           text=True, errors="replace", timeout=300)
        assert r.returncode == 0, (r.stderr + r.stdout)[-2000:]
        files[mode] = [open(o, "rb").read() for o in outs]
    tr = {k: int(v) for k, v in (l.split() for l in open(trace).read().split("\n") if l.strip())}
    assert not [k for k, v in tr.items() if k.endswith(".cpu") and v], tr
    n_short, n_long = ((len(f) - 12) // (4 * w) for f, w in zip(files["plain"], (129, 4097)))
    assert n_short > 100 and n_long >= 4 and tr.get("cSpecScale", 0) == n_short + n_long, tr
    assert files["plugin"] == files["plain"]

