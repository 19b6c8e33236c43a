"""config/spectrum/spectrogram.conf as SMILEHIP_CHAIN_SPECTROGRAM on the device: every cell and every row count equal the real binary's
(tests/golden/spectrogram_synth.npz, spectrogram_rates.npz, hard_spectrogram.npz, files/spectrogram_*), in both forms of
lld_spectrogram_frame, in the five forms of cFFTmagphase, for int16 and float samples, through the plan, against the library's own
per-component operators and through the front end. Equality of bits is the criterion everywhere."""
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import spectrogram_host as SH

pytestmark = pytest.mark.gpu
ROOT = SH.ROOT
GOLD = SH.GOLDEN
EXE = os.path.join(ROOT, "opensmile_amd", "smilextract_hip")
WAVE_FRAMES = 4                                            # frames per workgroup of the wave form (lld_spectrogram.hip: kSpgWaves)
WG_PER_CU_MAX = 4                                          # ... and its workgroups per CU at most (audspec_wave_grid_cap: 16 / kAudWaves)
SYNTH, RATES = "spectrogram_synth.npz", "spectrogram_rates.npz"
# the ragged 16 kHz batch: all ten fixture inputs (0, N - 1, N, N + H - 1, N + H samples, T = 3, 4, 5, 9, 17), shuffled
RAGGED = [2960, 0, 1040, 399, 400, 1680, 559, 720, 560, 880]


def offsets(pcms):
    return np.concatenate([[0], np.cumsum([len(p) for p in pcms])]).astype(np.int64)


def as_f32(pcm):
    return (np.asarray(pcm).astype(np.float32) / np.float32(32767.0)).astype(np.float32)


@pytest.fixture(scope="module")
def hip():
    from opensmile_amd import capi
    ctx = capi.Context(0)
    plan = capi.Plan(ctx, capi.spectrogram_config())
    g = plan.geometry
    assert (g.frame_size, g.frame_step, g.fft_size, g.n_bins, g.n_static, g.n_out) == (400, 160, 512, 257, 257, 257)
    assert plan.spectrum_form()[0] == SH.FLAGS["mag"]      # a fresh plan is plain magnitude
    return capi, ctx, plan


def case_index(name):
    return {c[0]: c for c in SH.cases(name)}


def check_batch(refs, b, out, what=""):
    """rows and every cell of the batch's utterances against the binary's"""
    from tolerance import assert_bits_equal
    for i, ref in enumerate(refs):
        assert b.frame_offsets[i + 1] - b.frame_offsets[i] == len(ref), (what, i, len(ref))
        if len(ref):
            assert_bits_equal(out[b.frame_offsets[i]:b.frame_offsets[i + 1]], ref, "%slevel lld, utterance %d" % (what, i))
    assert b.total_rows == sum(len(r) for r in refs)


def run_cases(capi, ctx, name, keys, f32=False):
    """fixture cases of one rate, geometry and zeroPadSymmetric as one batch on one plan, the form set per case's form"""
    idx = case_index(name)
    gold = SH.fixture(name)
    _, _, _, fs, _, zps, fsz, fst = idx[keys[0]]
    plan = capi.Plan(ctx, SH.config(fs, zps, fsz, fst))
    nfft = plan.geometry.fft_size
    for form in sorted({idx[k][4] for k in keys}):
        ks = [k for k in keys if idx[k][4] == form]
        assert all(idx[k][3:4] + idx[k][5:] == idx[keys[0]][3:4] + idx[keys[0]][5:] for k in ks)
        pcms = [SH.cut(idx[k][1], idx[k][2]) for k in ks]
        plan.set_spectrum_form(SH.FLAGS[form])
        b = capi.Batch(plan, offsets(pcms))
        x = np.concatenate(pcms)
        out = b.spectrogram_run_host(as_f32(x) if f32 else x, fill=np.nan)
        check_batch([gold["lld_" + k] for k in ks], b, out, "%s %s: " % (name, form))
    plan.close()
    return nfft


# ---------------------------------------------------------------------------------------------- 1. golden
@pytest.mark.parametrize("form", ["mag", "db"])
def test_golden_ragged_batch(hip, form):
    capi, ctx, plan = hip
    gold, idx = SH.fixture(SYNTH), case_index(SYNTH)
    keys = ["%s_n%d" % (form, n) for n in RAGGED]
    refs = [gold["lld_" + k] for k in keys]
    assert [len(r) for r in refs] == [17, 0, 5, 0, 1, 9, 1, 3, 2, 4]
    pcms = [SH.cut(idx[k][1], idx[k][2]) for k in keys]
    plan.set_spectrum_form(SH.FLAGS[form])
    try:
        b = capi.Batch(plan, offsets(pcms))
        x = np.concatenate(pcms)
        out = b.run_host(x)                                 # smilehip_lld_run_host serves the chain
        check_batch(refs, b, out)
        for f32 in (False, True):                           # poisoned output, twice over into the same buffer: every cell is written by every run
            o2 = b.spectrogram_run_host(as_f32(x) if f32 else x, fill=np.nan, runs=2)
            check_batch(refs, b, o2, "float input, " if f32 else "")
        o3 = b.spectrogram_run_host(x, ld_out=257 + 5, fill=-7.0)   # a wider matrix: the five columns behind K keep what they held
        check_batch(refs, b, o3[:, :257])
        assert (o3[:, 257:] == -7.0).all()
    finally:
        plan.set_spectrum_form(SH.FLAGS["mag"])


def test_every_form_at_16k(hip):
    capi, ctx, _ = hip
    for f32 in (False, True):
        assert run_cases(capi, ctx, SYNTH, ["mag_n1040", "db_n1040", "norm_n1040", "pow_n1040", "normpow_n1040"], f32) == 512
        assert run_cases(capi, ctx, SYNTH, ["mag_zps0_n1040", "db_zps0_n1040"], f32) == 512


def test_the_form_is_read_at_launch(hip):
    """one batch, the plan's form changed between runs: each run writes the form the plan holds then"""
    capi, ctx, plan = hip
    gold, idx = SH.fixture(SYNTH), case_index(SYNTH)
    pcm = SH.cut(idx["mag_n1040"][1], 1040)
    b = capi.Batch(plan, offsets([pcm]))
    try:
        for form in ("db", "mag", "normpow", "norm", "pow", "mag"):
            plan.set_spectrum_form(SH.FLAGS[form])
            check_batch([gold["lld_%s_n1040" % form]], b, b.spectrogram_run_host(pcm, fill=np.nan), form + ": ")
    finally:
        plan.set_spectrum_form(SH.FLAGS["mag"])


NFFT = {8000: 256, 11025: 512, 22050: 1024, 32000: 1024, 44100: 2048, 48000: 2048}


@pytest.mark.parametrize("fs", sorted(NFFT))
@pytest.mark.parametrize("f32", [False, True])
def test_golden_other_rates(fs, f32):
    """the wave form at 512 and 1024 points, the workgroup form at 256 and 2048; T = 1 and 5, magnitude and dB"""
    from opensmile_amd import capi
    ctx = capi.Context(0)
    keys = ["%s_r%d_T%d" % (form, fs, T) for form in ("mag", "db") for T in (1, 5)]
    assert run_cases(capi, ctx, RATES, keys, f32) == NFFT[fs]


@pytest.mark.parametrize("tag,nfft", [("g64", 64), ("g648", 1024), ("g8192", 8192)])
def test_edited_geometries(tag, nfft):
    """N = 64 at 8 kHz (K = 33, less than one wave of stores), N = 648 at 16 kHz (an odd pad split, H = 64), N = 6400 at 32 kHz"""
    from opensmile_amd import capi
    ctx = capi.Context(0)
    keys = ["%s_%s_T%d" % (form, tag, T) for form in ("mag", "db") for T in (1, 3)]
    for f32 in (False, True):
        assert run_cases(capi, ctx, RATES, keys, f32) == nfft


CHILD = r"""
import os, sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import numpy as np
import test_gpu_spectrogram as T
from opensmile_amd import capi
ctx = capi.Context(0)
for f32 in (False, True):
    T.run_cases(capi, ctx, T.SYNTH, ["%%s_n%%d" %% (form, n) for form in ("mag", "db") for n in T.RAGGED], f32)
    T.run_cases(capi, ctx, T.SYNTH, ["norm_n1040", "pow_n1040", "normpow_n1040"], f32)
T.run_cases(capi, ctx, T.SYNTH, ["mag_zps0_n1040", "db_zps0_n1040"])
T.run_cases(capi, ctx, T.RATES, ["%%s_r32000_T%%d" %% (form, n) for form in ("mag", "db") for n in (1, 5)])
T.run_cases(capi, ctx, T.RATES, ["%%s_g648_T%%d" %% (form, n) for form in ("mag", "db") for n in (1, 3)])
print("CHILD OK", os.environ.get("SMILEHIP_SPECTROGRAM"))
"""


def test_workgroup_form_equals_the_binary():
    """SMILEHIP_SPECTROGRAM=block: the workgroup-per-frame form where the wave form would run (512 / 1024 points), in a fresh process"""
    env = dict(os.environ, SMILEHIP_SPECTROGRAM="block")
    r = subprocess.run([sys.executable, "-c", CHILD % (ROOT, os.path.join(ROOT, "tests"))], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "CHILD OK block" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


# ---------------------------------------------------------------------------------------------- 2. the grid's second trip
@pytest.mark.parametrize("form", ["mag", "db"])
def test_persistent_grid_takes_a_second_trip(hip, form):
    """1 000 copies of the 17-frame utterance, 17 000 rows and 17 MB: more frames than one pass of the wave form's grid holds (its cap
    times four frames); every copy's rows equal the fixture's"""
    import torch
    capi, ctx, plan = hip
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    at_once = cus * WG_PER_CU_MAX * WAVE_FRAMES
    ref = SH.fixture(SYNTH)["lld_%s_n2960" % form]
    pcm = SH.cut(case_index(SYNTH)["mag_n2960"][1], 2960)
    copies = 1000
    assert len(ref) == 17 and copies * 17 > at_once + 17
    plan.set_spectrum_form(SH.FLAGS[form])
    try:
        b = capi.Batch(plan, offsets([pcm] * copies))
        assert b.total_frames == 17 * copies
        out = b.spectrogram_run_host(np.tile(pcm, copies), fill=np.nan)
    finally:
        plan.set_spectrum_form(SH.FLAGS["mag"])
    got = out.view(np.uint32).reshape(copies, 17, 257)
    assert (got == ref.view(np.uint32)[None]).all(), "copies %s differ from the fixture" % np.unique(np.argwhere(got != ref.view(np.uint32)[None])[:, 0])[:8]


# ---------------------------------------------------------------------------------------------- 3. the library's own operators
def per_component(capi, ctx, plan, pcm, flags):
    """the chain out of the operators, one launch each over all frames of one utterance"""
    import torch
    g = plan.geometry
    N, H, K, Nfft = g.frame_size, g.frame_step, g.n_bins, g.fft_size
    T = (len(pcm) - N) // H + 1
    x = as_f32(pcm)
    d_fr = torch.from_numpy(np.stack([x[t * H:t * H + N] for t in range(T)])).cuda()
    d_w, d_c, d_m = torch.zeros((T, N), device="cuda"), torch.zeros((T, Nfft), device="cuda"), torch.zeros((T, K), device="cuda")
    capi.window_frames(plan, d_fr.data_ptr(), N, d_w.data_ptr(), N, T)
    capi.rfft_frames(plan, d_w.data_ptr(), N, d_c.data_ptr(), Nfft, T)
    _, dbp_norm, min_dbp = plan.spectrum_form()             # (the operator takes mindBp as it is given: the plan's, behind the clamp)
    capi._check(capi.load().smilehip_fftmagphase_frames(ctx._h, d_c.data_ptr(), Nfft, Nfft, flags, dbp_norm, min_dbp, d_m.data_ptr(), K, T, None))
    torch.cuda.synchronize()
    return d_m.cpu().numpy()


@pytest.mark.parametrize("fs", [16000, 44100])
def test_fused_equals_per_component_operators(fs):
    """a seeded signal on which no fixture exists, once per kernel form, in the five forms. (The operator orders its MAX the other way
    round; on finite values the two agree, and this signal has no NaN.)"""
    from tolerance import assert_bits_equal
    from opensmile_amd import capi, synth
    ctx = capi.Context(0)
    plan = capi.Plan(ctx, capi.spectrogram_config(float(fs)))
    pcm = (synth.utterance(31, fs // 4).astype(np.int32) // 3).astype(np.int16)
    b = capi.Batch(plan, np.array([0, len(pcm)], np.int64))
    for form in SH.FORMS:
        plan.set_spectrum_form(SH.FLAGS[form])
        fused = b.spectrogram_run_host(pcm, fill=np.nan)
        ref = per_component(capi, ctx, plan, pcm, SH.FLAGS[form])
        assert np.isfinite(ref).all()
        assert_bits_equal(fused, ref, "level lld at %d Hz, %s" % (fs, form))
    plan.close()


# ---------------------------------------------------------------------------------------------- 4. hard signals
def test_hard_signals(hip):
    from tolerance import assert_bits_equal
    from helpers import hard_signals
    capi, ctx, plan = hip
    ref = SH.fixture("hard_spectrogram.npz")
    pcm = hard_signals.signals()
    seg = {str(r[0]): (int(r[1]), int(r[2])) for r in ref["segments"]}
    sig = [np.ascontiguousarray(pcm[n][seg[n][0]:seg[n][0] + seg[n][1]], np.int16) for n in hard_signals.NAMES]
    b = capi.Batch(plan, offsets(sig))
    floor = np.float32(-120.0) + np.float32(90.302)
    try:
        for form in ("mag", "db"):
            plan.set_spectrum_form(SH.FLAGS[form])
            out = b.spectrogram_run_host(np.concatenate(sig), fill=np.nan)
            on_floor = 0
            for i, n in enumerate(hard_signals.NAMES):
                o = out[b.frame_offsets[i]:b.frame_offsets[i + 1]]
                assert_bits_equal(o, ref["lld_%s_%s" % (form, n)], "hard signal %s, %s" % (n, form))
                if form == "db" and n in ("lsb_noise", "clicks_in_zeros", "zeros_voiced_zeros"):
                    on_floor += int((o == floor).sum())
            assert form == "mag" or on_floor > 0             # digital zeros and +-1 LSB noise sit on the mindBp floor
    finally:
        plan.set_spectrum_form(SH.FLAGS["mag"])


# ---------------------------------------------------------------------------------------------- 5. the front end
needs_exe = pytest.mark.skipif(not os.path.exists(EXE), reason="smilextract_hip not built")


def smilextract(*args):
    p = subprocess.run([EXE, *args], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    return p


def read(path):
    with open(path, "rb") as f:
        return f.read()


@needs_exe
@pytest.mark.parametrize("tag,args", [("spectrogram", []), ("spectrogram_db", ["-dB", "1"])])
def test_front_end_set_writes_the_binarys_files(tmp_path, tag, args):
    wav = os.path.join(GOLD, "files", "u3_4000.wav")
    htk, csv = str(tmp_path / "o.htk"), str(tmp_path / "o.csv")
    smilextract("--set", "spectrogram", "-I", wav, "-O", htk, "-csvoutput", csv, *args)
    assert read(htk) == read(os.path.join(GOLD, "files", tag + "_u3_4000.htk"))
    assert read(csv) == read(os.path.join(GOLD, "files", tag + "_u3_4000.csv"))
    conf = tmp_path / "m.conf"                              # the same through -C on the project's own text of the graph
    conf.write_text(SH.minimal_text())
    htk2, csv2 = str(tmp_path / "c.htk"), str(tmp_path / "c.csv")
    smilextract("--set", "spectrogram", "-C", str(conf), "-I", wav, "-O", htk2, "-csvoutput", csv2, *args)
    assert read(htk2) == read(htk) and read(csv2) == read(csv)


@needs_exe
def test_front_end_edited_copy_and_geometry(tmp_path):
    """-C on an edited copy built here (normalise + power; zeroPadSymmetric = 0), and the file's -frameSize / -frameStep with and
    without -C: the HTK rows are the binary's"""
    from oracle import lldo
    gold, rates, idx, ridx = SH.fixture(SYNTH), SH.fixture(RATES), case_index(SYNTH), case_index(RATES)
    wav = str(tmp_path / "in.wav")
    lldo.write_wav(wav, SH.cut(idx["mag_n1040"][1], 1040), 16000)
    for tag, key, args in (("normpow", "normpow_n1040", []), ("zps0", "db_zps0_n1040", ["-dB", "1"])):
        conf = tmp_path / (tag + ".conf")
        conf.write_text(SH.minimal_text(SH.TEXT_EDITS[tag]))
        htk = str(tmp_path / (tag + ".htk"))
        smilextract("--set", "spectrogram", "-C", str(conf), "-I", wav, "-O", htk, *args)
        rows, period, kind = lldo.read_htk(htk)
        assert (period, kind) == (100000, 9) and rows.shape == gold["lld_" + key].shape and rows.tobytes() == gold["lld_" + key].tobytes(), tag
    _, i, n, fs, _, _, fsz, fst = ridx["db_g648_T3"]
    lldo.write_wav(wav, SH.cut(i, n), fs)
    conf = tmp_path / "m.conf"
    conf.write_text(SH.minimal_text())
    for k, extra in enumerate(([], ["-C", str(conf)])):
        htk = str(tmp_path / ("g%d.htk" % k))
        smilextract("--set", "spectrogram", *extra, "-I", wav, "-O", htk, "-dB", "1", "-frameSize", repr(fsz), "-frameStep", repr(fst))
        rows, period, kind = lldo.read_htk(htk)
        ref = rates["lld_db_g648_T3"]
        assert (period, kind) == (40000, 9) and rows.shape == ref.shape and rows.tobytes() == ref.tobytes(), extra


@needs_exe
def test_front_end_file_list(tmp_path):
    """-filelist / -outdir as for the other LLD-only sets: one HTK and one CSV file per input"""
    import shutil
    a, b = str(tmp_path / "a.wav"), str(tmp_path / "b.wav")
    shutil.copy(os.path.join(GOLD, "files", "u3_4000.wav"), a)
    shutil.copy(os.path.join(GOLD, "files", "u3_4000.wav"), b)
    lst = tmp_path / "list.txt"
    lst.write_text(a + "\n" + b + "\tsecond\n")
    out = tmp_path / "out"
    out.mkdir()
    smilextract("--set", "spectrogram", "-filelist", str(lst), "-outdir", str(out), "-O", "1", "-csvoutput", "1", "-dB", "1")
    for stem in ("a", "b"):
        assert read(str(out / (stem + ".htk"))) == read(os.path.join(GOLD, "files", "spectrogram_db_u3_4000.htk"))
    want = read(os.path.join(GOLD, "files", "spectrogram_db_u3_4000.csv")).decode()
    assert read(str(out / "a.csv")).decode() == want.replace("'unknown'", "'a'") and read(str(out / "b.csv")).decode() == want.replace("'unknown'", "'second'")
