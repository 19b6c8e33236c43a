"""Functionals over fixed windows (cWinToVecProcessor frameMode = fixed) on the batch path: smilehip_funcspec_matrix_windows and
smilehip_batch_funcspec_windows against the CPU oracle on every window's slice (test_gpu_funcspec.check's rule: bits, 1e-6 for the
values that pass through libm), against the full-mode entry points on the same slice (bits: the same device code), across chunk
seams, lane packing and utterance boundaries, and -- for IS09_emotion -- against the real binary's bits
(tests/golden/func_windows_is09.npz, recorded by tests/golden/make_golden_func_windows.py)."""
import os
import subprocess

import numpy as np
import pytest

from test_gpu_funcspec import as_oracle_spec, check

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden", "func_windows_is09.npz")
SPECS = ["c16:A", "c16:B", "c16:F0", "c16:Nz", "c16:LLD", "c16:Delta", "eg:F0", "eg:Loudness", "eg:MVZ", "eg:MVV", "eg:MU",
         "eg:numPeaks", "eg:segF0", "eg:segF0pause", "eg:leq", "is09"]
COLS = (1, 25, 32, 33, 64, 65)             # packing with idle lanes, exact packing, no packing, two column groups
GEOMETRIES = ((1, 1), (3, 2), (10, 1), (10, 10), (10, 25))


@pytest.fixture(scope="module")
def hip():
    from opensmile_amd import capi
    return capi, capi.Context(0)


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def make_spec(capi, name):
    if name == "is09":
        return capi.funcspec_is09()
    kind, inst = name.split(":")
    return capi.funcspec_compare16(inst) if kind == "c16" else capi.funcspec_egemaps(inst)


def edge_data(rng, rows, cols):
    """as test_funcspec_edge_shapes: an all-zero column, a constant one, interleaved zeros, ties"""
    x = rng.standard_normal((rows, cols)).astype(np.float32)
    for c0 in range(0, cols - 5, 7):
        x[:, c0 + 1] = 0.0
        x[:, c0 + 2] = 3.5
        x[:, c0 + 3] = np.where(np.arange(rows) % 3 == 0, 0.0, x[:, c0 + 3])
        x[:, c0 + 4] = np.abs(x[:, c0 + 4])
        x[:, c0 + 5] = np.round(x[:, c0 + 5] * 2) / 2 + 0.0      # (+ 0.0: no -0.0 beside 0.0 -- where the two tie, the
        # sort network and the reference's sort may keep either one's bits as a quartile; funcspec_matrix_host differs from the
        # oracle in that way too, and the windows equal it bit for bit there)
    return x


def slices(x, size, step):
    n = (x.shape[0] - size) // step + 1 if x.shape[0] >= size else 0
    return [np.ascontiguousarray(x[k * step:k * step + size]) for k in range(n)]


def bits_equal(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("name", SPECS)
def test_windows_equal_their_slices(hip, oracle, name):
    """Every window equals the oracle on its slice (check's rule) and funcspec_matrix_host on its slice bit for bit."""
    capi, ctx = hip
    spec = make_spec(capi, name)
    per = capi.funcspec_count(spec)
    ospec = as_oracle_spec(oracle, spec)
    rng = np.random.default_rng(17)
    seen = 0
    for cols in COLS:
        for size, step in GEOMETRIES:
            for rows in sorted({size - 1, size, size + 1, size + step - 1, size + step, 37}):
                x = edge_data(rng, rows, cols)
                dev = capi.funcspec_matrix_windows_host(ctx, spec, x, size, step)
                sl = slices(x, size, step)
                assert dev.shape == (len(sl), cols * per), (cols, size, step, rows)
                if rows >= size:
                    assert len(sl) == (rows - size) // step + 1 >= 1
                for k, s in enumerate(sl):
                    what = f"{name}/cols{cols}/size{size}/step{step}/rows{rows}/window{k}"
                    got = dev[k].reshape(cols, per)
                    check(oracle, spec, got, oracle.funcspec(s, ospec), what)
                    assert bits_equal(got, capi.funcspec_matrix_host(ctx, spec, s)), what
                    seen += 1
    assert seen > 500


@pytest.mark.parametrize("size", [64, 65, 1024, 1025, 8200])
def test_percentile_sort_paths_on_windows(hip, oracle, size):
    """The wave sort's sizes around 64 and its upper end, the workgroup sort in LDS, and the sort in global scratch (each window
    its own region), two and three windows each; nonZeroFuncts makes the columns' lengths differ."""
    capi, ctx = hip
    spec = capi.funcspec_compare16("Nz")
    per = capi.funcspec_count(spec)
    rng = np.random.default_rng(size)
    for n_win, step in ((2, 7), (3, 1)):
        x = rng.standard_normal((size + (n_win - 1) * step, 5)).astype(np.float32)
        x[:, 1] = np.round(x[:, 1] * 2) / 2 + 0.0
        x[::5, 2] = 0.0
        x[:, 3] = np.abs(x[:, 3])
        dev = capi.funcspec_matrix_windows_host(ctx, spec, x, size, step)
        sl = slices(x, size, step)
        assert dev.shape[0] == len(sl) == n_win
        for k, s in enumerate(sl):
            got = dev[k].reshape(5, per)
            check(oracle, spec, got, oracle.funcspec(s, as_oracle_spec(oracle, spec)), f"Nz/size{size}/window{k}")
            assert bits_equal(got, capi.funcspec_matrix_host(ctx, spec, s))


@pytest.mark.parametrize("inst", ["Nz", "LLD"])
def test_chunk_seams(hip, monkeypatch, inst):
    """SMILEHIP_FUNC_WINDOWS_SCRATCH_MB (read at every call) down to one window per chunk and to a few: seams inside packed waves
    and between them; the compacted nonZeroFuncts copy (Nz) and Peaks2's alive bytes (LLD) are the scratch that is reused from
    chunk to chunk. Bit for bit the unbounded run."""
    capi, ctx = hip
    spec = capi.funcspec_compare16(inst)
    rng = np.random.default_rng(23)
    for cols in (25, 65):
        x = edge_data(rng, 60, cols)
        monkeypatch.delenv("SMILEHIP_FUNC_WINDOWS_SCRATCH_MB", raising=False)
        whole = capi.funcspec_matrix_windows_host(ctx, spec, x, 10, 1)
        assert whole.shape[0] == 51
        for k, s in enumerate(slices(x, 10, 1)):
            assert bits_equal(whole[k].reshape(cols, -1), capi.funcspec_matrix_host(ctx, spec, s))
        for mb in ("0.000001", "0.01", "0.03"):            # one window per chunk, then a few and a few more
            monkeypatch.setenv("SMILEHIP_FUNC_WINDOWS_SCRATCH_MB", mb)
            assert bits_equal(capi.funcspec_matrix_windows_host(ctx, spec, x, 10, 1), whole), (inst, cols, mb)


def test_ragged_batch(hip, oracle):
    """Batch.funcspec_windows_host on the lengths of test_batch_funcspec_ragged_with_cut_and_extra_row plus utterances of exactly
    one and exactly three windows next to each other (a packed wave spans the utterance boundary): win_off is the host rule,
    utterances without a window leave no row, every row equals its slice."""
    capi, ctx = hip
    from opensmile_amd import synth
    plan = capi.Plan(ctx, capi.compare16_config())
    lens = [48000, 0, 9000, 1760, 2560, 4160, 2560, 24000, 1600]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    pcm = np.concatenate([synth.utterance(70 + i, n) if n else np.zeros(0, np.int16) for i, n in enumerate(lens)])
    b = capi.Batch(plan, off)
    lld = b.run_host(pcm)
    rows = np.diff(b.frame_offsets)
    size, step = 10, 5
    assert list(np.diff(b.func_windows(size, step, 0))[[1, 4, 5, 6]]) == [0, 1, 3, 1]
    for inst, c0, nc, cut in (("A", 6, 4, 3), ("B", 10, 55, 0), ("Nz", 0, 6, 5), ("LLD", 6, 59, 1), ("F0", 0, 1, 0), ("A", 71, 32, 0)):
        spec = capi.funcspec_compare16(inst)
        per = capi.funcspec_count(spec)
        dev, win_off = b.funcspec_windows_host(lld, spec, c0, nc, cut, size, step)
        want = [0]
        for r in rows:
            r = int(r) - cut
            want.append(want[-1] + ((r - size) // step + 1 if r >= size else 0))
        assert list(win_off) == want and dev.shape == (want[-1], nc * per)
        assert want[2] == want[1] and want[-1] > 60                    # the empty utterance leaves no row
        for u in range(len(lens)):
            x = lld[b.frame_offsets[u]:b.frame_offsets[u + 1], c0:c0 + nc]
            x = x[:max(0, x.shape[0] - cut)]
            sl = slices(x, size, step)
            assert len(sl) == win_off[u + 1] - win_off[u]
            for k, s in enumerate(sl):
                check(oracle, spec, dev[win_off[u] + k].reshape(nc, per), oracle.funcspec(s, as_oracle_spec(oracle, spec)),
                      f"{inst}/utt{u}/window{k}")
    b.close()


def test_batch_refusals(hip):
    import ctypes as C
    capi, ctx = hip
    L = capi.load()
    plan = capi.Plan(ctx, capi.is09_lld_config())
    b = capi.Batch(plan, np.array([0, 16000], np.int64))
    with pytest.raises(capi.SmileHipError, match="size_rows and step_rows"):
        b.func_windows(0, 1)
    from test_func_windows_host import modulation_spec
    s = modulation_spec()
    rc = L.smilehip_batch_funcspec_windows(plan._h, b._h, C.byref(s), None, 32, 0, 32, 0, 20, 5, None, 32 * 11, None)
    assert rc == -1 and b"Modulation" in L.smilehip_last_error()
    b.close()


def test_strides_and_pads(hip):
    """Odd ld_lld / ld_func: the NaN pads of the input are never read into a value, those of the output stay untouched."""
    capi, ctx = hip
    rng = np.random.default_rng(3)
    for name, cols in (("is09", 32), ("c16:Nz", 7), ("c16:LLD", 33)):
        spec = make_spec(capi, name)
        per = capi.funcspec_count(spec)
        x = edge_data(rng, 41, cols)
        dense = capi.funcspec_matrix_windows_host(ctx, spec, x, 10, 3)
        vals, padded = capi.funcspec_matrix_windows_host(ctx, spec, x, 10, 3, ld_lld=cols + 3, ld_func=cols * per + 5)
        assert dense.shape[0] == 11 and bits_equal(vals, dense), name
        assert padded.shape == (11, cols * per + 5) and np.isnan(padded[:, cols * per:]).all(), name
        assert np.isfinite(dense).all()
    # the batch entry point: a column sub-range of a 130-wide matrix (ld_lld = 130 around 7 columns), odd ld_func
    from opensmile_amd import synth
    plan = capi.Plan(ctx, capi.compare16_config())
    lens = [9000, 2560, 4160]
    b = capi.Batch(plan, np.concatenate([[0], np.cumsum(lens)]).astype(np.int64))
    lld = b.run_host(np.concatenate([synth.utterance(80 + i, n) for i, n in enumerate(lens)]))
    spec = capi.funcspec_compare16("Nz")
    per = capi.funcspec_count(spec)
    dense, win_off = b.funcspec_windows_host(lld, spec, 3, 7, 0, 10, 5)
    poisoned = lld.copy()
    poisoned[:, :3] = np.nan
    poisoned[:, 10:] = np.nan                              # the columns outside the range are never read into a value
    padded, _ = b.funcspec_windows_host(poisoned, spec, 3, 7, 0, 10, 5, ld_func=7 * per + 3)
    assert dense.shape[0] == win_off[-1] == 9 + 1 + 3 and bits_equal(np.ascontiguousarray(padded[:, :7 * per]), dense)
    assert np.isnan(padded[:, 7 * per:]).all() and np.isfinite(dense).all()
    b.close()


def test_one_window_of_the_whole_utterance_is_full_mode(hip):
    """A window of exactly the utterance's rows = smilehip_batch_funcspec with rows_cut = 0, bit for bit."""
    capi, ctx = hip
    from opensmile_amd import synth
    plan = capi.Plan(ctx, capi.is09_lld_config())
    b = capi.Batch(plan, np.array([0, 16000], np.int64))
    lld = b.run_host(synth.utterance(4, 16000))
    rows = lld.shape[0]
    assert rows == 99
    for spec in (capi.funcspec_is09(), capi.funcspec_compare16("Nz"), capi.funcspec_compare16("LLD")):
        win, win_off = b.funcspec_windows_host(lld, spec, 0, 32, 0, rows, 1)
        assert list(win_off) == [0, 1]
        assert bits_equal(win, b.funcspec_host(lld, spec, 0, 32, 0))
    b.close()


def test_is09_windows_equal_the_real_binary(hip, golden):
    """The golden's files through smilehip_lld_run and smilehip_batch_funcspec_windows with smilehip_funcspec_is09: every one of
    the 384 values of every window is the real binary's bits, for every geometry of the fixture."""
    capi, ctx = hip
    from opensmile_amd import synth
    files = [(int(u), int(n)) for u, n in golden["files"]]
    plan = capi.Plan(ctx, capi.is09_lld_config())
    off = np.concatenate([[0], np.cumsum([n for _, n in files])]).astype(np.int64)
    b = capi.Batch(plan, off)
    lld = b.run_host(np.concatenate([synth.utterance(u, n) for u, n in files]))
    assert list(np.diff(b.frame_offsets)) == [int(golden[f"rows_{f}"]) for f in range(len(files))]
    spec = capi.funcspec_is09()
    total = 0
    for g in range(len(golden["geometries"])):
        size, step = int(golden[f"size_{g}"]), int(golden[f"step_{g}"])
        dev, win_off = b.funcspec_windows_host(lld, spec, 0, 32, 0, size, step)
        assert list(np.diff(win_off)) == [int(golden[f"n_{f}_{g}"]) for f in range(len(files))]
        for f in range(len(files)):
            ref = golden[f"func_{f}_{g}"]
            got = dev[win_off[f]:win_off[f + 1]]
            same = got.view(np.uint32) == ref.view(np.uint32)
            assert same.all(), (f"geometry {size}/{step}, file {f}: {int((~same).sum())} of {same.size} values differ, first at "
                                f"(window, value) {np.argwhere(~same)[:4].tolist()}: {got[~same][:4]} vs {ref[~same][:4]}")
            total += got.shape[0]
    assert total > 800
    b.close()


# ---- the front end: smilextract_hip --set is09_emotion -frameMode fixed
EXE = os.path.join(ROOT, "opensmile_amd", "smilextract_hip")
FILES = os.path.join(HERE, "golden", "files")


def test_front_end_writes_the_binarys_files(tmp_path):
    """ARFF and CSV of two files at frameSize 0.125 / frameStep 0.05 (13 rows every 5: the 12.5 rounds up): the bytes the real
    binary's sinks wrote for the same include file (tests/golden/files/is09_func_windows.*), one row per window with the window's
    frameTime in the CSV; a file shorter than a window -- first in the list -- writes no row."""
    from opensmile_amd import synth
    from oracle import lldo
    short = str(tmp_path / "short.wav")
    lldo.write_wav(short, synth.utterance(1, 1500))                    # 8 LLD rows
    lst = tmp_path / "list.txt"
    lst.write_text(f"{short}\tshort\n{os.path.join(FILES, 'u2_8000.wav')}\ta.wav\n{os.path.join(FILES, 'u3_4000.wav')}\tb'x\n")
    od = tmp_path / "out"
    od.mkdir()
    arff, fcsv = str(tmp_path / "f.arff"), str(tmp_path / "f.csv")
    subprocess.run([EXE, "--set", "is09_emotion", "-filelist", str(lst), "-O", arff, "-csvoutput", fcsv, "-htkoutput", "1", "-outdir", str(od),
                    "-frameMode", "fixed", "-frameSize", "0.125", "-frameStep", "0.05", "-frameCenterSpecial", "left"], check=True)
    assert open(fcsv).read() == open(os.path.join(FILES, "is09_func_windows.csv")).read()
    assert open(arff).read() == open(os.path.join(FILES, "is09_func_windows.arff")).read()
    assert open(fcsv).read().count("\n") == 1 + 8 + 3
    # the per-file functionals HTK file: one row per window, none for the short file
    assert not (od / "short.func.htk").exists()
    rows = np.frombuffer((od / "u3_4000.func.htk").read_bytes()[12:], ">f4").reshape(-1, 384)
    vals = np.array([ln.split(";")[2:] for ln in open(fcsv).read().splitlines()[9:]], np.float64)
    assert rows.shape == vals.shape == (3, 384) and np.allclose(rows, vals, rtol=2e-6, atol=0)


def test_front_end_full_mode_is_unchanged(tmp_path):
    """-frameMode full (and no option at all) is the one-row-per-file route."""
    outs = []
    for extra in ([], ["-frameMode", "full"]):
        fcsv = str(tmp_path / f"f{len(outs)}.csv")
        subprocess.run([EXE, "--set", "is09_emotion", "-I", os.path.join(FILES, "u2_8000.wav"), "-csvoutput", fcsv] + extra, check=True)
        outs.append(open(fcsv).read())
    assert outs[0] == outs[1] and outs[0].count("\n") == 2


def test_front_end_refusals(tmp_path):
    wav = os.path.join(FILES, "u2_8000.wav")

    def refused(*args):
        r = subprocess.run([EXE, *args, "-I", wav, "-csvoutput", str(tmp_path / "x.csv")], capture_output=True, text=True)
        assert r.returncode != 0 and not (tmp_path / "x.csv").exists()
        return r.stderr
    fixed = ["-frameMode", "fixed", "-frameSize", "0.125", "-frameStep", "0.05"]
    assert "-frameMode fixed" in refused("--set", "egemapsv02", *fixed)
    assert "-frameMode fixed" in refused("--set", "compare16", *fixed)
    assert "-frameCenterSpecial mid" in refused("--set", "is09_emotion", *fixed, "-frameCenterSpecial", "mid")
    assert "-frameMode var" in refused("--set", "is09_emotion", "-frameMode", "var")
    assert "frameSize" in refused("--set", "is09_emotion", "-frameMode", "fixed", "-frameSize", "0.004", "-frameStep", "0.05")
    assert "frameStep" in refused("--set", "is09_emotion", "-frameMode", "fixed", "-frameSize", "0.1", "-frameStep", "0")
    assert "--gather" in refused("--set", "is09_emotion", *fixed, "--gather")
