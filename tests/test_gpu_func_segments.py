"""Functionals over listed segments (cWinToVecProcessor frameMode = list) on the batch path: smilehip_funcspec_matrix_segments and
smilehip_batch_funcspec_segments against the CPU oracle on every segment's slice (test_gpu_funcspec.check's rule), against the
full-mode entry point on the same slice (bits: the same device code), across the three percentile sorts in one launch, chunk
seams, lane packing of unequal neighbours and utterance boundaries, and -- for IS09_emotion -- against the real binary's bits
(tests/golden/func_segments_is09.npz, recorded by tests/golden/make_golden_func_segments.py)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from helpers import op_layouts as OL
from test_gpu_func_windows import SPECS, bits_equal, edge_data, make_spec
from test_gpu_funcspec import as_oracle_spec, check

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden", "func_segments_is09.npz")
COLS = (1, 25, 32, 33, 64, 65)             # packing with idle lanes, exact packing, no packing, two column groups
# unequal neighbours in a packed wave, a duplicate, nesting, one row, the whole matrix, the last row, out of order
SEGMENTS = ((0, 3), (5, 30), (2, 1), (0, 40), (39, 1), (10, 10), (10, 10), (7, 17))


@pytest.fixture(scope="module")
def hip():
    from opensmile_amd import capi
    return capi, capi.Context(0)


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def split(segments):
    return [a for a, _ in segments], [n for _, n in segments]


@pytest.mark.parametrize("name", SPECS)
def test_segments_equal_their_slices(hip, oracle, name):
    """Every output row equals the oracle on its slice (check's rule) and funcspec_matrix_host on its slice bit for bit."""
    capi, ctx = hip
    spec = make_spec(capi, name)
    per = capi.funcspec_count(spec)
    ospec = as_oracle_spec(oracle, spec)
    rng = np.random.default_rng(29)
    full = {}
    for cols in COLS:
        x = edge_data(rng, 40, cols)
        dev = capi.funcspec_matrix_segments_host(ctx, spec, x, *split(SEGMENTS))
        assert dev.shape == (len(SEGMENTS), cols * per)
        for k, (a, n) in enumerate(SEGMENTS):
            what = f"{name}/cols{cols}/segment{k}"
            s = np.ascontiguousarray(x[a:a + n])
            got = dev[k].reshape(cols, per)
            check(oracle, spec, got, oracle.funcspec(s, ospec), what)
            if (cols, a, n) not in full:
                full[cols, a, n] = capi.funcspec_matrix_host(ctx, spec, s)
            assert bits_equal(got, full[cols, a, n]), what


def test_order_is_the_callers(hip):
    """A permuted list gives the permuted rows, bit for bit: the output row is the position in the list, whatever order the
    engine runs the segments in."""
    capi, ctx = hip
    spec = capi.funcspec_is09()
    rng = np.random.default_rng(31)
    x = edge_data(rng, 70, 32)
    seg = [(int(a), int(n)) for a, n in zip(rng.integers(0, 30, 23), rng.integers(1, 41, 23))]
    base = capi.funcspec_matrix_segments_host(ctx, spec, x, *split(seg))
    assert np.isfinite(base).all()
    for seed in (1, 2):
        perm = np.random.default_rng(seed).permutation(len(seg))
        got = capi.funcspec_matrix_segments_host(ctx, spec, x, *split([seg[i] for i in perm]))
        assert bits_equal(got, base[perm]), seed
    # no segment at all: nothing is written, no error
    assert capi.funcspec_matrix_segments_host(ctx, spec, x, [], []).shape == (0, 32 * 12)


def test_every_sort_class_in_one_launch(hip, oracle):
    """The wave sort (<= 1024 rows), the workgroup sort in LDS (<= 8192) and the sort in global scratch, short and long
    interleaved in the list; nonZeroFuncts makes the columns' lengths differ. A second call whose longest segment has 1024 rows
    launches no workgroup sort and gives the same rows."""
    capi, ctx = hip
    spec = capi.funcspec_compare16("Nz")
    per = capi.funcspec_count(spec)
    ospec = as_oracle_spec(oracle, spec)
    rng = np.random.default_rng(37)
    x = rng.standard_normal((8210, 5)).astype(np.float32)
    x[:, 1] = np.round(x[:, 1] * 2) / 2 + 0.0
    x[::5, 2] = 0.0
    x[:, 3] = np.abs(x[:, 3])
    seg = [(7, 3), (10, 8200), (100, 64), (0, 8192), (4000, 65), (18, 1025), (8207, 3), (3000, 1024)]
    dev = capi.funcspec_matrix_segments_host(ctx, spec, x, *split(seg))
    full = {}
    for k, (a, n) in enumerate(seg):
        s = np.ascontiguousarray(x[a:a + n])
        got = dev[k].reshape(5, per)
        check(oracle, spec, got, oracle.funcspec(s, ospec), f"Nz/segment{k} ({a}, {n})")
        full[a, n] = capi.funcspec_matrix_host(ctx, spec, s)
        assert bits_equal(got, full[a, n]), (a, n)
    short = [(k, s) for k, s in enumerate(seg) if s[1] <= 1024]
    assert len(short) == 5
    ran = []
    for segs in (seg, [s for _, s in short]):
        capi.kernel_timing(True)
        try:
            got = capi.funcspec_matrix_segments_host(ctx, spec, x, *split(segs))
            ran.append(set(capi.kernel_timing_report()))
        finally:
            capi.kernel_timing(False)
    assert "fs_percentiles_wave/seg" in ran[0] and "fs_percentiles/seg" in ran[0], ran[0]
    assert "fs_percentiles_wave/seg" in ran[1] and "fs_percentiles/seg" not in ran[1], ran[1]
    for j, (k, _) in enumerate(short):
        assert bits_equal(got[j], dev[k]), seg[k]


@pytest.mark.parametrize("inst", ["Nz", "LLD"])
def test_chunk_seams(hip, monkeypatch, inst):
    """SMILEHIP_FUNC_WINDOWS_SCRATCH_MB (read at every call) down to one segment per chunk and to a few: seams inside packed waves
    and between them; the compacted nonZeroFuncts copy (Nz) and Peaks2's alive bytes (LLD) are the scratch that is reused from
    chunk to chunk, at each chunk's own prefix of unequal lengths. Bit for bit the unbounded run."""
    capi, ctx = hip
    spec = capi.funcspec_compare16(inst)
    rng = np.random.default_rng(41)
    seg = [(int(a), int(n)) for a, n in zip(rng.integers(0, 20, 37), rng.integers(1, 41, 37))]
    for cols in (25, 65):
        x = edge_data(rng, 60, cols)
        monkeypatch.delenv("SMILEHIP_FUNC_WINDOWS_SCRATCH_MB", raising=False)
        whole = capi.funcspec_matrix_segments_host(ctx, spec, x, *split(seg))
        for k in (0, 5, 36):
            a, n = seg[k]
            assert bits_equal(whole[k].reshape(cols, -1), capi.funcspec_matrix_host(ctx, spec, np.ascontiguousarray(x[a:a + n])))
        for mb in ("0.000001", "0.01", "0.03"):            # one segment per chunk, then a few and a few more
            monkeypatch.setenv("SMILEHIP_FUNC_WINDOWS_SCRATCH_MB", mb)
            assert bits_equal(capi.funcspec_matrix_segments_host(ctx, spec, x, *split(seg)), whole), (inst, cols, mb)


@pytest.mark.parametrize("size,step", [(10, 1), (10, 25)])
def test_fixed_windows_as_a_list(hip, size, step):
    """The segments (k step, size) equal smilehip_funcspec_matrix_windows, bit for bit."""
    capi, ctx = hip
    rng = np.random.default_rng(43)
    x = edge_data(rng, 61, 25)
    for name in ("is09", "c16:Nz", "c16:LLD"):
        spec = make_spec(capi, name)
        win = capi.funcspec_matrix_windows_host(ctx, spec, x, size, step)
        n = (61 - size) // step + 1
        assert win.shape[0] == n >= 3
        seg = capi.funcspec_matrix_segments_host(ctx, spec, x, [k * step for k in range(n)], [size] * n)
        assert bits_equal(seg, win), name


def run_strided(capi, ctx, spec, x, seg, ld_lld, ld_func):
    """smilehip_funcspec_matrix_segments on padded() device buffers: the destination buffer as the call left it"""
    L = capi.load()
    rows, cols = x.shape
    first, n_rows = (np.array(v, np.int64) for v in split(seg))
    src, _ = OL.padded(x, ld_lld, np.nan)
    dst, _ = OL.padded(np.zeros((len(seg), 0), np.float32), ld_func, OL.SENTINEL)
    d_src, d_dst = C.c_void_p(), C.c_void_p()
    capi._check(L.smilehip_alloc(ctx._h, src.nbytes, C.byref(d_src)))
    capi._check(L.smilehip_alloc(ctx._h, dst.nbytes, C.byref(d_dst)))
    try:
        capi._check(L.smilehip_copy_to_device(ctx._h, d_src, src.ctypes.data, src.nbytes, None))
        capi._check(L.smilehip_copy_to_device(ctx._h, d_dst, dst.ctypes.data, dst.nbytes, None))
        capi._check(L.smilehip_funcspec_matrix_segments(ctx._h, C.byref(spec), d_src.value + 4 * OL.first_row_offset(ld_lld), ld_lld, rows, cols,
                                                        len(seg), first.ctypes.data, n_rows.ctypes.data,
                                                        d_dst.value + 4 * OL.first_row_offset(ld_func), ld_func, None))
        capi._check(L.smilehip_stream_synchronize(ctx._h, None))
        capi._check(L.smilehip_copy_to_host(ctx._h, dst.ctypes.data, d_dst, dst.nbytes, None))
    finally:
        L.smilehip_free(ctx._h, d_src)
        L.smilehip_free(ctx._h, d_dst)
    return dst


def test_strides_and_pads(hip):
    """Odd ld_lld > cols and ld_func > cols * per on buffers with poisoned pads, guard rows and unaligned rows
    (tests/helpers/op_layouts.py): the input's NaN pads are never read into a value, the output's pads, guards and lead are
    intact, and the rows equal the packed call's."""
    capi, ctx = hip
    rng = np.random.default_rng(47)
    for name, cols in (("is09", 32), ("c16:Nz", 7), ("c16:LLD", 33)):
        spec = make_spec(capi, name)
        per = capi.funcspec_count(spec)
        x = edge_data(rng, 40, cols)
        dense = capi.funcspec_matrix_segments_host(ctx, spec, x, *split(SEGMENTS))
        assert np.isfinite(dense).all()
        ld_lld, ld_func = cols + 3, cols * per + 5
        dst = run_strided(capi, ctx, spec, x, SEGMENTS, ld_lld, ld_func)
        OL.check_layout(dst, ld_func, cols * per, len(SEGMENTS), dense)
        # the capi mirror's own strides
        vals, padded = capi.funcspec_matrix_segments_host(ctx, spec, x, *split(SEGMENTS), ld_lld=ld_lld, ld_func=ld_func)
        assert bits_equal(vals, dense) and np.isnan(padded[:, cols * per:]).all()


@pytest.fixture(scope="module")
def batch4(hip):
    """four utterances of 0, 3, 1 (the whole utterance) and 2 (one ending on the last row) segments"""
    capi, ctx = hip
    from opensmile_amd import synth
    plan = capi.Plan(ctx, capi.is09_lld_config())
    lens = [4800, 16000, 2000, 8000]
    b = capi.Batch(plan, np.concatenate([[0], np.cumsum(lens)]).astype(np.int64))
    lld = b.run_host(np.concatenate([synth.utterance(90 + i, n) for i, n in enumerate(lens)]))
    yield b, lld
    b.close()


@pytest.mark.parametrize("rows_cut", [0, 1])
def test_batch(hip, batch4, rows_cut):
    """Every row equals the matrix call on that utterance's rows; rows_cut shortens what a segment may reach."""
    capi, ctx = hip
    b, lld = batch4
    rows = [int(r) - rows_cut for r in np.diff(b.frame_offsets)]
    assert rows == [29 - rows_cut, 99 - rows_cut, 12 - rows_cut, 49 - rows_cut]
    per_utt = [[], [(40, 30), (0, 5), (38, 40)], [(0, rows[2])], [(3, 20), (rows[3] - 7, 7)]]
    seg_off = np.concatenate([[0], np.cumsum([len(s) for s in per_utt])])
    flat = [s for u in per_utt for s in u]
    for spec, c0, nc in ((capi.funcspec_is09(), 0, 32), (capi.funcspec_compare16("Nz"), 3, 7)):
        per = capi.funcspec_count(spec)
        dev = b.funcspec_segments(lld, spec, c0, nc, rows_cut, seg_off, *split(flat))
        assert dev.shape == (6, nc * per)
        for u, segs in enumerate(per_utt):
            if not segs:
                continue
            x = np.ascontiguousarray(lld[b.frame_offsets[u]:b.frame_offsets[u] + rows[u], c0:c0 + nc])
            want = capi.funcspec_matrix_segments_host(ctx, spec, x, *split(segs))
            assert bits_equal(dev[seg_off[u]:seg_off[u + 1]], want), (u, rows_cut)
        # the whole utterance as one segment is full mode
        assert bits_equal(dev[3:4], b.funcspec_host(lld, spec, c0, nc, rows_cut)[2:3])


def test_refusals_leave_the_output_untouched(hip, batch4):
    """A segment one row too long, a zero-row segment and a non-monotone offset: the error names utterance and segment, and a
    poisoned output buffer is as it was."""
    capi, ctx = hip
    b, lld = batch4
    spec = capi.funcspec_is09()
    poison = np.float32(-12345.5)

    def refused(match, seg_off, segs, rows_cut=0):
        with pytest.raises(capi.SmileHipError, match=match) as e:
            b.funcspec_segments(lld, spec, 0, 32, rows_cut, np.array(seg_off, np.int64), *split(segs), fill=poison)
        out = e.value.output
        assert out.shape == (len(segs), 384) and (out == poison).all()
    good = [(40, 30), (0, 5), (0, 12), (3, 20)]
    assert np.isfinite(b.funcspec_segments(lld, spec, 0, 32, 0, [0, 0, 2, 3, 4], *split(good), fill=poison)).all()
    refused(r"utterance 1, segment 1.*\[60, 99\]", [0, 0, 2, 3, 4], [(40, 30), (60, 40), (0, 12), (3, 20)])
    refused(r"utterance 2, segment 0.*\[0, 11\]", [0, 0, 2, 3, 4], good, rows_cut=1)
    refused(r"utterance 3, segment 0.*0 rows", [0, 0, 2, 3, 4], [(40, 30), (0, 5), (0, 12), (3, 0)])
    refused(r"utterance 2.*not monotone", [0, 0, 3, 2, 4], good)
    refused(r"utterance 1, segment 0.*negative", [0, 0, 2, 3, 4], [(-1, 30), (0, 5), (0, 12), (3, 20)])
    # the matrix entry point
    x = np.ascontiguousarray(lld[:29, :32])
    with pytest.raises(capi.SmileHipError, match=r"utterance 0, segment 1.*\[20, 29\]") as e:
        capi.funcspec_matrix_segments_host(ctx, spec, x, [0, 20], [29, 10], fill=poison)
    assert (e.value.output == poison).all()


def test_is09_segments_equal_the_real_binary(hip, golden):
    """The golden's files through smilehip_lld_run and smilehip_batch_funcspec_segments with smilehip_funcspec_is09, the segments
    being those the binary was identified to have used: every one of the 384 values of every vector is the real binary's bits."""
    capi, ctx = hip
    from opensmile_amd import synth
    files = [(int(u), int(n)) for u, n in golden["files"]]
    plan = capi.Plan(ctx, capi.is09_lld_config())
    off = np.concatenate([[0], np.cumsum([n for _, n in files])]).astype(np.int64)
    b = capi.Batch(plan, off)
    lld = b.run_host(np.concatenate([synth.utterance(u, n) for u, n in files]))
    assert list(np.diff(b.frame_offsets)) == [int(golden[f"rows_{f}"]) for f in range(len(files))]
    spec = capi.funcspec_is09()
    lists = [str(s) for s in golden["lists"]]
    # one call for everything: utterance f owns the vectors of all its lists, one list after the other
    first, n_rows, ref, seg_off = [], [], [], [0]
    for f in range(len(files)):
        for li, fl in enumerate(lists):
            if f"n_{f}_{li}" not in golden:
                continue
            a, n = capi.func_list_parse(fl, 0.01)
            k = capi.func_list_fit(a, n, int(golden[f"rows_{f}"]))
            assert k == int(golden[f"n_{f}_{li}"])
            first += a[:k].tolist()
            n_rows += n[:k].tolist()
            ref.append(golden[f"func_{f}_{li}"])
        seg_off.append(len(first))
    ref = np.concatenate(ref)
    dev = b.funcspec_segments(lld, spec, 0, 32, 0, seg_off, first, n_rows)
    assert dev.shape == ref.shape == (92, 384)
    same = dev.view(np.uint32) == ref.view(np.uint32)
    assert same.all(), (f"{int((~same).sum())} of {same.size} values differ, first at (vector, value) {np.argwhere(~same)[:4].tolist()}: "
                        f"{dev[~same][:4]} vs {ref[~same][:4]}")
    b.close()


# ---- the front end: smilextract_hip --set is09_emotion -frameMode list
EXE = os.path.join(ROOT, "opensmile_amd", "smilextract_hip")
FILES = os.path.join(HERE, "golden", "files")


def test_front_end_writes_the_binarys_files(tmp_path, golden):
    """ARFF and CSV of two files, each with its own list in the file list's third column: the bytes the real binary's sinks wrote
    (tests/golden/files/is09_func_segments.*), one row per segment in list order, frameTime = the time of its first row."""
    la, lb = (str(s) for s in golden["file_lists"])
    lst = tmp_path / "list.txt"
    lst.write_text(f"{os.path.join(FILES, 'u2_8000.wav')}\ta.wav\t{la}\n{os.path.join(FILES, 'u3_4000.wav')}\tb'x\t{lb}\n")
    od = tmp_path / "out"
    od.mkdir()
    arff, fcsv = str(tmp_path / "f.arff"), str(tmp_path / "f.csv")
    subprocess.run([EXE, "--set", "is09_emotion", "-filelist", str(lst), "-O", arff, "-csvoutput", fcsv, "-htkoutput", "1", "-outdir", str(od),
                    "-frameMode", "list", "-frameList", "0-3"], check=True)          # (overridden by both third columns)
    assert open(fcsv).read() == open(os.path.join(FILES, "is09_func_segments.csv")).read()
    assert open(arff).read() == open(os.path.join(FILES, "is09_func_segments.arff")).read()
    assert open(fcsv).read().count("\n") == 1 + 4 + 3
    rows = np.frombuffer((od / "u3_4000.func.htk").read_bytes()[12:], ">f4").reshape(-1, 384)
    vals = np.array([ln.split(";")[2:] for ln in open(fcsv).read().splitlines()[5:]], np.float64)
    assert rows.shape == vals.shape == (3, 384) and np.allclose(rows, vals, rtol=2e-6, atol=0)


def test_front_end_list_options(tmp_path):
    """The same list through -frameList and through -frameListFile gives identical bytes; the file wins over the option; a list
    whose second segment does not fit writes one row, says so on stderr and exits 0."""
    wav = os.path.join(FILES, "u2_8000.wav")                           # 49 LLD rows
    flf = tmp_path / "frames.txt"
    flf.write_text("0.1s-0.3s,0.0s-0.2s\nsecond line, not read\n")         # only the first line is the list
    outs = []
    for extra in (["-frameList", "0.1s-0.3s,0.0s-0.2s"], ["-frameListFile", str(flf)], ["-frameListFile", str(flf), "-frameList", "0-10"]):
        fcsv = str(tmp_path / f"f{len(outs)}.csv")
        r = subprocess.run([EXE, "--set", "is09_emotion", "-I", wav, "-csvoutput", fcsv, "-frameMode", "list"] + extra, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        outs.append(open(fcsv).read())
    assert outs[0] == outs[1] == outs[2] and outs[0].count("\n") == 3
    assert [ln.split(";")[1] for ln in outs[0].splitlines()[1:]] == ["0.100000", "0.000000"]
    fcsv = str(tmp_path / "blocked.csv")
    r = subprocess.run([EXE, "--set", "is09_emotion", "-I", wav, "-csvoutput", fcsv, "-frameMode", "list", "-frameList", "0-20,30-49,5-10"],
                       capture_output=True, text=True)
    assert r.returncode == 0 and open(fcsv).read().count("\n") == 2
    assert "u2_8000.wav" in r.stderr and "segment 1" in r.stderr and r.stderr.count("does not fit") == 1


def test_front_end_refusals(tmp_path):
    wav = os.path.join(FILES, "u2_8000.wav")

    def refused(*args):
        r = subprocess.run([EXE, *args, "-I", wav, "-csvoutput", str(tmp_path / "x.csv")], capture_output=True, text=True)
        assert r.returncode != 0 and not (tmp_path / "x.csv").exists()
        return r.stderr
    lst = ["-frameMode", "list", "-frameList", "0-10"]
    assert "-frameMode list" in refused("--set", "egemapsv02", *lst)
    assert "-frameMode list" in refused("--set", "compare16", *lst)
    assert "--gather" in refused("--set", "is09_emotion", *lst, "--gather")
    assert "needs a list" in refused("--set", "is09_emotion", "-frameMode", "list")
    assert "-frameMode var" in refused("--set", "is09_emotion", "-frameMode", "var")
    assert "-frameMode meta" in refused("--set", "is09_emotion", "-frameMode", "meta")
    assert "10-E" in refused("--set", "is09_emotion", "-frameMode", "list", "-frameList", "0-5,10-E")
    assert "0.1s-0.5s" in refused("--set", "is09_emotion", "-frameMode", "list", "-frameList", "0-5,0.1s-0.5s")
    assert "30" in refused("--set", "is09_emotion", "-frameMode", "list", "-frameList", "0-5,30")
    assert "empty" in refused("--set", "is09_emotion", "-frameMode", "list", "-frameList", "0-5,,6-9")
