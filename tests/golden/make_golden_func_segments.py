#!/usr/bin/env python3
"""Generate tests/golden/func_segments_is09.npz: the REAL reference binary (oracle/_ref/SMILExtract) on is09-13/IS09_emotion.conf
with the functionals' frame mode include replaced (-frameModeFunctionalsConf) by

    frameMode = list, frameList = <list>, frameCenterSpecial = left

for the synth.utterance files of FILES (LLD rows L = 12, 29, 99, 369) and every list of LISTS (at L = 369 also BIG_LIST: 40
segments of 2 .. 4, 64 / 65 and 300 rows that overlap, nest and repeat). Per file f and list l:

    rows_f          L, the rows of the LLD level (-lldhtkoutput)
    n_f_l           vectors the binary wrote
    time_f_l        frameTime of every vector as the CSV sink prints it
    func_f_l        n x 384 float32, the HTK sink's bits
    first_f_l, len_f_l   the rows [first, first + len) behind every vector

The rows behind a vector are identified from the binary alone: `first` is the vector's frameTime in periods, and `len` is the one
window size R for which window `first` of the binary's own frameMode = fixed output (frameSize = R periods, frameStep = one
period) equals the vector bit for bit. (The sizes are tried nearest first around what the list's text suggests; the comparison
decides, and exactly one size must match.)

It also records tests/golden/files/is09_func_segments.arff and .csv: the binary's own ARFF and CSV sinks for the two files of
tests/golden/files (u2_8000.wav as instance "a.wav" with FILE_LISTS[0], u3_4000.wav as "b'x" with FILE_LISTS[1], appended into one
file each) -- what the front-end test compares smilextract_hip's files with, byte for byte.

The include file is written at run time. Run from the repo root where the reference is built:
    python tests/golden/make_golden_func_segments.py
The .npz is committed; the GPU box only reads it."""
import math
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import lldo  # noqa: E402
from opensmile_amd import synth  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "func_segments_is09.npz")
FILES = ((2, 2000), (3, 4800), (4, 16000), (5, 59200))           # (synth.utterance index, samples): L = 12, 29, 99, 369
LISTS = ("10-50", "0.3s-0.9s", "20,30,10", "0.2s,0.3s", "0.105s-0.2049s", "0.5s-0.98s", "0.29s-0.57s,0.07s-0.14s", "3-3", "5-6",
         "0-98", "0-99", "0.3s-0.9s,0.1s-0.5s", "0.1s-0.5s,0.1s-0.5s", "0.0s-0.5s,0.2s-5.0s,0.1s-0.3s",
         "0.5s-0.97s,0.5s-0.98s,0.5s-0.99s,0.5s-1.0s")
FILE_LISTS = ("10-30,0-20,25-45,10-30", "0.05s,0.08s,0.07s")
PERIOD = 0.01


def big_list():
    """40 segments in seconds for the file of 369 rows: short ones, 64 / 65 rows, 300 rows; overlapping, nested, repeated"""
    rng = np.random.default_rng(20261020)
    seg = []
    for k in range(40):
        kind = k % 4
        if kind == 0:
            a = int(rng.integers(0, 360)); b = a + int(rng.integers(1, 3))
        elif kind == 1:
            a = int(rng.integers(0, 300)); b = a + 63
        elif kind == 2:
            a = int(rng.integers(0, 300)); b = a + 64
        else:
            a = int(rng.integers(0, 60)); b = a + 299
        seg.append((a, b))
    seg[5] = seg[1]                                        # a repeat
    seg[6] = (seg[3][0] + 10, seg[3][0] + 74)              # nested in a 300-row one
    return ",".join("%.2fs-%.2fs" % (a / 100.0, b / 100.0) for a, b in seg)


def include(path, text):
    with open(path, "w") as f:
        f.write(text)


def run_binary(wav_path, inc_text, td, extra=()):
    """(lld rows, frame times, func n x 384) of the binary for one file and one frame mode include"""
    exe = os.path.join(lldo.REF_DIR, "SMILExtract")
    conf = os.path.join(lldo.REF_DIR, "config", "is09-13", "IS09_emotion.conf")
    inc = os.path.join(td, "fm.conf.inc")
    include(inc, inc_text)
    htk, csv, lld = (os.path.join(td, n) for n in ("f.htk", "f.csv", "l.htk"))
    for p in (htk, csv, lld):
        if os.path.exists(p):
            os.remove(p)
    r = subprocess.run([exe, "-C", conf, "-I", wav_path, "-frameModeFunctionalsConf", inc, "-htkoutput", htk, "-csvoutput", csv,
                        "-lldhtkoutput", lld, "-l", "0", *extra], cwd=td, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    assert r.returncode == 0, (inc_text, r.returncode)
    rows = lldo.read_htk(lld)[0].shape[0] if os.path.exists(lld) else 0
    func = lldo.read_htk(htk)[0] if os.path.exists(htk) and os.path.getsize(htk) > 12 else np.zeros((0, 384), np.float32)
    times = []
    if os.path.exists(csv):
        lines = open(csv).read().splitlines()
        col = lines[0].split(";").index("frameTime")
        times = [float(ln.split(";")[col]) for ln in lines[1:] if ln.strip()]
    assert len(times) == func.shape[0], (len(times), func.shape)
    return rows, np.array(times, np.float64), np.ascontiguousarray(func, np.float32)


def list_include(frame_list):
    return f"frameMode = list\nframeList = {frame_list}\nframeCenterSpecial = left\n"


def fixed_include(size_rows):
    return f"frameMode = fixed\nframeSize = {size_rows * PERIOD!r}\nframeStep = {PERIOD!r}\nframeCenterSpecial = left\n"


class Fixed:
    """the binary's fixed windows of one file, one size at a time"""

    def __init__(self, wav, rows, td):
        self.wav, self.rows, self.td, self.cache = wav, rows, td, {}

    def windows(self, size):
        if size not in self.cache:
            rows, t, func = run_binary(self.wav, fixed_include(size), self.td)
            assert rows == self.rows and func.shape[0] == max(0, rows - size + 1), (size, rows, func.shape)
            self.cache[size] = func
        return self.cache[size]

    def identify(self, vec, first, guess):
        """the one size R whose window `first` equals vec bit for bit"""
        cand = sorted(range(1, self.rows - first + 1), key=lambda r: abs(r - guess))
        hit = [r for r in cand[:12] if np.array_equal(self.windows(r)[first].view(np.uint32), vec.view(np.uint32))]
        if not hit:                                        # the text's suggestion was far off: every size
            hit = [r for r in cand if np.array_equal(self.windows(r)[first].view(np.uint32), vec.view(np.uint32))]
        assert len(hit) == 1, (first, guess, hit)
        return hit[0]


def guesses(frame_list):
    """what the list's text suggests as segment lengths, only to order the sizes identify() tries"""
    out, last = [], 0.0
    for tok in frame_list.split(","):
        sec = "s" in tok
        if "-" in tok:
            a, b = (float(v.strip().rstrip("s")) for v in tok.split("-"))
        else:
            a, b = last, last + float(tok.strip().rstrip("s")) - (0 if sec else 1)
            last += float(tok.strip().rstrip("s"))
        out.append(int(math.ceil(b / PERIOD) - math.floor(a / PERIOD)) + 1 if sec else int(b - a) + 1)
    return out


def write_files(td):
    """the ARFF / CSV sinks' text for the two wave files of tests/golden/files, one list each"""
    exe = os.path.join(lldo.REF_DIR, "SMILExtract")
    conf = os.path.join(lldo.REF_DIR, "config", "is09-13", "IS09_emotion.conf")
    files = os.path.join(os.path.dirname(os.path.abspath(__file__)), "files")
    arff, csv = os.path.join(td, "w.arff"), os.path.join(td, "w.csv")
    for (wav, name), fl in zip((("u2_8000.wav", "a.wav"), ("u3_4000.wav", "b'x")), FILE_LISTS):
        inc = os.path.join(td, "fm_files.conf.inc")
        include(inc, list_include(fl))
        subprocess.run([exe, "-C", conf, "-I", os.path.join(files, wav), "-frameModeFunctionalsConf", inc, "-O", arff, "-csvoutput", csv,
                        "-instname", name, "-l", "0"], check=True, cwd=td, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    for src, dst in ((arff, "is09_func_segments.arff"), (csv, "is09_func_segments.csv")):
        text = open(src).read()
        open(os.path.join(files, dst), "w").write(text)
        print(dst, len(text), "bytes,", text.count("\n"), "lines")


def main():
    lldo.build()
    assert lldo.have_ref(), "oracle/_ref/SMILExtract missing (the reference is not built)"
    lists = list(LISTS) + [big_list()]
    d = {"files": np.array(FILES, np.int64), "lists": np.array(lists), "file_lists": np.array(FILE_LISTS), "big": np.int64(len(LISTS))}
    with tempfile.TemporaryDirectory() as td:
        for f, (u, n) in enumerate(FILES):
            wav = os.path.join(td, f"in{f}.wav")
            lldo.write_wav(wav, synth.utterance(u, n))
            fixed = None
            for li, fl in enumerate(lists):
                if li == len(LISTS) and f != len(FILES) - 1:
                    continue                               # the long list: the longest file only
                rows, t, func = run_binary(wav, list_include(fl), td)
                fixed = fixed or Fixed(wav, rows, td)
                first = np.rint(t / PERIOD).astype(np.int64)
                assert np.allclose(first * PERIOD, t, atol=5e-7), t
                g = guesses(fl)
                length = np.array([fixed.identify(func[k], int(first[k]), g[k]) for k in range(len(t))], np.int64)
                d[f"rows_{f}"] = np.int64(rows)
                d[f"n_{f}_{li}"] = np.int64(func.shape[0])
                d[f"time_{f}_{li}"] = t
                d[f"func_{f}_{li}"] = func
                d[f"first_{f}_{li}"] = first
                d[f"len_{f}_{li}"] = length
                print(f"L = {rows}  {fl[:60]!r}: {list(zip(first.tolist(), length.tolist()))}")
        write_files(td)
    np.savez_compressed(OUT, **d)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
