#!/usr/bin/env python3
"""Generate tests/golden/func_windows_is09.npz: the REAL reference binary (oracle/_ref/SMILExtract) on is09-13/IS09_emotion.conf
with the functionals' frame mode include replaced (-frameModeFunctionalsConf) by

    frameMode = fixed, frameSize = S, frameStep = P, frameCenterSpecial = left

for the synth.utterance files of FILES (LLD rows L = 8, 12, 29, 99, 369) and every (S, P) of GEOMETRIES. Per file f and geometry g:

    rows_f         L, the rows of the LLD level (-lldhtkoutput)
    size_g, step_g the window geometry in rows that the window counts and frame times imply (see geometry_rows)
    n_f_g          windows
    time_f_g       frameTime of every window as the CSV sink prints it
    func_f_g       n x 384 float32, the HTK sink's bits

It also records tests/golden/files/is09_func_windows.arff and .csv: the binary's own ARFF and CSV sinks for the two files of
tests/golden/files (u2_8000.wav as instance "a.wav", u3_4000.wav as "b'x", appended into one file each) with frameSize 0.125 and
frameStep 0.05 -- what the front-end test compares smilextract_hip's files with, byte for byte.

The include file is written at run time. Run from the repo root where the reference is built:
    python tests/golden/make_golden_func_windows.py
The .npz is committed; the GPU box only reads it."""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import lldo  # noqa: E402
from opensmile_amd import synth  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "func_windows_is09.npz")
FILES = ((1, 1500), (2, 2000), (3, 4800), (4, 16000), (5, 59200))           # (synth.utterance index, samples)
GEOMETRIES = ((0.1, 0.01), (0.125, 0.05), (0.135, 0.135), (0.03, 0.02), (1.0, 0.5))
PERIOD = 0.01


def frame_mode_include(path, size, step, center="left"):
    with open(path, "w") as f:
        f.write(f"frameMode = fixed\nframeSize = {size!r}\nframeStep = {step!r}\nframeCenterSpecial = {center}\n")


def run_windows(pcm, size, step, td):
    """(lld rows, frame times, func n x 384) of the binary for one file and one geometry"""
    exe = os.path.join(lldo.REF_DIR, "SMILExtract")
    conf = os.path.join(lldo.REF_DIR, "config", "is09-13", "IS09_emotion.conf")
    inc = os.path.join(td, "fm.conf.inc")
    frame_mode_include(inc, size, step)
    wav, htk, csv, lld = (os.path.join(td, n) for n in ("in.wav", "f.htk", "f.csv", "l.htk"))
    for p in (htk, csv, lld):
        if os.path.exists(p):
            os.remove(p)
    lldo.write_wav(wav, pcm)
    subprocess.run([exe, "-C", conf, "-I", wav, "-frameModeFunctionalsConf", inc, "-htkoutput", htk, "-csvoutput", csv,
                    "-lldhtkoutput", lld, "-l", "0"], check=True, cwd=td, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    rows = lldo.read_htk(lld)[0].shape[0] if os.path.exists(lld) else 0
    func = lldo.read_htk(htk)[0] if os.path.exists(htk) and os.path.getsize(htk) > 12 else np.zeros((0, 384), np.float32)
    times = []
    if os.path.exists(csv):
        lines = open(csv).read().splitlines()
        col = lines[0].split(";").index("frameTime")
        times = [float(ln.split(";")[col]) for ln in lines[1:] if ln.strip()]
    assert len(times) == func.shape[0], (len(times), func.shape)
    return rows, np.array(times, np.float64), np.ascontiguousarray(func, np.float32)


def geometry_rows(counts, times, size_sec, step_sec, td):
    """The (size, step) in rows behind one geometry's windows, from the binary alone: the step from the frame times (frameTime of
    window k = k step PERIOD); the size from the counts (n = (L - size) // step + 1 for every file that has a window, 0 for those
    below) and, where several sizes fit them, from probe files of exactly L = size and L = size - 1 rows (one window, none)."""
    steps = {int(round((t[1] - t[0]) / PERIOD)) for t in times if len(t) > 1}
    assert len(steps) == 1, steps
    step = steps.pop()
    sizes = [s for s in range(1, 400) if all((n == ((L - s) // step + 1 if L >= s else 0)) for L, n in counts)]

    def windows_of(L):                                     # a file of L LLD rows: 25 ms frames every 10 ms, one row more than frames
        rows, t, _ = run_windows(synth.utterance(7, 400 + 160 * (L - 2)), size_sec, step_sec, td)
        assert rows == L, (rows, L)
        return len(t)
    if len(sizes) > 1:
        sizes = [s for s in sizes if s >= 3 and windows_of(s) == 1 and windows_of(s - 1) == 0]
    assert len(sizes) == 1, (sizes, counts)
    return sizes[0], step


def write_files(td):
    """the ARFF / CSV sinks' text for the two wave files of tests/golden/files at 0.125 / 0.05"""
    exe = os.path.join(lldo.REF_DIR, "SMILExtract")
    conf = os.path.join(lldo.REF_DIR, "config", "is09-13", "IS09_emotion.conf")
    files = os.path.join(os.path.dirname(os.path.abspath(__file__)), "files")
    inc = os.path.join(td, "fm_files.conf.inc")
    frame_mode_include(inc, 0.125, 0.05)
    arff, csv = os.path.join(td, "w.arff"), os.path.join(td, "w.csv")
    for wav, name in (("u2_8000.wav", "a.wav"), ("u3_4000.wav", "b'x")):
        subprocess.run([exe, "-C", conf, "-I", os.path.join(files, wav), "-frameModeFunctionalsConf", inc, "-O", arff, "-csvoutput", csv,
                        "-instname", name, "-l", "0"], check=True, cwd=td, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    for src, dst in ((arff, "is09_func_windows.arff"), (csv, "is09_func_windows.csv")):
        text = open(src).read()
        open(os.path.join(files, dst), "w").write(text)
        print(dst, len(text), "bytes,", text.count("\n"), "lines")


def main():
    lldo.build()
    assert lldo.have_ref(), "oracle/_ref/SMILExtract missing (the reference is not built)"
    d = {"files": np.array(FILES, np.int64), "geometries": np.array(GEOMETRIES, np.float64)}
    with tempfile.TemporaryDirectory() as td:
        for g, (size, step) in enumerate(GEOMETRIES):
            counts, times = [], []
            for f, (u, n) in enumerate(FILES):
                rows, t, func = run_windows(synth.utterance(u, n), size, step, td)
                d[f"rows_{f}"] = np.int64(rows)
                d[f"n_{f}_{g}"] = np.int64(func.shape[0])
                d[f"time_{f}_{g}"] = t
                d[f"func_{f}_{g}"] = func
                counts.append((rows, func.shape[0]))
                times.append(t)
            sr, st = geometry_rows(counts, times, size, step, td)
            d[f"size_{g}"], d[f"step_{g}"] = np.int64(sr), np.int64(st)
            print((size, step), "->", (sr, st), counts)
        write_files(td)
    np.savez_compressed(OUT, **d)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
