#!/usr/bin/env python3
"""Generate the chroma_fft fixtures under tests/golden/ by running the REAL reference binary (oracle/_ref/SMILExtract, built by
oracle/Makefile) on config/chroma/chroma_fft.conf:

    chroma_fft_synth.npz    per input: where its samples come from (synth.utterance index, length, rate), the tapped levels
                            `tonespec` (72 columns) and `chroma` (12) as cHtkSink wrote them, for the short inputs the level
                            `fftmag` as well, the CSV file's text; the same for edited copies of the file; the header line of a
                            printHeader = 1 copy
    hard_chroma_fft.npz     the chroma level for the hard-signal corpus (tests/helpers/hard_signals.py)
    files/chroma_fft_*.csv  the binary's output files for files/u2_8000.wav and files/u3_4000.wav

The file's one sink is a cCsvSink that prints seven digits, so the bits come from taps: the binary runs twice per input, on the
shipped file and on a copy written into a temporary directory with cHtkSink instances on fftmag, tonespec and chroma appended. The
copy's CSV file must equal the shipped run's byte for byte.

Run from the repo root where the reference is built:
    python tests/golden/make_golden_chroma_fft.py
The fixtures are committed; the GPU box only reads them."""
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import lldo  # noqa: E402
from opensmile_amd import synth  # noqa: E402
from helpers import hard_signals  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
CONF_REL = os.path.join("chroma", "chroma_fft.conf")

# (synth.utterance index, samples, rate, divisor): 0, N - 1, N, N + H - 1, N + H, N + 2H samples at 16 kHz (N = 1024, H = 160: the row rule),
# 1 s and 3 s; then one short input per other rate (Nfft 512: 8 kHz, 1024: 11.025 kHz, 2048: 22.05 / 32 kHz, 4096: 44.1 / 48 kHz; 64 ms
# is no whole number of samples at 11.025 / 22.05 / 44.1 kHz, and the frame is no power of two at 11.025 / 22.05 / 44.1 / 48 kHz)
# The two long cuts are divided by 128 and 64: at full scale the synthetic noise floor keeps every class sum above silThresh, divided
# the envelope's minima fall below it and whole rows come out zero (what main() asserts about the level).
INPUTS = [(2, 0, 16000, 1), (3, 1023, 16000, 1), (4, 1024, 16000, 1), (5, 1183, 16000, 1), (6, 1184, 16000, 1), (7, 1344, 16000, 1),
          (2, 16000, 16000, 128), (3, 48000, 16000, 64), (4, 1000, 8000, 1), (5, 1300, 11025, 1), (6, 2400, 22050, 1),
          (7, 3400, 32000, 1), (8, 4400, 44100, 1), (9, 4800, 48000, 1)]
LONG = (6, 7)                                              # the 16 kHz inputs of a second or more: no fftmag level in the fixture

TAP = """
[componentInstances:cComponentManager]
instance[tap_mag].type=cHtkSink
instance[tap_ts].type=cHtkSink
instance[tap_chroma].type=cHtkSink
[tap_mag:cHtkSink]
reader.dmLevel=fftmag
filename=tap_mag.htk
[tap_ts:cHtkSink]
reader.dmLevel=tonespec
filename=tap_ts.htk
[tap_chroma:cHtkSink]
reader.dmLevel=chroma
filename=tap_chroma.htk
"""
TAPS = (("fftmag", "tap_mag.htk"), ("tonespec", "tap_ts.htk"), ("chroma", "tap_chroma.htk"))

# edited copies: (key suffix, {text of the shipped file: replacement})
EDITS = [("o5tri", {"nOctaves = 6": "nOctaves = 5", "firstNote = 55": "firstNote = 110", "filterType = gau": "filterType = tri",
                    "usePower = 1": "usePower = 0", "dbA = 1": "dbA = 0"}),
         ("trp", {"filterType = gau": "filterType = trp"}),
         ("rec", {"filterType = gau": "filterType = rec"}),
         ("os24", {"octaveSize = 12": "octaveSize = 24"}),
         ("sil0", {"octaveSize = 12": "octaveSize = 12\nsilThresh = 0"})]
EDIT_INPUTS = (5, 6)                                       # N + 2H samples and 1 s


def cut(idx, n, div=1):
    """the samples of an input: synth.utterance(idx, n), floor-divided by div"""
    if not n:
        return np.zeros(0, np.int16)
    return (synth.utterance(idx, n).astype(np.int32) // div).astype(np.int16)


def edited_text(edits=None, header=False):
    text = open(os.path.join(lldo.REF_DIR, "config", CONF_REL), encoding="latin-1").read()
    for a, b in (edits or {}).items():
        assert text.count(a) == 1, a
        text = text.replace(a, b)
    if header:
        assert text.count("printHeader = 0") == 1
        text = text.replace("printHeader = 0", "printHeader = 1")
    return text


def tapped_conf(td, edits=None, header=False, tap=True):
    path = os.path.join(td, "chroma_fft_tap.conf")
    with open(path, "w", encoding="latin-1") as f:
        f.write(edited_text(edits, header) + (TAP if tap else ""))
    return path


def read_level(path):
    if not os.path.exists(path) or os.path.getsize(path) <= 12:
        return None
    return lldo.read_htk(path)[0]


def run(pcm, fs, conf, td, tag):
    exe = os.path.join(lldo.REF_DIR, "SMILExtract")
    wav, csv = os.path.join(td, tag + ".wav"), os.path.join(td, tag + ".csv")
    lldo.write_wav(wav, pcm, fs)
    for p in [csv] + [os.path.join(td, t[1]) for t in TAPS]:
        if os.path.exists(p):
            os.remove(p)
    r = subprocess.run([exe, "-C", conf, "-I", wav, "-O", csv, "-l", "0"], cwd=td, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    out = dict(csv=open(csv).read() if os.path.exists(csv) else "", rc=r.returncode)
    for key, name in TAPS:
        out[key] = read_level(os.path.join(td, name))
    return out


def tmpdir():
    return tempfile.TemporaryDirectory(dir="/dev/shm" if os.path.isdir("/dev/shm") else None)


def reference(pcm, fs=16000, edits=None):
    """{csv, fftmag, tonespec, chroma} of one input: the (edited) file as it is, then its tapped copy"""
    with tmpdir() as td:
        a = run(pcm, fs, tapped_conf(td, edits, tap=False) if edits else os.path.join(lldo.REF_DIR, "config", CONF_REL), td, "a")
        b = run(pcm, fs, tapped_conf(td, edits), td, "b")
    assert a["csv"] == b["csv"], "the tapped copy changed the CSV file"
    rows = len(a["csv"].splitlines())
    for key, _ in TAPS:
        if b[key] is None:
            assert rows == 0, (key, rows)
        else:
            assert len(b[key]) == rows, (key, len(b[key]), rows)
    return b


def store(d, suffix, r, with_mag):
    ts, ch = r["tonespec"], r["chroma"]
    d["tonespec_" + suffix] = ts if ts is not None else np.zeros((0, 0), np.float32)
    d["chroma_" + suffix] = ch if ch is not None else np.zeros((0, 0), np.float32)
    if with_mag:
        d["fftmag_" + suffix] = r["fftmag"] if r["fftmag"] is not None else np.zeros((0, 0), np.float32)
    d["csv_" + suffix] = np.array(r["csv"])


def main():
    lldo.build()
    assert lldo.have_ref(), "oracle/_ref/SMILExtract missing (the reference is not built)"
    d = {"inputs": np.array(INPUTS, np.int64)}
    zero_rows = one_rows = 0
    long_rows = long_nonzero = 0
    gap = False
    for k, (idx, n, fs, div) in enumerate(INPUTS):
        r = reference(cut(idx, n, div), fs)
        store(d, str(k), r, k not in LONG)
        ts, ch = d["tonespec_%d" % k], d["chroma_%d" % k]
        print("input", (idx, n, fs, div), "rows", len(ch), "tonespec", ts.shape, "chroma", ch.shape, "fftmag",
              None if r["fftmag"] is None else r["fftmag"].shape, "rc", r["rc"])
        if k in LONG:                                      # what the chroma level holds: a level of zeros would pass any test
            assert ts.shape[1] == 72 and ch.shape[1] == 12
            nz = (ch != 0).any(axis=1)
            s = ch.astype(np.float64).sum(axis=1)
            zero_rows += int((~nz).sum())
            one_rows += int((np.abs(s[nz] - 1.0) < 1e-5).sum())
            assert (np.abs(s[nz] - 1.0) < 1e-5).all()
            long_rows += len(ch)
            long_nonzero += int(nz.sum())
            used = (ts != 0).any(axis=0)
            empty = [c for c in range(1, 71) if not used[c] and used[:c].any() and used[c + 1:].any()]
            gap = gap or bool(empty)
            print("   non-zero rows", int(nz.sum()), "of", len(ch), "notes never set between set ones", empty)
    assert zero_rows > 0 and one_rows > 0, "the chroma level needs all-zero rows and rows that sum to 1: choose other synth indices"
    assert 4 * long_nonzero >= long_rows, "fewer than a quarter of the rows are non-zero: choose other synth indices or scale the cut"
    assert gap, "no note without bins between non-zero notes"
    for tag, edits in EDITS:
        for k in EDIT_INPUTS:
            idx, n, fs, div = INPUTS[k]
            r = reference(cut(idx, n, div), fs, edits)
            store(d, "%s_%d" % (tag, k), r, k not in LONG)
            print(tag, "input", (idx, n, fs, div), "tonespec", d["tonespec_%s_%d" % (tag, k)].shape, "chroma", d["chroma_%s_%d" % (tag, k)].shape,
                  "differs from the shipped file's:", r["csv"] != str(d["csv_%d" % k]),
                  "non-zero rows", int((d["chroma_%s_%d" % (tag, k)] != 0).any(axis=1).sum()))
    with tmpdir() as td:                                   # the names: a header-printing copy
        idx, n, fs, div = INPUTS[5]
        r = run(cut(idx, n, div), fs, tapped_conf(td, None, header=True, tap=False), td, "h")
    d["csv_header"] = np.array(r["csv"].splitlines()[0])
    print("header:", d["csv_header"])
    np.savez_compressed(os.path.join(OUT, "chroma_fft_synth.npz"), **d)
    h = {}
    for name, pcm in hard_signals.signals().items():
        r = reference(pcm)
        h["chroma_" + name] = r["chroma"] if r["chroma"] is not None else np.zeros((0, 12), np.float32)
        print(name, h["chroma_" + name].shape, "non-zero rows", int((h["chroma_" + name] != 0).any(axis=1).sum()))
    np.savez_compressed(os.path.join(OUT, "hard_chroma_fft.npz"), **h)
    conf = os.path.join(lldo.REF_DIR, "config", CONF_REL)
    with tempfile.TemporaryDirectory() as td:
        for stem in ("u2_8000", "u3_4000"):
            exe = os.path.join(lldo.REF_DIR, "SMILExtract")
            subprocess.run([exe, "-C", conf, "-I", os.path.join(OUT, "files", stem + ".wav"), "-O", os.path.join(td, "o.csv"), "-l", "0"],
                           check=True, cwd=td)
            shutil.copy(os.path.join(td, "o.csv"), os.path.join(OUT, "files", "chroma_fft_%s.csv" % stem))
    for f in ("chroma_fft_synth.npz", "hard_chroma_fft.npz", "files/chroma_fft_u2_8000.csv", "files/chroma_fft_u3_4000.csv"):
        print(f, os.path.getsize(os.path.join(OUT, f)), "bytes")


if __name__ == "__main__":
    main()
