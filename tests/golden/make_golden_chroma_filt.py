#!/usr/bin/env python3
"""Generate the chroma_filt fixtures under tests/golden/ by running the REAL reference binary (oracle/_ref/SMILExtract, built by
oracle/Makefile) on config/chroma/chroma_filt.conf:

    chroma_filt_synth.npz    per input: where its samples come from (synth.utterance index, length, rate, divisor), the tapped levels
                             `tonespec` (72 columns) and `chroma` (12) as cHtkSink wrote them, the CSV file's text, the final double
                             states s, c of the g++ build of the row functions and D, the largest relative change of a state when
                             every libm sine and cosine is moved one ulp with a seeded random sign; the same for edited copies of
                             the file; the text of a printHeader = 1 / timestamp = 1 copy (names and row times)
    hard_chroma_filt.npz     both levels for the hard-signal corpus (tests/helpers/hard_signals.py)
    files/chroma_filt_*.csv  the binary's output files for files/u2_8000.wav and files/u3_4000.wav

The file's one sink is a cCsvSink that prints seven digits, so the bits come from taps: the binary runs twice per input, on the
shipped file and on a copy written into a temporary directory with cHtkSink instances on tonespec and chroma appended. The copy's
CSV file must equal the shipped run's byte for byte. The generator also runs the g++ build of the row functions
(tests/helpers/tonefilt_host.py: lld_tonefilt_ops.hpp with the C library's sin / cos, lld_chroma_ops.hpp) on every input and asserts
that its two levels equal the binary's bit for bit.

Of the 60 s input at 8 kHz (large arguments) every 50th row and the last 20 are kept.

Run from the repo root where the reference is built:
    python tests/golden/make_golden_chroma_filt.py
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
from helpers import chroma_host, hard_signals, tonefilt_host  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
CONF_REL = os.path.join("chroma", "chroma_filt.conf")

# (synth.utterance index, samples, rate, divisor): 0, P - 1, P, P + 1, 2P - 1, 2P samples at 16 kHz (P = 160: the row rule, which
# main() asserts as measured: ceil(n / P) rows, the last block padded with the last sample); 1 s at 16 kHz divided so that whole rows
# fall under silThresh; one input of about 0.2 s per other rate, 20 P + 19 samples (0.01 s is no whole number of samples at 11.025,
# 22.05 and 44.1 kHz); 60 s at 8 kHz
INPUTS = [(2, 0, 16000, 1), (3, 159, 16000, 1), (4, 160, 16000, 1), (5, 161, 16000, 1), (6, 319, 16000, 1), (7, 320, 16000, 1),
          (2, 16000, 16000, 16), (4, 1619, 8000, 1), (5, 2219, 11025, 1), (6, 4439, 22050, 1), (7, 6419, 32000, 1),
          (8, 8839, 44100, 1), (9, 9619, 48000, 1), (3, 480000, 8000, 1)]
SIL = 6                                                    # the 1 s input
LONG = 13                                                  # the 60 s input
LONG_KEEP = 50
ROW_RULE = (0, 1, 2, 3, 4, 5)

TAP = """
[componentInstances:cComponentManager]
instance[tap_ts].type=cHtkSink
instance[tap_chroma].type=cHtkSink
[tap_ts:cHtkSink]
reader.dmLevel=tonespec
filename=tap_ts.htk
[tap_chroma:cHtkSink]
reader.dmLevel=chroma
filename=tap_chroma.htk
"""
TAPS = (("tonespec", "tap_ts.htk"), ("chroma", "tap_chroma.htk"))

# edited copies: (key suffix, {text of the shipped file: replacement}, the options the row functions take)
EDITS = [("n48", {"nNotes = 72": "nNotes = 48", "firstNote = 55": "firstNote = 110", "decayF0 = 0.999900": "decayF0 = 0.9995",
                  "decayFN = 0.999000": "decayFN = 0.998"}, dict(n_notes=48, first_note=110.0, decay_f0=0.9995, decay_fn=0.998)),
         ("op25", {"outputPeriod = 0.0100": "outputPeriod = 0.025"}, dict(output_period=0.025)),
         ("os24", {"octaveSize = 12": "octaveSize = 24"}, dict(octave_size=24)),
         ("sil0", {"octaveSize = 12": "octaveSize = 12\nsilThresh = 0"}, dict(sil_thresh=0.0))]
EDIT_INPUTS = (5, 6)                                       # 2P samples and 1 s


def cut(idx, n, div=1):
    """the samples of an input: synth.utterance(idx, n), floor-divided by div"""
    if not n:
        return np.zeros(0, np.int16)
    return (synth.utterance(idx, n).astype(np.int32) // div).astype(np.int16)


def kept_rows(k, n_rows):
    """the rows of input k the fixture holds"""
    if k != LONG:
        return np.arange(n_rows)
    return np.unique(np.concatenate([np.arange(0, n_rows, LONG_KEEP), np.arange(max(n_rows - 20, 0), n_rows)]))


def edited_text(edits=None, header=False):
    text = open(os.path.join(lldo.REF_DIR, "config", CONF_REL), encoding="latin-1").read()
    for a, b in (edits or {}).items():
        assert text.count(a) == 1, a
        text = text.replace(a, b)
    if header:
        for a in ("printHeader = 0", "timestamp = 0"):
            assert text.count(a) == 1
            text = text.replace(a, a[:-1] + "1")
    return text


def tapped_conf(td, edits=None, header=False, tap=True):
    path = os.path.join(td, "chroma_filt_tap.conf")
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
    """{csv, tonespec, chroma} of one input: the (edited) file as it is, then its tapped copy"""
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


def host_levels(pcm, fs, opts=None):
    """the g++ build of the row functions: (tonespec, chroma, s, c, D)"""
    o = dict(opts or {})
    octave_size, sil = o.pop("octave_size", 12), o.pop("sil_thresh", 0.001)
    ts, s, c = tonefilt_host.tonespec_rows(tonefilt_host.padded(pcm, fs, o), fs, o)
    ch = chroma_host.chroma_rows(ts, octave_size, sil) if len(ts) else np.zeros((0, octave_size), np.float32)
    _, s1, c1 = tonefilt_host.tonespec_rows(tonefilt_host.padded(pcm, fs, o), fs, o, mode=1, seed=0x5EED + len(pcm))
    a, b = np.concatenate([s, c]), np.concatenate([s1, c1])
    nz = a != 0
    D = float(np.max(np.abs(b[nz] - a[nz]) / np.abs(a[nz]))) if nz.any() else 0.0
    assert (b[~nz] == 0).all()
    return ts, ch, s, c, D


def store(d, suffix, k, r, pcm, fs, opts=None):
    ts = r["tonespec"] if r["tonespec"] is not None else np.zeros((0, 0), np.float32)
    ch = r["chroma"] if r["chroma"] is not None else np.zeros((0, 0), np.float32)
    hts, hch, s, c, D = host_levels(pcm, fs, opts)
    assert len(hts) == len(ts), ("rows", suffix, len(hts), len(ts))
    if len(ts):
        assert hts.shape == ts.shape and hch.shape == ch.shape, (suffix, hts.shape, ts.shape, hch.shape, ch.shape)
        assert (hts.view(np.uint32) == ts.view(np.uint32)).all(), ("the host row functions differ from the binary's tonespec level", suffix,
                                                                   int((hts.view(np.uint32) != ts.view(np.uint32)).sum()))
        assert (hch.view(np.uint32) == ch.view(np.uint32)).all(), ("the host row functions differ from the binary's chroma level", suffix)
    keep = kept_rows(k, len(ts))
    d["n_rows_" + suffix] = np.int64(len(ts))
    d["tonespec_" + suffix] = ts[keep] if len(ts) else ts
    d["chroma_" + suffix] = ch[keep] if len(ch) else ch
    d["csv_" + suffix] = np.array("".join(np.array(r["csv"].splitlines(True), dtype=object)[keep]) if len(ts) else r["csv"])
    d["state_s_" + suffix], d["state_c_" + suffix], d["D_" + suffix] = s, c, np.float64(D)
    return ts, ch, D


def main():
    lldo.build()
    assert lldo.have_ref(), "oracle/_ref/SMILExtract missing (the reference is not built)"
    d = {"inputs": np.array(INPUTS, np.int64), "long_keep": np.int64(LONG_KEEP)}
    for k, (idx, n, fs, div) in enumerate(INPUTS):
        pcm = cut(idx, n, div)
        r = reference(pcm, fs)
        ts, ch, D = store(d, str(k), k, r, pcm, fs)
        P = tonefilt_host.block_len(fs)
        print("input", (idx, n, fs, div), "P", P, "rows", len(ch), "= ceil(n / P)", -(-n // P), "tonespec", ts.shape, "chroma", ch.shape, "D %.3g" % D, "rc", r["rc"])
        assert len(ch) == -(-n // P), "the row rule"
        if k == SIL:                                       # what the chroma level holds: a level of zeros would pass any test
            assert ts.shape[1] == 72 and ch.shape[1] == 12
            nz = (ch != 0).any(axis=1)
            s = ch.astype(np.float64).sum(axis=1)
            print("   non-zero rows", int(nz.sum()), "of", len(ch))
            assert (~nz).sum() > 0 and nz.sum() > 0 and (np.abs(s[nz] - 1.0) < 1e-5).all(), "the chroma level needs all-zero rows and rows that sum to 1"
            assert 4 * int(nz.sum()) >= len(ch), "fewer than a quarter of the rows are non-zero: scale the cut"
    for tag, edits, opts in EDITS:
        for k in EDIT_INPUTS:
            idx, n, fs, div = INPUTS[k]
            pcm = cut(idx, n, div)
            r = reference(pcm, fs, edits)
            ts, ch, D = store(d, "%s_%d" % (tag, k), k, r, pcm, fs, opts)
            print(tag, "input", (idx, n, fs, div), "tonespec", ts.shape, "chroma", ch.shape, "differs from the shipped file's:",
                  r["csv"] != str(d["csv_%d" % k]), "non-zero rows", int((ch != 0).any(axis=1).sum()) if len(ch) else 0, "D %.3g" % D)
    with tmpdir() as td:                                   # names and row times: a copy that prints header and time stamps
        idx, n, fs, div = INPUTS[6]
        r = run(cut(idx, n, div)[:1700], fs, tapped_conf(td, None, header=True, tap=False), td, "h")
    d["csv_header_copy"] = np.array(r["csv"])
    print("header copy:", r["csv"].splitlines()[0], "|", [line.split(";")[0] for line in r["csv"].splitlines()[1:4]])
    # what the binary does where nNotes is no multiple of octaveSize
    with tmpdir() as td:
        idx, n, fs, div = INPUTS[5]
        r = run(cut(idx, n, div), fs, tapped_conf(td, {"nNotes = 72": "nNotes = 70"}), td, "m")
    d["n70_rc"], d["n70_csv"] = np.int64(r["rc"]), np.array(r["csv"])
    print("nNotes = 70, octaveSize = 12: rc", r["rc"], "csv", repr(r["csv"][:200]), "tonespec", None if r["tonespec"] is None else r["tonespec"].shape,
          "chroma", None if r["chroma"] is None else (r["chroma"].shape, r["chroma"][:2]))
    np.savez_compressed(os.path.join(OUT, "chroma_filt_synth.npz"), **d)
    h = {}
    for name, pcm in hard_signals.signals().items():
        r = reference(pcm)
        hts, hch, s, c, D = host_levels(pcm, 16000)
        assert (hts.view(np.uint32) == r["tonespec"].view(np.uint32)).all() and (hch.view(np.uint32) == r["chroma"].view(np.uint32)).all(), name
        h["tonespec_" + name], h["chroma_" + name] = r["tonespec"], r["chroma"]
        print(name, r["chroma"].shape, "non-zero rows", int((r["chroma"] != 0).any(axis=1).sum()), "D %.3g" % D)
    np.savez_compressed(os.path.join(OUT, "hard_chroma_filt.npz"), **h)
    conf = os.path.join(lldo.REF_DIR, "config", CONF_REL)
    with tempfile.TemporaryDirectory() as td:
        for stem in ("u2_8000", "u3_4000"):
            exe = os.path.join(lldo.REF_DIR, "SMILExtract")
            subprocess.run([exe, "-C", conf, "-I", os.path.join(OUT, "files", stem + ".wav"), "-O", os.path.join(td, "o.csv"), "-l", "0"],
                           check=True, cwd=td)
            shutil.copy(os.path.join(td, "o.csv"), os.path.join(OUT, "files", "chroma_filt_%s.csv" % stem))
    for f in ("chroma_filt_synth.npz", "hard_chroma_filt.npz", "files/chroma_filt_u2_8000.csv", "files/chroma_filt_u3_4000.csv"):
        print(f, os.path.getsize(os.path.join(OUT, f)), "bytes")


if __name__ == "__main__":
    main()
