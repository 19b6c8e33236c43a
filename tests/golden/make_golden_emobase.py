#!/usr/bin/env python3
"""Generate the emobase fixtures under tests/golden/ by running the REAL reference binary (oracle/_ref/SMILExtract, built by
oracle/Makefile) on config/emobase/emobase.conf, LLD level only (the sinks lldsink / lldhtksink on `lld;lld_de`):

    emobase_synth.npz   per input: where its samples come from (synth.utterance index, length, rate), the 52-column `lld;lld_de`
                        as the HTK sink wrote it, the frame times of the CSV sink, the tapped levels intens (2) | mfcc1 (12) |
                        lsp (p) | mzcr (1) | pitch (3), lpc (p, cLsp's input) and the F0raw column of a second cPitchACF instance (the
                        contour's input); the CSV header
    hard_emobase.npz    the 52 columns for the hard-signal corpus (tests/helpers/hard_signals.py)
    files/emobase_*.{htk,csv}   the binary's LLD output files for files/u2_8000.wav and files/u3_4000.wav

The binary runs twice per input: on the shipped file (what the level fixtures hold), and on a copy of it written into a temporary
directory with the sections of TAP appended (sinks on the levels in front of the smoother; the copy's lld must equal the first run's).

Run from the repo root where the reference is built:
    python tests/golden/make_golden_emobase.py
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
CONF_REL = os.path.join("emobase", "emobase.conf")

# (synth.utterance index, samples, rate). 16 kHz: (T25, T40) = (0,0) (0,0) (0,0) (1,0) (2,0) (2,0) (2,1) (3,1) (3,2) (4,2), then
# 2080 samples, 1 s and 3 s; then one input of about 0.3 s per other rate (the 25 / 40 ms transforms have 256 / 512 points at 8 kHz,
# 512 / 512 at 11.025, 1024 / 1024 at 22.05, 1024 / 2048 at 32, 2048 / 2048 at 44.1, 2048 / 2048 at 48 kHz)
INPUTS = [(2, 0, 16000), (3, 100, 16000), (4, 399, 16000), (5, 400, 16000), (6, 560, 16000), (7, 639, 16000), (8, 640, 16000),
          (9, 720, 16000), (2, 800, 16000), (3, 880, 16000), (9, 2080, 16000), (2, 16000, 16000), (3, 48000, 16000),
          (4, 2400, 8000), (5, 3308, 11025), (6, 6615, 22050), (7, 9600, 32000), (8, 13230, 44100), (9, 14400, 48000)]
N16 = 13                                                   # the first N16 inputs are the 16 kHz ones
SHORT = (3, 4, 5, 6, 7, 8, 9, 10)                          # the inputs the wider smoothing windows are recorded on

TAPS = (("intens", 2), ("mfcc1", 12), ("lsp", None), ("mzcr", 1), ("pitch", 3), ("lpc", None), ("f0raw", 1))   # None: cLpc's order


def tap_text(max_pitch="500"):
    """sinks on the levels in front of the smoother and on cLpc's, and a second cPitchACF with F0raw = 1 on a level of its own (the
    contour's input)"""
    s = "\n[componentInstances:cComponentManager]\ninstance[pitchraw].type=cPitchACF\n"
    for lv, _ in TAPS:
        s += "instance[tap_%s].type=cHtkSink\n" % lv
    s += ("[pitchraw:cPitchACF]\nreader.dmLevel=acf40;cepstrum40\nwriter.dmLevel=f0raw\nprocessArrayFields=0\nmaxPitch=%s\n"
          "voiceProb=0\nF0=0\nF0raw=1\n" % max_pitch)
    for lv, _ in TAPS:
        s += "[tap_%s:cHtkSink]\nreader.dmLevel=%s\nfilename=tap_%s.htk\n" % (lv, lv, lv)
    return s


# the chain's parameters, edited in a copy of the file: (key suffix, cLpc's order, {text of the shipped file: replacement})
EDITS = [("mp300", 8, {"maxPitch = 500": "maxPitch = 300", "voicingCutoff = 0.550000": "voicingCutoff = 0.700000"}),
         ("p10", 10, {"\np = 8\n": "\np = 10\n"})]


def tapped_conf(td, sma_win=3, edits=None, max_pitch="500"):
    """The shipped file with its include made absolute and the tap appended (and smaWin / other options edited), written into td."""
    cdir = os.path.join(lldo.REF_DIR, "config")
    text = open(os.path.join(cdir, CONF_REL), encoding="latin-1").read().replace("\\{../shared/", "\\{" + os.path.join(cdir, "shared") + "/")
    assert text.count("smaWin = 3") == 1
    text = text.replace("smaWin = 3", "smaWin = %d" % sma_win)
    for a, b in (edits or {}).items():
        assert text.count(a) == 1, a
        text = text.replace(a, b)
    path = os.path.join(td, "emobase_tap.conf")
    with open(path, "w", encoding="latin-1") as f:
        f.write(text + tap_text(max_pitch))
    return path


def run(pcm, fs, conf, td, tag, p=8):
    exe = os.path.join(lldo.REF_DIR, "SMILExtract")
    wav, htk, csv = (os.path.join(td, tag + e) for e in (".wav", ".htk", ".csv"))
    lldo.write_wav(wav, pcm, fs)
    for f in [htk, csv] + [os.path.join(td, "tap_%s.htk" % t[0]) for t in TAPS]:
        if os.path.exists(f):
            os.remove(f)
    r = subprocess.run([exe, "-C", conf, "-I", wav, "-lldhtkoutput", htk, "-lldcsvoutput", csv, "-instname", tag, "-l", "0"], cwd=td,
                       stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    ncol = 2 * (18 + p)
    lld = lldo.read_htk(htk)[0] if os.path.exists(htk) and os.path.getsize(htk) > 12 else np.zeros((0, ncol), np.float32)
    times, header = np.zeros(0), ""
    if os.path.exists(csv):
        lines = open(csv).read().splitlines()
        header = lines[0] if lines else ""
        times = np.array([float(ln.split(";")[1]) for ln in lines[1:]], np.float64)
    out = dict(lld=lld.reshape(-1, ncol), times=times, header=header, rc=r.returncode, htk=htk, csv=csv)
    for lv, nc in TAPS:
        nc = nc or p
        f = os.path.join(td, "tap_%s.htk" % lv)
        out[lv] = (lldo.read_htk(f)[0] if os.path.exists(f) and os.path.getsize(f) > 12 else np.zeros((0, nc), np.float32)).reshape(-1, nc)
    return out


def reference(pcm, fs=16000):
    """{lld, times, header, intens, mfcc1, lsp, mzcr, pitch, lpc} of one input"""
    conf = os.path.join(lldo.REF_DIR, "config", CONF_REL)
    with tempfile.TemporaryDirectory(dir="/dev/shm" if os.path.isdir("/dev/shm") else None) as td:
        a = run(pcm, fs, conf, td, "a")
        b = run(pcm, fs, tapped_conf(td), td, "b")
        assert a["lld"].tobytes() == b["lld"].tobytes(), "the tapped copy changed the lld level"
        assert len(a["times"]) == len(a["lld"])
        for lv, _ in TAPS:
            a[lv] = b[lv]
        return a


def main():
    lldo.build()
    assert lldo.have_ref(), "oracle/_ref/SMILExtract missing (the reference is not built)"
    d = {"inputs": np.array(INPUTS, np.int64)}
    header = None
    for k, (idx, n, fs) in enumerate(INPUTS):
        r = reference(synth.utterance(idx, n) if n else np.zeros(0, np.int16), fs)
        d["lld_%d" % k], d["times_%d" % k] = r["lld"], r["times"]
        for lv, _ in TAPS:
            d["%s_%d" % (lv, k)] = r[lv]
        f0 = r["lld"][:, 24] if len(r["lld"]) else np.zeros(0)
        print("input", (idx, n, fs), "rows", len(r["lld"]), "T25", len(r["intens"]), "T40", len(r["pitch"]), "voiced rows", int((f0 > 0).sum()),
              "rc", r["rc"], "times", r["times"][:3], r["times"][-3:])
        if n >= fs:                                        # both branches of F0 in every file of a second or more
            assert (f0 > 0).any() and (f0 == 0).any(), "choose another synth index for %r" % ((idx, n, fs),)
        if r["header"]:
            assert header in (None, r["header"])
            header = r["header"]
    d["csv_header"] = np.array(header)
    # the smoother's edge rules with wider windows, on the short inputs where they show: an edited copy (smaWin = 5, 7, 9)
    for sw in (5, 7, 9):
        for k in SHORT:
            idx, n, fs = INPUTS[k]
            with tempfile.TemporaryDirectory(dir="/dev/shm" if os.path.isdir("/dev/shm") else None) as td:
                r = run(synth.utterance(idx, n), fs, tapped_conf(td, sw), td, "w")
            assert all(r[lv].tobytes() == d["%s_%d" % (lv, k)].tobytes() for lv, _ in TAPS)
            d["lld_w%d_%d" % (sw, k)], d["times_w%d_%d" % (sw, k)] = r["lld"], r["times"]
            print("smaWin", sw, "input", (idx, n, fs), "rows", len(r["lld"]), "times", r["times"])
    # the chain's other parameters: edited copies on the 2080-sample and the 1 s input, with their own tapped levels
    for tag, p, edits in EDITS:
        for k in (10, 11):
            idx, n, fs = INPUTS[k]
            with tempfile.TemporaryDirectory(dir="/dev/shm" if os.path.isdir("/dev/shm") else None) as td:
                r = run(synth.utterance(idx, n), fs, tapped_conf(td, 3, edits, "300" if tag == "mp300" else "500"), td, "e", p)
            d["lld_%s_%d" % (tag, k)] = r["lld"]
            for lv, _ in TAPS:
                d["%s_%s_%d" % (lv, tag, k)] = r[lv]
            print(tag, "input", (idx, n, fs), "rows", r["lld"].shape)
    np.savez_compressed(os.path.join(OUT, "emobase_synth.npz"), **d)
    h = {}
    for name, pcm in hard_signals.signals().items():
        r = reference(pcm)
        h["lld_" + name] = r["lld"]
        print(name, r["lld"].shape, "voiced rows", int((r["lld"][:, 24] > 0).sum()))
    np.savez_compressed(os.path.join(OUT, "hard_emobase.npz"), **h)
    conf = os.path.join(lldo.REF_DIR, "config", CONF_REL)
    with tempfile.TemporaryDirectory() as td:
        for stem in ("u2_8000", "u3_4000"):
            exe = os.path.join(lldo.REF_DIR, "SMILExtract")
            subprocess.run([exe, "-C", conf, "-I", os.path.join(OUT, "files", stem + ".wav"), "-lldhtkoutput", os.path.join(td, "o.htk"),
                            "-lldcsvoutput", os.path.join(td, "o.csv"), "-instname", stem, "-l", "0"], check=True, cwd=td)
            for e in ("htk", "csv"):
                shutil.copy(os.path.join(td, "o." + e), os.path.join(OUT, "files", "emobase_%s.%s" % (stem, e)))
    for f in ("emobase_synth.npz", "hard_emobase.npz", "files/emobase_u2_8000.htk", "files/emobase_u2_8000.csv",
              "files/emobase_u3_4000.htk", "files/emobase_u3_4000.csv"):
        print(f, os.path.getsize(os.path.join(OUT, f)), "bytes")


if __name__ == "__main__":
    main()
