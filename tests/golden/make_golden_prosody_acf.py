#!/usr/bin/env python3
"""Generate the prosodyAcf fixtures under tests/golden/ by running the REAL reference binary (oracle/_ref/SMILExtract, built by
oracle/Makefile) on config/prosody/prosodyAcf.conf:

    prosody_acf_synth.npz   per input: where its samples come from (synth.utterance index, length, rate), the 3-column lld level
                            as the HTK sink wrote it, the frame times of the CSV sink, the tapped levels `pitch` (voiceProb | F0)
                            and `intens` (pcm_loudness) and the F0raw column of a second cPitchACF instance; the CSV header
    hard_prosody_acf.npz    the three lld columns for the hard-signal corpus (tests/helpers/hard_signals.py)
    files/prosody_acf_*.{htk,csv}   the binary's output files for files/u2_8000.wav and files/u3_4000.wav

The binary runs twice per input: on the shipped file (what the level fixtures hold), and on a copy of it written into a temporary
directory with the sections of TAP appended (sinks on the levels pitch and intens, and a second cPitchACF with F0raw = 1 on a level
of its own: the contour's input; the copy's lld level must equal the first run's).

Run from the repo root where the reference is built:
    python tests/golden/make_golden_prosody_acf.py
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
CONF_REL = os.path.join("prosody", "prosodyAcf.conf")

# (synth.utterance index, samples, rate): 0 .. 4 and 9 frames at 16 kHz (the row rule), 1 s and 3 s; then one input per other rate
# (Nfft 512: 8 / 11.025 kHz, 2048: 22.05 / 32 kHz, 4096: 44.1 / 48 kHz; 50 ms is no whole number of samples at 11.025 / 22.05 / 44.1 kHz)
INPUTS = [(2, 0, 16000), (3, 100, 16000), (4, 799, 16000), (5, 800, 16000), (6, 960, 16000), (7, 1120, 16000), (8, 1280, 16000),
          (9, 2080, 16000), (2, 16000, 16000), (3, 48000, 16000), (4, 4000, 8000), (5, 4410, 11025), (6, 8820, 22050),
          (7, 12800, 32000), (8, 13230, 44100), (9, 14400, 48000)]
N16 = 10                                                   # the first N16 inputs are the 16 kHz ones

TAP = """
[componentInstances:cComponentManager]
instance[tap_pitch].type=cHtkSink
instance[tap_int].type=cHtkSink
instance[pitchraw].type=cPitchACF
instance[tap_raw].type=cHtkSink
[tap_pitch:cHtkSink]
reader.dmLevel=pitch
filename=tap_pitch.htk
[tap_int:cHtkSink]
reader.dmLevel=intens
filename=tap_int.htk
[pitchraw:cPitchACF]
reader.dmLevel=acf;cepstrum
writer.dmLevel=pitchraw
processArrayFields=0
maxPitch=%s
voiceProb=0
F0=0
F0raw=1
[tap_raw:cHtkSink]
reader.dmLevel=pitchraw
filename=tap_raw.htk
"""

# the chain's parameters, edited in a copy of the file: (key suffix, maxPitch of the tap's own instance, {text of the shipped file: replacement})
EDITS = [("mp300", "300", {"maxPitch = 500": "maxPitch = 300", "voicingCutoff = 0.550000": "voicingCutoff = 0.700000"}),
         ("vc15", "500", {"voicingCutoff = 0.550000": "voicingCutoff = 1.500000"})]
TAPS = (("pitch", "tap_pitch.htk", 2), ("intens", "tap_int.htk", 1), ("f0raw", "tap_raw.htk", 1))


def tapped_conf(td, sma_win=3, edits=None, max_pitch="500"):
    """The shipped file with its includes made absolute and the tap appended (and smaWin / other options edited), written into td."""
    cdir = os.path.join(lldo.REF_DIR, "config")
    text = open(os.path.join(cdir, CONF_REL)).read().replace("\\{../shared/", "\\{" + os.path.join(cdir, "shared") + "/")
    assert text.count("smaWin = 3") == 1
    text = text.replace("smaWin = 3", "smaWin = %d" % sma_win)
    for a, b in (edits or {}).items():
        assert text.count(a) == 1, a
        text = text.replace(a, b)
    path = os.path.join(td, "prosodyAcf_tap.conf")
    with open(path, "w") as f:
        f.write(text + TAP % max_pitch)
    return path


def run(pcm, fs, conf, td, tag):
    exe = os.path.join(lldo.REF_DIR, "SMILExtract")
    wav, htk, csv = (os.path.join(td, tag + e) for e in (".wav", ".htk", ".csv"))
    lldo.write_wav(wav, pcm, fs)
    for p in [htk, csv] + [os.path.join(td, t[1]) for t in TAPS]:
        if os.path.exists(p):
            os.remove(p)
    r = subprocess.run([exe, "-C", conf, "-I", wav, "-O", htk, "-csvoutput", csv, "-instname", tag, "-l", "0"], cwd=td,
                       stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    lld = lldo.read_htk(htk)[0] if os.path.exists(htk) and os.path.getsize(htk) > 12 else np.zeros((0, 3), np.float32)
    times, header = np.zeros(0), ""
    if os.path.exists(csv):
        lines = open(csv).read().splitlines()
        header = lines[0] if lines else ""
        times = np.array([float(ln.split(";")[1]) for ln in lines[1:]], np.float64)
    out = dict(lld=lld.reshape(-1, 3), times=times, header=header, rc=r.returncode, htk=htk, csv=csv)
    for key, name, ncol in TAPS:
        p = os.path.join(td, name)
        out[key] = (lldo.read_htk(p)[0] if os.path.exists(p) and os.path.getsize(p) > 12 else np.zeros((0, ncol), np.float32)).reshape(-1, ncol)
    return out


def reference(pcm, fs=16000):
    """{lld, times, header, pitch, intens, f0raw} of one input (also what a pin test compares a fresh run with)."""
    conf = os.path.join(lldo.REF_DIR, "config", CONF_REL)
    with tempfile.TemporaryDirectory(dir="/dev/shm" if os.path.isdir("/dev/shm") else None) as td:
        a = run(pcm, fs, conf, td, "a")
        b = run(pcm, fs, tapped_conf(td), td, "b")
        assert a["lld"].tobytes() == b["lld"].tobytes(), "the tapped copy changed the lld level"
        assert len(a["times"]) == len(a["lld"])
        for key, _, _ in TAPS:
            a[key] = b[key]
        return a


def contour_input(r, cutoff=0.55):
    """the cut-off pitch candidate per frame (what the contour smooths), from the tapped levels"""
    return np.where(r["pitch"][:, 0].astype(np.float64) < cutoff, np.float32(0), r["f0raw"][:, 0])


def main():
    lldo.build()
    assert lldo.have_ref(), "oracle/_ref/SMILExtract missing (the reference is not built)"
    d = {"inputs": np.array(INPUTS, np.int64)}
    header = None
    reonset = False
    for k, (idx, n, fs) in enumerate(INPUTS):
        r = reference(synth.utterance(idx, n) if n else np.zeros(0, np.int16), fs)
        d["lld_%d" % k], d["times_%d" % k] = r["lld"], r["times"]
        for key, _, _ in TAPS:
            d["%s_%d" % (key, k)] = r[key]
        f0 = r["lld"][:, 1] if len(r["lld"]) else np.zeros(0)
        p = contour_input(r)
        v = (p > 0).astype(np.int8)
        # a voiced run that starts after an unvoiced one which itself follows a voiced frame: the contour's onset branches with state
        re = bool(len(v) > 2 and any(v[i] and not v[i - 1] and v[:i - 1].any() for i in range(2, len(v))))
        print("input", (idx, n, fs), "rows", len(r["lld"]), "pitch", r["pitch"].shape, "intens", r["intens"].shape, "f0raw", r["f0raw"].shape,
              "voiced rows", int((f0 > 0).sum()), "re-onset", re, "rc", r["rc"], "times", r["times"][:3], r["times"][-2:])
        if n >= fs:                                        # both branches of F0 in every file of a second or more
            assert (f0 > 0).any() and (f0 == 0).any(), "choose another synth index for %r" % ((idx, n, fs),)
            reonset = reonset or re
        if r["header"]:
            assert header in (None, r["header"])
            header = r["header"]
    assert reonset, "no input of a second or more has a voiced run that starts after an unvoiced one: choose other synth indices"
    d["csv_header"] = np.array(header)
    # the smoother's edge rules with wider windows, on the short inputs where they show: an edited copy (smaWin = 5, 7, 9)
    for sw in (5, 7, 9):
        for k in (4, 5, 6, 7, 8):
            idx, n, fs = INPUTS[k]
            with tempfile.TemporaryDirectory(dir="/dev/shm" if os.path.isdir("/dev/shm") else None) as td:
                r = run(synth.utterance(idx, n), fs, tapped_conf(td, sw), td, "w")
            assert r["pitch"].tobytes() == d["pitch_%d" % k].tobytes() and r["intens"].tobytes() == d["intens_%d" % k].tobytes()
            d["lld_w%d_%d" % (sw, k)] = r["lld"]
            print("smaWin", sw, "input", (idx, n, fs), "rows", len(r["lld"]))
    # the chain's other parameters: edited copies on the 9-frame and the 1 s input, with their own tapped levels
    for tag, mp, edits in EDITS:
        for k in (7, 8):
            idx, n, fs = INPUTS[k]
            with tempfile.TemporaryDirectory(dir="/dev/shm" if os.path.isdir("/dev/shm") else None) as td:
                r = run(synth.utterance(idx, n), fs, tapped_conf(td, 3, edits, mp), td, "e")
            d["lld_%s_%d" % (tag, k)] = r["lld"]
            for key, _, _ in TAPS:
                d["%s_%s_%d" % (key, tag, k)] = r[key]
            print(tag, "input", (idx, n, fs), "rows", len(r["lld"]), "differs from the shipped file's:",
                  r["lld"].tobytes() != d["lld_%d" % k].tobytes())
    np.savez_compressed(os.path.join(OUT, "prosody_acf_synth.npz"), **d)
    h = {}
    for name, pcm in hard_signals.signals().items():
        r = reference(pcm)
        h["lld_" + name] = r["lld"]
        print(name, r["lld"].shape, "voiced rows", int((r["lld"][:, 1] > 0).sum()))
    np.savez_compressed(os.path.join(OUT, "hard_prosody_acf.npz"), **h)
    conf = os.path.join(lldo.REF_DIR, "config", CONF_REL)
    with tempfile.TemporaryDirectory() as td:
        for stem in ("u2_8000", "u3_4000"):
            exe = os.path.join(lldo.REF_DIR, "SMILExtract")
            subprocess.run([exe, "-C", conf, "-I", os.path.join(OUT, "files", stem + ".wav"), "-O", os.path.join(td, "o.htk"),
                            "-csvoutput", os.path.join(td, "o.csv"), "-instname", stem, "-l", "0"], check=True, cwd=td)
            for e in ("htk", "csv"):
                shutil.copy(os.path.join(td, "o." + e), os.path.join(OUT, "files", "prosody_acf_%s.%s" % (stem, e)))
    for f in ("prosody_acf_synth.npz", "hard_prosody_acf.npz", "files/prosody_acf_u2_8000.htk", "files/prosody_acf_u2_8000.csv",
              "files/prosody_acf_u3_4000.htk", "files/prosody_acf_u3_4000.csv"):
        print(f, os.path.getsize(os.path.join(OUT, f)), "bytes")


if __name__ == "__main__":
    main()
