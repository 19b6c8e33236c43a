#!/usr/bin/env python3
"""Generate the prosodyShs fixtures under tests/golden/ by running the REAL reference binary (oracle/_ref/SMILExtract, built by
oracle/Makefile) on config/prosody/prosodyShs.conf:

    prosody_shs_synth.npz   per input: where its samples come from (synth.utterance index, length, rate), the 3-column lld level
                            as the HTK sink wrote it, the frame times of the CSV sink and the cPitchShs rows (level pitchShs:
                            nCandidates | F0Cand[4] | candVoicing[4] | candScore[4] | F0raw | voicingClip); the CSV header
    hard_prosody_shs.npz    the same three columns for the hard-signal corpus (tests/helpers/hard_signals.py)
    files/prosody_shs_*.{htk,csv}   the binary's output files for files/u2_8000.wav and files/u3_4000.wav

The binary runs twice per input: on the shipped file (what the level fixtures hold), and on a copy of it written into a temporary
directory with one HTK sink on the pitchShs level appended (the candidate rows; its lld level must equal the first run's).

Run from the repo root where the reference is built:
    python tests/golden/make_golden_prosody_shs.py
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
CONF_REL = os.path.join("prosody", "prosodyShs.conf")

# (synth.utterance index, samples, rate): 0 .. 4 and 9 frames (one past the frame kernels' 8-frame tile), 1 s and 3 s; other rates
INPUTS = [(2, 0, 16000), (3, 100, 16000), (4, 799, 16000), (5, 800, 16000), (6, 960, 16000), (7, 1120, 16000), (8, 1280, 16000),
          (9, 2080, 16000), (2, 16000, 16000), (3, 48000, 16000), (4, 4000, 8000), (5, 22050, 44100), (6, 24000, 48000)]

TAP = """
[componentInstances:cComponentManager]
instance[tap_shs].type=cHtkSink
[tap_shs:cHtkSink]
reader.dmLevel=pitchShs
filename=tap_shs.htk
"""


# the other parameters of the chain, edited in a copy of the file: (key suffix, {text of the shipped file: replacement})
EDITS = [("maxpitch400", {"maxPitch = 620": "maxPitch = 400"}),
         ("all", {"maxPitch = 620": "maxPitch = 400", "minPitch = 52": "minPitch = 60", "nCandidates = 4": "nCandidates = 6", "minF = 25": "minF = 20",
                  "voicingCutoff = 0.700000": "voicingCutoff = 0.600000", "nHarmonics = 15": "nHarmonics = 12",
                  "compressionFactor = 0.850000": "compressionFactor = 0.800000"})]


def tapped_conf(td, sma_win=3, edits=None):
    """The shipped file with its includes made absolute and the tap appended (and smaWin / other options edited), written into td."""
    cdir = os.path.join(lldo.REF_DIR, "config")
    text = open(os.path.join(cdir, CONF_REL)).read().replace("\\{../shared/", "\\{" + os.path.join(cdir, "shared") + "/")
    assert text.count("smaWin = 3") == 1
    text = text.replace("smaWin = 3", "smaWin = %d" % sma_win)
    for a, b in (edits or {}).items():
        assert text.count(a) == 1, a
        text = text.replace(a, b)
    path = os.path.join(td, "prosodyShs_tap.conf")
    with open(path, "w") as f:
        f.write(text + TAP)
    return path


def run(pcm, fs, conf, td, tag):
    exe = os.path.join(lldo.REF_DIR, "SMILExtract")
    wav, htk, csv = (os.path.join(td, tag + e) for e in (".wav", ".htk", ".csv"))
    lldo.write_wav(wav, pcm, fs)
    for p in (htk, csv, os.path.join(td, "tap_shs.htk")):
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
    tap = os.path.join(td, "tap_shs.htk")
    shs = lldo.read_htk(tap)[0] if os.path.exists(tap) and os.path.getsize(tap) > 12 else np.zeros((0, 15), np.float32)
    return dict(lld=lld.reshape(-1, 3), times=times, header=header, shs=shs, rc=r.returncode, htk=htk, csv=csv)


def reference(pcm, fs=16000):
    """{lld, times, header, shs} of one input (also what a pin test compares a fresh run with)."""
    conf = os.path.join(lldo.REF_DIR, "config", CONF_REL)
    with tempfile.TemporaryDirectory(dir="/dev/shm" if os.path.isdir("/dev/shm") else None) as td:
        a = run(pcm, fs, conf, td, "a")
        b = run(pcm, fs, tapped_conf(td), td, "b")
        assert a["lld"].tobytes() == b["lld"].tobytes(), "the tapped copy changed the lld level"
        assert len(a["times"]) == len(a["lld"])
        a["shs"] = b["shs"]
        return a


def main():
    lldo.build()
    assert lldo.have_ref(), "oracle/_ref/SMILExtract missing (the reference is not built)"
    d = {"inputs": np.array(INPUTS, np.int64)}
    header = None
    for k, (idx, n, fs) in enumerate(INPUTS):
        r = reference(synth.utterance(idx, n) if n else np.zeros(0, np.int16), fs)
        d["lld_%d" % k], d["times_%d" % k], d["shs_%d" % k] = r["lld"], r["times"], r["shs"]
        f0 = r["lld"][:, 0] if len(r["lld"]) else np.zeros(0)
        print("input", (idx, n, fs), "rows", len(r["lld"]), "shs rows", r["shs"].shape, "voiced rows", int((f0 > 0).sum()), "rc", r["rc"])
        if n >= fs:                                        # both branches of F0final in every file of a second or more
            assert (f0 > 0).sum() * 4 >= len(f0) and (f0 == 0).any(), "choose another synth index for %r" % ((idx, n, fs),)
        if r["header"]:
            assert header in (None, r["header"])
            header = r["header"]
    d["csv_header"] = np.array(header)
    # the smoother's edge rules with wider windows, on the short inputs where they show: an edited copy (smaWin = 5, 7, 9)
    for sw in (5, 7, 9):
        for k in (4, 5, 6, 7, 8):
            idx, n, fs = INPUTS[k]
            with tempfile.TemporaryDirectory(dir="/dev/shm" if os.path.isdir("/dev/shm") else None) as td:
                r = run(synth.utterance(idx, n), fs, tapped_conf(td, sw), td, "w")
            assert r["shs"].tobytes() == d["shs_%d" % k].tobytes()
            d["lld_w%d_%d" % (sw, k)] = r["lld"]
            print("smaWin", sw, "input", (idx, n, fs), "rows", len(r["lld"]))
    # the chain's other parameters: edited copies on the 9-frame and the 1 s input, with their own cPitchShs rows
    for tag, edits in EDITS:
        for k in (7, 8):
            idx, n, fs = INPUTS[k]
            with tempfile.TemporaryDirectory(dir="/dev/shm" if os.path.isdir("/dev/shm") else None) as td:
                r = run(synth.utterance(idx, n), fs, tapped_conf(td, 3, edits), td, "e")
            d["lld_%s_%d" % (tag, k)], d["shs_%s_%d" % (tag, k)] = r["lld"], r["shs"]
            print(tag, "input", (idx, n, fs), "rows", len(r["lld"]), "shs", r["shs"].shape, "differs from the shipped file's:",
                  r["lld"].tobytes() != d["lld_%d" % k].tobytes())
    np.savez_compressed(os.path.join(OUT, "prosody_shs_synth.npz"), **d)
    h = {}
    for name, pcm in hard_signals.signals().items():
        r = reference(pcm)
        h["lld_" + name] = r["lld"]
        print(name, r["lld"].shape, "voiced rows", int((r["lld"][:, 0] > 0).sum()))
    np.savez_compressed(os.path.join(OUT, "hard_prosody_shs.npz"), **h)
    conf = os.path.join(lldo.REF_DIR, "config", CONF_REL)
    with tempfile.TemporaryDirectory() as td:
        for stem in ("u2_8000", "u3_4000"):
            exe = os.path.join(lldo.REF_DIR, "SMILExtract")
            subprocess.run([exe, "-C", conf, "-I", os.path.join(OUT, "files", stem + ".wav"), "-O", os.path.join(td, "o.htk"),
                            "-csvoutput", os.path.join(td, "o.csv"), "-instname", stem, "-l", "0"], check=True, cwd=td)
            for e in ("htk", "csv"):
                shutil.copy(os.path.join(td, "o." + e), os.path.join(OUT, "files", "prosody_shs_%s.%s" % (stem, e)))
    for f in ("prosody_shs_synth.npz", "hard_prosody_shs.npz", "files/prosody_shs_u2_8000.htk", "files/prosody_shs_u2_8000.csv",
              "files/prosody_shs_u3_4000.htk", "files/prosody_shs_u3_4000.csv"):
        print(f, os.path.getsize(os.path.join(OUT, f)), "bytes")


if __name__ == "__main__":
    main()
