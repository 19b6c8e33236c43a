#!/usr/bin/env python3
"""Generate the audspec fixtures under tests/golden/ by running the REAL reference binary (oracle/_ref/SMILExtract, built by
oracle/Makefile) on config/audspec/audspec.conf and audspec_compat.conf:

    audspec_synth.npz       per input: where its samples come from (synth.utterance index, length, rate, divisor), the level `lld`
                            (78 columns) as the file's own cHtkSink wrote it, for inputs of up to a second the tapped level `melspec`
                            (26 columns), for the short inputs `fftmag` as well (the tapped level `plp` is the lld level's first
                            block, bit for bit: checked here, not stored); the same for audspec_compat.conf and for edited copies of
                            audspec.conf; the header line of the file's CSV sink and the header words of its HTK file
    hard_audspec.npz        the lld level for the hard-signal corpus (tests/helpers/hard_signals.py)
    files/audspec_*.htk / .csv, files/audspec_compat_*.htk
                            the binary's output files for files/u2_8000.wav and files/u3_4000.wav

The file's HTK sink (-O) writes the lld level as big-endian floats: those are the bits. The other levels come from taps: the binary
runs twice per input, on the shipped file and on a copy written into a temporary directory (its include lines pointed at the
reference's config/shared) with cHtkSink instances on fftmag, melspec and plp appended. The copy's lld file must equal the shipped
run's byte for byte.

Run from the repo root where the reference is built:
    python tests/golden/make_golden_audspec.py
The fixtures are committed; the GPU box only reads them."""
import os
import shutil
import struct
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
CONF_REL = os.path.join("audspec", "audspec.conf")
COMPAT_REL = os.path.join("audspec", "audspec_compat.conf")

# (synth.utterance index, samples, rate, divisor); index -1: digital silence. At 16 kHz N = 400, H = 160:
#   0, N - 1, N, N + H - 1, N + H, N + 2H samples (the row rule; T = 0, 0, 1, 1, 2, 3), then T = 5, 16, 17 (lld_chain_short /
#   lld_chain_tiled), 20 (the edited copies' input), 128, 129, 257 (the window chain's tile), one second (T = 98), and 0.2 s of
#   digital silence (every band on cPlp's floor). Then one input of N + 2H samples per other rate.
F16 = lambda T: 400 + 160 * (T - 1)  # noqa: E731
INPUTS = [(2, 0, 16000, 1), (3, 399, 16000, 1), (4, 400, 16000, 1), (5, 559, 16000, 1), (6, 560, 16000, 1), (7, 720, 16000, 1),
          (8, F16(5), 16000, 1), (9, F16(16), 16000, 1), (2, F16(17), 16000, 1), (3, F16(20), 16000, 1), (4, F16(128), 16000, 1),
          (5, F16(129), 16000, 1), (6, F16(257), 16000, 1), (7, 16000, 16000, 1), (-1, 3200, 16000, 1), (8, F16(20), 16000, 8192),
          (4, 200 + 2 * 80, 8000, 1), (5, 276 + 2 * 110, 11025, 1), (6, 551 + 2 * 221, 22050, 1), (7, 800 + 2 * 320, 32000, 1),
          (8, 1103 + 2 * 441, 44100, 1), (9, 1200 + 2 * 480, 48000, 1)]
SHORT_MAX = 2200                                           # inputs of at most this many samples keep their fftmag level
TAP_MAX = 16000                                            # ... and of at most this many their melspec level
SILENCE, QUIET = 14, 15                                    # the floor inputs: zeros, and a cut divided by 8192 (samples of -1, 0 and 1)
COMPAT_INPUTS = (5, 6, 7, 8, 9, 13, 16, 17, 18, 19, 20, 21)   # the compat file: T = 3, 5, 16, 17, 20, one second, the other rates
EDIT_INPUTS = (6, 9)                                       # T = 5 (with fftmag) and T = 20

TAP = """
[componentInstances:cComponentManager]
instance[tap_mag].type=cHtkSink
instance[tap_mel].type=cHtkSink
instance[tap_plp].type=cHtkSink
[tap_mag:cHtkSink]
reader.dmLevel=fftmag
filename=tap_mag.htk
[tap_mel:cHtkSink]
reader.dmLevel=melspec
filename=tap_mel.htk
[tap_plp:cHtkSink]
reader.dmLevel=plp
filename=tap_plp.htk
"""
TAPS = (("fftmag", "tap_mag.htk"), ("melspec", "tap_mel.htk"), ("plp", "tap_plp.htk"))

# edited copies of audspec.conf: (key suffix, {text of the shipped file: (replacement, occurrences)})
EDITS = [("nb20", {"nBands = 26": ("nBands = 20", 1)}),
         ("nb40", {"nBands = 26": ("nBands = 40", 1)}),
         ("lohi", {"lofreq = 0": ("lofreq = 100", 1), "hifreq = 8000": ("hifreq = 4000", 1)}),
         ("comp05", {"compression = 0.33": ("compression = 0.5", 1)}),
         ("dw3", {"deltawin=2": ("deltawin=3", 2)}),
         ("d1", {"reader.dmLevel = plp;plpde;plpdede": ("reader.dmLevel = plp;plpde", 1)}),
         ("d0", {"reader.dmLevel = plp;plpde;plpdede": ("reader.dmLevel = plp", 1)}),
         ("fs32", {"frameSize = 0.0250": ("frameSize = 0.032", 1)}),
         ("han", {"winFunc = ham": ("winFunc = han", 1)}),
         ("inert", {"lpOrder = 5": ("lpOrder = 8", 1), "firstCC = 0": ("firstCC = 1", 1), "cepLifter = 22": ("cepLifter = 0", 1)})]


def cut(idx, n, div=1):
    """the samples of an input: synth.utterance(idx, n), floor-divided by div; idx -1: zeros"""
    if not n:
        return np.zeros(0, np.int16)
    if idx < 0:
        return np.zeros(n, np.int16)
    return (synth.utterance(idx, n).astype(np.int32) // div).astype(np.int16)


def edited_text(conf_rel=CONF_REL, edits=None):
    text = open(os.path.join(lldo.REF_DIR, "config", conf_rel), encoding="latin-1").read()
    shared = os.path.join(lldo.REF_DIR, "config", "shared") + os.sep
    assert text.count("\\{../shared/") >= 1
    text = text.replace("\\{../shared/", "\\{" + shared)   # the copy lives in another directory
    for a, (b, n) in (edits or {}).items():
        assert text.count(a) == n, (a, text.count(a))
        text = text.replace(a, b)
    return text


def written_conf(td, conf_rel=CONF_REL, edits=None, tap=True):
    path = os.path.join(td, "audspec_tap.conf" if tap else "audspec_copy.conf")
    with open(path, "w", encoding="latin-1") as f:
        f.write(edited_text(conf_rel, edits) + (TAP if tap else ""))
    return path


def read_level(path):
    if not os.path.exists(path) or os.path.getsize(path) <= 12:
        return None
    return lldo.read_htk(path)[0]


def run(pcm, fs, conf, td, tag, csv=False):
    exe = os.path.join(lldo.REF_DIR, "SMILExtract")
    wav, htk, csvp = os.path.join(td, tag + ".wav"), os.path.join(td, tag + ".htk"), os.path.join(td, tag + ".csv")
    lldo.write_wav(wav, pcm, fs)
    for p in [htk, csvp] + [os.path.join(td, t[1]) for t in TAPS]:
        if os.path.exists(p):
            os.remove(p)
    r = subprocess.run([exe, "-C", conf, "-I", wav, "-O", htk, "-l", "0"] + (["-csvoutput", csvp] if csv else []), cwd=td,
                       stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    out = dict(htk=open(htk, "rb").read() if os.path.exists(htk) else b"", rc=r.returncode,
               csv=open(csvp).read() if csv and os.path.exists(csvp) else "")
    out["lld"] = read_level(htk)
    for key, name in TAPS:
        out[key] = read_level(os.path.join(td, name))
    return out


def tmpdir():
    return tempfile.TemporaryDirectory(dir="/dev/shm" if os.path.isdir("/dev/shm") else None)


def reference(pcm, fs=16000, conf_rel=CONF_REL, edits=None):
    """{htk, lld, fftmag, melspec, plp} of one input: the (edited) file as it is, then its tapped copy"""
    with tmpdir() as td:
        a = run(pcm, fs, written_conf(td, conf_rel, edits, tap=False) if edits else os.path.join(lldo.REF_DIR, "config", conf_rel), td, "a")
        b = run(pcm, fs, written_conf(td, conf_rel, edits), td, "b")
    assert a["htk"] == b["htk"], "the tapped copy changed the lld file"
    rows = 0 if b["lld"] is None else len(b["lld"])
    for key, _ in TAPS:
        if b[key] is None:
            assert rows == 0, (key, rows)
        else:
            assert len(b[key]) == rows, (key, len(b[key]), rows)
    return b


def store(d, suffix, r, n):
    """lld always, melspec for inputs of at most TAP_MAX samples, fftmag for those of at most SHORT_MAX; the plp level is the lld
    level's first block (cVectorConcat copies it), which is asserted here instead of stored twice"""
    for key in ("lld",) + (("melspec",) if n <= TAP_MAX else ()) + (("fftmag",) if n <= SHORT_MAX else ()):
        d["%s_%s" % (key, suffix)] = r[key] if r[key] is not None else np.zeros((0, 0), np.float32)
    if r["lld"] is not None:
        nb = r["plp"].shape[1]
        assert (r["lld"][:, :nb].view(np.uint32) == r["plp"].view(np.uint32)).all() and r["melspec"].shape == r["plp"].shape


def main():
    lldo.build()
    assert lldo.have_ref(), "oracle/_ref/SMILExtract missing (the reference is not built)"
    d = {"inputs": np.array(INPUTS, np.int64)}
    on_floor = off_floor = 0
    for k, (idx, n, fs, div) in enumerate(INPUTS):
        r = reference(cut(idx, n, div), fs)
        store(d, str(k), r, n)
        lld, mel = d["lld_%d" % k], (r["melspec"] if r["melspec"] is not None else np.zeros((0, 0), np.float32))
        print("input", (idx, n, fs, div), "lld", lld.shape, "melspec", mel.shape, "kept:", sorted(x for x in d if x.endswith("_%d" % k)), "rc", r["rc"], "bands below the floor", int((mel < 1.0).sum()), "of", mel.size)
        if len(lld):
            assert lld.shape[1] == 78 and mel.shape[1] == 26
        on_floor += int((mel < 1.0).sum())
        off_floor += int((mel >= 1.0).sum())
    # what the fixture holds: both branches of cPlp's floor (plp.cpp:502), most bands above it
    assert (d["melspec_%d" % SILENCE] < 1.0).all() and len(d["melspec_%d" % SILENCE]) > 0, "the silence input must sit on the floor"
    assert on_floor > 0 and off_floor > 4 * on_floor, (on_floor, off_floor)
    for k in COMPAT_INPUTS:
        idx, n, fs, div = INPUTS[k]
        r = reference(cut(idx, n, div), fs, COMPAT_REL)
        store(d, "compat_%d" % k, r, n)
        same = d["lld_compat_%d" % k].shape == d["lld_%d" % k].shape and (d["lld_compat_%d" % k] == d["lld_%d" % k]).all()
        print("compat input", (idx, n, fs, div), "lld", d["lld_compat_%d" % k].shape, "equals audspec.conf's:", bool(same))
    for tag, edits in EDITS:
        for k in EDIT_INPUTS:
            idx, n, fs, div = INPUTS[k]
            r = reference(cut(idx, n, div), fs, CONF_REL, edits)
            store(d, "%s_%d" % (tag, k), r, n)
            e = d["lld_%s_%d" % (tag, k)]
            same = e.shape == d["lld_%d" % k].shape and (e == d["lld_%d" % k]).all()
            print(tag, "input", (idx, n, fs, div), "lld", e.shape, "equals the shipped file's:", bool(same))
            if tag == "inert":                             # lpOrder, firstCC, cepLifter: no effect on the auditory spectrum
                assert same, "the inert-options copy changed the output"
            else:
                assert not same, tag
    with tmpdir() as td:                                   # the names and the HTK header: the file's own sinks
        idx, n, fs, div = INPUTS[7]
        r = run(cut(idx, n, div), fs, os.path.join(lldo.REF_DIR, "config", CONF_REL), td, "h", csv=True)
    d["csv_header"] = np.array(r["csv"].splitlines()[0])
    d["htk_header"] = np.array(struct.unpack(">IIHH", r["htk"][:12]), np.int64)
    print("header:", str(d["csv_header"])[:120], "...", "htk:", d["htk_header"])
    np.savez_compressed(os.path.join(OUT, "audspec_synth.npz"), **d)
    h = {}
    for name, pcm in hard_signals.signals().items():
        r = reference(pcm)
        h["lld_" + name] = r["lld"] if r["lld"] is not None else np.zeros((0, 78), np.float32)
        print(name, h["lld_" + name].shape, "bands on the floor", int((r["melspec"] < 1.0).sum()) if r["melspec"] is not None else 0)
    np.savez_compressed(os.path.join(OUT, "hard_audspec.npz"), **h)
    exe = os.path.join(lldo.REF_DIR, "SMILExtract")
    with tempfile.TemporaryDirectory() as td:
        for stem in ("u2_8000", "u3_4000"):
            for tag, rel in (("audspec", CONF_REL), ("audspec_compat", COMPAT_REL)):
                subprocess.run([exe, "-C", os.path.join(lldo.REF_DIR, "config", rel), "-I", os.path.join(OUT, "files", stem + ".wav"), "-O",
                                os.path.join(td, "o.htk"), "-csvoutput", os.path.join(td, "o.csv"), "-l", "0"], check=True, cwd=td)
                shutil.copy(os.path.join(td, "o.htk"), os.path.join(OUT, "files", "%s_%s.htk" % (tag, stem)))
                if tag == "audspec":
                    shutil.copy(os.path.join(td, "o.csv"), os.path.join(OUT, "files", "%s_%s.csv" % (tag, stem)))
                os.remove(os.path.join(td, "o.htk"))
                os.remove(os.path.join(td, "o.csv"))
    for f in ("audspec_synth.npz", "hard_audspec.npz", "files/audspec_u2_8000.htk", "files/audspec_u2_8000.csv", "files/audspec_u3_4000.htk",
              "files/audspec_u3_4000.csv", "files/audspec_compat_u2_8000.htk", "files/audspec_compat_u3_4000.htk"):
        print(f, os.path.getsize(os.path.join(OUT, f)), "bytes")


if __name__ == "__main__":
    main()
