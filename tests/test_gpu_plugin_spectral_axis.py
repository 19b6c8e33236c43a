"""cSpectral on any spectrum inside the UNMODIFIED reference binary (oracle/_ref/SMILExtract) through the plugin, every override on
and no component on the reference's CPU code: the file the run writes equals the plain binary's byte for byte. Both graphs hold
cSpectral instances that the wave-parallel routes (ComParE's set, the two GeMAPS sets) do not take; before
smilehip_spectral_axis_op_* such a run ended with the plugin's cSpectral refusal."""
import os
import shutil
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLUGDIR = os.path.join(ROOT, "opensmile_amd", "plugin")
CONF_FILE = os.path.join(ROOT, "tests", "conf", "spectral_axis.conf")


def _smilextract(oracle, tmp_path, tag, pcm, fs, conf, out_opt, env_extra):
    exe = os.path.join(oracle.REF_DIR, "SMILExtract")
    plug = os.path.join(PLUGDIR, "plugins", "libsmilehip_plugin.so")
    if not (os.path.exists(exe) and os.path.exists(plug)):
        pytest.skip("oracle/_ref/SMILExtract or the plugin .so not built (needs the reference sources at build time)")
    wav, out, trace = (str(tmp_path / f"{tag}_{n}") for n in ("in.wav", "out.htk", "trace.txt"))
    oracle.write_wav(wav, pcm, fs)
    e = dict(os.environ)
    e["LD_LIBRARY_PATH"] = os.pathsep.join([os.path.join(ROOT, "opensmile_amd"), oracle.REF_DIR, e.get("LD_LIBRARY_PATH", "")])
    e["SMILEHIP_PLUGIN_TRACE"] = trace
    e.pop("SMILEHIP_PLUGIN_ALLOW_CPU", None)
    e.update(env_extra or {})
    r = subprocess.run([exe, "-C", conf, "-I", wav, out_opt, out, "-l", "1"], cwd=PLUGDIR, env=e, capture_output=True, text=True,
                       errors="replace", timeout=300)
    data = open(out, "rb").read() if os.path.exists(out) else b""
    tr = dict(l.split() for l in open(trace).read().split("\n") if l.strip()) if os.path.exists(trace) else {}
    return r, data, {k: int(v) for k, v in tr.items()}


def _same_file(oracle, tmp_path, pcm, fs, conf, out_opt):
    r0, ref, _ = _smilextract(oracle, tmp_path, "plain", pcm, fs, conf, out_opt, {"SMILEHIP_PLUGIN_COMPONENTS": "none"})
    assert r0.returncode == 0 and len(ref) > 12, r0.stderr[-2000:]
    r1, own, tr = _smilextract(oracle, tmp_path, "plugin", pcm, fs, conf, out_opt, None)
    assert r1.returncode == 0, (r1.stderr + r1.stdout)[-2000:]
    assert not [k for k, v in tr.items() if k.endswith(".cpu") and v], tr
    assert own == ref
    return tr, ref


@pytest.mark.parametrize("fs", [16000, 44100])
def test_plugin_runs_the_option_sets(oracle, tmp_path, fs):
    """tests/conf/spectral_axis.conf: nine cSpectral instances (log spectrum with three slopes on two ranges, normalised bands, the new
    slope scale, the old roll-off, power input, behind a bark and a mel cSpecScale, the GeMAPS options), on 257 and on 1025 bins"""
    from opensmile_amd import synth
    pcm = synth.utterance(3, 6400)
    tr, ref = _same_file(oracle, tmp_path, pcm, fs, CONF_FILE, "-O")
    n_col = (257 if fs == 16000 else 1025) + 138
    n_frames = (len(ref) - 12) // (4 * n_col)
    assert len(ref) == 12 + 4 * n_col * n_frames and n_frames >= 2
    assert tr.get("cSpectral", 0) == 9 * n_frames, tr


def test_plugin_runs_an_edited_egemaps_chain(oracle, tmp_path):
    """eGeMAPSv02's LLD chain with one edit to its log-spectral instance: a third slope band (oldSlopeScale = 0 as the file has it)
    on 25 ms frames -- no longer one of the two GeMAPS sets, so the instance goes to the operator for any option set"""
    from opensmile_amd import synth
    for d in ("shared", "gemaps", "egemaps"):
        shutil.copytree(os.path.join(oracle.REF_DIR, "config", d), tmp_path / "config" / d)
    inc = tmp_path / "config" / "gemaps" / "v01b" / "GeMAPSv01b_core.lld.conf.inc"
    text = inc.read_text(errors="replace")
    assert text.count("slopes[1] = 500-1500\n") == 1 and text.count("frameSize = 0.020\n") == 1
    text = text.replace("slopes[1] = 500-1500\n", "slopes[1] = 500-1500\nslopes[2] = 1500-3000\n").replace("frameSize = 0.020\n", "frameSize = 0.025\n")
    inc.write_text(text)
    pcm = synth.utterance(10, 9600)
    tr, ref = _same_file(oracle, tmp_path, pcm, 16000, str(tmp_path / "config" / "egemaps" / "v02" / "eGeMAPSv02.conf"), "-lldhtkoutput")
    assert tr.get("cSpectral", 0) > 0, tr
