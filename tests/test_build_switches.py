"""The compile-time switches of opensmile_amd/csrc are the ones listed here and no others: every identifier that a preprocessor
condition (#if, #ifdef, #ifndef, #elif) of a .hip / .hpp / .cpp file tests. A measured-and-rejected form is recorded in DESIGN.md
and taken out of the source, it does not stay behind a macro; a new switch has to be added to this list on purpose, with the
tool that defines it."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "opensmile_amd", "csrc")

SWITCHES = {
    "SMILEHIP_PHASE_TIMING",   # tools/ubench/variant.sh, variant_any.sh, variant_cmp.sh, variant_f0.sh: phase_timing.hpp's counters
    "SMILEHIP_DEBUG_KNOBS",    # tools/ubench/variant.sh (make MFCC512_EXTRA=...): the SMILEHIP_DEBUG_GRID environment switch
    "QPHASE",                  # tools/dev/phase_insts.sh: lld_compare_quad.hpp's phase marks as assembler comments
}
# set by the compiler, not by a build of ours (glibc_float.hpp: one source for the host check and the device)
COMPILER_MACROS = {"__HIPCC__", "__HIP_DEVICE_COMPILE__"}

_CONDITION = re.compile(r"^[ \t]*#[ \t]*(if|ifdef|ifndef|elif)\b(.*)$", re.M)
_IDENT = re.compile(r"[A-Za-z_]\w*")


def _tested_identifiers(text):
    text = re.sub(r"\\\n", " ", text)                      # a condition continued over lines is one condition
    found = set()
    for _, cond in _CONDITION.findall(text):
        cond = re.sub(r"//.*|/\*.*?\*/", " ", cond)
        found.update(i for i in _IDENT.findall(cond) if i != "defined")
    return found


def test_the_parser_sees_every_form_of_condition():
    text = ("#ifdef A\n#endif\n  # ifndef B // not C\n#if defined(D) || \\\n    !defined E && F > 2\n#elif defined(G)\n#else\n#endif\n"
            "// #ifdef H\nint x; #ifdef I\n")
    assert _tested_identifiers(text) == {"A", "B", "D", "E", "F", "G"}


def test_compile_time_switches_are_the_listed_ones():
    files = sorted(f for ext in ("hip", "hpp", "cpp") for f in glob.glob(os.path.join(CSRC, "*." + ext)))
    assert len(files) > 30, files                          # the directory was found
    where = {}
    for f in files:
        for ident in _tested_identifiers(open(f).read()):
            where.setdefault(ident, []).append(os.path.basename(f))
    for ident in COMPILER_MACROS:
        where.pop(ident, None)
    unlisted = {i: fs for i, fs in where.items() if i not in SWITCHES}
    assert not unlisted, f"compile-time switches that tests/test_build_switches.py does not list: {unlisted}"
    gone = SWITCHES - set(where)
    assert not gone, f"listed switches that no source file tests any more: {sorted(gone)}"
