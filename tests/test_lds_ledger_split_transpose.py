"""The split-complex transposition buffer of lld_mfcc512 in the LDS ledger (tools/lds_bank_sim.py, `split_layout`): two address-free
stores per index and four ds_read_b128 per plane are free of bank conflicts in all eight wave regions of a block, for MP = 13 and
16, UC = 6 and 8 and both lane -> column maps; the bench instance's ledger has the figures the change was made for (the
transposition's stores 96 -> 64 busy cycles, the pass 466 -> 434); every instance's block fits twice into a CU's LDS and every
wave's region into the 16 bits of M0. The model is not vacuous: no uniform row stride is conflict-free, and a row moved off its
quad collides. The table is the kernel source's."""
import importlib.util
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (MP, UC, regression stages fused, PLP chain): every class of instance; the column map goes by the last two and MP
INSTANCES = [(mp, uc, delta, plp) for mp in (13, 16) for uc in (6, 8) for delta in (False, True) for plp in (False, True)]


@pytest.fixture(scope="module")
def sim():
    spec = importlib.util.spec_from_file_location("lds_bank_sim_split", os.path.join(ROOT, "tools", "lds_bank_sim.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.mark.parametrize("mp,uc,delta,plp", INSTANCES)
def test_stores_and_loads_are_conflict_free_in_every_wave_region(sim, mp, uc, delta, plp):
    L = sim.split_layout(mp, uc, delta, plp)
    assert L.split and L.column_map == sim.one_hop_exchange(mp, plp, delta)
    for wave in range(8):
        assert sim.transposition_split(wave, L) == (0, 0), wave
        led = sim.ledger(L, wave, delta=delta)
        assert led.conflicts(sim.TR_WRITE_SPLIT) == 0 and led.conflicts(sim.TR_READ_SPLIT) == 0
        assert led.kinds(sim.TR_WRITE_SPLIT) == {"wtid": 32} and led.kinds(sim.TR_READ_SPLIT) == {"r128": 8}
        assert sim.TR_WRITE not in led.rows and sim.TR_READ not in led.rows
        # nothing else moves: every other class has the figures of the interleaved buffer's ledger
        old = sim.ledger(sim.tree_layout(mp, uc, delta), wave, delta=delta)
        for name in old.rows:
            if name not in (sim.TR_WRITE, sim.TR_READ):
                assert (led.count(name), led.array(name), led.conflicts(name), led.transfer(name)) == \
                    (old.count(name), old.array(name), old.conflicts(name), old.transfer(name)), (wave, name)


def test_bench_instance_ledger(sim):
    for wave in range(8):
        led = sim.ledger(sim.split_layout(), wave)
        w, r = sim.TR_WRITE_SPLIT, sim.TR_READ_SPLIT
        assert (led.count(w), led.array(w), led.conflicts(w), led.transfer(w), led.busy(w)) == (32, 64, 0, 64, 64)
        assert (led.count(r), led.array(r), led.conflicts(r), led.busy(r)) == (8, 32, 0, 32)
        t = led.totals()
        assert t["instructions"] == 141 and t["busy"] == 434 and t["array"] == 374
        old = sim.ledger(sim.tree_layout(), wave)
        assert old.totals()["busy"] == 466 and old.busy(sim.TR_WRITE) == 96 and old.totals()["instructions"] == 133


@pytest.mark.parametrize("mp,uc,delta,plp", INSTANCES)
def test_block_fits_twice_and_regions_fit_m0(sim, mp, uc, delta, plp):
    L = sim.split_layout(mp, uc, delta, plp)
    assert L.k_wave == sim.K_TS_WAVE and 4 * (L.k_lmel + L.k_pb) <= L.k_wave and L.k_wave % 4 == 0
    block = 4 * (L.shared + 8 * L.k_wave)
    assert block <= 81920                                              # two blocks per CU: 163 840 bytes
    assert 4 * sim.wave_base(7, L) < 65536                             # M0 holds 16 bits of LDS byte address
    assert sim.table_base(L) == 8 * L.k_wave and sim.wave_base(0, L) == 0
    rows = sorted(sim.tsplit_base(r, im) for r in range(16) for im in (False, True))
    assert all(b - a >= 64 for a, b in zip(rows, rows[1:])) and rows[0] == 0 and rows[-1] + 64 == L.k_wave      # rows do not overlap
    assert all(b % 4 == 0 for b in rows)                               # 16-byte aligned ds_read_b128
    assert all(sim.tsplit_base(r, True) - sim.tsplit_base(r, False) == 128 for r in range(16))


def test_model_is_not_vacuous(sim):
    for L in (sim.split_layout(), sim.split_layout(16, 6, True)):         # both lane -> column maps
        assert sim.transposition_split(0, L) == (0, 0)
        for stride in range(64, 132, 4):                                   # no uniform row stride serves the loads
            _, loads = sim.transposition_split(0, L, base=lambda r, im=False: stride * r + (16 * stride if im else 0))
            assert loads > 0, stride
        # one row on a bank quad outside 0 .. 3, 8 .. 11 collides with a row of the neighbouring frame group
        _, loads = sim.transposition_split(0, L, base=lambda r, im=False: sim.tsplit_base(r, im) + (16 if r == 2 else 0))
        assert loads > 0
        # two rows of one lane set on one quad collide
        _, loads = sim.transposition_split(0, L, base=lambda r, im=False: sim.tsplit_base(r, im) + (4 if r == 0 else 0))
        assert loads > 0
        # stores are lane-linear: free wherever the rows stand
        stores, _ = sim.transposition_split(0, L, base=lambda r, im=False: 67 * r + (1100 if im else 0))
        assert stores == 0


def test_table_follows_the_kernel(sim):
    src = open(os.path.join(ROOT, "opensmile_amd", "csrc", "lld_mfcc512.hip")).read()
    assert f"constexpr int kTSWaveFloats = {sim.K_TS_WAVE};" in src
    m = re.search(r"constexpr bool split_transpose\(\) \{\s*return (.*?);", src)
    assert m and m.group(1) == "!PLP && !(MP == 16 && DELTA)"
    assert [sim.split_transpose(mp, plp, delta) for mp in (13, 16) for plp in (False, True) for delta in (False, True)] == \
        [not plp and not (mp == 16 and delta) for mp in (13, 16) for plp in (False, True) for delta in (False, True)]
    assert sim.split_transpose(13) and sim.split_layout().column_map          # the bench's instance takes the split form
    # the kernel's constexpr table, evaluated by a C++ compiler from its source text
    fn = re.search(r"constexpr int tsplit_base\(int r, bool imag\) \{.*?\n\}", src, re.S).group(0)
    prog = "#include <cstdio>\n" + fn + "\nint main() { for (int r = 0; r < 16; ++r) for (int i = 0; i < 2; ++i) " \
        "std::printf(\"%d \", tsplit_base(r, i != 0)); return 0; }\n"
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.cpp"), "w").write(prog)
        subprocess.run([cxx, "-std=c++17", "-o", os.path.join(d, "t"), os.path.join(d, "t.cpp")], check=True)
        got = [int(x) for x in subprocess.run([os.path.join(d, "t")], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [sim.tsplit_base(r, i) for r in range(16) for i in (False, True)]
