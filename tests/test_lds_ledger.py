"""tools/lds_bank_sim.py as a per-pass LDS ledger of lld_mfcc512. With the kernel's layout (band vectors 68 floats apart) the DCT's
band-vector reads and the transposition are free of bank conflicts in all eight wave regions of a block, for MP = 13 and 16 and for
UC = 6 and 8, and no read of the power buffer, of the mel weights or of the DCT rows has more conflict cycles than in the parent's
layout. The lane-major layout of the loop-invariant tables (built, measured and not taken: DESIGN.md 4.1) is conflict-free on each
of its tables. The model is not vacuous (the parent's 64 floats give the 28 cycles it always reported; a table row that is a multiple
of 16 bank quads collides), and the instruction count of each class is the one the kernel source's loop bounds give."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INSTANCES = [(mp, uc) for mp in (13, 16) for uc in (6, 8)]


@pytest.fixture(scope="module")
def sim():
    spec = importlib.util.spec_from_file_location("lds_bank_sim_ledger", os.path.join(ROOT, "tools", "lds_bank_sim.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.fixture(scope="module")
def tables(sim):
    """uc -> (unit octets, the builder's own extra cycles) from the library's host-side dump: 26 bands (the bench) and 24 bands"""
    out = {}
    for n_bands in (26, 24):
        octets, extra = sim.library_tables(n_bands)
        out[len(octets)] = (octets, extra)
    assert sorted(out) == [6, 8]
    return out


def test_recorded_unit_table_is_the_library_s(sim, tables):
    octets, extra = tables[6]
    assert octets == sim.BENCH_OCTETS and extra == sim.BENCH_BUILDER_EXTRA


@pytest.mark.parametrize("mp,uc", INSTANCES)
def test_layouts_are_conflict_free_where_they_claim(sim, tables, mp, uc):
    octets, extra = tables[uc]
    tree, parent, cand = sim.tree_layout(mp, uc), sim.parent_layout(mp, uc), sim.lane_major_layout(mp, uc)
    assert tree.k_lmel == 68 and not tree.lane_major and tree.shared == parent.shared
    assert cand.row % 8 == 4 and cand.shared < parent.shared
    for L in (tree, cand):
        assert 4 * (L.k_lmel + L.k_pb) <= L.k_wave
        assert 4 * (L.shared + 8 * L.k_wave) * 2 <= 160 * 1024           # two blocks of eight waves per CU
    for wave in range(8):
        old = sim.ledger(parent, wave, octets)
        for L in (tree, cand):
            new = sim.ledger(L, wave, octets)
            for name in (sim.LMEL_READ, sim.WINDOW, sim.TW256, sim.TW512, sim.TR_WRITE, sim.TR_READ):
                assert new.conflicts(name) == 0, (wave, name, new.conflicts(name))
            assert sim.transposition(wave=wave, layout=L) == (0, 0, True)
            for name in (sim.MEL_POWER, sim.MEL_WEIGHT, sim.DCT_READ, sim.POWER_WRITE, sim.BAND_WRITE):
                assert new.conflicts(name) <= old.conflicts(name), (wave, name, new.conflicts(name), old.conflicts(name))
            # the power-buffer reads: what the host's own bank model reports, on each of the 4 lane groups of both reads of a unit
            assert new.conflicts(sim.MEL_POWER) == old.conflicts(sim.MEL_POWER) == 8 * extra
            assert new.conflicts(sim.MEL_WEIGHT) == 0 and new.conflicts(sim.DCT_READ) == 0
            assert new.busy(sim.POWER_WRITE) == new.transfer(sim.POWER_WRITE)      # at most 2-way: free under the store's transfer
            assert new.totals()["conflicts"] == old.totals()["conflicts"] - 28


@pytest.mark.parametrize("mp,uc", INSTANCES)
def test_model_is_not_vacuous(sim, mp, uc):
    for wave in range(8):
        assert sim.ledger(sim.parent_layout(mp, uc), wave).conflicts(sim.LMEL_READ) == 28
        assert sim.ledger(sim.lane_major_layout(mp, uc, k_lmel=64), wave).conflicts(sim.LMEL_READ) == 28
        for row in (128, 192):                            # a multiple of 16 bank quads: the sixteen rows start on one quad
            bad = sim.ledger(sim.lane_major_layout(mp, uc, tab_row=row), wave)
            for name in (sim.WINDOW, sim.TW256, sim.TW512):
                assert bad.conflicts(name) > 0, (row, name)
        even = sim.ledger(sim.lane_major_layout(mp, uc, tab_row=sim.lane_major_layout(mp, uc).row + 4), wave)      # an even number of quads
        assert even.conflicts(sim.WINDOW) > 0


@pytest.mark.parametrize("mp,uc", INSTANCES)
def test_instruction_counts_are_the_kernel_source_s(sim, mp, uc):
    b = sim.kernel_loop_bounds()
    assert b["window_reads_per_m"] == 1 and b["mel_reads_per_unit"] == 4
    for L in (sim.parent_layout(mp, uc), sim.tree_layout(mp, uc)):
        led = sim.ledger(L)
        assert [led.count(n) for n in (sim.WINDOW, sim.TW256, sim.TR_WRITE, sim.TR_READ, sim.TW512)] == [mp, 15, 16, 16, 8]
        from_source = [mp * b["window_reads_per_m"], b["tw256_reads"], b["transpose_write"], b["transpose_read"], b["tw512_reads"]]
        assert [led.count(n) for n in (sim.WINDOW, sim.TW256, sim.TR_WRITE, sim.TR_READ, sim.TW512)] == from_source
        assert led.count(sim.MEL_POWER) == led.count(sim.MEL_WEIGHT) == 2 * uc
        assert led.count(sim.MEL_POWER) + led.count(sim.MEL_WEIGHT) == b["mel_reads_per_unit"] * uc
        assert led.count(sim.LMEL_READ) == led.count(sim.DCT_READ) == 7 and led.count(sim.BPERMUTE) == 5
        if (mp, uc) == (13, 6):                           # the bench's instance: SQ_INSTS_LDS / wave-passes = 133.3
            assert led.totals()["instructions"] == 133
    cand = sim.ledger(sim.lane_major_layout(mp, uc))
    # all of them 16-byte reads but the two whose second pair nobody uses (the window's last at MP = 13, tw256's pair k1 = 0)
    assert cand.kinds(sim.WINDOW) == ({"r128": 6, "r64": 1} if mp == 13 else {"r128": 8})
    assert cand.kinds(sim.TW256) == {"r128": 7, "r64": 1} and cand.kinds(sim.TW512) == {"r128": 4}


def test_layout_constants_follow_the_kernel(sim):
    src = open(os.path.join(ROOT, "opensmile_amd", "csrc", "lld_mfcc512.hip")).read()
    for name, val in (("kTB2Row", sim.K_TB2_ROW), ("kLmelFloats", sim.K_LMEL), ("kOctetFloats", sim.K_OCTET),
                      ("kPbFloats", sim.K_PB), ("kWaveFloats", sim.K_WAVE)):
        assert f"constexpr int {name} = {val};" in src, name
    assert "256 * 2 + MP * 16 * 2 + 256 * 2 + UC * 16 * 8 + 16 * 28 + 48" in src and sim.tree_layout().shared == 256 * 2 + 13 * 32 + 512 + 6 * 128 + 448 + 48
