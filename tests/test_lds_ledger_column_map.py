"""lld_mfcc512's lane-to-column map of the second DFT16 (lane j transforms column KC[j] = 0 .. 7, 9 .. 15, 8) in the LDS ledger
(tools/lds_bank_sim.py): the transposition's loads, the tw512 reads and the power buffer's stores go by the map, and the map permutes
the sixteen lanes of a frame group, whole frame groups of which make up every lane group of those instructions. So the ledger with
the map gives the ledger without it -- every class's instruction count, array, conflict and transfer cycles -- in all eight wave
regions of a block, for MP = 13 and 16 and UC = 6 and 8; and the map is the one the kernel source states."""
import dataclasses
import importlib.util
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INSTANCES = [(mp, uc) for mp in (13, 16) for uc in (6, 8)]


@pytest.fixture(scope="module")
def sim():
    spec = importlib.util.spec_from_file_location("lds_bank_sim_column_map", os.path.join(ROOT, "tools", "lds_bank_sim.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_map_pairs_partner_columns_under_row_mirror(sim):
    kc = [int(x) for x in sim.KC[:16]]
    assert sorted(kc) == list(range(16)) and kc[0] == 0 and kc[15] == 8
    for i in range(1, 15):
        assert kc[i] + kc[15 - i] == 16, i                 # bin kc + 16 q pairs with column 16 - kc
    assert all(int(sim.KC[l]) == kc[l & 15] for l in range(64))
    src = open(os.path.join(ROOT, "opensmile_amd", "csrc", "lld_mfcc512.hip")).read()
    assert "(j < 8 ? j : (j == 15 ? 8 : j + 1))" in src
    for use in ("kc * kTB2Row", "s_tw512[kc + 16 * q]", "pb_pos(kc)", "pb_pos(256 - kc)"):
        assert use in src, use
    m = re.search(r"constexpr bool one_hop_exchange\(\) \{\s*return (.*?);", src)
    assert m and m.group(1) == "!PLP && !(MP == 16 && DELTA)"
    assert [sim.one_hop_exchange(mp, plp, delta) for mp in (13, 16) for plp in (False, True) for delta in (False, True)] == \
        [not plp and not (mp == 16 and delta) for mp in (13, 16) for plp in (False, True) for delta in (False, True)]
    assert sim.tree_layout(13, 6).column_map and not sim.tree_layout(16, 6).column_map and sim.tree_layout(16, 6, delta=False).column_map


@pytest.mark.parametrize("mp,uc", INSTANCES)
def test_ledger_with_the_map_is_the_parent_s(sim, mp, uc):
    base = dataclasses.replace(sim.tree_layout(mp, uc), column_map=False)
    mapped = dataclasses.replace(base, column_map=True)
    for wave in range(8):
        old, new = sim.ledger(base, wave), sim.ledger(mapped, wave)
        assert list(old.rows) == list(new.rows)
        for name in old.rows:
            want = (old.count(name), old.kinds(name), old.array(name), old.conflicts(name), old.transfer(name), old.busy(name))
            got = (new.count(name), new.kinds(name), new.array(name), new.conflicts(name), new.transfer(name), new.busy(name))
            assert got == want, (wave, name, got, want)
        assert old.totals() == new.totals()
        assert sim.transposition(wave=wave, layout=mapped) == sim.transposition(wave=wave, layout=base) == (0, 0, True)


def test_map_is_seen_by_the_model(sim):
    """Not vacuous: the mapped addresses differ lane by lane, and the mapped loads still collide where the unmapped ones do (a
    transposition row without its 8 bytes of padding)."""
    mapped = dataclasses.replace(sim.tree_layout(), column_map=True)
    assert (sim.column(mapped) != sim.j).sum() == 4 * 8 and (sim.column(dataclasses.replace(mapped, column_map=False)) == sim.j).all()
    unpadded = dataclasses.replace(mapped, k_tb2_row=64)
    _, loads, _ = sim.transposition(layout=unpadded)
    _, loads_unmapped, _ = sim.transposition(layout=dataclasses.replace(unpadded, column_map=False))
    assert loads == loads_unmapped > 0
