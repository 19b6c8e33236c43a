"""tools/lds_bank_sim.py models the present transposition layout of lld_mfcc512 (rows of four groups interleaved, 65 float2 per
row): the sixteen b64 stores and the sixteen b64 loads are conflict-free in the order of the DFT layers (0, 4, 8, 12 | 1, 5, 9, 13
| ...: round 8's order of the stores, and of the loads under SMILEHIP_MFCC512_READS_IN_DFT_ORDER) and in the parent's index order -- the same count, because an instruction's lane -> bank
pattern depends on its own index only."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _sim():
    spec = importlib.util.spec_from_file_location("lds_bank_sim", os.path.join(ROOT, "tools", "lds_bank_sim.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_transposition_conflict_free_in_both_orders():
    sim = _sim()
    assert sim.TRANSPOSE_ORDER_R8[:8] == [0, 4, 8, 12, 1, 5, 9, 13]
    assert sim.TRANSPOSE_ORDER_PARENT == list(range(16))
    for wave in range(8):                                  # every wave region of a block
        new = sim.transposition(sim.TRANSPOSE_ORDER_R8, sim.TRANSPOSE_ORDER_R8, wave)
        old = sim.transposition(sim.TRANSPOSE_ORDER_PARENT, sim.TRANSPOSE_ORDER_PARENT, wave)
        assert new == (0, 0, True), (wave, new)
        assert old == new, (wave, old, new)


def test_model_detects_an_unpadded_layout():
    """The model is not vacuous: without the 8 bytes of row padding (64 float2 per row) the column loads collide."""
    sim = _sim()
    sim.K_TB2_ROW = 64
    _, loads, _ = sim.transposition()
    assert loads > 0


def test_layout_constants_match_the_kernel():
    src = open(os.path.join(ROOT, "opensmile_amd", "csrc", "lld_mfcc512.hip")).read()
    sim = _sim()
    for name, val in (("kTB2Row", sim.K_TB2_ROW), ("kLmelFloats", sim.K_LMEL), ("kOctetFloats", sim.K_OCTET),
                      ("kPbFloats", sim.K_PB), ("kWaveFloats", sim.K_WAVE)):
        assert f"constexpr int {name} = {val};" in src, name
