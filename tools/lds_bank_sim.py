#!/usr/bin/env python3
"""LDS bank-conflict model of the fast MFCC kernel's wave-level access patterns (opensmile_amd/csrc/lld_mfcc512.hip, the layout
of its `LDS layout` comment; bank rules of the gfx950 LDS: 64 banks of 4 bytes, a b64 load served per half wave, a b64 store and
a b128 access per group of 16 lanes). Prints the extra (conflict) cycles per DS instruction class for one pass of one wave.

The transposition is modelled per instruction and in issue order (`transposition`): an instruction's lane -> bank pattern depends
on its own row / column index only, so the ORDER in which the sixteen stores and the sixteen loads are issued cannot change the
conflict count -- the function checks that and returns the count for any order (since round 8 the stores are issued in the order of
the first DFT's last layer, TRANSPOSE_ORDER_R8; the loads in that order too were measured and are no gain; before
round 8 both were issued in index order)."""
import numpy as np

MP, UC = 13, 6                       # the bench's instance
K_TB2_ROW = 65                       # float2 per 4-group row of the transpose buffer
K_LMEL, K_OCTET, K_PB, K_WAVE = 64, 12, 448, 2080
SHARED = 256 * 2 + MP * 16 * 2 + 256 * 2 + UC * 16 * 8 + 16 * 28 + 48      # floats in front of the per-wave regions
OFF_TW512, OFF_WIN = 0, 512
OFF_TW256 = OFF_WIN + MP * 32
OFF_MELW0 = OFF_TW256 + 512
OFF_MELW1 = OFF_MELW0 + UC * 64
OFF_DCT = OFF_MELW1 + UC * 64

TRANSPOSE_ORDER_PARENT = list(range(16))
TRANSPOSE_ORDER_R8 = [q + 4 * p for q in range(4) for p in range(4)]       # 0, 4, 8, 12 | 1, 5, 9, 13 | ...


def groups(kind):
    if kind in ("r32", "w32", "r64"):
        return [list(range(0, 32)), list(range(32, 64))]
    if kind in ("w64", "r2_64"):
        return [list(range(16 * i, 16 * i + 16)) for i in range(4)]
    if kind == "r128":
        return [[0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27],
                [4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31],
                [32, 33, 34, 35, 44, 45, 46, 47, 52, 53, 54, 55, 56, 57, 58, 59],
                [36, 37, 38, 39, 40, 41, 42, 43, 48, 49, 50, 51, 60, 61, 62, 63]]
    raise ValueError(kind)


def cost(kind, addr_bytes, active=None):
    """extra cycles beyond the conflict-free cost for one wave instruction"""
    nb = {"r32": 32, "w32": 32, "w64": 32, "r2_64": 32, "r64": 64, "r128": 64}[kind]
    width = {"r32": 1, "w32": 1, "w64": 2, "r2_64": 2, "r64": 2, "r128": 4}[kind]
    extra = 0
    for g in groups(kind):
        per_bank = {}
        for l in g:
            if active is not None and not active[l]:
                continue
            a = int(addr_bytes[l])
            for k in range(width):
                bank = ((a // 4) + k) % nb
                per_bank.setdefault(bank, set()).add((a // 4 + k))
        worst = max((len(v) for v in per_bank.values()), default=1)
        extra += worst - 1
    return extra


lane = np.arange(64)
g, j = lane >> 4, lane & 15


def wave_base(wave=0):
    return SHARED + wave * K_WAVE


def transposition(store_order=TRANSPOSE_ORDER_R8, load_order=TRANSPOSE_ORDER_R8, wave=0):
    """The 16 ds_write_b64 (row k1 of group g: float2 index g*16 + j + k1*65) and the 16 ds_read_b64 (column jj: g*16 + j*65 + jj)
    in the given issue orders -> (extra cycles of the stores, of the loads, order_independent). `order_independent`: every
    instruction has the conflict count it has in index order (its addresses do not depend on its position)."""
    assert sorted(store_order) == list(range(16)) and sorted(load_order) == list(range(16))
    wb = wave_base(wave)
    st = {k1: cost("w64", 4 * wb + 8 * (g * 16 + j + k1 * K_TB2_ROW)) for k1 in range(16)}
    ld = {jj: cost("r64", 4 * wb + 8 * (g * 16 + j * K_TB2_ROW + jj)) for jj in range(16)}
    st_seq = [cost("w64", 4 * wb + 8 * (g * 16 + j + k1 * K_TB2_ROW)) for k1 in store_order]
    ld_seq = [cost("r64", 4 * wb + 8 * (g * 16 + j * K_TB2_ROW + jj)) for jj in load_order]
    same = st_seq == [st[k] for k in store_order] and ld_seq == [ld[k] for k in load_order]
    return sum(st_seq), sum(ld_seq), same


def pb_pos(k):
    return k + (K_OCTET - 8) * (k >> 3)


def model(wave=0):
    tot = {}

    def add(name, c):
        tot[name] = tot.get(name, 0) + c

    wb = wave_base(wave)
    lmel = wb + g * K_LMEL
    pb = wb + 4 * K_LMEL + g * K_PB
    for m in range(MP):
        add("window read b64", cost("r64", 4 * (OFF_WIN + 2 * (m * 16 + j))))
    for k1 in range(1, 16):
        add("tw256 read b64", cost("r64", 4 * (OFF_TW256 + 2 * (k1 * 16 + j))))
    s, l, _ = transposition(wave=wave)
    add("transpose write b64", s)
    add("transpose read b64", l)
    for q in range(8):
        add("tw512 read b64", cost("r64", 4 * (OFF_TW512 + 2 * (j + 16 * q))))
        add("power write b32", cost("w32", 4 * (pb + pb_pos(j) + 2 * K_OCTET * q)) + cost("w32", 4 * (pb + pb_pos(256 - j) - 2 * K_OCTET * q)))
    for i in range(UC):
        # the octets of a step are the host's choice (fast512_build_host orders every lane's units so that the 16 lanes of a frame
        # touch 16 different bank quads and prints its own count with SMILEHIP_DEBUG_TABLES=1); the weights are table rows
        add("mel weight read b128", cost("r128", 4 * (OFF_MELW0 + 4 * (i * 16 + j))) + cost("r128", 4 * (OFF_MELW1 + 4 * (i * 16 + j))))
    act = j < 13
    for q in range(7):
        add("log-mel read b128", cost("r128", 4 * (lmel + 4 * q), act))
        add("dct read b128", cost("r128", 4 * (OFF_DCT + j * 28 + 4 * q), act))
    return tot


def main():
    tot = model()
    for name, c in tot.items():
        print(f"{name:22s} extra cycles {c}")
    print("total extra", sum(tot.values()))
    for name, order in (("index order (parent)", TRANSPOSE_ORDER_PARENT), ("DFT-layer order (round 8)", TRANSPOSE_ORDER_R8)):
        worst_s = worst_l = 0
        for wave in range(8):
            s, l, same = transposition(order, order, wave)
            assert same
            worst_s, worst_l = max(worst_s, s), max(worst_l, l)
        print(f"transposition, {name}: stores {worst_s}, loads {worst_l} extra cycles (worst of the 8 waves of a block); "
              "the per-instruction lane -> bank pattern does not depend on the issue order")


if __name__ == "__main__":
    main()
