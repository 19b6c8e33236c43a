#!/usr/bin/env python3
"""Per-pass LDS ledger of the fast MFCC kernel (opensmile_amd/csrc/lld_mfcc512.hip, the layout of its `LDS layout` comment): every
LDS instruction of one steady-state pass of one wave, by class, with the instruction count, the conflict-free LDS-array cycles, the
conflict cycles of the bank model and, for stores, the cycles of the register transfer that sets a store's cost.

Bank rules of the gfx950 LDS: 64 banks of 4 bytes; a wave's access is served in fixed lane groups, one array cycle per group when
conflict-free, one more for every further distinct address on a busy bank (identical addresses broadcast):
  ds_read_b32 / ds_write_b32   2 groups of 32 lanes, bank (a/4) mod 32    array 2    store transfer 4 (address + 1 dword, 2 cycles each)
  ds_read_b64                  2 groups of 32 lanes, bank (a/4) mod 64    array 2
  ds_write_b64                 4 groups of 16 lanes, bank (a/4) mod 32    array 4    store transfer 6
  ds_read_b128                 4 groups of 16 lanes {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31}, + 32; bank (a/4) mod 64    array 4
  ds_bpermute_b32              taken as a ds_read_b32 without bank access (the crossbar alone): array 2, no conflicts -- an assumption
A store conflict costs time only once array + conflict cycles exceed the transfer: `busy` = max(transfer, array + conflicts).

The layout constants and the table layouts are parameters (`Layout`). `parent_layout` is the layout before the band vectors were
moved apart (kLmelFloats = 64), `tree_layout` the kernel source's, and `lane_major_layout` a candidate that was built, measured and
NOT taken (profiles/lds_layout_ab.txt): the loop-invariant tables of (x, y) pairs -- tw512, window, tw256 -- lane-major,
one row per lane j [tw512 8 pairs | window MP pairs, padded to an even count | tw256 16 pairs, pair k1 = q + 4 p at 4 q + (p + 3) % 4],
read two pairs at a time with ds_read_b128: 19 reads per pass at MP = 13 in place of 36 ds_read_b64. A b128 lane group holds every
j = 0 .. 15 once, so those reads are conflict-free iff a row is an odd number of bank quads long (76 floats at MP = 13, 84 at MP = 16).
`python tools/lds_bank_sim.py` prints the three ledgers for the bench's instance lld_mfcc512<13, true, true, true, false, 6, true>.

`column_map`: the instances with the one-hop untangle exchange (the kernel's one_hop_exchange(): all but the PLP chain and MP = 16
with the regression stages fused) deal the columns of the second DFT16 to the lanes by KC = 0 .. 7, 9 .. 15, 8; the transposition's
loads, the tw512 reads and the power buffer's stores go by it. `tree_layout` carries it; the figures do not move.

The mel units' octets are the host's choice (fast512_build_host orders every lane's units so that the 16 lanes of a frame touch 16
different bank quads). BENCH_OCTETS is that table for the bench configuration (26 bands, six units per lane), dumped once by the
library itself: SMILEHIP_DEBUG_TABLES=1 prints it, with the builder's own conflict count, when a plan is created (`library_tables`
reruns that on the host; no GPU). The builder counts one set of 16 lanes per step; a ds_read_b128 lane group holds eight lanes each of
two frame groups, whose buffers start on the same bank and who read the same octets, so every one of the four lane groups and both
reads of a unit pay the builder's figure: ledger conflict cycles = 4 x 2 x the builder's.

The transposition is modelled per instruction and in issue order (`transposition`): an instruction's lane -> bank pattern depends
on its own row / column index only, so the ORDER in which the sixteen stores and the sixteen loads are issued cannot change the
conflict count -- the function checks that and returns the count for any order (since round 8 the stores are issued in the order of
the first DFT's last layer, TRANSPOSE_ORDER_R8; the loads in that order too were measured and are no gain; before
round 8 both were issued in index order).

`split_layout`: the kernel's SPLIT-COMPLEX transposition buffer (its split_transpose() instances: all but the PLP chain and MP = 16
with the regression stages fused, the rule of one_hop_exchange(); those keep the interleaved buffer of `tree_layout`, which is also
what the split form was measured against). A plane of real and a plane of
imaginary parts, a row = the 64 floats the 64 lanes hold for one index k1, at TSPLIT row base + lane:
  ds_write_addtid_b32          address = M0 + immediate + 4 x lane, no address register: banked as a ds_write_b32 (2 groups of 32
                               consecutive dwords: never a conflict), array 2, store transfer 2 (one data dword)
Two of them per index (32 per pass), and the reader -- lane (g, kc) takes columns 0 .. 15 of row kc of its group -- four ds_read_b128
per plane. A b128 lane group mixes lanes j = 0 .. 3, 12 .. 15 of one frame group with j = 4 .. 11 of the next, so the row bases are a
table (`tsplit_base`, the kernel's function of the same name): four rows (re A | re B | im A | im B) on each of the bank quads 0, 1,
2, 3, 8, 9, 10, 11, 2048 + 44 floats per wave. The per-wave regions of these instances come first in the block's LDS (M0 holds 16 bits
of byte address), the shared tables behind them."""
import os
import re
import subprocess
import sys
from dataclasses import dataclass

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MP, UC = 13, 6                       # the bench's instance
K_TB2_ROW = 65                       # float2 per 4-group row of the transpose buffer
K_LMEL, K_OCTET, K_PB, K_WAVE = 68, 12, 448, 2080
K_TS_WAVE = 2092                     # per-wave LDS of the split-complex instances (kTSWaveFloats)

TRANSPOSE_ORDER_PARENT = list(range(16))
TRANSPOSE_ORDER_R8 = [q + 4 * p for q in range(4) for p in range(4)]       # 0, 4, 8, 12 | 1, 5, 9, 13 | ...

# [step i][lane j] -> octet of the unit (padding units included), bench configuration: 26 bands, 83 units on 15 lanes, 6 per lane
BENCH_OCTETS = None                  # filled below (kept at the end of the file: 96 numbers)
BENCH_BUILDER_EXTRA = 2              # "bank model: 2 extra cycles over 6 steps" of the same dump


@dataclass(frozen=True)
class Layout:
    mp: int = MP
    uc: int = UC
    k_lmel: int = K_LMEL
    k_octet: int = K_OCTET
    k_pb: int = K_PB
    k_wave: int = K_WAVE
    k_tb2_row: int = None            # None: the module's K_TB2_ROW at the time of the call
    lane_major: bool = False         # the tables of pairs: one row per lane (tw512 | window | tw256), read 16 bytes at a time
    column_map: bool = False         # lane j transforms column KC[j] of the second DFT16 (the one-hop untangle exchange)
    tab_row: int = None              # floats per lane-major row; None: the smallest odd number of bank quads that holds a row
    split: bool = False              # the split-complex transposition buffer; the per-wave regions in front of the shared tables
    plp: bool = False                # (only the column map of the split form depends on it)

    # ---- the shared tables in front of the per-wave regions (float offsets)
    @property
    def win_floats(self):
        return 2 * ((self.mp + 1) & ~1)

    @property
    def row(self):
        if self.tab_row is not None:
            return self.tab_row
        f = 16 + self.win_floats + 32
        return f if f % 8 == 4 else f + 4

    @property
    def pairs_floats(self):
        return 16 * self.row if self.lane_major else 256 * 2 + self.mp * 16 * 2 + 256 * 2

    @property
    def off_melw0(self):
        return self.pairs_floats

    @property
    def off_melw1(self):
        return self.off_melw0 + self.uc * 64

    @property
    def off_dct(self):
        return self.off_melw1 + self.uc * 64

    @property
    def shared(self):
        return self.pairs_floats + self.uc * 16 * 8 + 16 * 28 + 48

    @property
    def tb2_row(self):
        return K_TB2_ROW if self.k_tb2_row is None else self.k_tb2_row


def one_hop_exchange(mp, plp=False, delta=True):
    """the kernel's rule of the same name: which instances deal the columns by KC"""
    return not plp and not (mp == 16 and delta)


def tree_layout(mp=MP, uc=UC, delta=True):
    return Layout(mp=mp, uc=uc, column_map=one_hop_exchange(mp, delta=delta))


def split_transpose(mp, plp=False, delta=True):
    """the kernel's rule of the same name: which instances move the transposition through the split-complex buffer"""
    return not plp and not (mp == 16 and delta)


def split_layout(mp=MP, uc=UC, delta=True, plp=False):
    """(for any instance: the row table serves both lane -> column maps)"""
    return Layout(mp=mp, uc=uc, k_wave=K_TS_WAVE, column_map=one_hop_exchange(mp, plp, delta), split=True, plp=plp)


def tsplit_base(r, imag=False):
    """float offset of row r (index k1 of the stores, column kc of the loads) in the wave's region: the kernel's tsplit_base. Slot
    s = 0 .. 7 stands on bank quad 0, 1, 2, 3, 8, 9, 10, 11 and holds four rows of 64 floats: re, im of one of the rows 0 .. 3,
    12 .. 15 and re, im of one of the rows 4 .. 11. One table for both lane -> column maps: lanes j = 0 .. 3, 12 .. 15 read rows 0 .. 3,
    12 .. 15 (kc = j) or 0 .. 3, 13, 14, 15, 8 (KC), and either set meets every slot once."""
    s = r if r < 4 else (r - 4 if r < 12 else r - 8)
    b = 4 <= r < 12
    return 256 * s + 4 * (s if s < 4 else s + 4) + (64 if b else 0) + (128 if imag else 0)


def parent_layout(mp=MP, uc=UC):
    return Layout(mp=mp, uc=uc, k_lmel=64)


def lane_major_layout(mp=MP, uc=UC, **kw):
    return Layout(mp=mp, uc=uc, lane_major=True, **kw)


def groups(kind):
    if kind in ("r32", "w32", "r64", "wtid"):
        return [list(range(0, 32)), list(range(32, 64))]
    if kind in ("w64", "r2_64"):
        return [list(range(16 * i, 16 * i + 16)) for i in range(4)]
    if kind == "r128":
        return [[0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27],
                [4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31],
                [32, 33, 34, 35, 44, 45, 46, 47, 52, 53, 54, 55, 56, 57, 58, 59],
                [36, 37, 38, 39, 40, 41, 42, 43, 48, 49, 50, 51, 60, 61, 62, 63]]
    raise ValueError(kind)


ARRAY_CYCLES = {"r32": 2, "w32": 2, "r64": 2, "w64": 4, "r128": 4, "bperm": 2, "wtid": 2}
TRANSFER_CYCLES = {"w32": 4, "w64": 6, "wtid": 2}


def cost(kind, addr_bytes, active=None):
    """extra cycles beyond the conflict-free cost for one wave instruction"""
    nb = {"r32": 32, "w32": 32, "wtid": 32, "w64": 32, "r2_64": 32, "r64": 64, "r128": 64}[kind]
    width = {"r32": 1, "w32": 1, "wtid": 1, "w64": 2, "r2_64": 2, "r64": 2, "r128": 4}[kind]
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
# The column of the second DFT16 that lane j transforms under the map: 0 .. 7, 9 .. 15, 8 -- lanes i and 15 - i hold the partner
# columns i and 16 - i (row_mirror), lane 15 the self-paired column 8, lane 0 the self-paired column 0. A permutation of the 16 lanes
# of a frame group, and every lane group of the instructions it touches (the transposition's ds_read_b64, the tw512 ds_read_b64, the
# power buffer's ds_write_b32: 32 lanes each) holds whole frame groups: the address multiset of a lane group is the one without the
# map, so is every figure of the ledger (tests/test_lds_ledger_column_map.py).
KC = np.where(j < 8, j, np.where(j == 15, 8, j + 1))


def column(layout):
    return KC if layout.column_map else j


def wave_base(wave=0, layout=None):
    layout = layout or tree_layout()
    return wave * layout.k_wave if layout.split else layout.shared + wave * layout.k_wave


def table_base(layout):
    """float offset of the shared tables"""
    return 8 * layout.k_wave if layout.split else 0


def transposition_split(wave=0, layout=None, base=tsplit_base):
    """The split-complex buffer: per index k1 two ds_write_addtid_b32 (row k1 of the real and of the imaginary plane, address = wave
    region + row base + lane) and per plane four ds_read_b128 (lane (g, kc): row base of kc + 16 g + 4 i) -> (extra cycles of the 32
    stores, of the 8 loads). `base`: the row-base table (another one shows that the model sees it)."""
    layout = layout or split_layout()
    wb, kc = wave_base(wave, layout), column(layout)
    st = sum(cost("wtid", 4 * (wb + base(k1, im) + lane)) for k1 in range(16) for im in (False, True))
    rd = np.array([base(int(c)) for c in kc])
    ld = sum(cost("r128", 4 * (wb + rd + 16 * g + 4 * i + (128 if im else 0))) for im in (False, True) for i in range(4))
    return st, ld


def transposition(store_order=TRANSPOSE_ORDER_R8, load_order=TRANSPOSE_ORDER_R8, wave=0, layout=None):
    """The 16 ds_write_b64 (row k1 of group g: float2 index g*16 + j + k1*65) and the 16 ds_read_b64 (column jj: g*16 + kc*65 + jj,
    kc = the lane's column: j, or KC[j] under the layout's column map) in the given issue orders -> (extra cycles of the stores, of the loads, order_independent). `order_independent`: every
    instruction has the conflict count it has in index order (its addresses do not depend on its position)."""
    assert sorted(store_order) == list(range(16)) and sorted(load_order) == list(range(16))
    layout = layout or tree_layout()
    wb, row, kc = wave_base(wave, layout), layout.tb2_row, column(layout)
    st = {k1: cost("w64", 4 * wb + 8 * (g * 16 + j + k1 * row)) for k1 in range(16)}
    ld = {jj: cost("r64", 4 * wb + 8 * (g * 16 + kc * row + jj)) for jj in range(16)}
    st_seq = [cost("w64", 4 * wb + 8 * (g * 16 + j + k1 * row)) for k1 in store_order]
    ld_seq = [cost("r64", 4 * wb + 8 * (g * 16 + kc * row + jj)) for jj in load_order]
    same = st_seq == [st[k] for k in store_order] and ld_seq == [ld[k] for k in load_order]
    return sum(st_seq), sum(ld_seq), same


def pb_pos(k, k_octet=K_OCTET):
    return k + (k_octet - 8) * (k >> 3)


def tw256_pos(k1):
    return 4 * (k1 & 3) + (((k1 >> 2) + 3) & 3)


class Ledger:
    """rows: class -> [instructions, conflict-free array cycles, conflict cycles, store transfer cycles, instructions by kind]"""

    def __init__(self):
        self.rows = {}

    def add(self, name, kind, conflicts, n=1):
        r = self.rows.setdefault(name, [0, 0, 0, 0, {}])
        r[0] += n
        r[1] += n * ARRAY_CYCLES[kind]
        r[2] += conflicts
        r[3] += n * TRANSFER_CYCLES.get(kind, 0)
        r[4][kind] = r[4].get(kind, 0) + n

    def count(self, name):
        return self.rows[name][0]

    def kinds(self, name):
        return dict(self.rows[name][4])

    def conflicts(self, name):
        return self.rows[name][2]

    def array(self, name):
        return self.rows[name][1]

    def transfer(self, name):
        return self.rows[name][3]

    def busy(self, name):
        return max(self.transfer(name), self.array(name) + self.conflicts(name))

    def totals(self):
        names = list(self.rows)
        return {"instructions": sum(self.count(n) for n in names), "array": sum(self.array(n) for n in names),
                "conflicts": sum(self.conflicts(n) for n in names), "transfer": sum(self.transfer(n) for n in names),
                "busy": sum(self.busy(n) for n in names)}


WINDOW, TW256, TR_WRITE, TR_READ, TW512 = "window read", "tw256 read", "transpose write b64", "transpose read b64", "tw512 read"
TR_WRITE_SPLIT, TR_READ_SPLIT = "transpose write addtid b32", "transpose read b128"
POWER_WRITE, MEL_POWER, MEL_WEIGHT = "power write b32", "mel power read b128", "mel weight read b128"
BAND_WRITE, LMEL_READ, DCT_READ, BPERMUTE = "band vector write b32", "log-mel read b128", "dct read b128", "regression ds_bpermute"


def ledger(layout=None, wave=0, octets=None, n_mfcc=13, n_bands=26, delta=True):
    """One steady-state pass of one wave of the MFCC chain (no PLP stage). `octets`: [uc][16] unit octets (default: the bench's table
    when the layout has its six units per lane, else octet = lane, a conflict-free stand-in)."""
    L = layout or tree_layout()
    led = Ledger()
    wb = wave_base(wave, L)
    kc = column(L)                              # the lane's bins kc + 16 q: their twiddles and their places in the power buffer
    tb = table_base(L)
    lmel = wb + g * L.k_lmel
    pb = wb + 4 * L.k_lmel + g * L.k_pb
    if octets is None:
        octets = BENCH_OCTETS if L.uc == 6 else [list(range(16))] * L.uc
    octets = np.asarray(octets).reshape(L.uc, 16)
    if delta:                                   # delta_fast: s1, s3, d1, d3, drow -- the crossbar, no bank
        led.add(BPERMUTE, "bperm", 0, 5)
    if L.lane_major:
        tab = tb + L.row * j                    # float offset of lane j's row: tw512 [16] | window | tw256 [32]
        # (a read whose second pair is never used -- the window's last at an odd MP, group 0's second of tw256, which ends in the
        # pair k1 = 0 -- is narrowed by the compiler to a ds_read_b64 of its first pair)
        for i in range((L.mp + 1) // 2):
            kind = "r64" if 2 * i + 1 >= L.mp else "r128"
            led.add(WINDOW, kind, cost(kind, 4 * (tab + 16 + 4 * i)))
        for i in range(8):
            kind = "r64" if i == 1 else "r128"
            led.add(TW256, kind, cost(kind, 4 * (tab + 16 + L.win_floats + 4 * i)))
    else:
        off_win, off_tw256 = tb + 512, tb + 512 + L.mp * 32
        for m in range(L.mp):
            led.add(WINDOW, "r64", cost("r64", 4 * (off_win + 2 * (m * 16 + j))))
        for k1 in range(1, 16):
            led.add(TW256, "r64", cost("r64", 4 * (off_tw256 + 2 * (k1 * 16 + j))))
    if L.split:
        s, l = transposition_split(wave=wave, layout=L)
        led.add(TR_WRITE_SPLIT, "wtid", s, 32)
        led.add(TR_READ_SPLIT, "r128", l, 8)
    else:
        s, l, _ = transposition(wave=wave, layout=L)
        led.add(TR_WRITE, "w64", s, 16)
        led.add(TR_READ, "r64", l, 16)
    if L.lane_major:
        for i in range(4):
            led.add(TW512, "r128", cost("r128", 4 * (tb + L.row * j + 4 * i)))
    else:
        for q in range(8):
            led.add(TW512, "r64", cost("r64", 4 * (tb + 2 * (kc + 16 * q))))
    for q in range(8):
        led.add(POWER_WRITE, "w32", cost("w32", 4 * (pb + pb_pos(kc, L.k_octet) + 2 * L.k_octet * q)))
        led.add(POWER_WRITE, "w32", cost("w32", 4 * (pb + pb_pos(256 - kc, L.k_octet) - 2 * L.k_octet * q)))
    led.add(POWER_WRITE, "w32", cost("w32", 4 * (pb + pb_pos(128, L.k_octet)), j == 0))                       # bin 128
    led.add(POWER_WRITE, "w32", cost("w32", 4 * (pb + pb_pos(256, L.k_octet) + j), (j > 0) & (j < 8)))        # octet 32's zeros
    for i in range(L.uc):
        a = pb + L.k_octet * octets[i][j]
        led.add(MEL_POWER, "r128", cost("r128", 4 * a) + cost("r128", 4 * (a + 4)), 2)
        led.add(MEL_WEIGHT, "r128", cost("r128", 4 * (tb + L.off_melw0 + 4 * (i * 16 + j))) + cost("r128", 4 * (tb + L.off_melw1 + 4 * (i * 16 + j))), 2)
    # the lane's two bands (each lane owns other bands: 16 different dwords of 32 per frame group) and the pads up to 32
    led.add(BAND_WRITE, "w32", cost("w32", 4 * (lmel + j)))
    led.add(BAND_WRITE, "w32", cost("w32", 4 * (lmel + 16 + j), j + 16 < n_bands))
    led.add(BAND_WRITE, "w32", cost("w32", 4 * (lmel + 16 + j), j + 16 >= n_bands))
    led.add(BAND_WRITE, "w32", cost("w32", 4 * (lmel + j), j >= n_bands))
    act = j < n_mfcc
    for q in range(7):
        led.add(LMEL_READ, "r128", cost("r128", 4 * (lmel + 4 * q), act))
        led.add(DCT_READ, "r128", cost("r128", 4 * (tb + L.off_dct + j * 28 + 4 * q), act))
    return led


def model(wave=0, layout=None):
    """class -> conflict cycles of one pass (the ledger's conflict column)"""
    led = ledger(layout, wave)
    return {name: led.conflicts(name) for name in led.rows}


def kernel_loop_bounds(src=None):
    """The counts the kernel source gives for the classes whose number is a loop bound or a template parameter: window reads per MP
    (one per m), tw256 reads (three in front of the DFT, four in front of each of three groups), the transposition's stores and
    loads, the tw512 reads, the reads of a mel unit. Parsed from lld_mfcc512.hip."""
    if src is None:
        src = open(os.path.join(ROOT, "opensmile_amd", "csrc", "lld_mfcc512.hip")).read()
    out = {}
    out["window_reads_per_m"] = len(re.findall(r"const float2 w = s_win\[m \* 16 \+ j\];", src))
    m = re.search(r"for \(int p = (\d+); p < (\d+); \+\+p\) w\[p\] = s_tw256\[\(4 \* p\) \* 16 \+ j\];", src)
    first = int(m.group(2)) - int(m.group(1))
    m = re.search(r"for \(int q = 0; q < (\d+); \+\+q\) \{\s*if \(q < (\d+)\) \{\s*#pragma unroll\s*for \(int p = 0; p < (\d+); \+\+p\) wn\[p\] = s_tw256", src)
    out["tw256_reads"] = first + int(m.group(2)) * int(m.group(3))
    out["transpose_write"] = int(m.group(1)) * int(re.search(r"dft16_last\(re, im, q\);\s*#pragma unroll\s*for \(int p = 0; p < (\d+); \+\+p\) \{", src).group(1))
    out["transpose_read"] = int(re.search(r"for \(int jj = 0; jj < (\d+); \+\+jj\) \{\s*// one ds_read_b64 each", src).group(1))
    out["tw512_reads"] = int(re.search(r"for \(int q = 0; q < (\d+); \+\+q\) tw5\[q\] = s_tw512\[kc \+ 16 \* q\];", src).group(1))
    out["mel_reads_per_unit"] = 4 if "const float4 p0 = pp[0], p1 = pp[1];" in src and "w0 = s_melw0[i * 16 + j], w1 = s_melw1[i * 16 + j];" in src else None
    return out


def library_tables(n_bands=26, frame_size_sec=None):
    """(octets [uc][16], the builder's own extra cycles per step set) from the library's SMILEHIP_DEBUG_TABLES dump of a host-only
    plan, in a process of its own (the dump goes to stderr)."""
    code = ("import sys; sys.path.insert(0, %r)\nfrom opensmile_amd import capi\ncfg = capi.mfcc12_0_d_a_config()\ncfg.n_bands = %d\n"
            % (ROOT, n_bands))
    if frame_size_sec is not None:
        code += "cfg.frame_size_sec = %r\n" % frame_size_sec
    code += "capi.Plan(None, cfg).close()\n"
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, SMILEHIP_DEBUG_TABLES="1"), capture_output=True, text=True, check=True)
    m = re.search(r"fast512: \d+ mel units on \d+ lanes, (\d+) per lane, bank model: (\d+) extra cycles", r.stderr)
    o = re.search(r"fast512: unit octets \[step\]\[lane\]:((?: \d+)+)", r.stderr)
    uc = int(m.group(1))
    octets = [int(x) for x in o.group(1).split()]
    assert len(octets) == uc * 16
    return [octets[16 * i:16 * i + 16] for i in range(uc)], int(m.group(2))


def print_ledger(title, led):
    print(title)
    print(f"  {'class':26s} {'instr':>5s} {'array':>6s} {'confl':>6s} {'xfer':>5s} {'busy':>5s}")
    for name in led.rows:
        print(f"  {name:26s} {led.count(name):5d} {led.array(name):6d} {led.conflicts(name):6d} {led.transfer(name):5d} {led.busy(name):5d}")
    t = led.totals()
    print(f"  {'per pass':26s} {t['instructions']:5d} {t['array']:6d} {t['conflicts']:6d} {t['transfer']:5d} {t['busy']:5d}")
    left = {n: led.conflicts(n) for n in led.rows if led.conflicts(n)}
    print("  conflict cycles left, by class:", left if left else "none")
    return t


def main():
    print("columns: instructions | conflict-free LDS-array cycles | conflict cycles | store transfer cycles | busy = max(transfer, array + conflicts)")
    cand = lane_major_layout()
    for title, L in (("parent layout (kLmelFloats 64, tables of pairs [index][lane], ds_read_b64)", parent_layout()),
                     ("interleaved transposition buffer (kLmelFloats %d, tables of pairs [index][lane], ds_read_b64)" % K_LMEL, tree_layout()),
                     ("tree layout: split-complex transposition buffer, address-free stores, ds_read_b128", split_layout()),
                     ("candidate, measured and not taken (kLmelFloats %d, tables of pairs lane-major in rows of %d floats, ds_read_b128)"
                      % (K_LMEL, cand.row), cand)):
        per = [ledger(L, w).totals()["conflicts"] for w in range(8)]
        worst = per.index(max(per))
        led = ledger(L, worst)
        print_ledger(f"{title}; wave {worst} of the block (the worst of the 8)", led)
        print("  conflict cycles per pass of the 8 waves of a block:", per)
        if L.split:
            print("  bytes of LDS per block:", {(mp, uc): 4 * (split_layout(mp, uc).shared + 8 * K_TS_WAVE) for mp in (13, 16) for uc in (6, 8)})
        print(f"  log-mel read b128 extra cycles {led.conflicts(LMEL_READ)}; mel power reads: the ledger's "
              f"{led.conflicts(MEL_POWER)} = 4 lane groups x 2 reads x the builder's own {BENCH_BUILDER_EXTRA} "
              "(SMILEHIP_DEBUG_TABLES: 'bank model: 2 extra cycles over 6 steps')")
    if "--library" in sys.argv:
        octets, extra = library_tables()
        print("library dump:", "equal to BENCH_OCTETS" if octets == BENCH_OCTETS else "DIFFERS from BENCH_OCTETS", "| builder's count", extra)
    for name, order in (("index order (parent)", TRANSPOSE_ORDER_PARENT), ("DFT-layer order (round 8)", TRANSPOSE_ORDER_R8)):
        worst_s = worst_l = 0
        for wave in range(8):
            s, l, same = transposition(order, order, wave)
            assert same
            worst_s, worst_l = max(worst_s, s), max(worst_l, l)
        print(f"transposition, {name}: stores {worst_s}, loads {worst_l} extra cycles (worst of the 8 waves of a block); "
              "the per-instruction lane -> bank pattern does not depend on the issue order")


BENCH_OCTETS = [
    [21, 23, 26, 13, 15,  1,  0,  9, 12,  3,  6,  8, 11,  2,  4, 14],
    [22, 24, 27,  0, 17, 18, 21, 10, 13,  4,  7,  9,  3,  3,  5, 12],
    [23, 25, 28, 17, 16, 20, 22, 11, 14,  5,  8, 10,  2,  3, 13, 15],
    [24, 26, 29, 16, 18, 17, 19, 12, 15,  5,  7, 11,  9,  4,  6, 14],
    [25, 27, 30, 15, 19, 21, 23,  0,  1,  6,  8, 12,  2,  4, 10, 13],
    [26, 28, 31, 14,  0, 19, 20,  1,  2,  7,  9, 13,  1,  6,  5,  8],
]

if __name__ == "__main__":
    main()
