"""Static check of the bench's instance lld_mfcc512<13, true, true, true, false, 6, true> as the compiler builds it (the Makefile's
flags, compiled to assembly by tools/ubench/valu_replay_gen.py; no GPU):

  * M0 -- the base of the transposition's address-free stores -- is written once, at the head of the pass, from a scalar register, one
    wait state in front of the next instruction, and nothing else in the kernel names M0;
  * the pass holds the 32 address-free stores, at the byte offsets of the ledger's row table (tools/lds_bank_sim.py), and behind the
    last of them the 8 ds_read_b128 of the transposition: one address register, the real plane at +0 .. +48, the imaginary plane 512
    bytes on, aligned 4-register destinations;
  * <= 128 VGPRs, no scratch, no static LDS in front of the dynamic block (M0 is an address inside the block);
  * <= 767 vector instructions per steady-state pass (773 before: six additions of a literal zero left the first DFT16, and the
    16-byte loads brought no register moves)."""
import importlib.util
import json
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(name, *path):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, *path))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    """(lines of the kernel's body, (first, last) line of the pass loop, the generator's figures, the kernel descriptor's text)"""
    gen = _load("valu_replay_gen_static", "tools", "ubench", "valu_replay_gen.py")
    out = str(tmp_path_factory.mktemp("mfcc512_static"))
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "ubench", "valu_replay_gen.py"), out], check=True, stdout=subprocess.DEVNULL)
    asm = os.path.join(out, "lld_mfcc512.s")
    body, _ = gen.kernel_body(asm)
    text = open(asm).read()
    i = text.index(".amdhsa_kernel " + gen.KERNEL)
    desc = text[i:text.index(".end_amdhsa_kernel", i)]
    return body, gen.pass_loop(body), json.load(open(os.path.join(out, "valu_replay_info.json"))), desc


def _instructions(lines):
    """(line index, text) of the instruction lines"""
    out = []
    for i, l in enumerate(lines):
        t = l.split(";")[0].strip()
        if t and not t.startswith(".") and not t.endswith(":"):
            out.append((i, t))
    return out


def test_m0_is_written_once_at_the_head_of_the_pass(built):
    body, (lo, hi), _, _ = built
    ins = _instructions(body)
    named = [(i, t) for i, t in ins if re.search(r"\bm0\b", t)]
    assert len(named) == 1, named
    i, t = named[0]
    assert re.fullmatch(r"s_mov_b32 m0, s\d+", t), t
    assert lo < i < hi
    k = [n for n, (ii, _) in enumerate(ins) if ii == i][0]
    assert ins[k + 1][1] == "s_nop 0"                                   # the wait state in front of an LDS instruction that adds the lane number
    first_store = next(ii for ii, tt in ins if tt.startswith("ds_write_addtid_b32"))
    assert i < first_store
    # head of the pass: nothing that addresses the LDS stands between the loop's head and the write (the regression stages' first
    # ds_bpermute do: the crossbar, no address)
    assert not any(tt.startswith("ds_") and not tt.startswith("ds_bpermute_b32") for ii, tt in ins if lo <= ii < i)


def test_transposition_stores_and_loads(built):
    body, (lo, hi), _, _ = built
    sim = _load("lds_bank_sim_static", "tools", "lds_bank_sim.py")
    ins = _instructions(body)
    stores = [(i, t) for i, t in ins if t.startswith("ds_write_addtid_b32")]
    assert len(stores) == 32 and all(lo < i < hi for i, _ in stores)
    offs = []
    for _, t in stores:
        m = re.fullmatch(r"ds_write_addtid_b32 v\d+(?: offset:(\w+))?", t)
        assert m, t
        offs.append(int(m.group(1), 0) if m.group(1) else 0)
    assert sorted(offs) == sorted(4 * sim.tsplit_base(r, im) for r in range(16) for im in (False, True))
    assert not any(t.startswith("ds_write_b64") for i, t in ins if lo < i < hi)       # the interleaved buffer's stores are gone
    # behind the last store: the next eight LDS instructions are the loads
    last = stores[-1][0]
    nxt = [t for i, t in ins if i > last and t.startswith("ds_")][:8]
    regs, loads = set(), []
    for t in nxt:
        m = re.fullmatch(r"ds_read_b128 v\[(\d+):(\d+)\], (v\d+)(?: offset:(\w+))?", t)
        assert m, t
        assert int(m.group(1)) % 4 == 0 and int(m.group(2)) == int(m.group(1)) + 3
        regs.add(m.group(3))
        loads.append(int(m.group(4), 0) if m.group(4) else 0)
    assert len(regs) == 1 and sorted(loads) == [0, 16, 32, 48, 512, 528, 544, 560]


def test_registers_scratch_and_static_lds(built):
    _, _, _, desc = built

    def field(name):
        return int(re.search(r"\.amdhsa_" + name + r"\s+(\d+)", desc).group(1))

    assert field("next_free_vgpr") <= 128
    assert field("private_segment_fixed_size") == 0
    assert field("group_segment_fixed_size") == 0


def test_vector_instructions_per_pass(built):
    body, (lo, hi), info, _ = built
    assert info["valu_in_stream"] <= 767, info["valu_in_stream"]
    loop = _instructions(body[lo:hi + 1])
    assert not any(t.startswith("v_readlane") for _, t in loop)
