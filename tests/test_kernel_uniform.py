"""Wave-uniform work on the vector unit (voxmap_amd/kernel_meta.py: uniform_scan, UNIFORM_VALU_LIMITS;
tools/isa_uniform.py prints the listing): the parser on a committed snippet of assembly whose every line is
there for a reason, in the compiler's syntax and in the disassembler's; the limits table against the built
library, for every timed (non-STATS) k_render instantiation."""
import os
import re
import subprocess
import sys

import pytest

from voxmap_amd import kernel_meta

HERE = os.path.dirname(os.path.abspath(__file__))
SNIPPET = os.path.join(HERE, "golden", "uniform_snippet.s")
NAME = "_ZN2vx12_GLOBAL__N_18k_renderILi1ELb0ELb0ELi1ELb1EEEvNS_10KernelArgsE"
# scalar-only sources: the convert of an argument, the compare of one with 0, the sum of two; not the
# convert or compare of a lane's value, not the moves, not v_cndmask (its SGPR pair is a lane mask), not
# the multiply whose operand came through a register
UNIFORM = ["v_cvt_f32_i32_e32 v2, s4", "v_cmp_lt_f32_e64 s[14:15], s10, 0", "v_add_f32_e64 v6, s4, s4"]
# indexed into the arguments: through a 64-bit per-lane address, through an SGPR pair offset from the
# argument pointer, and through that pair after a spill to a lane and back; not the loads through a
# pointer that was itself loaded from the arguments (s[12:13], or s22 reloaded from its lane)
KERNARG = ["global_load_dword v10, v[8:9], off offset:600", "global_load_dword v11, v0, s[8:9]",
           "global_load_dword v16, v[14:15], off"]


def test_snippet_in_compiler_syntax():
    ks = kernel_meta.asm_kernels(open(SNIPPET).read())
    assert list(ks) == [NAME] and kernel_meta.render_params(NAME) == (1, 0, 0, 1, 1)
    body = ks[NAME]
    assert len(body) == 32 and body[0].startswith("s_load_dwordx2") and body[-1] == "s_endpgm"
    uni, kl = kernel_meta.uniform_scan(body)
    assert uni == UNIFORM
    assert kl == KERNARG


def test_snippet_in_disassembler_syntax():
    """The same instructions as llvm-objdump prints them: an address and the symbol in angle brackets, the
    encoding in a // comment."""
    lines = [f"0000000000001900 <{NAME}>:"]
    for i, ins in enumerate(kernel_meta.asm_kernels(open(SNIPPET).read())[NAME]):
        lines.append(f"\t{ins:58s} // {0x1900 + 4 * i:012X}: 7E040A04")
    ks = kernel_meta.asm_kernels("\n".join(["", "lib.o:\tfile format elf64-amdgpu", "", "Disassembly of section .text:", ""]
                                           + lines))
    assert list(ks) == [NAME]
    assert kernel_meta.uniform_scan(ks[NAME]) == (UNIFORM, KERNARG)


def test_tool_lists_the_snippet():
    out = subprocess.run([sys.executable, os.path.join(HERE, "..", "tools", "isa_uniform.py"), SNIPPET],
                         check=True, capture_output=True, text=True).stdout
    assert "k_render(1, 0, 0, 1, 1): 3 uniform VALU (10 cycles), 3 kernarg loads" in out
    for ins in UNIFORM + KERNARG:
        assert ins in out


def test_limits_hold_for_every_timed_render_kernel(built):
    from voxmap_amd import build as vb
    counts = kernel_meta.uniform_valu(vb.OUT)
    params = {n: kernel_meta.render_params(n) for n in counts}         # by name: k_render and k_render_gen
    assert not any(p[1] for p in params.values())
    assert {p[3] for p in params.values()} == set(kernel_meta.UNIFORM_VALU_LIMITS) == set(range(7))
    assert len(counts) >= 40
    for n, (u, k) in sorted(counts.items()):
        lu, lk = kernel_meta.UNIFORM_VALU_LIMITS[params[n][3]]
        assert u <= lu and k <= lk, (n, u, k)
    # the counting kernels touch no scratch
    assert all(n == 0 for name, n in kernel_meta.scratch_ops(vb.OUT).items() if kernel_meta.render_params(name)[1])


def test_a_lower_limit_is_reported(built, monkeypatch):
    from voxmap_amd import build as vb
    monkeypatch.setitem(kernel_meta.UNIFORM_VALU_LIMITS, 1, (0, 0))
    bad = kernel_meta.check_uniform(vb.OUT)
    assert len(bad) == 8 and all(re.match(r"k_render\(\d, 0, \d, 1, \d\): ", b) and "limit 0" in b for b in bad)
