"""Before/after static VALU pricing of one render-kernel instantiation, block by
block, with tools/isa_cost.py's cost table.

Each basic block of the kernel gets a signature: VALU instructions, priced
cycles, the cycles of its v_cmp + v_cndmask, and the marker instructions it
holds (typed loads, stores, roots, reciprocals, IEEE-division steps, 64-bit
address arithmetic, converts), which is what tells the regions apart: the AO
block is the one with four 8_8_8_8 typed loads and a root, pack + store the one
with the global store, and so on.  With two files, the blocks whose signature
occurs in one and not in the other are printed: what a change did to the
straight-line regions, leaving out the hundreds of blocks it did not touch.

usage: python tools/isa_table.py FMT,STATS,TILED,EXT,F32IDX before.s [after.s]
  *.s: hipcc <build.py flags, the unit's own included> --offload-device-only -S vx_render_e<EXT>.hip
"""
import re
import sys
from collections import Counter

from isa_cost import cost

MARKS = ("buffer_load_format_xyzw", "buffer_load_format_x", "global_store", "global_load_dword", "v_sqrt", "v_rcp",
         "v_div_scale", "v_ldexp", "v_med3", "v_cvt_f32_ubyte1", "v_cvt_u32_f32", "v_mad_i64", "v_lshl_add_u64")


def kernel_text(path, params):
    tag = "k_renderILi%dELb%dELb%dELi%dELb%dE" % params
    out, on = [], False
    for line in open(path):
        if re.match(r"^_ZN\S*%s\S*:" % tag, line):
            on = True
            continue
        if on and (line.startswith("\t.section") or ".amdhsa_kernel" in line):
            break
        if on:
            out.append(line)
    if not out:
        raise SystemExit(f"{path}: no kernel {tag}")
    return out


def blocks(path, params):
    """[(instr, cycles, select cycles, marks)] of the kernel's basic blocks."""
    out, cur = [], None
    for line in kernel_text(path, params):
        m = re.match(r"^(\.LBB\w+|; %bb\.\d+):?", line)
        if m or cur is None:
            cur = {"n": 0, "cyc": 0, "sel": 0, "marks": Counter()}
            out.append(cur)
            if m:
                continue
        t = line.split()
        if not t or t[0].startswith((";", ".")):
            continue
        op = t[0]
        if op.startswith("v_"):
            cur["n"] += 1
            cur["cyc"] += cost(op)
            if op.startswith(("v_cmp", "v_cndmask")):
                cur["sel"] += cost(op)
        for k in MARKS:
            if op == k or op.startswith(k + "_"):
                cur["marks"][k] += 1
                break
    return [(b["n"], b["cyc"], b["sel"], " ".join(f"{k}:{v}" for k, v in sorted(b["marks"].items()))) for b in out]


def main():
    params = tuple(int(v) for v in sys.argv[1].split(","))
    sets = [Counter(blocks(p, params)) for p in sys.argv[2:4]]
    print(f"k_render<{', '.join(str(p) for p in params)}>: basic blocks as (VALU instr, priced cycles, of which "
          f"v_cmp + v_cndmask, marker instructions)")
    if len(sets) == 1:
        for (n, cyc, sel, marks), k in sorted(sets[0].items()):
            if cyc >= 40:
                print(f"  {k:3d} x  {n:4d} instr {cyc:5d} cycles {sel:4d} select   {marks}")
        return
    for label, a, b in (("only before", sets[0], sets[1]), ("only after", sets[1], sets[0])):
        print(f"{label}:")
        for (n, cyc, sel, marks), k in sorted((a - b).items()):
            if cyc >= 40:                       # (the scheduler reshuffles the small glue blocks)
                print(f"  {k:3d} x  {n:4d} instr {cyc:5d} cycles {sel:4d} select   {marks}")


if __name__ == "__main__":
    main()
