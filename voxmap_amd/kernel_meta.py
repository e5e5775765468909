"""Per-kernel resource metadata of a built library (scratch, registers, spills).

Reads the gfx950 code object out of the library's ``.hip_fatbin`` section
(``llvm-objcopy`` + ``clang-offload-bundler``) and parses its AMDHSA metadata
note (``llvm-readelf --notes``).  ``check()`` is the guard ``build()`` runs:
the render kernels must keep 8 waves/SIMD (<= 64 VGPRs) and must not carry a
KernelArgs-sized private segment -- a pointer phi into the kernel arguments
makes the compiler copy the whole 1.7 KB struct to scratch per thread, which
fails silently (correct frames, ~14 GB of scratch traffic per frame).
It also reads the kernel descriptors: every render kernel must run with
DX10_CLAMP set (descriptor_modes).
DESIGN.md §3 lists the measured budgets.
"""
from __future__ import annotations

import os
import re
import subprocess
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin"
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
FIELDS = ("private_segment_fixed_size", "vgpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count",
          "group_segment_fixed_size")
RENDER_SCRATCH_LIMIT = 256      # bytes per thread: spill slots yes, a KernelArgs copy (~1.7 KB) no
# The counting (STATS) instantiations keep 13 more per-lane counters live through every
# loop.  Held to the frames' 64-VGPR budget they spilled 300-500 VGPRs, and some of them
# then summed wrong shadow_fetches and march counters under frames that were right
# (soft shadows on the literal march; tests/test_shapes_gpu.py).  They are not timed, so
# they carry no occupancy floor (vx_render.h VX_OCC_WAVES): 110-145 VGPRs, no VGPR spill
# and no scratch access, and the guard keeps it so: no scratch instruction in the
# kernel's code (scratch_ops), and a private segment of at most the 20 bytes that the
# compiler reserves, and that nothing reads or writes, when a 128-bit SGPR tuple (a
# buffer descriptor) is spilled to VGPR lanes: the tuple's unused 16-byte slot and the
# register scavenger's word.
STATS_SCRATCH_LIMIT = 20
STATS_SPILL_LIMIT = 0
# VGPR spill slots allowed per EXT mode of a timed (non-STATS) k_render
# instantiation (the modes 0-6 are listed once, as kExt* in csrc/vx_internal.h).
# The rare paths (glass in draw order where panes stack, the stacked
# chain) spill at the 8-wave budget; what must never spill is a
# hot loop -- hot_loop_spills() checks the march and primary loops themselves.
# Each limit is the largest count of the current build plus a small margin
# (round 6, ADVICE r05: EXT 0 17, EXT 1 58, EXT 2 60, EXT 3 65, EXT 4 115,
# EXT 5 13, EXT 6 14 slots, all in tiled instantiations): a change that moves
# one is a change to look at, and the limit moves with it, measured.
# round 6: the sun march with the doom rule (its codes resolved after the
# step loop) reloads a few SGPR / scratch values inside the hard units' step
# loop; measured faster than the spill-free in-loop form on C3, v1 and
# REFLECT_ALL (profiles/r06_ab_doom10_c3.txt), so a handful is allowed there
HOT_LOOP_SPILL_LIMITS = {1: 8, 2: 2, 5: 8}
# (EXT 4, the opt-in LDS-brick mode: 134 slots in its fp32 integer-index instantiation since the host's
# float copies of the dimensions joined the arguments, 130 in the RGBA8 ones; no reshape was tried for a
# mode that is opt-in and measured slower than the default; re-timed, -5.6 %: profiles/uniform_ab.txt)
SPILL_LIMITS = {0: 19, 1: 62, 2: 64, 3: 70, 4: 136, 5: 16, 6: 16}
V1_SCRATCH_LIMIT = 72           # EXT 0's private segment (64 B now): the chain's slots, no KernelArgs copy
RENDER_VGPR_LIMIT = 64          # 8 waves/SIMD
GENERAL_VGPR_LIMIT = 96         # EXT 5/6: 5 waves/SIMD (their own unit, vx_render_e56.hip)


def _tool(name: str) -> str:
    p = os.path.join(LLVM, name)
    return p if os.path.exists(p) else name


def code_objects(lib: str, d: str) -> list[str]:
    """The gfx950 code objects of ``lib``, unbundled into directory ``d``: the
    linker concatenates one offload bundle per HIP translation unit into the
    library's .hip_fatbin section."""
    fb = os.path.join(d, "fb.bin")
    subprocess.run([_tool("llvm-objcopy"), f"--dump-section=.hip_fatbin={fb}", lib, os.path.join(d, "x")],
                   check=True, capture_output=True)
    data = open(fb, "rb").read()
    magic = b"__CLANG_OFFLOAD_BUNDLE__"
    starts = [m.start() for m in re.finditer(re.escape(magic), data)]
    out = []
    for i, s in enumerate(starts):
        part, co = os.path.join(d, f"b{i}.bin"), os.path.join(d, f"co{i}.o")
        with open(part, "wb") as f:
            f.write(data[s:starts[i + 1] if i + 1 < len(starts) else len(data)])
        subprocess.run([_tool("clang-offload-bundler"), "--unbundle", "--type=o", f"--targets={TARGET}",
                        f"--input={part}", f"--output={co}"], check=True, capture_output=True)
        out.append(co)
    return out


def kernels(lib: str) -> dict[str, dict[str, int]]:
    """{mangled kernel name: {field: value}} for every kernel in ``lib``."""
    notes = ""
    with tempfile.TemporaryDirectory() as d:
        for co in code_objects(lib, d):
            notes += subprocess.run([_tool("llvm-readelf"), "--notes", co], check=True, capture_output=True,
                                    text=True).stdout
    # one YAML list item per kernel ("- .agpr_count: ..."), keys in alphabetical
    # order, so .group_segment_fixed_size precedes .name within the item
    out: dict[str, dict[str, int]] = {}
    blocks, cur = [], None
    for line in notes.splitlines():
        if re.match(r"\s+- \.", line):
            cur = {}
            blocks.append(cur)
        if cur is None:
            continue
        m = re.match(r"\s+(?:- )?\.name:\s+(\S+)$", line)
        if m:
            cur["__name"] = m.group(1)
            continue
        m = re.match(r"\s+(?:- )?\.(\w+):\s+(\d+)$", line)
        if m and m.group(1) in FIELDS:
            cur[m.group(1)] = int(m.group(2))
    for b in blocks:
        name = b.pop("__name", None)
        if name and "private_segment_fixed_size" in b:
            out[name] = b
    return out


def descriptor_modes(lib: str) -> dict[str, dict[str, int]]:
    """{mangled kernel name: {"dx10_clamp": 0/1, "ieee_mode": 0/1}} from the kernel
    descriptors (the ``<kernel>.kd`` objects in .rodata, which llvm-objdump prints
    as .amdhsa_* directives).  DX10_CLAMP is what makes the clamp output modifier
    take a NaN to 0: vx_math.h's clamp01 relies on it."""
    out: dict[str, dict[str, int]] = {}
    with tempfile.TemporaryDirectory() as d:
        for co in code_objects(lib, d):
            txt = subprocess.run([_tool("llvm-objdump"), "-d", "-j", ".rodata", co], check=True,
                                 capture_output=True, text=True).stdout
            cur = None
            for line in txt.splitlines():
                m = re.match(r"\.amdhsa_kernel\s+(\S+)", line)
                if m:
                    cur = out.setdefault(m.group(1), {})
                    continue
                m = re.match(r"\s+\.amdhsa_(dx10_clamp|ieee_mode)\s+(\d+)", line)
                if m and cur is not None:
                    cur[m.group(1)] = int(m.group(2))
    return out


def render_params(name: str):
    """(FMT, STATS, TILED, EXT, F32IDX) of a mangled k_render instantiation, else None."""
    m = re.search(r"k_render(?:_gen)?ILi(\d)ELb(\d)ELb(\d)ELi(\d)ELb(\d)E", name)
    return tuple(int(g) for g in m.groups()) if m else None


def hot_loop_spills(lib: str, ext_max: int = 6) -> dict[tuple, tuple[int, int]]:
    """(hot loops, spill instructions inside them) of each render kernel that
    renders frames (RGBA8, no stats, EXT <= ext_max).  Spill instructions: scratch_*,
    v_writelane, v_readlane.  Hot loops: the loops of the kernel's main body
    (before its first s_endpgm; the compiler places the rare paths after it)
    that are innermost, at most 400 instructions long, and hold a march texel
    load (buffer_load_format_x) or the primary walk's extent decode
    (v_cvt_f32_ubyte1): the step loops."""
    out: dict[tuple, tuple[int, int]] = {}
    with tempfile.TemporaryDirectory() as d:
        for co in code_objects(lib, d):
            txt = subprocess.run([_tool("llvm-objdump"), "-d", "--no-show-raw-insn", co], check=True,
                                 capture_output=True, text=True).stdout
            name, body = None, []
            for line in txt.splitlines() + ["0 <END>:"]:
                m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
                if m:
                    p = render_params(name) if name else None
                    if p and p[0] == 1 and p[1] == 0 and p[3] <= ext_max:
                        out[p] = _hot_spills(body)
                    name, body = m.group(1), []
                elif name and "//" in line:
                    ins, cmt = line.split("//", 1)
                    am = re.match(r"\s*([0-9A-Fa-f]+):", cmt)
                    if am:
                        body.append((int(am.group(1), 16), ins.strip()))
    return out


def _hot_spills(body: list[tuple[int, str]]) -> tuple[int, int]:
    end = next((i for i, (_, l) in enumerate(body) if l.startswith("s_endpgm")), len(body))
    body = body[:end]
    index = {a: i for i, (a, _) in enumerate(body)}
    spill = [bool(re.match(r"(scratch_|v_writelane|v_readlane)", l)) for _, l in body]
    hot = [bool(re.match(r"(buffer_load_format_x\s|v_cvt_f32_ubyte1)", l)) for _, l in body]
    back = []                                             # backward branches: (loop head, latch)
    for i, (a, l) in enumerate(body):
        m = re.match(r"s_(?:cbranch_\w+|branch)\s+(\d+)", l)
        if not m:
            continue
        off = int(m.group(1))
        off = off - 65536 if off >= 32768 else off        # simm16, printed unsigned
        tgt = index.get(a + 4 + 4 * off)                  # SOPP branch: PC + 4 + 4 * simm16
        if tgt is not None and tgt < i:
            back.append((tgt, i))
    loops = n = 0
    for h, e in back:                                     # innermost loops: the step loops themselves
        if (e - h > 400 or any(h <= h2 and e2 <= e and (h2, e2) != (h, e) for h2, e2 in back)
                or not any(hot[h:e + 1])):
            continue
        loops += 1
        n = max(n, sum(spill[h:e + 1]))
    return loops, n


# ---- wave-uniform work on the vector unit (tools/isa_uniform.py prints the listing) ----
# gfx950 has no scalar float unit: a float convert or compare of kernel arguments
# runs on the vector unit, once per wave, at a quarter-rate price, for a result
# that is the same for the whole frame -- the host passes such values instead
# (KernelArgs::Xf .., FrameConsts::sun_down, ::sun_sg).  Two counts per kernel:
#   uniform  VALU instructions none of whose source operands is a vector
#            register (SGPRs, literals and inline constants only).  Not counted:
#            moves and lane moves (v_mov, v_readlane, v_writelane,
#            v_readfirstlane, v_accvgpr), v_mbcnt (the lane id), v_nop, and
#            v_cndmask, whose SGPR-pair condition is a lane mask as a rule;
#   kernarg  global loads whose address derives from the kernel-argument
#            pointer (a per-lane index into a table inside KernelArgs).
# Per EXT mode, the largest counts over the timed (non-STATS) k_render
# instantiations of the current build: what is left is listed in
# profiles/uniform_valu_after.txt and explained line by line in DESIGN.md §3
# "Round 8" (the slab tests of primary()'s general branch, 2 * cloudTime, face_key's
# division by CHUNK, the tile prologue's divisions, the soft loops' sample count).
# A change that moves one is a change to look at, and the limit moves with it.
UNIFORM_VALU_LIMITS: dict[int, tuple[int, int]] = {0: (19, 6), 1: (21, 10), 2: (49, 14), 3: (51, 14), 4: (50, 22),
                                                   5: (21, 10), 6: (49, 10)}
_UNIFORM_SKIP = ("v_mov_", "v_readlane", "v_writelane", "v_readfirstlane", "v_accvgpr", "v_mbcnt", "v_nop", "v_cndmask",
                 "v_swap")
_VREG = re.compile(r"(?<![\w.])[va](?:\d+|\[\d+:\d+\])")
_REG = re.compile(r"(?<![\w.])([sv])(?:(\d+)|\[(\d+):(\d+)\])")


def _regs(text: str) -> set[tuple[str, int]]:
    out = set()
    for kind, one, lo, hi in _REG.findall(text):
        out.update((kind, i) for i in (range(int(lo), int(hi) + 1) if lo else (int(one),)))
    return out


def asm_kernels(text: str) -> dict[str, list[str]]:
    """{symbol: [instruction, ...]} of compiler assembly (hipcc -S: ``name:`` labels,
    ``;`` comments) or of a disassembly (llvm-objdump -d: ``<name>:`` headers,
    ``//`` comments): mnemonic and operands, comments and directives dropped."""
    out: dict[str, list[str]] = {}
    cur = None
    for line in text.splitlines():
        m = re.match(r"^(?:[0-9a-f]+ <(\S+)>:|([A-Za-z_][\w$.]*):)\s*(?:;.*)?$", line)
        if m:
            cur = out.setdefault(m.group(1) or m.group(2), [])     # (basic-block labels start with a dot)
            continue
        ins = re.split(r";|//", line, 1)[0].strip()
        if cur is not None and ins and re.match(r"[a-z]+_\w+", ins):
            cur.append(ins)
    return out


def uniform_scan(body: list[str]) -> tuple[list[str], list[str]]:
    """(uniform VALU instructions, kernarg-derived global loads) of one kernel's
    instructions, in program order.  The kernel-argument pointer is the base of the
    kernel's first s_load; what is computed from it (scalar or vector adds, spills
    to and from lanes) is followed in program order, not along the control flow."""
    uniform, kload = [], []
    karg: set = set()                     # registers (and (vgpr, lane) spill slots) holding a kernarg address
    seeded = False
    for ins in body:
        op, _, rest = ins.partition(" ")
        ops = [o.strip() for o in re.split(r",(?![^\[]*\])", rest)] if rest.strip() else []
        if not seeded and op.startswith("s_load_") and len(ops) >= 2:
            karg |= _regs(ops[1])
            seeded = True
        if op.startswith("v_") and not op.startswith(_UNIFORM_SKIP) and len(ops) >= 2:
            if not any(_VREG.search(o) for o in ops[1:]):
                uniform.append(ins)
        if op.startswith("global_load_") and len(ops) >= 2 and any(r in karg for o in ops[1:] for r in _regs(o)):
            kload.append(ins)
        if not ops:
            continue
        # follow the address: destination tainted iff a source is (loads return data, not addresses)
        dst = _regs(ops[0])
        if op.startswith("v_writelane") and len(ops) == 3:
            slot = (ops[0], ops[2])
            (karg.add if _regs(ops[1]) & karg else karg.discard)(slot)
            continue
        if op.startswith("v_readlane") and len(ops) == 3:
            src = (ops[1], ops[2]) in karg
        elif op.startswith(("s_load", "global_load", "buffer_load", "scratch_load", "ds_read", "s_waitcnt", "s_cbranch",
                            "s_branch", "global_store", "scratch_store", "buffer_store", "ds_write", "s_cmp", "v_cmp")):
            src = False
            if "store" in op or op.startswith(("ds_write", "s_cmp", "v_cmp", "s_cbranch", "s_branch", "s_waitcnt")):
                continue
        else:
            src = any(r in karg for o in ops[1:] for r in _regs(o))
        for r in dst:
            (karg.add if src else karg.discard)(r)
    return uniform, kload


_BODIES: dict[tuple, dict[str, list[str]]] = {}


def render_bodies(lib: str) -> dict[str, list[str]]:
    """{mangled k_render name: its instructions} from the gfx950 disassembly of ``lib``
    (kept per library file and modification time: two guards read it)."""
    key = (os.path.abspath(lib), os.path.getmtime(lib), os.path.getsize(lib))
    if key not in _BODIES:
        out: dict[str, list[str]] = {}
        with tempfile.TemporaryDirectory() as d:
            for co in code_objects(lib, d):
                txt = subprocess.run([_tool("llvm-objdump"), "-d", "--no-show-raw-insn", co], check=True,
                                     capture_output=True, text=True).stdout
                out.update({n: b for n, b in asm_kernels(txt).items() if render_params(n)})
        _BODIES.clear()
        _BODIES[key] = out
    return _BODIES[key]


def uniform_valu(lib: str, stats: bool = False) -> dict[str, tuple[int, int]]:
    """{mangled k_render name: (uniform VALU instructions, kernarg-derived global loads)} of the
    timed render kernels in ``lib``, with ``stats`` of the counting ones too (uniform_scan over
    the gfx950 disassembly)."""
    return {name: tuple(len(x) for x in uniform_scan(body)) for name, body in render_bodies(lib).items()
            if stats or not render_params(name)[1]}


def scratch_ops(lib: str) -> dict[str, int]:
    """{mangled k_render name: scratch_* instructions in its code} of every render kernel in ``lib``."""
    return {name: sum(1 for i in body if i.startswith("scratch_")) for name, body in render_bodies(lib).items()}


def check_uniform(lib: str) -> list[str]:
    """The UNIFORM_VALU_LIMITS violations of ``lib``'s timed render kernels."""
    bad = []
    for name, (u, k) in sorted(uniform_valu(lib).items()):
        p = render_params(name)
        if p[1] == 1 or p[3] not in UNIFORM_VALU_LIMITS:
            continue
        lu, lk = UNIFORM_VALU_LIMITS[p[3]]
        if u > lu or k > lk:
            bad.append(f"k_render{p}: {u} wave-uniform VALU instructions (limit {lu}), {k} loads indexed into the "
                       f"kernel arguments (limit {lk}): tools/isa_uniform.py lists them")
    return bad


def check(lib: str) -> dict[str, dict[str, int]]:
    """Raise if a render kernel copies its arguments to scratch or loses occupancy."""
    ks = kernels(lib)
    render = {k: v for k, v in ks.items() if "k_render" in k}
    if not render:
        raise RuntimeError(f"{lib}: no k_render kernels found in the gfx950 code object")
    bad = []
    for name, v in render.items():
        p = render_params(name)
        stats = p is not None and p[1] == 1                        # STATS instantiation: counting only
        # EXT 4 (VX_FLAG_SOFT_BRICK, an opt-in experiment): its 8 KB of LDS bricks
        # cap it at 7 waves/SIMD anyway, so the compiler may use 73 VGPRs
        brick = p is not None and p[3] == 4
        lim = STATS_SCRATCH_LIMIT if stats else RENDER_SCRATCH_LIMIT
        if v.get("private_segment_fixed_size", 0) > lim:
            bad.append(f"{name}: private segment {v['private_segment_fixed_size']} B > {lim}")
        # the timed product kernels: v1 and the extensions spill-free, soft shadows a
        # few VGPRs (scratch traffic in the hot path doubled the EXT 1 frame once)
        spill_lim = STATS_SPILL_LIMIT if stats else SPILL_LIMITS.get(p[3]) if p is not None else None
        if spill_lim is not None and v.get("vgpr_spill_count", 0) > spill_lim:
            bad.append(f"{name}: {v['vgpr_spill_count']} VGPRs spilled > {spill_lim}")
        # EXT 5/6 (glass in draw order, REFLECT_ALL): a budget of their own (vx_render_e56.hip, 5 waves/SIMD)
        general = p is not None and p[3] >= 5
        if not stats and v.get("vgpr_count", 0) > (80 if brick else GENERAL_VGPR_LIMIT if general else RENDER_VGPR_LIMIT):
            bad.append(f"{name}: {v['vgpr_count']} VGPRs > {RENDER_VGPR_LIMIT}")
    # clamp01 (vx_math.h) relies on the clamp modifier taking a NaN to 0
    modes = descriptor_modes(lib)
    for name in render:
        if modes.get(name, {}).get("dx10_clamp") != 1:
            bad.append(f"{name}: DX10_CLAMP is not set in the kernel descriptor ({modes.get(name)})")
    # the counting kernels touch no scratch (their private segment, if any, is the unused slot
    # of an SGPR tuple spilled to lanes: STATS_SCRATCH_LIMIT)
    for name, n in scratch_ops(lib).items():
        if render_params(name)[1] == 1 and n:
            bad.append(f"{name}: {n} scratch instructions in a counting (STATS) kernel")
    bad += check_uniform(lib)
    for p, (loops, n) in hot_loop_spills(lib).items():
        if not loops:
            bad.append(f"k_render{p}: no march / primary loop found in the disassembly (check the parser)")
        if n > HOT_LOOP_SPILL_LIMITS.get(p[3] if p else -1, 0):
            bad.append(f"k_render{p}: {n} spill instructions inside a march / primary loop")
    if bad:
        raise RuntimeError("render kernel resource check failed:\n  " + "\n  ".join(bad))
    return ks


if __name__ == "__main__":
    import sys
    lib = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(__file__), "libvoxmap_hip.so")
    for name, v in sorted(kernels(lib).items()):
        print(f"{name[:70]:70s} " + " ".join(f"{f.split('_')[0][:5]}={v.get(f, 0)}" for f in FIELDS))
