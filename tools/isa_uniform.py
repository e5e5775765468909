"""Wave-uniform work on the vector unit, per k_render instantiation.

For a built library (its gfx950 code objects are disassembled) or a compiler
assembly file (hipcc --offload-device-only -S of a vx_render_e<EXT>.hip), lists
per render kernel
  * every VALU instruction none of whose source operands is a vector register
    (SGPRs, literals, inline constants): its result is the same in every lane,
    and where its inputs are kernel arguments, the same for the whole frame --
    the host can pass it (voxmap_amd/kernel_meta.py says what is not counted);
  * every global load whose address derives from the kernel-argument pointer:
    a per-lane index into a table inside KernelArgs.
priced with tools/isa_cost.py's table.  voxmap_amd.kernel_meta.uniform_valu()
returns the two counts, and build() holds them to UNIFORM_VALU_LIMITS.

usage: python tools/isa_uniform.py [--stats] [--counts] [libvoxmap_hip.so | kernel.s ...]
  --stats   the counting (STATS) instantiations too
  --counts  one line per kernel, no listing
"""
import os
import subprocess
import sys
import tempfile
from collections import Counter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from isa_cost import cost  # noqa: E402

from voxmap_amd import kernel_meta as km  # noqa: E402


def texts(path):
    """The assembly texts of ``path``: the file itself, or a library's disassembled code objects."""
    if path.endswith(".s"):
        yield open(path).read()
        return
    with tempfile.TemporaryDirectory() as d:
        for co in km.code_objects(path, d):
            yield subprocess.run([km._tool("llvm-objdump"), "-d", "--no-show-raw-insn", co], check=True,
                                 capture_output=True, text=True).stdout


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    stats, counts = "--stats" in sys.argv, "--counts" in sys.argv
    for path in args or [os.path.join(ROOT, "voxmap_amd", "libvoxmap_hip.so")]:
        rows = []
        for text in texts(path):
            for name, body in km.asm_kernels(text).items():
                p = km.render_params(name)
                if p and (stats or not p[1]):
                    rows.append((p, "_gen" in name, *km.uniform_scan(body)))
        print(f"# {os.path.basename(path)}: k_render<FMT, STATS, TILED, EXT, F32IDX>, wave-uniform VALU instructions "
              f"(priced SIMD-cycles) and loads indexed into the kernel arguments")
        for p, gen, uni, kl in sorted(rows, key=lambda r: (r[0][3], r[0], r[1])):
            cyc = sum(cost(i.split()[0]) for i in uni)
            print(f"k_render{'_gen' if gen else ''}{p}: {len(uni)} uniform VALU ({cyc} cycles), {len(kl)} kernarg loads")
            if counts:
                continue
            for ins, n in sorted(Counter(uni).items(), key=lambda t: (t[0].split()[0], t[0])):
                print(f"    {n:2d} x  {ins}")
            for ins, n in sorted(Counter(kl).items()):
                print(f"    {n:2d} x  {ins}    <- kernarg")


if __name__ == "__main__":
    main()
