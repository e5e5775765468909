"""The frame's depth and surface planes, the host half (no GPU): the header's
prototype and VX_SURF_* macros, the ctypes mirrors, unpack_surface against
hand-packed words, vx_render_gbuffer's NULL check, and the k_gbuffer kernels'
resources in the built library."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "voxmap.h")).read()


def test_header_carries_the_prototype_and_the_macros():
    flat = " ".join(HEADER.split())
    assert ("int vx_render_gbuffer(vx_scene *scene, const vx_frame_params *p, int w, int h, "
            "const vx_gbuffer_planes *out, int out_on_device, void *stream, vx_query_stats *stats);") in flat
    assert re.search(r"typedef struct vx_gbuffer_planes \{[^}]*float \*depth;[^}]*float \*opaque_depth;[^}]*"
                     r"uint32_t \*surface;[^}]*\} vx_gbuffer_planes;", flat)
    # each macro's shift and mask, as the issue's bit layout states them
    want = {"VX_SURF_N": (0, 3), "VX_SURF_NORMAL": (2, 7), "VX_SURF_COLOR": (8, 0xFF),
            "VX_SURF_OPAQUE_NORMAL": (18, 7), "VX_SURF_OPAQUE_COLOR": (24, 0xFF)}
    for name, (shift, mask) in want.items():
        m = re.search(rf"#define {name}\(word\) (.*)", HEADER)
        assert m, name
        body = m.group(1).replace("(word)", "word")
        got_shift = int(re.search(r">> (\d+)", body).group(1)) if ">>" in body else 0
        got_mask = int(re.search(r"& (0x[0-9a-fA-F]+|\d+)u", body).group(1), 0)
        assert (got_shift, got_mask) == (shift, mask), (name, body)
    assert "#define VX_ABI_VERSION 10" in HEADER and "vx_render_gbuffer" in HEADER.split("#define VX_ABI_VERSION")[0]


def test_struct_sizes_match_the_c_ones(tmp_path):
    """sizeof and offsetof from a C compiler over the header, against the ctypes mirrors."""
    from voxmap_amd import _abi
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "voxmap.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu\\n", sizeof(vx_gbuffer_planes), '
                   'offsetof(vx_gbuffer_planes, depth), offsetof(vx_gbuffer_planes, opaque_depth), '
                   'offsetof(vx_gbuffer_planes, surface), sizeof(vx_query_stats)); return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.run([os.environ.get("CC", "gcc"), f"-I{os.path.join(ROOT, 'include')}", "-o", str(exe), str(src)],
                   check=True, capture_output=True)                  # the oracle's compiler (oracle/Makefile)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    P = _abi.GbufferPlanes
    assert got == [C.sizeof(P), P.depth.offset, P.opaque_depth.offset, P.surface.offset, C.sizeof(_abi.QueryStats)]
    assert [n for n, _ in P._fields_] == ["depth", "opaque_depth", "surface"]


def _pack(n, normal, color, onormal, ocolor):
    return n | normal << 2 | color << 8 | onormal << 18 | ocolor << 24


def test_unpack_surface_against_hand_packed_words():
    import voxmap_amd as vx
    fields = ("n", "normal_idx", "color", "opaque_normal_idx", "opaque_color")
    assert vx.SURF_DTYPE.names == fields
    top = (3, 7, 255, 7, 255)
    rows = [(0, 0, 0, 0, 0), top]
    for k in range(5):                                   # each field alone at its extreme, and alone at zero
        rows.append(tuple(top[i] if i == k else 0 for i in range(5)))
        rows.append(tuple(0 if i == k else top[i] for i in range(5)))
    rows += [(2, 5, 21, 4, 7), (1, 1, 3, 1, 3), (1, 0, 21, 0, 0)]     # glass over opaque, opaque, glass over sky
    words = np.array([_pack(*r) for r in rows], np.uint32)
    got = vx.unpack_surface(words)
    assert got.dtype == vx.SURF_DTYPE and got.shape == words.shape
    for i, r in enumerate(rows):
        assert tuple(int(got[f][i]) for f in fields) == r, (i, hex(words[i]))
    assert words[1] == 0xFF1CFF1F                         # the bits no field owns stay clear at every extreme
    z = vx.unpack_surface(np.zeros((2, 3), np.uint32))
    assert z.shape == (2, 3) and not z.view(np.uint8).any()
    # the bits no field owns are ignored
    assert not vx.unpack_surface(np.array([0x00E300E0 & ~_pack(*top)], np.uint32)).view(np.uint8).any()


def test_null_scene_is_einval_with_a_message(built):
    import voxmap_amd as vx
    from voxmap_amd import _abi
    L = vx.lib()
    fr = vx.make_frame((48.0, 24.0, 18.0), (1.1, 0.0, 0.6), 8, 8)
    buf = np.zeros(64, np.float32)
    pl = _abi.GbufferPlanes(buf.ctypes.data, None, None)
    st = _abi.QueryStats()
    assert L.vx_render_gbuffer(None, C.byref(fr.params), 8, 8, C.byref(pl), 0, None, C.byref(st)) == _abi.VX_EINVAL
    assert b"vx_render_gbuffer" in L.vx_last_error()
    assert not buf.any()


def test_k_gbuffer_kernel_resources(built):
    """k_gbuffer<STATS> is in the library twice (with and without counters), keeps its arguments and its
    walk state out of scratch, and its unit holds neither a render nor a query kernel."""
    from voxmap_amd import _abi, kernel_meta
    ks = kernel_meta.kernels(_abi.LIB_PATH)
    g = {k: v for k, v in ks.items() if "k_gbuffer" in k}
    assert len(g) == 2, sorted(g)
    for name, v in g.items():
        assert "k_render" not in name and "k_query" not in name
        assert v["private_segment_fixed_size"] <= kernel_meta.RENDER_SCRATCH_LIMIT, (name, v)
        assert v.get("vgpr_spill_count", 0) == 0, (name, v)
    with tempfile.TemporaryDirectory() as d:
        found = 0
        for co in kernel_meta.code_objects(_abi.LIB_PATH, d):
            notes = subprocess.run([kernel_meta._tool("llvm-readelf"), "--notes", co], check=True,
                                   capture_output=True, text=True).stdout
            if "k_gbuffer" in notes:
                found += 1
                assert "k_render" not in notes and "k_query" not in notes
        assert found == 1
