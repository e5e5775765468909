"""Orthographic frame rate (vx_render_ortho) beside vx_render at the same size.

S-proc (the C3 field), 3840 x 2160 RGBA8, one stream, device events, warm-up then
repeats with all legs interleaved in one process (every leg sees the same
machine); median and range reported:

  ortho plan          the north-up plan over the field's full y extent (no sky, one octant)
  ortho iso           the oblique direction (.4, .8, -.9) over the whole field (sky around it)
  vx_render K0 / K1   the perspective frame at the near-vertical camera K0 and at the
                      bench's camera K1 (this kernel is the parent commit's: tools/isa_diff.py)

each with the v1 flags and with REFLECT | ROUGH.  Also the fetches per pixel of
every leg and k_ortho's registers, scratch and occupancy from the library's
metadata.  The workloads differ (a plan has no sky and its rays never diverge
in octant), so the legs are reported side by side, not as a ratio to hold.
A measuring tool: it fixes no number.

    python tools/ortho_rate.py [--repeats 20] [--warmup 3] [--out FILE]
"""
import argparse
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import voxmap_amd as vx
from voxmap_amd import _abi, kernel_meta, presets


def resources():
    """k_ortho's metadata per instantiation: registers, scratch, spills, waves per SIMD by the VGPR count
    (512 per SIMD lane, allocated in eights, at most 8 waves)."""
    out = []
    for name, v in sorted(kernel_meta.kernels(_abi.LIB_PATH).items()):
        if "k_ortho" not in name:
            continue
        fmt, stats = name[name.index("k_orthoILi") + 10], name[name.index("ELb") + 3]
        vg = v.get("vgpr_count", 0)
        waves = min(8, 512 // max(8, -(-vg // 8) * 8))
        out.append(f"k_ortho<{'RGBA8' if fmt == '1' else 'RGBA32F'}, {'STATS' if stats == '1' else 'timed'}>: "
                   f"{vg} VGPRs, {v.get('sgpr_count', 0)} SGPRs, {v.get('private_segment_fixed_size', 0)} B scratch, "
                   f"{v.get('vgpr_spill_count', 0)} VGPR / {v.get('sgpr_spill_count', 0)} SGPR spills, "
                   f"{v.get('group_segment_fixed_size', 0)} B LDS: {waves} waves/SIMD")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--width", type=int, default=presets.CONFIGS["C3"]["w"])
    ap.add_argument("--height", type=int, default=presets.CONFIGS["C3"]["h"])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ortho_rate: no GPU visible (this tool measures; it has no CPU fallback)")
    c = presets.CONFIGS["C3"]
    w, h = args.width, args.height
    grid = presets.scene_grid(c["scene"])
    Z, Y, X = grid.shape
    sc = vx.Scene(map_bytes=grid.tobytes(), map_format=vx.FORMAT_GRID, dims=(X, Y, Z), device=0)
    sun = presets.sun_dir()
    n = w * h
    iso = (.4, .8, -.9)
    il = math.sqrt(sum(v * v for v in iso))
    views = {
        # half the field's y extent up and down: no pixel off the grid
        "ortho plan": lambda fl: vx.frame_from_ortho((X / 2, Y / 2, 0.0), -math.pi / 2, math.pi / 2, Y / 2 * w / h,
                                                     Z + 8.0, w, h, sun=sun, flags=fl),
        "ortho iso": lambda fl: vx.frame_from_ortho((X / 2, Y / 2, Z / 4), math.atan2(-iso[1], -iso[0]),
                                                    math.asin(-iso[2] / il), 0.6 * X, 4.0 * Z + Y, w, h, sun=sun, flags=fl),
    }
    img = torch.zeros(n, dtype=torch.int32, device="cuda")
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s = stream.cuda_stream

    def timed(fn):
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    legs, counted = {}, {}
    for tag, fl in (("v1", 0), ("REFLECT|ROUGH", vx.FLAG_FULL_QUALITY)):
        for name, make in views.items():
            fr = make(fl)
            legs[f"{name}, {tag}"] = lambda fr=fr: sc.render_ortho_device(fr, img.data_ptr(), pixel_format=vx.PIXEL_RGBA8,
                                                                         stream=s)
            counted[f"{name}, {tag}"] = lambda fr=fr: sc.render_ortho_device(fr, img.data_ptr(), stream=s, stats=True,
                                                                            pixel_format=vx.PIXEL_RGBA8)
        for cam in ("K0", c["camera"]):
            fr = presets.camera_frame(cam, w, h, flags=fl)
            legs[f"vx_render {cam}, {tag}"] = lambda fr=fr: sc.render_device(fr, img.data_ptr(), stream=s,
                                                                            pixel_format=vx.PIXEL_RGBA8)
            counted[f"vx_render {cam}, {tag}"] = lambda fr=fr: sc.render_device(fr, img.data_ptr(), stream=s, stats=True,
                                                                               pixel_format=vx.PIXEL_RGBA8)
    for _ in range(args.warmup):
        for fn in legs.values():
            timed(fn)
    t = {name: [] for name in legs}
    for _ in range(args.repeats):                       # interleaved: every leg sees the same machine
        for name, fn in legs.items():
            t[name].append(timed(fn))
    out = [f"ortho_rate: S-proc {X}x{Y}x{Z}, {w}x{h} = {n} pixels, RGBA8, sun {tuple(round(v, 4) for v in sun)}; "
           f"{args.repeats} repeats after {args.warmup} warm-up, device events, one stream, legs interleaved; "
           f"one machine's numbers"]
    for name, v in t.items():
        st = counted[name]().as_dict()
        out.append(f"{name}: median {statistics.median(v):.3f} ms, min {min(v):.3f}, max {max(v):.3f}; per pixel "
                   f"{st['primary_fetches'] / n:.2f} primary + {st['shadow_fetches'] / n:.2f} shadow + "
                   f"{st['reflect_fetches'] / n:.2f} mirror fetches; sky {st['sky_px'] / n:.1%}, glass "
                   f"{st['glass_px'] / n:.1%}, shadow rays {st['shadow_rays'] / n:.2f}, cap hits {st['primary_cap_hits']}")
    out += resources()
    text = "\n".join(out)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")
    sc.close()


if __name__ == "__main__":
    main()
