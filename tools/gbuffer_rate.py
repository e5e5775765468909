"""Frame G-buffer rate (vx_render_gbuffer) beside the two routes to the same data that came before it.

S-proc at the C3 camera, 3840 x 2160, device events, warm-up then repeats with all legs
interleaved in one process (every leg sees the same machine); median and range reported:

  gbuffer, 3 planes   vx_render_gbuffer with depth, opaque_depth and surface (12 bytes out per pixel)
  gbuffer, depth      vx_render_gbuffer with depth alone (4 bytes out; the walk is the same)
  query route         vx_query_rays(on_device) over device-built pixel rays (48 bytes in, 88 out):
                      the only way to this data before vx_render_gbuffer
  PRIMARY_ONLY frame  vx_render with VX_FLAG_PRIMARY_ONLY, RGBA8: the same walk with 4 bytes out

The tool also checks that the planes equal what the query route's hits say, on every pixel.
A measuring tool: it fixes no number.

    python tools/gbuffer_rate.py [--repeats 15] [--warmup 3] [--out FILE]
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import voxmap_amd as vx
from voxmap_amd import presets
from query_rate import device_pixel_rays


def planes_of_hits(hv: np.ndarray):
    """(depth bits, opaque_depth bits, surface words) from vx_ray_hit records as (n, 22) int32 rows
    (include/voxmap.h: n, reserved, then two 10-word vx_surface records: id, color, normal_idx, ..., t)."""
    inf = np.float32(np.inf).view(np.int32)
    n = np.maximum(hv[:, 0], 0)
    rec = [hv[:, 2:12], hv[:, 12:22]]
    first = n >= 1
    k0 = first & (rec[0][:, 0] == 0)
    k1 = (n >= 2) & (rec[1][:, 0] == 0) & ~k0
    depth = np.where(first, rec[0][:, 9], inf)
    opaque = np.where(k0, rec[0][:, 9], np.where(k1, rec[1][:, 9], inf))
    half = [r[:, 2] << 2 | r[:, 1] << 8 for r in rec]
    word = np.where(first, n | half[0], 0) | np.where(k0, half[0], np.where(k1, half[1], 0)) << 16
    return depth.view(np.uint32), opaque.view(np.uint32), word.astype(np.uint32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--width", type=int, default=presets.CONFIGS["C3"]["w"])
    ap.add_argument("--height", type=int, default=presets.CONFIGS["C3"]["h"])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gbuffer_rate: no GPU visible (this tool measures; it has no CPU fallback)")
    c = presets.CONFIGS["C3"]
    w, h = args.width, args.height
    grid = presets.scene_grid(c["scene"])
    Z, Y, X = grid.shape
    sc = vx.Scene(map_bytes=grid.tobytes(), map_format=vx.FORMAT_GRID, dims=(X, Y, Z), device=0)
    fr = presets.camera_frame(c["camera"], w, h, flags=vx.FLAG_PRIMARY_ONLY)
    n = w * h
    rays = device_pixel_rays(fr, w, h)
    hits = torch.zeros((n, vx.HIT_DTYPE.itemsize // 4), dtype=torch.int32, device="cuda")
    img = torch.zeros(n, dtype=torch.int32, device="cuda")
    planes = torch.zeros((3, n), dtype=torch.int32, device="cuda")
    depth_only = torch.zeros(n, dtype=torch.int32, device="cuda")
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

    def gbuffer(**kw):
        return sc.gbuffer_device(fr, depth=planes[0].data_ptr(), opaque_depth=planes[1].data_ptr(),
                                 surface=planes[2].data_ptr(), stream=s, **kw)

    legs = {
        "vx_render_gbuffer, 3 planes": gbuffer,
        "vx_render_gbuffer, depth only": lambda: sc.gbuffer_device(fr, depth=depth_only.data_ptr(), stream=s),
        "vx_query_rays(on_device) over pixel rays": lambda: sc.query_rays_device(rays.data_ptr(), n, hits.data_ptr(), stream=s),
        "vx_render PRIMARY_ONLY RGBA8": lambda: sc.render_device(fr, img.data_ptr(), pixel_format=vx.PIXEL_RGBA8, stream=s),
    }
    for _ in range(args.warmup):
        for fn in legs.values():
            timed(fn)
    t = {name: [] for name in legs}
    for _ in range(args.repeats):                       # interleaved: every leg sees the same machine
        for name, fn in legs.items():
            t[name].append(timed(fn))
    st = gbuffer(stats=True)
    qst = sc.query_rays_device(rays.data_ptr(), n, hits.data_ptr(), stream=s, stats=True)
    stream.synchronize()
    want = planes_of_hits(hits.cpu().numpy())
    got = planes.cpu().numpy().view(np.uint32)
    bad = [int(np.count_nonzero(want[k] != got[k])) for k in range(3)]
    bad.append(int(np.count_nonzero(depth_only.cpu().numpy().view(np.uint32) != want[0])))

    med = {name: statistics.median(v) for name, v in t.items()}
    names = list(legs)
    out = [f"gbuffer_rate: S-proc {X}x{Y}x{Z}, camera {c['camera']}, {w}x{h} = {n} pixels"]
    out += [f"{name}: median {med[name]:.3f} ms, min {min(v):.3f}, max {max(v):.3f} "
            f"({len(v)} repeats after {args.warmup} warm-up, device events, legs interleaved)" for name, v in t.items()]
    out += [
        f"3 planes / query route {med[names[0]] / med[names[2]]:.2f}; 3 planes / PRIMARY_ONLY frame "
        f"{med[names[0]] / med[names[3]]:.2f}; depth only / PRIMARY_ONLY frame {med[names[1]] / med[names[3]]:.2f}; "
        f"query route / PRIMARY_ONLY frame {med[names[2]] / med[names[3]]:.2f}",
        f"gbuffer counters: {st.as_dict()}",
        f"query counters:   {qst.as_dict()}",
        f"fetches per pixel {st.fetches / n:.2f}; bytes per pixel: gbuffer 0 in, 12 (4) out; query route 48 in, 88 out",
        f"planes vs the query route's hits: depth, opaque_depth, surface, depth-only differ at {bad} of {n} pixels",
    ]
    text = "\n".join(out)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")
    sc.close()
    same_counts = {k: v for k, v in st.as_dict().items() if k != "kernel_ms"} == \
        {k: v for k, v in qst.as_dict().items() if k != "kernel_ms"}
    if any(bad) or not same_counts:
        raise SystemExit("gbuffer_rate: the planes or the counters disagree with the query route")


if __name__ == "__main__":
    main()
