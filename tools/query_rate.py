"""Ray-query rate (vx_query_rays, on_device) beside the PRIMARY_ONLY frame of the same camera.

S-proc at the C3 camera: the 3840 x 2160 pixel rays are built on the device with
vx_pixel_ray's formula, walked by k_query and timed with device events (warm-up,
then repeats alternating with the VX_FLAG_PRIMARY_ONLY frame; median and spread
reported).  The tool also checks that every pixel's first record colour, through
kPalette, is the PRIMARY_ONLY frame's pixel.  A measuring tool: it fixes no number.

    python tools/query_rate.py [--repeats 15] [--warmup 3] [--out FILE]
"""
import argparse
import os
import re
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import voxmap_amd as vx
from voxmap_amd import presets

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def palette_rgba8() -> np.ndarray:
    """kPalette of csrc/vx_loads.h as the RGBA8 words a PRIMARY_ONLY frame holds (pack_rgba8)."""
    src = open(os.path.join(ROOT, "voxmap_amd", "csrc", "vx_loads.h")).read()
    body = re.search(r"kPalette\[22\]\[3\] = \{(.*?)\n\};", src, re.S).group(1)
    pal = np.array([[float(v.rstrip("f")) for v in row.split(",")] for row in re.findall(r"\{([^{}]+)\}", body)],
                   np.float32)
    assert pal.shape == (22, 3)
    b = np.floor(np.clip(pal, 0, 1) * np.float32(255) + np.float32(0.5)).astype(np.uint32)
    return b[:, 0] | b[:, 1] << 8 | b[:, 2] << 16 | np.uint32(255) << 24


def device_pixel_rays(fr, w: int, h: int) -> torch.Tensor:
    """(w*h, 12) int32 on the device: vx_ray records of every pixel, row-major.  nx, ny come
    from the host (w + h fp32 quotients, vx_pixel_ray's own); the per-pixel sums
    (fwd + nx*right) + ny*up are separate fp32 device operations in that order."""
    p = fr.params
    nx = torch.from_numpy((2 * np.arange(w) + 1).astype(np.float32) / np.float32(w) - np.float32(1)).cuda()
    ny = torch.from_numpy(np.float32(1) - (2 * np.arange(h) + 1).astype(np.float32) / np.float32(h)).cuda()
    rays = torch.zeros((h, w, 12), dtype=torch.int32, device="cuda")
    f = rays.view(torch.float32)
    for i in range(3):
        rays[:, :, i] = int(p.cam_cell[i])
        f[:, :, 3 + i] = float(p.cam_fract[i])
        a = nx * float(p.ray_right[i])
        a = a + float(p.ray_fwd[i])                     # fwd + nx*right (the sum commutes exactly)
        b = ny * float(p.ray_up[i])
        f[:, :, 6 + i] = a[None, :] + b[:, None]
    f[:, :, 9] = float("inf")
    return rays.view(w * h, 12)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--width", type=int, default=presets.CONFIGS["C3"]["w"])
    ap.add_argument("--height", type=int, default=presets.CONFIGS["C3"]["h"])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("query_rate: no GPU visible (this tool measures; it has no CPU fallback)")
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
    # the device rays are vx_pixel_ray's, bit for bit, on a sample of pixels
    host = rays[:: max(1, n // 997)].cpu().numpy()
    for k, rec in zip(range(0, n, max(1, n // 997)), host):
        want = vx.pixel_ray(fr, k % w, k // w)
        assert rec.tobytes() == want.tobytes(), f"device ray of pixel {k} differs from vx_pixel_ray"
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(fn):
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    def query():
        sc.query_rays_device(rays.data_ptr(), n, hits.data_ptr(), stream=stream.cuda_stream)

    def frame():
        sc.render_device(fr, img.data_ptr(), pixel_format=vx.PIXEL_RGBA8, stream=stream.cuda_stream)

    for _ in range(args.warmup):
        timed(query)
        timed(frame)
    tq, tf = [], []
    for _ in range(args.repeats):                       # alternating: both see the same machine
        tq.append(timed(query))
        tf.append(timed(frame))
    st = sc.query_rays_device(rays.data_ptr(), n, hits.data_ptr(), stream=stream.cuda_stream, stats=True)
    stream.synchronize()
    # every pixel's first record colour is the PRIMARY_ONLY frame's pixel
    hv = hits.cpu().numpy()
    nrec, color0 = hv[:, 0], hv[:, 3]                   # n; s[0].color
    want = palette_rgba8()[np.where(nrec >= 1, color0, 0)]
    got = img.cpu().numpy().view(np.uint32)
    bad = int(np.count_nonzero(want != got))

    def line(name, t):
        return (f"{name}: median {statistics.median(t):.3f} ms, min {min(t):.3f}, max {max(t):.3f} "
                f"({len(t)} repeats after {args.warmup} warm-up, device events)")
    mq, mf = statistics.median(tq), statistics.median(tf)
    out = [
        f"query_rate: S-proc {X}x{Y}x{Z}, camera {c['camera']}, {w}x{h} = {n} pixel rays, t_max = inf",
        line("vx_query_rays(on_device)", tq),
        line("vx_render PRIMARY_ONLY RGBA8", tf),
        f"rate: {n / mq / 1e3:.1f} Mrays/s (queries) vs {n / mf / 1e3:.1f} Mpixels/s (PRIMARY_ONLY); "
        f"query / frame time ratio {mq / mf:.2f}",
        f"counters: {st.as_dict()}",
        f"fetches per ray {st.fetches / n:.2f}; bytes moved per ray: 48 in, 88 out",
        f"first-record colour vs PRIMARY_ONLY pixel: {bad} of {n} differ",
    ]
    text = "\n".join(out)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")
    sc.close()
    if bad:
        raise SystemExit(f"query_rate: {bad} pixels disagree with the PRIMARY_ONLY frame")


if __name__ == "__main__":
    main()
