"""Sun-query rate (vx_query_sun, on_device): one call over a day's sweep against one call per sun.

S-proc at C3 size; the points are the field's ground points (vx_ground_points), the
suns a daylight sweep of 144 (vx_sun_from_hour).  Three legs, interleaved in one
process and timed with device events (warm-up, then repeats; median and range):
  (a) one vx_query_sun call with k = 144: the kernel's loop over the suns;
  (b) 144 calls with k = 1: what a host would write without that loop;
  (c) for context, the cost per shadow ray of a frame: vx_render v1 with and without
      VX_FLAG_NO_SHADOW at the C3 camera, the difference divided by shadow_rays.
The tool also checks that (a) and (b) agree on every word.  A measuring tool: it fixes no number.

    python tools/sun_rate.py [--repeats 9] [--warmup 2] [--suns 144] [--out FILE]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--suns", type=int, default=144)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sun_rate: no GPU visible (this tool measures; it has no CPU fallback)")
    c = presets.CONFIGS["C3"]
    w, h, k = c["w"], c["h"], args.suns
    grid = presets.scene_grid(c["scene"])
    Z, Y, X = grid.shape
    sc = vx.Scene(map_bytes=grid.tobytes(), map_format=vx.FORMAT_GRID, dims=(X, Y, Z), device=0)
    pts, _ = vx.ground_points(sc.read_field())
    n = len(pts)
    suns = np.array([vx.sun_from_hour(t) for t in np.linspace(-1.5, 1.5, k)], np.float32)
    W = vx.sun_words(k)
    d_pts = torch.from_numpy(pts.view(np.uint8).copy()).cuda()
    out_a = torch.zeros((n, W), dtype=torch.int32, device="cuda")
    out_b = torch.zeros((k, n, 2), dtype=torch.int32, device="cuda")
    img = torch.zeros(w * h, dtype=torch.int32, device="cuda")
    fr = presets.camera_frame(c["camera"], w, h)
    fr_ns = presets.camera_frame(c["camera"], w, h, flags=vx.FLAG_NO_SHADOW)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(fn):
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    def leg_a():
        sc.query_sun_device(d_pts.data_ptr(), n, suns, out_a.data_ptr(), stream=stream.cuda_stream)

    def leg_b():
        for j in range(k):
            sc.query_sun_device(d_pts.data_ptr(), n, suns[j:j + 1], out_b[j].data_ptr(), stream=stream.cuda_stream)

    def frame(f):
        return lambda: sc.render_device(f, img.data_ptr(), pixel_format=vx.PIXEL_RGBA8, stream=stream.cuda_stream)

    legs = {"a": leg_a, "b": leg_b, "frame": frame(fr), "frame_ns": frame(fr_ns)}
    for _ in range(args.warmup):
        for fn in legs.values():
            timed(fn)
    t = {name: [] for name in legs}
    for _ in range(args.repeats):                       # interleaved: every leg sees the same machine
        for name, fn in legs.items():
            t[name].append(timed(fn))
    st_a = sc.query_sun_device(d_pts.data_ptr(), n, suns, out_a.data_ptr(), stream=stream.cuda_stream, stats=True)
    st_plain = sc.query_sun_device(d_pts.data_ptr(), n, suns, out_a.data_ptr(), stream=stream.cuda_stream, stats=True,
                                   flags=vx.SUNQ_NO_EXIT)
    leg_a()
    stream.synchronize()
    _, st_fr = sc.render(fr, pixel_format=vx.PIXEL_RGBA8, stats=True)
    # (a) and (b) agree on every word: (a)'s words rebuilt from (b)'s k answers
    a = out_a.cpu().numpy().view(np.uint32)
    b = out_b.cpu().numpy().view(np.uint32)
    want = np.zeros((n, W), np.uint32)
    for j in range(k):
        assert np.array_equal(b[j, :, 0], b[j, :, 1]) and (b[j, :, 0] <= 1).all(), f"k = 1 answer of sun {j} is no flag"
        want[:, 1 + j // 32] |= b[j, :, 0] << np.uint32(j % 32)
        want[:, 0] += b[j, :, 0]
    bad = int(np.count_nonzero(a != want))

    def line(name, v):
        return (f"{name}: median {statistics.median(v):.3f} ms, min {min(v):.3f}, max {max(v):.3f} "
                f"({len(v)} repeats after {args.warmup} warm-up, device events)")
    ma, mb = statistics.median(t["a"]), statistics.median(t["b"])
    mf, mn = statistics.median(t["frame"]), statistics.median(t["frame_ns"])
    out = [
        f"sun_rate: S-proc {X}x{Y}x{Z}, {n} ground points x {k} suns (hour -1.5 .. 1.5)",
        line(f"(a) vx_query_sun, one call, k = {k}", t["a"]),
        line(f"(b) vx_query_sun, {k} calls, k = 1", t["b"]),
        f"(a) vs (b): {mb / ma:.2f}x; per march (a) {1e6 * ma / max(1, st_a.rays):.3f} ns, (b) "
        f"{1e6 * mb / max(1, st_a.rays):.3f} ns; per call of (b) {1e3 * mb / k:.1f} us",
        f"counters (a): {st_a.as_dict()}",
        f"fetches per march: {st_a.fetches / max(1, st_a.rays):.2f} with the exit copies, "
        f"{st_plain.fetches / max(1, st_plain.rays):.2f} with VX_SUNQ_NO_EXIT; kernel_ms {st_a.kernel_ms:.3f} / "
        f"{st_plain.kernel_ms:.3f}",
        line(f"(c) vx_render v1 {w}x{h} RGBA8, camera {c['camera']}", t["frame"]),
        line("(c) the same with VX_FLAG_NO_SHADOW", t["frame_ns"]),
        f"(c) shadow cost: {mf - mn:.3f} ms over {st_fr.shadow_rays} shadow rays = "
        f"{1e6 * (mf - mn) / max(1, st_fr.shadow_rays):.3f} ns per ray ({st_fr.shadow_fetches / max(1, st_fr.shadow_rays):.2f} "
        f"fetches per ray)",
        f"(a) against (b), every word: {bad} of {a.size} differ",
    ]
    text = "\n".join(out)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")
    sc.close()
    if bad:
        raise SystemExit(f"sun_rate: {bad} words of the one-call and per-sun answers disagree")


if __name__ == "__main__":
    main()
