"""vx_render_aa beside the hi-res vx_render it is defined by, and the scratch-cap sweep.

S-proc at the C3 camera, full quality, output 3840 x 2160.  The yardstick of a
factor s is what a caller could do before vx_render_aa existed: vx_render of the
(s*w) x (s*h) frame into a device buffer, the hi-res render alone (no resolve).
Timed with device events on one stream, warm-ups first, then repeats with every
leg interleaved in one process so all see the same machine; median and range.

  * RGBA8, s = 2: vx_render_aa at each scratch cap of the sweep / the hi-res render.
    The resolve moves 4*s*s*w*h bytes in and 4*w*h out; at the streaming rate
    (--stream-tbps, 6.3 TB/s measured for a float4 copy) that is the floor's
    time if the chunks come from HBM.  A ratio near 1 + floor / render means the
    chunks missed the cache, a ratio near 1.0 that they stayed on-die.
  * s = 4 (RGBA8) and RGBA32F (s = 2) once each, at the default cap.

It also checks the RGBA8 s = 2 frame against the hi-res frame resolved with
torch integer arithmetic on the device.  A measuring tool: it fixes no number.
VOXMAP_LIB selects a variant library (build.py: defines=["VX_RESOLVE_NT=1"]).

    python tools/aa_rate.py [--repeats 15] [--warmup 3] [--out FILE]
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import voxmap_amd as vx
from voxmap_amd import _abi, presets

MIB = 1 << 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--width", type=int, default=presets.CONFIGS["C3"]["w"])
    ap.add_argument("--height", type=int, default=presets.CONFIGS["C3"]["h"])
    ap.add_argument("--caps-mib", default="8,32,128", help="scratch caps of the sweep; the whole hi-res frame is added")
    ap.add_argument("--stream-tbps", type=float, default=6.3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("aa_rate: no GPU visible (this tool measures; it has no CPU fallback)")
    c = presets.CONFIGS["C3"]
    w, h = args.width, args.height
    grid = presets.scene_grid(c["scene"])
    Z, Y, X = grid.shape
    sc = vx.Scene(map_bytes=grid.tobytes(), map_format=vx.FORMAT_GRID, dims=(X, Y, Z), device=0)
    fr = presets.camera_frame(c["camera"], w, h, flags=vx.FLAG_FULL_QUALITY)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(fn):
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    bpp = {vx.PIXEL_RGBA8: 4, vx.PIXEL_RGBA32F: 16}
    out = torch.zeros(w * h * 16, dtype=torch.uint8, device="cuda")          # any format's output
    hi_bufs = {}

    def hi_leg(s, fmt):
        """vx_render of the (s*w) x (s*h) frame: the parent's own capability."""
        n = s * w * s * h * bpp[fmt]
        if n not in hi_bufs:
            hi_bufs[n] = torch.zeros(n, dtype=torch.uint8, device="cuda")
        f = vx.Frame(fr.params, s * w, s * h)
        return lambda: sc.render_device(f, hi_bufs[n].data_ptr(), pixel_format=fmt, stream=stream.cuda_stream)

    def aa_leg(s, fmt, cap):
        return lambda: sc.render_aa_device(fr, s, out.data_ptr(), pixel_format=fmt, stream=stream.cuda_stream,
                                           scratch_cap=cap)

    whole = 2 * w * 2 * h * 4 + 8 * 2 * w * 4                                   # the hi-res frame, rows rounded up to 8
    caps = [int(v) * MIB for v in args.caps_mib.split(",")] + [whole]
    legs = {"hi s=2 u8": hi_leg(2, vx.PIXEL_RGBA8)}
    for cap in caps:
        legs[f"aa s=2 u8 cap {cap / MIB:.0f} MiB"] = aa_leg(2, vx.PIXEL_RGBA8, cap)
    legs["hi s=4 u8"] = hi_leg(4, vx.PIXEL_RGBA8)
    legs["aa s=4 u8 default cap"] = aa_leg(4, vx.PIXEL_RGBA8, 0)
    legs["hi s=2 f32"] = hi_leg(2, vx.PIXEL_RGBA32F)
    legs["aa s=2 f32 default cap"] = aa_leg(2, vx.PIXEL_RGBA32F, 0)
    for _ in range(args.warmup):
        for fn in legs.values():
            timed(fn)
    times = {k: [] for k in legs}
    for _ in range(args.repeats):                       # interleaved: every leg sees the same machine
        for k, fn in legs.items():
            times[k].append(timed(fn))
    med = {k: statistics.median(t) for k, t in times.items()}

    # the RGBA8 s = 2 frame against the hi-res frame resolved in integers on the device
    timed(legs["hi s=2 u8"])
    timed(aa_leg(2, vx.PIXEL_RGBA8, 0))
    hi = hi_bufs[2 * w * 2 * h * 4].view(h, 2, w, 2, 4).to(torch.int32)
    want = ((hi.sum(dim=(1, 3)) + 2) >> 2).to(torch.uint8)
    got = out[:w * h * 4].view(h, w, 4)
    bad = int((want != got).sum().item())

    def line(name):
        t = times[name]
        return f"{name:28s} median {med[name]:.4f} ms, min {min(t):.4f}, max {max(t):.4f}"

    lines = [
        f"aa_rate: S-proc {X}x{Y}x{Z}, camera {c['camera']}, full quality, output {w}x{h}; library "
        f"{os.path.basename(_abi.LIB_PATH) if os.environ.get('VOXMAP_LIB') else 'the product build'}",
        f"{args.repeats} repeats after {args.warmup} warm-ups, device events, all legs interleaved in one process",
        f"default scratch cap (VX_AA_DEFAULT_SCRATCH): {vx.AA_DEFAULT_SCRATCH / MIB:.0f} MiB",
        "", line("hi s=2 u8")]
    traffic = 4 * 4 * w * h + 4 * w * h
    floor_ms = traffic / (args.stream_tbps * 1e12) * 1e3
    for cap in caps:
        k = f"aa s=2 u8 cap {cap / MIB:.0f} MiB"
        plan = vx.aa_plan(w, h, 2, vx.PIXEL_RGBA8, cap)
        lines.append(f"{line(k)}  ratio {med[k] / med['hi s=2 u8']:.3f}  ({plan['n_chunks']} chunks of "
                     f"{plan['chunk_rows_out']} rows, {plan['scratch_bytes'] / MIB:.1f} MiB)")
    lines += [
        f"resolve traffic {traffic / 1e6:.0f} MB; at {args.stream_tbps} TB/s {floor_ms:.4f} ms: a ratio of "
        f"{1 + floor_ms / med['hi s=2 u8']:.3f} would mean the chunks came from HBM, 1.0 that they stayed on-die",
        "", line("hi s=4 u8"),
        f"{line('aa s=4 u8 default cap')}  ratio {med['aa s=4 u8 default cap'] / med['hi s=4 u8']:.3f}",
        line("hi s=2 f32"),
        f"{line('aa s=2 f32 default cap')}  ratio {med['aa s=2 f32 default cap'] / med['hi s=2 f32']:.3f}",
        "", f"RGBA8 s=2 frame vs the hi-res frame resolved in integers on the device: {bad} of {w * h * 4} bytes differ",
    ]
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")
    sc.close()
    if bad:
        raise SystemExit(f"aa_rate: {bad} bytes disagree with the resolved hi-res frame")


if __name__ == "__main__":
    main()
