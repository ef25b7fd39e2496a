"""Time of the temporal accumulation with history clipping (RPT_TEMPORAL_CLIP), after tools/temporal_bench.py and
tools/temporal_motion_bench.py: TemporalAccumulator.accumulate_device alone on C3's frame at 1024 x 1024 and 1920 x 1080, default
parameters, the frame 4 batches x 4 spp in a DeviceBuffer with the feature planes of the 16 samples, two cameras a small step apart
alternating so that every timed call reprojects.  HIP events around the stream, a warm-up round, then the median of the rounds with
min-max in brackets; a round is `--calls` calls back to back, divided by their number.

  no flag           the kernel's first instantiation
  clip, r = 1..3    the clipped instantiation: the block's (16 + 2r)^2 halo staged in LDS, then 9 / 25 / 49 window cells per pixel that
                    took history (27 / 75 / 147 additions and as many multiply-adds' worth of squares), gamma 0.5, clip_history 1

The floor of the pass (240 B per pixel over the HBM peak) is tools/temporal_bench.py's: the clipped form reads no plane the kernel
does not already read, and the halo's re-reads of rgb and ids fall on lines a neighbouring block has just fetched.
Usage: python tools/temporal_clip_bench.py [--sizes 1024x1024,1920x1080] [--spp 16] [--rounds 5] [--calls 20]"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from rpt_amd import Camera, DeviceBuffer, Renderer, TemporalAccumulator, TemporalParams, _lib, scenes  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", default="1024x1024,1920x1080")
ap.add_argument("--spp", type=int, default=16)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--calls", type=int, default=20)
args = ap.parse_args()
HBM_PEAK_GBS = 8000.0
FLOOR_BYTES = 240
stream = torch.cuda.Stream()


def timed(job, rounds=args.rounds, calls=1):
    ms = []
    for rnd in range(rounds + 1):   # round 0 warms up
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            a.record(stream)
            for k in range(calls):
                job(k)
            b.record(stream)
        b.synchronize()
        if rnd:
            ms.append(a.elapsed_time(b) / calls)
    return ms


def fmt(ms):
    return f"{statistics.median(ms):.4f} ms [{min(ms):.4f}-{max(ms):.4f}]"


def zeros(k):
    return torch.zeros(k, dtype=torch.float64, device="cuda")


def stepped(cam):
    """The camera a small step to its right: 0.2 % of the eye's distance from the origin."""
    right = np.cross(cam.direction, cam.up)
    right = right / np.linalg.norm(right)
    return Camera(cam.eye + 0.002 * max(float(np.linalg.norm(cam.eye)), 1.0) * right, cam.direction, cam.up, cam.fov, cam.aperture, cam.focal_distance)


print(f"library {_lib.LIB_PATH}", flush=True)
for size in args.sizes.split(","):
    w, h = [int(t) for t in size.split("x")]
    n = w * h
    floor_ms = n * FLOOR_BYTES / (HBM_PEAK_GBS * 1e6)
    scene, cam, cfg = scenes.CONFIGS["C3"]()
    cams = [cam, stepped(cam)]
    r = Renderer(scene, cam).width(w).height(h).max_bounces(cfg["max_bounces"]).seed(1)
    planes = [[zeros(3 * n) for _ in range(3)] for _ in cams]
    rgb, var = zeros(3 * n), zeros(n)
    out, out_var, out_len = zeros(3 * n), zeros(n), zeros(n)
    torch.cuda.synchronize()
    for c, pl in zip(cams, planes):
        r.camera = c
        r.features_device(args.spp, *[p.data_ptr() for p in pl], sample_offset=0)
    r.camera = cam
    buf = DeviceBuffer(w, h)
    r._sample_offset = 0
    for _ in range(4):
        r.sample(args.spp // 4, buf)
    torch.cuda.synchronize()
    buf.mean_device(rgb.data_ptr(), var.data_ptr())
    torch.cuda.synchronize()
    print(f"C3 {w}x{h}x{args.spp}; floor {floor_ms:.4f} ms", flush=True)

    def run(what, p, radius=None):
        acc = TemporalAccumulator(w, h)
        if radius is not None:
            acc.set_clip(radius, 0.5, 1)

        def accumulate(k):
            pl = planes[k % 2]
            acc.accumulate_device(cams[k % 2], rgb.data_ptr(), var.data_ptr(), pl[1].data_ptr(), pl[2].data_ptr(), out.data_ptr(), out_var.data_ptr(),
                                  out_len.data_ptr(), params=p, stream_ptr=stream.cuda_stream)

        ms = timed(accumulate, calls=2 * (args.calls // 2))
        torch.cuda.synchronize()
        took = float((out_len > 1.0).double().mean())
        med = statistics.median(ms)
        print(f"  accumulate, {what}: {fmt(ms)} = {med / floor_ms:.2f} x the floor; {took * 100:.1f} % of the pixels took history, "
              f"mean len {float(out_len.mean()):.2f}", flush=True)
        acc.close()
        return med

    base = run("no flag", TemporalParams())
    for radius in (1, 2, 3):
        med = run(f"clip, r = {radius}", TemporalParams(clip=True), radius)
        print(f"    {med - base:+.4f} ms against no flag ({(med / base - 1.0) * 100:+.1f} %)", flush=True)
    again = run("no flag, again", TemporalParams())
    print(f"    {again - base:+.4f} ms against the first measurement: the sitting's drift", flush=True)
    buf.close()
    scene.close()
