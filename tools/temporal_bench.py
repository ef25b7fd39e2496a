"""Time of the temporal accumulation (TemporalAccumulator.accumulate_device) alone on C3's and C5's frames at 1024 x 1024, default
parameters, next to the render of the same 16 spp, the feature pass, the per-pixel mean and variance and the denoiser's default call.
The frame is 4 batches x 4 spp in a DeviceBuffer with the feature planes of the 16 samples; two cameras a small step apart alternate,
so every timed call reprojects (the share of pixels that took history is printed).  HIP events around the stream, a warm-up round, then
the median of the rounds with min-max in brackets; a round of the accumulation is `--calls` calls back to back, divided by their number
(one call is tens of microseconds).
Floor of the pass: the inputs (rgb, var, normal, depth: 80 B), one record read and one record written (80 B each) per pixel, 240 B,
over the HBM peak bench.py's roofline uses (8 TB/s); the outputs (40 B) and the up to three further taps, which neighbouring lanes
share, are not in it.  A device-to-device copy of the same 240 B per pixel is measured next to it.
Usage: python tools/temporal_bench.py [--size 1024] [--spp 16] [--rounds 5] [--calls 20]"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from rpt_amd import Camera, DenoiseParams, Denoiser, DeviceBuffer, Renderer, TemporalAccumulator, TemporalParams, scenes  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, default=1024)
ap.add_argument("--spp", type=int, default=16)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--calls", type=int, default=20)
args = ap.parse_args()
HBM_PEAK_GBS = 8000.0
FLOOR_BYTES = 240

n = args.size * args.size
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


floor_ms = n * FLOOR_BYTES / (HBM_PEAK_GBS * 1e6)
src, dst = zeros(15 * n), zeros(15 * n)
copy_ms = timed(lambda k: dst.copy_(src))
print(f"floor of the accumulation at {args.size}x{args.size}: {FLOOR_BYTES} B per pixel / {HBM_PEAK_GBS / 1000:.0f} TB/s = {floor_ms:.4f} ms; "
      f"device-to-device copy of 120 B per pixel (120 B read + 120 B written): {fmt(copy_ms)}", flush=True)

for name in ("C3", "C5"):
    scene, cam, cfg = scenes.CONFIGS[name]()
    cams = [cam, stepped(cam)]
    r = Renderer(scene, cam).width(args.size).height(args.size).max_bounces(cfg["max_bounces"]).seed(1)
    planes = [[zeros(3 * n) for _ in range(3)] for _ in cams]          # albedo, normal, depth of each camera
    frame, rgb, var = zeros(3 * n), zeros(3 * n), zeros(n)
    out, out_var, out_len, filtered = zeros(3 * n), zeros(n), zeros(n), zeros(3 * n)
    torch.cuda.synchronize()

    def render(k):
        r._sample_offset = 0
        r.sample_device(args.spp, frame.data_ptr(), stream.cuda_stream)

    render_ms = timed(render)
    feature_ms = timed(lambda k: r.features_device(args.spp, *[p.data_ptr() for p in planes[0]], stream_ptr=stream.cuda_stream, sample_offset=0))
    for c, pl in zip(cams, planes):
        r.camera = c
        r.features_device(args.spp, *[p.data_ptr() for p in pl], sample_offset=0)
    r.camera = cam
    buf = DeviceBuffer(args.size, args.size)
    r._sample_offset = 0
    for _ in range(4):
        r.sample(args.spp // 4, buf)
    torch.cuda.synchronize()
    mean_ms = timed(lambda k: buf.mean_device(rgb.data_ptr(), var.data_ptr(), stream.cuda_stream))
    denoiser, acc = Denoiser(args.size, args.size), TemporalAccumulator(args.size, args.size)
    denoise_ms = timed(lambda k: denoiser.denoise_device(rgb.data_ptr(), var.data_ptr(), *[p.data_ptr() for p in planes[0]], filtered.data_ptr(),
                                                         out_var.data_ptr(), params=DenoiseParams(), stream_ptr=stream.cuda_stream))
    p = TemporalParams()

    def accumulate(k):
        pl = planes[k % 2]
        acc.accumulate_device(cams[k % 2], rgb.data_ptr(), var.data_ptr(), pl[1].data_ptr(), pl[2].data_ptr(), out.data_ptr(), out_var.data_ptr(),
                              out_len.data_ptr(), params=p, stream_ptr=stream.cuda_stream)

    acc_ms = timed(accumulate, calls=2 * (args.calls // 2))
    torch.cuda.synchronize()
    took = float((out_len > 1.0).double().mean())
    med = statistics.median(acc_ms)
    print(f"{name} {args.size}x{args.size}x{args.spp}: render {fmt(render_ms)}; feature planes {fmt(feature_ms)}; mean + variance {fmt(mean_ms)}; "
          f"denoiser, default call {fmt(denoise_ms)}", flush=True)
    print(f"  {name} accumulate, one call of {args.calls} back to back: {fmt(acc_ms)} = {med / floor_ms:.2f} x the floor, "
          f"{med / statistics.median(copy_ms):.2f} x the copy, {med / statistics.median(render_ms) * 100:.2f} % of the render; "
          f"{took * 100:.1f} % of the pixels took history, mean len {float(out_len.mean()):.2f}, frames {acc.frames}", flush=True)
    acc.close()
    denoiser.close()
    buf.close()
