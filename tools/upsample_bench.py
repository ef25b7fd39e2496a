"""Time of the guided upsampling (rpt_upsample_device) at 1024 x 1024 from 512 x 512 (s = 2) and from 256 x 256 (s = 4), r = 1 and 2,
the default terms (demodulation, id match, normal term) with both outputs, on rendered lampshade frames: HIP events on a non-blocking
stream, median of the rounds after a warm-up, min-max in brackets.  Next to it its HBM floor -- the bytes the kernel must move (72 B
of full-resolution guides read and 32 B written per pixel, 104 B read per low-resolution pixel) over the bandwidth of a
device-to-device copy measured here -- the feature passes and the render of the low-resolution frame.
Then the whole frame: Renderer.render_upsampled next to Renderer.render_denoised at full resolution with the same spp and next to
render_denoised with spp / s^2 (the equal-budget render), wall clock around the synchronous calls, each with its RMS in 8-bit levels
against a --ref-spp frame of another seed.  Recorded in DESIGN.md section 4, "Guided upsampling"; nothing here is asserted.
Usage: python tools/upsample_bench.py [--spp 16] [--rounds 5] [--frame 512] [--ref-spp 512] [--scenes lampshade,cornell]"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from rpt_amd import DenoiseParams, DeviceBuffer, Renderer, UpsampleParams, scenes, upsample_device  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--spp", type=int, default=16)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--frame", type=int, default=512)
ap.add_argument("--ref-spp", type=int, default=512)
ap.add_argument("--scenes", default="lampshade,cornell")
args = ap.parse_args()
SIZE = 1024
stream = torch.cuda.Stream()


def timed(job, rounds=args.rounds):
    ms = []
    for rnd in range(rounds + 1):   # round 0 warms up
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            a.record(stream)
            job()
            b.record(stream)
        b.synchronize()
        if rnd:
            ms.append(a.elapsed_time(b))
    return ms


def wall(job, rounds=args.rounds):
    ms, out = [], None
    for rnd in range(rounds + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = job()
        torch.cuda.synchronize()
        if rnd:
            ms.append(1e3 * (time.perf_counter() - t0))
    return ms, out


def fmt(ms):
    return f"{statistics.median(ms):.3f} ms [{min(ms):.3f}-{max(ms):.3f}]"


def zeros(n):
    return torch.zeros(n, dtype=torch.float64, device="cuda")


N = SIZE * SIZE
a, b = zeros(8 * N), zeros(8 * N)
copy_ms = timed(lambda: b.copy_(a))
copy_gbs = 2 * 64 * N / (statistics.median(copy_ms) * 1e6)
print(f"device-to-device copy of 64 B per pixel at {SIZE}x{SIZE} (read + written): {fmt(copy_ms)} = {copy_gbs:.0f} GB/s", flush=True)
del a, b

scene, cam, cfg = scenes.lampshade()
hi_r = Renderer(scene, cam).width(SIZE).height(SIZE).max_bounces(cfg["max_bounces"]).seed(1)
hi_planes = [zeros(3 * N) for _ in range(3)]
out, out_var = zeros(3 * N), zeros(N)
torch.cuda.synchronize()
guide_ms = timed(lambda: hi_r.features_device(1, *[p.data_ptr() for p in hi_planes], stream_ptr=stream.cuda_stream, sample_offset=0))
print(f"lampshade {SIZE}x{SIZE}: full-resolution feature planes of 1 sample {fmt(guide_ms)}", flush=True)
for s in (2, 4):
    w = SIZE // s
    n = w * w
    lo_r = Renderer(scene, cam).width(w).height(w).max_bounces(cfg["max_bounces"]).seed(1)
    lo_planes = [zeros(3 * n) for _ in range(3)]
    frame, rgb, var = zeros(3 * n), zeros(3 * n), zeros(n)
    torch.cuda.synchronize()

    def render():
        lo_r._sample_offset = 0
        lo_r.sample_device(args.spp, frame.data_ptr(), stream.cuda_stream)

    render_ms = timed(render)
    feature_ms = timed(lambda: lo_r.features_device(args.spp, *[p.data_ptr() for p in lo_planes], stream_ptr=stream.cuda_stream, sample_offset=0))
    buf = DeviceBuffer(w, w)
    lo_r._sample_offset = 0
    for _ in range(4):
        lo_r.sample(args.spp // 4, buf)
    torch.cuda.synchronize()
    buf.mean_device(rgb.data_ptr(), var.data_ptr(), stream.cuda_stream)
    torch.cuda.synchronize()
    print(f"lampshade {w}x{w}x{args.spp} (s = {s}): render {fmt(render_ms)}; low-resolution feature planes {fmt(feature_ms)}", flush=True)
    nbytes = 104 * N + 104 * n
    for r in (1, 2):
        p = UpsampleParams(scale=s, radius=r)
        ms = timed(lambda: upsample_device(w, w, rgb.data_ptr(), var.data_ptr(), *[q.data_ptr() for q in lo_planes], *[q.data_ptr() for q in hi_planes],
                                           out.data_ptr(), out_var.data_ptr(), params=p, stream_ptr=stream.cuda_stream))
        med = statistics.median(ms)
        print(f"  upsample {w}x{w} -> {SIZE}x{SIZE}, r = {r}: {fmt(ms)}; floor {nbytes / 1e6:.1f} MB / {copy_gbs:.0f} GB/s = {nbytes / (copy_gbs * 1e6):.3f} ms "
              f"({nbytes / (med * 1e6):.0f} GB/s achieved, {100.0 * nbytes / (copy_gbs * 1e6) / med:.0f} % of the copy's rate); "
              f"output mean {float(out.mean()):.6f}, input mean {float(rgb.mean()):.6f}", flush=True)
    buf.close()

# ---- the whole frame
F = args.frame
for name in args.scenes.split(","):
    scene, cam, cfg = getattr(scenes, name)()
    make = lambda size, seed, spp: Renderer(scene, cam).width(size).height(size).max_bounces(cfg["max_bounces"]).seed(seed).num_samples(spp)  # noqa: E731
    converged = make(F, 1234, args.ref_spp).render().astype(np.float64)
    rms = lambda img: float(np.sqrt(np.mean((img.astype(np.float64) - converged) ** 2)))  # noqa: E731
    ms, img = wall(lambda: make(F, 3, args.spp).render_denoised(4))
    full = statistics.median(ms)
    print(f"{name} {F}x{F}: render_denoised, {args.spp} spp at full resolution: {fmt(ms)}, RMS {rms(img):.2f} levels against {args.ref_spp} spp", flush=True)
    for s in (2, 4):
        ms, img = wall(lambda: make(F, 3, args.spp).render_upsampled(UpsampleParams(scale=s), 4))
        print(f"  s = {s}: render_upsampled, {args.spp} spp at {F // s}x{F // s}: {fmt(ms)} (x {full / statistics.median(ms):.2f}), RMS {rms(img):.2f}", flush=True)
        ms, img = wall(lambda: make(F, 3, args.spp).render_upsampled(UpsampleParams(scale=s, demodulate=False), 4, DenoiseParams()))
        print(f"  s = {s}: render_upsampled without demodulation, filtered at the low resolution: {fmt(ms)} (x {full / statistics.median(ms):.2f}), RMS {rms(img):.2f}",
              flush=True)
        budget = max(args.spp // (s * s), 2)
        ms, img = wall(lambda: make(F, 3, budget).render_denoised(2))
        print(f"  s = {s}: the equal-budget render: render_denoised, {budget} spp at full resolution in 2 batches: {fmt(ms)} (x {full / statistics.median(ms):.2f}), "
              f"RMS {rms(img):.2f}", flush=True)
