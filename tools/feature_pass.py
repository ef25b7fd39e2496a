"""Time of the first-hit feature pass (Renderer.features_device) next to the renders of the same samples, on C3's and C5's scenes at
1024 x 1024 x 16: one line per scene with the pass, the render at max_bounces = 0 and the render at the scene's own max_bounces,
each timed with HIP events around its stream, after a warm-up of each, the three alternating.
Usage: python tools/feature_pass.py [--size 1024] [--spp 16] [--rounds 5] [--epsilon]"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from rpt_amd import Renderer, scenes  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, default=1024)
ap.add_argument("--spp", type=int, default=16)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--epsilon", action="store_true", help="the reference-epsilon mode")
args = ap.parse_args()

n = args.size * args.size * 3
for name in ("C3", "C5"):
    scene, cam, cfg = scenes.CONFIGS[name]()
    if args.epsilon:
        scene.set_option("epsilon_policy", 1)
    stream = torch.cuda.Stream()
    frame = torch.zeros(n, dtype=torch.float64, device="cuda")
    planes = [torch.zeros(n, dtype=torch.float64, device="cuda") for _ in range(3)]

    def renderer(bounces):
        return Renderer(scene, cam).width(args.size).height(args.size).max_bounces(bounces).seed(1)

    direct, full = renderer(0), renderer(cfg["max_bounces"])

    def run_pass():
        direct.features_device(args.spp, *[p.data_ptr() for p in planes], stream_ptr=stream.cuda_stream, sample_offset=0)

    def run_render(r):
        r._sample_offset = 0
        r.sample_device(args.spp, frame.data_ptr(), stream.cuda_stream)

    jobs = {"features": run_pass, "render, max_bounces 0": lambda: run_render(direct),
            f"render, max_bounces {cfg['max_bounces']}": lambda: run_render(full)}
    times = {k: [] for k in jobs}
    for rnd in range(args.rounds + 1):   # round 0 warms every kernel up
        for k, job in jobs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(stream):
                a.record(stream)
                job()
                b.record(stream)
            b.synchronize()
            if rnd:
                times[k].append(a.elapsed_time(b))
    cov = float(planes[2].view(-1, 3)[:, 1].mean())
    print(f"{name} {args.size}x{args.size}x{args.spp}{' reference-epsilon' if args.epsilon else ''} (coverage {cov:.3f}): " + "; ".join(
        f"{k} {statistics.median(v):.3f} ms (min {min(v):.3f}, max {max(v):.3f})" for k, v in times.items()), flush=True)
