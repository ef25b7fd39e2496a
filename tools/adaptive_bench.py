"""Time and error of adaptive sampling by tile (Renderer.sample_adaptive) on C3's and C5's frames at 1024 x 1024, next to the uniform
render of max_batches * spp_per_batch samples in the same batches: the time of each, the share of tile-batches the adaptive render
traced, the RMS of each mean frame against a uniform render of 8 x as many samples under another seed, and the refine step alone
(tile errors + selection + the 4-byte read-back) next to the tile-list render of the round it selects.  HIP events on the default
stream (the loop runs there), median of the rounds after a warm-up, min-max in brackets.
Usage: python tools/adaptive_bench.py [--size 1024] [--spp 4] [--min 4] [--max 16] [--threshold 0.05 0.1] [--floor 0.05] [--rounds 3]"""
import argparse
import ctypes as C
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from rpt_amd import AdaptiveParams, DeviceBuffer, Renderer, _lib, scenes  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, default=1024)
ap.add_argument("--spp", type=int, default=4)
ap.add_argument("--min", type=int, default=4)
ap.add_argument("--max", type=int, default=16)
ap.add_argument("--threshold", type=float, nargs="+", default=[0.05, 0.1])
ap.add_argument("--floor", type=float, default=0.05)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--workloads", nargs="+", default=["C3", "C5"])
args = ap.parse_args()

n = args.size * args.size
total = args.max * args.spp


def timed(job, rounds=args.rounds):
    ms = []
    for rnd in range(rounds + 1):   # round 0 warms up
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        job(rnd)
        b.record()
        b.synchronize()
        if rnd:
            ms.append(a.elapsed_time(b))
    return ms


def fmt(ms):
    return f"{statistics.median(ms):.3f} ms [{min(ms):.3f}-{max(ms):.3f}]"


def rms(a, b):
    return float(np.sqrt(np.mean((a - b) ** 2)))


for name in args.workloads:
    scene, cam, cfg = scenes.CONFIGS[name]()
    make = lambda seed: Renderer(scene, cam).width(args.size).height(args.size).max_bounces(cfg["max_bounces"]).seed(seed)  # noqa: E731
    r = make(1)
    # the yardstick: 8 x the samples, another seed
    ref = make(1234).sample_array(8 * total).reshape(args.size, args.size, 3)

    def uniform(buf):
        r._sample_offset = 0
        for _ in range(args.max):
            r.sample(args.spp, buf)

    bufs = [DeviceBuffer(args.size, args.size) for _ in range(args.rounds + 1)]
    torch.cuda.synchronize()
    uniform_ms = timed(lambda rnd: uniform(bufs[rnd]))
    uniform_rms = rms(bufs[-1].mean()[0], ref)
    for b in bufs:
        b.close()
    print(f"{name} {args.size}x{args.size}: uniform {args.max} batches x {args.spp} spp: {fmt(uniform_ms)}; RMS against {8 * total} spp {uniform_rms:.5f}",
          flush=True)
    for thr in args.threshold:
        p = AdaptiveParams(args.spp, args.min, args.max, thr, args.floor)
        bufs = [DeviceBuffer(args.size, args.size) for _ in range(args.rounds + 1)]
        stats = []
        torch.cuda.synchronize()
        adaptive_ms = timed(lambda rnd: stats.append(r.sample_adaptive(p, bufs[rnd])))
        counts = bufs[-1].tile_batches()
        s = stats[-1]
        print(f"  {name} threshold {thr}, floor {args.floor}, min {args.min}: adaptive {fmt(adaptive_ms)} = {statistics.median(adaptive_ms) / statistics.median(uniform_ms):.3f} "
              f"of uniform; {s[0]} rounds, {s[1]} of {args.max * s[3]} tile-batches ({s[1] / (args.max * s[3]):.3f}), {s[2]} of {s[3]} tiles at max_batches, "
              f"mean {counts.mean():.2f} batches per tile; RMS against {8 * total} spp {rms(bufs[-1].mean()[0], ref):.5f}", flush=True)
        for b in bufs:
            b.close()
    # the refine step alone after min_batches, and the tile-list render of the round it selects
    p = AdaptiveParams(args.spp, args.min, args.max, args.threshold[0], args.floor)
    buf = DeviceBuffer(args.size, args.size)
    r._sample_offset = 0
    for _ in range(args.min):
        r.sample(args.spp, buf)
    tx, ty = buf.tiles
    d_ids = torch.zeros(tx * ty, dtype=torch.int32, device="cuda")
    frame = torch.zeros(3 * n, dtype=torch.float64, device="cuda")
    count = C.c_uint32()
    desc = p.desc()
    torch.cuda.synchronize()
    lib = _lib.load()
    refine_ms = timed(lambda rnd: _lib.check(lib.rpt_buffer_refine_tiles(buf._h, C.byref(desc), C.c_void_p(d_ids.data_ptr()), C.byref(count), None, None)),
                      rounds=max(args.rounds, 10))

    def round_render(rnd):
        r._sample_offset = args.min * args.spp
        r.sample_tiles_device(args.spp, d_ids.data_ptr(), count.value, frame.data_ptr())

    round_ms = timed(round_render)
    r._sample_offset = args.min * args.spp
    full_ms = timed(lambda rnd: (setattr(r, "_sample_offset", args.min * args.spp), r.sample_device(args.spp, frame.data_ptr())))
    print(f"  {name} refine (errors of {tx * ty} tiles + selection + read-back) {fmt(refine_ms)}; the round it selects, {count.value} of {tx * ty} tiles x "
          f"{args.spp} spp: {fmt(round_ms)}; a full frame x {args.spp} spp: {fmt(full_ms)}", flush=True)
    buf.close()
