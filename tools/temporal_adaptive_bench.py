"""Cost and saving of adaptive sampling over a sequence (rpt_render_adaptive_temporal), after tools/adaptive_bench.py and
tools/temporal_clip_bench.py: an 8-frame sequence of scenes.sliding_shadow (the cube moves, the camera rests) at 1024 x 1024 and
512 x 512, every frame finished by DeviceBuffer.temporal_image, three ways of sampling a frame:

  temporal loop     Renderer.sample_adaptive_temporal against the sequence's accumulator (the new path)
  plain loop        Renderer.sample_adaptive, the frame's own error (the parent's path)
  uniform           max_batches full-frame batches (the parent's path)

Per way: the tile-batches of every frame and the wall time of a frame (features + sampling + temporal_image, synchronised), the median
over the rounds with min-max in brackets after a warm-up round.  Then the two kernels of a round alone, HIP events around `--calls`
calls back to back: the preview over every tile and the tile errors of planes, next to their HBM floor (bytes moved over the 8 TB/s
bench.py's roofline uses: preview 24 rgb + 8 var + 24 normal + 24 depth + 80 one history record + 40 outputs = 200 B per pixel; tile
errors 32 B per pixel) and next to the render time of one tile batch (a full-frame batch of spp_per_batch samples over the tiles).
No figure here is a pass mark; DESIGN.md section 4 records them with the commit they were taken on.
Usage: python tools/temporal_adaptive_bench.py [--sizes 1024x1024,512x512] [--frames 8] [--rounds 3] [--calls 20]"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from rpt_amd import AdaptiveParams, DeviceBuffer, Renderer, TemporalAccumulator, TemporalParams, _lib, scenes, temporal_motion_record  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", default="1024x1024,512x512")
ap.add_argument("--frames", type=int, default=8)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--calls", type=int, default=20)
ap.add_argument("--threshold", type=float, default=0.05)
args = ap.parse_args()
HBM_PEAK_GBS = 8000.0
PREVIEW_BYTES, ERROR_BYTES = 200, 32
PARAMS = AdaptiveParams(spp_per_batch=4, min_batches=2, max_batches=8, threshold=args.threshold, floor=0.05)
SPAN = PARAMS.max_batches * PARAMS.spp_per_batch
TEMPORAL = TemporalParams()
stream = torch.cuda.Stream()


def fmt(ms):
    return f"{statistics.median(ms):.3f} ms [{min(ms):.3f}-{max(ms):.3f}]"


def zeros(k):
    return torch.zeros(k, dtype=torch.float64, device="cuda")


def timed(job, calls):
    ms = []
    for rnd in range(args.rounds + 1):   # round 0 warms up
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            a.record(stream)
            for _ in range(calls):
                job()
            b.record(stream)
        b.synchronize()
        if rnd:
            ms.append(a.elapsed_time(b) / calls)
    return ms


def tables_of(seq):
    return [None] + [np.stack([temporal_motion_record(c.shape.matrix(), p.shape.matrix()) for c, p in zip(cur[0].objects, prev[0].objects)])
                     for prev, cur in zip(seq, seq[1:])]


def run_sequence(way, seq, tables, w, h, planes):
    """-> (per frame wall ms, per frame tile-batches)"""
    acc = TemporalAccumulator(w, h)
    ptrs = [p.data_ptr() for p in planes]
    named = dict(zip(("albedo", "normal", "depth"), ptrs))
    tiles = ((w + 31) // 32) * ((h + 31) // 32)
    ms, batches = [], []
    for f, ((scene, cam, cfg), table) in enumerate(zip(seq, tables)):
        r = Renderer(scene, cam).width(w).height(h).max_bounces(cfg["max_bounces"]).seed(3)
        buf = DeviceBuffer(w, h)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        acc.set_motion(table)
        if way == "temporal loop":
            r.features_device(PARAMS.min_batches * PARAMS.spp_per_batch, *ptrs, sample_offset=f * SPAN)
            stats = r.sample_adaptive_temporal(PARAMS, buf, acc, {"normal": ptrs[1], "depth": ptrs[2]}, TEMPORAL, sample_offset=f * SPAN)
        elif way == "plain loop":
            r.features_device(PARAMS.min_batches * PARAMS.spp_per_batch, *ptrs, sample_offset=0)
            stats = r.sample_adaptive(PARAMS, buf)
        else:
            r.features_device(SPAN, *ptrs, sample_offset=f * SPAN)
            r._sample_offset = f * SPAN
            for _ in range(PARAMS.max_batches):
                r.sample(PARAMS.spp_per_batch, buf)
            stats = (0, PARAMS.max_batches * tiles, tiles, tiles)
        buf.temporal_image(acc, cam, named, TEMPORAL)
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
        batches.append(int(stats[1]))
        buf.close()
    acc.close()
    return ms, batches


print(f"library {_lib.LIB_PATH}", flush=True)
for size in args.sizes.split(","):
    w, h = [int(t) for t in size.split("x")]
    n = w * h
    tiles = ((w + 31) // 32) * ((h + 31) // 32)
    seq = [scenes.sliding_shadow(f) for f in range(args.frames)]
    tables = tables_of(seq)
    planes = [zeros(3 * n) for _ in range(3)]
    torch.cuda.synchronize()
    print(f"sliding_shadow {w}x{h}, {args.frames} frames, {tiles} tiles, spp_per_batch {PARAMS.spp_per_batch}, batches {PARAMS.min_batches}..{PARAMS.max_batches}, "
          f"threshold {PARAMS.threshold}", flush=True)
    for way in ("temporal loop", "plain loop", "uniform"):
        rounds = [run_sequence(way, seq, tables, w, h, planes) for _ in range(args.rounds + 1)][1:]   # round 0 warms up (commits, JIT)
        per_frame = [fmt([rnd[0][f] for rnd in rounds]) for f in range(args.frames)]
        total = [sum(rnd[0]) for rnd in rounds]
        print(f"  {way}: sequence {fmt(total)}; tile-batches per frame {rounds[-1][1]}, sum {sum(rounds[-1][1])}", flush=True)
        print(f"    per frame: {'; '.join(per_frame)}", flush=True)
    # the two kernels of a round alone, on the last frame's planes behind one accumulated frame
    scene, cam, cfg = seq[-1]
    r = Renderer(scene, cam).width(w).height(h).max_bounces(cfg["max_bounces"]).seed(3)
    r.features_device(8, *[p.data_ptr() for p in planes], sample_offset=0)
    buf = DeviceBuffer(w, h)
    for _ in range(2):
        r.sample(PARAMS.spp_per_batch, buf)
    rgb, var, out, out_var, err = zeros(3 * n), zeros(n), zeros(3 * n), zeros(n), zeros(tiles)
    ids = torch.arange(tiles, dtype=torch.int32, device="cuda")
    frame = zeros(3 * n)
    torch.cuda.synchronize()
    buf.mean_device(rgb.data_ptr(), var.data_ptr())
    acc = TemporalAccumulator(w, h)
    acc.accumulate_device(cam, rgb.data_ptr(), var.data_ptr(), planes[1].data_ptr(), planes[2].data_ptr(), out.data_ptr(), out_var.data_ptr())
    torch.cuda.synchronize()
    lib, C = _lib.load(), __import__("ctypes")
    for what, d_tiles, n_tiles in (("every tile (the frame's grid)", 0, 0), ("a list of every tile", ids.data_ptr(), tiles)):
        pv = timed(lambda: acc.preview_device(cam, rgb.data_ptr(), var.data_ptr(), planes[1].data_ptr(), planes[2].data_ptr(), out.data_ptr(),
                                              out_var.data_ptr(), 0, TEMPORAL, d_tiles, n_tiles, stream.cuda_stream), args.calls)
        te = timed(lambda: _lib.check(lib.rpt_temporal_tile_errors_device(acc._h, C.c_void_p(out.data_ptr()), C.c_void_p(out_var.data_ptr()), 0.05,
                                                                          C.c_void_p(d_tiles or None), n_tiles, C.c_void_p(err.data_ptr()),
                                                                          C.c_void_p(stream.cuda_stream))), args.calls)
        print(f"  preview, {what}: {fmt(pv)}, floor {n * PREVIEW_BYTES / (HBM_PEAK_GBS * 1e6):.4f} ms; tile errors: {fmt(te)}, "
              f"floor {n * ERROR_BYTES / (HBM_PEAK_GBS * 1e6):.4f} ms", flush=True)
    batch = timed(lambda: r.sample_tiles_device(PARAMS.spp_per_batch, ids.data_ptr(), tiles, frame.data_ptr(), stream.cuda_stream), 4)
    print(f"  one batch of {PARAMS.spp_per_batch} spp over every tile: {fmt(batch)} = {statistics.median(batch) / tiles * 1e3:.3f} us per tile batch; a round's "
          f"two kernels cost {(statistics.median(pv) + statistics.median(te)) / statistics.median(batch) * tiles:.2f} tile batches", flush=True)
    acc.close()
    buf.close()
    for s in seq:
        s[0].close()
