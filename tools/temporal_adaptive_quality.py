"""What adaptive sampling over a sequence buys per sample, on the CPU: the numpy restatement of the loop
(tests/temporal_adaptive_ref.py) on the oracle's renders, no GPU involved.  scenes.sliding_shadow(0 .. frames - 1) at 96 x 64 under its
resting camera, the settings of tests/temporal_adaptive_ref.py (2 spp per batch, 2 .. 8 batches, threshold 0.06), the default
accumulation with the motion tables of the sequence:

  adaptive   every frame sampled by the loop against the accumulator; tile-batches T_f per frame
  uniform    every frame sampled by ceil(T_f / tiles) full-frame batches (at least 2): the same samples or a few more, spread evenly

RMS, in 8-bit levels, of the accumulated last frame against the oracle's `--spp`-sample frame of the last scene with another seed,
for `--seeds` seeds, and the spread of the difference across them: the margin by which a test may let the loop be worse.
Usage: python tools/temporal_adaptive_quality.py [--frames 4] [--spp 512] [--seeds 3,4,5]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

from oracle import pyoracle  # noqa: E402
from rpt_amd import color_bytes, scenes, temporal_camera_record, temporal_motion_record  # noqa: E402
from tests import temporal_adaptive_ref as tar  # noqa: E402
from tests.adaptive_ref import RefBuffer  # noqa: E402
from tests.temporal_clip_ref import ClipRef  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=4)
ap.add_argument("--spp", type=int, default=512)
ap.add_argument("--seeds", default="3,4,5")
args = ap.parse_args()
W, H, LOOP = tar.QUALITY_W, tar.QUALITY_H, tar.QUALITY_LOOP
TILES = ((W + 31) // 32) * ((H + 31) // 32)
seq = [scenes.sliding_shadow(f) for f in range(args.frames)]
tables = [None] + [np.stack([temporal_motion_record(c.shape.matrix(), p.shape.matrix()) for c, p in zip(cur[0].objects, prev[0].objects)])
                   for prev, cur in zip(seq, seq[1:])]
oracles = [pyoracle.OracleScene(s[0]) for s in seq]
scene, cam, cfg = seq[-1]
converged = color_bytes(oracles[-1].render(cam, W, H, args.spp, cfg["max_bounces"], seed=1234, robust=1).reshape(H, W, 3))
rms = lambda a: float(np.sqrt(np.mean((color_bytes(a).astype(np.float64) - converged.astype(np.float64)) ** 2)))  # noqa: E731
diffs = []
for seed in [int(t) for t in args.seeds.split(",")]:
    ref_a, ref_u = ClipRef(W, H), ClipRef(W, H)
    spent_a = spent_u = 0
    for f, ((scene, cam, cfg), table, osc) in enumerate(zip(seq, tables, oracles)):
        rec, offset = temporal_camera_record(cam), tar.frame_offset(f)
        batch_at, planes_at = tar.oracle_frame_inputs(osc, cam, cfg["max_bounces"], W, H, seed, LOOP["spp_per_batch"], LOOP["min_batches"])
        normal, depth = planes_at(offset)
        buf, stats, _, _ = tar.adaptive_temporal_loop(batch_at, W, H, ref_a, rec, normal, depth, sample_offset=offset, motion=table, **LOOP)
        out_a, _, _ = ref_a.accumulate(rec, *buf.mean(), normal, depth, motion=table)
        n_uniform = max(LOOP["min_batches"], -(-stats[1] // TILES))
        uni = RefBuffer(W, H)
        for k in range(n_uniform):
            uni.add(batch_at(offset + k * LOOP["spp_per_batch"]))
        out_u, _, _ = ref_u.accumulate(rec, *uni.mean(), normal, depth, motion=table)
        spent_a += stats[1]
        spent_u += n_uniform * TILES
        print(f"seed {seed} frame {f}: adaptive {buf.tile_batches().reshape(-1).tolist()} = {stats[1]} tile-batches, uniform {n_uniform} batches = "
              f"{n_uniform * TILES}", flush=True)
    a, u = rms(out_a), rms(out_u)
    diffs.append(a - u)
    print(f"seed {seed}: RMS of the accumulated last frame against {args.spp} spp, adaptive {a:.3f} levels with {spent_a} tile-batches, uniform {u:.3f} with "
          f"{spent_u}; adaptive - uniform {a - u:+.3f}", flush=True)
print(f"adaptive - uniform over the seeds: mean {np.mean(diffs):+.3f}, min {min(diffs):+.3f}, max {max(diffs):+.3f}, spread {max(diffs) - min(diffs):.3f} levels")
