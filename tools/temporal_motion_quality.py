"""The quality condition of the temporal accumulation with moving objects, on the CPU: the numpy restatement of the definition
(tests/temporal_motion_ref.py) on the oracle's renders, no GPU involved.  Eight frames of 4 batches x 1 spp of the sequence of
examples/simple_video.rs as tests/test_gpu_temporal_motion.py renders it (scenes.simple_video(1 + f, 0.25), 64 x 48, the default
camera): feature planes from the oracle's closest hits of the same camera samples, the motion table of frame f from the matrices
of scenes f and f - 1; RMS, in 8-bit levels and over the cube's pixels, of the last accumulated frame against the oracle's 512-spp
frame of the last scene with another seed, next to that of the last frame alone -- with the table and, recorded only, without one (a
one-colour object hides misplaced history).  tests/test_gpu_temporal_motion.py asserts the first ratio < 1 for the device;
DESIGN.md section 4, "Moving objects", records the figures.
Usage: python tools/temporal_motion_quality.py [--frames 8] [--spp 512]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

from oracle import pyoracle  # noqa: E402
from rpt_amd import color_bytes, scenes, temporal_camera_record, temporal_motion_record  # noqa: E402
from tests.temporal_motion_ref import MotionRef  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=8)
ap.add_argument("--spp", type=int, default=512)
args = ap.parse_args()
W, H = 64, 48
FIRST, STEP = 1, 0.25
BATCHES, SEED = 4, 3


def planes_of(osc, scene, cam, offset):
    """normal, depth of the BATCHES camera samples from `offset` on, as rpt_render_features defines them."""
    acc, first = np.zeros((W * H, 5)), None
    for s in range(BATCHES):
        cs = pyoracle.camera_rays(cam, W, H, sample=offset + s, seed=SEED)
        t, obj, nrm = osc.intersect(cs["o"], cs["d"], robust=1)
        hit = obj >= 0
        acc += np.concatenate([np.where(hit[:, None], nrm, 0.0), np.where(hit, t, 0.0)[:, None], hit[:, None].astype(np.float64)], axis=1)
        first = obj if first is None else first
    mean = acc / float(BATCHES)
    depth = np.stack([mean[:, 3], mean[:, 4], (first + 1).astype(np.float64)], axis=1)
    return mean[:, 0:3].reshape(H, W, 3), depth.reshape(H, W, 3)


with_table, without, prev = MotionRef(W, H), MotionRef(W, H), None
for f in range(args.frames):
    scene, cam, cfg = scenes.simple_video(FIRST + f, STEP)
    osc = pyoracle.OracleScene(scene)
    off = f * BATCHES
    batches = [osc.render(cam, W, H, 1, cfg["max_bounces"], seed=SEED, sample_offset=off + k, robust=1) for k in range(BATCHES)]
    total, sumsq = np.zeros((W * H, 3)), np.zeros(W * H)
    for b in batches:
        total = total + b
        sumsq = sumsq + ((b[:, 0] * b[:, 0] + b[:, 1] * b[:, 1]) + b[:, 2] * b[:, 2])
    fn = float(BATCHES)
    mean = total / fn
    var = np.fmax(sumsq - fn * ((mean[:, 0] * mean[:, 0] + mean[:, 1] * mean[:, 1]) + mean[:, 2] * mean[:, 2]), 0.0) / (fn - 1.0) / fn
    mean, var = mean.reshape(H, W, 3), var.reshape(H, W)
    normal, depth = planes_of(osc, scene, cam, off)
    table = None
    if prev is not None:
        table = np.stack([temporal_motion_record(c.shape.matrix(), p.shape.matrix()) for c, p in zip(scene.objects, prev.objects)])
    rec = temporal_camera_record(cam)
    out, _, _ = with_table.accumulate(rec, mean, var, normal, depth, motion=table)
    blind, _, _ = without.accumulate(rec, mean, var, normal, depth)
    cube = depth[..., 2] == 2.0
    print(f"frame {f}: cube {int(cube.sum())} pixels; took history with the table {int((with_table.last['took'] & cube).sum())}, "
          f"without {int((without.last['took'] & cube).sum())}", flush=True)
    prev = scene
converged = color_bytes(osc.render(cam, W, H, args.spp, cfg["max_bounces"], seed=1234, robust=1).reshape(H, W, 3))
rms = lambda a: float(np.sqrt(np.mean((color_bytes(a).astype(np.float64) - converged.astype(np.float64))[cube] ** 2)))  # noqa: E731
print(f"quality (CPU: oracle + restatement), simple_video {W} x {H}, {args.frames} frames of {BATCHES} x 1 spp against {args.spp} spp over the "
      f"cube's {int(cube.sum())} pixels: RMS {rms(mean):.2f} -> {rms(out):.2f} levels with the table, ratio {rms(out) / rms(mean):.3f}; "
      f"without a table {rms(blind):.2f}, ratio {rms(blind) / rms(mean):.3f}", flush=True)
