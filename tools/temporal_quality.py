"""The quality condition of the temporal accumulation, on the CPU: the numpy restatement of the definition (tests/temporal_ref.py) on
the oracle's renders, no GPU involved.  Eight frames of 4 batches x 1 spp on a small arc (the cameras of tests/test_gpu_temporal.py),
cornell and lampshade at 64 x 64; feature planes from the oracle's closest hits of the same camera samples; RMS, in 8-bit levels, of
the last accumulated frame against the oracle's 512-spp frame at the last camera with another seed, next to that of the last frame
alone, and the same pair behind the a-trous filter (tests/denoise_ref.py).  tests/test_gpu_temporal.py asserts the first ratio < 1
for the device and prints all four figures; DESIGN.md section 4, "Temporal accumulation", records both.
Usage: python tools/temporal_quality.py [--size 64] [--frames 8] [--spp 512]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

from oracle import pyoracle  # noqa: E402
from rpt_amd import color_bytes, scenes, temporal_camera_record  # noqa: E402
from tests.denoise_ref import denoise_ref  # noqa: E402
from tests.temporal_ref import TemporalRef, arc_cameras  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, default=64)
ap.add_argument("--frames", type=int, default=8)
ap.add_argument("--spp", type=int, default=512)
args = ap.parse_args()
W = H = args.size
BATCHES, SEED = 4, 3


def planes_of(osc, scene, cam, offset):
    """albedo, normal, depth of the BATCHES camera samples from `offset` on, as rpt_render_features defines them."""
    colors = np.array([o.material_.color() for o in scene.objects], dtype=np.float64).reshape(-1, 3)
    acc, first = np.zeros((W * H, 8)), None
    for s in range(BATCHES):
        cs = pyoracle.camera_rays(cam, W, H, sample=offset + s, seed=SEED)
        t, obj, nrm = osc.intersect(cs["o"], cs["d"], robust=1)
        hit = obj >= 0
        a = np.zeros((W * H, 3))
        a[hit] = colors[obj[hit]]
        if not hit.all():
            a[~hit] = osc.env_color(cs["d"][~hit])
        acc += np.concatenate([a, np.where(hit[:, None], nrm, 0.0), np.where(hit, t, 0.0)[:, None], hit[:, None].astype(np.float64)], axis=1)
        first = obj if first is None else first
    mean = acc / float(BATCHES)
    depth = np.stack([mean[:, 6], mean[:, 7], (first + 1).astype(np.float64)], axis=1)
    return mean[:, 0:3].reshape(H, W, 3), mean[:, 3:6].reshape(H, W, 3), depth.reshape(H, W, 3)


for name in ("cornell", "lampshade"):
    scene, cam, cfg = getattr(scenes, name)()
    osc = pyoracle.OracleScene(scene)
    cams = arc_cameras(cam, args.frames, 1080.0)
    ref, ref2 = TemporalRef(W, H), TemporalRef(W, H)
    for f, c in enumerate(cams):
        off = f * BATCHES
        batches = [osc.render(c, W, H, 1, cfg["max_bounces"], seed=SEED, sample_offset=off + k, robust=1) for k in range(BATCHES)]
        total, sumsq = np.zeros((W * H, 3)), np.zeros(W * H)
        for b in batches:
            total = total + b
            sumsq = sumsq + ((b[:, 0] * b[:, 0] + b[:, 1] * b[:, 1]) + b[:, 2] * b[:, 2])
        fn = float(BATCHES)
        mean = total / fn
        var = np.fmax(sumsq - fn * ((mean[:, 0] * mean[:, 0] + mean[:, 1] * mean[:, 1]) + mean[:, 2] * mean[:, 2]), 0.0) / (fn - 1.0) / fn
        mean, var = mean.reshape(H, W, 3), var.reshape(H, W)
        albedo, normal, depth = planes_of(osc, scene, c, off)
        out, out_v, length = ref.accumulate(temporal_camera_record(c), mean, var, normal, depth)
        print(f"{name} frame {f}: {int(ref.last['took'].sum())} of {int(ref.last['hit'].sum())} hit pixels take history, mean len {length.mean():.2f}",
              flush=True)
    converged = color_bytes(osc.render(cams[-1], W, H, args.spp, cfg["max_bounces"], seed=1234, robust=1).reshape(H, W, 3))
    rms = lambda a: float(np.sqrt(np.mean((color_bytes(a).astype(np.float64) - converged.astype(np.float64)) ** 2)))  # noqa: E731
    filtered, _ = denoise_ref(mean, var, albedo, normal, depth)
    both, _ = denoise_ref(out, out_v, albedo, normal, depth)
    print(f"quality (CPU: oracle + restatement), {name} {W} x {H}, {args.frames} frames of {BATCHES} x 1 spp against {args.spp} spp: "
          f"RMS {rms(mean):.2f} -> {rms(out):.2f} levels, ratio {rms(out) / rms(mean):.3f}; denoise alone {rms(filtered):.2f}, "
          f"accumulate + denoise {rms(both):.2f}, ratio {rms(both) / rms(filtered):.3f}", flush=True)
