"""The quality conditions of the guided upsampling, on the CPU: the numpy restatement of the definition (tests/upsample_ref.py) on the
oracle's renders, no GPU involved.  scenes.lampshade() (scenes.spheres() renders black under the reference's semantics and can show
nothing; --scene takes any committed scene) at 64 x 48, 4 batches x 4 spp; feature planes from the oracle's closest hits: the
low-resolution ones of the same 16 camera samples, the full-resolution ones of one sample.  For every scale x radius x sigma_normal x
sigma_depth of the grid: the share of full-resolution pixels that take the fallback, and the RMS, in 8-bit levels, of the upsampled
frame against the oracle's --spp frame at full resolution with another seed, next to that of plain s x s replication of the same
low-resolution frame.  tests/test_upsample_host.py asserts both conditions for s = 2 with the defaults; DESIGN.md section 4, "Guided
upsampling", records the grid.
Usage: python tools/upsample_quality.py [--scene lampshade] [--spp 512] [--scales 2,3,4]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

from oracle import pyoracle  # noqa: E402
from rpt_amd import color_bytes, scenes  # noqa: E402
from tests.upsample_ref import mean_and_variance, oracle_planes, replicate, upsample_ref  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--scene", default="lampshade")
ap.add_argument("--spp", type=int, default=512)
ap.add_argument("--scales", default="2,3,4")
args = ap.parse_args()
w, h = 64, 48
BATCHES, SPP, SEED = 4, 4, 3

scene, cam, cfg = getattr(scenes, args.scene)()
osc = pyoracle.OracleScene(scene)
batches = [osc.render(cam, w, h, SPP, cfg["max_bounces"], seed=SEED, sample_offset=k * SPP, robust=1) for k in range(BATCHES)]
mean, var = mean_and_variance(batches)
mean, var = mean.reshape(h, w, 3), var.reshape(h, w)
lo = oracle_planes(osc, scene, cam, w, h, BATCHES * SPP, SEED)
for s in [int(v) for v in args.scales.split(",")]:
    W, H = s * w, s * h
    hi = oracle_planes(osc, scene, cam, W, H, 1, SEED)
    converged = color_bytes(osc.render(cam, W, H, args.spp, cfg["max_bounces"], seed=1234, robust=1).reshape(H, W, 3)).astype(np.float64)
    rms = lambda a: float(np.sqrt(np.mean((color_bytes(a).astype(np.float64) - converged) ** 2)))  # noqa: E731
    print(f"{args.scene} {w} x {h} -> {W} x {H}, {BATCHES} x {SPP} spp against {args.spp} spp: replication RMS {rms(replicate(mean, s)):.2f} levels",
          flush=True)
    for r in (1, 2):
        for sn in (0.0, 0.25, 0.5, 1.0):
            for sd in (0.0, 0.05, 0.2):
                for flags in (3, 0) if (sn, sd) == (0.5, 0.0) else (3,):
                    out, _, fb = upsample_ref(mean, var, *lo, *hi, scale=s, radius=r, flags=flags, sigma_normal=sn, sigma_depth=sd,
                                              return_fallback=True)
                    print(f"  s {s} r {r} flags {flags} sigma_normal {sn:4.2f} sigma_depth {sd:4.2f}: fallback {100.0 * fb.mean():5.2f} %, "
                          f"RMS {rms(out):.2f}", flush=True)
