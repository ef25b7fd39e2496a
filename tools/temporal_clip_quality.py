"""The quality measurement of the history clipping (RPT_TEMPORAL_CLIP), on the CPU: the numpy restatement of the definition
(tests/temporal_clip_ref.py) on the oracle's renders, no GPU involved.  For scenes.sliding_shadow and scenes.moving_light: eight frames
of 4 batches x 1 spp at 64 x 48 with seed 3, motion tables from the scenes' matrices; the reference is the oracle's 512-spp frame of the
last scene with another seed.  "Static" pixels keep one id in all frames, not the cube's or the light's; "changed" pixels are static
pixels whose 512-spp frame differs by >= 16 levels in some channel from the 512-spp frame two scenes earlier.  Prints the RMS, in 8-bit
levels, over both masks for the last frame alone, the accumulation without the flag, and with it over the grid
r in {1, 2, 3} x gamma in {0.25, 0.5, 1, 1.5} x clip_history in {0, 1, 3}, and marks the grid points that meet the three conditions
tests/test_temporal_clip_host.py and tests/test_gpu_temporal_clip.py assert at the defaults.  DESIGN.md section 4, "History
clipping", records the output.
Usage: python tools/temporal_clip_quality.py [--spp 512]"""
import argparse
import itertools
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from rpt_amd import scenes  # noqa: E402
from tests.temporal_clip_ref import oracle_sequence, quality_rows  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--spp", type=int, default=512)
args = ap.parse_args()
GRID = list(itertools.product((1, 2, 3), (0.25, 0.5, 1.0, 1.5), (0, 1, 3)))

results = {}
for name, fn in (("sliding_shadow", scenes.sliding_shadow), ("moving_light", scenes.moving_light)):
    frames, converged, earlier = oracle_sequence(fn, args.spp)
    n_static, n_changed, rows = quality_rows(frames, converged, earlier, GRID)
    results[name] = (n_changed, rows)
    print(f"{name}: {n_static} static pixels, {n_changed} changed; RMS in 8-bit levels against {args.spp} spp (changed, static)")
    print(f"  last frame alone        {rows['alone'][0]:6.2f} {rows['alone'][1]:6.2f}")
    print(f"  accumulated, no flag    {rows['plain'][0]:6.2f} {rows['plain'][1]:6.2f}")
    for s in GRID:
        c, st = rows[s]
        ok = n_changed >= 30 and c < rows["plain"][0] and st < rows["plain"][1] and st < rows["alone"][1]
        print(f"  r {s[0]} gamma {s[1]:4.2f} history {s[2]}  {c:6.2f} {st:6.2f}  {'ok' if ok else 'misses a condition'}", flush=True)


def meets(s):
    return all(n >= 30 and rows[s][0] < rows["plain"][0] and rows[s][1] < rows["plain"][1] and rows[s][1] < rows["alone"][1]
               for n, rows in results.values())


good = [s for s in GRID if meets(s)]
total = lambda s: sum(rows[s][0] for _, rows in results.values())  # noqa: E731
print(f"{len(good)} of {len(GRID)} grid points meet the three conditions on both scenes; the defaults (1, 0.5, 1): {'yes' if meets((1, 0.5, 1)) else 'NO'}")
if good:
    best = min(good, key=total)
    print(f"smallest sum of the two changed-mask RMS among them: r {best[0]} gamma {best[1]} history {best[2]}: {total(best):.2f}"
          f" (the defaults: {total((1, 0.5, 1)):.2f})")
