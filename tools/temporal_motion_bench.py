"""Time of the temporal accumulation with a motion table, after tools/temporal_bench.py: TemporalAccumulator.accumulate_device alone
on C3's frame at 1024 x 1024, default parameters, the frame 4 batches x 4 spp in a DeviceBuffer with the feature planes of the 16
samples, two cameras a small step apart alternating so that every timed call reprojects.  HIP events around the stream, a warm-up
round, then the median of the rounds with min-max in brackets; a round is `--calls` calls back to back, divided by their number.

  no table          the kernel's first instantiation, the one every call took before there were tables
  identity table    one identity record per object (set_motion_device before every call: the table is one-shot)
  moving table      every object shifted by 0.3 pixel (at the eye's distance from the origin) along the camera's right
  moving, host      the same table through set_motion: the call uploads its 192 bytes per object on the stream first

The floor of the pass (240 B per pixel over the HBM peak) is tools/temporal_bench.py's; the table adds 21 loads per lane, which a
wave's lanes share (one or two ids per wave), and 21 multiplies.
--no-table measures the first line alone and needs none of the motion entry points: with RPT_LIB set to a library built from the
commit before them it gives that commit's figure, and the two are alternated in one sitting.
Usage: [RPT_LIB=...] python tools/temporal_motion_bench.py [--no-table] [--size 1024] [--spp 16] [--rounds 5] [--calls 20]"""
import argparse
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, default=1024)
ap.add_argument("--spp", type=int, default=16)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--calls", type=int, default=20)
ap.add_argument("--no-table", action="store_true")
args = ap.parse_args()

from rpt_amd import _lib  # noqa: E402

if args.no_table:   # a library from before the motion entry points loads too
    _lib.SYMBOLS[:] = [s for s in _lib.SYMBOLS if s[0] not in ("rpt_temporal_motion_record", "rpt_temporal_set_motion", "rpt_temporal_set_motion_device")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from rpt_amd import Camera, DeviceBuffer, Renderer, TemporalAccumulator, TemporalParams, scenes  # noqa: E402

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


def right_of(cam):
    right = np.cross(cam.direction, cam.up)
    return right / np.linalg.norm(right)


def stepped(cam):
    """The camera a small step to its right: 0.2 % of the eye's distance from the origin."""
    return Camera(cam.eye + 0.002 * max(float(np.linalg.norm(cam.eye)), 1.0) * right_of(cam), cam.direction, cam.up, cam.fov, cam.aperture,
                  cam.focal_distance)


floor_ms = n * FLOOR_BYTES / (HBM_PEAK_GBS * 1e6)
scene, cam, cfg = scenes.CONFIGS["C3"]()
cams = [cam, stepped(cam)]
r = Renderer(scene, cam).width(args.size).height(args.size).max_bounces(cfg["max_bounces"]).seed(1)
planes = [[zeros(3 * n) for _ in range(3)] for _ in cams]
rgb, var = zeros(3 * n), zeros(n)
out, out_var, out_len = zeros(3 * n), zeros(n), zeros(n)
torch.cuda.synchronize()
for c, pl in zip(cams, planes):
    r.camera = c
    r.features_device(args.spp, *[p.data_ptr() for p in pl], sample_offset=0)
r.camera = cam
buf = DeviceBuffer(args.size, args.size)
r._sample_offset = 0
for _ in range(4):
    r.sample(args.spp // 4, buf)
torch.cuda.synchronize()
buf.mean_device(rgb.data_ptr(), var.data_ptr())
torch.cuda.synchronize()
p = TemporalParams()
m = len(scene.objects)
print(f"library {_lib.LIB_PATH}; C3 {args.size}x{args.size}x{args.spp}, {m} objects; floor {floor_ms:.4f} ms", flush=True)


def run(what, before):
    acc = TemporalAccumulator(args.size, args.size)

    def accumulate(k):
        pl = planes[k % 2]
        before(acc)
        acc.accumulate_device(cams[k % 2], rgb.data_ptr(), var.data_ptr(), pl[1].data_ptr(), pl[2].data_ptr(), out.data_ptr(), out_var.data_ptr(),
                              out_len.data_ptr(), params=p, stream_ptr=stream.cuda_stream)

    ms = timed(accumulate, calls=2 * (args.calls // 2))
    torch.cuda.synchronize()
    took = float((out_len > 1.0).double().mean())
    med = statistics.median(ms)
    print(f"  accumulate, {what}: {fmt(ms)} = {med / floor_ms:.2f} x the floor; {took * 100:.1f} % of the pixels took history, "
          f"mean len {float(out_len.mean()):.2f}", flush=True)
    acc.close()
    return med


base = run("no table", lambda acc: None)
if not args.no_table:
    identity = np.zeros((m, 24))
    identity[:, [0, 5, 10, 12, 16, 20]] = 1.0
    dist = max(float(np.linalg.norm(cam.eye)), 1.0)
    pixel = 2.0 * dist * math.tan(cam.fov / 2.0) / args.size
    moving = identity.copy()
    moving[:, [3, 7, 11]] = 0.3 * pixel * right_of(cam)
    d_identity, d_moving = torch.from_numpy(identity).cuda(), torch.from_numpy(moving).cuda()
    torch.cuda.synchronize()
    for what, before in (("identity table (device)", lambda acc: acc.set_motion_device(d_identity.data_ptr(), m)),
                         ("moving table (device)", lambda acc: acc.set_motion_device(d_moving.data_ptr(), m)),
                         ("moving table (host, uploaded per call)", lambda acc: acc.set_motion(moving))):
        med = run(what, before)
        print(f"    {med - base:+.4f} ms against no table ({(med / base - 1.0) * 100:+.1f} %)", flush=True)
buf.close()
