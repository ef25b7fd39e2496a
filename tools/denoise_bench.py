"""Time of the a-trous denoiser (Denoiser.denoise_device) on C3's and C5's frames at 1024 x 1024, default parameters, next to the
render of the same 16 spp: 4 batches x 4 spp into a DeviceBuffer, the feature planes of the 16 samples, the per-pixel mean and the
variance of the mean, then the filter with 1 .. P passes for each "denoise_stage" setting -- 0: every pass gathers its taps from
global memory (form a), 1 / 2: the passes of step <= 1 / <= 2 stage their tile and halo in LDS (form b).  HIP events around the
stream, median of the rounds after a warm-up, min-max in brackets.  A call of P passes is prepare + P passes, the last of which
writes the frame (32 B per pixel) in place of records (64 B): the time of the pass of step 2^(P-1) is the call of P passes minus the
call of P - 1 passes, up to that difference.  Floor of a pass: one record read and one written per pixel (128 B) over the HBM peak
bench.py's roofline uses (8 TB/s), next to a device-to-device copy of one record array measured here.
Usage: python tools/denoise_bench.py [--size 1024] [--spp 16] [--rounds 5] [--passes 4]"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from rpt_amd import DenoiseParams, Denoiser, DeviceBuffer, Renderer, _lib, scenes  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, default=1024)
ap.add_argument("--spp", type=int, default=16)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--passes", type=int, default=4)
args = ap.parse_args()
HBM_PEAK_GBS = 8000.0

n = args.size * args.size
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


def fmt(ms):
    return f"{statistics.median(ms):.3f} ms [{min(ms):.3f}-{max(ms):.3f}]"


denoisers = {}
for stage in (0, 1, 2):
    _lib.check(_lib.load().rpt_set_option(b"denoise_stage", stage))
    denoisers[stage] = Denoiser(args.size, args.size)
_lib.check(_lib.load().rpt_set_option(b"denoise_stage", -1))

rec_a, rec_b = torch.zeros(8 * n, dtype=torch.float64, device="cuda"), torch.zeros(8 * n, dtype=torch.float64, device="cuda")
copy_ms = timed(lambda: rec_b.copy_(rec_a))
print(f"floor of a pass at {args.size}x{args.size}: 128 B per pixel / {HBM_PEAK_GBS / 1000:.0f} TB/s = {n * 128 / (HBM_PEAK_GBS * 1e6):.4f} ms; "
      f"device-to-device copy of one record array (64 B read + 64 B written per pixel): {fmt(copy_ms)}", flush=True)

for name in ("C3", "C5"):
    scene, cam, cfg = scenes.CONFIGS[name]()
    r = Renderer(scene, cam).width(args.size).height(args.size).max_bounces(cfg["max_bounces"]).seed(1)
    planes = [torch.zeros(3 * n, dtype=torch.float64, device="cuda") for _ in range(3)]
    frame = torch.zeros(3 * n, dtype=torch.float64, device="cuda")
    rgb, var = torch.zeros(3 * n, dtype=torch.float64, device="cuda"), torch.zeros(n, dtype=torch.float64, device="cuda")
    outs = {s: torch.zeros(3 * n, dtype=torch.float64, device="cuda") for s in denoisers}
    out_var = torch.zeros(n, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()

    def render():
        r._sample_offset = 0
        r.sample_device(args.spp, frame.data_ptr(), stream.cuda_stream)

    render_ms = timed(render)
    feature_ms = timed(lambda: r.features_device(args.spp, *[p.data_ptr() for p in planes], stream_ptr=stream.cuda_stream, sample_offset=0))
    buf = DeviceBuffer(args.size, args.size)
    r._sample_offset = 0
    for _ in range(4):
        r.sample(args.spp // 4, buf)
    torch.cuda.synchronize()
    mean_ms = timed(lambda: buf.mean_device(rgb.data_ptr(), var.data_ptr(), stream.cuda_stream))
    print(f"{name} {args.size}x{args.size}x{args.spp}: render {fmt(render_ms)}; feature planes {fmt(feature_ms)}; mean + variance {fmt(mean_ms)}", flush=True)
    for passes in range(1, args.passes + 1):
        p = DenoiseParams(passes=passes)
        line = []
        for stage, d in denoisers.items():
            ms = timed(lambda: d.denoise_device(rgb.data_ptr(), var.data_ptr(), *[q.data_ptr() for q in planes], outs[stage].data_ptr(),
                                                out_var.data_ptr(), params=p, stream_ptr=stream.cuda_stream))
            line.append(f"denoise_stage {stage}: {fmt(ms)}")
        print(f"  {name} prepare + {passes} pass{'es' if passes > 1 else ''} (steps 1..{1 << (passes - 1)}): " + "; ".join(line), flush=True)
    torch.cuda.synchronize()
    same = all(torch.equal(outs[0], outs[s]) for s in denoisers)
    print(f"  {name} the {args.passes}-pass frames of the three settings are the same bits: {same}; filtered mean {float(outs[0].mean()):.6f}, "
          f"input mean {float(rgb.mean()):.6f}", flush=True)
