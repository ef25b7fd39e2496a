"""examples/monomial_glass.rs (scenes.monomial_glass) timed in both render modes: at the example's size (800 x 600, 100 spp,
max_bounces(1)) and at 1024 x 1024 x 256.  Prints one line per (mode, size): the best of three device-side renders (HIP events),
Msamples/s, the mean pixel value.

    python tools/monomial_bench.py              # timings
    python tools/monomial_bench.py --rocprof    # the same under rocprofv3 --kernel-trace --stats (a child process; CSVs in
                                                # rocprof_monomial/, the per-kernel totals printed at the end)
"""
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = [(800, 600, 100), (1024, 1024, 256)]


def run():
    import torch
    from rpt_amd import Renderer, scenes, set_option
    set_option("timing", 1)
    for eps in (0, 1):
        for w, h, spp in SIZES:
            scene, cam, cfg = scenes.monomial_glass()
            scene.set_option("epsilon_policy", eps)
            r = Renderer(scene, cam).width(w).height(h).max_bounces(cfg["max_bounces"]).seed(1)
            frame = torch.zeros(w * h * 3, dtype=torch.float64, device="cuda")
            ms = []
            for _ in range(4):
                r._sample_offset = 0
                torch.cuda.synchronize()
                r.sample_device(spp, frame.data_ptr(), 0)
                torch.cuda.synchronize()
                ms.append(r.timing()[0])
            best = min(ms[1:])
            mean = float(frame.mean())
            print(f"{'fp64 reference-epsilon' if eps else 'fp32 robust':24s} {w}x{h}x{spp}: {best:9.2f} ms  "
                  f"{w * h * spp / best / 1e3:8.1f} Msamples/s  mean {mean:.6f}", flush=True)


def main():
    if "--rocprof" in sys.argv:
        out = os.path.join(ROOT, "rocprof_monomial")
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", out, "-o", "monomial", "--output-format", "csv", "--",
               sys.executable, os.path.abspath(__file__)]
        subprocess.run(cmd, check=True)
        for dirpath, _, files in os.walk(out):
            for f in files:
                if f.endswith("kernel_stats.csv"):
                    print(open(os.path.join(dirpath, f)).read())
        return
    t0 = time.perf_counter()
    run()
    print(f"(wall {time.perf_counter() - t0:.1f} s)")


if __name__ == "__main__":
    main()
