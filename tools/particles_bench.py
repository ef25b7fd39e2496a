"""Measurements for the particle systems ("Particle systems"): per frame of rk4_integrate(state, 1/16, 1/10000)
at n = 25, 100 and 256 the device time (events around the chained launches, after a warm-up) next to rpt_particles_integrate_host on
one thread of the same machine; the longest single launch (256 steps at n = 256); the block-size / lanes-per-particle sweep at
n = 25; the display-position pass alone; the simulation's share of a marbles frame.  Needs a GPU: there is no fallback.

    python tools/particles_bench.py [--reps 5] [--out file.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from rpt_amd import MarblesSystem, ParticleSimulator, ParticleState, Renderer, _lib, scenes  # noqa: E402
from rpt_amd._lib import ParticlesParams, vp  # noqa: E402

R, TIME, STEP = 0.15, 1.0 / 16.0, 1.0 / 10000.0


def state(n, seed=1):
    """Marbles at rest in and around the glass, close enough that many touch: the load of a frame late in the sequence."""
    rng = np.random.default_rng(seed)
    side = max(0.4, 0.22 * n ** (1.0 / 3.0))
    return ParticleState(rng.uniform([-side, 0.1, -side], [side, 0.1 + 2.0 * side, side], (n, 3)))


def device_ms(n, reps, time_=TIME, tune=None, warm=1):
    if tune:
        os.environ["RPT_PARTICLES_TUNE"] = "%d,%d" % tune
    else:
        os.environ.pop("RPT_PARTICLES_TUNE", None)
    sim = ParticleSimulator(MarblesSystem(R), state(n))
    st = torch.cuda.Stream()
    out = []
    try:
        for i in range(warm + reps):
            sim.set_state(state(n))                        # the same work every time
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(st)
            sim.integrate(time_, STEP, st.cuda_stream)
            b.record(st)
            b.synchronize()
            if i >= warm:
                out.append(a.elapsed_time(b))
        counters = sim.counters()
    finally:
        sim.close()
        os.environ.pop("RPT_PARTICLES_TUNE", None)
    return {"median_ms": statistics.median(out), "min_ms": min(out), "max_ms": max(out), "contacts_per_eval": counters[1] / max(1, counters[0])}


def host_ms(n, reps):
    lib = _lib.load()
    out = []
    for _ in range(reps):
        s = state(n)
        prm, cnt = ParticlesParams(2, n, R, 2.0), (C.c_uint64 * 8)()
        t = time.perf_counter()
        _lib.check(lib.rpt_particles_integrate_host(C.byref(prm), vp(s.pos), vp(s.vel), TIME, STEP, cnt))
        out.append((time.perf_counter() - t) * 1e3)
    return {"median_ms": statistics.median(out), "min_ms": min(out), "max_ms": max(out)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--render", default="400x300x32")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("particles_bench: no GPU")
    res = {"frame": {}, "sweep_n25": {}}
    for n in (25, 100, 256):
        res["frame"][n] = {"device": device_ms(n, a.reps), "host_one_thread": host_ms(n, max(1, a.reps // 2))}
    # the longest launch the library issues: 256 steps at n = 256 (a time just short of 256 steps: one launch)
    res["longest_launch_n256_256_steps"] = device_ms(256, a.reps, time_=256 * STEP * (1.0 - 2.0 ** -30))
    for block in (256, 512, 1024):
        for lanes in (8, 16, 32, 64):
            res["sweep_n25"]["%dx%d" % (block, lanes)] = device_ms(25, a.reps, tune=(block, lanes))["median_ms"]
    sim = ParticleSimulator(MarblesSystem(R), state(25))
    try:
        sim.display_positions()
        ts = []
        for _ in range(a.reps):
            t = time.perf_counter()
            shown = sim.display_positions()
            ts.append((time.perf_counter() - t) * 1e3)
        res["display_positions_n25_ms_wall"] = statistics.median(ts)      # launch + kernel + the copy back
    finally:
        sim.close()
    w, h, spp = (int(x) for x in a.render.split("x"))
    scene, cam, cfg = scenes.marbles(shown)
    r = Renderer(scene, cam).width(w).height(h).max_bounces(cfg["max_bounces"]).seed(1)
    r.sample_array(2)
    ts = []
    for _ in range(max(1, a.reps // 2)):
        t = time.perf_counter()
        r.sample_array(spp)
        ts.append((time.perf_counter() - t) * 1e3)
    render = statistics.median(ts)
    sim_ms = res["frame"][25]["device"]["median_ms"]
    res["marbles_frame"] = {"render": a.render, "render_ms": render, "simulation_ms": sim_ms, "simulation_share": sim_ms / (sim_ms + render)}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
