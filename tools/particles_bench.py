"""Measurements for the particle systems ("Particle systems"): per frame of rk4_integrate(state, 1/16, 1/10000)
at n = 25, 100 and 256 the device time (events around the chained launches, after a warm-up) next to rpt_particles_integrate_host on
one thread of the same machine; the longest single launch (256 steps at n = 256); the block-size / lanes-per-particle sweep at
n = 25; the display-position pass alone; the simulation's share of a marbles frame.  With --batch the ensembles' rows instead
("Ensembles"): a frame at n = 25 for 1, 64, R/2, R, 2R and 4R systems next to that many single-handle frames;
the longest launch of a batch at n = 256 for R and 4R systems next to the single handle's; dynamic LDS sized to the batch against
padded to the single kernel's 54.6 KiB; the block-size / lanes sweep at R systems; one marbles_field frame of a 4 x 4 grid.
Needs a GPU: there is no fallback.

    python tools/particles_bench.py [--reps 5] [--out file.json] [--batch]
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

from rpt_amd import MarblesSystem, ParticleEnsemble, ParticleSimulator, ParticleState, Renderer, _lib, scenes  # noqa: E402
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


def batch_ms(n, n_systems, reps, time_=TIME, tune=None, warm=1, one_launch=False):
    """A batch of n_systems marble systems of n particles (states of their own): the device time of integrate(time_, STEP), or with
    one_launch of 256 / rounds steps: the launch the rule would issue if blocks that share a CU cost each other nothing."""
    if tune:
        os.environ["RPT_PARTICLES_TUNE"] = ",".join(str(x) for x in tune)
    else:
        os.environ.pop("RPT_PARTICLES_TUNE", None)
    states = [state(n, seed=1 + s) for s in range(n_systems)]
    sim = ParticleEnsemble([MarblesSystem(R)] * n_systems, states)
    info = sim.info()
    if one_launch:
        time_ = max(1, 256 // info["rounds"]) * STEP * (1.0 - 2.0 ** -30)
    st = torch.cuda.Stream()
    out = []
    try:
        for i in range(warm + reps):
            for s in range(n_systems):                     # the same work every time
                sim.set_state(s, states[s])
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(st)
            sim.integrate(time_, STEP, st.cuda_stream)
            b.record(st)
            b.synchronize()
            if i >= warm:
                out.append(a.elapsed_time(b))
    finally:
        sim.close()
        os.environ.pop("RPT_PARTICLES_TUNE", None)
    return {"n_systems": n_systems, "median_ms": statistics.median(out), "min_ms": min(out), "max_ms": max(out), **info}


def resident(n, tune=None):
    if tune:
        os.environ["RPT_PARTICLES_TUNE"] = ",".join(str(x) for x in tune)
    sim = ParticleEnsemble([MarblesSystem(R)], [state(n)])
    try:
        return sim.info()
    finally:
        sim.close()
        os.environ.pop("RPT_PARTICLES_TUNE", None)


def batch_rows(a):
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    res = {"compute_units": cus}
    single = device_ms(25, a.reps)["median_ms"]
    r25 = resident(25)["resident_blocks"]
    res["frame_n25"] = {"single_handle_ms": single, "resident_blocks": r25, "rows": []}
    for m in (1, 64, r25 // 2, r25, min(4096, 2 * r25), min(4096, 4 * r25)):
        row = batch_ms(25, m, a.reps)
        row["n_systems_x_single_ms"] = m * single
        res["frame_n25"]["rows"].append(row)
    # the longest launch: the single handle's 256 steps at n = 256 next to one launch of a batch at n = 256
    r256 = resident(256)["resident_blocks"]
    res["longest_launch_n256"] = {"single_handle_ms": device_ms(256, a.reps, time_=256 * STEP * (1.0 - 2.0 ** -30))["median_ms"], "resident_blocks": r256,
                                  "rows": [batch_ms(256, m, a.reps, one_launch=True) for m in (r256, min(4096, 4 * r256))]}
    # dynamic LDS sized to the batch against the single kernel's 54.6 KiB (RPT_PARTICLES_TUNE's third number pads it)
    pad = 54568 - resident(25)["lds_bytes"]
    padded = resident(25, (256, 8, pad))
    m = min(4096, 4 * r25)
    res["lds_n25"] = {"sized_to_batch": batch_ms(25, m, a.reps), "padded_to_54568": batch_ms(25, m, a.reps, tune=(256, 8, pad)),
                      "blocks_per_cu": {"sized_to_batch": r25 // cus, "padded_to_54568": padded["resident_blocks"] // cus}}
    res["sweep_n25_at_R"] = {}
    for block in (256, 512, 1024):
        for lanes in (8, 16, 32, 64):
            rr = resident(25, (block, lanes))["resident_blocks"]
            row = batch_ms(25, rr, a.reps, tune=(block, lanes))
            res["sweep_n25_at_R"]["%dx%d" % (block, lanes)] = {"resident_blocks": rr, "median_ms": row["median_ms"], "ms_per_system": row["median_ms"] / rr}
    # one marbles_field frame of a 4 x 4 grid: the simulation of its 16 glasses and the render
    offsets = scenes.marbles_field_offsets((4, 4), 3.0)
    sim_ms = batch_ms(25, 16, a.reps)["median_ms"]
    shown = [MarblesSystem(R).display_positions(state(25, seed=1 + g).pos) + np.array([ox, 0.0, oz]) for g, (ox, oz) in enumerate(offsets)]
    w, h, spp = (int(x) for x in a.render.split("x"))
    scene, cam, cfg = scenes.marbles_field(shown, offsets)
    r = Renderer(scene, cam).width(w).height(h).max_bounces(cfg["max_bounces"]).seed(1)
    r.sample_array(2)
    ts = []
    for _ in range(max(1, a.reps // 2)):
        t = time.perf_counter()
        r.sample_array(spp)
        ts.append((time.perf_counter() - t) * 1e3)
    render = statistics.median(ts)
    res["marbles_field_frame_4x4"] = {"render": a.render, "render_ms": render, "simulation_ms": sim_ms, "simulation_share": sim_ms / (sim_ms + render),
                                      "sixteen_single_handles_ms": 16 * single}
    return res


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
    ap.add_argument("--batch", action="store_true", help="the ensembles' rows instead of the single handle's")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("particles_bench: no GPU")
    if a.batch:
        line = json.dumps(batch_rows(a))
        print(line)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(line + "\n")
        return
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
