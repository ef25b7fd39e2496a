"""What moving a committed scene's spheres on the device costs, next to what the sequences did before: rebuild and recommit.

  python tools/scene_update_bench.py [--out FILE]

Four measurements ("Moving spheres"); warm-up, then the median of 5, the two paths alternated in one run:
  1. per frame of marbles (25 marbles) and of marbles_field at 2 x 2 and 4 x 4: host wall time from "the state is ready on the device"
     to "the render can be launched" -- the parent path (download of the display positions, the Python scene, the commit, the host
     motion records) and the update path (display_positions_device + move_spheres_device, waited for);
  2. the update kernels alone, between two events on the stream, with the scene tree's refit as one workgroup and as one launch per height;
  3. the refit's decay: the render of a marbles_field frame on the tree refitted 1, 30 and 180 times over a running simulation, against
     a fresh commit of the same positions;
  4. a 400 x 300 x 32 spp preview frame of the live sequence end to end, next to the generator path.
Needs a GPU; nothing here is a pass / fail threshold."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from rpt_amd import Renderer, scenes  # noqa: E402
from rpt_amd.api import TemporalAccumulator, TemporalParams, temporal_motion_record  # noqa: E402
from rpt_amd.ode import MarblesSystem, ParticleEnsemble, ParticleSimulator  # noqa: E402

REPEATS, WARMUP = 5, 2


def sync():
    import torch
    torch.cuda.synchronize()


def settled(n_sys, seed=0):
    """States a little above the glass: marbles that move from frame to frame."""
    out = []
    for g in range(n_sys):
        s = scenes.marbles_initial(seed=123 + seed + g)
        s.pos[:, 1] = 0.3 + 0.05 * (np.arange(len(s)) % 5)
        out.append(s)
    return out


class Case:
    """One sequence: a simulation, the offsets of its glasses, and the builders of both paths."""

    def __init__(self, grid):
        self.grid = grid
        self.offsets = scenes.marbles_field_offsets(grid) if grid else None
        states = settled(len(self.offsets) if grid else 1)
        if grid:
            self.sim = ParticleEnsemble([MarblesSystem(scenes.MARBLES_RADIUS)] * len(states), states, device=0)
        else:
            self.sim = ParticleSimulator(MarblesSystem(scenes.MARBLES_RADIUS), states[0], device=0)
        self.name = f"marbles_field {grid[0]} x {grid[1]}" if grid else "marbles"

    def shown(self):
        if not self.grid:
            return self.sim.display_positions()
        return [p + np.array([ox, 0.0, oz]) for p, (ox, oz) in zip(self.sim.display_positions(), self.offsets)]

    def scene(self, shown):
        return scenes.marbles_field(shown, self.offsets)[:2] if self.grid else scenes.marbles(shown)[:2]

    def live(self):
        """(scene, camera, objects, device offsets or None, motion table) of the update path, committed at the current state."""
        from rpt_amd.api import _device_copy
        scene, camera = self.scene(self.shown())
        if self.grid:
            objects, shifts, at = [], [], 0
            for size, (ox, oz) in zip(self.sim.sizes, self.offsets):
                objects += list(range(at + 1, at + 1 + size))
                shifts += [[ox, 0.0, oz]] * size
                at += 1 + size
            offsets = _device_copy(np.array(shifts), 0)
        else:
            objects, offsets = list(range(1, 1 + self.sim.n)), None
        scene.set_movable_spheres(objects)
        identity = np.zeros(24)
        identity[[0, 5, 10, 12, 16, 20]] = 1.0
        table = _device_copy(np.tile(identity, (len(scene.objects), 1)), 0)
        sync()
        return scene, camera, objects, offsets, table

    def advance(self, time_=1.0 / 16.0):
        self.sim.integrate(time_, 1.0 / 10000.0)


def frame_preparation(case):
    """Measurement 1: both paths from a ready state to a launchable render, alternated."""
    acc = TemporalAccumulator(64, 48, 0)
    scene, camera, objects, offsets, table = case.live()
    prev, _ = case.scene(case.shown())
    parent, update = [], []
    for k in range(WARMUP + REPEATS):
        case.advance(1.0 / 64.0)
        sync()
        t0 = time.perf_counter()
        cur, _ = case.scene(case.shown())
        cur._commit(0)
        acc.set_motion(np.stack([temporal_motion_record(c.shape.matrix(), p.shape.matrix()) for c, p in zip(cur.objects, prev.objects)]))
        t1 = time.perf_counter()
        scene.move_spheres_device(case.sim.display_positions_device(), offsets.data_ptr() if offsets is not None else 0, table.data_ptr())
        acc.set_motion_device(table.data_ptr(), len(scene.objects))
        t2 = time.perf_counter()   # enqueued: the render could be launched behind it now
        sync()
        t3 = time.perf_counter()
        prev.close()
        prev = cur
        if k >= WARMUP:
            parent.append(1e3 * (t1 - t0))
            update.append((1e3 * (t2 - t1), 1e3 * (t3 - t1)))
    prev.close()
    info = scene.movable_info()
    scene.close()
    acc.close()
    return {"case": case.name, "spheres": len(objects), "tree_nodes": info["tree_nodes"], "tree_heights": info["tree_heights"],
            "parent_ms": statistics.median(parent), "update_enqueue_ms": statistics.median(u[0] for u in update),
            "update_waited_ms": statistics.median(u[1] for u in update)}


def kernels_alone(case):
    """Measurement 2: the update's kernels between two events, one workgroup and one launch per height."""
    import torch
    out = {"case": case.name}
    for per_height in (0, 1):
        scene, camera, objects, offsets, table = case.live()
        scene.set_option("refit_per_height", per_height)
        d = case.sim.display_positions_device()
        sync()
        ms = []
        for k in range(WARMUP + 4 * REPEATS):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            scene.move_spheres_device(d, offsets.data_ptr() if offsets is not None else 0, table.data_ptr())
            b.record()
            sync()
            if k >= WARMUP:
                ms.append(a.elapsed_time(b))
        out["per_height_ms" if per_height else "one_workgroup_ms"] = statistics.median(ms)
        scene.close()
    return out


def render_ms(scene, camera, w=400, h=300, spp=32):
    import torch
    r = Renderer(scene, camera).width(w).height(h).max_bounces(9).seed(1)
    frame = torch.zeros(w * h * 3, dtype=torch.float64, device="cuda")
    ms = []
    for k in range(WARMUP + REPEATS):
        sync()
        t0 = time.perf_counter()
        r.sample_device(spp, frame.data_ptr())
        sync()
        if k >= WARMUP:
            ms.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(ms)


def refit_decay(grid):
    """Measurement 3: the refitted tree's render time against a fresh commit's, after 1, 30 and 180 updates."""
    case = Case(grid)
    scene, camera, objects, offsets, table = case.live()
    rows, done = [], 0
    for target in (1, 30, 180):
        while done < target:
            case.advance()
            scene.move_spheres_device(case.sim.display_positions_device(), offsets.data_ptr(), 0)
            done += 1
        sync()
        fresh, _ = case.scene(case.shown())
        a, b = render_ms(scene, camera), render_ms(fresh, camera)
        a2, b2 = render_ms(scene, camera), render_ms(fresh, camera)
        fresh.close()
        rows.append({"updates": target, "refitted_ms": min(a, a2), "fresh_ms": min(b, b2), "ratio": min(a, a2) / min(b, b2)})
    scene.close()
    case.sim.close()
    return {"case": case.name, "decay": rows}


def preview_frames(frames=6):
    """Measurement 4: wall time per 400 x 300 x 32 spp frame of the sequence, the live path and the generator path: a warm-up pass
    of each, then five timed passes of `frames` frames, the two paths in turn; the median pass of each."""
    def one(name):
        state = settled(1)[0]
        sync()
        t0 = time.perf_counter()
        if name == "live":
            scene, camera, mover = scenes.marbles_live(frames, state=state)
            r = Renderer(scene, camera).width(400).height(300).max_bounces(9).seed(3).num_samples(32)
            n = sum(1 for _ in r.render_sequence([camera] * frames, batches=2, temporal=TemporalParams(), live=mover))
            mover.close()
            scene.close()
        else:
            pairs = list(scenes.marbles_sequence(frames, state=state))
            r = Renderer(pairs[0][0], pairs[0][1]).width(400).height(300).max_bounces(9).seed(3).num_samples(32)
            n = sum(1 for _ in r.render_sequence([pairs[0][1]] * frames, batches=2, temporal=TemporalParams(), scenes=[p[0] for p in pairs]))
            for p in pairs:
                p[0].close()
        sync()
        return 1e3 * (time.perf_counter() - t0) / n
    ms = {"generator": [], "live": []}
    for k in range(1 + REPEATS):
        for name in ("generator", "live"):
            t = one(name)
            if k >= 1:
                ms[name].append(t)
    return {"generator_ms_per_frame": statistics.median(ms["generator"]), "live_ms_per_frame": statistics.median(ms["live"]),
            "generator_passes": ms["generator"], "live_passes": ms["live"], "frames_per_pass": frames}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    results = {"frame_preparation": [], "kernels": []}
    for grid in (None, (2, 2), (4, 4)):
        case = Case(grid)
        results["frame_preparation"].append(frame_preparation(case))
        results["kernels"].append(kernels_alone(case))
        case.sim.close()
        print(json.dumps({k: v[-1] for k, v in results.items()}), flush=True)
    results["refit_decay"] = [refit_decay((2, 2)), refit_decay((4, 4))]
    print(json.dumps(results["refit_decay"]), flush=True)
    results["preview"] = preview_frames()
    print(json.dumps(results["preview"]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
