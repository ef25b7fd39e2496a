"""Reference-epsilon mode: where a mesh's candidate tree (scene option "f64_mesh_tree_min") starts to pay.

Renders scenes.mesh_in_fog(nu, nv) -- one mesh of 2 nu nv triangles, a plane, an emissive quad, fog -- in the mode at SIZE x SIZE x SPP for
a ladder of mesh sizes, once with a tree over the mesh ("f64_mesh_tree_min" = 1) and once with the scan of all its triangles (= 0), checks
that the two frames are the same bits and prints the kernel times (HIP events, best of three) of both.  The crossover is the default of
the option.  `--c5` adds the full C5 mesh (224 x 224: 100,352 triangles) at 64 x 64 x 4, scan included (one run of it).

    python tools/f64_mesh_tree.py [--size 256] [--spp 16] [--c5]"""
import argparse
import sys

import numpy as np

sys.path.insert(0, ".")
from rpt_amd import Renderer, scenes  # noqa: E402

LADDER = [(2, 2), (3, 2), (4, 2), (4, 3), (4, 4), (6, 4), (8, 4), (8, 6), (8, 8), (12, 8), (16, 8), (24, 12), (48, 24)]


def run(nu, nv, size, spp, tree_min, repeats):
    scene, cam, cfg = scenes.mesh_in_fog(nu, nv)
    scene.set_option("epsilon_policy", 1)
    scene.set_option("timing", 1)
    scene.set_option("f64_mesh_tree_min", tree_min)
    r = Renderer(scene, cam).width(size).height(size).max_bounces(cfg["max_bounces"]).seed(1)
    ms, frame = [], None
    for _ in range(repeats):
        r._sample_offset = 0
        frame = r.sample_array(spp)
        ms.append(r.timing()[0])
    return min(ms), frame, r.f64_mesh_tree_info()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--c5", action="store_true")
    a = ap.parse_args()
    print(f"mesh_in_fog(nu, nv), reference-epsilon mode, {a.size} x {a.size} x {a.spp}, kernel ms (best of 3): tree | scan | scan / tree", flush=True)
    for nu, nv in LADDER:
        t_ms, t_frame, info = run(nu, nv, a.size, a.spp, 1, 3)
        s_ms, s_frame, _ = run(nu, nv, a.size, a.spp, 0, 3)
        same = np.array_equal(t_frame.view(np.uint64), s_frame.view(np.uint64))
        print(f"{2 * nu * nv:7d} triangles ({nu} x {nv}): {t_ms:9.3f} | {s_ms:9.3f} | {s_ms / t_ms:6.2f}   nodes {info['nodes']}, depth {info['depth']}, "
              f"frames {'equal' if same else 'DIFFER'}", flush=True)
    if a.c5:
        t_ms, t_frame, info = run(224, 224, 64, 4, 64, 3)
        s_ms, s_frame, _ = run(224, 224, 64, 4, 0, 1)
        same = np.array_equal(t_frame.view(np.uint64), s_frame.view(np.uint64))
        print(f"C5's mesh, {info['triangles']} triangles, 64 x 64 x 4: tree {t_ms:.3f} ms | scan {s_ms:.3f} ms | {s_ms / t_ms:.1f} x   nodes {info['nodes']}, "
              f"depth {info['depth']}, {info['bytes']} bytes, frames {'equal' if same else 'DIFFER'}", flush=True)


if __name__ == "__main__":
    main()
