"""The candidate trees of the reference-epsilon mode's meshes (scene option "f64_mesh_tree_min"), on a CPU.

1. tests/host/mesh_tree_harness.cpp commits scenes through the real rpt_capi.cpp under AddressSanitizer + UBSan and checks every tree
   it finds in the arena: each triangle of the mesh in exactly one leaf; child boxes inside parent boxes; every fp64 vertex inside its
   leaf's fp32 box by the padding, no box with a zero extent; the depth within the limit.  Here: what each case must report.
2. A numpy restatement of the device's walk (kernels_f64.hip, mesh_tree_walk: cull32's slab test in fp32 on the padded boxes) over
   100,000 rays on the harness's torus, with the tree the commit built: every triangle that the fp64 test of the scan's loop can accept
   for a ray is among the triangles the walk reaches, and no node above it begins beyond the hit's time as the walk compares it.  That
   is what makes the walk's result the loop's: (smallest accepted time, smallest index among the triangles that reach it).

No GPU, no oracle."""
import os
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "mesh_tree_harness.cpp")
F32 = np.float32


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    if not os.path.exists("/opt/rocm/include/hip/hip_runtime_api.h"):
        pytest.skip("HIP headers not installed")
    d = tmp_path_factory.mktemp("mesh_tree")
    exe, dump = str(d / "harness"), str(d / "tree.bin")
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-std=c++17", "-w",
                           "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + os.path.join(ROOT, "include"), SRC, "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1")
    p = subprocess.run([exe, dump], capture_output=True, text=True, env=env, timeout=300)
    assert p.returncode == 0, p.stdout[-1000:] + p.stderr[-2000:]
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-2000:]
    lines = {}
    for l in p.stdout.splitlines():
        f = l.split()
        lines[f[0]] = {k: int(v) for k, v in (kv.split("=", 1) for kv in f[1:])}
    with open(dump, "rb") as f:
        raw = f.read()
    n_nodes, n_leaf, n_tris, root = struct.unpack_from("<4I", raw, 0)
    off = 16
    nodes = np.frombuffer(raw, dtype=np.dtype([("lo", "<f4", 3), ("first", "<u4"), ("hi", "<f4", 3), ("count", "<u4")]), count=n_nodes, offset=off)
    off += 32 * n_nodes
    leaf = np.frombuffer(raw, dtype="<u4", count=n_leaf, offset=off)
    off += 4 * n_leaf
    tris = np.frombuffer(raw, dtype="<f8", count=18 * n_tris, offset=off).reshape(n_tris, 6, 3)
    return lines, (nodes, leaf, tris, root)


BUILT = ("torus", "torus_xf", "one", "two", "grid", "far_grid", "shared", "default", "chain", "group_light")


@pytest.mark.parametrize("name", BUILT)
def test_every_tree_holds_its_mesh(harness, name):
    d = harness[0][name]
    assert d["rc"] == 0 and d["info_rc"] == 0 and d["meshes"] >= 1
    assert d["once"] == 1, "a triangle is in no leaf or in several"
    assert d["nested"] == 1, "a child's box reaches outside its parent's"
    assert d["padded"] == 1, "a vertex is not inside its leaf's box by the padding"
    assert d["thick"] == 1, "a box with a zero extent"
    assert d["trees"] == d["meshes"] and d["walked_triangles"] == d["triangles"]
    assert d["walked_depth"] == d["depth"] <= 20
    assert d["bytes"] >= 32 * d["nodes"] + 4 * d["triangles"]


def test_what_the_cases_report(harness):
    L = harness[0]
    assert L["torus"]["triangles"] == 576 and L["torus"]["render"] == 1 and L["torus"]["photon"] == 0 and L["torus"]["min"] == 1
    # a root that is a leaf
    assert (L["one"]["nodes"], L["one"]["depth"], L["one"]["triangles"]) == (1, 0, 1)
    assert (L["two"]["nodes"], L["two"]["depth"], L["two"]["triangles"]) == (1, 0, 2)
    # a mesh that shapes share is stored once and has one tree
    assert L["shared"]["meshes"] == 2 and L["shared"]["triangles"] == 576 + 12
    # the default threshold leaves a 12-triangle mesh (the walls and boxes of C2 - C4) on the scan; 0 and f64_cull = 0: no tree
    assert L["default"]["meshes"] == 1 and L["default"]["triangles"] == 576 and L["default"]["min"] > 12
    for name in ("never", "full_scan", "needle"):
        assert L[name]["rc"] == 0 and (L[name]["meshes"], L[name]["nodes"], L[name]["bytes"], L[name]["render"]) == (0, 0, 0, 0), name
    # depth: rebuilt within the limit, refused (RPT_ERR_UNSUPPORTED) only when a balanced tree does not fit either
    assert L["chain"]["depth"] <= 5
    assert L["too_deep"]["rc"] == -4
    # a flavour without the walk builds the trees and reports that it scans
    assert L["group_light"]["meshes"] == 1 and L["group_light"]["render"] == 0
    # RPT_ERR_STATE before the commit and for an fp32 scene, RPT_ERR_INVALID for a null pointer
    assert (L["fp32"]["rc"], L["fp32"]["before_commit"], L["fp32"]["info_rc"], L["fp32"]["null"]) == (0, -2, -2, -1)


# ------------------------------------------------------------------ the walk, restated
def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _rays(nodes, tris, rng):
    """100,000 rays in the mesh's own space: random; aimed at vertices and edges; starting on the surface; parallel to an axis with
    exact zero components, starting in face planes of the tree's own padded boxes (as fp32 holds them) and of the unpadded ones;
    lying in the faces of the root's box."""
    v = tris[:, :3, :]
    lo, hi = v.reshape(-1, 3).min(axis=0), v.reshape(-1, 3).max(axis=0)
    c, ext = 0.5 * (lo + hi), float(np.max(hi - lo))
    n = 20000
    O, D = [], []
    o = c + _unit(rng.standard_normal((n, 3))) * ext * rng.uniform(0.6, 3.0, (n, 1))
    O.append(o)
    D.append(_unit(lo + rng.uniform(-0.1, 1.1, (n, 3)) * (hi - lo) - o))
    k = rng.integers(0, len(v), n)
    a, b = v[k, rng.integers(0, 3, n)], v[k, rng.integers(0, 3, n)]
    tgt = a + np.where(rng.uniform(size=(n, 1)) < 0.5, 0.0, rng.uniform(size=(n, 1))) * (b - a)
    o = c + _unit(rng.standard_normal((n, 3))) * ext * 2.0
    O.append(o)
    D.append(_unit(tgt - o))
    k = rng.integers(0, len(v), n)
    w = rng.dirichlet((1.0, 1.0, 1.0), n)
    O.append(w[:, :1] * v[k, 0] + w[:, 1:2] * v[k, 1] + w[:, 2:] * v[k, 2])
    D.append(_unit(rng.standard_normal((n, 3))))
    ax = rng.integers(0, 3, n)
    d = np.zeros((n, 3))
    d[np.arange(n), ax] = rng.choice([-1.0, 1.0], n)
    o = v[rng.integers(0, len(v), n), rng.integers(0, 3, n)].copy()
    other = (ax + rng.integers(1, 3, n)) % 3
    node = rng.integers(0, len(nodes), n)
    plane = np.where(rng.uniform(size=n) < 0.5, nodes["lo"][node, other], nodes["hi"][node, other]).astype(np.float64)
    o[np.arange(n), other] = np.where(rng.uniform(size=n) < 0.6, plane, o[np.arange(n), other])
    o[np.arange(n), ax] = np.where(rng.uniform(size=n) < 0.5, o[np.arange(n), ax], (lo - ext)[ax])
    O.append(o)
    D.append(d)
    face = rng.integers(0, 3, n)
    o = c + _unit(rng.standard_normal((n, 3))) * ext * 1.5
    tgt = lo + rng.uniform(size=(n, 3)) * (hi - lo)
    side = np.where(rng.uniform(size=n) < 0.5, lo[face], hi[face])
    o[np.arange(n), face] = side
    tgt[np.arange(n), face] = side
    O.append(o)
    D.append(tgt - o)
    return np.concatenate(O), np.concatenate(D)


def _accepted(tris, o, d):
    """Triangle::intersect as the scan's loop runs it (eval_pair), without the comparison against the hit at hand: (rays, triangles)
    booleans and times.  Same operations in the same order, fp64, nothing fused."""
    v1, v2, v3 = tris[:, 0], tris[:, 1], tris[:, 2]
    d0, d1 = v2 - v1, v3 - v1
    cr = np.stack([d0[:, 1] * d1[:, 2] - d0[:, 2] * d1[:, 1], d0[:, 2] * d1[:, 0] - d0[:, 0] * d1[:, 2], d0[:, 0] * d1[:, 1] - d0[:, 1] * d1[:, 0]], axis=1)
    pn = cr / np.sqrt(cr[:, 0] * cr[:, 0] + cr[:, 1] * cr[:, 1] + cr[:, 2] * cr[:, 2])[:, None]

    def dot(a, b):
        return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]
    d00, d01, d11 = dot(d0, d0), dot(d0, d1), dot(d1, d1)
    den = d00 * d11 - d01 * d01
    with np.errstate(all="ignore"):
        cosine = dot(pn[None], d[:, None])
        time = dot(pn[None], v1[None] - o[:, None]) / cosine
        d2 = (o[:, None] + time[..., None] * d[:, None]) - v1[None]
        d20, d21 = dot(d2, d0[None]), dot(d2, d1[None])
        vv, ww = (d11 * d20 - d01 * d21) / den, (d00 * d21 - d01 * d20) / den
        uu = 1.0 - vv - ww
        ok = ~(np.abs(cosine) < 1e-8) & (time >= 1e-12) & (time < np.inf) & (uu >= 0.0) & (vv >= 0.0) & (ww >= 0.0)
    return ok, time


def _entry_times(nodes, o, d):
    """mesh_tree_walk's test of every node for every ray, in fp32 as the device forms it (its reciprocal is within an ulp of this
    one: the 4e-6 widening is thirty times that): -> (rays, nodes) `out` without the limit comparison, and the widened entry time."""
    with np.errstate(all="ignore"):
        of, df = o.astype(F32), d.astype(F32)
        eo = F32(1e-6) * np.abs(of).max(axis=1)
        lost = ((d != 0.0) & (np.abs(df) < F32(1.17549435e-38))) | np.isinf(df) | ~(eo < F32(np.inf))[:, None]
        inv = np.where(lost, F32(np.nan), F32(1.0) / df)
        ol, oh = of + eo[:, None], of - eo[:, None]
        lo, hi = nodes["lo"][None], nodes["hi"][None]
        a = (lo - ol[:, None]) * inv[:, None]
        b = (hi - oh[:, None]) * inv[:, None]
        tn = np.fmax(np.fmax(np.fmin(a[..., 0], b[..., 0]), np.fmin(a[..., 1], b[..., 1])), np.fmin(a[..., 2], b[..., 2]))
        tf = np.fmin(np.fmin(np.fmax(a[..., 0], b[..., 0]), np.fmax(a[..., 1], b[..., 1])), np.fmax(a[..., 2], b[..., 2]))
        less, more = F32(1.0) - F32(4e-6), F32(1.0) + F32(4e-6)
        tn_lo = np.fmin(tn * less, tn * more)
        tf_hi = np.fmax(tf * less, tf * more)
        out = (tn_lo > tf_hi) | (tf_hi < F32(0.0))
    assert tn_lo.dtype == F32
    return out, tn_lo


def test_the_padded_fp32_walk_reaches_every_triangle_the_fp64_loop_accepts(harness):
    nodes, leaf, tris, root = harness[1]
    assert len(tris) == 576 and root == 0
    # the path from the root to every triangle's leaf
    parent = np.full(len(nodes), -1)
    for k in np.flatnonzero(nodes["count"] == 0):
        parent[nodes["first"][k]] = parent[nodes["first"][k] + 1] = k
    order = range(len(nodes))                            # (children have larger indices than their parents: top-down)
    assert all(parent[k] < k for k in range(len(nodes)))
    leaf_of = np.full(len(tris), -1)
    for k in np.flatnonzero(nodes["count"] != 0):
        leaf_of[leaf[nodes["first"][k]:nodes["first"][k] + nodes["count"][k]]] = k
    assert (leaf_of >= 0).all()
    o, d = _rays(nodes, tris, np.random.default_rng(41))
    assert len(o) == 100000
    n_acc = n_zero = 0
    for s in range(0, len(o), 10000):
        oo, dd = o[s:s + 10000], d[s:s + 10000]
        ok, time = _accepted(tris, oo, dd)
        out, tn_lo = _entry_times(nodes, oo, dd)
        # a node is reached iff no node on its path is out; it may be left out later only if it begins beyond the limit, and the limit is
        # never below fp32(time) * 1.00001 of a triangle the loop accepts (min over the accepted hits so far, the search limit aside)
        reached = ~out
        late = np.zeros_like(out)
        with np.errstate(all="ignore"):
            lim = time.astype(F32) * F32(1.00001)       # (rays, triangles)
        worst = tn_lo.copy()                             # the largest widened entry time on the path (NaN: never compared true)
        for k in order:
            if parent[k] >= 0:
                reached[:, k] &= reached[:, parent[k]]
                worst[:, k] = np.fmax(worst[:, k], worst[:, parent[k]])
        cand = reached[:, leaf_of]                       # (rays, triangles)
        with np.errstate(invalid="ignore"):
            late = worst[:, leaf_of] > lim
        missed = ok & ~cand
        assert not missed.any(), ("the walk never reaches an accepted triangle", np.argwhere(missed)[:5], s)
        assert not (ok & late).any(), ("a node above an accepted triangle begins beyond its time", np.argwhere(ok & late)[:5], s)
        n_acc += int(ok.sum())
        n_zero += int((ok.any(axis=1) & (dd == 0.0).any(axis=1)).sum())
        # the test means something: the walk leaves most triangles out, for every kind of ray (axis-parallel ones included)
        assert cand.mean() < 0.1, (s, cand.mean())
    assert n_acc > 60000 and n_zero > 2000
