"""The candidate trees of the reference-epsilon mode's meshes (scene option "f64_mesh_tree_min"; kernels_f64.hip, mesh_tree_walk).

A tree chooses which triangles of a mesh a ray is tested against; the test itself is the scan's, in fp64, and a visited triangle
replaces the hit iff its time is smaller, or equal with a smaller index.  So everything here is an on / off comparison, bit for bit
(float64 bit patterns, NaNs included): "f64_mesh_tree_min" = 1 (every mesh has a tree) against 0 (every triangle of a mesh is tested,
in given order: the kernels of before).  The bounds against the literal oracle are those the suite already asserts for this mode:
test_gpu_monomial.py's for single hits, test_small_renders_follow_the_literal_oracle's for a frame."""
import json
import os

import numpy as np
import pytest

from rpt_amd import (Camera, KdTree, Light, Material, Medium, Mesh, Object, Renderer, RptError, Scene, monomial_surface, plane, scenes,
                     sphere, vec3)
from tests.util import rel_rms

pytestmark = pytest.mark.gpu

COUNTERS = ("rays", "hits", "self_hits", "shadow_tests", "shadow_pass", "shadow_near", "samples", "vertices")


def _oracle(scene):
    from oracle.pyoracle import OracleScene
    return OracleScene(scene)


def _eps_counters(r):
    from tests.test_gpu_epsilon import _eps_counters as f
    return f(r)


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _with_trees(make, tree_min, **options):
    """make() -> (scene, camera, ...); the scene in the mode with the given threshold."""
    out = make()
    out[0].set_option("epsilon_policy", 1)
    out[0].set_option("f64_mesh_tree_min", tree_min)
    for k, v in options.items():
        out[0].set_option(k, v)
    return out


# ------------------------------------------------------------------ rays
def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _to_world(m, p):
    return p if m is None else p @ m[:3, :3].T + m[:3, 3]


def _rays(tris, m, rng, n):
    """World-space rays at a mesh (tris: (k, 6, 3), local; m: its 4 x 4 matrix or None), n of each kind: random ones; aimed at shared
    vertices and at points of shared edges; starting on the surface (self-hits at t ~ 1e-12 are the mode's business); parallel to an axis
    of the mesh's own space with exact zero components, starting in the planes of the vertices' coordinates and of the bounds (the faces
    of the tree's boxes before the padding); lying in the faces of the bounds and through its corners (grazing)."""
    v = tris[:, :3, :]
    lo, hi = v.reshape(-1, 3).min(axis=0), v.reshape(-1, 3).max(axis=0)
    c, ext = 0.5 * (lo + hi), float(np.max(hi - lo)) + 1e-3
    o_l, d_l = [], []
    # random: origins in a shell around the mesh, aimed at points in its box
    o = c + _unit(rng.standard_normal((n, 3))) * ext * rng.uniform(0.8, 3.0, (n, 1))
    o_l.append(o)
    d_l.append(_unit(lo + rng.uniform(-0.1, 1.1, (n, 3)) * (hi - lo) - o))
    # aimed at vertices and at points of edges (the direction is rounded: some land on either side, some exactly on it)
    k = rng.integers(0, len(v), n)
    a, b = v[k, rng.integers(0, 3, n)], v[k, rng.integers(0, 3, n)]
    s = np.where(rng.uniform(size=(n, 1)) < 0.5, 0.0, rng.uniform(size=(n, 1)))
    tgt = a + s * (b - a)
    o = c + _unit(rng.standard_normal((n, 3))) * ext * 2.0
    o_l.append(o)
    d_l.append(_unit(tgt - o))
    # starting on the surface
    k = rng.integers(0, len(v), n)
    w = rng.dirichlet((1.0, 1.0, 1.0), n)
    o_l.append(w[:, :1] * v[k, 0] + w[:, 1:2] * v[k, 1] + w[:, 2:] * v[k, 2])
    d_l.append(_unit(rng.standard_normal((n, 3))))
    # axis-parallel, exact zeros, origins in coordinate planes of vertices / of the bounds
    ax = rng.integers(0, 3, n)
    d = np.zeros((n, 3))
    d[np.arange(n), ax] = rng.choice([-1.0, 1.0], n)
    o = v[rng.integers(0, len(v), n), rng.integers(0, 3, n)].copy()            # a vertex: all three coordinates lie in box planes
    other = (ax + rng.integers(1, 3, n)) % 3
    pick = rng.uniform(size=n)
    o[np.arange(n), other] = np.where(pick < 0.3, lo[other], np.where(pick < 0.6, hi[other], o[np.arange(n), other]))
    o[np.arange(n), ax] = np.where(rng.uniform(size=n) < 0.5, o[np.arange(n), ax], (lo - ext)[ax])   # on the surface, or from outside
    o_l.append(o)
    d_l.append(d)
    # grazing the bounds: in a face plane of the box, and through a corner
    face = rng.integers(0, 3, n)
    o = c + _unit(rng.standard_normal((n, 3))) * ext * 1.5
    tgt = lo + rng.uniform(size=(n, 3)) * (hi - lo)
    side = np.where(rng.uniform(size=n) < 0.5, lo[face], hi[face])
    o[np.arange(n), face] = side
    tgt[np.arange(n), face] = side
    corner = np.where(rng.uniform(size=(n, 3)) < 0.5, lo, hi)
    tgt = np.where(rng.uniform(size=(n, 1)) < 0.3, corner, tgt)
    o_l.append(o)
    d_l.append(tgt - o)                                                         # (not normalised: exact zeros stay exact)
    o, d = np.concatenate(o_l), np.concatenate(d_l)
    if m is None:
        return o, d
    return _to_world(m, o), d @ m[:3, :3].T


def _quad_grid(n):
    """n x n unit quads in the plane y = 0: every box of the tree has a zero extent before it is padded."""
    t = []
    up = np.array([0.0, 1.0, 0.0])
    for i in range(n):
        for j in range(n):
            a, b, c, d = (np.array(p, dtype=np.float64) for p in ((i, 0, j), (i + 1, 0, j), (i + 1, 0, j + 1), (i, 0, j + 1)))
            t += [[a, c, b, up, up, up], [a, d, c, up, up, up]]
    return np.array(t)


def _duplicates(rng):
    """Every triangle of a small torus twice, the copy with the normals negated, shuffled: of the two the lower index must win."""
    base = scenes.bumpy_torus(10, 8, major=0.5, minor=0.22, bump=0.1)
    copy = base.copy()
    copy[:, 3:, :] = -copy[:, 3:, :]
    both = np.concatenate([base, copy])
    perm = rng.permutation(len(both))
    where = np.empty(len(both), dtype=np.int64)
    where[perm] = np.arange(len(both))                   # where[k]: the index triangle k of `both` got
    g = len(base)
    sign = np.where(where[:g] < where[g:], 1.0, -1.0)    # per geometric triangle: the normals of its lower copy
    return base, both[perm], sign, np.abs(where[:g] - where[g:])


HIT_CASES = ["torus", "leaf roots", "grid", "duplicates"]


def _hit_scene(case):
    """-> (scene, [(tris, matrix)] to aim at, extra)"""
    rng = np.random.default_rng(17)
    sc = Scene()
    grey = Material.diffuse(vec3(0.7, 0.7, 0.7))
    extra = None
    if case == "torus":     # 576 triangles under a rotation and a non-uniform scale, and the same mesh as it is (one tree for both)
        tris = scenes.bumpy_torus(24, 12)
        mesh = Mesh(tris)
        xf = mesh.scale(vec3(3.4, 1.3, 2.1)).rotate_x(0.6).rotate_y(1.1).translate(vec3(5.0, 0.5, -1.0))
        sc.add(Object(xf).material(grey))
        sc.add(Object(mesh).material(grey))
        targets = [(tris, xf.matrix()), (tris, None)]
    elif case == "leaf roots":   # a 1-triangle and a 2-triangle mesh: the root is a leaf (and the records fit the kernels' LDS tables)
        one = np.array([[[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [0, 0, 1], [0, 0, 1]]], dtype=np.float64)
        two = np.array([[[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [0, 0, 1], [0, 0, 1]],
                        [[1, 0, 0], [1, 1, 0.5], [0, 1, 0], [0, 0, 1], [0, 0, 1], [0, 0, 1]]], dtype=np.float64)
        xf = Mesh(two).rotate_z(0.4).translate(vec3(3.0, 0.0, 0.0))
        sc.add(Object(Mesh(one)).material(grey))
        sc.add(Object(xf).material(grey))
        targets = [(one, None), (two, xf.matrix())]
    elif case == "grid":
        tris = _quad_grid(9)
        sc.add(Object(Mesh(tris)).material(grey))
        targets = [(tris, None)]
    else:
        base, tris, sign, apart = _duplicates(rng)
        assert np.median(apart) > 40                        # the copies are far apart in index
        sc.add(Object(Mesh(tris)).material(grey))
        targets = [(base, None)]
        extra = (base, sign)
    return sc, targets, extra


@pytest.fixture(scope="module")
def hit_rays():
    out = {}
    for case in HIT_CASES:
        _, targets, _ = _hit_scene(case)
        rng = np.random.default_rng(23)
        per = 2600 // len(targets)                          # 5 kinds x 2,600 rays x 4 cases: 52,000 rays
        parts = [_rays(t, m, rng, per) for t, m in targets]
        out[case] = (np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]))
    return out


# ------------------------------------------------------------------ 1. hits, tree = scan
@pytest.mark.parametrize("case", HIT_CASES)
def test_hits_with_trees_equal_the_scan_bit_for_bit(case, hit_rays):
    o, d = hit_rays[case]
    res = {}
    for tree_min in (1, 0):
        sc, _, extra = _hit_scene(case)
        sc.set_option("epsilon_policy", 1)
        sc.set_option("f64_mesh_tree_min", tree_min)
        r = Renderer(sc, Camera())
        res[tree_min] = r.get_closest_hit_f64(o, d)
        info = r.f64_mesh_tree_info()
        if tree_min:
            assert info["meshes"] == (2 if case == "leaf roots" else 1) and info["render_uses_trees"] == 1 and info["tree_min"] == 1
            assert info["depth"] == 0 if case == "leaf roots" else info["depth"] > 3
        else:
            assert info["meshes"] == 0 and info["nodes"] == 0 and info["render_uses_trees"] == 0
    (t1, obj1, n1), (t0, obj0, n0) = res[1], res[0]
    hit = obj0 >= 0
    print(f"{case}: {len(o)} rays, {int(hit.sum())} hits, {int((t0[hit] < 1e-9).sum())} self-hits")
    assert hit.sum() > len(o) // 5
    assert np.array_equal(obj1, obj0)
    assert _same_bits(t1, t0)
    assert _same_bits(n1[hit], n0[hit])
    if case == "duplicates":      # the winner of two coincident triangles is the lower index: its normals, not the copy's
        base, sign = extra
        ref = Scene()
        ref.add(Object(Mesh(base)).material(Material.diffuse(vec3(0.7, 0.7, 0.7))))
        ref.set_option("epsilon_policy", 1)
        ref.set_option("f64_mesh_tree_min", 0)
        tb, objb, nb = Renderer(ref, Camera()).get_closest_hit_f64(o, d)
        # which geometric triangle: the one whose plane and interior hold the hit point (interior hits only: unambiguous)
        with np.errstate(invalid="ignore"):
            p = o + tb[:, None] * d                         # (a miss: t = inf)
        v1, e0, e1 = base[:, 0], base[:, 1] - base[:, 0], base[:, 2] - base[:, 0]
        nn = _unit(np.cross(e0, e1))
        ok = hit & (objb >= 0) & (tb == t0) & (tb > 1e-6)
        idx = np.flatnonzero(ok)
        rel = p[idx, None, :] - v1[None, :, :]
        dist = np.abs(np.einsum("rkc,kc->rk", rel, nn))
        d00, d01, d11 = (e0 * e0).sum(1), (e0 * e1).sum(1), (e1 * e1).sum(1)
        d20, d21 = np.einsum("rkc,kc->rk", rel, e0), np.einsum("rkc,kc->rk", rel, e1)
        den = d00 * d11 - d01 * d01
        bv, bw = (d11 * d20 - d01 * d21) / den, (d00 * d21 - d01 * d20) / den
        inside = (dist < 1e-9) & (bv > 1e-3) & (bw > 1e-3) & (1 - bv - bw > 1e-3)
        sure = inside.sum(axis=1) == 1
        g = inside.argmax(axis=1)[sure]
        rows = idx[sure]
        assert len(rows) > 1000
        assert np.array_equal(n1[rows], sign[g][:, None] * nb[rows])      # (negating the vertex normals negates the result exactly)
        assert (sign[g] > 0).sum() > 100 and (sign[g] < 0).sum() > 100


# ------------------------------------------------------------------ 2. hits against the literal oracle
def test_hits_with_trees_follow_the_literal_oracle():
    """Bounds of test_gpu_monomial.py (test_fp64_hits_through_groups_and_transforms): the same object for 99.95 % of the rays, t within
    1e-12 relative and the normal within 1e-9 where both hit it."""
    sc, targets, _ = _hit_scene("torus")
    rng = np.random.default_rng(29)
    parts = []
    for tris, m in targets:
        o, d = _rays(tris, m, rng, 2000)
        parts.append((o[:2000], d[:2000]))                  # the random kind (the oracle's own kd-tree decides edge-on rays for itself)
    o, d = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    te, obje, nrme = _oracle(sc).intersect(o, d, robust=0)
    sc.set_option("epsilon_policy", 1)
    sc.set_option("f64_mesh_tree_min", 1)
    r = Renderer(sc, Camera())
    t, obj, nrm = r.get_closest_hit_f64(o, d)
    assert r.f64_mesh_tree_info()["render_uses_trees"] == 1
    same = obj == obje
    assert same.mean() > 0.9995
    hit = same & (obj >= 0) & np.isfinite(te)
    assert hit.sum() > 1000
    assert np.max(np.abs(t[hit] - te[hit]) / np.abs(te[hit])) < 1e-12
    assert np.max(np.abs(nrm[hit] - nrme[hit])) < 1e-9


# ------------------------------------------------------------------ 3. frames, tree = scan
def _mesh_light(fog):
    """A mesh as a Light::Object with its twin among the objects, over a plane and beside a second mesh."""
    sc = Scene()
    lamp = Mesh(scenes.bumpy_torus(8, 6)).scale(vec3(1.5, 1.5, 1.5)).rotate_x(0.4).translate(vec3(0.0, 2.2, 0.0))
    glow = Material.light(vec3(1.0, 0.9, 0.8), 20.0)
    sc.add(Object(lamp.clone()).material(glow))
    sc.add(Light.Object(Object(lamp.clone()).material(glow)))
    sc.add(Object(Mesh(scenes.bumpy_torus(16, 10)).scale(vec3(2.5, 2.5, 2.5))).material(Material.specular(vec3(0.8, 0.6, 0.3), 0.3)))
    sc.add(Object(plane(vec3(0, 1, 0), -1.0)).material(Material.diffuse(vec3(0.8, 0.8, 0.8))))
    sc.add(Light.Ambient(vec3(0.02, 0.02, 0.02)))
    if fog:
        sc.add(Medium.homogeneous_isotropic(0.02, 0.08))
    return sc, Camera.look_at(vec3(0.0, 2.0, 6.0), vec3(0.0, 0.5, 0.0), vec3(0, 1, 0), 0.8), {"max_bounces": 3}


FRAME_SCENES = {
    "mesh in fog": lambda: scenes.mesh_in_fog(24, 12),
    "mesh among spheres": lambda: scenes.mesh_among_spheres(24, 12, n_spheres=8),
    "fractal meshes": lambda: scenes.fractal_meshes(levels=2, nu=12, nv=6),
    "mesh light": lambda: _mesh_light(False),
    "mesh light in fog": lambda: _mesh_light(True),
}


@pytest.mark.parametrize("name", list(FRAME_SCENES))
def test_frames_with_trees_equal_the_scan_bit_for_bit(name):
    """64 x 64 x 8, the counters build and the plain one: equal frames, equal work counters."""
    size, spp = 64, 8
    frames, counts = {}, {}
    for tree_min in (1, 0):
        sc, cam, cfg = _with_trees(FRAME_SCENES[name], tree_min, counters=1)
        r = Renderer(sc, cam).width(size).height(size).max_bounces(cfg["max_bounces"]).seed(13)
        with_counters = r.sample_array(spp)
        counts[tree_min] = _eps_counters(r)
        sc.set_option("counters", 0)
        r._sample_offset = 0
        frames[tree_min] = r.sample_array(spp)
        assert _same_bits(frames[tree_min], with_counters), (name, tree_min)
        info = r.f64_mesh_tree_info()
        assert info["render_uses_trees"] == tree_min and (info["meshes"] > 0) == bool(tree_min), (name, info)
    assert np.all(np.isfinite(frames[0])) and frames[0].mean() > 0
    assert _same_bits(frames[1], frames[0]), (name, int((frames[1] != frames[0]).any(axis=1).sum()))
    for k in COUNTERS:
        assert counts[1][k] == counts[0][k], (name, k, counts[1][k], counts[0][k])
    assert counts[0]["hits"] > 0


# ------------------------------------------------------------------ 4. a frame against the literal oracle
def test_a_frame_with_trees_follows_the_literal_oracle():
    """mesh_in_fog(24, 12) with trees, with the assertions of test_small_renders_follow_the_literal_oracle at its size (96 x 96 x 32)."""
    size, spp = 96, 32
    scene, cam, cfg = _with_trees(lambda: scenes.mesh_in_fog(24, 12), 1, counters=1)
    r = Renderer(scene, cam).width(size).height(size).max_bounces(cfg["max_bounces"]).seed(3)
    got = r.sample_array(spp)
    cnt = _eps_counters(r)
    assert r.f64_mesh_tree_info()["render_uses_trees"] == 1
    exp, oc = _oracle(scene).render(cam, size, size, spp, cfg["max_bounces"], seed=3, robust=0, counters=True)
    print(f"rel RMS {rel_rms(got, exp):.3e}, mean {got.mean():.6e} against {exp.mean():.6e}")
    assert np.all(np.isfinite(got)) and exp.mean() > 0
    assert rel_rms(got, exp) < 2e-3
    assert abs(got.mean() - exp.mean()) < 1e-4 * exp.mean()
    for k in ("rays", "hits", "samples", "vertices", "shadow_tests", "shadow_pass"):
        assert abs(cnt[k] - oc[k]) <= 2e-3 * max(oc[k], 1) + 2, (k, cnt[k], oc[k])
    for k in ("self_hits", "shadow_near"):
        assert abs(cnt[k] - oc[k]) <= 0.05 * oc[k] + 3.0 * np.sqrt(oc[k] + 1.0), (k, cnt[k], oc[k])


# ------------------------------------------------------------------ 5. schedule
def test_tree_flavour_on_small_grids():
    """The pattern of test_gpu_schedule.py for the tree flavour: the 960-triangle mesh in fog of its "records outside LDS" case, 96 x 72 x
    24, on the default grid (one item per lane), on 1 block and on an odd number of blocks (8 or more items per lane), crossed with
    "pull_batch" and "f64_surf_batch"; every frame equals the isolated one, the counters build's too; and that one equals the scan's."""
    from tests.test_gpu_schedule import FP64_COUNTERS, _mesh_in_fog_scene, _pt_items, _run_grids
    w, h, spp, mb, seed = 96, 72, 24, 3, 11
    sc, cam = _with_trees(_mesh_in_fog_scene, 1)
    r = Renderer(sc, cam).width(w).height(h).max_bounces(mb).seed(seed)
    assert r.f64_mesh_tree_info()["render_uses_trees"] == 1
    variants = [{"pull_batch": 2, "f64_surf_batch": 8}, {"pull_batch": 1, "f64_surf_batch": 64}, {"pull_batch": 64, "f64_surf_batch": 1}]
    iso = _run_grids(f"render_f64_kernel mesh trees {w}x{h}x{spp}", r, lambda: r.sample_array(spp), _pt_items(r, w, h, spp), variants,
                     counters=_eps_counters, counter_keys=FP64_COUNTERS, counters_keep_the_frame=True)
    sc0, cam0 = _with_trees(_mesh_in_fog_scene, 0)
    scan = Renderer(sc0, cam0).width(w).height(h).max_bounces(mb).seed(seed).sample_array(spp)
    assert _same_bits(iso, scan)


# ------------------------------------------------------------------ 6. fallbacks and interface
def _mono_and_mesh():
    sc = Scene()
    sc.add(Object(monomial_surface(2.0, 4.0).translate(vec3(0.0, -1.0, 0.0))).material(Material.metallic(vec3(1, 1, 1), 0.0001)))
    sc.add(Object(Mesh(scenes.bumpy_torus(24, 12)).scale(vec3(1.5, 1.5, 1.5)).translate(vec3(0.3, 0.2, 0.0))).material(
        Material.specular(vec3(0.8, 0.4, 0.3), 0.3)))
    sc.add(Object(plane(vec3(0, 1, 0), -1.0)).material(Material.diffuse(vec3(0.7, 0.7, 0.7))))
    sc.add(Light.Ambient(vec3(0.05, 0.05, 0.05)))
    sc.add(Light.Point(vec3(100.0, 100.0, 100.0), vec3(0.0, 5.0, 5.0)))
    return sc, Camera.look_at(vec3(0.0, 1.5, 5.0), vec3(0.0, 0.0, 0.0), vec3(0, 1, 0), 0.8), {"max_bounces": 2}


def test_a_scene_with_a_monomial_surface_keeps_the_scan_and_says_so():
    frames, hits = {}, {}
    rng = np.random.default_rng(3)
    o = np.array([0.3, 3.0, 0.0]) + 0.1 * rng.standard_normal((4000, 3))      # from above, into the glass: the mesh floats in it
    d = _unit(np.array([0.3, 0.2, 0.0]) + rng.uniform(-1.0, 1.0, (4000, 3)) * np.array([0.9, 0.1, 0.9]) - o)
    for tree_min in (1, 0):
        sc, cam, cfg = _with_trees(_mono_and_mesh, tree_min)
        r = Renderer(sc, cam).width(64).height(64).max_bounces(cfg["max_bounces"]).seed(5)
        frames[tree_min] = r.sample_array(8)
        hits[tree_min] = r.get_closest_hit_f64(o, d)
        info = r.f64_mesh_tree_info()
        assert info["render_uses_trees"] == 0 and info["photon_uses_trees"] == 0
        assert (info["meshes"], info["triangles"]) == ((1, 576) if tree_min else (0, 0))
    assert np.all(np.isfinite(frames[0])) and frames[0].mean() > 0
    assert _same_bits(frames[1], frames[0])
    assert (hits[0][1] == 1).sum() > 200                     # the mesh is in view
    assert np.array_equal(hits[1][1], hits[0][1]) and _same_bits(hits[1][0], hits[0][0])


def test_the_photon_passes_keep_the_scan_and_say_so():
    n, size, spp = 5000, 32, 4
    images, frames = {}, {}
    for tree_min in (1, 0):
        sc, cam, cfg = _with_trees(lambda: scenes.mesh_in_fog(24, 12), tree_min)
        r = Renderer(sc, cam).width(size).height(size).watts(60.0).gather_size(20).gather_size_volume(3).seed(4)
        images[tree_min] = np.asarray(r.photon_point_query_beam_render(n))
        frames[tree_min] = r.photon_sample_array(spp)
        info = r.f64_mesh_tree_info()
        assert info["photon_uses_trees"] == 0 and info["render_uses_trees"] == tree_min
    assert np.all(np.isfinite(frames[0])) and frames[0].mean() > 0
    assert np.array_equal(images[1], images[0])
    assert _same_bits(frames[1], frames[0])


def test_info_needs_the_mode_and_the_defaults_leave_c3_alone():
    sc, cam, _ = scenes.mesh_in_fog(24, 12)
    with pytest.raises(RptError) as e:
        Renderer(sc, cam).f64_mesh_tree_info()
    assert "rpt error -2" in str(e.value)                    # RPT_ERR_STATE
    for name in ("C2", "C3"):
        scene, cam, _ = scenes.CONFIGS[name]()
        scene.set_option("epsilon_policy", 1)
        info = Renderer(scene, cam).f64_mesh_tree_info()
        assert info["meshes"] == 0 and info["nodes"] == 0 and info["bytes"] == 0 and info["render_uses_trees"] == 0, (name, info)
        assert info["tree_min"] > 12                         # their 12-triangle meshes stay on the scan


# ------------------------------------------------------------------ 7. size
def test_c5s_mesh_with_default_options():
    """mesh_in_fog(224, 224), 100,352 triangles, 64 x 64 x 4 with default options: the mesh has a tree, and the frame is the scan's."""
    size, spp = 64, 4
    out = {}
    frames = {}
    for label, opts in (("tree", {}), ("scan", {"f64_mesh_tree_min": 0})):
        sc, cam, cfg = scenes.mesh_in_fog(224, 224)
        sc.set_option("epsilon_policy", 1)
        sc.set_option("timing", 1)
        for k, v in opts.items():
            sc.set_option(k, v)
        r = Renderer(sc, cam).width(size).height(size).max_bounces(cfg["max_bounces"]).seed(1)
        frames[label] = r.sample_array(spp)
        out[label + "_kernel_ms"] = r.timing()[0]
        out[label + "_info"] = r.f64_mesh_tree_info()
    info = out["tree_info"]
    assert info["meshes"] == 1 and info["triangles"] == 100352 and info["render_uses_trees"] == 1 and 0 < info["depth"] <= 20
    assert out["scan_info"]["meshes"] == 0
    print(out)
    path = os.environ.get("RPT_MESH_TREE_LOG")             # (a file to keep the kernel times in, if one is named)
    if path:
        with open(path, "w") as f:
            json.dump(dict(out, size=[size, size, spp]), f, indent=1)
    assert np.all(np.isfinite(frames["scan"])) and frames["scan"].mean() > 0
    assert _same_bits(frames["tree"], frames["scan"])
