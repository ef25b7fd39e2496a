"""Closest hits on structured rays, ray by ray, in both modes (tests/ray_cloud.py has the rule and the rays; test_ray_cloud_host.py pins
them with the oracle alone).

Every ray of every family -- exact zeros of both signs in the direction, rays through vertices, edges, corners and face planes, silhouette
cones, origins on surfaces, random ones -- is put to rpt_intersect_batch under ten flatten-time layouts, to rpt_intersect_batch_f64 with and
without candidate trees for every mesh, and to rpt_intersect_segments; the answer must be one the oracle gives in the ray's cloud: this
object, this t, this normal for a decided ray.  No quantile.  The library is compared with itself only where the headers document bit
identity: "scan_specialise" on = off, "room_shell" on = off for rays that hit no wall, rpt_intersect_segments with t_max = inf =
rpt_intersect_batch.

Both modes pass on every ray.  Three defects that these rays found at the edges of records are fixed with them ("Structured
rays"): a ray on the edge two triangles share passed through the mesh, a box hit on a silhouette edge could carry the hidden face's
normal, and a ray at the common edge of two wall rectangles could leave the room.

Each test prints one line per family: rays, decided, failures, worst t error, worst normal error."""
import ctypes as C

import numpy as np
import pytest

from rpt_amd import Camera, Renderer, _lib
from tests import ray_cloud as rc

pytestmark = pytest.mark.gpu

MISS = 0xFFFFFFFF
N_TORUS = 192
# reference-epsilon mode: a hit names a record, and the shapes of a group are records of their own ("First-hit feature buffers")
F64_RECORD_OBJECT = np.array([0, 1, 2, 3, 4, 4, 4, 4, 4, 5, 6, 7, 8, 9])


# layout -> (scene variant of ray_cloud.VARIANTS, scene options, what scene_stats() must say)
def _per_mesh_trees(st, meshes):
    return st["scene_bvh"] == 0 and st["instances"] == 0 and st["shared_meshes"] == 0 and st["bvh_tris"] == meshes * N_TORUS and st["bvh_nodes"] > 0


LAYOUTS = {
    "default": ("base", {}, lambda st: _per_mesh_trees(st, 1) and st["shell_faces"] == 5 and st["rects"] == 5 and st["aabbs"] == 1),
    "room_shell 0": ("base", {"room_shell": 0}, lambda st: _per_mesh_trees(st, 1) and st["shell_faces"] == 0 and st["rects"] == 5 and st["aabbs"] == 1),
    "scan_specialise 0": ("base", {"scan_specialise": 0}, lambda st: _per_mesh_trees(st, 1) and st["shell_faces"] == 5 and st["rects"] == 5),
    "per-mesh trees, linear scan": ("base", {"instancing": 0, "scene_bvh_min": 1 << 20},
                                    lambda st: _per_mesh_trees(st, 1) and st["shell_faces"] == 5 and st["aabbs"] == 1),
    "bvh_leaf_max 1": ("base", {"bvh_leaf_max": 1}, lambda st: _per_mesh_trees(st, 1) and st["bvh_nodes"] == N_TORUS - 1),
    "bvh_sweep_below 0": ("base", {"bvh_sweep_below": 0}, lambda st: _per_mesh_trees(st, 1)),
    "scene tree": ("lattice", {}, lambda st: st["scene_bvh"] == 2 and st["scene_bvh_prims"] > 64 and st["shell_faces"] == 0 and st["instances"] == 0
                   and st["bvh_tris"] == N_TORUS),
    "scene tree, meshes inside": ("lattice", {"scene_tree_meshes": 1},
                                  lambda st: st["scene_bvh"] == 1 and st["scene_bvh_prims"] > 64 and st["shell_faces"] == 0 and st["instances"] == 0),
    "instances": ("instances", {}, lambda st: st["scene_bvh"] == 1 and st["instances"] == 2 and st["shared_meshes"] == 1 and st["bvh_tris"] == N_TORUS),
    "two per-mesh trees, linear scan": ("instances", {"instancing": 0, "scene_bvh_min": 1 << 20},
                                        lambda st: _per_mesh_trees(st, 2) and st["shell_faces"] == 5 and st["spheres"] == 1 + 4 + 64),
}
_answers = {}


def _renderer(variant, options):
    sc = rc.scene(**rc.VARIANTS[variant])
    for k, v in options.items():
        sc.set_option(k, v)
    return Renderer(sc, Camera())


def _answer(layout):
    """(obj, t, nrm) of every ray under the layout, once per process."""
    if layout not in _answers:
        variant, options, claim = LAYOUTS[layout]
        r = _renderer(variant, options)
        st = r.scene_stats()
        print(f"{layout}: {st}")
        assert claim(st), (layout, st)
        p = rc.prepared("fp32", variant)
        t, obj, nrm = r.get_closest_hit(p["o"], p["d"])
        _answers[layout] = (obj, t, nrm)
    return _answers[layout]


def _f64_answer(tree_min):
    sc = rc.scene()
    sc.set_option("epsilon_policy", 1)
    if tree_min is not None:
        sc.set_option("f64_mesh_tree_min", tree_min)
    r = Renderer(sc, Camera())
    info = r.f64_mesh_tree_info()
    print(info)
    # by default the torus alone has a candidate tree; with 1 every mesh has one, the two-triangle walls too
    assert info["render_uses_trees"] == 1 and (info["meshes"], info["triangles"]) == ((1, N_TORUS) if tree_min is None else (6, N_TORUS + 10))
    p = rc.prepared("fp64")
    t, rec, nrm = r.get_closest_hit_f64(p["o"], p["d"])
    assert rec.min() >= -1 and rec.max() < len(F64_RECORD_OBJECT)
    return np.where(rec >= 0, F64_RECORD_OBJECT[np.maximum(rec, 0)], -1), t, nrm


def _report(title, p, rep):
    rc.print_table(title, rc.table(p["cloud"], p["family"], p["names"], rep, groups=rc.GROUPS))


# ------------------------------------------------------------------ fp32
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_fp32_closest_hits_ray_by_ray(layout):
    obj, t, nrm = _answer(layout)
    p = rc.prepared("fp32", LAYOUTS[layout][0])
    rep = rc.check(p["cloud"], obj, t, nrm, "fp32", p["family"], p["names"], layout=f"{layout} {LAYOUTS[layout][1]}")
    _report(f"fp32, {layout}", p, rep)
    assert not rep.failed.any(), f"{int(rep.failed.sum())} rays fail (printed above)"


def test_fp32_layouts_agree_where_the_headers_say_bit_for_bit():
    """The object of a decided ray is the same under every layout by the rule alone (each names the oracle's).  t: bit-equal between
    "scan_specialise" 1 and 0, and between "room_shell" 1 and 0 on rays that hit no wall."""
    base = _answer("default")
    obj, t, nrm = _answer("scan_specialise 0")
    assert np.array_equal(obj, base[0]) and np.array_equal(t.view(np.uint32), base[1].view(np.uint32))
    assert np.array_equal(nrm.view(np.uint32), base[2].view(np.uint32))
    obj, t, nrm = _answer("room_shell 0")
    no_wall = ~np.isin(obj, range(5, 10)) & ~np.isin(base[0], range(5, 10))
    assert no_wall.sum() > 8000
    assert np.array_equal(obj[no_wall], base[0][no_wall]) and np.array_equal(t[no_wall].view(np.uint32), base[1][no_wall].view(np.uint32))
    assert np.array_equal(nrm[no_wall].view(np.uint32), base[2][no_wall].view(np.uint32))


# ------------------------------------------------------------------ fp64
@pytest.mark.parametrize("tree_min", [None, 1])
def test_fp64_closest_hits_ray_by_ray(tree_min):
    obj, t, nrm = _f64_answer(tree_min)
    p = rc.prepared("fp64")
    rep = rc.check(p["cloud"], obj, t, nrm, "fp64", p["family"], p["names"], layout=f"fp64, f64_mesh_tree_min {tree_min}")
    _report(f"fp64, f64_mesh_tree_min {tree_min}", p, rep)
    assert not rep.failed.any(), f"{int(rep.failed.sum())} rays fail (printed above)"


# ------------------------------------------------------------------ segments
def _segments(r, o, d, tmax):
    n = len(o)
    o32, d32, m32 = (np.ascontiguousarray(a, dtype=np.float32) for a in (o, d, tmax))
    t, code = np.empty(n, dtype=np.float32), np.empty(n, dtype=np.uint32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    _lib.check(_lib.load().rpt_intersect_segments(r.scene._commit(r.device_), n, vp(o32), vp(d32), vp(m32), vp(t), vp(code)))
    return t, code


def _scan_answers():
    """The linear-scan scene's answers -> closest hits (obj, t, nrm) and the segments' (t, code) for t_max = inf, t (1 + 1e-3), t (1 - 1e-3)
    on the decided hits (inf elsewhere)."""
    r = _renderer("scan", {})
    st = r.scene_stats()
    print(st)
    assert st["bvh_nodes"] == 0 and st["scene_bvh"] == 0 and st["instances"] == 0 and st["tris"] == 32 and st["shell_faces"] == 5 and st["aabbs"] == 1
    p = rc.prepared("fp32", "scan")
    cl, o, d = p["cloud"], p["o"], p["d"]
    t_b, obj_b, nrm_b = r.get_closest_hit(o, d)
    out = {"batch": (obj_b, t_b, nrm_b), "inf": _segments(r, o, d, np.full(len(o), np.inf))}
    hits = cl.decided & (cl.obj[:, 0] >= 0)
    for name, f in (("longer", 1.0 + 1e-3), ("shorter", 1.0 - 1e-3)):
        out[name] = _segments(r, o, d, np.where(hits, cl.t[:, 0] * f, np.inf))
    return out


def test_segments_ray_by_ray():
    """rpt_intersect_segments is the linear scan's query: the scene with the torus at 32 triangles (triangle records, no tree).  A hit code
    names a record, not an object; which object a code belongs to is read off the rays that rpt_intersect_batch answers with the same
    bits (the t_max = inf run), and that query's objects are held to the rule first."""
    ans = _scan_answers()
    p = rc.prepared("fp32", "scan")
    cl, o, d = p["cloud"], p["o"], p["d"]
    n = len(o)
    obj_b, t_b, nrm_b = ans["batch"]
    rep = rc.check(cl, obj_b, t_b, nrm_b, "fp32", p["family"], p["names"], layout="linear scan, 32-triangle torus")
    _report("fp32, linear scan", p, rep)
    assert not rep.failed.any()
    # t_max = inf: rpt_intersect_batch bit for bit, on all rays
    t_inf, code_inf = ans["inf"]
    assert np.array_equal(t_inf.view(np.uint32), t_b.view(np.uint32))
    assert np.array_equal(code_inf == MISS, obj_b < 0)
    owner = {}
    for c, ob in zip(code_inf.tolist(), obj_b.tolist()):
        assert owner.setdefault(c, ob) == ob, "one hit code, two objects"
    assert len(set(owner.values())) == len(rc.OBJECTS) + 1
    # the decided hits, cut just behind and just before the oracle's t
    t_ref = cl.t[:, 0]
    hits = cl.decided & (cl.obj[:, 0] >= 0)
    assert hits.sum() > 30000
    t_l, code_l = ans["longer"]
    assert set(np.unique(code_l).tolist()) <= set(owner)
    obj_l = np.array([owner[c] for c in code_l.tolist()])
    rep = rc.check(cl, obj_l, np.where(obj_l < 0, np.inf, t_l), None, "fp32", p["family"], p["names"], layout="segments, t_max = t (1 + 1e-3)")
    _report("segments, t_max = t (1 + 1e-3)", p, rep)
    assert not rep.failed.any() and np.all(obj_l[hits] == cl.obj[hits, 0])
    t_s, code_s = ans["shorter"]
    shorter = np.where(hits, t_ref * (1.0 - 1e-3), np.inf).astype(np.float32)
    wrong = np.flatnonzero(hits & (code_s != MISS))
    print(f"segments, t_max = t (1 - 1e-3): {int(hits.sum())} decided hits, {len(wrong)} not missed")
    for i in wrong[:8]:
        print(f"  ray {i} [{p['names'][p['family'][i]]}] o = {o[i].tolist()!r} d = {d[i].tolist()!r} t_ref {t_ref[i]!r}: code {code_s[i]:#x} t {t_s[i]!r}")
    assert len(wrong) == 0
    assert np.array_equal(t_s[hits].view(np.uint32), shorter[hits].view(np.uint32))         # a miss leaves t_max in t
