"""Closest hits ray by ray: what to demand of a ray that may lie exactly on a decision boundary (CPU only: numpy + the oracle).

A closest-hit query decides things: which face of a box, which of two triangles that share an edge, hit or graze, self-hit or not.
On a ray that lies exactly on such a boundary the fp32 (or fp64) arithmetic of the library and the fp64 arithmetic of the oracle may
decide differently and both be right.  So the oracle is asked not about the ray alone but about a small cloud around it
(`cloud`), and the library's answer has to be one the cloud contains (`check`): one rule for every ray, no quantile, no exceptions.

  mode     oracle policy   amplitude on the origin      on the direction   b_t      b_n
  "fp32"   robust = 1      2e-6 (1 + max|o|)            2e-6               2e-4     5e-3     (rays rounded to fp32 first)
  "fp64"   robust = 0      1e-14 (1 + max|o|)           1e-14              1e-12    1e-9

The fp32 amplitude is a tenth of the library's self-hit scale, ray_tmin = 2e-5 (1 + max|o|); the fp64 one a hundredth of the
reference's EPSILON = 1e-12.  b_t and b_n are the bounds the suite already uses for single hits (test_gpu_fuzz.py;
test_gpu_epsilon_mesh_tree.py).

First pass: the ray itself and 16 seeded random perturbations.  Second pass, only for rays whose 17 answers name different objects:
the 26 origin offsets {-a, 0, a}^3 \\ {0}, the same 26 on the direction, and 32 more random ones.  Third pass, for the same rays
(`_edge_of_the_answers`): at a silhouette t approaches its end like sqrt(2 R delta) in the lateral offset delta, so 50 hits spread over
8e-6 stop about 1.8e-4 (relative, at t = 2.8) short of the tangent point, against b_t = 2e-4, while the library may answer from anywhere
in the neighbourhood; a larger amplitude does not move the samples closer.  72 answers more come from bisections between two of the
samples towards the place where an object's hits end.  Each is the oracle's answer for a ray inside the neighbourhood; no bound and no
amplitude is changed.  A ray is *decided* when every answer
of its cloud names the same object (or every answer is a miss), the t values agree within b_t and the normals within b_n: for such a
ray the rule is "this object, this t, this normal".

The scene (`scene`) holds every record kind: an axis-aligned box, a cube rotated about the vertical axis, a scaled sphere, a closed mesh
of 192 triangles, a group of four spheres and a cube under rotate_z, and five walls of the box [-5, 5]^3 (the side x = +5 is open:
rays can miss).  `families` is the set of rays: structured ones (exact zeros of both signs in the direction, rays through vertices,
edges, corners, face planes and silhouettes, origins on surfaces) and random ones as a control."""
import itertools

import numpy as np

from rpt_amd import KdTree, Material, Mesh, Object, Scene, cube, polygon, scenes, sphere, vec3

MODES = {
    "fp32": {"robust": 1, "amp": 2e-6, "b_t": 2e-4, "b_n": 5e-3, "dtype": np.float32},
    "fp64": {"robust": 0, "amp": 1e-14, "b_t": 1e-12, "b_n": 1e-9, "dtype": np.float64},
}
N_FIRST, N_MORE = 16, 32
LO, HI = -5.0, 5.0
OBJECTS = ["box", "rotated cube", "sphere", "torus", "group", "wall z-", "wall z+", "wall y-", "wall y+", "wall x-"]
BOX_LO, BOX_HI = np.array([-2.5, -0.25, -0.375]), np.array([-1.5, 0.25, 0.375])
TORUS_SCALE, TORUS_AT = 3.0, np.array([0.0, -2.0, 0.0])
SPHERE_SCALE, SPHERE_AT = np.array([1.0, 0.6, 0.8]), np.array([0.0, 2.5, 1.5])
EYE = np.array([3.5, 3.0, 4.0])
CONE_EYE = np.array([0.1, 0.0, -0.2])     # close to the origin: the cloud's amplitude grows with max|o|, and a grazing hit magnifies it

# families by what the host test asks of them
INTERIOR = ("axis", "one zero", "torus centroids", "cone 0.99 ", "cone 0.999 ", "cone 1.001 ", "cone 1.01 ", "surface steep", "random")
BOUNDARY = ("torus vertices", "box planes", "box edges", "cone 1 ", "room edges")
GROUPS = INTERIOR + BOUNDARY + ("torus edges", "surface shallow", "near surface")     # every ray belongs to exactly one


def scene(lattice=False, torus=(12, 8), second_use=False):
    """The scene of the structured-ray tests -> Scene; object i is OBJECTS[i].  lattice: 64 small spheres more (objects 10..73), enough
    for the scene-level tree.  torus: (nu, nv) of the mesh; (4, 4) gives 32 triangles, which the library scans as triangle records.
    second_use: the torus's mesh once more, smaller and rotated (the last object): a mesh with two uses is stored once and instanced."""
    sc = Scene()
    grey = Material.diffuse(vec3(0.7, 0.7, 0.7))
    sc.add(Object(cube().scale(vec3(1.0, 0.5, 0.75)).translate(vec3(-2.0, 0.0, 0.0))).material(grey))
    sc.add(Object(cube().scale(vec3(1.2, 0.8, 1.0)).rotate_y(0.5).translate(vec3(2.5, 1.5, -1.5))).material(grey))
    sc.add(Object(sphere().scale(vec3(*SPHERE_SCALE)).translate(vec3(*SPHERE_AT))).material(grey))
    mesh = Mesh(scenes.bumpy_torus(*torus))
    sc.add(Object(mesh.scale(vec3(TORUS_SCALE, TORUS_SCALE, TORUS_SCALE)).translate(vec3(*TORUS_AT))).material(grey))
    kids = [sphere().scale(vec3(0.4, 0.4, 0.4)).translate(vec3(x, y, 0.0)) for x in (-0.6, 0.6) for y in (-0.6, 0.6)]
    kids.append(cube().scale(vec3(0.5, 0.5, 0.5)).translate(vec3(0.0, 0.0, 0.8)))
    sc.add(Object(KdTree(kids).rotate_z(0.4).translate(vec3(2.8, -2.5, 2.5))).material(grey))
    c = [[LO, LO, LO], [HI, LO, LO], [HI, HI, LO], [LO, HI, LO], [LO, LO, HI], [HI, LO, HI], [HI, HI, HI], [LO, HI, HI]]
    for q in [(0, 1, 2, 3), (4, 7, 6, 5), (0, 4, 5, 1), (3, 2, 6, 7), (0, 3, 7, 4)]:
        sc.add(Object(polygon([vec3(*c[k]) for k in q])).material(grey))
    if lattice:
        for i, j, k in itertools.product(range(4), repeat=3):
            at = vec3(-4.2 + 0.4 * i, 1.0 + 0.4 * j, -4.2 + 0.4 * k)
            sc.add(Object(sphere().scale(vec3(0.12, 0.12, 0.12)).translate(at)).material(grey))
    if second_use:
        sc.add(Object(mesh.scale(vec3(1.5, 1.5, 1.5)).rotate_y(0.7).rotate_x(0.3).translate(vec3(-2.5, -3.5, 2.5))).material(grey))
    return sc


def oracle_scene(sc):
    from oracle.pyoracle import OracleScene
    return OracleScene(sc)


# ------------------------------------------------------------------ rays
def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _axis_rays(points, axis, sense, zero=0.0):
    """Rays along `sense` * axis from 0.1 inside the wall behind them: origin = the point with that coordinate set to -sense * 4.9,
    the direction's two other components `zero` (+0.0 or -0.0)."""
    o = np.array(points, dtype=np.float64).reshape(-1, 3)
    o[:, axis] = -sense * 4.9
    d = np.full_like(o, zero)
    d[:, axis] = sense
    return o, d


def _torus_points():
    """World-space vertices, edge midpoints and centroids of the torus."""
    tris = scenes.bumpy_torus(12, 8)[:, :3, :] * TORUS_SCALE + TORUS_AT
    verts, inv = np.unique(tris.reshape(-1, 3).round(12), axis=0, return_inverse=True)
    inv = inv.reshape(-1, 3)
    edges = np.unique(np.sort(np.concatenate([inv[:, [0, 1]], inv[:, [1, 2]], inv[:, [2, 0]]]), axis=1), axis=0)
    return verts, 0.5 * (verts[edges[:, 0]] + verts[edges[:, 1]]), tris.mean(axis=1)


def _box_edge_points(lo, hi, per_edge):
    s = np.linspace(0.0, 1.0, per_edge)[:, None]
    out = []
    for axis in range(3):
        u, w = (axis + 1) % 3, (axis + 2) % 3
        for cu, cw in itertools.product((lo[u], hi[u]), (lo[w], hi[w])):
            a, b = np.zeros(3), np.zeros(3)
            a[axis], b[axis] = lo[axis], hi[axis]
            a[u] = b[u] = cu
            a[w] = b[w] = cw
            out.append(a + s * (b - a))
    return np.concatenate(out)


def _silhouette(factor, n):
    """Rays from CONE_EYE on the cone `factor` x the tangent angle of the scaled sphere (the cone is circular in the sphere's own space)."""
    e = (CONE_EYE - SPHERE_AT) / SPHERE_SCALE
    dist = np.linalg.norm(e)
    axis = -e / dist
    theta = factor * np.arcsin(1.0 / dist)
    u = _unit(np.cross(axis, [0.0, 1.0, 0.0]))
    v = np.cross(axis, u)
    phi = np.arange(n) * (2 * np.pi / n) + 0.003
    dl = np.cos(theta) * axis + np.sin(theta) * (np.cos(phi)[:, None] * u + np.sin(phi)[:, None] * v)
    return np.broadcast_to(CONE_EYE, (n, 3)).copy(), _unit(dl * SPHERE_SCALE)


def families(mode, osc):
    """-> [(name, origins, directions)]: fp64 arrays of values of the mode's type, every direction finite and of unit length (to the
    rounding of the type).  osc: the OracleScene of scene() (the origins on surfaces are its hit points)."""
    cfg = MODES[mode]
    rng = np.random.default_rng(20261)
    fam = []
    # axis-parallel lattices, 49 x 49, with both signs of zero
    g = np.linspace(-4.9, 4.9, 49)
    for axis, sense in itertools.product(range(3), (1.0, -1.0)):
        p = np.zeros((49 * 49, 3))
        a, b = np.meshgrid(g, g, indexing="ij")
        p[:, (axis + 1) % 3], p[:, (axis + 2) % 3] = a.ravel(), b.ravel()
        for zero, zname in ((0.0, "+0"), (-0.0, "-0")):
            fam.append((f"axis {'+-'[sense < 0]}{'xyz'[axis]} {zname}",) + _axis_rays(p, axis, sense, zero))
    # one zero component
    for axis in range(3):
        o = rng.uniform(-4.5, 4.5, (2000, 3))
        tgt = rng.uniform(-3.0, 3.0, (2000, 3))
        tgt[:, axis] = o[:, axis]
        fam.append((f"one zero {'xyz'[axis]}", o, _unit(tgt - o)))
    # torus vertices, edge midpoints, centroids: along each axis and from the eye
    for what, pts in zip(("vertices", "edges", "centroids"), _torus_points()):
        for axis in range(3):
            fam.append((f"torus {what} -{'xyz'[axis]}",) + _axis_rays(pts, axis, -1.0))
        fam.append((f"torus {what} eye", np.broadcast_to(EYE, pts.shape).copy(), _unit(pts - EYE)))
    # the box's own coordinates: rays in face planes, along edges, through corners
    mid = 0.5 * (BOX_LO + BOX_HI)
    o_l, d_l = [], []
    for axis in range(3):
        u, w = (axis + 1) % 3, (axis + 2) % 3
        vals = lambda k: (BOX_LO[k] - 0.1, BOX_LO[k], mid[k], BOX_HI[k], BOX_HI[k] + 0.1)
        p = np.zeros((25, 3))
        p[:, u], p[:, w] = [x.ravel() for x in np.meshgrid(vals(u), vals(w), indexing="ij")]
        for sense in (1.0, -1.0):
            o, d = _axis_rays(p, axis, sense)
            o_l.append(o)
            d_l.append(d)
    fam.append(("box planes", np.concatenate(o_l), np.concatenate(d_l)))
    eye = np.array([-4.0, 2.0, 3.0])
    pts = _box_edge_points(BOX_LO, BOX_HI, 21)
    fam.append(("box edges", np.broadcast_to(eye, pts.shape).copy(), _unit(pts - eye)))
    eye = np.array([0.3, 0.2, -0.4])
    pts = _box_edge_points(np.full(3, LO), np.full(3, HI), 21)
    fam.append(("room edges", np.broadcast_to(eye, pts.shape).copy(), _unit(pts - eye)))
    # sphere silhouette
    for factor in (0.99, 0.999, 1, 1.001, 1.01):
        fam.append((f"cone {factor} x",) + _silhouette(factor, 180))
    # origins on surfaces
    from tests.util import random_rays
    o, d = random_rays(rng, 3000, np.zeros(3), 4.5)
    t, obj, nrm = osc.intersect(o, d, robust=cfg["robust"])
    hit = obj >= 0
    p = (o[hit] + t[hit, None] * d[hit]).astype(cfg["dtype"]).astype(np.float64)
    fresh = _unit(rng.normal(size=p.shape))
    steep = np.abs((fresh * nrm[hit]).sum(axis=1)) >= 0.2
    fam.append(("surface steep", p[steep], fresh[steep]))
    fam.append(("surface shallow", p[~steep], fresh[~steep]))
    # control
    fam.append(("random",) + random_rays(rng, 3000, np.zeros(3), 4.5))
    # just in front of a surface: the hit lies at 0.3, 2, 4 and 8 times the mode's t_min (the self-hit decision), incidence above 60 degrees
    # (not at 1 x: there the library may hit anywhere from t_min on, and no finite sample of hits reaches down to t_min itself)
    rng = np.random.default_rng(20262)
    o, d = random_rays(rng, 500, np.zeros(3), 4.5)
    t, obj, nrm = osc.intersect(o, d, robust=cfg["robust"])
    hit = (obj >= 0) & (np.abs((d * nrm).sum(axis=1)) >= 0.5)
    p = o[hit] + t[hit, None] * d[hit]
    t_min = 2e-5 * (1.0 + np.abs(p).max(axis=1, keepdims=True)) if mode == "fp32" else 1e-12
    for k in (0.3, 2, 4, 8):
        fam.append((f"near surface {k} x", p - k * t_min * d[hit], d[hit]))
    return [(name, _round(o, cfg), _round(d, cfg)) for name, o, d in fam]


def _round(a, cfg):
    return np.ascontiguousarray(a, dtype=np.float64).astype(cfg["dtype"]).astype(np.float64)


def join(fam):
    """-> origins, directions, family index per ray, family names."""
    return (np.concatenate([f[1] for f in fam]), np.concatenate([f[2] for f in fam]),
            np.concatenate([np.full(len(f[1]), i) for i, f in enumerate(fam)]), [f[0] for f in fam])


# ------------------------------------------------------------------ the cloud
class Cloud:
    """The oracle's answers around n rays.  obj, t, nrm: (n, 17) [, 3], column 0 the ray itself; for the rows `again` (those whose 17
    answers name different objects) obj2, t2, nrm2: (m, 173) [, 3], the 17, the second pass and the third.  decided: (n,) bool."""

    def __init__(self, mode, o, d, obj, t, nrm, again, obj2, t2, nrm2):
        self.mode, self.o, self.d = mode, o, d
        self.obj, self.t, self.nrm = obj, t, nrm
        self.again, self.obj2, self.t2, self.nrm2 = again, obj2, t2, nrm2
        cfg = MODES[mode]
        same = (obj == obj[:, :1]).all(axis=1)
        miss = obj[:, 0] < 0
        with np.errstate(invalid="ignore"):
            t_ok = t.max(axis=1) <= t.min(axis=1) * (1.0 + cfg["b_t"])
            n_ok = (nrm.max(axis=1) - nrm.min(axis=1)).max(axis=1) <= cfg["b_n"]
        self.decided = same & (miss | (t_ok & n_ok))

    def __len__(self):
        return len(self.o)

    def answers(self, i):
        """(obj, t, nrm) of ray i's whole cloud."""
        k = np.flatnonzero(self.again == i)
        if len(k):
            return self.obj2[k[0]], self.t2[k[0]], self.nrm2[k[0]]
        return self.obj[i], self.t[i], self.nrm[i]


def _ask(osc, o, d, robust):
    """o, d: (n, k, 3) -> obj (n, k), t (n, k), nrm (n, k, 3)."""
    n, k = o.shape[:2]
    t, obj, nrm = osc.intersect(o.reshape(-1, 3), d.reshape(-1, 3), robust=robust)
    return obj.reshape(n, k), t.reshape(n, k), nrm.reshape(n, k, 3)


def cloud(osc, o, d, mode, amp=None, seed=7):
    """The answers of OracleScene `osc` in the neighbourhood of every ray (o, d) -> Cloud."""
    cfg = MODES[mode]
    amp = cfg["amp"] if amp is None else amp
    o, d = _round(np.reshape(o, (-1, 3)), cfg), _round(np.reshape(d, (-1, 3)), cfg)
    rng = np.random.default_rng(seed)
    a = (amp * (1.0 + np.abs(o).max(axis=1)))[:, None, None]
    n = len(o)

    def shaken(oo, dd, aa, k):
        po = oo[:, None, :] + aa * rng.uniform(-1.0, 1.0, (len(oo), k, 3))
        pd = dd[:, None, :] + amp * rng.uniform(-1.0, 1.0, (len(oo), k, 3))
        return po, pd

    po, pd = shaken(o, d, a, N_FIRST)
    obj, t, nrm = _ask(osc, np.concatenate([o[:, None, :], po], axis=1), np.concatenate([d[:, None, :], pd], axis=1), cfg["robust"])
    again = np.flatnonzero((obj != obj[:, :1]).any(axis=1))
    m = len(again)
    offs = np.array([c for c in itertools.product((-1.0, 0.0, 1.0), repeat=3) if any(c)])           # (26, 3)
    o2, d2, a2 = o[again], d[again], a[again]
    so, sd = shaken(o2, d2, a2, N_MORE)
    qo = np.concatenate([o2[:, None, :] + a2 * offs[None], np.repeat(o2[:, None, :], 26, axis=1), so], axis=1)
    qd = np.concatenate([np.repeat(d2[:, None, :], 26, axis=1), d2[:, None, :] + amp * offs[None], sd], axis=1)
    if m:
        obj2, t2, nrm2 = _ask(osc, qo, qd, cfg["robust"])
    else:
        obj2, t2, nrm2 = np.zeros((0, 84), np.int32), np.zeros((0, 84)), np.zeros((0, 84, 3))
    obj2, t2, nrm2 = np.concatenate([obj[again], obj2], axis=1), np.concatenate([t[again], t2], axis=1), np.concatenate([nrm[again], nrm2], axis=1)
    if m:
        qo, qd = np.concatenate([o2[:, None, :], po[again], qo], axis=1), np.concatenate([d2[:, None, :], pd[again], qd], axis=1)
        obj2, t2, nrm2 = _edge_of_the_answers(osc, cfg["robust"], qo, qd, obj2, t2, nrm2)
    return Cloud(mode, o, d, obj, t, nrm, again, obj2, t2, nrm2)


N_OBJECTS_BISECTED, N_BISECTIONS = 3, 12


def _edge_of_the_answers(osc, robust, qo, qd, obj, t, nrm):
    """Third pass, for the rays of the second: where an object's hits end inside the neighbourhood (a silhouette, the self-hit threshold),
    t runs up to that edge like a square root, and a hundred samples stop a few b_t short of it.  For each of the ray's first three hit
    objects, from the sample with its largest t and from the one with its smallest, bisect 12 times towards a sample with another answer
    (a point between two samples lies in the neighbourhood as well) and keep every answer with that object met on the way."""
    m, k = obj.shape
    rows = np.arange(m)
    add_obj, add_t, add_n = [], [], []
    for slot in range(N_OBJECTS_BISECTED):
        want = np.full(m, -2)
        for r in range(m):
            u = np.unique(obj[r][obj[r] >= 0])
            if len(u) > slot:
                want[r] = u[slot]
        mine = obj == want[:, None]
        other = np.argmax(~mine, axis=1)                                   # (the rows of the second pass have one)
        for pick in (np.argmax(np.where(mine, t, -np.inf), axis=1), np.argmin(np.where(mine, t, np.inf), axis=1)):
            lo_o, lo_d, hi_o, hi_d = qo[rows, pick], qd[rows, pick], qo[rows, other], qd[rows, other]
            keep = (obj[rows, pick].copy(), t[rows, pick].copy(), nrm[rows, pick].copy())
            for _ in range(N_BISECTIONS):
                mo, md = 0.5 * (lo_o + hi_o), 0.5 * (lo_d + hi_d)
                t1, o1, n1 = osc.intersect(mo, md, robust=robust)
                same = (o1 == want) & (want >= 0)
                lo_o, lo_d = np.where(same[:, None], mo, lo_o), np.where(same[:, None], md, lo_d)
                hi_o, hi_d = np.where(same[:, None], hi_o, mo), np.where(same[:, None], hi_d, md)
                keep = (np.where(same, o1, keep[0]), np.where(same, t1, keep[1]), np.where(same[:, None], n1, keep[2]))
                add_obj.append(keep[0].copy())
                add_t.append(keep[1].copy())
                add_n.append(keep[2].copy())
    return (np.concatenate([obj, np.stack(add_obj, axis=1)], axis=1), np.concatenate([t, np.stack(add_t, axis=1)], axis=1),
            np.concatenate([nrm, np.stack(add_n, axis=1)], axis=1))


# ------------------------------------------------------------------ the rule
class Report:
    """failed: (n,) bool; t_err: relative distance of t from the cloud's t range of that object, n_err: max-norm distance to the nearest
    of its normals (both NaN where the object is not in the cloud or the answer is a miss)."""

    def __init__(self, failed, t_err, n_err):
        self.failed, self.t_err, self.n_err = failed, t_err, n_err


def _rule(co, ct, cn, obj, t, nrm, cfg):
    match = co == obj[:, None]
    known = match.any(axis=1)
    hit = obj >= 0
    with np.errstate(invalid="ignore", over="ignore"):
        tlo, thi = np.where(match, ct, np.inf).min(axis=1), np.where(match, ct, -np.inf).max(axis=1)
        t_err = np.maximum(np.maximum((tlo - t) / tlo, (t - thi) / thi), 0.0)
        t_ok = (t >= tlo * (1.0 - cfg["b_t"])) & (t <= thi * (1.0 + cfg["b_t"]))
        if nrm is None:
            n_err = np.zeros(len(t))
        else:
            n_err = np.where(match, np.abs(cn - nrm[:, None, :]).max(axis=2), np.inf).min(axis=1)
        n_ok = n_err <= cfg["b_n"]
    nan = np.isnan(t) if nrm is None else np.isnan(t) | np.isnan(nrm).any(axis=1)
    ok = known & ~nan & np.where(hit, t_ok & n_ok, np.isposinf(t))
    shown = hit & known
    return ~ok, np.where(shown, t_err, np.nan), np.where(shown, n_err, np.nan)


def check(cl, obj, t, nrm, mode, family=None, names=None, layout="", show=8):
    """The rule, for every ray of Cloud `cl`: the answer (obj, t, nrm) of the library must be one the cloud contains -> Report.
      * obj is an object of the cloud (a miss, -1, counts as one);
      * a hit: min t_k (1 - b_t) <= t <= max t_k (1 + b_t) over the cloud's answers k with that object, and the normal within b_n
        (max-norm) of one of theirs;
      * a miss: t = +inf;
      * nothing is NaN.
    nrm = None (a query that returns no normal) leaves the normals out.
    Failing rays are printed (the first `show`) with the library's answer, their cloud, their family and `layout`."""
    assert mode == cl.mode
    cfg = MODES[mode]
    obj = np.asarray(obj).astype(np.int64).reshape(-1)
    t = np.asarray(t, dtype=np.float64).reshape(-1)
    nrm = None if nrm is None else np.asarray(nrm, dtype=np.float64).reshape(-1, 3)
    assert len(obj) == len(t) == len(cl) and (nrm is None or len(nrm) == len(cl))
    failed, t_err, n_err = _rule(cl.obj, cl.t, cl.nrm, obj, t, nrm, cfg)
    k = cl.again
    if len(k):
        failed[k], t_err[k], n_err[k] = _rule(cl.obj2, cl.t2, cl.nrm2, obj[k], t[k], None if nrm is None else nrm[k], cfg)
    bad = np.flatnonzero(failed)
    if len(bad):
        print(f"{len(bad)} of {len(cl)} rays fail the {mode} rule; layout: {layout}")
    for i in bad[:show]:
        co, ct, cn = cl.answers(i)
        fam = names[family[i]] if family is not None and names is not None else "?"
        print(f"  ray {i} [{fam}] {'decided' if cl.decided[i] else 'undecided'}: o = {cl.o[i].tolist()!r} d = {cl.d[i].tolist()!r}")
        print(f"    library: obj {obj[i]} t {t[i]!r} n {None if nrm is None else nrm[i].tolist()!r}")
        for ob in np.unique(co):
            sel = co == ob
            if ob < 0:
                print(f"    cloud: miss x {int(sel.sum())}")
            else:
                j = np.flatnonzero(sel)[0]
                print(f"    cloud: obj {ob} x {int(sel.sum())}, t in [{ct[sel].min()!r}, {ct[sel].max()!r}], n e.g. {cn[j].tolist()!r}")
    return Report(failed, t_err, n_err)


def table(cl, family, names, report=None, groups=None):
    """One line per family (or per group of families: name prefixes): rays, decided, failures, worst t and normal error."""
    rows = []
    keys = groups if groups is not None else names
    for key in keys:
        sel = np.array([nm.startswith(key) for nm in names])[family] if groups is not None else family == names.index(key)
        row = {"family": key.strip(), "rays": int(sel.sum()), "decided": int(cl.decided[sel].sum())}
        if report is not None:
            with np.errstate(invalid="ignore"):
                te, ne = report.t_err[sel], report.n_err[sel]
                row.update(failures=int(report.failed[sel].sum()), t_err=float(np.nanmax(te)) if np.isfinite(te).any() else 0.0,
                           n_err=float(np.nanmax(ne)) if np.isfinite(ne).any() else 0.0)
        rows.append(row)
    return rows


def print_table(title, rows):
    print(title)
    for r in rows:
        line = f"  {r['family']:<22} rays {r['rays']:>6} decided {r['decided']:>6} ({100.0 * r['decided'] / max(r['rays'], 1):5.1f} %)"
        if "failures" in r:
            line += f"  failures {r['failures']:>4}  worst t err {r['t_err']:.2e}  worst n err {r['n_err']:.2e}"
        print(line)


# ------------------------------------------------------------------ shared between the test modules
VARIANTS = {"base": {}, "lattice": {"lattice": True}, "instances": {"lattice": True, "second_use": True}, "scan": {"torus": (4, 4)}}
_prepared = {}


def prepared(mode, variant="base"):
    """The rays (always those of the base scene, so that they are the same for every variant) and their cloud in scene(**VARIANTS[variant]),
    computed once per process -> dict of scene_args, o, d, family, names, cloud."""
    key = (mode, variant)
    if key not in _prepared:
        if variant == "base":
            osc = oracle_scene(scene())
            o, d, family, names = join(families(mode, osc))
        else:
            base = prepared(mode, "base")
            osc = oracle_scene(scene(**VARIANTS[variant]))
            o, d, family, names = base["o"], base["d"], base["family"], base["names"]
        _prepared[key] = {"scene_args": VARIANTS[variant], "o": o, "d": d, "family": family, "names": names, "cloud": cloud(osc, o, d, mode)}
    return _prepared[key]
