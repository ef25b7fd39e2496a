"""MonomialSurface (src/shape/monomial_surface.rs) on the device, in both render modes: closest hits against the fp64 restatement
in tests/monomial_ref.py (and the oracle for the other shapes), the white furnace, placement in the scan / the scene tree /
KdTree groups, small renders of examples/monomial_glass.rs, and what the library refuses."""
import math

import numpy as np
import pytest

from rpt_amd import (Camera, KdTree, Light, Material, Mesh, Object, Renderer, RptError, Scene, cube, monomial_surface, plane,
                     scenes, sphere, vec3)
from rpt_amd import _lib
from tests.monomial_ref import closest_hit as ref_closest_hit
from tests.monomial_ref import intersect_world
from tests.test_oracle_kat import furnace_scene
from tests.util import random_rays, rel_rms

pytestmark = pytest.mark.gpu

DIFF = Material.diffuse(vec3(0.7, 0.7, 0.7))


def _ray_tmin(o):   # kernels.hip ray_tmin: the fp32 policy's t_min
    return 2e-5 * (1.0 + np.max(np.abs(o), axis=1))


def _mono_shapes():
    """(shape, height, 4x4 matrix) of surfaces translated, non-uniformly scaled and rotated."""
    out = []
    s = monomial_surface(2.0, 4.0).translate(vec3(0.0, -1.0, 0.0))
    out.append((s, 2.0, s.matrix()))
    s = monomial_surface(0.7, 4.0).scale(vec3(0.8, 1.5, 0.6)).translate(vec3(2.3, 0.2, -0.5))
    out.append((s, 0.7, s.matrix()))
    s = monomial_surface(-1.2, 4.0).rotate_x(0.6).rotate_y(0.4).translate(vec3(-2.2, 0.5, 0.3))
    out.append((s, -1.2, s.matrix()))
    return out


def _others():
    tris = Mesh.__new__(Mesh)
    v = np.array([[0.0, 2.5, -2.0], [1.5, 3.5, -2.0], [-1.0, 3.8, -1.0]])
    n = np.cross(v[1] - v[0], v[2] - v[0])
    n /= np.linalg.norm(n)
    tris.tris = np.array([[v[0], v[1], v[2], n, n, n]])
    return [sphere().scale(vec3(0.6, 0.6, 0.6)).translate(vec3(0.0, 0.4, 2.2)), plane(vec3(0.0, 1.0, 0.0), -2.5), tris]


ADV_SETS = ["down", "up", "near-vertical", "rim", "on-surface"]   # _adversarial_rays' blocks, in order
ADV_K = 400


def _adversarial_rays(rng):
    o, d = [], []
    k = ADV_K
    xz = rng.uniform(-1.2, 1.2, size=(k, 2))
    for sgn in (-1.0, 1.0):      # axis-parallel vertical rays over the first surface (local (x, z) = world (x, z))
        o.append(np.stack([xz[:, 0], np.full(k, 3.0 if sgn < 0 else -3.0), xz[:, 1]], axis=1))
        d.append(np.tile([0.0, sgn, 0.0], (k, 1)))
    tilt = rng.normal(size=(k, 3)) * 1e-3   # near-vertical
    dd = np.array([0.0, -1.0, 0.0]) + tilt
    o.append(np.stack([xz[:, 0], np.full(k, 3.0), xz[:, 1]], axis=1))
    d.append(dd / np.linalg.norm(dd, axis=1, keepdims=True))
    ang = rng.uniform(0, 2 * math.pi, k)   # horizontal rays grazing the rim (radius 1, height h = 2, at y = 1 - 1e-3 .. 1)
    y = 1.0 - rng.uniform(0, 1e-3, k)
    o.append(np.stack([np.cos(ang) - 3 * np.sin(ang), y, np.sin(ang) + 3 * np.cos(ang)], axis=1))
    d.append(np.stack([np.sin(ang), np.zeros(k), -np.cos(ang)], axis=1))
    r = np.sqrt(rng.uniform(0, 1, k))      # origins on the surface, random directions
    ph = rng.uniform(0, 2 * math.pi, k)
    px, pz = r * np.cos(ph), r * np.sin(ph)
    o.append(np.stack([px, 2.0 * (px * px + pz * pz) ** 2 - 1.0, pz], axis=1))
    dd = rng.normal(size=(k, 3))
    d.append(dd / np.linalg.norm(dd, axis=1, keepdims=True))
    return np.concatenate(o), np.concatenate(d)


def _scene(shapes, eps=False):
    sc = Scene()
    for s in shapes:
        sc.add(Object(s).material(DIFF))
    sc.add(Light.Ambient(vec3(0.1, 0.1, 0.1)))
    if eps:
        sc.set_option("epsilon_policy", 1)
    return sc


# ------------------------------------------------------------------ 1. fp32 closest hit
def test_fp32_closest_hit_matches_the_restatement_and_the_oracle():
    from oracle.pyoracle import OracleScene
    monos = _mono_shapes()
    others = _others()
    full = _scene([m[0] for m in monos] + others)
    rng = np.random.default_rng(7)
    o1, d1 = random_rays(rng, 20000, np.array([0.0, 0.5, 0.0]), 5.0)
    o2, d2 = _adversarial_rays(rng)
    o = np.concatenate([o1, o2]).astype(np.float32)
    d = np.concatenate([d1, d2]).astype(np.float32)
    t, obj, nrm = Renderer(full, Camera()).get_closest_hit(o, d)
    o64, d64 = o.astype(np.float64), d.astype(np.float64)
    # expected: the closest of the monomial surfaces (restatement, the fp32 policy's t_min, NaN = miss) and of the rest (oracle)
    te = np.full(len(o), np.inf)
    obje = np.full(len(o), -1)
    nrme = np.zeros((len(o), 3))
    tmin = _ray_tmin(o64)
    for k, (_, h, m) in enumerate(monos):
        ok, tk, nk = _with_tmin(o64, d64, h, m, tmin)
        ok &= np.isfinite(tk)
        better = ok & (tk < te)
        te, obje, nrme = np.where(better, tk, te), np.where(better, k, obje), np.where(better[:, None], nk, nrme)
    tr, objr, nrmr = OracleScene(_scene(others)).intersect(o, d, robust=1)
    better = (objr >= 0) & (tr < te)
    te, obje, nrme = np.where(better, tr, te), np.where(better, objr + len(monos), obje), np.where(better[:, None], nrmr, nrme)
    same = obj == obje
    both = (obj >= 0) & (obje >= 0)
    with np.errstate(invalid="ignore"):
        coincident = both & ~same & (np.abs(t - te) <= 2e-4 * np.abs(te))
    frac = (same | coincident).mean()
    labels = np.array(["random"] * len(o1) + [n for n in ADV_SETS for _ in range(ADV_K)])
    hit = same & (obje >= 0)
    rel_t = np.full(len(o), 0.0)
    nerr = np.full(len(o), 0.0)
    rel_t[hit] = np.abs(t[hit] - te[hit]) / te[hit]
    nerr[hit] = np.max(np.abs(nrm[hit] - nrme[hit]), axis=1)
    abs_t = np.zeros(len(o))
    abs_t[hit] = np.abs(t[hit] - te[hit])
    print(f"fp32 closest hit: same object {frac:.5f}; monomial hits {(hit & (obje < len(monos))).sum()}")
    for name in ["random"] + ADV_SETS:
        sel = labels == name
        w = np.argmax(np.where(sel, rel_t, -1.0))
        print(f"  {name:14s} same {(same | coincident)[sel].mean():.5f}  max rel t {rel_t[sel].max():.3e}  max abs t "
              f"{abs_t[sel].max():.3e}  max normal {nerr[sel].max():.3e}  worst: o {o[w]} d {d[w]} t {t[w]:.6e} expected "
              f"{te[w]:.6e} obj {obj[w]}")
    assert frac >= 0.9995
    assert (hit & (obje < len(monos))).sum() > 2000
    assert nerr.max() < 2e-3
    # Time: the issue's 2e-4 relative bound holds for every ray except those that start ON a surface.  Those leave it at small t
    # (measured down to ~4e-3), where the root lies on a shallow stretch of dist(t): fp32's rounding of dist (~1e-7 of values of
    # order 1) moves the root by ~1e-6 in absolute terms -- 8.3e-4 of t for the worst one (t = 4.66e-3, off by 3.9e-6).  They are
    # bounded in absolute terms instead, by the fp32 policy's own t_min scale (ray_tmin: 2e-5 (1 + |o|)).
    on = labels == "on-surface"
    assert rel_t[~on].max() < 2e-4
    assert np.all((rel_t[on] < 2e-4) | (abs_t[on] < _ray_tmin(o64[on])))
    assert np.all(np.isinf(t[same & (obje < 0)]))


def _with_tmin(o, d, h, m, tmin):
    """intersect_world with a per-ray t_min (the restatement takes a scalar): rays grouped by their t_min value."""
    ok = np.zeros(len(o), dtype=bool)
    t = np.full(len(o), np.inf)
    n = np.zeros((len(o), 3))
    for v in np.unique(tmin):
        sel = tmin == v
        a, b, c = intersect_world(o[sel], d[sel], h, float(v), m)
        ok[sel], t[sel], n[sel] = a, b, c
    return ok, t, n


# ------------------------------------------------------------------ 2. fp64 closest hit, bit for bit
def _same_bits(a, b):
    """Equal bit for bit, a NaN matching any NaN (its payload is not part of the reference's result)."""
    na, nb = np.isnan(a), np.isnan(b)
    u = np.uint32 if a.dtype == np.float32 else np.uint64
    return np.array_equal(na, nb) and np.array_equal(a[~na].view(u), b[~nb].view(u))


def _exact_surfaces():
    """Bare, translated and power-of-two-scaled surfaces: M^-1 is exact, so the restatement sees the library's local rays."""
    return [(monomial_surface(2.0, 4.0), 2.0, None),
            (monomial_surface(0.5, 4.0).translate(vec3(2.25, -0.5, 0.75)), 0.5, None),
            (monomial_surface(-1.5, 4.0).scale(vec3(2.0, 0.5, 4.0)).translate(vec3(-3.0, 1.0, -0.5)), -1.5, None)]


def test_fp64_closest_hit_is_the_restatement_bit_for_bit():
    surf = _exact_surfaces()
    mats = [(h, s.matrix()) for s, h, _ in surf]
    sc = _scene([s for s, _, _ in surf], eps=True)
    rng = np.random.default_rng(11)
    o1, d1 = random_rays(rng, 20000, np.array([0.0, 0.5, 0.0]), 5.0)
    o2, d2 = _adversarial_rays(rng)
    nan_o, nan_d = np.array([[0.9, -1.0, 0.1], [0.5, 3.0, 0.3]]), np.array([[0.0, 1.0, 0.0], [0.0, -1.0, 0.0]])
    o = np.concatenate([o1, o2, nan_o])
    d = np.concatenate([d1, d2, nan_d])
    t, obj, nrm = Renderer(sc, Camera()).get_closest_hit_f64(o, d)
    te, obje, nrme = ref_closest_hit(o, d, mats)
    assert np.array_equal(obj, obje)
    assert _same_bits(t, te)
    hit = obj >= 0
    assert _same_bits(nrm[hit], nrme[hit])
    assert obj[-2] == 0 and np.isnan(t[-2])             # the reference's NaN hit (deriv2 = -0: Newton steps to infinity)
    assert obj[-1] == 0 and abs(t[-1] - 2.7688) < 1e-12  # the vertical hit at x = 0.5, z = 0.3
    assert hit.sum() > 3000 and np.isnan(t[hit]).sum() >= 1


def test_fp64_objects_inside_and_in_front_of_the_surface():
    """Spheres added BEFORE a monomial surface, inside its box and in front of it (marbles in a glass): the surface's own hit
    behind the record must not replace it (`r > record.time`, monomial_surface.rs:85) -- also when other lanes of the wave see
    the surface first --, and a sphere added after it competes as usual.  Bit for bit against the restatement."""
    inner = sphere().scale(vec3(0.25, 0.25, 0.25)).translate(vec3(0.0, 0.5, 0.0))
    small = sphere().scale(vec3(0.125, 0.125, 0.125)).translate(vec3(0.5, 0.25, -0.25))
    above = sphere().scale(vec3(0.5, 0.5, 0.5)).translate(vec3(-0.5, 3.0, 0.5))
    glass = monomial_surface(2.0, 4.0)
    after = sphere().scale(vec3(0.25, 0.25, 0.25)).translate(vec3(-0.25, 1.0, 0.25))
    shapes = [inner, small, above, glass, after]
    spec = [("sphere", inner.matrix()), ("sphere", small.matrix()), ("sphere", above.matrix()), (2.0, None), ("sphere", after.matrix())]
    sc = _scene(shapes, eps=True)
    rng = np.random.default_rng(13)
    k = 8192
    xz = rng.uniform(-1.1, 1.1, size=(k, 2))
    o1 = np.stack([xz[:, 0], np.full(k, 4.0), xz[:, 1]], axis=1)        # straight down into the glass
    d1 = np.tile([0.0, -1.0, 0.0], (k, 1))
    o2, d2 = random_rays(rng, k, np.array([0.0, 1.0, 0.0]), 4.0)
    o = np.concatenate([[[0.0, 1.5, 0.0]], o1, o2])
    d = np.concatenate([[[0.0, -1.0, 0.0]], d1, d2])
    t, obj, nrm = Renderer(sc, Camera()).get_closest_hit_f64(o, d)
    te, obje, nrme = ref_closest_hit(o, d, spec)
    assert obj[0] == 0 and t[0] == 0.75   # the sphere, not the surface below it at t = 1.5
    assert np.array_equal(obj, obje)
    assert _same_bits(t, te)
    hit = obj >= 0
    assert _same_bits(nrm[hit], nrme[hit])
    # the case at stake: a sphere earlier in scene order holds the record and the surface's own hit lies behind it
    ok_g, t_g, _ = intersect_world(o, d, 2.0, 1e-12)
    behind = (obj >= 0) & (obj < 3) & ok_g & (t_g > t)
    assert behind.sum() > 500


def test_fp64_closest_hit_with_rotations_within_1e12():
    surf = _mono_shapes()
    sc = _scene([s for s, _, _ in surf], eps=True)
    rng = np.random.default_rng(12)
    o, d = random_rays(rng, 20000, np.array([0.0, 0.5, 0.0]), 5.0)
    t, obj, nrm = Renderer(sc, Camera()).get_closest_hit_f64(o, d)
    te, obje, nrme = ref_closest_hit(o, d, [(h, m) for _, h, m in surf])
    same = obj == obje
    assert same.mean() > 0.9995
    hit = same & (obj >= 0) & np.isfinite(te)
    assert hit.sum() > 2000
    assert np.max(np.abs(t[hit] - te[hit]) / np.abs(te[hit])) < 1e-12
    assert np.max(np.abs(nrm[hit] - nrme[hit])) < 1e-9


def test_fp64_entry_point_needs_the_mode():
    sc = _scene([monomial_surface(2.0, 4.0)])
    r = Renderer(sc, Camera())
    with pytest.raises(RptError) as e:
        r.get_closest_hit_f64(np.zeros((1, 3)), np.array([[0.0, 1.0, 0.0]]))
    assert "epsilon_policy" in str(e.value)
    lib = _lib.load()
    buf = np.zeros(8)
    rc = lib.rpt_intersect_batch_f64(sc._handle, 1, buf.ctypes.data, buf.ctypes.data, buf.ctypes.data, buf.ctypes.data,
                                     None)
    assert rc == -2   # RPT_ERR_STATE


# ------------------------------------------------------------------ 3. white furnace
@pytest.mark.parametrize("eps", [False, True])
@pytest.mark.parametrize("bounces", [0, 3])
def test_white_furnace_with_monomial_surfaces(eps, bounces):
    rho, c = 0.6, 0.25
    scene, cam = furnace_scene(rho, c)
    m = Material.diffuse(vec3(rho, rho, rho))
    scene.add(Object(monomial_surface(2.0, 4.0).scale(vec3(3.0, 1.0, 3.0)).translate(vec3(0.0, -4.0, -5.0))).material(m))
    scene.add(Object(monomial_surface(-1.0, 4.0).rotate_z(0.7).scale(vec3(2.0, 2.0, 2.0)).translate(vec3(3.0, 2.0, -4.0))).material(m))
    scene.add(Object(KdTree([monomial_surface(1.0, 4.0).translate(vec3(-4.0, 0.0, -6.0)), sphere().translate(vec3(-5.0, 3.0, -7.0))]))
              .material(m))
    if eps:
        scene.set_option("epsilon_policy", 1)
    img = Renderer(scene, cam).width(24).height(24).max_bounces(bounces).seed(4).sample_array(8)
    expect = c * rho * sum(rho ** k for k in range(bounces + 1))
    assert np.allclose(img, expect, rtol=2e-5)


# ------------------------------------------------------------------ 4. placement: scan, scene tree, nested groups
def _placement_scenes(eps):
    base = [monomial_surface(2.0, 4.0).translate(vec3(0.0, -1.0, 0.0)),
            monomial_surface(-0.75, 4.0).scale(vec3(0.5, 1.0, 0.5)).translate(vec3(2.5, 0.5, 0.0))]
    scan = _scene(base, eps)
    far = [sphere().scale(vec3(0.1, 0.1, 0.1)).translate(vec3(50.0 + i, 50.0, 50.0)) for i in range(70)]
    tree = _scene(base + far, eps)
    grouped = _scene([KdTree([KdTree([monomial_surface(2.0, 4.0).translate(vec3(0.0, -0.25, 0.0))]).translate(vec3(0.0, -0.5, 0.0)),
                              sphere().translate(vec3(40.0, 0.0, 0.0))]).translate(vec3(0.0, -0.25, 0.0)),
                      base[1]], eps)
    return scan, tree, grouped


@pytest.mark.parametrize("eps", [False, True])
def test_same_hits_in_the_scan_the_scene_tree_and_groups(eps):
    scan, tree, grouped = _placement_scenes(eps)
    rng = np.random.default_rng(5)
    o, d = random_rays(rng, 20000, np.array([1.0, 0.0, 0.0]), 4.0)
    q = (lambda r: r.get_closest_hit_f64(o, d)) if eps else (lambda r: r.get_closest_hit(o, d))
    ts, objs, ns = q(Renderer(scan, Camera()))
    rt = Renderer(tree, Camera())
    tt, objt, nt = q(rt)
    if not eps:
        assert rt.scene_stats()["scene_bvh"] == 1
    assert np.array_equal(objs, objt)
    assert _same_bits(ts, tt)   # the same arithmetic on the same records
    hit = objs >= 0
    assert hit.sum() > 3000
    assert _same_bits(ns[hit], nt[hit])
    tg, objg, ng = q(Renderer(grouped, Camera()))
    agree = (objs == objg) & hit
    assert (objs != objg).mean() < 1e-3
    tol = 1e-12 if eps else 2e-6   # (the groups' translations are applied one level at a time)
    fin = agree & np.isfinite(ts)
    assert np.max(np.abs(tg[fin] - ts[fin]) / ts[fin]) < tol
    assert np.max(np.abs(ng[fin] - ns[fin])) < (1e-9 if eps else 1e-4)


# ------------------------------------------------------------------ 5. renders of examples/monomial_glass.rs
def _glass(eps, w=96, h=72):
    scene, cam, cfg = scenes.monomial_glass()
    if eps:
        scene.set_option("epsilon_policy", 1)
    return Renderer(scene, cam).width(w).height(h).max_bounces(cfg["max_bounces"]).seed(9)


@pytest.mark.parametrize("eps", [False, True])
def test_glass_render_is_deterministic_and_shards_add_up(eps):
    a = _glass(eps).sample_array(16)
    b = _glass(eps).sample_array(16)
    assert np.array_equal(a, b) and np.all(np.isfinite(a))
    parts = sum(_glass(eps).shard(k, 3).sample_array(16) for k in range(3))
    assert np.array_equal(parts, a)


def test_glass_means_of_the_two_modes_agree():
    a = _glass(False).sample_array(64)
    b = _glass(True).sample_array(64)
    ma, mb = a.mean(), np.nanmean(b)
    print(f"monomial_glass 96x72x64: fp32 mean {ma:.6f}, fp64 mode mean {mb:.6f}, rel {abs(ma - mb) / mb:.2e}, rel RMS {rel_rms(a, b):.3e}")
    assert abs(ma - mb) <= 0.01 * mb


def _tessellated_glass(height=2.0, nr=96, na=192):
    """The glass surface y = h (x^2 + z^2)^2 as a fine triangle mesh with the analytic normals at its vertices."""
    r = np.linspace(0.0, 1.0, nr + 1)
    a = np.linspace(0.0, 2 * math.pi, na + 1)
    R, A = np.meshgrid(r, a, indexing="ij")
    X, Z = R * np.cos(A), R * np.sin(A)
    Y = height * (X * X + Z * Z) ** 2
    N = np.stack([height * 4 * X * (X * X + Z * Z), -np.ones_like(X), height * 4 * Z * (X * X + Z * Z)], axis=-1)
    N /= np.linalg.norm(N, axis=-1, keepdims=True)
    P = np.stack([X, Y, Z], axis=-1)
    tris = []
    for i in range(nr):
        for j in range(na):
            p00, p10, p01, p11 = (i, j), (i + 1, j), (i, j + 1), (i + 1, j + 1)
            for q in ((p00, p10, p11), (p00, p11, p01)):
                v = [P[k] for k in q]
                if np.linalg.norm(np.cross(v[1] - v[0], v[2] - v[0])) < 1e-14:
                    continue
                tris.append(np.concatenate([np.array(v), np.array([N[k] for k in q])]))
    m = Mesh.__new__(Mesh)
    m.tris = np.array(tris)
    return m


@pytest.mark.parametrize("eps", [False, True])
def test_glass_matches_a_fine_tessellation(eps):
    scene, cam, cfg = scenes.monomial_glass()
    mesh_scene, _, _ = scenes.monomial_glass()
    mesh_scene.objects[0] = Object(_tessellated_glass().translate(vec3(0.0, -1.0, 0.0))).material(Material.metallic(vec3(1.0, 1.0, 1.0), 0.0001))
    for sc in (scene, mesh_scene):
        if eps:
            sc.set_option("epsilon_policy", 1)
    a = Renderer(scene, cam).width(96).height(72).max_bounces(1).seed(9).sample_array(64)
    b = Renderer(mesh_scene, cam).width(96).height(72).max_bounces(1).seed(9).sample_array(64)
    e = rel_rms(np.nan_to_num(a), np.nan_to_num(b))
    print(f"monomial_glass vs tessellation ({'fp64 mode' if eps else 'fp32'}): rel RMS {e:.3e}")
    assert e < 5e-3   # measured on MI355X: 1.35e-3 (fp32), 1.32e-3 (fp64 mode) -- the facets' silhouette and shading error


# ------------------------------------------------------------------ 6. refusals
def test_what_is_refused():
    m = Material.light(vec3(1.0, 1.0, 1.0), 2.0)
    for shape in (monomial_surface(1.0, 4.0), KdTree([sphere(), monomial_surface(1.0, 4.0).translate(vec3(3.0, 0.0, 0.0))])):
        sc = Scene()
        sc.add(Object(sphere()).material(DIFF))
        sc.add(Light.Object(Object(shape).material(m)))
        with pytest.raises(RptError) as e:
            Renderer(sc, Camera()).width(4).height(4).sample_array(1)
        assert "MonomialSurface" in str(e.value)
    sc = Scene()
    sc.add(Object(monomial_surface(2.0, 4.0)).material(DIFF))
    sc.add(Light.Object(Object(sphere().translate(vec3(0.0, 5.0, 0.0))).material(m)))
    r = Renderer(sc, Camera())
    with pytest.raises(RptError) as e:
        r.photon_map_build(1000, Renderer.PHOTON_MAP)
    assert "MonomialSurface" in str(e.value)
    with pytest.raises(RptError):
        r.photon_shoot(1000, Renderer.PHOTON_MAP)
    lib = _lib.load()
    assert lib.rpt_photon_map_build(sc._handle, 1000, 0, 100.0, 1) == -4
    assert lib.rpt_photon_shoot(sc._handle, 1000, 0, 100.0, 1, 0, 1, None) == -4
