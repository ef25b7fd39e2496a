"""Known-answer tests that pin the CPU oracle (oracle/rpt_oracle.cpp).

The reference's own test-suite holds ONE test on this path (src/color.rs:30-38, reproduced in
test_colors_work); every other expected value below was derived by hand from the cited lines
of the reference (SURVEY.md section 8c lists them as KAT 1-13).  No GPU needed."""
import ctypes as C
import math

import numpy as np
import pytest

from oracle import pyoracle
from oracle.pyoracle import CameraDesc, MaterialDesc, OracleScene, ShapeDesc
from rpt_amd import (Camera, Environment, KdTree, Light, Material, Medium, Mesh, Object, Scene, cube, hex_color, plane, polygon,
                     scenes, sphere, vec3)
from rpt_amd.api import camera_desc, material_desc, shape_desc


def D(*v):
    return (C.c_double * len(v))(*v)


def intersect(shape, o, d, t_min=1e-12, t_max=math.inf):
    L = pyoracle.lib()
    sd, _keep = shape_desc(shape, ShapeDesc)
    t, n = C.c_double(), D(0, 0, 0)
    hit = L.orc_shape_intersect(C.byref(sd), D(*o), D(*d), t_min, t_max, C.byref(t), n, 0)
    return bool(hit), t.value, np.array(list(n))


# ---- KAT 1: the reference's own test, src/color.rs:30-38
def test_colors_work():
    L = pyoracle.lib()
    for hexv, expect in [(0x000000, [0, 0, 0]), (0xFFFFFF, [255, 255, 255]), (0xFF0000, [255, 0, 0])]:
        rgb = D(0, 0, 0)
        L.orc_hex_color(hexv, rgb)
        out = (C.c_uint8 * 3)()
        L.orc_color_bytes(rgb, out)
        assert list(out) == expect


def test_color_bytes_truncates_and_gamma():
    # color.rs:18-24: (0.5^(1/2.2))*255 = 186.07 -> 186 (truncation, not rounding)
    L = pyoracle.lib()
    out = (C.c_uint8 * 3)()
    L.orc_color_bytes(D(0.5, 2.0, -1.0), out)
    assert list(out) == [186, 255, 0]
    rgb = D(0, 0, 0)
    L.orc_hex_color(0xD2B48C, rgb)
    assert np.allclose(list(rgb), [(0xD2 / 255) ** 2.2, (0xB4 / 255) ** 2.2, (0x8C / 255) ** 2.2], rtol=1e-15)


# ---- KAT 2-6: primitive intersections
def test_sphere_outside_and_inside():
    hit, t, n = intersect(sphere(), (0, 0, 5), (0, 0, -1))
    assert hit and t == 4.0 and np.array_equal(n, [0, 0, 1])
    hit, t, n = intersect(sphere(), (0, 0, 0), (0, 0, -1))
    assert hit and t == 1.0 and np.array_equal(n, [0, 0, -1])
    hit, _, _ = intersect(sphere(), (0, 2, 5), (0, 0, -1))
    assert not hit
    # non-unit direction: t scales inversely (sphere.rs:16-18 keeps `a = |d|^2`)
    hit, t, _ = intersect(sphere(), (0, 0, 5), (0, 0, -2))
    assert hit and t == 2.0


def test_cube_faces_and_tiebreak():
    hit, t, n = intersect(cube(), (0, 0, 5), (0, 0, -1))
    assert hit and t == 4.5 and np.array_equal(n, [0, 0, 1])
    hit, t, n = intersect(cube(), (0, 0, 0), (1, 0, 0))       # from inside: exit face
    assert hit and t == 0.5 and np.array_equal(n, [1, 0, 0])
    # corner ray: x1 == y1 == z1 -> neither `x1 > y1 && x1 > z1` nor `y1 > z1` -> z (cube.rs:40-48)
    hit, t, n = intersect(cube(), (-2, -2, -2), (1, 1, 1))
    assert hit and t == 1.5 and np.array_equal(n, [0, 0, -1])


def test_plane_normal_faces_the_ray():
    hit, t, n = intersect(plane(vec3(0, 0, 1), 0.0), (0, 0, 1), (0, 0, -1))
    assert hit and t == 1.0 and np.array_equal(n, [0, 0, 1])
    hit, t, n = intersect(plane(vec3(0, 0, 2), 0.0), (0, 0, -1), (0, 0, 1))   # plane.rs:27 flips and normalises
    assert hit and t == 1.0 and np.array_equal(n, [0, 0, -1])
    hit, _, _ = intersect(plane(vec3(0, 0, 1), 0.0), (0, 0, 1), (1, 0, 0))    # parallel (|cos| < 1e-8)
    assert not hit


def test_triangle_front_and_back_keep_the_normal():
    tri = polygon([vec3(0, 0, 0), vec3(1, 0, 0), vec3(0, 1, 0)])
    hit, t, n = intersect(tri, (0.25, 0.25, 1), (0, 0, -1))
    assert hit and t == 1.0 and np.array_equal(n, [0, 0, 1])
    hit, t, n = intersect(tri, (0.25, 0.25, -1), (0, 0, 1))     # mesh.rs:78: never face-forwarded
    assert hit and t == 1.0 and np.array_equal(n, [0, 0, 1])
    hit, _, _ = intersect(tri, (0.75, 0.75, 1), (0, 0, -1))     # outside: u < 0
    assert not hit


def test_transformed_preserves_t_and_maps_normals():
    s = sphere().scale(vec3(2, 2, 2)).translate(vec3(0, 0, -10))
    hit, t, n = intersect(s, (0, 0, 0), (0, 0, -1))
    assert hit and t == 8.0 and np.allclose(n, [0, 0, 1])
    # non-uniform scale: normal goes through M^-T (shape.rs:133)
    e = sphere().scale(vec3(1, 2, 1))
    o = np.array([3.0, 2.0 * math.sqrt(0.5), 0.0])
    hit, t, n = intersect(e, o, (-1, 0, 0))
    x = math.sqrt(0.5)
    expect = np.array([x, math.sqrt(0.5) / 2.0, 0.0])
    assert hit and abs(t - (3.0 - x)) < 1e-12 and np.allclose(n, expect / np.linalg.norm(expect))
    # chained calls left-multiply: cube().scale(s).rotate_y(a).translate(t) == T*R*S (shape.rs:237-284)
    c = cube().scale(vec3(2, 2, 2)).rotate_y(math.pi / 2).translate(vec3(5, 0, 0))
    hit, t, n = intersect(c, (0, 0, 0), (1, 0, 0))
    assert hit and abs(t - 4.0) < 1e-12 and np.allclose(n, [-1, 0, 0])


# ---- KAT 7: kd-tree == brute force
def test_kdtree_matches_brute_force():
    L = pyoracle.lib()
    tris = scenes.bumpy_torus(48, 48)                       # 4,608 triangles, smooth normals
    mesh = Mesh(tris)
    sd, keep = shape_desc(mesh, ShapeDesc)
    rng = np.random.default_rng(0)
    n = 4000
    o = rng.normal(size=(n, 3))
    o = 1.5 * o / np.linalg.norm(o, axis=1, keepdims=True)
    tgt = rng.uniform(-0.4, 0.4, size=(n, 3))
    d = tgt - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    o, d = np.ascontiguousarray(o), np.ascontiguousarray(d)
    t = np.zeros(n)
    bad = L.orc_mesh_kd_vs_brute(C.byref(sd), n, o.ctypes.data_as(C.c_void_p), d.ctypes.data_as(C.c_void_p),
                                 t.ctypes.data_as(C.c_void_p))
    assert bad == 0
    assert 0.2 < np.isfinite(t).mean() < 0.99


# ---- KAT 7b: KdTree<Box<dyn Bounded>> (kdtree.rs:103-227 over shapes) == the same shapes as separate objects
def test_shape_kdtree_matches_a_flat_scene_and_transforms_like_any_shape():
    rng = np.random.default_rng(1)
    kids = []
    for i in range(200):
        base = sphere() if i % 3 else cube()
        kids.append(base.scale(rng.uniform(0.05, 0.3, 3)).rotate_y(rng.uniform(0, 3)).translate(rng.uniform(-2, 2, 3)))
    kids.append(Mesh(scenes.bumpy_torus(8, 6)).translate(vec3(0.0, 0.5, 0.0)))
    white = Material.diffuse(vec3(1, 1, 1))
    grouped, flat = Scene(), Scene()
    grouped.add(Object(KdTree(kids).rotate_x(0.3).translate(vec3(0.1, 0.2, 0.3))).material(white))
    for k in kids:
        flat.add(Object(k.rotate_x(0.3).translate(vec3(0.1, 0.2, 0.3))).material(white))
    n = 20000
    o = rng.uniform(-3, 3, (n, 3))
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    tg, objg, ng = OracleScene(grouped).intersect(o, d)
    tf, objf, nf = OracleScene(flat).intersect(o, d)
    hit = np.isfinite(tf)
    assert 0.1 < hit.mean() < 0.9 and np.array_equal(hit, np.isfinite(tg))
    assert np.all(objg[hit] == 0)
    # the group composes its transform with each child's (Transformed<KdTree<Transformed<T>>>): two
    # inverse applications instead of one, so equal to rounding rather than to the bit
    assert np.max(np.abs(tg[hit] - tf[hit]) / tf[hit]) < 1e-9
    assert np.max(np.abs(ng[hit] - nf[hit])) < 1e-6
    # sampling a group picks a child uniformly and divides its pdf by the child count (kdtree.rs:141-146)
    L = pyoracle.lib()
    # (a uniformly scaled cube has a position-independent pdf, so the extra index draw does not matter)
    one, _k1 = shape_desc(cube().scale(vec3(0.5, 0.5, 0.5)), ShapeDesc)
    grp, _k2 = shape_desc(KdTree([cube().scale(vec3(0.5, 0.5, 0.5))] * 4), ShapeDesc)
    v1, n1, p1 = D(0, 0, 0), D(0, 0, 0), C.c_double()
    v4, n4, p4 = D(0, 0, 0), D(0, 0, 0), C.c_double()
    L.orc_shape_sample(C.byref(one), D(0, 3, 0), C.c_uint64(0), 3, 0, v1, n1, C.byref(p1))
    L.orc_shape_sample(C.byref(grp), D(0, 3, 0), C.c_uint64(0), 3, 0, v4, n4, C.byref(p4))
    assert p1.value > 0 and abs(p4.value - p1.value / 4.0) < 1e-15 * p1.value


# ---- KAT 8-9: materials
def bsdf(mat, n, wo, wi):
    out = D(0, 0, 0)
    pyoracle.lib().orc_material_bsdf(C.byref(material_desc(mat, MaterialDesc)), D(*n), D(*wo), D(*wi), out)
    return np.array(list(out))


def sample_f(mat, n, wo, seed, pixel):
    wi, pdf, draws = D(0, 0, 0), C.c_double(), C.c_int()
    some = pyoracle.lib().orc_material_sample_f(C.byref(material_desc(mat, MaterialDesc)), D(*n), D(*wo),
                                                C.c_uint64(seed), pixel, 0, wi, C.byref(pdf), C.byref(draws))
    return bool(some), np.array(list(wi)), pdf.value, draws.value


def test_bsdf_is_zero_below_the_surface():
    n = (0, 0, 1)
    up, down = (0.3, 0.1, 0.9), (0.3, 0.1, -0.9)
    for mat in [Material.diffuse(vec3(0.8, 0.5, 0.2)), Material.specular(vec3(0.8, 0.5, 0.2), 4.0), Material.mirror(),
                Material.transmissive(1.5)]:
        assert np.all(bsdf(mat, n, up, down) == 0)
        assert np.all(bsdf(mat, n, down, up) == 0)
        assert np.all(bsdf(mat, n, up, up) > 0)
    assert np.allclose(bsdf(Material.diffuse(vec3(0.8, 0.5, 0.2)), n, up, up), np.array([0.8, 0.5, 0.2]) / math.pi)
    # material.rs:269-273 tests is_sign_positive, so a grazing wo (n.wo == +0.0) still passes
    assert np.all(bsdf(Material.mirror(), n, (1, 0, 0.0), up) == 1)


def test_lambertian_sampling_is_cosine_weighted():
    mat = Material.diffuse(vec3(0.7, 0.6, 0.5))
    for n in [(0.0, 0.0, 1.0), (0.0, -1.0, 0.0), (0.0, 1.0, 0.0), tuple(np.array([1.0, 2.0, -2.0]) / 3.0)]:
        wo = n
        acc, inv_pdf, N = np.zeros(3), 0.0, 4000
        for i in range(N):
            some, wi, pdf, draws = sample_f(mat, n, wo, 11, i)
            assert some and draws == 2 and abs(np.linalg.norm(wi) - 1) < 1e-12
            c = float(np.dot(wi, n))
            assert c > -1e-12 and abs(pdf - c / math.pi) < 1e-9      # pdf = cos/pi (material.rs:179)
            acc += bsdf(mat, n, wo, wi) * abs(c) / pdf
            inv_pdf += c / pdf
        assert np.allclose(acc / N, [0.7, 0.6, 0.5], rtol=1e-9)       # f*cos/pdf == albedo, every sample
        assert abs(inv_pdf / N - math.pi) < 1e-9


def test_phong_pdf_is_normalised_and_rotation_fallbacks():
    mat = Material.specular(vec3(1, 1, 1), 3.0)
    n, wo = (0.0, 0.0, 1.0), tuple(np.array([0.3, 0.2, 0.9]) / np.linalg.norm([0.3, 0.2, 0.9]))
    N, s = 6000, 0.0
    refl = 2 * np.dot(n, wo) * np.array(n) - np.array(wo)
    for i in range(N):
        some, wi, pdf, draws = sample_f(mat, n, wo, 5, i)
        assert some and draws == 2
        c = float(np.dot(wi, refl))
        assert abs(pdf - 4.0 / (2 * math.pi) * c ** 3) < 1e-9          # (s+1)/(2 pi) cos^s about the mirror direction
        s += c
    assert abs(s / N - 4.0 / 5.0) < 0.01                              # E[cos] = (s+1)/(s+2) under pdf ~ cos^s
    # reflected == -Y: quat_rotation falls back to identity -> lobe around +Y
    some, wi, pdf, _ = sample_f(Material.specular(vec3(1, 1, 1), 200.0), (0.0, -1.0, 0.0), (0.0, -1.0, 0.0), 1, 0)
    assert wi[1] > 0.9
    # Lambertian with n == -Y: retry from (0,1,1e-8) = half-turn about X -> hemisphere below (material.rs:186-194)
    some, wi, pdf, _ = sample_f(Material.diffuse(vec3(1, 1, 1)), (0.0, -1.0, 0.0), (0.0, -1.0, 0.0), 1, 0)
    assert wi[1] < 0 and abs(pdf + wi[1] / math.pi) < 1e-9


def test_mirror_and_transmissive():
    n = (0.0, 0.0, 1.0)
    wo = np.array([0.6, 0.0, 0.8])
    some, wi, pdf, draws = sample_f(Material.mirror(), n, wo, 0, 0)
    assert some and pdf == 1.0 and draws == 0 and np.allclose(wi, [-0.6, 0.0, 0.8])
    glass = Material.transmissive(1.5)
    refl = refr = 0
    for i in range(2000):
        some, wi, pdf, draws = sample_f(glass, n, wo, 3, i)
        assert some and pdf == 1.0 and draws == 1
        if wi[2] > 0:
            refl += 1
            assert np.allclose(wi, [-0.6, 0.0, 0.8])
        else:
            refr += 1                                   # Snell: sin_t = 0.6 / 1.5
            assert abs(math.hypot(wi[0], wi[1]) - 0.4) < 1e-12 and abs(np.linalg.norm(wi) - 1) < 1e-12
    r0 = ((1 - 1.5) / (1 + 1.5)) ** 2
    schlick = r0 + (1 - r0) * (1 - 0.8) ** 5
    assert abs(refl / 2000 - schlick) < 0.02
    # total internal reflection from inside at a grazing angle -> None unless the Fresnel branch reflects
    wo_in = np.array([0.9, 0.0, -math.sqrt(1 - 0.81)])
    nones = sum(1 for i in range(200) if not sample_f(glass, n, wo_in, 4, i)[0])
    assert nones > 0


# ---- KAT 10: medium
def test_medium_sample_d_is_exponential():
    L = pyoracle.lib()
    sa, ss = 5e-5, 3e-3
    ds = []
    for i in range(20000):
        dist, pdf, cdf = C.c_double(), C.c_double(), C.c_double()
        L.orc_medium_sample_d(0, sa, ss, C.c_uint64(9), i, 0, C.byref(dist), C.byref(pdf), C.byref(cdf))
        st = sa + ss
        assert abs(pdf.value - st * math.exp(-st * dist.value)) < 1e-15
        assert abs(cdf.value - (1 - math.exp(-st * dist.value))) < 1e-12
        ds.append(dist.value)
    ds = np.array(ds)
    assert abs(ds.mean() * (sa + ss) - 1.0) < 0.03
    assert abs((ds < 1 / (sa + ss)).mean() - (1 - math.exp(-1))) < 0.015


def test_medium_phase_sampling_normalises_a_cube_sample():
    L = pyoracle.lib()
    for kind, p_expect in [(0, 1 / (4 * math.pi)), (1, 1.0 / 4.0 * math.pi)]:   # medium.rs:85 vs :110 (sic)
        wi, p = D(0, 0, 0), C.c_double()
        L.orc_medium_sample_ph(kind, C.c_uint64(2), 7, 0, wi, C.byref(p))
        assert abs(np.linalg.norm(list(wi)) - 1) < 1e-12 and p.value == p_expect
    u = np.zeros(3)
    L.orc_rng_uniform(C.c_uint64(2), 7, 0, 3, u.ctypes.data_as(C.c_void_p))
    wi, p = D(0, 0, 0), C.c_double()
    L.orc_medium_sample_ph(0, C.c_uint64(2), 7, 0, wi, C.byref(p))
    v = 2 * u - 1
    assert np.allclose(list(wi), v / np.linalg.norm(v), rtol=1e-14)


# ---- KAT 11: C1 is black under the reference's visibility test
def test_spheres_example_renders_black():
    scene, cam, cfg = scenes.spheres()
    img, cnt = OracleScene(scene).render(cam, 48, 48, 4, cfg["max_bounces"], seed=0, counters=True)
    assert np.all(img == 0.0)
    assert cnt["shadow_tests"] > 0 and cnt["shadow_pass"] == 0


# ---- KAT 12: white furnace
def furnace_scene(rho, ambient):
    s = 10.0
    scene = Scene()
    m = Material.diffuse(vec3(rho, rho, rho))
    quads = [  # inward-facing normals ((v2-v1)x(v3-v1) points into the box)
        [(-s, -s, -s), (-s, -s, s), (s, -s, s), (s, -s, -s)],     # floor, n = +y
        [(-s, s, -s), (s, s, -s), (s, s, s), (-s, s, s)],         # ceiling, n = -y
        [(-s, -s, -s), (-s, s, -s), (-s, s, s), (-s, -s, s)],     # x = -s, n = +x
        [(s, -s, -s), (s, -s, s), (s, s, s), (s, s, -s)],         # x = +s, n = -x
        [(-s, -s, -s), (s, -s, -s), (s, s, -s), (-s, s, -s)],     # z = -s, n = +z
        [(-s, -s, s), (-s, s, s), (s, s, s), (s, -s, s)],         # z = +s, n = -z
    ]
    for q in quads:
        scene.add(Object(polygon([vec3(*p) for p in q])).material(m))
    scene.add(Light.Ambient(vec3(ambient, ambient, ambient)))
    cam = Camera(eye=vec3(0.5, 0.3, 0.1), direction=vec3(0, 0, -1), up=vec3(0, 1, 0), fov=1.0)
    return scene, cam


@pytest.mark.parametrize("bounces", [0, 1, 4])
def test_white_furnace_is_a_geometric_series(bounces):
    rho, c = 0.6, 0.25
    scene, cam = furnace_scene(rho, c)
    img = OracleScene(scene).render(cam, 16, 16, 2, bounces, seed=4)
    expect = c * rho * sum(rho ** k for k in range(bounces + 1))
    assert np.allclose(img, expect, rtol=1e-12)


# ---- KAT 13: pixel mapping and camera
def test_pixel_to_ndc_mapping():
    L = pyoracle.lib()
    xn, yn = C.c_double(), C.c_double()
    L.orc_pixel_ndc(0, 0, 256, 256, C.byref(xn), C.byref(yn))
    assert xn.value == -255 / 256 and yn.value == 255 / 256
    L.orc_pixel_ndc(799, 599, 800, 600, C.byref(xn), C.byref(yn))       # dim = max(w, h) = 800
    assert xn.value == 799 / 800 and yn.value == (1 - 600) / 800


def test_camera_pinhole_and_thin_lens():
    L = pyoracle.lib()
    cam = Camera(eye=vec3(1, 2, 3), direction=vec3(0, 0, -1), up=vec3(0, 1, 0), fov=math.pi / 2)
    o, d = D(0, 0, 0), D(0, 0, 0)
    L.orc_camera_cast_ray(C.byref(camera_desc(cam, CameraDesc)), 0.5, -0.25, C.c_uint64(0), 0, 0, o, d)
    v = np.array([0.5, -0.25, -1.0])            # cot(pi/4) = 1; right = dir x up = (1,0,0)
    assert np.allclose(list(o), [1, 2, 3]) and np.allclose(list(d), v / np.linalg.norm(v), rtol=1e-15)
    lens = Camera.look_at(vec3(0, 0, 5), vec3(0, 0, 0), vec3(0, 1, 0), 0.5).focus(vec3(0, 0, 0), 0.2)
    assert lens.focal_distance == 5.0
    for i in range(50):
        L.orc_camera_cast_ray(C.byref(camera_desc(lens, CameraDesc)), 0.1, 0.2, C.c_uint64(1), i, 0, o, d)
        oo, dd = np.array(list(o)), np.array(list(d))
        assert np.hypot(oo[0], oo[1]) <= 0.2 + 1e-12 and oo[2] == 5.0
        # every lens sample passes through the same point at focal distance along the pinhole ray
        pin = np.array([0.1, 0.2, -1 / math.tan(0.25)])
        focal = np.array([0, 0, 5.0]) + pin / np.linalg.norm(pin) * 5.0
        tt = np.dot(focal - oo, dd)
        assert np.allclose(oo + tt * dd, focal, atol=1e-12)


# ---- light sampling and illuminate (light.rs:34-45, mesh.rs:85-99, shape.rs:140-151)
def test_quad_light_illuminate_matches_closed_form():
    scene, cam, cfg = scenes.cornell()
    osc = OracleScene(scene)
    L = pyoracle.lib()
    pos = np.array([278.0, 100.0, 280.0])
    for i in range(200):
        I, wi, dist = D(0, 0, 0), D(0, 0, 0), C.c_double()
        L.orc_light_illuminate(osc.h, 0, D(*pos), C.c_uint64(1), i, 0, I, wi, C.byref(dist))
        wi_ = np.array(list(wi))
        p = pos + dist.value * wi_
        assert abs(p[1] - 548.8) < 1e-9 and 213 - 1e-9 <= p[0] <= 343 + 1e-9 and 227 - 1e-9 <= p[2] <= 332 + 1e-9
        # two triangles of area 130*105/2 each, picked uniformly: pdf = (1/area)/2; normal = -Y
        cos_l = wi_[1]
        expect = hex_color(0xFFFEFA) * 100.0 * cos_l / dist.value ** 2 * (130 * 105 / 2) * 2
        assert np.allclose(list(I), expect, rtol=1e-12)


def test_transformed_sphere_sample_pdf_is_per_world_area():
    L = pyoracle.lib()
    s = sphere().scale(vec3(2, 2, 2)).translate(vec3(0, 0, 8))
    sd, _ = shape_desc(s, ShapeDesc)
    v, n, p = D(0, 0, 0), D(0, 0, 0), C.c_double()
    draws = L.orc_shape_sample(C.byref(sd), D(0, 0, 0), C.c_uint64(0), 3, 0, v, n, C.byref(p))
    vv, nn = np.array(list(v)), np.array(list(n))
    assert draws >= 2 and abs(np.linalg.norm(vv - [0, 0, 8]) - 2) < 1e-12
    assert np.allclose(nn, (vv - [0, 0, 8]) / 2)
    # local pdf z/pi on the unit sphere, divided by the area scale 4 (shape.rs:144-150)
    local = (vv - [0, 0, 8]) / 2
    z = float(np.dot(local, [0, 0, -1]))            # hemisphere faces the target (origin is toward -z in local space)
    assert abs(p.value - z / math.pi / 4) < 1e-12


def test_rng_uniform_is_open_interval_and_exact_in_fp32():
    L = pyoracle.lib()
    u = np.zeros(4096)
    L.orc_rng_uniform(C.c_uint64(123), 5, 6, 4096, u.ctypes.data_as(C.c_void_p))
    assert u.min() > 0 and u.max() < 1
    assert np.array_equal(u.astype(np.float32).astype(np.float64), u)          # representable in fp32
    assert np.all((u * 2 ** 24) % 2 == 1)                                      # odd multiples of 2^-24
    assert abs(u.mean() - 0.5) < 0.02


def test_hdri_lookup_is_equirectangular_bilinear():
    """Hdri::get_color (src/environment.rs:25-52): azimuth = atan2(z, x) + pi, polar = acos(y)."""
    from rpt_amd import Environment
    w, h = 8, 4
    img = np.zeros((h, w, 3))
    img[..., 0] = np.arange(w)[None, :]          # red encodes the column
    img[..., 1] = np.arange(h)[:, None]          # green encodes the row
    sc = Scene()
    sc.environment = Environment.Hdri(w, h, img.reshape(-1, 3))
    osc = OracleScene(sc)
    # no geometry: every camera ray misses and returns the environment
    for d in [(1.0, 0.0, 0.0), (0.0, 0.0, 1.0), (-1.0, 0.2, 0.0), (0.3, 0.9, -0.3), (0.0, -0.7, 0.7)]:
        dv = np.array(d) / np.linalg.norm(d)
        cam = Camera(eye=vec3(0, 0, 0), direction=dv, up=np.cross(np.cross(dv, [0.1, 0.9, 0.3]), dv), fov=1e-6)
        got = osc.render(cam, 1, 1, 1, 0, seed=0)[0]
        az = math.atan2(dv[2], dv[0]) + math.pi
        x = az / (2 * math.pi) * (w - 1)
        y = math.acos(dv[1]) / math.pi * (h - 1)
        assert np.allclose(got, [x, y, 0.0], atol=1e-4)        # a linear ramp is reproduced exactly by bilinear lookup


# ---- the array entry points the per-call device tests compare against (tests/test_gpu_device_samplers.py)
@pytest.mark.parametrize("case", ["A", "B", "C", "D", "E", "F", "G"])
def test_light_sample_is_shape_sample_and_illuminate_bit_for_bit(case):
    """orc_light_sample over an array of positions = orc_shape_sample and orc_light_illuminate case by case, every bit; the word it
    reports after illuminate is the stream's word at the position the shape's own draw count gives."""
    from tests import sampler_cases as sc
    L = pyoracle.lib()
    shape = sc.light_shapes()[case]
    osc = OracleScene(sc.light_scene(shape))
    pos = sc.positions(96, seed=3).astype(np.float64)
    got = osc.light_sample(0, pos, seed=5)
    sd, _keep = shape_desc(shape, ShapeDesc)
    for i in range(pos.shape[0]):
        I, wi, dist = D(0, 0, 0), D(0, 0, 0), C.c_double()
        L.orc_light_illuminate(osc.h, 0, D(*pos[i]), C.c_uint64(5), i, 0, I, wi, C.byref(dist))
        assert list(I) == list(got["intensity"][i]) and list(wi) == list(got["wi"][i]) and dist.value == got["dist"][i]
        v, n, p = D(0, 0, 0), D(0, 0, 0), C.c_double()
        draws = L.orc_shape_sample(C.byref(sd), D(*pos[i]), C.c_uint64(5), i, 0, v, n, C.byref(p))
        assert list(v) == list(got["v"][i]) and list(n) == list(got["nrm"][i]) and p.value == got["p"][i]
        words = np.zeros(draws + 1, dtype=np.uint32)
        L.orc_rng_u32(C.c_uint64(5), i, 0, draws + 1, words.ctypes.data_as(C.c_void_p))
        assert words[draws] == got["next_word"][i]
    assert np.all(np.isfinite(got["intensity"])) and np.all(got["p"] != 0)
    if case in "DG":      # a mirrored transform: the reference divides by a signed area factor
        assert np.all(got["intensity"] <= 0) and np.any(got["intensity"] < 0) and np.all(got["p"] < 0)
    with pytest.raises(ValueError):
        osc.light_sample(1, pos)
    amb = Scene()
    amb.add(Light.Ambient(vec3(1, 1, 1)))
    with pytest.raises(ValueError):
        OracleScene(amb).light_sample(0, pos)


def test_env_color_reproduces_a_linear_ramp():
    """orc_env_color = Environment::get_color: bilinear lookup of a linear ramp is the ramp, x = azimuth / 2 pi (w - 1),
    y = polar / pi (h - 1) (the closed form of test_hdri_lookup_is_equirectangular_bilinear, without the camera)."""
    from tests import sampler_cases as sc
    ramp = sc.sky_images()["ramp8x4"]
    h, w = ramp.shape[:2]
    osc = OracleScene(sc.sky_scene(ramp))
    d = sc.sky_directions().astype(np.float64)
    got = osc.env_color(d)
    u = d / np.linalg.norm(d, axis=1, keepdims=True)
    x = (np.arctan2(u[:, 2], u[:, 0]) + math.pi) / (2 * math.pi) * (w - 1)
    y = np.arccos(u[:, 1]) / math.pi * (h - 1)
    assert np.allclose(got, np.stack([x, y, np.full_like(x, 0.5)], 1), rtol=0, atol=1e-12)
    assert got[:, 0].min() == 0.0 and got[:, 0].max() > 6.99       # both sides of the seam are among the directions
    const = Scene()
    const.environment = Environment.Color(vec3(0.25, 0.5, 0.75))
    assert np.array_equal(OracleScene(const).env_color(d[:5]), np.broadcast_to([0.25, 0.5, 0.75], (5, 3)))


# ---- the array entry points and the case tables of tests/test_gpu_device_materials.py
def _kat_subset(labels, k=192):
    """The first k random cases and every structured one."""
    return np.concatenate([np.arange(k), np.flatnonzero(labels != "")])


@pytest.mark.parametrize("name", ["lambertian", "phong6", "phong1000", "mirror", "glass1.5", "glass1over1.5"])
def test_material_sample_is_sample_f_and_bsdf_bit_for_bit(name):
    """orc_material_sample over an array = orc_material_sample_f, then orc_material_bsdf at its direction, case by case, every bit;
    next_word is the stream's word at the position sample_f's draw count gives; orc_material_bsdf_n = orc_material_bsdf."""
    from tests import material_cases as mc
    L = pyoracle.lib()
    mat = mc.materials()[name]
    n, wo, labels = mc.inputs(name, True)
    got = pyoracle.material_sample(mat, n, wo, seed=5)
    fn = pyoracle.material_bsdf(mat, n, wo, got["wi"])
    md = material_desc(mat, MaterialDesc)
    for i in _kat_subset(labels):
        wi, pdf, draws, f = D(0, 0, 0), C.c_double(), C.c_int(), D(0, 0, 0)
        some = L.orc_material_sample_f(C.byref(md), D(*n[i]), D(*wo[i]), C.c_uint64(5), int(i), 0, wi, C.byref(pdf), C.byref(draws))
        assert some == got["some"][i] and list(wi) == list(got["wi"][i]) and pdf.value == got["pdf"][i]
        L.orc_material_bsdf(C.byref(md), D(*n[i]), D(*wo[i]), wi, f)
        assert list(f) == list(fn[i]) and (list(f) == list(got["f"][i]) if some else not got["f"][i].any())
        words = np.zeros(draws.value + 1, dtype=np.uint32)
        L.orc_rng_u32(C.c_uint64(5), int(i), 0, draws.value + 1, words.ctypes.data_as(C.c_void_p))
        assert words[draws.value] == got["next_word"][i]
    assert np.all(np.isfinite(got["wi"])) and np.all(np.isfinite(got["pdf"]))


def test_rotation_falls_back_below_epsilon_as_nalgebra_does():
    """The pole family on the oracle: for a normal (a, -1, 0) the Lambertian sample is the half-turn about X of the lobe direction
    when a <= f64::EPSILON (2.2e-16; sin(pi) = 1.2e-16 is below) and the half-turn about Z above it; Phong keeps the lobe
    direction (identity) for a mirror direction within EPSILON of -Y."""
    from tests import material_cases as mc
    up = np.array([[0.0, 1.0, 0.0]])
    wo = np.array([[0.3, -0.8, 0.52]]) / np.linalg.norm([0.3, -0.8, 0.52])
    lobe = pyoracle.material_sample(mc.materials()["lambertian"], up, -wo, seed=7)["wi"][0]      # rotation onto +Y: identity
    for a, about_x in ((1e-20, True), (1e-17, True), (math.sin(math.pi), True), (2.2e-16, True), (2.3e-16, False), (1e-15, False), (1e-10, False)):
        wi = pyoracle.material_sample(mc.materials()["lambertian"], np.array([[a, -1.0, 0.0]]), wo, seed=7)["wi"][0]
        expect = lobe * ([1, -1, -1] if about_x else [-1, -1, 1])
        assert np.allclose(wi, expect, rtol=0, atol=1e-7), (a, wi, expect)
    phong = mc.materials()["phong6"]
    lobe = pyoracle.material_sample(phong, up, up, seed=7)["wi"][0]
    for a in (0.0, 1e-17, 2.2e-16):
        wi = pyoracle.material_sample(phong, -up, np.array([[a, -1.0, 0.0]]), seed=7)["wi"][0]
        assert np.allclose(wi, lobe, rtol=0, atol=1e-15), (a, wi, lobe)


@pytest.mark.parametrize("name", ["lambertian", "phong50", "glass1.5"])
def test_bounce_is_trace_rays_continuation(name):
    """orc_bounce = the roulette or the max_bounces rule, orc_material_sample_f, orc_material_bsdf and the weight
    (1 / (pdf rr)) f |wi.n| of Renderer::trace_ray, composed here from the single-call entries; at a medium event the roulette, a
    unit direction and (scat / ext) / ph_p * colour * phase / 0.8.  (That the factored halves still are trace_ray's arithmetic is
    what the golden frames pin.)"""
    from rpt_amd import Medium
    from tests import material_cases as mc
    mat = mc.materials()[name]
    n, wo, labels = mc.inputs(name, True)
    idx = _kat_subset(labels, 96)
    n, wo = n[idx], wo[idx]
    won = wo / np.linalg.norm(wo, axis=1, keepdims=True)
    fog = Medium.homogeneous_isotropic(0.02, 0.1)
    u = mc.uniforms(5, n.shape[0], 1)[:, 0]
    plain = pyoracle.bounce(mat, n, -wo, max_bounces=3, depth=1, seed=5)
    s = pyoracle.material_sample(mat, n, -(-won), seed=5)
    dot = s["wi"][:, 0] * n[:, 0] + s["wi"][:, 1] * n[:, 1] + s["wi"][:, 2] * n[:, 2]      # (in the oracle's order)
    with np.errstate(divide="ignore", invalid="ignore"):
        k = (1.0 / s["pdf"])[:, None] * s["f"] * np.abs(dot)[:, None]
    assert np.array_equal(plain["cont"], s["some"]) and np.array_equal(plain["next_word"], s["next_word"])
    on = s["some"] == 1
    assert np.array_equal(plain["wi"][on], s["wi"][on]) and np.array_equal(plain["k"][on], k[on])
    assert not plain["k"][~on].any() and not plain["wi"][~on].any()
    last = pyoracle.bounce(mat, n, -wo, max_bounces=3, depth=3, seed=5)
    assert not last["cont"].any() and not last["k"].any() and np.array_equal(last["next_word"], pyoracle.bounce(mat, n, -wo, max_bounces=0, depth=0, seed=5)["next_word"])
    foggy = pyoracle.bounce(mat, n, -wo, max_bounces=0, depth=7, seed=5, medium=fog)          # max_bounces plays no part in a medium
    assert np.array_equal(foggy["cont"] == 1, (u < 0.8) & (foggy["cont"] == 1)) and not foggy["cont"][u >= 0.8].any()
    if mat.kind != 3:
        assert np.array_equal(foggy["cont"] == 1, u < 0.8)
    ev = pyoracle.bounce(mat, n, -wo, seed=5, medium=fog, medium_event=True)
    assert np.array_equal(ev["cont"] == 1, u < 0.8)
    go = ev["cont"] == 1
    assert np.allclose(np.linalg.norm(ev["wi"][go], axis=1), 1.0, rtol=0, atol=1e-15)
    ph = 1.0 / (4.0 * math.pi)
    expect = np.array(hex_color(0xD2B48C)) * ((0.1 / (0.02 + 0.1)) / ph) * ph / 0.8
    assert np.allclose(ev["k"][go], expect, rtol=1e-15, atol=0) and not ev["k"][~go].any()
    with pytest.raises(ValueError):
        pyoracle.bounce(mat, n, -wo, medium_event=True)


def test_camera_rays_is_pixel_ndc_jitter_and_cast_ray():
    """orc_camera_rays for a pinhole = orc_pixel_ndc, two uniforms and orc_camera_cast_ray (whose restart of the stream does not
    matter without a lens), every bit, and next_word is the stream's third word; for a lens next_word is the word after the jitter
    and the candidates material_cases.lens_flags counts."""
    from tests import material_cases as mc
    L = pyoracle.lib()
    for name, cam in mc.cameras().items():
        for w, h in ((33, 17), (17, 33), (1, 1)):
            got = pyoracle.camera_rays(cam, w, h, sample=1023, seed=7)
            flagged, cands = mc.lens_flags(w, h, 1023, seed=7)
            cd = camera_desc(cam, CameraDesc)
            dim = float(max(w, h))
            for i in range(w * h):
                draws = 2 + (2 * int(cands[i]) if cam.aperture > 0 else 0)
                words = np.zeros(draws + 1, dtype=np.uint32)
                L.orc_rng_u32(C.c_uint64(7), i, 1023, draws + 1, words.ctypes.data_as(C.c_void_p))
                assert words[draws] == got["next_word"][i], (name, w, h, i)
                if cam.aperture > 0:
                    continue
                xn, yn, uu = C.c_double(), C.c_double(), np.zeros(2)
                L.orc_pixel_ndc(i % w, i // w, w, h, C.byref(xn), C.byref(yn))
                L.orc_rng_uniform(C.c_uint64(7), i, 1023, 2, uu.ctypes.data_as(C.c_void_p))
                o, d = D(0, 0, 0), D(0, 0, 0)
                L.orc_camera_cast_ray(C.byref(cd), xn.value + (-1.0 / dim + (1.0 / dim - -1.0 / dim) * uu[0]),
                                      yn.value + (-1.0 / dim + (1.0 / dim - -1.0 / dim) * uu[1]), C.c_uint64(7), i, 1023, o, d)
                assert list(o) == list(got["o"][i]) and list(d) == list(got["d"][i]), (name, w, h, i)
            if cam.aperture > 0:
                assert np.all(np.linalg.norm(got["o"] - cam.eye, axis=1) <= cam.aperture * (1 + np.linalg.norm(cam.up)))   # |dx right + dy up|


def test_material_cases_flag_few_random_cases_and_only_named_structured_ones():
    """What tests/test_gpu_device_materials.py relies on: the flags (decisions fp32 cannot be asked to reproduce, from the reference
    alone) cover at most 0.5 % of the random cases of any material -- a handful of 4096 --, every structured case is unflagged or
    named in material_cases.BOUNDARY, no pixel of the camera frames is flagged, and the numpy restatements the flagged cases are
    judged by (the glass outcomes, the bsdf with its sign tests passed, sample_f's pdf) agree with the oracle where nothing is flagged."""
    from tests import material_cases as mc
    for name, mat in mc.materials().items():
        for f64 in (False, True):
            n, wo, labels = mc.inputs(name, f64)
            m = n.shape[0]
            ref = pyoracle.material_sample(mat, n, wo, seed=mc.SEED)
            fl = mc.sample_flags(name, n, wo, mc.SEED)
            sflag = fl["u_sr"] | fl["k"]
            wi = np.where((ref["some"] == 1)[:, None], ref["wi"], wo)
            bflag = mc.bsdf_flags(n, wo, wi)
            rnd, named = labels == "", mc.is_boundary(labels, name)
            assert (sflag | bflag)[rnd].mean() <= 0.005, name
            stray = np.flatnonzero((sflag | bflag) & ~rnd & ~named)
            assert stray.size == 0, (name, labels[stray])
            u = mc.uniforms(mc.SEED, m, 2)
            assert np.allclose(mc.sample_pdf(name, u[:, 1]), ref["pdf"], rtol=1e-12, atol=0) or mat.kind == 3
            unsigned = mc.bsdf_unsigned(name, n, wo, wi)
            both = (np.einsum("ij,ij->i", n, wi) > 0) & (np.einsum("ij,ij->i", n, wo) > 0) & (ref["some"] == 1)
            assert both.sum() > 100 or mat.kind == 3
            assert np.allclose(unsigned[both], ref["f"][both], rtol=1e-9, atol=1e-300), name
            if mat.kind == 3:
                reflect, refract, g = mc.glass_outcomes(n, wo, mat.ior)
                refl = u[:, 0] < g["sr"]
                clear = ~sflag
                assert np.array_equal(ref["some"][clear] == 1, (refl | (g["k"] >= 0))[clear])
                assert np.allclose(ref["wi"][clear & refl], reflect[clear & refl], rtol=0, atol=1e-12)
                thru = clear & ~refl & (g["k"] >= 0)
                assert np.allclose(ref["wi"][thru], refract[thru], rtol=0, atol=1e-12)
                assert refl[rnd].sum() > 50 and thru[rnd].sum() > 500 and (clear & ~refl & (g["k"] < 0)).sum() >= (16 if mat.ior != 1.0 else 0)
        n2, wo2, wi2, labels2 = mc.bsdf_inputs(name, False)
        assert mc.bsdf_flags(n2, wo2, wi2)[labels2 == ""].mean() <= 0.005
        # the tangent-plane inputs: zero normal components of both signs, decided by the sign of an exact zero
        tang = labels2 == "tangent"
        f = pyoracle.material_bsdf(mat, n2[tang], wo2[tang], wi2[tang])
        lit = np.any(f != 0, axis=1).sum()
        assert lit < tang.sum() and (lit > 0 or mat.shininess >= 50), name      # (a narrow lobe is zero at these angles anyway)
    for w, h in mc.FRAMES:
        for sample in mc.SAMPLES:
            flagged, cands = mc.lens_flags(w, h, sample)
            assert not flagged.any() and cands.max() > (1 if w * h > 1 else 0)


# ---- the path recorder only looks on (orc_render_paths; tests/path_cloud.py)
@pytest.mark.parametrize("fog", [None, "fog"])
@pytest.mark.parametrize("robust", [0, 1])
def test_path_records_leave_the_radiance_bit_identical(fog, robust):
    from tests import path_cloud as pc
    sc, cam, mb = pc.clamp(fog, torus=True)
    orc = OracleScene(sc)
    for off in (0, 3):
        plain, cnt = orc.render(cam, 48, 48, 1, mb, seed=6, sample_offset=off, robust=robust, counters=True)
        rad, rec, light_pass = orc.render_paths(cam, 48, 48, mb, seed=6, sample_offset=off, robust=robust, threads=3)
        assert np.array_equal(rad.view(np.uint64), plain.view(np.uint64))
        # and the record counts what the counters count: one level per trace_ray call, the shadow passes
        assert light_pass.sum() == cnt["shadow_pass"] and cnt["samples"] == len(rec)
        assert rec["levels"].sum() == cnt["vertices"]
        assert (rec["clamp"] != 0).sum() >= (150 if fog is None else 0) and ((rec["clamp"] != 0).sum() == 0 or fog is None)
