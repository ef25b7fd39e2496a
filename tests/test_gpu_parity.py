"""GPU parity tests: the HIP path (through the C ABI) against the fp64 oracle on the same seeded
inputs.  Tolerances are stated per test."""
import ctypes as C

import numpy as np
import pytest

from rpt_amd import Camera, Material, Object, Renderer, RptError, Scene, plane, scenes, vec3
from rpt_amd import _lib
from tests.util import random_rays, rel_rms

pytestmark = pytest.mark.gpu


def _oracle(scene):
    from oracle.pyoracle import OracleScene
    return OracleScene(scene)


def test_rng_stream_bit_exact(oracle_lib):
    lib = _lib.load()
    for seed, pixel, sample in [(0, 0, 0), (1, 12345, 7), (2 ** 63 + 5, 4194303, 1023)]:
        got = np.zeros(64, dtype=np.uint32)
        _lib.check(lib.rpt_debug_rng_u32(C.c_uint64(seed), pixel, sample, 64, got.ctypes.data_as(C.c_void_p)))
        exp = np.zeros(64, dtype=np.uint32)
        oracle_lib.orc_rng_u32(C.c_uint64(seed), pixel, sample, 64, exp.ctypes.data_as(C.c_void_p))
        assert np.array_equal(got, exp)


@pytest.mark.parametrize("name,center,radius", [("C1", (0.5, 0.0, 1.0), 12.0), ("C2", (278.0, 274.0, 280.0), 700.0),
                                                ("C3", (278.0, 274.0, 280.0), 700.0)])
def test_closest_hit_matches_oracle(name, center, radius):
    scene, cam, cfg = scenes.CONFIGS[name]()
    rng = np.random.default_rng(1)
    o, d = random_rays(rng, 20000, np.array(center), radius)
    t, obj, nrm = Renderer(scene, cam).get_closest_hit(o, d)
    # the oracle is given the fp32-rounded rays so both trace the same input
    te, obje, nrme = _oracle(scene).intersect(o.astype(np.float32), d.astype(np.float32), robust=1)
    same = obj == obje
    # Coincident surfaces (the Cornell box stands exactly on the floor) are decided by rounding in
    # fp64 and fp32 alike: a different object at the same distance is not a mismatch.
    both = (obj >= 0) & (obje >= 0)
    coincident = both & ~same & (np.abs(t - te) <= 2e-4 * np.abs(te))
    assert (same | coincident).mean() > 0.9995          # silhouette / edge rays may flip in fp32
    hit = same & (obje >= 0)
    assert hit.sum() > 5000
    assert np.max(np.abs(t[hit] - te[hit]) / te[hit]) < 2e-4
    assert np.max(np.abs(nrm[hit] - nrme[hit])) < 2e-3
    assert np.all(np.isinf(t[same & (obje < 0)]))


@pytest.mark.parametrize("name,size,spp,tol", [("C1", 64, 8, 0.0), ("C1lit", 64, 16, 2e-3), ("C2", 96, 32, 2e-3),
                                               ("C3", 96, 32, 3e-3)])
def test_render_matches_oracle_same_seed(name, size, spp, tol):
    """Same seed, same RNG stream: the fp32 image must match the fp64 oracle (robust epsilon
    policy, i.e. the one the fp32 path implements) to a relative RMS of `tol`."""
    scene, cam, cfg = (scenes.spheres_lit() if name == "C1lit" else scenes.CONFIGS[name]())
    r = Renderer(scene, cam).width(size).height(size).max_bounces(cfg["max_bounces"]).seed(3)
    got = r.sample_array(spp)
    exp = _oracle(scene).render(cam, size, size, spp, cfg["max_bounces"], seed=3, robust=1)
    assert np.all(np.isfinite(got))
    if tol == 0.0:
        assert np.all(got == 0.0) and np.all(exp == 0.0)   # KAT 11: C1 is black
    else:
        assert rel_rms(got, exp) < tol


# ------------------------------------------------------------------ device function hooks
def _mat_desc(mat):
    from rpt_amd.api import material_desc
    return material_desc(mat, _lib.MaterialDesc)


@pytest.mark.parametrize("kind", ["diffuse", "phong", "mirror", "glass"])
def test_sample_f_and_bsdf_match_oracle(kind, oracle_lib):
    from oracle.pyoracle import MaterialDesc
    from rpt_amd import Material, vec3
    from rpt_amd.api import material_desc
    mat = {"diffuse": Material.diffuse(vec3(0.7, 0.5, 0.3)), "phong": Material.specular(vec3(0.7, 0.5, 0.3), 6.0),
           "mirror": Material.mirror(), "glass": Material.transmissive(1.5)}[kind]
    rng = np.random.default_rng(2)
    n = 4096
    nrm = rng.normal(size=(n, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    nrm[:8] = [[0, 1, 0], [0, -1, 0], [1, 0, 0], [0, 0, 1], [0, 0, -1], [-1, 0, 0], [0, 1, 0], [0, -1, 0]]
    wo = rng.normal(size=(n, 3))
    wo /= np.linalg.norm(wo, axis=1, keepdims=True)
    if kind != "glass":
        wo = np.where((np.einsum("ij,ij->i", wo, nrm) < 0)[:, None], -wo, wo)      # above the surface
    nrm32, wo32 = nrm.astype(np.float32), wo.astype(np.float32)
    lib = _lib.load()
    wi = np.zeros((n, 3), np.float32)
    pdf = np.zeros(n, np.float32)
    some = np.zeros(n, np.int32)
    md = _mat_desc(mat)
    _lib.check(lib.rpt_debug_material_sample_f(C.byref(md), n, nrm32.ctypes.data_as(C.c_void_p),
                                               wo32.ctypes.data_as(C.c_void_p), C.c_uint64(7),
                                               wi.ctypes.data_as(C.c_void_p), pdf.ctypes.data_as(C.c_void_p),
                                               some.ctypes.data_as(C.c_void_p)))
    omd = material_desc(mat, MaterialDesc)
    wie, pdfe, somee = np.zeros((n, 3)), np.zeros(n), np.zeros(n, np.int32)
    D3 = C.c_double * 3
    for i in range(n):
        w, p = D3(), C.c_double()
        somee[i] = oracle_lib.orc_material_sample_f(C.byref(omd), D3(*nrm32[i].astype(float)), D3(*wo32[i].astype(float)),
                                                    C.c_uint64(7), i, 0, w, C.byref(p), None)
        wie[i], pdfe[i] = list(w), p.value
    assert np.array_equal(some, somee)
    ok = somee == 1
    assert np.max(np.abs(wi[ok] - wie[ok])) < 5e-5                      # fp32 tolerance on a unit vector
    assert np.max(np.abs(pdf[ok] - pdfe[ok]) / np.maximum(pdfe[ok], 1e-3)) < 2e-4
    # bsdf on (n, wo, wi_oracle)
    wi_in = wie.astype(np.float32)
    f = np.zeros((n, 3), np.float32)
    _lib.check(lib.rpt_debug_material_bsdf(C.byref(md), n, nrm32.ctypes.data_as(C.c_void_p),
                                           wo32.ctypes.data_as(C.c_void_p), wi_in.ctypes.data_as(C.c_void_p),
                                           f.ctypes.data_as(C.c_void_p)))
    fe = np.zeros((n, 3))
    for i in range(n):
        o = D3()
        oracle_lib.orc_material_bsdf(C.byref(omd), D3(*nrm32[i].astype(float)), D3(*wo32[i].astype(float)),
                                     D3(*wi_in[i].astype(float)), o)
        fe[i] = list(o)
    # sign decisions at exactly grazing wi may flip in fp32; everything else within 1e-3 relative
    bad = np.abs(f - fe) > 2e-3 * np.maximum(np.abs(fe), 1e-2)
    assert bad.any(axis=1).mean() < 2e-3


def test_camera_rays_match_oracle(oracle_lib):
    from oracle.pyoracle import CameraDesc
    from rpt_amd.api import camera_desc
    scene, cam, cfg = scenes.spheres()                      # thin lens: exercises UnitDisc rejection
    w, h = 32, 24
    prm = _lib.RenderParams(w, h, 0.0, 0, 0, 1)
    o = np.zeros((w * h, 3), np.float32)
    d = np.zeros((w * h, 3), np.float32)
    _lib.check(_lib.load().rpt_debug_camera_rays(C.byref(camera_desc(cam, _lib.CameraDesc)), C.byref(prm),
                                                 C.c_uint64(3), 5, o.ctypes.data_as(C.c_void_p),
                                                 d.ctypes.data_as(C.c_void_p)))
    D3 = C.c_double * 3
    cd = camera_desc(cam, CameraDesc)
    dim = float(max(w, h))
    for i in range(0, w * h, 7):
        x, y = i % w, i // w
        xn, yn = C.c_double(), C.c_double()
        oracle_lib.orc_pixel_ndc(x, y, w, h, C.byref(xn), C.byref(yn))
        u = np.zeros(2)
        oracle_lib.orc_rng_uniform(C.c_uint64(3), i, 5, 2, u.ctypes.data_as(C.c_void_p))
        dx, dy = -1 / dim + (2 / dim) * u[0], -1 / dim + (2 / dim) * u[1]
        # the oracle's cast_ray restarts the stream, so feed it a stream advanced by the 2 jitter draws:
        # compare through the full render path instead when apertures are involved
        oo, dd = D3(), D3()
        oracle_lib.orc_camera_cast_ray(C.byref(cd), xn.value + dx, yn.value + dy, C.c_uint64(3), i, 5, oo, dd)
        # same focal point regardless of the lens sample: the GPU ray must pass through it
        pin_o, pin_d = np.array(cam.eye), None
        pc = type(cam)(cam.eye, cam.direction, cam.up, cam.fov)        # pinhole twin
        po, pd = D3(), D3()
        oracle_lib.orc_camera_cast_ray(C.byref(camera_desc(pc, CameraDesc)), xn.value + dx, yn.value + dy,
                                       C.c_uint64(3), i, 5, po, pd)
        focal = np.array(list(po)) + np.array(list(pd)) * cam.focal_distance
        tt = np.dot(focal - o[i], d[i])
        assert np.linalg.norm(o[i] + tt * d[i] - focal) < 2e-4
        assert np.linalg.norm(o[i] - cam.eye) <= cam.aperture * (1 + 1e-5)
        assert abs(np.linalg.norm(d[i]) - 1) < 1e-5


# ------------------------------------------------------------------ whole-path properties
def test_white_furnace_is_exact_on_the_gpu():
    from tests.test_oracle_kat import furnace_scene
    rho, c = 0.6, 0.25
    for bounces in (0, 3):
        scene, cam = furnace_scene(rho, c)
        got = Renderer(scene, cam).width(40).height(24).max_bounces(bounces).seed(1).sample_array(4)
        expect = c * rho * sum(rho ** k for k in range(bounces + 1))
        assert np.allclose(got, expect, rtol=2e-5)


def test_shards_grid_sizes_and_reruns_are_bit_identical():
    import rpt_amd
    scene, cam, cfg = scenes.lampshade()
    w, h, spp = 100, 70, 9                                   # ragged: tiles clipped, spp not a chunk multiple
    grids = []
    def render(rank=0, count=1):
        s2, c2, _ = scenes.lampshade()
        s2.set_option("timing", 1)
        r = Renderer(s2, c2).width(w).height(h).max_bounces(10).seed(2).shard(rank, count)
        img = r.sample_array(spp)
        grids.append(r.timing()[2])
        return img
    full = render()
    assert np.array_equal(full, render())                    # deterministic
    parts = [render(r, 3) for r in range(3)]
    owned = [(p != 0).any(axis=1) for p in parts]
    assert np.array_equal(sum(parts), full)                  # disjoint shards, zeros elsewhere
    assert (np.sum(owned, axis=0) <= 1).all()
    rpt_amd.set_option("blocks_per_cu", 1)
    try:
        assert np.array_equal(full, render())                # independent of the persistent grid size
    finally:
        rpt_amd.set_option("blocks_per_cu", 0)
    # 12 tiles x 1024 pixel slots x 5 chunks = 61,440 items are 240 blocks' worth: blocks_per_cu = 1 launches the same grid on a card
    # with 240 CUs or more.  "max_blocks" does change it: 1 block (240 items per lane) and 7 blocks (34 per lane)
    default_grid, n_items = grids[0], 12 * 1024 * Renderer(scene, cam).chunking(spp)[1]
    assert n_items <= default_grid * 256                     # every lane of the frames above had one item at most
    try:
        for cap in (1, 7):
            rpt_amd.set_option("max_blocks", cap)
            assert np.array_equal(full, render())
            assert grids[-1] == cap != default_grid and n_items >= 8 * cap * 256
            print(f"max_blocks {cap}: {grids[-1]} blocks instead of {default_grid}, {n_items / (cap * 256):.1f} items per lane")
        rpt_amd.set_option("max_blocks", 3)                  # ... and the shards on a small grid
        assert np.array_equal(sum(render(r, 3) for r in range(3)), full)
    finally:
        rpt_amd.set_option("max_blocks", 0)
    exp = _oracle(scene).render(cam, w, h, spp, 10, seed=2, robust=1)
    assert rel_rms(full, exp) < 5e-3


def test_sample_offset_and_exposure_follow_iterative_render():
    scene, cam, cfg = scenes.cornell()
    r = Renderer(scene, cam).width(48).height(48).max_bounces(2).seed(4).exposure_value(1.0)
    a = r.sample_array(4)                                    # samples 0..3
    b = r.sample_array(4)                                    # samples 4..7 (iterative_render, renderer.rs:144-156)
    orc = _oracle(scene)
    ea = orc.render(cam, 48, 48, 4, 2, seed=4, sample_offset=0, exposure_value=1.0, robust=1)
    eb = orc.render(cam, 48, 48, 4, 2, seed=4, sample_offset=4, exposure_value=1.0, robust=1)
    assert rel_rms(a, ea) < 3e-3 and rel_rms(b, eb) < 3e-3
    assert rel_rms(a, eb) > 0.05                             # different sample indices -> different noise


def _materials_scene(fog=None):
    from rpt_amd import Light, Material, Medium, Object, Scene, cube, hex_color, plane, polygon, sphere, vec3, Camera
    sc = Scene()
    sc.add(Object(plane(vec3(0, 1, 0), 0.0)).material(Material.diffuse(hex_color(0xCCCCCC))))
    sc.add(Object(sphere().translate(vec3(-2.2, 1, 0))).material(Material.mirror()))
    sc.add(Object(sphere().scale(vec3(1, 1.3, 1)).translate(vec3(0, 1.3, 0))).material(Material.transmissive(1.5)))
    sc.add(Object(cube().scale(vec3(1.5, 1.5, 1.5)).rotate_y(0.6).translate(vec3(2.4, 0.75, 0.3))).material(
        Material.specular(hex_color(0xE7A94D), 8.0)))
    sc.add(Object(sphere().scale(vec3(0.6, 0.6, 0.6)).translate(vec3(0.8, 0.6, 2.0))).material(
        Material.metallic(hex_color(0x7CA3E7), 0.4)))
    quad = polygon([vec3(2, 5, -2), vec3(2, 5, 2), vec3(-2, 5, 2), vec3(-2, 5, -2)])
    sc.add((quad, Material.light(vec3(1, 1, 1), 12.0)))
    sc.add((cube().scale(vec3(0.5, 0.5, 0.5)).translate(vec3(-3.5, 2.5, 2.0)), Material.light(vec3(1.0, 0.6, 0.3), 30.0)))
    lamp = sphere().scale(vec3(0.4, 0.4, 0.4)).translate(vec3(3.5, 3.0, 2.5))
    sc.add(Object(lamp).material(Material.light(vec3(0.4, 0.6, 1.0), 40.0)))
    sc.add(Light.Object(Object(sphere().scale(vec3(0.4, 0.4, 0.4)).translate(vec3(3.5, 3.0, 2.5))).material(
        Material.light(vec3(0.4, 0.6, 1.0), 40.0))))
    sc.add(Light.Ambient(vec3(0.02, 0.02, 0.03)))
    sc.add(Light.Point(vec3(5, 5, 5), vec3(0, 8, 0)))       # never passes the reference's test: contributes 0
    sc.add(Light.Directional(vec3(1, 1, 1), vec3(0, -1, 0)))
    sc.environment.color = np.array([0.05, 0.07, 0.1])
    if fog == "fog":
        sc.add(Medium.homogeneous_isotropic(0.01, 0.04))
    elif fog == "glow":
        sc.add(Medium.colored_glowing_fog(0.02, 0.02))
    cam = Camera.look_at(vec3(0.5, 3.0, 8.0), vec3(0, 1, 0), vec3(0, 1, 0), 0.6)
    return sc, cam


@pytest.mark.parametrize("fog,tol", [(None, 4e-3), ("fog", 6e-3), ("glow", 6e-3)])
def test_all_materials_lights_and_media_match_oracle(fog, tol):
    """Mirror, Transmissive, Phong (two shininess values), Lambertian; quad, cube and sphere object
    lights with twins; ambient / point / directional lights; environment colour; both media."""
    scene, cam = _materials_scene(fog)
    size, spp, mb = 80, 24, 4
    got = Renderer(scene, cam).width(size).height(size).max_bounces(mb).seed(6).sample_array(spp)
    exp, cnt = _oracle(scene).render(cam, size, size, spp, mb, seed=6, robust=1, counters=True)
    assert np.all(np.isfinite(got)) and cnt["shadow_pass"] > 1000
    assert rel_rms(got, exp) < tol
    assert abs(got.mean() - exp.mean()) / exp.mean() < 2e-3


# ------------------------------------------------------------------ BVH mesh path (C5 row)
def test_mesh_closest_hit_matches_oracle_kdtree():
    import math
    from rpt_amd import Material, Mesh, Object, Scene, Camera, plane, vec3
    tris = scenes.bumpy_torus(96, 96)                        # 18,432 triangles -> BVH on the device, kd-tree in the oracle
    sc = Scene()
    sc.add(Object(Mesh(tris).scale(vec3(3.4, 3.4, 3.4)).rotate_y(math.pi / 2)).material(Material.diffuse(vec3(1, 1, 1))))
    sc.add(Object(plane(vec3(0, 1, 0), -1.0)).material(Material.diffuse(vec3(1, 1, 1))))
    cam = Camera()
    rng = np.random.default_rng(3)
    o, d = random_rays(rng, 40000, np.zeros(3), 4.0)
    t, obj, nrm = Renderer(sc, cam).get_closest_hit(o, d)
    te, obje, nrme = _oracle(sc).intersect(o.astype(np.float32), d.astype(np.float32), robust=1)
    same = obj == obje
    assert same.mean() > 0.999
    hit = same & (obje >= 0)
    assert (obje == 0).sum() > 5000
    rel = np.abs(t[hit] - te[hit]) / te[hit]
    assert np.quantile(rel, 0.999) < 2e-4                    # silhouette edges may pick the neighbouring triangle
    close = hit & (np.abs(t - te) <= 2e-4 * te)
    assert np.quantile(np.abs(nrm[close] - nrme[close]).max(axis=1), 0.999) < 5e-3


def test_mesh_in_fog_render_matches_oracle():
    scene, cam, cfg = scenes.mesh_in_fog(nu=64, nv=64)       # 8,192-triangle version of config C5
    size, spp = 64, 16
    got = Renderer(scene, cam).width(size).height(size).max_bounces(cfg["max_bounces"]).seed(8).sample_array(spp)
    exp = _oracle(scene).render(cam, size, size, spp, cfg["max_bounces"], seed=8, robust=1)
    assert np.all(np.isfinite(got)) and exp.mean() > 0
    assert rel_rms(got, exp) < 1e-2
    assert abs(got.mean() - exp.mean()) / exp.mean() < 5e-3


def test_c5_at_its_configured_mesh_size_matches_oracle():
    """Config C5 as bench.py --workload C5 renders it: scenes.mesh_in_fog() at its default 224 x 224 x 2 = 100,352
    triangles (examples/dragon.rs:32-73 layout).  The device walks its two-box BVH with deferred, resumable walks; the
    oracle walks the reference's kd-tree (src/kdtree.rs:154-226) recursively.  (a) closest hits on 40 k rays,
    (b) a 64x64x16 render of the full mesh in fog at the same seed.  tests/golden/C5.npz freezes the same two things."""
    scene, cam, cfg = scenes.mesh_in_fog()
    r = Renderer(scene, cam)
    st = r.scene_stats()
    assert st["bvh_tris"] == 100352 and st["scene_bvh"] == 0 and st["tree_depth"] <= 20
    o, d = random_rays(np.random.default_rng(3), 40000, np.zeros(3), 4.0)
    t, obj, nrm = r.get_closest_hit(o, d)
    orc = _oracle(scene)
    te, obje, nrme = orc.intersect(o.astype(np.float32), d.astype(np.float32), robust=1)
    same = obj == obje
    assert same.mean() > 0.999 and (obje == 0).sum() > 5000
    hit = same & (obje >= 0)
    rel = np.abs(t[hit] - te[hit]) / te[hit]
    assert np.quantile(rel, 0.999) < 2e-4                    # silhouette edges may pick the neighbouring triangle
    close = hit & (np.abs(t - te) <= 2e-4 * te)
    assert np.quantile(np.abs(nrm[close] - nrme[close]).max(axis=1), 0.999) < 5e-3
    size, spp = 64, 16
    got = r.width(size).height(size).max_bounces(cfg["max_bounces"]).seed(8).sample_array(spp)
    exp = orc.render(cam, size, size, spp, cfg["max_bounces"], seed=8, robust=1)
    assert np.all(np.isfinite(got)) and exp.mean() > 0
    assert rel_rms(got, exp) < 1e-2
    assert abs(got.mean() - exp.mean()) / exp.mean() < 5e-3


@pytest.mark.parametrize("fog", [True, False])
def test_deferred_tree_walks_do_not_depend_on_the_schedule(fog):
    """Per-mesh-tree kernels park the tree walks of a wave and run them together (kernels.hip, PH_WAIT*):
    when they start ("defer_lanes") and when the wave leaves them ("defer_stop") must not change one bit --
    every lane computes its own path in its own order -- and the frame matches the oracle.  Two meshes, two
    object lights with twins (shadow walks with an occluder range), surface and medium events."""
    import rpt_amd
    from rpt_amd import Light, Medium, Mesh
    sc = Scene()
    sc.add(Object(Mesh(scenes.bumpy_torus(40, 24)).scale(vec3(2, 2, 2)).rotate_x(0.6)).material(Material.specular(vec3(0.8, 0.6, 0.3), 0.2)))
    sc.add(Object(Mesh(scenes.bumpy_torus(24, 24)).translate(vec3(1.0, 0.8, 0.5))).material(Material.diffuse(vec3(0.3, 0.6, 0.9))))
    sc.add(Object(plane(vec3(0, 1, 0), -1.0)).material(Material.diffuse(vec3(0.8, 0.8, 0.8))))
    for pos, col in ((vec3(0.0, 3.0, 0.0), vec3(1, 1, 1)), (vec3(2.5, 1.0, 2.0), vec3(1.0, 0.5, 0.2))):
        lamp = Mesh(scenes.bumpy_torus(4, 3)).scale(vec3(0.8, 0.8, 0.8)).translate(pos)
        sc.add(Object(lamp.clone()).material(Material.light(col, 30.0)))
        sc.add(Light.Object(Object(lamp.clone()).material(Material.light(col, 30.0))))
    if fog:
        sc.add(Medium.homogeneous_isotropic(0.02, 0.1))
    cam = Camera.look_at(vec3(0.0, 1.5, 6.0), vec3(0.0, 0.0, 0.0), vec3(0, 1, 0), 0.8)
    w, h, spp = 96, 72, 24
    sc.set_option("timing", 1)
    capped = []                                                   # per render: on the grid of 37 blocks

    def render(lanes, stop, leaf_quarters=6):
        rpt_amd.set_option("defer_lanes", lanes)
        rpt_amd.set_option("defer_stop", stop)
        rpt_amd.set_option("walk_leaf_quarters", leaf_quarters)   # when a walk's descent pauses for the triangle tests
        r = Renderer(sc, cam).width(w).height(h).max_bounces(3).seed(6)
        img = r.sample_array(spp)
        st = r.scene_stats()
        assert st["bvh_nodes"] > 0 and st["scene_bvh"] == 0      # the per-mesh-tree kernel
        capped.append(r.timing()[2] == 37)
        return img
    def render_detached(lanes, trigger, stop, leaf_quarters=6):
        rpt_amd.set_option("detach_lanes", lanes)
        rpt_amd.set_option("detach_trigger", trigger)
        return render(32, stop, leaf_quarters)
    try:
        # (in fog the lamps' shadow queries leave their paths by default: here the parked form, the detached one below)
        rpt_amd.set_option("detach_shadows", 0)
        frames = [render(*v) for v in ((32, 16), (1, 1), (64, 64), (64, 1), (8, 5), (32, 16, 0), (32, 16, 1), (40, 8, 64))]
        # how many lanes wait for a new work item before the wave hands items out ("pull_batch"): lanes between items idle
        # (on a grid of 37 blocks, 11 items per lane: on the default grid every lane has one item and never waits for a second)
        rpt_amd.set_option("max_blocks", 37)
        for pb in (1, 7, 64):
            rpt_amd.set_option("pull_batch", pb)
            frames.append(render(32, 16))
        rpt_amd.set_option("pull_batch", 2)
        rpt_amd.set_option("max_blocks", 0)
        rpt_amd.set_option("detach_shadows", 1)
        # detached shadow queries (kernels.hip, DETACH): when a walk session starts (waiting + queued queries, queued alone), when
        # it is left, a queue that overflows at every vertex (trigger 32 with sessions that start late) -- not one bit
        detached = [render_detached(*v) for v in ((48, 20, 16), (1, 1, 1), (96, 32, 32), (64, 32, 1), (8, 3, 5), (48, 20, 16, 0), (96, 32, 8, 64))] if fog else []
        if fog:   # stalled lanes (answers outstanding), lanes waiting for the hand-out and the session trigger must not wait for each other
            rpt_amd.set_option("max_blocks", 37)
            for pb in (1, 9, 64):
                rpt_amd.set_option("pull_batch", pb)
                detached.append(render_detached(48, 20, 16))
            rpt_amd.set_option("pull_batch", 2)
            rpt_amd.set_option("max_blocks", 0)
        # streamed walks (DETACH = 2): primary queries leave as well, their paths wait in memory; session threshold and exit rule
        streamed = []
        have_streamed = fog
        if fog:
            try:
                rpt_amd.set_option("detach_shadows", 2)
            except RptError:   # a rejected prototype: in the library only when it is built with -DRPT_EXPERIMENTS
                have_streamed = False
        if have_streamed:
            for backlog, stop, contexts in ((128, 16, 4), (1, 1, 1), (256, 64, 6), (64, 32, 2), (200, 1, 3), (48, 16, 1)):
                rpt_amd.set_option("stream_backlog", backlog)
                rpt_amd.set_option("stream_contexts", contexts)
                streamed.append(render(32, stop))
            rpt_amd.set_option("pull_batch", 16)
            streamed.append(render(32, 16))
    finally:
        rpt_amd.set_option("max_blocks", 0)
        rpt_amd.set_option("pull_batch", 2)
        rpt_amd.set_option("detach_shadows", 1)
        rpt_amd.set_option("stream_backlog", 48)
        rpt_amd.set_option("stream_contexts", 1)
        rpt_amd.set_option("defer_lanes", 32)
        rpt_amd.set_option("defer_stop", 16)
        rpt_amd.set_option("walk_leaf_quarters", 6)
        rpt_amd.set_option("detach_lanes", 44)
        rpt_amd.set_option("detach_trigger", 28)
    n_items = 9 * 1024 * Renderer(sc, cam).chunking(spp)[1]
    assert sum(capped) == (6 if fog else 3) and not capped[0] and n_items >= 8 * 37 * 256   # the pull_batch legs: 8+ items per lane
    for f in frames[1:]:
        assert np.array_equal(frames[0], f)
    for f in detached[1:]:
        assert np.array_equal(detached[0], f)
    for f in streamed[1:]:   # streamed walks: the order in which queries are answered and paths resumed changes no bit either
        assert np.array_equal(streamed[0], f)
    exp = _oracle(sc).render(cam, w, h, spp, 3, seed=6, robust=1)
    assert np.all(np.isfinite(frames[0])) and exp.mean() > 0
    assert rel_rms(frames[0], exp) < 2e-2
    assert abs(frames[0].mean() - exp.mean()) / exp.mean() < 5e-3
    if fog:   # the same algorithm in another kernel: last bits, and the odd path whose fp32 decision falls the other way (1e-6 per decision)
        assert rel_rms(detached[0], frames[0]) < 2e-4 and abs(detached[0].mean() - frames[0].mean()) < 1e-5 * frames[0].mean()
        assert rel_rms(detached[0], exp) < 2e-2 and abs(detached[0].mean() - exp.mean()) / exp.mean() < 5e-3
        if streamed:
            assert rel_rms(streamed[0], frames[0]) < 2e-4 and abs(streamed[0].mean() - frames[0].mean()) < 1e-5 * frames[0].mean()
            assert rel_rms(streamed[0], exp) < 2e-2 and abs(streamed[0].mean() - exp.mean()) / exp.mean() < 5e-3


def test_too_deep_mesh_tree_is_rebuilt_balanced_with_the_same_hits():
    """The walk's stack holds 32 levels: a mesh tree the SAH builder makes deeper than "bvh_max_depth" is rebuilt
    with object-median splits (rpt_capi.cpp BvhBuilder::balanced).  Forced here on an ordinary mesh: shallower tree,
    identical closest hits (same triangles, same fp32 tests: bit-equal t and object, normals too except on a shared edge)."""
    import rpt_amd
    from rpt_amd import Mesh
    tris = scenes.bumpy_torus(64, 48)

    def build():
        sc = Scene()
        sc.add(Object(Mesh(tris).scale(vec3(2, 2, 2)).rotate_x(0.4)).material(Material.diffuse(vec3(1, 1, 1))))
        sc.add(Object(plane(vec3(0, 1, 0), -1.5)).material(Material.diffuse(vec3(1, 1, 1))))
        return Renderer(sc, Camera())
    o, d = random_rays(np.random.default_rng(3), 50000, np.zeros(3), 3.0)
    sah = build()
    t0, obj0, n0 = sah.get_closest_hit(o, d)
    rpt_amd.set_option("bvh_max_depth", 5)
    try:
        bal = build()
        t1, obj1, n1 = bal.get_closest_hit(o, d)
    finally:
        rpt_amd.set_option("bvh_max_depth", 20)
    d_sah, d_bal = sah.scene_stats()["tree_depth"], bal.scene_stats()["tree_depth"]
    assert 5 < d_bal < d_sah <= 20 and d_bal == 11              # 6144 triangles: ceil(log2(6144 / 4)) = 11 levels
    assert (obj0 == 0).mean() > 0.05
    assert np.array_equal(obj0, obj1) and np.array_equal(t0, t1)
    assert (np.abs(n0 - n1).max(axis=1) > 0).sum() <= 3       # an edge shared by two triangles: either may win the tie


def test_mesh_scene_without_lights_under_an_environment_colour():
    """Per-mesh-tree kernel with an empty light list (stage L has no iterations): only the environment lights
    the scene (src/renderer.rs:288), mirror and diffuse bounces up to max_bounces."""
    from rpt_amd import Environment, Mesh, sphere
    sc = Scene()
    sc.add(Object(Mesh(scenes.bumpy_torus(24, 16)).scale(vec3(2, 2, 2)).rotate_x(0.9)).material(Material.diffuse(vec3(0.7, 0.5, 0.3))))
    sc.add(Object(plane(vec3(0, 1, 0), -1.0)).material(Material.diffuse(vec3(0.8, 0.8, 0.8))))
    sc.add(Object(sphere().scale(vec3(0.5, 0.5, 0.5)).translate(vec3(1.5, -0.5, 1.0))).material(Material.mirror()))
    sc.environment = Environment.Color(vec3(0.6, 0.7, 0.9))
    cam = Camera.look_at(vec3(0.0, 1.5, 6.0), vec3(0.0, 0.0, 0.0), vec3(0, 1, 0), 0.8)
    w, h, spp = 80, 60, 32
    r = Renderer(sc, cam).width(w).height(h).max_bounces(3).seed(12)
    got = r.sample_array(spp)
    assert r.scene_stats()["bvh_nodes"] > 0 and r.scene_stats()["scene_bvh"] == 0
    exp = _oracle(sc).render(cam, w, h, spp, 3, seed=12, robust=1)
    assert np.all(np.isfinite(got)) and exp.mean() > 0.1
    assert rel_rms(got, exp) < 1e-2
    assert abs(got.mean() - exp.mean()) / exp.mean() < 3e-3


def test_cpp_mirror_example_renders_the_same_bytes_as_the_python_mirror():
    """examples/cornell.cpp (include/rpt.hpp over the C ABI) vs rpt_amd.api on the same scene/seed."""
    import os
    import subprocess
    from rpt_amd import Filter
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "examples", "cornell")
    assert os.path.exists(exe), "build() compiles examples/cornell"
    size, spp = 64, 8
    line = subprocess.check_output([exe, str(size), str(spp)], text=True).split()
    assert [int(v) for v in line[:3]] == [size, size, spp]
    scene, cam, cfg = scenes.cornell()
    seen = {}

    def cb(iteration, buffer):
        seen["img"] = buffer.image()
        seen["var"] = buffer.variance()
    Renderer(scene, cam).width(size).height(size).filter(Filter.Box(1)).max_bounces(2).num_samples(spp).seed(1) \
        .iterative_render(spp // 2, cb)
    h = 1469598103934665603
    for b in seen["img"].reshape(-1).tolist():
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    assert line[3] == f"{h:016x}"
    assert abs(float(line[4]) - seen["var"]) <= 1e-9 * seen["var"]
    # the same binary with a 4th argument also runs photon_point_query_beam_render through rpt.hpp
    ppm = os.path.join(root, "gpurun_out", "cornell_cpp.ppm")
    os.makedirs(os.path.dirname(ppm), exist_ok=True)
    subprocess.check_call([exe, "32", "2", ppm, "photon"])
    assert open(ppm, "rb").read(2) == b"P6"


# ------------------------------------------------------------------ BASELINE.json full sizes
# (config, pixels in the subset, rel-RMS bound vs the robust oracle, vs the literal oracle, bound on the mean bias vs literal)
# The last column is the known delta to rpt itself: the reference's 1e-12 shadow / t_min
# epsilons lose energy to fp64 self-hits and false shadow rejections, which the fp32 policy does not reproduce; measured
# +0.77 % (C2), +0.16 % (C3), -0.002 % (C5: small coordinates, the 1e-12 tests rarely misfire).  The bounds sit just above the measured values so that the gap cannot grow unseen.
@pytest.mark.parametrize("name,npix,tol_robust,tol_literal,bias_literal", [
    ("C2", 4096, 2e-3, 2e-2, (6.5e-3, 9.0e-3)), ("C3", 2048, 2e-3, 3e-2, (0.5e-3, 2.5e-3)), ("C5", 1024, 2e-3, 2e-3, (-5e-4, 5e-4))])
def test_full_size_configs_match_oracle_on_a_pixel_subset(name, npix, tol_robust, tol_literal, bias_literal):
    """The full BASELINE configuration (C2 512x512x64, C3 1024x1024x256, C5 2048x2048x1024 over the 100,352-triangle
    mesh) on the GPU; the fp64 oracle renders the same seed on a random pixel subset (it is ~1000x slower).  Both
    epsilon policies of the oracle are reported: `robust` is what the fp32 path implements, `literal` is the
    reference's 1e-12 policy whose fp64 rounding noise the fp32 path cannot reproduce; the mean bias against
    `literal` is asserted to stay inside the recorded interval."""
    import json
    import os
    scene, cam, cfg = scenes.CONFIGS[name]()
    w, h, spp, mb = cfg["width"], cfg["height"], cfg["spp"], cfg["max_bounces"]
    got = Renderer(scene, cam).width(w).height(h).max_bounces(mb).seed(11).sample_array(spp)
    assert np.all(np.isfinite(got)) and got.min() >= 0.0
    pix = np.sort(np.random.default_rng(5).choice(w * h, size=npix, replace=False)).astype(np.uint32)
    orc = _oracle(scene)
    rob = orc.render(cam, w, h, spp, mb, seed=11, robust=1, pixels=pix)[pix]
    lit = orc.render(cam, w, h, spp, mb, seed=11, robust=0, pixels=pix)[pix]
    e_rob, e_lit, e_orc = rel_rms(got[pix], rob), rel_rms(got[pix], lit), rel_rms(rob, lit)
    bias_rob = (got[pix].mean() - rob.mean()) / rob.mean()
    bias_lit = (got[pix].mean() - lit.mean()) / lit.mean()
    out = {"config": name, "size": [w, h, spp], "pixels": int(npix), "rel_rms_vs_robust_oracle": e_rob,
           "rel_rms_vs_literal_oracle": e_lit, "rel_rms_oracle_robust_vs_literal": e_orc,
           "mean_gpu": float(got[pix].mean()), "mean_robust": float(rob.mean()), "mean_literal": float(lit.mean()),
           "mean_bias_vs_robust": float(bias_rob), "mean_bias_vs_literal": float(bias_lit)}
    os.makedirs("gpurun_out", exist_ok=True)
    with open(f"gpurun_out/parity_full_{name}.json", "w") as f:
        json.dump(out, f, indent=1)
    print(out)
    assert e_rob < tol_robust
    assert e_lit < tol_literal
    assert abs(bias_rob) < 1e-3
    assert bias_literal[0] < bias_lit < bias_literal[1]


def test_hdri_environment_matches_oracle():
    """Environment::Hdri (src/environment.rs:3-52): spheres under an equirectangular sky, no lights;
    all radiance arrives through environment lookups on missed bounce and camera rays."""
    from rpt_amd import Camera, Environment, Material, Object, Scene, hex_color, plane, sphere, vec3
    w, h = 64, 32
    yy, xx = np.mgrid[0:h, 0:w]
    sky = np.stack([0.2 + 0.8 * xx / (w - 1), 0.3 + 0.5 * (1 - yy / (h - 1)), 0.1 + 0.9 * ((xx // 8 + yy // 8) % 2)], axis=-1)
    sc = Scene()
    sc.environment = Environment.Hdri(w, h, sky.reshape(-1, 3))
    sc.add(Object(plane(vec3(0, 1, 0), 0.0)).material(Material.diffuse(hex_color(0xCCCCCC))))
    sc.add(Object(sphere().translate(vec3(-1.2, 1, 0))).material(Material.mirror()))
    sc.add(Object(sphere().translate(vec3(1.2, 1, 0))).material(Material.specular(hex_color(0xE7A94D), 20.0)))
    cam = Camera.look_at(vec3(0, 2.0, 6.0), vec3(0, 0.8, 0), vec3(0, 1, 0), 0.7)
    size, spp, mb = 64, 16, 3
    got = Renderer(sc, cam).width(size).height(size).max_bounces(mb).seed(12).sample_array(spp)
    exp = _oracle(sc).render(cam, size, size, spp, mb, seed=12, robust=1)
    assert exp.min() > 0 and np.all(np.isfinite(got))
    assert rel_rms(got, exp) < 3e-3
    # a camera ray straight at the sky returns the bilinear texel value: compare one pixel at 1 bounce, many spp
    top = Renderer(sc, cam).width(size).height(size).max_bounces(0).seed(1).sample_array(4)
    exp_top = _oracle(sc).render(cam, size, size, 4, 0, seed=1, robust=1)
    assert np.allclose(top[:size], exp_top[:size], rtol=2e-4, atol=1e-6)       # first image row sees only sky


@pytest.mark.parametrize("name", ["C2", "C3"])
def test_item_hand_out_batches_do_not_change_the_frame(name):
    """Scan kernels: a wave hands out work items when "pull_batch" lanes wait for one (or nothing else is left to do);
    lanes between items take no part in a trip.  Which lane renders an item, and when, must not change one bit."""
    import rpt_amd
    scene, cam, cfg = scenes.CONFIGS[name]()
    scene.set_option("timing", 1)
    r = Renderer(scene, cam).width(80).height(72).max_bounces(cfg["max_bounces"]).seed(3)
    n_items = 9 * 1024 * r.chunking(40)[1]
    frames = [r.sample_array(40)]                                # the default grid: one item per lane, the hand-out never runs again
    assert n_items <= r.timing()[2] * 256
    try:
        # 37 blocks, 13 items per lane: lanes do wait for a next item, and "pull_batch" decides when they get it
        rpt_amd.set_option("max_blocks", 37)
        for pb in (1, 2, 5, 33, 64):
            rpt_amd.set_option("pull_batch", pb)
            r = Renderer(scene, cam).width(80).height(72).max_bounces(cfg["max_bounces"]).seed(3)
            frames.append(r.sample_array(40))
            assert r.timing()[2] == 37 and n_items >= 8 * 37 * 256
    finally:
        rpt_amd.set_option("pull_batch", 2)
        rpt_amd.set_option("max_blocks", 0)
    assert np.all(np.isfinite(frames[0])) and frames[0].mean() > 0
    for f in frames[1:]:
        assert np.array_equal(frames[0], f)
