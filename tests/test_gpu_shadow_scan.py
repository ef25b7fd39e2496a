"""The shadow form of the linear scan (option "shadow_scan": the shadow query of an object light keeps one bit, "the closest hit is a
record of the light's twin", instead of the hit code) must decide every shadow test as the closest-hit scan does.

rpt_debug_shadow_test runs the scan kernels' own shadow query and light decision, one segment per lane.  For every scene below its
answers -- the decision and the closest hit's t -- are the same BITS with the option on and off, and both are the decision that
stage_light_term's rule gives in numpy from the closest hit (t, code) of rpt_intersect_segments over [t_min, dist (1 + 1e-3)):
the hit is a twin record and t >= dist (1 - 1e-3).  No segment is left out of the comparison.

Scenes: C3, C2, a sphere light with its twin, a tilted two-triangle light whose twin is two triangle records (segments through the
shared diagonal), two tie scenes -- a box whose bottom face lies exactly in the light rectangle's plane (the box is scanned first:
the tie goes to the box, the light is not visible there) and a triangle record coplanar with the rectangle (scanned after it) --, a
scene with two object lights, and three lights that keep the closest-hit scan: a group light, a light whose twin is a face of the
room shell, and any light with the option off.

Segments (64 consecutive ones form a wave), >= 10^5 per scene: random ones; aimed at points on the light, from points in the room and
from points ON surfaces (the hit points of camera-like rays), with the sampler's own (wi, dist), with dist scaled by 1 +- 1e-3, and
with dist 0, +-1, +-2 ulp around both thresholds (hit_t / (1 + 1e-3) and hit_t / (1 - 1e-3)); axis-parallel directions with both
signs of zero.  Every special segment is there twice: packed 64 to a wave, and alone in a wave of 63 segments far from everything.

Frames: shadow_scan on = off at 64 x 64 x 8 spp on C3 and C2, and on a grid capped with max_blocks so that lanes take >= 8 items."""
import ctypes as C

import numpy as np
import pytest

from rpt_amd import KdTree, Light, Material, Medium, Object, Renderer, Scene, _lib, cube, polygon, scenes, sphere, vec3

pytestmark = pytest.mark.gpu

BLOCK_LANES = 256
MISS = 0xFFFFFFFF
K_TRI, K_AABB, K_RECT = 3, 5, 6
ONE_PLUS, ONE_MINUS = np.float32(1.0) + np.float32(1e-3), np.float32(1.0) - np.float32(1e-3)   # the kernels' 1.f +- 1e-3f
LAMP = [vec3(330.0, 548.8, 240.0), vec3(330.0, 548.8, 319.0), vec3(226.0, 548.8, 319.0), vec3(226.0, 548.8, 240.0)]


# ------------------------------------------------------------------ scenes
def _room():
    sc = Scene()
    white = Material.diffuse(vec3(0.7, 0.7, 0.7))
    scenes._cornell_walls(sc, white, Material.diffuse(vec3(0.7, 0.1, 0.1)), Material.diffuse(vec3(0.1, 0.7, 0.1)))
    return sc, white


def _lamp_mtl():
    return Material.light(vec3(1.0, 1.0, 1.0), 150.0)


def _sphere_light():
    sc, white = _room()
    sc.add(Object(sphere().scale(vec3(70.0, 70.0, 70.0)).translate(vec3(150.0, 70.0, 400.0))).material(white))
    sc.add(Object(cube().scale(vec3(90.0, 150.0, 70.0)).rotate_y(0.4).translate(vec3(400.0, 75.0, 200.0))).material(white))
    lamp = sphere().scale(vec3(40.0, 60.0, 40.0)).rotate_y(0.7).translate(vec3(300.0, 400.0, 300.0))
    sc.add(Object(lamp).material(_lamp_mtl()))
    sc.add(Light.Object(Object(lamp).material(_lamp_mtl())))
    sc.add(Object(cube().scale(vec3(60.0, 60.0, 60.0)).translate(vec3(200.0, 300.0, 250.0))).material(white))   # a box: scanned after the spheres
    return sc


TILTED = [np.array(p) for p in ([330.0, 500.0, 240.0], [330.0, 540.0, 319.0], [226.0, 530.0, 319.0], [226.0, 490.0, 240.0])]


def _two_triangle_light():
    """A tilted quadrilateral: two triangle records (not a rectangle record), the twin range has two entries."""
    sc, white = _room()
    sc.add(Object(polygon([vec3(100.0, 300.0, 100.0), vec3(200.0, 330.0, 120.0), vec3(130.0, 350.0, 220.0)])).material(white))   # a triangle before the twin
    sc.add((polygon([vec3(*p) for p in TILTED]), _lamp_mtl()))
    sc.add(Object(polygon([vec3(300.0, 200.0, 300.0), vec3(420.0, 230.0, 320.0), vec3(330.0, 250.0, 420.0)])).material(white))   # ... and one behind it
    sc.add(Object(cube().scale(vec3(60.0, 60.0, 60.0)).translate(vec3(250.0, 380.0, 280.0))).material(white))
    return sc


def _tie_box():
    """A box whose bottom face lies in the plane of the light's rectangle (y = 548.8) over half of it."""
    sc, white = _room()
    sc.add(Object(cube().scale(vec3(60.0, 40.0, 200.0)).translate(vec3(300.0, 568.8, 280.0))).material(white))   # y from 548.8 to 588.8, x from 270 to 330
    sc.add((polygon(LAMP), _lamp_mtl()))
    return sc


def _tie_triangle():
    """A triangle record in the plane of the light's rectangle, overlapping it."""
    sc, white = _room()
    sc.add((polygon(LAMP), _lamp_mtl()))
    sc.add(Object(polygon([vec3(200.0, 548.8, 200.0), vec3(400.0, 548.8, 260.0), vec3(260.0, 548.8, 400.0)])).material(white))
    return sc


def _two_lights():
    sc, white = _room()
    sc.add(Object(cube().scale(vec3(120.0, 200.0, 120.0)).rotate_y(0.3).translate(vec3(380.0, 100.0, 300.0))).material(white))
    sc.add((polygon(LAMP), _lamp_mtl()))
    lamp = sphere().scale(vec3(30.0, 30.0, 30.0)).translate(vec3(120.0, 300.0, 200.0))
    sc.add(Object(lamp).material(_lamp_mtl()))
    sc.add(Light.Object(Object(lamp).material(_lamp_mtl())))
    sc.add(Light.Ambient(vec3(0.02, 0.02, 0.02)))
    return sc


def _group_light():
    sc, white = _room()
    sc.add(Object(cube().scale(vec3(90.0, 150.0, 70.0)).translate(vec3(400.0, 75.0, 200.0))).material(white))
    lamp = KdTree([sphere().scale(vec3(40.0, 40.0, 40.0)).translate(vec3(200.0, 400.0, 300.0)),
                   cube().scale(vec3(50.0, 30.0, 50.0)).rotate_y(0.5).translate(vec3(330.0, 420.0, 250.0))])
    sc.add(Object(lamp).material(_lamp_mtl()))
    sc.add(Light.Object(Object(lamp).material(_lamp_mtl())))
    return sc


def _ceiling_light():
    """The light is the whole ceiling: its twin is a face of the room shell."""
    sc = Scene()
    white = Material.diffuse(vec3(0.7, 0.7, 0.7))
    floor = polygon([vec3(0.0, 0.0, 0.0), vec3(0.0, 0.0, 559.2), vec3(556.0, 0.0, 559.2), vec3(556.0, 0.0, 0.0)])
    ceiling = polygon([vec3(0.0, 548.9, 0.0), vec3(556.0, 548.9, 0.0), vec3(556.0, 548.9, 559.2), vec3(0.0, 548.9, 559.2)])
    back = polygon([vec3(0.0, 0.0, 559.2), vec3(0.0, 548.9, 559.2), vec3(556.0, 548.9, 559.2), vec3(556.0, 0.0, 559.2)])
    right = polygon([vec3(0.0, 0.0, 0.0), vec3(0.0, 548.9, 0.0), vec3(0.0, 548.9, 559.2), vec3(0.0, 0.0, 559.2)])
    left = polygon([vec3(556.0, 0.0, 0.0), vec3(556.0, 0.0, 559.2), vec3(556.0, 548.9, 559.2), vec3(556.0, 548.9, 0.0)])
    for p in (floor, back, left, right):
        sc.add(Object(p).material(white))
    sc.add((ceiling, Material.light(vec3(1.0, 1.0, 1.0), 2.0)))
    sc.add(Object(cube().scale(vec3(120.0, 200.0, 120.0)).rotate_y(0.3).translate(vec3(380.0, 100.0, 300.0))).material(white))
    return sc


SCENES = {
    "C3": lambda: scenes.CONFIGS["C3"]()[0],
    "C2": lambda: scenes.CONFIGS["C2"]()[0],
    "sphere_light": _sphere_light,
    "two_triangle_light": _two_triangle_light,
    "tie_box": _tie_box,
    "tie_triangle": _tie_triangle,
    "two_lights": _two_lights,
    "group_light": _group_light,
    "ceiling_light": _ceiling_light,
}
KEEP_THE_CLOSEST_HIT_SCAN = ("group_light", "ceiling_light")
ROOM_LO, ROOM_HI = np.array([0.0, 0.0, 0.0]), np.array([556.0, 548.9, 559.2])


def _object_lights(scene):
    return [i for i, l in enumerate(scene.lights) if l.kind == Light.OBJECT]


# ------------------------------------------------------------------ the hooks
def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def _closest(r, o, d, tmax):
    n = o.shape[0]
    t, code = np.empty(n, dtype=np.float32), np.empty(n, dtype=np.uint32)
    _lib.check(_lib.load().rpt_intersect_segments(r.scene._commit(r.device_), n, _vp(o), _vp(d), _vp(tmax), _vp(t), _vp(code)))
    return t, code


def _code_objects(r, rng):
    """hit code -> object index, from rays that both queries answer (only a light without a code range needs it)."""
    n = 1 << 16
    o = rng.uniform(ROOM_LO + 1.0, ROOM_HI - 1.0, size=(n, 3)).astype(np.float32)
    d = _unit(rng.normal(size=(n, 3))).astype(np.float32)
    _, code = _closest(r, o, d, np.full(n, np.inf, dtype=np.float32))
    _, obj, _ = r.get_closest_hit(o, d)
    table = {}
    for c, ob in zip(code.tolist(), obj.tolist()):
        assert table.setdefault(c, ob) == ob
    return table


def _reference(r, light, o, d, dist, rng):
    """stage_light_term's rule on the closest hit of the segment [t_min, dist (1 + 1e-3))."""
    t, code = _closest(r, o, d, (dist * ONE_PLUS).astype(np.float32))
    info = r.shadow_scan_info(light)
    if info["twin_lo"] <= info["twin_hi"]:
        twin = (code >= info["twin_lo"]) & (code <= info["twin_hi"])
    else:
        table = _code_objects(r, rng)
        seen = set(np.unique(code).tolist()) - {MISS}
        assert seen <= set(table), "a hit code the table of random rays does not know"
        twin = np.array([c != MISS and table[c] == info["twin_object"] for c in code.tolist()])
    flag = (code != MISS) & (t >= (dist * ONE_MINUS).astype(np.float32)) & twin
    return flag.astype(np.int32), t, code


# ------------------------------------------------------------------ segments
def _unit(v):
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _ulps(x, k):
    x = np.asarray(x, dtype=np.float32).copy()
    for _ in range(abs(k)):
        x = np.nextafter(x, np.float32(np.inf if k > 0 else -np.inf))
    return x


def _segments(r, light, rng, extra_targets=None):
    """-> origins, directions, dist (fp32), the number of special segments (each is there packed and alone)."""
    special = []

    def add(o, d, dist):
        o = np.asarray(o, dtype=np.float32).reshape(-1, 3)
        special.append((o, np.asarray(d, dtype=np.float32).reshape(-1, 3), np.broadcast_to(np.asarray(dist, dtype=np.float32).reshape(-1), (o.shape[0],))))

    k = 512
    # points in the room and points ON surfaces: where camera-like rays land (fp32 hit points, as the kernels form them)
    inside = rng.uniform(ROOM_LO + 2.0, ROOM_HI - 2.0, size=(k, 3)).astype(np.float32)
    co = np.tile(np.array([278.0, 273.0, -800.0], dtype=np.float32), (k, 1))
    cd = _unit(np.stack([rng.uniform(-0.33, 0.33, k), rng.uniform(-0.33, 0.33, k), np.ones(k)], 1)).astype(np.float32)
    ct, cobj, _ = r.get_closest_hit(co, cd)
    on_faces = (co + ct[:, None] * cd)[cobj >= 0].astype(np.float32)
    assert on_faces.shape[0] > k // 2
    for pos in (inside, on_faces):
        s = r.debug_light_sample(light, pos, seed=int(rng.integers(1 << 30)))
        wi, dist = s["wi"], s["dist"]
        add(pos, wi, dist)
        add(pos, wi, dist * ONE_PLUS)
        add(pos, wi, dist * ONE_MINUS)
        # where the segment meets the light (if it does): dist around both thresholds of that hit
        flag, t = r.debug_shadow_test(light, pos, wi, dist)
        lit = flag != 0
        for scale in (ONE_PLUS, ONE_MINUS):
            base = (t[lit] / scale).astype(np.float32)
            for u in (-2, -1, 0, 1, 2):
                add(pos[lit], wi[lit], _ulps(base, u))
    if extra_targets is not None:   # aimed at given points of the light
        o = rng.uniform(ROOM_LO + 2.0, ROOM_HI - 2.0, size=(extra_targets.shape[0], 3))
        d = extra_targets - o
        dist = np.linalg.norm(d, axis=1).astype(np.float32)
        for u in (-1, 0, 1):
            add(o, _unit(d), _ulps(dist, u))
    # axis-parallel: one and two zero components, +0 and -0; long enough to reach the ceiling from anywhere
    for zero in (0.0, -0.0):
        for axis in range(3):
            d = rng.normal(size=(64, 3))
            d[:, axis] = zero
            add(rng.uniform(ROOM_LO + 2.0, ROOM_HI - 2.0, size=(64, 3)), _unit(d), rng.uniform(10.0, 700.0, size=64))
            for sign in (1.0, -1.0):
                d = np.full((64, 3), zero)
                d[:, axis] = sign
                o = rng.uniform(ROOM_LO + 2.0, ROOM_HI - 2.0, size=(64, 3)).astype(np.float32)
                add(o, d, rng.uniform(10.0, 700.0, size=64))
                # ... straight up under the lamp, dist the distance to its plane (the slab parameter itself) and 1 ulp around it
                if axis == 1 and sign > 0:
                    o = o.copy()
                    o[:, 0], o[:, 2] = rng.uniform(228.0, 328.0, 64), rng.uniform(242.0, 317.0, 64)
                    for u in (-1, 0, 1):
                        add(o, d, _ulps(np.float32(548.8) - o[:, 1], u))
    so, sd, sdist = (np.concatenate([s[i] for s in special]) for i in range(3))
    n_special = so.shape[0]
    # random segments
    n = 1 << 15
    ro = rng.uniform(ROOM_LO + 1.0, ROOM_HI - 1.0, size=(n, 3)).astype(np.float32)
    rd = _unit(rng.normal(size=(n, 3))).astype(np.float32)
    rdist = rng.exponential(300.0, size=n).astype(np.float32)
    # every special segment alone: lane 0 of a wave whose other lanes are far from everything
    far_o = np.tile(np.array([278.0, 273.0, -20000.0], dtype=np.float32), (64 * n_special, 1))
    far_d = np.tile(np.array([0.0, 0.0, -1.0], dtype=np.float32), (64 * n_special, 1))
    far_dist = np.full(64 * n_special, 1.0, dtype=np.float32)
    far_o[::64], far_d[::64], far_dist[::64] = so, sd, sdist
    o = np.concatenate([so, ro, far_o])
    d = np.concatenate([sd, rd, far_d])
    dist = np.concatenate([sdist, rdist, far_dist])
    return np.ascontiguousarray(o), np.ascontiguousarray(d), np.ascontiguousarray(dist), n_special


def _diagonal_points(rng):
    """Points of the diagonal the two triangles of the tilted light share (polygon() fans from the first corner: v0 - v2)."""
    s = rng.uniform(0.02, 0.98, size=(256, 1))
    return TILTED[0] + s * (TILTED[2] - TILTED[0])


@pytest.mark.parametrize("name", list(SCENES))
def test_decisions_are_bit_equal_on_and_off_and_follow_the_closest_hit(name):
    res, segs = {}, {}
    for on in (1, 0):
        scene = SCENES[name]()
        scene.set_option("shadow_scan", on)
        r = Renderer(scene, scenes._cornell_camera())
        st = r.scene_stats()
        assert st["scene_bvh"] == 0 and st["bvh_nodes"] == 0            # the scan kernels are what is under test
        lights = _object_lights(scene)
        assert len(lights) == (2 if name == "two_lights" else 1)
        for li in lights:
            info = r.shadow_scan_info(li)
            assert info["twin_object"] >= 0
            assert info["shadow_form"] == (1 if on and name not in KEEP_THE_CLOSEST_HIT_SCAN else 0), info
            if li not in segs:
                extra = _diagonal_points(np.random.default_rng(3)) if name == "two_triangle_light" else None
                segs[li] = _segments(r, li, np.random.default_rng(2027 + li), extra)
            o, d, dist, n_special = segs[li]
            flag, t = r.debug_shadow_test(li, o, d, dist)
            ref = _reference(r, li, o, d, dist, np.random.default_rng(5)) if on else None
            res[(on, li)] = (flag, t, ref, info)
    for li in segs:
        o, d, dist, n_special = segs[li]
        n = o.shape[0]
        (f1, t1, (fr, tr, code), info), (f0, t0, _, _) = res[(1, li)], res[(0, li)]
        alone = slice(n - 64 * n_special, n, 64)
        hit = code != MISS
        twin_hits = hit & (fr != 0)
        ties = int((hit & ~twin_hits & (np.abs(tr - dist) <= 1e-3 * dist) & ((code >> 28) == (K_AABB if name == "tie_box" else K_TRI))).sum())
        print(f"{name} light {li}: {n} segments ({n_special} special ones, packed and alone), {int(hit.sum())} hits, visible {int(fr.sum())} "
              f"(alone: {int(fr[alone].sum())} of {n_special}), blocked within 1e-3 of the sample by a {'box' if name == 'tie_box' else 'triangle'}: {ties}; "
              f"twin codes {info['twin_lo']:#x}..{info['twin_hi']:#x}")
        assert n >= 100_000
        assert 0 < fr.sum() < n and 0 < fr[alone].sum() < n_special                 # both answers occur, also in the lone lanes
        if name == "tie_box":
            assert ties > 100                                                        # the box took the tie: hit at the sample's distance, light not visible
        if name == "two_triangle_light":
            assert info["twin_hi"] == info["twin_lo"] + 1 and (info["twin_lo"] >> 28) == K_TRI
            assert set(np.unique(code[fr != 0]).tolist()) == {info["twin_lo"], info["twin_hi"]}
        assert np.array_equal(t1.view(np.uint32), t0.view(np.uint32))
        assert np.array_equal(f1, f0)
        assert np.array_equal(t1.view(np.uint32), tr.view(np.uint32))
        assert np.array_equal(f1, fr)


# ------------------------------------------------------------------ frames
@pytest.mark.parametrize("name", ["C3", "C2"])
def test_frames_are_bit_identical_with_the_shadow_form_on_and_off(name):
    imgs = {}
    for on in (1, 0):
        scene, cam, cfg = scenes.CONFIGS[name]()
        scene.set_option("shadow_scan", on)
        r = Renderer(scene, cam).width(64).height(64).max_bounces(cfg["max_bounces"]).seed(5)
        imgs[on] = r.sample_array(8)
        assert r.shadow_scan_info(_object_lights(scene)[0])["shadow_form"] == on
    assert np.all(np.isfinite(imgs[1])) and imgs[1].mean() > 0
    assert np.array_equal(imgs[1], imgs[0])


def test_c3_on_a_capped_grid_every_lane_renders_many_items_and_the_frame_keeps_its_bits():
    imgs = {}
    for on, cap in ((1, 0), (1, 4), (0, 4)):
        scene, cam, cfg = scenes.CONFIGS["C3"]()
        scene.set_option("shadow_scan", on)
        scene.set_option("timing", 1)
        scene.set_option("max_blocks", cap)
        r = Renderer(scene, cam).width(64).height(64).max_bounces(cfg["max_bounces"]).seed(5)
        imgs[(on, cap)] = r.sample_array(8)
        if cap:
            chunk, n_chunks = r.chunking(8)
            n_items, blocks = 2 * 2 * 1024 * n_chunks, r.timing()[2]
            print(f"shadow_scan {on}, max_blocks {cap}: {blocks} blocks, {n_items} items, {n_items / (blocks * BLOCK_LANES):.1f} per lane")
            assert blocks == cap and n_items >= 8 * blocks * BLOCK_LANES
    assert np.array_equal(imgs[(1, 4)], imgs[(1, 0)])
    assert np.array_equal(imgs[(1, 4)], imgs[(0, 4)])
