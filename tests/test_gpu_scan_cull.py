"""The tail cull of the primary scans in a medium (option "scan_cull": the boxes, rectangles and triangles behind the shell are left
out when no lane of the wave has a search interval that reaches the box around them) may only leave out records that no lane could
have hit: every frame and every primary query -- parameter and hit code -- must be the same BITS with the option on and off.

  * frames: C3 on the default grid and on a capped grid (every lane renders >= 8 items, the rule of test_gpu_schedule.py), a fog
    scene whose boxes stick out of the room on two sides, a fog scene with two spheres and a triangle record;
  * counters (rpt_scan_cull_counters, counters build): on C3 the cull ran, left the tail out in some trips and not in others, and
    never with the option off; the counters build renders the same frame;
  * segments (rpt_intersect_segments, >= 200k per scene, 64 consecutive ones form a wave): random ones; ending inside the tail box;
    ending on, 1 ulp before and 1 ulp after every face of the tail box, of the bound and of every candidate group box, along the
    axis (where the end is the slab parameter itself) and obliquely; through points of the boxes' edges; axis-parallel with both
    signs of zero, also from origins that lie exactly in a face plane; starting on faces.  The special segments appear twice: packed
    64 to a wave, and each alone in a wave of 63 segments that end far from everything -- alone, its own box test decides whether
    the wave scans the tail.  No segment is left out of the comparison."""
import ctypes as C

import numpy as np
import pytest

from rpt_amd import Material, Medium, Object, Renderer, Scene, _lib, cube, polygon, scenes, sphere, vec3

pytestmark = pytest.mark.gpu

BLOCK_LANES = 256


def _fog_room():
    sc = Scene()
    white = Material.diffuse(vec3(0.7, 0.7, 0.7))
    scenes._cornell_walls(sc, white, Material.diffuse(vec3(0.7, 0.1, 0.1)), Material.diffuse(vec3(0.1, 0.7, 0.1)))
    return sc, white


def _sticks():
    """Boxes that stick out of the room through the right wall and through the floor, one inside; the light under the ceiling."""
    sc, white = _fog_room()
    sc.add(Object(cube().scale(vec3(120.0, 60.0, 80.0)).translate(vec3(556.0, 300.0, 200.0))).material(white))
    sc.add(Object(cube().scale(vec3(90.0, 150.0, 70.0)).translate(vec3(150.0, 20.0, 400.0))).material(white))
    sc.add(Object(cube().scale(vec3(60.0, 60.0, 60.0)).translate(vec3(300.0, 200.0, 300.0))).material(white))
    lamp = polygon([vec3(330.0, 548.8, 240.0), vec3(330.0, 548.8, 319.0), vec3(226.0, 548.8, 319.0), vec3(226.0, 548.8, 240.0)])
    sc.add((lamp, Material.light(vec3(1.0, 1.0, 1.0), 150.0)))
    sc.add(Medium.homogeneous_isotropic(0.00005, 0.003))
    return sc


def _spheres_and_triangle():
    """Two spheres (not in the tail), a lone triangle and the light's rectangle (the tail)."""
    sc, white = _fog_room()
    sc.add(Object(sphere().scale(vec3(80.0, 80.0, 80.0)).translate(vec3(150.0, 80.0, 400.0))).material(white))
    sc.add(Object(sphere().scale(vec3(40.0, 70.0, 40.0)).rotate_y(0.7).translate(vec3(400.0, 300.0, 150.0))).material(white))
    sc.add(Object(polygon([vec3(100.0, 400.0, 100.0), vec3(200.0, 430.0, 120.0), vec3(130.0, 450.0, 220.0)])).material(white))
    lamp = polygon([vec3(330.0, 548.8, 240.0), vec3(330.0, 548.8, 319.0), vec3(226.0, 548.8, 319.0), vec3(226.0, 548.8, 240.0)])
    sc.add((lamp, Material.light(vec3(1.0, 1.0, 1.0), 150.0)))
    sc.add(Medium.homogeneous_isotropic(0.00005, 0.003))
    return sc


def _scene(name):
    if name == "C3":
        scene, cam, cfg = scenes.CONFIGS["C3"]()
        return scene, cam, cfg["max_bounces"]
    return (_sticks() if name == "sticks" else _spheres_and_triangle()), scenes._cornell_camera(), 10


def _boxes(r):
    """(bound, groups, tail, enabled) of the committed scene."""
    boxes, masks, ng, en = (C.c_float * 36)(), (C.c_uint64 * 5)(), C.c_uint32(), C.c_uint32()
    _lib.check(_lib.load().rpt_scan_cull_groups(r.scene._commit(r.device_), boxes, masks, C.byref(ng), C.byref(en)))
    b = np.array(list(boxes), dtype=np.float32).reshape(6, 2, 3)
    return b[0], [b[1 + g] for g in range(ng.value)], b[5], en.value


def _cull_counters(r):
    out = (C.c_uint64 * 16)()
    _lib.check(_lib.load().rpt_scan_cull_counters(r.scene._handle, out))
    return [int(v) for v in out]


# ------------------------------------------------------------------ frames
@pytest.mark.parametrize("name", ["C3", "sticks", "spheres_triangle"])
def test_frames_are_bit_identical_with_the_cull_on_and_off(name):
    imgs = {}
    for on in (1, 0):
        scene, cam, bounces = _scene(name)
        scene.set_option("scan_cull", on)
        r = Renderer(scene, cam).width(64).height(64).max_bounces(bounces).seed(5)
        imgs[on] = r.sample_array(8)
        st = r.scene_stats()
        assert st["scene_bvh"] == 0 and st["bvh_nodes"] == 0            # the scan kernels are what is under test
        assert _boxes(r)[3] == on
    assert np.all(np.isfinite(imgs[1])) and imgs[1].mean() > 0
    assert np.array_equal(imgs[1], imgs[0])


def test_c3_on_a_capped_grid_every_lane_renders_many_items_and_the_frame_keeps_its_bits():
    imgs = {}
    for on, cap in ((1, 0), (1, 4), (0, 4)):
        scene, cam, bounces = _scene("C3")
        scene.set_option("scan_cull", on)
        scene.set_option("timing", 1)
        scene.set_option("max_blocks", cap)
        r = Renderer(scene, cam).width(64).height(64).max_bounces(bounces).seed(5)
        imgs[(on, cap)] = r.sample_array(8)
        if cap:
            chunk, n_chunks = r.chunking(8)
            n_items, blocks = 2 * 2 * 1024 * n_chunks, r.timing()[2]
            print(f"scan_cull {on}, max_blocks {cap}: {blocks} blocks, {n_items} items, {n_items / (blocks * BLOCK_LANES):.1f} per lane")
            assert blocks == cap and n_items >= 8 * blocks * BLOCK_LANES
    assert np.array_equal(imgs[(1, 4)], imgs[(1, 0)])
    assert np.array_equal(imgs[(1, 4)], imgs[(0, 4)])


def test_counters_on_c3_the_tail_is_left_out_in_some_trips_and_never_with_the_option_off():
    res = {}
    for on in (1, 0):
        scene, cam, bounces = _scene("C3")
        scene.set_option("scan_cull", on)
        r = Renderer(scene, cam).width(64).height(64).max_bounces(bounces).seed(5)
        plain = r.sample_array(8)
        scene.set_option("counters", 1)
        r._sample_offset = 0
        counted = r.sample_array(8)
        res[on] = (plain, counted, _cull_counters(r), r.counters())
    for on in (1, 0):
        plain, counted, c, base = res[on]
        trips = sum(c[0:5])
        print(f"scan_cull {on}: {trips} trips with a primary query, by lanes reaching the bound {c[0:5]}, groups unreached {c[5:9]}, tail left out {c[9]}")
        assert np.array_equal(plain, counted)
        assert trips > 0 and trips <= base["wave_trips"] and c[12] == 1 and c[13] == 4 and c[15] == on
        assert c[0] <= c[9] if on else c[9] == 0                        # no lane reaches the bound -> none reaches the tail
    assert 0 < res[1][2][9] < sum(res[1][2][0:5])                       # left out in some trips, scanned in others
    assert np.array_equal(res[1][0], res[0][0])


# ------------------------------------------------------------------ segments
def _unit(v):
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _segments(bound, groups, tail, rng):
    """-> origins, directions, t_max (fp32), and the number of special segments (each is there packed and alone)."""
    lo, hi = bound[0].astype(np.float64), bound[1].astype(np.float64)
    center, ext = 0.5 * (lo + hi), float(np.max(hi - lo))
    special = []

    def add(o, d, t):
        o = np.asarray(o, dtype=np.float64).reshape(-1, 3)
        d = np.broadcast_to(np.asarray(d, dtype=np.float64).reshape(-1, 3), o.shape)
        t = np.broadcast_to(np.asarray(t, dtype=np.float32).reshape(-1), (o.shape[0],))
        special.append((o.astype(np.float32), d.astype(np.float32), t.astype(np.float32)))

    def outside(n):
        return center + (0.6 + rng.uniform(0.0, 1.0, size=(n, 1))) * ext * _unit(rng.normal(size=(n, 3)))

    def ulps(t, k):
        t = np.asarray(t, dtype=np.float32)
        for _ in range(abs(k)):
            t = np.nextafter(t, np.float32(np.inf if k > 0 else -np.inf))
        return t

    k = 64
    boxes = [tail, bound] + list(groups)
    # ending inside the tail box
    p = rng.uniform(tail[0], tail[1], size=(8 * k, 3))
    o = outside(8 * k)
    add(o, _unit(p - o), np.linalg.norm(p - o, axis=1))
    for b in boxes:
        blo, bhi = b[0].astype(np.float64), b[1].astype(np.float64)
        for axis in range(3):
            for side, plane in ((0, b[0][axis]), (1, b[1][axis])):
                sign = 1.0 if side == 0 else -1.0          # travelling towards the face from outside
                # along the axis: the end is the slab parameter (plane - o) * (+-1) itself, so +-1 ulp straddles the decision
                p = rng.uniform(blo, bhi, size=(k, 3))
                o32 = p.astype(np.float32)
                o32[:, axis] = np.float32(plane) - np.float32(sign) * rng.uniform(1.0, ext, size=k).astype(np.float32)
                d = np.zeros((k, 3))
                d[:, axis] = sign
                t = ((np.float32(plane) - o32[:, axis]) * np.float32(sign)).astype(np.float32)
                for u in (-1, 0, 1):
                    add(o32, d, ulps(t, u))
                # obliquely: the end a few ulp around the distance to a point of the face
                p = rng.uniform(blo, bhi, size=(k, 3))
                p[:, axis] = plane
                o = p - sign * np.abs(rng.normal(size=(k, 3)) * ext * 0.5) * np.eye(3)[axis] + rng.normal(size=(k, 3)) * ext * 0.2 * (1 - np.eye(3)[axis])
                dist = np.linalg.norm(p - o, axis=1).astype(np.float32)
                for u in (-4, -1, 0, 1, 4):
                    add(o, _unit(p - o), ulps(dist, u))
                # starting on the face, any direction
                add(p.astype(np.float32), _unit(rng.normal(size=(k, 3))), rng.exponential(300.0, size=k))
                # ... and parallel to it from a point of its plane, with both signs of zero
                for zero in (0.0, -0.0):
                    d = rng.normal(size=(k, 3))
                    d[:, axis] = zero
                    q = outside(k)
                    q[:, axis] = plane
                    add(q, _unit(d), np.float32(np.inf))
                    add(p, _unit(d), np.float32(np.inf))
        # through points of the edges
        e = rng.uniform(blo, bhi, size=(4 * k, 3))
        ax = rng.integers(0, 3, 4 * k)
        e[np.arange(4 * k), ax] = np.where(rng.integers(0, 2, 4 * k) == 0, blo[ax], bhi[ax])
        a2 = (ax + 1) % 3
        e[np.arange(4 * k), a2] = np.where(rng.integers(0, 2, 4 * k) == 0, blo[a2], bhi[a2])
        o = outside(4 * k)
        add(o, _unit(e - o), np.float32(np.inf))
        add(o, _unit(e - o), np.linalg.norm(e - o, axis=1))
    # axis-parallel with one and two zero components, +0 and -0
    for zero in (0.0, -0.0):
        for axis in range(3):
            d = rng.normal(size=(2 * k, 3))
            d[:, axis] = zero
            add(center + rng.uniform(-0.7, 0.7, size=(2 * k, 3)) * ext, _unit(d), rng.exponential(300.0, size=2 * k))
            for sign in (1.0, -1.0):
                d = np.full((2 * k, 3), zero)
                d[:, axis] = sign
                add(center + rng.uniform(-0.7, 0.7, size=(2 * k, 3)) * ext, d, np.float32(np.inf))
    so, sd, st = (np.concatenate([s[i] for s in special]) for i in range(3))
    n_special = so.shape[0]
    # random segments: from around the scene and from inside it, ends exponential (a third without end)
    n = 1 << 16
    ro = np.concatenate([outside(n // 2), center + rng.uniform(-0.5, 0.5, size=(n // 2, 3)) * (hi - lo)])
    rd = _unit(np.concatenate([center + rng.uniform(-0.5, 0.5, size=(n // 2, 3)) * ext - ro[:n // 2], rng.normal(size=(n // 2, 3))]))
    rt = np.where(rng.uniform(size=n) < 0.33, np.inf, rng.exponential(300.0, size=n))
    # every special segment alone: lane 0 of a wave whose other lanes end far from everything
    far_o = np.tile((center + np.array([0.0, 0.0, -20.0 * ext])).astype(np.float32), (64 * n_special, 1))
    far_d = np.tile(np.array([0.0, 0.0, -1.0], dtype=np.float32), (64 * n_special, 1))
    far_t = np.full(64 * n_special, 1.0, dtype=np.float32)
    far_o[::64], far_d[::64], far_t[::64] = so, sd, st
    o = np.concatenate([so, ro.astype(np.float32), far_o])
    d = np.concatenate([sd, rd.astype(np.float32), far_d])
    t = np.concatenate([st, rt.astype(np.float32), far_t])
    return np.ascontiguousarray(o), np.ascontiguousarray(d), np.ascontiguousarray(t), n_special


def _query(r, o, d, tmax):
    n = o.shape[0]
    t, code = np.empty(n, dtype=np.float32), np.empty(n, dtype=np.uint32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    _lib.check(_lib.load().rpt_intersect_segments(r.scene._commit(r.device_), n, p(o), p(d), p(tmax), p(t), p(code)))
    return t, code


@pytest.mark.parametrize("name", ["C3", "sticks", "spheres_triangle"])
def test_primary_queries_are_bit_equal_with_the_cull_on_and_off(name):
    res, segs = {}, None
    for on in (1, 0):
        scene, cam, _ = _scene(name)
        scene.set_option("scan_cull", on)
        r = Renderer(scene, cam)
        bound, groups, tail, enabled = _boxes(r)
        assert enabled == on and len(groups) >= 1
        if segs is None:
            segs = _segments(bound, groups, tail, np.random.default_rng(2026))
        res[on] = _query(r, *segs[:3])
    o, d, tmax, n_special = segs
    (t1, c1), (t0, c0) = res[1], res[0]
    n = o.shape[0]
    assert n >= 200_000 and t0.shape == (n,) and t1.shape == (n,)
    hit = c0 != 0xFFFFFFFF
    kinds = sorted(set((c0[hit] >> 28).tolist()))
    alone = slice(n - 64 * n_special, n, 64)
    print(f"{name}: {n} segments ({n_special} special ones, packed and alone), {int(hit.sum())} hits, kinds hit {kinds}; "
          f"alone: {int(hit[alone].sum())} hits, {int((~hit[alone]).sum())} misses")
    assert np.array_equal(t0[~hit].view(np.uint32), tmax[~hit].view(np.uint32))       # a miss leaves the end where it was
    assert any(kd in kinds for kd in (3, 5, 6)), "no tail record was hit"               # K_TRI, K_AABB, K_RECT
    assert hit[alone].sum() > n_special // 20 and (~hit[alone]).sum() > n_special // 20
    assert np.array_equal(c1, c0)
    assert np.array_equal(t1.view(np.uint32), t0.view(np.uint32))
