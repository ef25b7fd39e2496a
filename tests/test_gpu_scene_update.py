"""Moving spheres on the device (rpt_scene_set_movable_spheres, rpt_scene_move_spheres*), against fresh commits.

The pattern throughout: a committed scene A is moved to centres X; a fresh scene B is built at X with the same options; the two are
compared -- the bytes of every array an update touches (rpt_debug_scene_records), closest hits on structured rays (the forms of
tests/ray_cloud.py: axis rays with signed zeros, rays at the centres, cones just inside and just outside every silhouette, and a
cloud), frames and feature planes.  Scanned scenes in both modes must agree in every byte.  A scene tree is refitted, not rebuilt: its
node boxes must be the union restated in numpy (tests/scene_update_ref.py) from the downloaded leaves, and its hits and frames those
of B; a ray on which they differ counts as undecided only if B itself differs there from a commit without a tree (at most 1 in
1,000).  Also the motion table, the ordering against queued renders on two streams, the stale photon map, the display positions that
stay on the device, and three frames of the live sequences end to end against the generator path."""
import math

import numpy as np
import pytest

from rpt_amd import Camera, Environment, Light, Material, Object, Renderer, RptError, Scene, hex_color, polygon, plane, scenes, sphere, vec3
from rpt_amd.api import TemporalParams, temporal_motion_record
from rpt_amd.ode import MarblesSystem, ParticleEnsemble, ParticleSimulator
from tests import scene_update_ref as ref
from tests.ray_cloud import _axis_rays, _unit

pytestmark = pytest.mark.gpu

W, H, SPP = 32, 24, 4
CAM = Camera.look_at(vec3(2.0, 2.5, 11.0), vec3(2.0, 1.5, 2.0), vec3(0.0, 1.0, 0.0), math.pi / 3.5)


def same(a, b):
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()


def grid(n, seed, jitter=0.25):
    """n centres a unit apart on a cubic grid, jittered: spheres of radius <= 0.22 stay at least 0.06 apart."""
    rng = np.random.default_rng(seed)
    side = int(math.ceil(n ** (1.0 / 3.0)))
    base = np.array([[i % side, (i // side) % side, i // (side * side)] for i in range(n)], dtype=np.float64)
    return base + rng.uniform(-jitter, jitter, (n, 3))


def radius(i):
    return 0.2 * (1.0 + 0.01 * (i % 7))


def build(centres, eps=False, ground="floor", options=(), lamp=True):
    """The ground, the twin of the sphere light (a sphere record that never moves), then the spheres: objects sc.first .. sc.first + n - 1,
    so that the last objects of a scene are movable ones."""
    sc = Scene()
    sc.environment = Environment.Color(vec3(0.6, 0.65, 0.7))
    if eps:
        sc.set_option("epsilon_policy", 1)
    for name, value in options:
        sc.set_option(name, value)
    if ground == "floor":
        sc.add(Object(polygon([vec3(30.0, -1.0, 30.0), vec3(30.0, -1.0, -30.0), vec3(-30.0, -1.0, -30.0), vec3(-30.0, -1.0, 30.0)])).material(Material.diffuse(hex_color(0xAAAAAA))))
    elif ground == "plane":
        sc.add(Object(plane(vec3(0.0, 1.0, 0.0), -1.0)).material(Material.diffuse(hex_color(0xAAAAAA))))
    if lamp:
        for add in (lambda o: sc.add(o), lambda o: sc.add(Light.Object(o))):
            add(Object(sphere().scale(vec3(1.5, 1.5, 1.5)).translate(vec3(2.0, 9.0, 2.0))).material(Material.light(hex_color(0xFFFFFF), 15.0)))
    sc.first = len(sc.objects)
    colors = [0x264653, 0x2A9D8F, 0xE9C46A, 0xF4A261, 0xE76F51]
    for i, c in enumerate(np.asarray(centres, dtype=np.float64).reshape(-1, 3)):
        r = radius(i)
        sc.add(Object(sphere().scale(vec3(r, r, r)).translate(vec3(*c))).material(Material.specular(hex_color(colors[i % 5]), 0.1)))
    return sc


def every(sc, n):
    return list(range(sc.first, sc.first + n))


def renderer(sc, cam=None):
    return Renderer(sc, cam or CAM).width(W).height(H).max_bounces(3).seed(5)


def rays(centres, seed=3):
    """A few thousand structured rays about the spheres at `centres` (fp64; every direction of unit length)."""
    c = np.asarray(centres, dtype=np.float64).reshape(-1, 3)
    rng = np.random.default_rng(seed)
    o, d = [], []
    for axis in range(3):
        for sense, zero in ((1.0, 0.0), (-1.0, -0.0)):
            ao, ad = _axis_rays(c, axis, sense, zero)       # through the centres along an axis, the other components +-0
            o.append(ao * 3.0)                              # (the helper starts at 4.9: outside this scene)
            d.append(ad)
            o[-1][:, [(axis + 1) % 3, (axis + 2) % 3]] = c[:, [(axis + 1) % 3, (axis + 2) % 3]]
    eye = np.array([2.0, 2.5, 11.0])
    o.append(np.broadcast_to(eye, c.shape).copy())
    d.append(_unit(c - eye))                                # at every centre
    for factor in (0.999, 1.001):                           # cones just inside / outside every silhouette
        for k, ck in enumerate(c):
            e = eye - ck
            dist = np.linalg.norm(e)
            ax = -e / dist
            theta = factor * math.asin(radius(k) / dist)
            u = _unit(np.cross(ax, [0.0, 1.0, 0.0]))
            v = np.cross(ax, u)
            phi = np.arange(6) * (2 * math.pi / 6) + 0.003 + k
            d.append(_unit(math.cos(theta) * ax + math.sin(theta) * (np.cos(phi)[:, None] * u + np.sin(phi)[:, None] * v)))
            o.append(np.broadcast_to(eye, (6, 3)).copy())
    n = 1500
    o.append(rng.uniform(-2.0, 6.0, (n, 3)))
    d.append(_unit(rng.normal(size=(n, 3))))
    return np.concatenate(o), np.concatenate(d)


def hits(sc, o, d, eps, cam=None):
    r = renderer(sc, cam)
    return r.get_closest_hit_f64(o, d) if eps else r.get_closest_hit(o, d)


def frame_and_planes(sc, cam=None):
    r = renderer(sc, cam)
    planes = r.features_array(SPP, sample_offset=0)
    return (r.sample_array(SPP),) + tuple(planes[k] for k in ("albedo", "normal", "depth"))


def arrays(sc, eps):
    which = [ref.SPH, ref.SPH_SHADE, ref.PBOX] + ([ref.RECS, ref.SHADE, ref.CULLS, ref.CULL32] if eps else [])
    sc._commit(0)
    return [sc.debug_records(w) for w in which]


def assert_same_scene(a, b, eps, o, d, frames=True):
    for k, (x, y) in enumerate(zip(arrays(a, eps), arrays(b, eps))):
        assert len(x) and same(x, y), f"array {k} differs"
    for k, (x, y) in enumerate(zip(hits(a, o, d, eps), hits(b, o, d, eps))):
        assert same(x, y), f"hits: output {k} differs on {int((np.asarray(x) != np.asarray(y)).sum())} values"
    if frames:
        for k, (x, y) in enumerate(zip(frame_and_planes(a), frame_and_planes(b))):
            assert np.isfinite(x).all() and same(x, y), f"frame / plane {k} differs"


# ---- records: every list form, every size, both modes
@pytest.mark.parametrize("eps", [False, True], ids=["fp32", "epsilon"])
@pytest.mark.parametrize("n,ground,lamp,lists", [(1, None, False, ("all",)), (3, "plane", True, ("all", "last", "none")), (31, "plane", True, ("all", "last")),
                                                 (63, "plane", True, ("all", "last"))])
def test_records_of_a_moved_scene_equal_a_fresh_commit(n, ground, lamp, lists, eps):
    """1 sphere alone; 3 spheres and a plane; 33 and 65 objects: the last object is a movable sphere beyond a cull32 group boundary."""
    x0, x1 = grid(n, 1), grid(n, 2)
    for form in lists:
        a = build(x0, eps, ground, lamp=lamp)
        listed = {"all": every(a, n), "last": [a.first + n - 1], "none": []}[form]
        a.set_movable_spheres(listed)
        rows = [k - a.first for k in listed]
        want = x0.copy()
        want[rows] = x1[rows]
        a.move_spheres(want[rows])
        b = build(want, eps, ground, lamp=lamp)
        b._commit(0)
        assert len(a.objects) == n + a.first
        for k, (x, y) in enumerate(zip(arrays(a, eps), arrays(b, eps))):
            assert len(x) and same(x, y), (form, k)
        info = a.movable_info()
        assert info["spheres"] == len(listed) and info["moves"] == (1 if listed else 0) and info["epsilon"] == int(eps)
        if eps:
            assert info["cull32_groups"] == len({k // 32 for k in listed})
            if form == "all" and n >= 31:
                assert info["cull32_groups"] == (n + 2 + 31) // 32 >= 2
        a.close()
        b.close()


@pytest.mark.parametrize("eps", [False, True], ids=["fp32", "epsilon"])
@pytest.mark.parametrize("form", ["all", "last", "none"])
def test_the_marble_scene_moved_equals_the_marble_scene_committed(form, eps):
    x0 = scenes.marbles_initial().pos * np.array([1.0, 0.1, 1.0])
    x1 = x0 + np.random.default_rng(4).uniform(-0.05, 0.05, x0.shape)
    listed = {"all": list(range(1, 26)), "last": [25], "none": []}[form]
    rows = [k - 1 for k in listed]
    want = x0.copy()
    want[rows] = x1[rows]
    a, cam, _ = scenes.marbles(x0)
    b, _, _ = scenes.marbles(want)
    if eps:
        a.set_option("epsilon_policy", 1)
        b.set_option("epsilon_policy", 1)
    a.set_movable_spheres(listed)
    a.move_spheres(want[rows])
    for k, (x, y) in enumerate(zip(arrays(a, eps), arrays(b, eps))):
        assert len(x) and same(x, y), k
    ra, rb = (Renderer(s, cam).width(W).height(H).max_bounces(4).seed(2) for s in (a, b))
    assert same(ra.sample_array(SPP), rb.sample_array(SPP))
    a.close()
    b.close()


# ---- the motion table
def test_motion_table_is_rpt_temporal_motion_record_per_object():
    n = 9
    x0, x1 = grid(n, 5), grid(n, 6)
    a = build(x0, False, "floor")
    f = a.first
    listed = [f, f + 1, f + 2, f + 4, f + 7]
    a.set_movable_spheres(listed)
    target = x1[[k - f for k in listed]]
    target[2] = x0[2]                                   # sphere 2 moves onto its own place
    table = a.move_spheres(target, motion=True)
    assert table.shape == (n + f, 24)
    for o in range(n + f):
        if o in listed:
            k = o - f
            want = temporal_motion_record(ref.matrix(radius(k), target[listed.index(o)]), ref.matrix(radius(k), x0[k]))
        else:
            want = ref.IDENTITY_RECORD
        assert same(table[o], np.asarray(want).reshape(-1)), o
    assert same(table[f + 2], ref.IDENTITY_RECORD) and not same(table[f], ref.IDENTITY_RECORD)
    # a second move: the previous centre is the first move's
    table2 = a.move_spheres(x0[[k - f for k in listed]], motion=True)
    assert same(table2[f], np.asarray(temporal_motion_record(ref.matrix(radius(0), x0[0]), ref.matrix(radius(0), target[0]))).reshape(-1))
    assert same(table2[f + 2], ref.IDENTITY_RECORD)
    # offsets: one rounded add per component
    off = np.full((len(listed), 3), 0.1)
    a.move_spheres(target - off, offsets=off)
    t = a.debug_records(ref.MOVABLE_TABLE, ref.TABLE)
    assert same(t["centre"], (target - off) + off) and list(t["object"]) == listed
    a.close()


# ---- scanned scenes: hits, frames and planes, bit for bit, after 1 move and after 5 chained moves
@pytest.mark.parametrize("eps", [False, True], ids=["fp32", "epsilon"])
def test_hits_and_frames_of_a_scanned_scene(eps):
    n = 12
    xs = [grid(n, 10 + k) for k in range(6)]
    a = build(xs[0], eps, "floor")
    a.set_movable_spheres(every(a, n))
    assert a.movable_info()["tree_nodes"] == 0
    for k in range(1, 6):
        a.move_spheres(xs[k])
        if k in (1, 5):
            b = build(xs[k], eps, "floor")
            assert_same_scene(a, b, eps, *rays(xs[k]))
            b.close()
    a.close()


# ---- a scene tree: refitted boxes, the same hits and frames
def tree_check(a, b, flat, o, d, eps=False, cam=None):
    nodes = a.debug_records(ref.TREE_NODES, ref.NODE)
    entries, order = a.debug_records(ref.TREE_ENTRIES, ref.ENTRY), a.debug_records(ref.TREE_ORDER, "<u4")
    items = a.debug_records(ref.ITEM_BOXES, "<f4").reshape(-1, 2, 4)
    assert len(nodes) > 16 and a.movable_info()["tree_nodes"] == len(nodes)
    ref.check_order(entries, order)
    raw, boxes = ref.refit(entries, order, items)
    assert same(boxes, ref.node_boxes(nodes)), "a node box is not the padded union of what lies below it"
    assert same(raw, a.debug_records(ref.TREE_RAW, "<f4").reshape(-1, 2, 4)[:, :, :3])
    for k, (x, y) in enumerate(zip(arrays(a, eps), arrays(b, eps))):
        assert same(x, y), f"array {k} differs"
    ha, hb = hits(a, o, d, eps, cam), hits(b, o, d, eps, cam)
    differ = np.zeros(len(o), dtype=bool)
    for x, y in zip(ha, hb):
        differ |= (np.asarray(x).reshape(len(o), -1) != np.asarray(y).reshape(len(o), -1)).any(axis=1)
    if differ.any():   # undecided only where B's own tree and a scan disagree
        hf = hits(flat, o, d, eps, cam)
        own = np.zeros(len(o), dtype=bool)
        for y, z in zip(hb, hf):
            own |= (np.asarray(y).reshape(len(o), -1) != np.asarray(z).reshape(len(o), -1)).any(axis=1)
        print("rays on which A and B differ:", np.flatnonzero(differ).tolist(), "of them undecided in B itself:", np.flatnonzero(differ & own).tolist())
        assert not (differ & ~own).any(), np.flatnonzero(differ & ~own)[:10]
        assert differ.sum() * 1000 <= len(o)
    for k, (x, y) in enumerate(zip(frame_and_planes(a, cam), frame_and_planes(b, cam))):
        assert np.isfinite(x).all() and same(x, y), f"frame / plane {k} differs on {int((x != y).sum())} values"


@pytest.mark.parametrize("n", [70, 200])
def test_a_refitted_scene_tree_finds_what_a_fresh_commit_finds(n):
    x0, x1, x2 = grid(n, 21), grid(n, 22), grid(n, 23, 0.12)
    a = build(x0, False, "floor")
    a.set_movable_spheres(every(a, n))
    nodes0 = a.debug_records(ref.TREE_NODES)
    a.move_spheres(x0)                                   # onto their own places: no byte of the tree changes
    assert same(a.debug_records(ref.TREE_NODES), nodes0)
    a.move_spheres(x1)
    a.move_spheres(x2)
    b = build(x2, False, "floor")
    flat = build(x2, False, "floor", options=(("scene_bvh_min", 10 * n),))
    o, d = rays(x2)
    tree_check(a, b, flat, o, d)
    # one launch per height gives the same boxes as one workgroup
    c = build(x0, False, "floor", options=(("refit_per_height", 1),))
    c.set_movable_spheres(every(c, n))
    c.move_spheres(x1)
    c.move_spheres(x2)
    assert same(c.debug_records(ref.TREE_NODES), a.debug_records(ref.TREE_NODES))
    for s in (a, b, c, flat):
        s.close()


def test_a_second_list_after_a_move_starts_where_the_spheres_are():
    """set, move, set with another list, move: a listed sphere's motion row starts where the first list left it, a sphere that was moved
    and then dropped keeps its place and stays inside the refitted tree, and the scene equals a fresh commit."""
    n = 70
    x0, x1, x2 = grid(n, 51), grid(n, 52), grid(n, 53)
    a = build(x0, False, "floor")
    f = a.first
    a.set_movable_spheres(every(a, n))
    a.move_spheres(x1)
    odd = [f + k for k in range(n) if k & 1]
    a.set_movable_spheres(odd)
    rows = [k - f for k in odd]
    table = a.move_spheres(x2[rows], motion=True)
    now = x1.copy()
    now[rows] = x2[rows]
    for k in range(n):
        want = temporal_motion_record(ref.matrix(radius(k), now[k]), ref.matrix(radius(k), x1[k])) if k & 1 else ref.IDENTITY_RECORD
        assert same(table[f + k], np.asarray(want).reshape(-1)), k
    b = build(now, False, "floor")
    flat = build(now, False, "floor", options=(("scene_bvh_min", 10 * n),))
    tree_check(a, b, flat, *rays(now))
    for s in (a, b, flat):
        s.close()


def test_a_marbles_field_moved_equals_a_marbles_field_committed():
    offsets = scenes.marbles_field_offsets((2, 2))
    rng = np.random.default_rng(8)
    rest = [scenes.marbles_initial(seed=123 + g).pos * np.array([1.0, 0.1, 1.0]) + np.array([ox, 0.0, oz]) for g, (ox, oz) in enumerate(offsets)]
    moved = [p + rng.uniform(-0.04, 0.04, p.shape) for p in rest]
    a, cam, _ = scenes.marbles_field(rest, offsets)
    objects = [g * 26 + 1 + i for g in range(4) for i in range(25)]
    a.set_movable_spheres(objects)
    assert a.movable_info()["tree_nodes"] > 0           # more than scene_bvh_min bounded records: the marbles are leaves of the scene tree
    a.move_spheres(np.concatenate(moved))
    b, _, _ = scenes.marbles_field(moved, offsets)
    flat, _, _ = scenes.marbles_field(moved, offsets)
    flat.set_option("scene_bvh_min", 100000)
    c = np.concatenate(moved)
    o, d = rays(c[::4])
    tree_check(a, b, flat, o, d, cam=cam)
    for s in (a, b, flat):
        s.close()


# ---- ordering: a move behind a queued render does not change it, a render behind the move sees it; two scenes, two streams in turn
def test_a_move_is_ordered_like_a_render_of_its_scene():
    import torch
    n = 6
    x0, x1 = grid(n, 31), grid(n, 32)
    w, h, long_spp = 96, 96, 4096                        # (the long render: 3.5 ms, tests/test_gpu_call_sequences.py)
    lone = {}
    for name, x in (("before", x0), ("after", x1)):
        s = build(x, False, "floor")
        r = Renderer(s, CAM).width(w).height(h).max_bounces(3).seed(7)
        lone[name, "long"] = r.sample_array(long_spp)
        r = Renderer(s, CAM).width(w).height(h).max_bounces(3).seed(7)
        lone[name, "short"] = r.sample_array(8)
        s.close()
    pair = [build(x0, False, "floor") for _ in range(2)]
    for s in pair:
        s.set_movable_spheres(every(s, n))
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    target = torch.from_numpy(x1.reshape(-1)).to("cuda")
    frames = [[torch.zeros(w * h * 3, dtype=torch.float64, device="cuda") for _ in range(2)] for _ in range(2)]
    torch.cuda.synchronize()
    for k, s in enumerate(pair):                         # scene k: long render on its stream, the move and the short render on the OTHER stream
        Renderer(s, CAM).width(w).height(h).max_bounces(3).seed(7).sample_device(long_spp, frames[k][0].data_ptr(), streams[k].cuda_stream)
    for k, s in enumerate(pair):
        other = streams[1 - k].cuda_stream
        s.move_spheres_device(target.data_ptr(), 0, 0, other)
        Renderer(s, CAM).width(w).height(h).max_bounces(3).seed(7).sample_device(8, frames[k][1].data_ptr(), streams[k].cuda_stream)
    torch.cuda.synchronize()
    for k in range(2):
        assert same(frames[k][0].cpu().numpy().reshape(-1, 3), lone["before", "long"]), f"scene {k}: the move reached a render queued before it"
        assert same(frames[k][1].cpu().numpy().reshape(-1, 3), lone["after", "short"]), f"scene {k}: a render queued behind the move did not see it"
    for s in pair:
        s.close()


# ---- the photon map is stale after a move
def test_a_photon_map_is_stale_after_a_move_and_good_after_a_rebuild():
    n = 4
    x0, x1 = grid(n, 41), grid(n, 42)
    a, b = build(x0, False, "floor"), build(x1, False, "floor")
    ra, rb = (Renderer(s, CAM).width(W).height(H).max_bounces(3).seed(3).gather_size(8) for s in (a, b))
    a.set_movable_spheres(every(a, n))
    ra.photon_map_build(4000, Renderer.PHOTON_MAP)
    ra.photon_sample_array(2)
    a.move_spheres(x1)
    with pytest.raises(RptError, match="rebuild the map"):
        ra.photon_sample_array(2)
    ra.photon_map_build(4000, Renderer.PHOTON_MAP)
    rb.photon_map_build(4000, Renderer.PHOTON_MAP)
    ra._sample_offset = rb._sample_offset = 0
    assert same(ra.photon_sample_array(2), rb.photon_sample_array(2))
    a.close()
    b.close()


# ---- display positions that stay on the device: integrate -> display_positions_device -> move_spheres_device, read back from the scene
def test_display_positions_device_equal_the_synchronous_entry():
    sim = ParticleSimulator(MarblesSystem(scenes.MARBLES_RADIUS), scenes.marbles_initial(), device=0)
    scene = build(np.zeros((sim.n, 3)) + np.arange(sim.n)[:, None], False, "floor")
    scene.set_movable_spheres(every(scene, sim.n))
    sim.integrate(1.0 / 64.0, 1.0 / 10000.0)
    scene.move_spheres_device(sim.display_positions_device())
    got = scene.debug_records(ref.MOVABLE_TABLE, ref.TABLE)["centre"]
    want = sim.display_positions()
    assert same(got, want) and np.isfinite(want).all() and sim.counters()[6] >= 3   # launches: the integration and both display calls
    sim.close()
    scene.close()
    states = [scenes.marbles_initial(n=5 + g, seed=7 + g) for g in range(3)]
    total = sum(len(s) for s in states)
    ens = ParticleEnsemble([MarblesSystem(scenes.MARBLES_RADIUS)] * 3, states, device=0)
    scene = build(np.zeros((total, 3)) + np.arange(total)[:, None], False, "floor")
    scene.set_movable_spheres(every(scene, total))
    ens.integrate(1.0 / 64.0, 1.0 / 10000.0)
    scene.move_spheres_device(ens.display_positions_device())
    got = scene.debug_records(ref.MOVABLE_TABLE, ref.TABLE)["centre"]
    assert same(got, np.concatenate(ens.display_positions()))
    ens.close()
    scene.close()


# ---- end to end: three frames of the live sequence are the generator path's frames
def sequence(scene, camera, frames, **kw):
    r = Renderer(scene, camera).width(64).height(48).max_bounces(4).seed(11).num_samples(4)
    return list(r.render_sequence([camera] * frames, batches=2, temporal=TemporalParams(max_history=8), **kw))


def test_marbles_live_renders_the_frames_of_marbles_sequence():
    state = scenes.marbles_initial()
    state.pos[:, 1] = 0.3 + 0.05 * (np.arange(25) % 5)   # near the glass: three frames in which the marbles move and touch
    pairs = list(scenes.marbles_sequence(3, state=state.copy()))
    want = sequence(pairs[0][0], pairs[0][1], 3, scenes=[p[0] for p in pairs])
    scene, camera, mover = scenes.marbles_live(3, state=state.copy())
    try:
        got = sequence(scene, camera, 3, live=mover)
    finally:
        mover.close()
    assert len(got) == 3 and not same(got[0], got[2])
    for f in range(3):
        assert same(got[f], want[f]), f"frame {f} differs on {int((got[f] != want[f]).sum())} bytes"
    assert scene.movable_info()["moves"] == 2


def test_marbles_field_live_renders_the_frames_of_marbles_field_sequence():
    states = [scenes.marbles_initial(seed=50 + g) for g in range(4)]
    for s in states:
        s.pos[:, 1] = 0.3 + 0.05 * (np.arange(25) % 5)
    pairs = list(scenes.marbles_field_sequence(3, grid=(2, 2), states=[s.copy() for s in states]))
    want = sequence(pairs[0][0], pairs[0][1], 3, scenes=[p[0] for p in pairs])
    scene, camera, mover = scenes.marbles_field_live(3, grid=(2, 2), states=[s.copy() for s in states])
    try:
        got = sequence(scene, camera, 3, live=mover)
    finally:
        mover.close()
    for f in range(3):
        assert same(got[f], want[f]), f"frame {f} differs on {int((got[f] != want[f]).sum())} bytes"
    assert scene.movable_info()["tree_nodes"] > 0
