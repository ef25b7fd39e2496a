"""Persistent kernels with MANY work items per lane (or wave), on varied grids.

Every heavy kernel is a persistent grid whose waves pull work items from a counter (or are dealt them statically).  The grid is
min(CUs x blocks per CU, ceil(items / 256)) blocks -- ceil(items / 4) for the kernels whose items are wave-level --, so at test
sizes every lane receives exactly ONE item and the code that hands out a second one never runs.  Option "max_blocks" caps the
grid.  One principle throughout:

    the launch in which every lane (wave) has at most one item is the isolated evaluation of each item; a launch on a small grid
    must reproduce it bit for bit, and that frame must meet the oracle within the bound the suite already asserts for the scene.

No tolerance is introduced here: each case names the existing test whose bound it reuses.  Each case asserts its own premise from
the grid the library reports: items <= lanes in the isolated launch, items >= 8 x lanes in every capped one.  Every case prints the
grids it ran and the items per lane (and appends them to the file the environment variable RPT_SCHEDULE_LOG names, if it is set)."""
import os

import numpy as np
import pytest

from rpt_amd import Camera, KdTree, Light, Material, Medium, Mesh, Object, Renderer, Scene, cube, plane, polygon, scenes, sphere, vec3
from tests.util import rel_rms

pytestmark = pytest.mark.gpu

BLOCK_LANES, BLOCK_WAVES = 256, 4


def _oracle(scene):
    from oracle.pyoracle import OracleScene
    return OracleScene(scene)


def _log(line):
    print(line)
    path = os.environ.get("RPT_SCHEDULE_LOG")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def _odd_cap(n_items, per_block, most=37):
    """The largest odd block count <= `most` that still leaves every lane (wave) of the grid 8 items; below 3: none."""
    c = min(most, n_items // (8 * per_block))
    return c if c % 2 else c - 1


def _caps(n_items, per_block, most=37):
    odd = _odd_cap(n_items, per_block, most)
    return [0, 1] + ([odd] if odd >= 3 else [])


def _check_premise(label, cap, blocks, n_items, per_block):
    """`blocks` is what the library launched.  Uncapped: the isolated launch.  Capped: at least 8 items per lane (wave)."""
    if cap == 0:
        assert n_items <= blocks * per_block, (label, "not the isolated launch", n_items, blocks)
    else:
        assert blocks == cap, (label, cap, blocks)
        assert n_items >= 8 * blocks * per_block, (label, "too few items per lane", n_items, blocks)
    return n_items / (blocks * per_block)


def _pt_items(r, w, h, spp):
    """Work items of a path-traced frame: one per (pixel slot of a 32x32 tile, chunk of samples)."""
    chunk, n_chunks = r.chunking(spp)
    return ((w + 31) // 32) * ((h + 31) // 32) * 1024 * n_chunks


def _run_grids(label, r, render, n_items, variants, counters=None, counter_keys=(), counters_keep_the_frame=False):
    """Renders every variant (dicts of scene options; the first one holds the defaults) on the default grid, on 1 block and on an odd
    number of blocks; all frames must equal the first, the isolated one, which is returned.  Then the same grids with the counters
    build: equal work counters, equal frames."""
    sc = r.scene
    sc.set_option("timing", 1)
    caps = _caps(n_items, BLOCK_LANES)
    iso = None
    try:
        for cap in caps:
            sc.set_option("max_blocks", cap)
            for v in variants:
                for k, val in v.items():
                    sc.set_option(k, val)
                r._sample_offset = 0
                frame = render()
                blocks = r.timing()[2]
                per = _check_premise(label, cap, blocks, n_items, BLOCK_LANES)
                if iso is None:
                    iso = frame
                    assert np.all(np.isfinite(iso)) and iso.mean() > 0, label
                equal = np.array_equal(frame, iso)
                _log(f"{label}: max_blocks {cap} -> {blocks} blocks, {n_items} items, {per:.2f} per lane, {v}: "
                     f"{'equal to' if equal else 'DIFFERS from'} the isolated frame ({int((frame != iso).any(axis=1).sum())} pixels differ)")
                assert equal, (label, cap, v)
        for k, val in variants[0].items():
            sc.set_option(k, val)
        if counters is not None:
            sc.set_option("counters", 1)
            seen = []
            for cap in caps:
                sc.set_option("max_blocks", cap)
                r._sample_offset = 0
                frame = render()
                _check_premise(label, cap, r.timing()[2], n_items, BLOCK_LANES)
                seen.append((frame, counters(r)))
            for frame, cnt in seen:
                assert np.array_equal(frame, seen[0][0]), (label, "counters build")
                for k in counter_keys:
                    assert cnt[k] == seen[0][1][k], (label, k, cnt[k], seen[0][1][k])
                if counters_keep_the_frame:
                    assert np.array_equal(frame, iso), (label, "counters build against the plain one")
            assert seen[0][1][counter_keys[0]] > 0
            _log(f"{label}: counters build on {caps}: frames and {list(counter_keys)} equal")
    finally:
        sc.set_option("counters", 0)
        sc.set_option("max_blocks", 0)
    return iso


FP32_COUNTERS = ("samples", "rays", "vertices", "prim_tests", "stack_overflows")
FP64_COUNTERS = ("rays", "hits", "self_hits", "shadow_tests", "shadow_pass", "shadow_near", "samples", "vertices")


def _pull_batches(values, default=2):
    return [{"pull_batch": default}] + [{"pull_batch": v} for v in values if v != default]


# ------------------------------------------------------------------ render_kernel (fp32)
@pytest.mark.parametrize("name,tol", [("C2", 2e-3), ("C3", 3e-3)])
def test_scan_kernels_on_small_grids(name, tol):
    """render_kernel's linear scans, surface (C2) and medium (C3), 96x96x32: "pull_batch" 1, 2, 33, 64 crossed with the grids.
    Oracle bound: test_render_matches_oracle_same_seed (robust policy, same seed)."""
    scene, cam, cfg = scenes.CONFIGS[name]()
    size, spp = 96, 32
    r = Renderer(scene, cam).width(size).height(size).max_bounces(cfg["max_bounces"]).seed(3)
    iso = _run_grids(f"render_kernel scan {name} {size}x{size}x{spp}", r, lambda: r.sample_array(spp), _pt_items(r, size, size, spp),
                     _pull_batches((1, 2, 33, 64)), counters=lambda q: q.counters(), counter_keys=FP32_COUNTERS)
    exp = _oracle(scene).render(cam, size, size, spp, cfg["max_bounces"], seed=3, robust=1)
    assert rel_rms(iso, exp) < tol


def _two_torus_scene(fog):
    """The scene of test_deferred_tree_walks_do_not_depend_on_the_schedule: two meshes with trees of their own, two mesh lights."""
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
    return sc, Camera.look_at(vec3(0.0, 1.5, 6.0), vec3(0.0, 0.0, 0.0), vec3(0, 1, 0), 0.8)


@pytest.mark.parametrize("fog,detach", [(False, 0), (True, 0), (True, 1)])
def test_mesh_tree_kernels_on_small_grids(fog, detach):
    """render_kernel over per-mesh trees, 96x72x24: parked walks (detach_shadows = 0) and, in fog, detached shadow queries.
    Oracle bound: test_deferred_tree_walks_do_not_depend_on_the_schedule."""
    sc, cam = _two_torus_scene(fog)
    sc.set_option("detach_shadows", detach)
    w, h, spp = 96, 72, 24
    r = Renderer(sc, cam).width(w).height(h).max_bounces(3).seed(6)
    st = r.scene_stats()
    assert st["bvh_nodes"] > 0 and st["scene_bvh"] == 0
    iso = _run_grids(f"render_kernel mesh trees fog={fog} detach={detach} {w}x{h}x{spp}", r, lambda: r.sample_array(spp),
                     _pt_items(r, w, h, spp), _pull_batches((1, 9, 64)), counters=lambda q: q.counters(), counter_keys=FP32_COUNTERS)
    exp = _oracle(sc).render(cam, w, h, spp, 3, seed=6, robust=1)
    assert exp.mean() > 0
    assert rel_rms(iso, exp) < 2e-2
    assert abs(iso.mean() - exp.mean()) / exp.mean() < 5e-3


@pytest.mark.parametrize("which", ["scene tree", "scene tree + parked mesh"])
def test_scene_tree_kernels_on_small_grids(which):
    """render_kernel with a scene-level tree (BVH = 2: fractal_spheres, as test_fractal_spheres_render_matches_oracle renders it) and
    with a mesh parked beside it (BVH = 3: the scene of test_large_mesh_in_a_group_is_walked_outside_the_scene_tree_with_parked_walks).
    Oracle bounds: those tests'."""
    if which == "scene tree":
        scene, cam, _ = scenes.fractal_spheres()
        w, h, spp, mb, seed, tol, tol_mean, mode = 160, 120, 16, 2, 4, 5e-3, 2e-3, 1
    else:
        scene, cam, cfg = scenes.mesh_among_spheres(nu=48, nv=32, n_spheres=64)
        w, h, spp, mb, seed, tol, tol_mean, mode = 96, 72, 16, cfg["max_bounces"], 4, 1e-2, 5e-3, 2
    r = Renderer(scene, cam).width(w).height(h).max_bounces(mb).seed(seed)
    assert r.scene_stats()["scene_bvh"] == mode
    iso = _run_grids(f"render_kernel {which} {w}x{h}x{spp}", r, lambda: r.sample_array(spp), _pt_items(r, w, h, spp),
                     _pull_batches((1, 64)), counters=lambda q: q.counters(), counter_keys=FP32_COUNTERS)
    exp = _oracle(scene).render(cam, w, h, spp, mb, seed=seed, robust=1)
    assert exp.mean() > 0
    assert rel_rms(iso, exp) < tol
    assert abs(iso.mean() - exp.mean()) / exp.mean() < tol_mean


@pytest.mark.parametrize("eps", [False, True])
def test_monomial_kernels_on_small_grids(eps):
    """The MONO instantiations of render_kernel and render_f64_kernel on monomial_glass, as
    test_glass_render_is_deterministic_and_shards_add_up renders it (the oracle has no MonomialSurface: bit equality only)."""
    scene, cam, cfg = scenes.monomial_glass()
    if eps:
        scene.set_option("epsilon_policy", 1)
    w, h, spp = 96, 72, 16
    r = Renderer(scene, cam).width(w).height(h).max_bounces(cfg["max_bounces"]).seed(9)
    _run_grids(f"{'render_f64_kernel' if eps else 'render_kernel'} MONO {w}x{h}x{spp}", r, lambda: r.sample_array(spp),
               _pt_items(r, w, h, spp), _pull_batches((1, 64)))


# ------------------------------------------------------------------ render_f64_kernel
def _eps_counters(r):
    from tests.test_gpu_epsilon import _eps_counters as f
    return f(r)


@pytest.mark.parametrize("name", ["C2", "C3"])
def test_f64_render_on_small_grids(name):
    """render_f64_kernel, 96x96x32, seed 3: "pull_batch" and (in the medium of C3) "f64_surf_batch" 1, 8, 64 crossed with the grids.
    Oracle bound: test_small_renders_follow_the_literal_oracle (rel. RMS < 2e-3, mean within 1e-4)."""
    scene, cam, cfg = scenes.CONFIGS[name]()
    scene.set_option("epsilon_policy", 1)
    size, spp = 96, 32
    r = Renderer(scene, cam).width(size).height(size).max_bounces(cfg["max_bounces"]).seed(3)
    surf = (8, 1, 64) if name == "C3" else (8,)
    variants = [{"pull_batch": 2, "f64_surf_batch": 8}] + [{"pull_batch": pb, "f64_surf_batch": sb} for pb in (1, 8, 64) for sb in surf]
    iso = _run_grids(f"render_f64_kernel {name} {size}x{size}x{spp}", r, lambda: r.sample_array(spp), _pt_items(r, size, size, spp),
                     variants, counters=_eps_counters, counter_keys=FP64_COUNTERS, counters_keep_the_frame=True)
    exp = _oracle(scene).render(cam, size, size, spp, cfg["max_bounces"], seed=3, robust=0)
    assert exp.mean() > 0
    assert rel_rms(iso, exp) < 2e-3
    assert abs(iso.mean() - exp.mean()) < 1e-4 * exp.mean()


def _mesh_in_fog_scene():
    """The 960-triangle mesh, plane and fog of test_gather_lists_in_global_memory_and_records_outside_lds: more triangle records
    than the fp64 kernels' LDS tables hold."""
    sc = Scene()
    sc.add(Object(Mesh(scenes.bumpy_torus(24, 20)).scale(vec3(1.5, 1.5, 1.5)).rotate_x(0.5)).material(Material.diffuse(vec3(0.8, 0.6, 0.3))))
    sc.add(Object(plane(vec3(0, 1, 0), -1.2)).material(Material.diffuse(vec3(0.7, 0.7, 0.7))))
    quad = [vec3(1.0, 3.0, -1.0), vec3(1.0, 3.0, 1.0), vec3(-1.0, 3.0, 1.0), vec3(-1.0, 3.0, -1.0)]
    sc.add(Object(polygon(quad)).material(Material.light(vec3(1, 1, 1), 40.0)))
    sc.add(Light.Object(Object(polygon(quad)).material(Material.light(vec3(1, 1, 1), 40.0))))
    sc.add(Medium.homogeneous_isotropic(0.02, 0.08))
    return sc, Camera.look_at(vec3(0.0, 1.5, 5.0), vec3(0.0, 0.0, 0.0), vec3(0, 1, 0), 0.8)


def _group_light_scene():
    """The scene of test_group_as_object_light_follows_the_literal_oracle, in fog."""
    lamp_kids = [
        sphere().scale(vec3(0.3, 0.3, 0.3)).translate(vec3(-1.5, 2.5, 0.0)),
        cube().scale(vec3(0.5, 0.1, 0.5)).rotate_y(0.5).translate(vec3(1.5, 2.6, 0.3)),
        Mesh(scenes.bumpy_torus(4, 3)).scale(vec3(0.4, 0.4, 0.4)).translate(vec3(0.0, 2.4, -1.0)),
        KdTree([sphere().scale(vec3(0.2, 0.2, 0.2)).translate(vec3(0.0, 0.0, 1.0)),
                KdTree([sphere().scale(vec3(0.15, 0.3, 0.15)).translate(vec3(0.6, 0.0, 1.2))]).rotate_x(0.2)]).translate(vec3(0.0, 2.3, 0.0)),
    ]
    glow = Material.light(vec3(1.0, 0.9, 0.7), 25.0)

    def lamp():
        return KdTree([k.clone() for k in lamp_kids]).rotate_z(0.1).translate(vec3(0.0, 0.2, 0.0))
    sc = Scene()
    sc.add(Object(lamp()).material(glow))
    sc.add(Light.Object(Object(lamp()).material(glow)))
    sc.add(Object(plane(vec3(0, 1, 0), -1.0)).material(Material.diffuse(vec3(0.8, 0.8, 0.8))))
    sc.add(Object(sphere().translate(vec3(0.0, 0.0, 0.0))).material(Material.specular(vec3(0.9, 0.5, 0.5), 0.3)))
    sc.add(Object(cube().translate(vec3(2.0, -0.5, 0.5))).material(Material.diffuse(vec3(0.3, 0.8, 0.4))))
    sc.add(Medium.homogeneous_isotropic(0.02, 0.05))
    return sc, Camera.look_at(vec3(0.0, 1.5, 7.0), vec3(0.0, 1.0, 0.0), vec3(0, 1, 0), 0.9)


@pytest.mark.parametrize("case", ["records outside LDS", "more than 32 objects", "group light"])
def test_f64_render_flavours_on_small_grids(case):
    """The other instantiations of render_f64_kernel: triangle records read from global memory (the mesh-in-fog scene of
    test_gather_lists_in_global_memory_and_records_outside_lds, bound of that test's mesh leg: 2e-3 / 5e-4), more than 32 objects
    (cull32's union boxes; the "spheres" scene of test_kdtree_groups_follow_the_literal_oracle at its size and bound: 5e-3 / 5e-4)
    and a KdTree group as the light (test_group_as_object_light_follows_the_literal_oracle, in fog, at its size and bound)."""
    if case == "records outside LDS":
        (sc, cam), w, h, spp, mb, seed, tol, tol_mean = _mesh_in_fog_scene(), 96, 72, 24, 3, 11, 2e-3, 5e-4
    elif case == "more than 32 objects":
        from tests.test_gpu_epsilon import _group_scene
        sc, cam, mb = _group_scene("spheres")
        assert sum(len(o.shape.base().shapes) if isinstance(o.shape.base(), KdTree) else 1 for o in sc.objects) > 32
        w, h, spp, seed, tol, tol_mean = 72, 54, 8, 5, 5e-3, 5e-4
    else:
        (sc, cam), w, h, spp, mb, seed, tol, tol_mean = _group_light_scene(), 80, 60, 32, 3, 9, 5e-3, 5e-4
    sc.set_option("epsilon_policy", 1)
    r = Renderer(sc, cam).width(w).height(h).max_bounces(mb).seed(seed)
    variants = [{"pull_batch": 2, "f64_surf_batch": 8}, {"pull_batch": 1, "f64_surf_batch": 64}, {"pull_batch": 64, "f64_surf_batch": 1}]
    iso = _run_grids(f"render_f64_kernel {case} {w}x{h}x{spp}", r, lambda: r.sample_array(spp), _pt_items(r, w, h, spp), variants,
                     counters=_eps_counters, counter_keys=FP64_COUNTERS, counters_keep_the_frame=True)
    exp = _oracle(sc).render(cam, w, h, spp, mb, seed=seed, robust=0)
    assert exp.mean() > 0
    assert rel_rms(iso, exp) < tol, case
    assert abs(iso.mean() - exp.mean()) < tol_mean * exp.mean(), case


# ------------------------------------------------------------------ photon_query_kernel (fp32): work items are wave-level
def _photon_frames(label, r, w, h, spp, parts_list, caps_most=3):
    """Camera pass of the map `r` holds on the default grid, 1 block and 3 blocks, for every "photon_parts"; -> {parts: isolated frame}.
    An item is (strip of an 8x8 pixel block, chunk of 256 samples) and belongs to one wave."""
    sc = r.scene
    sc.set_option("timing", 1)
    out = {}
    try:
        for parts in parts_list:
            sc.set_option("photon_parts", parts)
            n_items = ((w + 31) // 32) * ((h + 31) // 32) * 16 * parts * ((spp + 255) // 256)
            for cap in _caps(n_items, BLOCK_WAVES, caps_most):
                sc.set_option("max_blocks", cap)
                r._sample_offset = 0
                frame = r.photon_sample_array(spp)
                blocks = r.timing()[2]
                per = _check_premise(label, cap, blocks, n_items, BLOCK_WAVES)
                if cap == 0:
                    out[parts] = frame
                    assert np.all(np.isfinite(frame)) and frame.mean() > 0, label
                equal = np.array_equal(frame, out[parts])
                _log(f"{label}: photon_parts {parts}, max_blocks {cap} -> {blocks} blocks, {n_items} items, {per:.2f} per wave: "
                     f"{'equal to' if equal else 'DIFFERS from'} the isolated frame ({int((frame != out[parts]).any(axis=1).sum())} pixels differ)")
                assert equal, (label, parts, cap)
    finally:
        sc.set_option("photon_parts", 4)
        sc.set_option("max_blocks", 0)
    return out


@pytest.mark.parametrize("name,tol", [("C4", 5e-3), ("C2", 3e-2)])
def test_photon_camera_pass_on_small_grids(name, tol):
    """Beam x point camera pass exactly as test_photon_camera_pass_matches_oracle runs it (20 k photons, 64x64x4, seed 0), 256 items
    on 12 and on 4 waves (64 items on 4 waves with "photon_parts" = 1), and that test's three assertions on the isolated frames."""
    scene, cam, cfg = scenes.CONFIGS[name]()
    n, size, spp = 20000, 64, 4
    watts = 14.65 * n
    r = Renderer(scene, cam).width(size).height(size).watts(watts).gather_size(20).gather_size_volume(3).seed(0)
    r.photon_map_build(n, 1)
    frames = _photon_frames(f"photon_query_kernel beam x point {name} {size}x{size}x{spp}", r, size, size, spp, (4, 1))
    exp = _oracle(scene).photon_map(n, 1, watts, 20, 3, seed=0, robust=1).render(cam, size, size, spp, seed=0)
    assert exp.mean() > 0
    for parts, got in frames.items():
        assert rel_rms(got, exp) < tol, parts
        assert abs(got.mean() - exp.mean()) / exp.mean() < 2e-3, parts
        d = np.abs(got - exp).sum(axis=1) / (np.abs(exp).sum(axis=1) + 1e-9)
        assert (d > 0.01).mean() < 0.03, parts


def test_photon_camera_pass_on_a_ragged_frame_on_small_grids():
    """50x37x5: clipped tiles and pixel blocks, a sample count below a chunk.  Bit equality across the grids."""
    scene, cam, cfg = scenes.CONFIGS["C4"]()
    n, w, h, spp = 20000, 50, 37, 5
    r = Renderer(scene, cam).width(w).height(h).watts(14.65 * n).gather_size(20).gather_size_volume(3).seed(0)
    r.photon_map_build(n, 1)
    _photon_frames(f"photon_query_kernel beam x point C4 {w}x{h}x{spp}", r, w, h, spp, (4, 1))


@pytest.mark.parametrize("name,kind", [("C4", 0), ("C2", 0), ("C4", 2)])
def test_the_other_photon_estimators_on_small_grids(name, kind):
    """Point x point as test_point_point_photon_map_matches_oracle runs it (64x64x4, gather 20 / 8, seed 2; C4 2e-2, C2 3e-2) and
    beam x beam as test_beam_beam_photon_map_matches_oracle does (200 k photons, 48x48x2, seed 5; 3e-2), with their bounds."""
    scene, cam, cfg = scenes.CONFIGS[name]()
    if kind == 0:
        n, size, spp, gv, seed, tol, tol_mean = 20000, 64, 4, 8, 2, (2e-2 if name == "C4" else 3e-2), 5e-3
    else:
        n, size, spp, gv, seed, tol, tol_mean = 200000, 48, 2, 3, 5, 3e-2, 5e-3
    watts = 14.65 * n
    r = Renderer(scene, cam).width(size).height(size).watts(watts).gather_size(20).gather_size_volume(gv).seed(seed)
    r.photon_map_build(n, kind)
    frames = _photon_frames(f"photon_query_kernel kind {kind} {name} {size}x{size}x{spp}", r, size, size, spp, (4, 1))
    exp = _oracle(scene).photon_map(n, kind, watts, 20, gv, seed=seed, robust=1).render(cam, size, size, spp, seed=seed)
    assert exp.mean() > 0
    for parts, got in frames.items():
        assert rel_rms(got, exp) < tol, parts
        assert abs(got.mean() - exp.mean()) / exp.mean() < tol_mean, parts
        if kind == 0:
            d = np.abs(got - exp).sum(axis=1) / (np.abs(exp).sum(axis=1) + 1e-9)
            assert (d > 0.01).mean() < 0.05, parts


# ------------------------------------------------------------------ photon_query_kernel<EMIT> + photon_surface_f64_kernel
def _device_photons(r):
    ps = r.photon_map_download(0).astype(np.float64)
    ps[:, :3] = r.photon_positions64()
    return ps, r.photon_map_download(1).astype(np.float64)


@pytest.mark.parametrize("name,w,h", [("C4", 32, 32), ("C2", 32, 32), ("C4", 40, 24)])
def test_f64_photon_camera_pass_on_small_grids(name, w, h):
    """The reference-epsilon camera pass, 20 k photons, 80 spp: one full group of 64 samples and one with 16 live lanes per pixel,
    2,048-4,096 wave-level items, so the default grid (CUs x 4 blocks x 4 waves) is the isolated launch; 37 blocks (13+ items per wave)
    and 1 block reproduce it bit for bit, per-sample selections included (they tell which of the two kernels moved).  Oracle bound:
    test_camera_pass_on_the_devices_own_photons (literal pass over the device's photons; set at 16 spp, 80 spp only lowers the noise
    it has to cover)."""
    n, spp = 20000, 80
    scene, cam, cfg = scenes.CONFIGS[name]()
    scene.set_option("epsilon_policy", 1)
    scene.set_option("timing", 1)
    r = Renderer(scene, cam).width(w).height(h).watts(14.65 * n).gather_size(20).gather_size_volume(3)
    r.seed(7).photon_map_build(n, Renderer.PHOTON_POINT_BEAM)
    r.seed(0)
    n_owned = ((w + 31) // 32) * ((h + 31) // 32) * 1024
    n_items = n_owned * ((spp + 63) // 64)                    # photon_surface_f64_kernel: one wave per (pixel slot, 64 samples)
    n_emit = (n_owned // 64) * 4                              # its EMIT partner: 8x8 pixel blocks x 4 strips, one chunk
    label = f"photon_surface_f64_kernel {name} {w}x{h}x{spp}"
    iso = sel = None
    try:
        for cap in _caps(n_items, BLOCK_WAVES):
            scene.set_option("max_blocks", cap)
            r._sample_offset = 0
            frame = r.photon_sample_array(spp)
            blocks, emit_blocks = r._photon_stats()["surface64_blocks"], r.timing()[2]
            per = _check_premise(label, cap, blocks, n_items, BLOCK_WAVES)
            if cap == 1:
                _check_premise(label + " (EMIT)", cap, emit_blocks, n_emit, BLOCK_WAVES)
            picked = r.photon_selections()
            if iso is None:
                iso, sel = frame, picked
                assert np.all(np.isfinite(iso)) and iso.mean() > 0
            equal, sel_equal = np.array_equal(frame, iso), np.array_equal(picked, sel)
            _log(f"{label}: max_blocks {cap} -> {blocks} blocks ({emit_blocks} for EMIT), {n_items} items, {per:.2f} per wave: "
                 f"frame {'equal to' if equal else 'DIFFERS from'} the isolated one ({int((frame != iso).any(axis=1).sum())} pixels differ), "
                 f"selections {'equal' if sel_equal else 'DIFFER'}")
            assert sel_equal, (label, cap, "photon_query_kernel<EMIT> moved")
            assert equal, (label, cap, "photon_surface_f64_kernel moved")
    finally:
        scene.set_option("max_blocks", 0)
    ps, pv = _device_photons(r)
    scene0, _, _ = scenes.CONFIGS[name]()
    exp = _oracle(scene0).photon_map_from_photons(n, 1, 14.65 * n, 20, 3, ps, pv, robust=0).render(cam, w, h, spp, seed=0)
    err, bias = rel_rms(iso, exp), (iso.mean() - exp.mean()) / exp.mean()
    _log(f"{label}: against the literal oracle on the device's photons: rel RMS {err:.3e}, bias {bias:+.3e}")
    assert exp.mean() > 0
    assert err < 5e-4 and abs(bias) < 5e-5


# ------------------------------------------------------------------ photon_shoot_f64_kernel: count pass + write pass
def _shoot(name, kind, n, cap=0):
    scene, cam, cfg = scenes.CONFIGS[name]()
    scene.set_option("epsilon_policy", 1)
    scene.set_option("max_blocks", cap)
    r = Renderer(scene, cam).watts(16.0 * n).seed(7)          # per-photon power exactly 16 for every n
    st = r.photon_map_build(n, kind)                          # (fails with RptError when the write pass does not retrace the count pass)
    maps = [r.photon_map_download(0), r.photon_map_download(1), r.photon_positions64()]
    assert len(maps[0]) == st["surface"] and len(maps[1]) == st["volume"]
    return st, maps


def _unmatched(have, want, tol):
    """Share of the photons `want` (positions, (n, 3)) without a twin among `have` within tol * (1 + |x|_inf)."""
    from scipy.spatial import cKDTree
    if len(want) == 0:
        return 0.0
    if len(have) == 0:
        return 1.0
    d, _ = cKDTree(have).query(want)
    return float((d > tol * (1.0 + np.abs(want).max(axis=1))).mean())


@pytest.mark.parametrize("name", ["C4", "C2"])
@pytest.mark.parametrize("kind", [0, 1, 2])
def test_f64_shooting_pass_on_small_grids(name, kind):
    """photon_shoot_f64_kernel, 20,000 photons = 313 batches of 64 drawn from a counter.
    Grids: records, fp64 positions and counts bit-equal on the default grid (316 waves), 1 block (78 batches per wave) and 3 blocks.
    Prefix: a photon's chain is keyed by its global index alone, so the records of a map of 64 photons -- one wave, one batch, every
    lane in its initial state: the isolated evaluation -- are the first records of the maps of 4,096 and 20,000, and those of 4,096 a
    prefix of 20,000's (all but the gather radius, which belongs to the map).
    Per photon against the literal oracle: u_dev = share of the oracle's literal photons without a device twin within
    1e-9 (1 + |x|) (fp64 surface positions; the volume records are fp32: 1e-6 there, 16 fp32 ulps), u_rob = the same share against the
    ROBUST oracle's map.  The robust policy parts from the literal one at every self-intersection the literal one accepts
    (probability p per hit); a device whose last bits differ redraws that lottery independently and parts with probability
    <= 2 p (1 - p).  So u_dev <= 2.5 u_rob + 10 / n_stored (2 + 25 % for the counting noise of ~80 photons)."""
    n = 20000
    n_batches = (n + 63) // 64
    label = f"photon_shoot_f64_kernel {name} kind {kind}"
    st, iso = _shoot(name, kind, n)
    _check_premise(label, 0, st["shoot_blocks"], n_batches, BLOCK_WAVES)
    for cap in (1, 3):
        st_c, maps = _shoot(name, kind, n, cap)
        per = _check_premise(label, cap, st_c["shoot_blocks"], n_batches, BLOCK_WAVES)
        equal = all(np.array_equal(a, b) for a, b in zip(iso, maps))
        _log(f"{label}: max_blocks {cap} -> {st_c['shoot_blocks']} blocks, {n_batches} batches, {per:.2f} per wave: maps "
             f"{'equal to' if equal else 'DIFFER from'} the default grid's ({st['shoot_blocks']} blocks); {st_c['surface']} + {st_c['volume']} records")
        assert (st_c["surface"], st_c["volume"]) == (st["surface"], st["volume"]), (label, cap)
        assert equal, (label, cap)
    # ---- prefix
    small = {m: _shoot(name, kind, m)[1] for m in (64, 4096)}
    for m, big in ((64, small[4096]), (64, iso), (4096, iso)):
        s = small[m]
        ok = (np.array_equal(s[0][:, :9], big[0][:len(s[0]), :9]) and np.array_equal(s[1][:, :9], big[1][:len(s[1]), :9])
              and np.array_equal(s[2], big[2][:len(s[2])]))
        _log(f"{label}: the {len(s[0])} + {len(s[1])} records of {m} photons are {'a prefix' if ok else 'NOT a prefix'} of a larger map's")
        assert ok, (label, m)
    assert len(small[64][0]) > 0
    # ---- per photon against the literal oracle
    scene, cam, cfg = scenes.CONFIGS[name]()
    lit = _oracle(scene).photon_map(n, kind, 16.0 * n, 20, 3, seed=7, robust=0)
    rob = _oracle(scene).photon_map(n, kind, 16.0 * n, 20, 3, seed=7, robust=1)
    for which, dev, tol in ((0, iso[2], 1e-9), (1, iso[1][:, :3].astype(np.float64), 1e-6)):
        e, e_rob = lit.photons(which)[:, :3], rob.photons(which)[:, :3]
        if len(e) == 0:
            assert len(dev) == 0
            continue
        u_dev, u_rob = _unmatched(dev, e, tol), _unmatched(e_rob, e, tol)
        _log(f"{label}: {'surface' if which == 0 else 'volume'} photons: {len(e)} literal, {len(dev)} device; u_dev = {u_dev:.3e}, u_rob = {u_rob:.3e}")
        assert u_dev <= 2.5 * u_rob + 10.0 / len(e), (label, which, u_dev, u_rob)
