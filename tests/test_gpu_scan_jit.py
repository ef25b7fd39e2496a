"""The scan kernels compiled for a scene's record counts (option "scan_jit", rpt_scan_jit_info).

The specialised kernel runs the same record tests in the same order on the same records as the AOT one, so every frame here is
compared bit for bit (torch.equal) between "scan_jit" = 2 (always) and 0 (never).  Every case also asserts, through the query, which
kernel it ran: a frame that equals the AOT frame because the AOT kernel rendered both proves nothing.

The cache directory is the module's own (RPT_JIT_CACHE), so nothing here depends on or changes the user's cache; a shape is compiled
once per session and found in the process afterwards."""
import glob
import os

import numpy as np
import pytest
import torch

from rpt_amd import Camera, Light, Material, Medium, Object, Renderer, Scene, _lib, cube, plane, polygon, scenes, sphere, vec3

pytestmark = pytest.mark.gpu

W = H = 64
SPP = 8


@pytest.fixture(scope="module", autouse=True)
def jit_cache(tmp_path_factory):
    old = {k: os.environ.get(k) for k in ("RPT_JIT_CACHE", "RPT_HIPRTC_LIB")}
    d = tmp_path_factory.mktemp("scan_jit_cache")
    os.environ["RPT_JIT_CACHE"] = str(d)
    os.environ.pop("RPT_HIPRTC_LIB", None)
    yield d
    for k, v in old.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v


def _renderer(make, jit, w=W, h=H, seed=1, **options):
    out = make()
    scene, cam = out[0], out[1]
    mb = out[2]["max_bounces"] if len(out) > 2 else 3
    scene.set_option("scan_jit", jit)
    for k, v in options.items():
        scene.set_option(k, v)
    return Renderer(scene, cam).width(w).height(h).max_bounces(mb).seed(seed)


def _frame(r, spp=SPP):
    return torch.from_numpy(np.ascontiguousarray(r.sample_array(spp)))


def _both(make, expect_state="active", **options):
    """-> (frame with scan_jit = 0, frame with 2, query of the second); asserts which kernel ran."""
    r0, r2 = _renderer(make, 0, **options), _renderer(make, 2, **options)
    f0, f2 = _frame(r0), _frame(r2)
    i0, i2 = r0.scan_jit_info(), r2.scan_jit_info()
    print("scan_jit 2:", i2)
    assert i0["state"] == "off" and i0["launches"] == 0
    assert i2["state"] == expect_state, i2
    if expect_state == "active":
        assert i2["launches"] == 1 and 0 < i2["vgprs"] <= i2["aot_vgprs"] <= 80, i2
    else:
        assert i2["launches"] == 0, i2
    assert torch.isfinite(f0).all() and f0.mean() > 0
    return f0, f2, i2


def _every_kind():
    """Fog; one sphere (and the light's own: two sphere records), three cubes (one not a y-rotation: the pair body takes the general form, the third is the leftover loop), a plane,
    three boxes (a pair and a single), rectangles on all three axes, a triangle record, and a sphere as the light."""
    sc = Scene()
    grey, red = Material.diffuse(vec3(0.7, 0.7, 0.7)), Material.diffuse(vec3(0.8, 0.3, 0.2))
    sc.add(Object(sphere().scale(vec3(0.5, 0.5, 0.5)).translate(vec3(-1.5, -0.5, 0.5))).material(Material.specular(vec3(0.8, 0.8, 0.3), 0.2)))
    sc.add(Object(cube().scale(vec3(0.6, 0.6, 0.6)).rotate_y(0.4).translate(vec3(1.6, -0.7, 0.2))).material(red))
    sc.add(Object(cube().scale(vec3(0.5, 0.8, 0.5)).rotate_x(0.3).translate(vec3(0.2, -0.5, -1.2))).material(grey))
    sc.add(Object(cube().scale(vec3(0.3, 0.3, 0.3)).rotate_y(1.1).translate(vec3(-0.4, -0.85, 1.4))).material(red))
    sc.add(Object(plane(vec3(0, 1, 0), -1.0)).material(grey))
    for x in (-2.6, 2.6, 0.0):
        sc.add(Object(cube().scale(vec3(0.2, 1.5, 0.2)).translate(vec3(x, -0.25, -2.0))).material(grey))
    sc.add(Object(polygon([vec3(-3, -1, -3), vec3(-3, 2, -3), vec3(-3, 2, 2), vec3(-3, -1, 2)])).material(red))            # x
    sc.add(Object(polygon([vec3(-1, -0.2, -1), vec3(-1, -0.2, 0), vec3(0, -0.2, 0), vec3(0, -0.2, -1)])).material(grey))   # y
    sc.add(Object(polygon([vec3(-3, -1, -3), vec3(3, -1, -3), vec3(3, 2, -3), vec3(-3, 2, -3)])).material(grey))          # z
    sc.add(Object(polygon([vec3(0.5, -1.0, 1.0), vec3(1.3, -1.0, 1.3), vec3(0.9, 0.2, 1.1)])).material(red))
    lamp = sphere().scale(vec3(0.3, 0.3, 0.3)).translate(vec3(0.0, 2.2, 0.5))
    glow = Material.light(vec3(1.0, 0.95, 0.9), 40.0)
    sc.add(Object(lamp.clone()).material(glow))
    sc.add(Light.Object(Object(lamp.clone()).material(glow)))
    sc.add(Medium.homogeneous_isotropic(0.02, 0.06))
    return sc, Camera.look_at(vec3(0.0, 1.0, 6.0), vec3(0.0, 0.0, 0.0), vec3(0, 1, 0), 0.9)


def _shell_only():
    """The five walls of the Cornell room fold into the shell; nothing else is scanned.  A point and an ambient light, no fog."""
    sc = Scene()
    scenes._cornell_walls(sc, Material.diffuse(vec3(0.7, 0.7, 0.7)), Material.diffuse(vec3(0.7, 0.1, 0.1)), Material.diffuse(vec3(0.1, 0.7, 0.1)))
    sc.add(Light.Point(vec3(2e5, 2e5, 2e5), vec3(278.0, 400.0, 280.0)))
    sc.add(Light.Ambient(vec3(0.3, 0.3, 0.3)))
    return sc, scenes._cornell_camera()


def _two_spheres(shift):
    def make():
        sc = Scene()
        sc.add(Object(sphere().scale(vec3(0.6, 0.6, 0.6)).translate(vec3(-1.0 + shift, 0.0, 0.0))).material(Material.diffuse(vec3(0.8, 0.4, 0.3))))
        sc.add(Object(sphere().scale(vec3(0.4 + shift, 0.4, 0.4)).translate(vec3(1.0, -0.2, 0.5 * shift))).material(Material.specular(vec3(0.6, 0.8, 0.9), 0.3)))
        quad = [vec3(1.0, 3.0, -1.0), vec3(1.0, 3.0, 1.0), vec3(-1.0, 3.0, 1.0), vec3(-1.0, 3.0, -1.0)]
        sc.add((polygon(quad), Material.light(vec3(1, 1, 1), 40.0)))
        sc.add(Medium.homogeneous_isotropic(0.02, 0.08))
        return sc, Camera.look_at(vec3(0.0, 1.0, 5.0), vec3(0.0, 0.0, 0.0), vec3(0, 1, 0), 0.8)
    return make


@pytest.mark.parametrize("max_blocks", [0, 1])
def test_c3_equals_its_aot_frame(max_blocks):
    """C3 at 64x64x8 on the default grid and on one block, where every lane pulls 64 items (asserted from the reported grid)."""
    f0, f2, info = _both(scenes.lampshade, max_blocks=max_blocks, timing=1)
    assert torch.equal(f0, f2)
    assert info["shape"] == "0,2,0,4,0,1,0,0,1,1,0x0ull,0x3ull;medium=1"
    if max_blocks:
        r = _renderer(scenes.lampshade, 2, max_blocks=max_blocks, timing=1)
        f = _frame(r)
        blocks, (chunk, n_chunks) = r.timing()[2], r.chunking(SPP)
        n_items = ((W + 31) // 32) * ((H + 31) // 32) * 1024 * n_chunks
        assert blocks == 1 and n_items >= 8 * 256 * blocks, (blocks, n_items)
        assert r.scan_jit_info()["cache"] == "memory" and torch.equal(f, f0)


def test_c2_equals_its_aot_frame():
    f0, f2, info = _both(scenes.cornell)
    assert torch.equal(f0, f2)
    assert info["shape"] == "1,1,0,0,0,1,0,0,1,1,0x1ull,0x1ull;medium=0" and info["scratch"] == 0


@pytest.mark.parametrize("shadow_scan", [1, 0])
def test_every_scanned_kind_at_awkward_counts(shadow_scan):
    """Both shadow forms of one code object: the light's own form and, with "shadow_scan" = 0, the closest-hit one."""
    f0, f2, info = _both(_every_kind, shadow_scan=shadow_scan)
    assert torch.equal(f0, f2)
    assert info["shape"].startswith("2,3,1,3,1,1,1,1,0,") and info["shape"].endswith("0x3ull,0x5ull;medium=1"), info
    assert info["cache"] == ("miss" if shadow_scan else "memory")


def test_the_shell_and_nothing_else():
    f0, f2, info = _both(_shell_only)
    assert torch.equal(f0, f2)
    assert info["shape"].startswith("0,0,0,0,0,0,0,0,1,"), info


def test_scenes_of_one_shape_share_one_compile():
    a0, a2, ia = _both(_two_spheres(0.0))
    b0, b2, ib = _both(_two_spheres(0.25))
    assert ia["shape"] == ib["shape"]
    assert ia["cache"] == "miss" and ia["compile_ms"] > 0
    assert ib["cache"] == "memory" and ib["compile_ms"] == 0 and ib["compiles"] == ia["compiles"]
    assert torch.equal(a0, a2) and torch.equal(b0, b2) and not torch.equal(a0, b0)


def test_feature_planes_and_tile_lists_with_the_option_forced():
    r0, r2 = _renderer(scenes.lampshade, 0, w=96, h=64), _renderer(scenes.lampshade, 2, w=96, h=64)
    p0, p2 = r0.features_array(4), r2.features_array(4)
    for k in p0:
        assert torch.equal(torch.from_numpy(p0[k]), torch.from_numpy(p2[k])), k
    tiles = [4, 1, 3]                    # of 3 x 2
    o0, o2 = np.full((64 * 96, 3), 7.0), np.full((64 * 96, 3), 7.0)
    r0.sample_tiles_array(SPP, tiles, o0)
    r2.sample_tiles_array(SPP, tiles, o2)
    assert torch.equal(torch.from_numpy(o0), torch.from_numpy(o2)) and (o0 != 7.0).any() and (o0 == 7.0).any()
    info = r2.scan_jit_info()
    assert info["state"] == "active" and info["launches"] == 1, info      # (the feature pass has a kernel of its own)


def test_a_missing_compiler_leaves_the_aot_kernel(monkeypatch):
    monkeypatch.setenv("RPT_HIPRTC_LIB", "/nonexistent/libhiprtc.so")
    f0, f2, info = _both(scenes.lampshade, expect_state="fallback")
    assert torch.equal(f0, f2)
    assert "hiprtc not available" in info["reason"] and "/nonexistent/libhiprtc.so" in info["reason"], info


def test_cache_files_are_read_and_a_truncated_one_is_discarded(jit_cache):
    """Three spheres: a shape of this test's own.  Compiled and written; dropped from the process and read from the file; the file cut
    short: under the default policy the scene stays on the AOT kernel and says why, forced it compiles again."""
    lib = _lib.load()

    def make():
        sc, cam = _two_spheres(0.1)()
        sc.add(Object(sphere().scale(vec3(0.2, 0.2, 0.2)).translate(vec3(0.0, 0.8, 0.0))).material(Material.diffuse(vec3(0.5, 0.5, 0.5))))
        return sc, cam
    before = set(glob.glob(str(jit_cache / "*.co")))
    f0, f2, info = _both(make)
    assert info["cache"] == "miss" and torch.equal(f0, f2)
    new = set(glob.glob(str(jit_cache / "*.co"))) - before
    assert len(new) == 1 and not glob.glob(str(jit_cache / "*.tmp.*"))
    path = new.pop()
    assert lib.rpt_scan_jit_forget() >= 1
    r = _renderer(make, 1)               # the default policy uses a cached object at any size
    f = _frame(r)
    info = r.scan_jit_info()
    assert info["state"] == "active" and info["cache"] == "disk" and info["compile_ms"] == 0 and torch.equal(f, f0), info
    size = os.path.getsize(path)
    with open(path, "r+b") as fh:
        fh.truncate(size // 2)
    assert lib.rpt_scan_jit_forget() >= 1
    r = _renderer(make, 1)
    f = _frame(r)
    info = r.scan_jit_info()
    assert info["state"] == "idle" and info["launches"] == 0 and "cache file discarded" in info["reason"] and torch.equal(f, f0), info
    assert not os.path.exists(path)
    with open(path, "wb") as fh:
        fh.write(b"RPTJIT01" + b"\0" * 40)
    _, f2, info = _both(make)
    assert info["cache"] == "miss" and "cache file discarded" in info["reason"] and torch.equal(f2, f0), info
    assert os.path.getsize(path) == size                              # (written again, whole)


def _group_light():
    from tests.test_gpu_schedule import _group_light_scene
    return _group_light_scene()


def _mesh_tree():
    from tests.test_gpu_schedule import _two_torus_scene
    return _two_torus_scene(True)


@pytest.mark.parametrize("make,word", [(_group_light, "group"), (scenes.monomial_glass, "monomial"), (_mesh_tree, "tree")])
def test_flavours_outside_the_scope_attempt_nothing(make, word):
    compiles = _renderer(scenes.lampshade, 0).scan_jit_info()["compiles"]
    f0, f2, info = _both(make, expect_state="out_of_scope")
    assert torch.equal(f0, f2)
    assert word in info["reason"] and info["compiles"] == compiles and info["cache"] == "none", info


def test_the_default_policy_compiles_nothing_at_these_sizes():
    """Four spheres: a shape nothing has compiled and no cache holds."""
    def make():
        sc, cam = _two_spheres(0.2)()
        for x in (-0.3, 0.3):
            sc.add(Object(sphere().scale(vec3(0.2, 0.2, 0.2)).translate(vec3(x, 0.8, 0.0))).material(Material.diffuse(vec3(0.5, 0.5, 0.5))))
        return sc, cam
    r0, r1 = _renderer(make, 0), _renderer(make, 1)
    compiles = r0.scan_jit_info()["compiles"]
    assert r1.scan_jit_info()["state"] == "idle"                      # before any render
    f0, f1 = _frame(r0), _frame(r1)
    info = r1.scan_jit_info()
    assert info["state"] == "idle" and "threshold" in info["reason"] and info["compiles"] == compiles and info["launches"] == 0, info
    assert torch.equal(f0, f1)
    assert W * H * SPP < 2 ** 27
