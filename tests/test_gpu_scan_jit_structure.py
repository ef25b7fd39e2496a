"""The scan JIT's second constant block: the scene's structure (lights, staged tables, material kinds, medium kind, HDRI, box pairs'
common slabs; rpt_scan_jit_structure, "structure" in Renderer.scan_jit_info()).

The specialised kernel makes at compile time the choices the AOT kernel makes at run time, on the same records in the same order, so
every frame here is compared bit for bit (torch.equal) between "scan_jit" = 2 (always) and 0 (never), at 64x64x8.  Every case also
asserts, through the query, which kernel ran and which structure it was compiled with: a frame that equals the AOT frame because the
AOT kernel rendered both proves nothing, and a code object keyed too coarsely would be reused where it must not be.

The cache directory is the module's own (RPT_JIT_CACHE).  Code objects other modules compiled earlier in the process are found in
memory, so "miss" is asserted only for structures that are this module's own."""
import os
import re

import numpy as np
import pytest
import torch

from rpt_amd import Camera, Environment, Light, Material, Medium, Object, Renderer, Scene, cube, polygon, scenes, sphere, vec3

pytestmark = pytest.mark.gpu

W = H = 64
SPP = 8
ALL = "groups=lights+tables+mats+pairs"                    # the default block; "small" (medium kind, no HDRI) is a switch


@pytest.fixture(scope="module", autouse=True)
def jit_cache(tmp_path_factory):
    old = {k: os.environ.get(k) for k in ("RPT_JIT_CACHE", "RPT_HIPRTC_LIB", "RPT_SCAN_STRUCT_GROUPS")}
    os.environ["RPT_JIT_CACHE"] = str(tmp_path_factory.mktemp("scan_jit_structure_cache"))
    os.environ.pop("RPT_HIPRTC_LIB", None)
    os.environ.pop("RPT_SCAN_STRUCT_GROUPS", None)
    yield
    for k, v in old.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v


def _renderer(make, jit, **options):
    out = make()
    scene, cam = out[0], out[1]
    mb = out[2]["max_bounces"] if len(out) > 2 else 3
    scene.set_option("scan_jit", jit)
    for k, v in options.items():
        scene.set_option(k, v)
    return Renderer(scene, cam).width(W).height(H).max_bounces(mb).seed(1)


def _frame(r):
    return torch.from_numpy(np.ascontiguousarray(r.sample_array(SPP)))


def _both(make, **options):
    """-> (frame with scan_jit = 0, frame with 2, query of the second, its structure as a dict); asserts which kernel ran."""
    r0, r2 = _renderer(make, 0, **options), _renderer(make, 2, **options)
    f0, f2 = _frame(r0), _frame(r2)
    i0, i2 = r0.scan_jit_info(), r2.scan_jit_info()
    print("scan_jit 2:", i2)
    assert i0["state"] == "off" and i0["launches"] == 0
    assert i2["state"] == "active" and i2["launches"] == 1 and 0 < i2["vgprs"] <= i2["aot_vgprs"] <= 80, i2
    assert i0["structure"] == i2["structure"]                          # (the structure is the commit's, whatever the option)
    assert torch.isfinite(f0).all() and f0.mean() > 0
    return f0, f2, i2, dict(kv.split("=", 1) for kv in i2["structure"].split(";"))


# ---- 1. C3 and C2
QUAD_LIGHT = "1:object/mesh/twin/60000000-60000000"      # the quad on the ceiling: a mesh light whose twin is rectangle record 0


@pytest.mark.parametrize("max_blocks", [0, 1])
def test_c3(max_blocks):
    """... on the default grid and (case 8) on one block, where every lane pulls many items."""
    f0, f2, info, _ = _both(scenes.lampshade, max_blocks=max_blocks)
    assert torch.equal(f0, f2)
    assert info["shape"] == "0,2,0,4,0,1,0,0,1,1,0x0ull,0x3ull;medium=1"
    assert info["structure"] == ALL + ";lights=" + QUAD_LIGHT + ";mats=0x1;medium_kind=view;hdri=view;pairs=0x1e"
    assert info["scratch"] <= 24                                       # the resource rule: no more than the shape block alone (80 VGPRs / 24 B)
    if max_blocks:
        assert info["cache"] == "memory"


def test_c2():
    f0, f2, info, _ = _both(scenes.cornell)
    assert torch.equal(f0, f2)
    assert info["shape"] == "1,1,0,0,0,1,0,0,1,1,0x1ull,0x1ull;medium=0"
    assert info["structure"] == ALL + ";lights=" + QUAD_LIGHT + ";mats=0x1;medium_kind=view;hdri=view;pairs=0x0"
    assert info["scratch"] == 0


# ---- 2. two object lights of different shapes with an ambient light between them
def _two_lights(fog):
    def make():
        sc = Scene()
        grey = Material.diffuse(vec3(0.7, 0.7, 0.7))
        sc.add(Object(polygon([vec3(-4, -1, -4), vec3(-4, -1, 4), vec3(4, -1, 4), vec3(4, -1, -4)])).material(grey))
        sc.add(Object(sphere().scale(vec3(0.6, 0.6, 0.6)).translate(vec3(-0.8, -0.4, 0.0))).material(Material.diffuse(vec3(0.8, 0.4, 0.3))))
        sc.add(Object(cube().scale(vec3(0.7, 0.7, 0.7)).rotate_y(0.5).translate(vec3(1.0, -0.65, 0.4))).material(grey))
        # a tilted pentagon: a fan of three triangles (a count that is no power of two), no rectangle
        fan = polygon([vec3(-0.6, 2.4, -0.3), vec3(0.0, 2.6, -0.7), vec3(0.6, 2.5, -0.2), vec3(0.4, 2.3, 0.5), vec3(-0.4, 2.2, 0.4)])
        assert fan.tris.shape[0] == 3
        glow, warm = Material.light(vec3(1.0, 0.95, 0.9), 25.0), Material.light(vec3(1.0, 0.6, 0.3), 30.0)
        sc.add(Object(fan.clone()).material(glow))
        sc.add(Light.Object(Object(fan.clone()).material(glow)))
        sc.add(Light.Ambient(vec3(0.05, 0.05, 0.08)))
        lamp = cube().scale(vec3(0.3, 0.2, 0.4)).rotate_y(0.7).translate(vec3(2.2, 0.6, 1.0))
        sc.add(Object(lamp.clone()).material(warm))
        sc.add(Light.Object(Object(lamp.clone()).material(warm)))
        if fog:
            sc.add(Medium.homogeneous_isotropic(0.02, 0.06))
        return sc, Camera.look_at(vec3(0.0, 1.2, 6.0), vec3(0.0, 0.3, 0.0), vec3(0, 1, 0), 0.9)
    return make


@pytest.mark.parametrize("fog", [True, False])
def test_two_light_shapes_around_an_ambient_light(fog):
    f0, f2, info, st = _both(_two_lights(fog))
    assert torch.equal(f0, f2)
    assert info["shape"].endswith(";medium=1" if fog else ";medium=0")
    assert info["cache"] == "miss"           # in fog and without: alike in every count and field, two instantiations, two code objects
    assert st["groups"] == ALL.split("=")[1]
    # a mesh light of three triangle records (codes 0x3000000k), the ambient light, a transformed cube light whose twin is cube record 1
    assert re.fullmatch(r"3:object/mesh/twin/([0-9a-f]+)-([0-9a-f]+)\|ambient\|object/cube/xf/twin/10000001-10000001", st["lights"]), st
    lo, hi = (int(x, 16) for x in re.match(r"3:object/mesh/twin/([0-9a-f]+)-([0-9a-f]+)", st["lights"]).groups())
    assert (lo, hi) == (0x30000000, 0x30000002)


# ---- 3. and 4. material kinds; values
def _balls(kinds, shift=0.0):
    """Four spheres over a floor quad under a quad light; `kinds`: their materials."""
    def make():
        sc = Scene()
        sc.add(Object(polygon([vec3(-4, -1, -4), vec3(-4, -1, 4), vec3(4, -1, 4), vec3(4, -1, -4)])).material(Material.diffuse(vec3(0.7 - shift, 0.7, 0.7))))
        for i, m in enumerate(kinds):
            sc.add(Object(sphere().scale(vec3(0.45 + shift, 0.45, 0.45)).translate(vec3(-1.8 + 1.2 * i + shift, -0.55, 0.3 * (i % 2)))).material(m))
        for x in (-2.5, 2.5 + shift):                                   # a pair of boxes with common y and z slabs
            sc.add(Object(cube().scale(vec3(0.3, 1.2 + shift, 0.3)).translate(vec3(x, -0.4, -1.5))).material(Material.diffuse(vec3(0.4, 0.5 + shift, 0.6))))
        quad = [vec3(1.0 + shift, 3.0, -1.0), vec3(1.0 + shift, 3.0, 1.0), vec3(-1.0, 3.0, 1.0), vec3(-1.0, 3.0, -1.0)]
        sc.add((polygon(quad), Material.light(vec3(1, 1 - shift, 1), 40.0 + 10.0 * shift)))
        sc.add(Medium.homogeneous_isotropic(0.02, 0.05))
        return sc, Camera.look_at(vec3(0.0, 1.0, 6.0), vec3(0.0, 0.0, 0.0), vec3(0, 1, 0), 0.8)
    return make


def _four_kinds():
    return [Material.diffuse(vec3(0.8, 0.4, 0.3)), Material.specular(vec3(0.6, 0.8, 0.9), 8.0), Material.mirror(), Material.clear(1.5)]


def _lambertian():
    return [Material.diffuse(vec3(0.8, 0.4, 0.3)), Material.diffuse(vec3(0.6, 0.8, 0.9)), Material.diffuse(vec3(0.2, 0.7, 0.3)), Material.diffuse(vec3(0.9, 0.9, 0.2))]


def test_material_kinds_key_the_code_object():
    """One shape, two structures, two compiles: the Lambertian-only object has no Phong, mirror or glass code and must not serve the other."""
    a0, a2, ia, sa = _both(_balls(_four_kinds()))
    b0, b2, ib, sb = _both(_balls(_lambertian()))
    assert ia["shape"] == ib["shape"] and ia["structure"] != ib["structure"]
    assert (sa["mats"], sb["mats"]) == ("0xf", "0x1") and {k for k in sa if sa[k] != sb[k]} == {"mats"}
    assert ia["cache"] == "miss" and ib["cache"] == "miss" and ib["compiles"] == ia["compiles"] + 1
    assert torch.equal(a0, a2) and torch.equal(b0, b2) and not torch.equal(a0, b0)
    c0, c2, ic, _ = _both(_balls(_four_kinds()))                        # ... and back: the first object again
    assert ic["cache"] == "memory" and ic["compiles"] == ib["compiles"] and torch.equal(c2, a0) and torch.equal(c0, a0)


def test_values_are_not_part_of_the_structure():
    """Other colours, light size and power, sphere and box sizes and places: one compile."""
    a0, a2, ia, _ = _both(_balls(_lambertian()))
    b0, b2, ib, _ = _both(_balls(_lambertian(), shift=0.25))
    assert ia["shape"] == ib["shape"] and ia["structure"] == ib["structure"]
    assert ib["cache"] == "memory" and ib["compile_ms"] == 0 and ib["compiles"] == ia["compiles"]
    assert torch.equal(a0, a2) and torch.equal(b0, b2) and not torch.equal(a0, b0)


# ---- 5. a thin-lens camera and an HDRI environment
def _lens_and_sky():
    sc, _ = _balls(_four_kinds())()
    sc.media.clear()                                                    # no fog: rays leave the scene and read the sky
    rng = np.random.default_rng(7)
    sc.environment = Environment.Hdri(8, 4, 0.2 + rng.random((4, 8, 3)))
    cam = Camera.look_at(vec3(0.0, 1.0, 6.0), vec3(0.0, 0.0, 0.0), vec3(0, 1, 0), 0.8).focus(vec3(0.0, -0.5, 0.0), 0.2)
    return sc, cam


def test_aperture_and_hdri():
    f0, f2, info, st = _both(_lens_and_sky)
    assert torch.equal(f0, f2)
    assert st["hdri"] == "view" and st["mats"] == "0xf" and info["shape"].endswith(";medium=0")


def test_aperture_and_hdri_with_every_group(monkeypatch):
    """... and with the group outside the default switched on: only the absence of an HDRI is a constant, so this scene still asks the view."""
    monkeypatch.setenv("RPT_SCAN_STRUCT_GROUPS", "31")
    f0, f2, info, st = _both(_lens_and_sky)
    assert torch.equal(f0, f2)
    assert st["hdri"] == "1" and st["medium_kind"] == "0" and st["groups"] == "lights+tables+mats+small+pairs"


# ---- 6. both shadow forms of one code object
@pytest.mark.parametrize("shadow_scan", [1, 0])
def test_both_shadow_forms_in_one_code_object(shadow_scan):
    from tests.test_gpu_scan_jit import _every_kind
    f0, f2, info, st = _both(_every_kind, shadow_scan=shadow_scan)
    assert torch.equal(f0, f2)
    assert st["lights"] == "1:object/sphere/xf/twin/1-1" and st["mats"] == "0x3", st       # the lamp is sphere record 1; Lambertian and Phong
    if not shadow_scan:
        assert info["cache"] == "memory"                                # the per-light mark is data: no second compile


# ---- 7. more lights than the block describes
def _six_lights():
    sc, cam = _balls(_lambertian())()
    for i in range(5):
        sc.add(Light.Ambient(vec3(0.01 * (i + 1), 0.01, 0.01)))
    return sc, cam


def test_more_lights_than_the_cap_read_from_the_view():
    f0, f2, info, st = _both(_six_lights)
    assert torch.equal(f0, f2)
    assert st["lights"] == "view" and st["groups"] == "tables+mats+pairs" and st["mats"] == "0x1", st
