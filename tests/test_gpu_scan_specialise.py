"""The commit-time scan specialisation (option "scan_specialise": to_local_y for records rotated about the vertical axis,
common slabs of adjacent boxes computed once) drops only terms that are exactly zero and operations on identical operands: every
closest hit -- parameter, object and normal -- and every frame must be the same BITS with the option on and off.

The rays: 2^20 random ones (half from outside the scene, half from inside it), rays with one and with two zero direction components
(both signs of the zero: the one thing the dropped terms can change is the sign of a zero in the local direction), rays that start
on a face of every transformed cube / sphere / box, and rays through points of the cubes' and boxes' edges."""
import numpy as np
import pytest

from rpt_amd import Camera, Material, Object, Renderer, Scene, cube, polygon, scenes, sphere, vec3
from rpt_amd.api import Cube, Sphere, Transformed

pytestmark = pytest.mark.gpu

N_RANDOM = 1 << 20


def _mixed():
    """One cube about y, one about x, a sphere about y (and a box, a floor and a light so that it renders)."""
    sc = Scene()
    grey = Material.diffuse(vec3(0.7, 0.7, 0.7))
    sc.add(Object(cube().scale(vec3(2.0, 3.0, 1.0)).rotate_y(0.4).translate(vec3(1.0, 1.5, 3.0))).material(grey))
    sc.add(Object(cube().scale(vec3(2.0, 3.0, 1.0)).rotate_x(0.4).translate(vec3(-4.0, 2.0, 3.0))).material(grey))
    sc.add(Object(sphere().scale(vec3(1.0, 2.0, 1.0)).rotate_y(1.1).translate(vec3(0.0, 2.0, -2.0))).material(grey))
    sc.add(Object(cube().scale(vec3(1.0, 1.0, 1.0)).translate(vec3(4.0, 0.5, -1.0))).material(grey))
    sc.add(Object(polygon([vec3(-8.0, 0.0, -8.0), vec3(-8.0, 0.0, 8.0), vec3(8.0, 0.0, 8.0), vec3(8.0, 0.0, -8.0)])).material(grey))
    lamp = polygon([vec3(1.0, 7.0, -1.0), vec3(1.0, 7.0, 1.0), vec3(-1.0, 7.0, 1.0), vec3(-1.0, 7.0, -1.0)])
    sc.add((lamp, Material.light(vec3(1.0, 1.0, 1.0), 40.0)))
    return sc


def _scene(name):
    if name == "mixed":
        return _mixed(), Camera(), np.array([0.0, 2.0, 0.5]), 9.0
    scene, cam, _ = scenes.CONFIGS[name]()
    return scene, cam, np.array([278.0, 274.0, 280.0]), 700.0


def _unit(v):
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _rays(scene, center, radius):
    rng = np.random.default_rng(77)
    os_, ds_ = [], []

    def add(o, d):
        os_.append(np.asarray(o, dtype=np.float64).reshape(-1, 3))
        ds_.append(np.asarray(d, dtype=np.float64).reshape(-1, 3))

    # random: from a sphere around the scene at its inside, and from points inside it in any direction
    n = N_RANDOM // 2
    d = _unit(rng.normal(size=(n, 3)))
    o = center + radius * d
    add(o, _unit(center + rng.uniform(-0.6, 0.6, size=(n, 3)) * radius - o))
    add(center + rng.uniform(-0.45, 0.45, size=(n, 3)) * radius, _unit(rng.normal(size=(n, 3))))
    # one and two zero direction components, +0 and -0
    m = 1 << 14
    for zero in (0.0, -0.0):
        for axis in range(3):
            d = rng.normal(size=(m, 3))
            d[:, axis] = zero
            add(center + rng.uniform(-0.45, 0.45, size=(m, 3)) * radius, _unit(d))
            for sign in (1.0, -1.0):
                d = np.full((m, 3), zero)
                d[:, axis] = sign
                add(center + rng.uniform(-0.45, 0.45, size=(m, 3)) * radius, d)
    # the transformed unit shapes: rays that start on a face / the surface, and rays through points of the cubes' edges
    for ob in scene.objects:
        sh = ob.shape
        if not (isinstance(sh, Transformed) and isinstance(sh.base(), (Cube, Sphere))):
            continue
        M = np.asarray(sh.matrix(), dtype=np.float64)
        world = lambda p: p @ M[:3, :3].T + M[:3, 3]
        k = 1 << 12
        if isinstance(sh.base(), Cube):
            p = rng.uniform(-0.5, 0.5, size=(k, 3))
            p[np.arange(k), rng.integers(0, 3, k)] = rng.choice([-0.5, 0.5], k)            # on a face
            e = rng.uniform(-0.5, 0.5, size=(k, 3))
            ax = rng.integers(0, 3, k)
            e[np.arange(k), ax] = rng.choice([-0.5, 0.5], k)
            e[np.arange(k), (ax + 1) % 3] = rng.choice([-0.5, 0.5], k)                     # on an edge
            eo = center + radius * _unit(rng.normal(size=(k, 3)))
            add(eo, _unit(world(e) - eo))
            # along an edge's own face planes: the direction of one local axis through a point of a parallel edge
            add(world(e) - 3.0 * radius * _unit(M[:3, (ax + 2) % 3].T), _unit(M[:3, (ax + 2) % 3].T))
        else:
            p = _unit(rng.normal(size=(k, 3)))                                              # the unit sphere's surface
        add(world(p), _unit(rng.normal(size=(k, 3))))
        add(world(p), _unit(world(rng.uniform(-0.5, 0.5, size=(k, 3))) - world(p)))         # ... and into the shape
    return np.concatenate(os_).astype(np.float32), np.concatenate(ds_).astype(np.float32)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("name", ["C3", "C2", "mixed"])
def test_closest_hits_are_bit_equal_with_the_option_on_and_off(name):
    res = {}
    for on in (1, 0):
        scene, cam, center, radius = _scene(name)
        scene.set_option("scan_specialise", on)
        o, d = _rays(scene, center, radius)
        assert o.shape[0] >= N_RANDOM
        r = Renderer(scene, cam)
        assert r.scene_stats()["scene_bvh"] == 0                 # the linear scan is what is under test
        res[on] = r.get_closest_hit(o, d)
    (t1, o1, n1), (t0, o0, n0) = res[1], res[0]
    hit = o0 >= 0
    print(f"{name}: {o.shape[0]} rays, {int(hit.sum())} hits, objects hit: {sorted(set(o0[hit].tolist()))}")
    assert hit.mean() > 0.5 and len(set(o0[hit].tolist())) >= 4
    assert np.array_equal(o1, o0)
    assert np.array_equal(_bits(t1), _bits(t0))
    assert np.array_equal(_bits(n1), _bits(n0))


@pytest.mark.parametrize("name", ["C3", "C2"])
def test_frames_are_equal_with_the_option_on_and_off(name):
    imgs = {}
    for on in (1, 0):
        scene, cam, cfg = scenes.CONFIGS[name]()
        scene.set_option("scan_specialise", on)
        imgs[on] = Renderer(scene, cam).width(128).height(128).max_bounces(cfg["max_bounces"]).seed(3).sample_array(16)
    assert np.all(np.isfinite(imgs[1])) and imgs[1].mean() > 0
    assert np.array_equal(imgs[1], imgs[0])
