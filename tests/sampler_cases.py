"""Cases of the per-call sampler tests (tests/test_gpu_device_samplers.py and their CPU counterparts in test_oracle_kat.py):
the light shapes, with what a test has to know about them because it built them -- which leaf a case lands on and that leaf's
composed matrix --, the sky images and the sky directions."""
import numpy as np

from rpt_amd import Environment, KdTree, Light, Material, Mesh, Object, Scene, cube, polygon, scenes, sphere, vec3
from rpt_amd.api import Sphere

LIGHT_COLOR, LIGHT_EMIT = vec3(1.0, 0.8, 0.6), 30.0


def _torus24():
    return Mesh(scenes.bumpy_torus(4, 3))


def fan_mesh(k):
    """k triangles around a raised centre, every vertex with a normal of its own (so Triangle::sample interpolates)."""
    ang = np.arange(k + 1) * (2 * np.pi / (k + 1.5))          # not closed: k triangles from k + 1 rim vertices
    rim = np.stack([np.cos(ang) * (0.8 + 0.1 * np.arange(k + 1)), 0.05 * np.arange(k + 1), np.sin(ang)], axis=1)
    c = np.array([0.0, 0.4, 0.0])
    nrm = lambda p: (p + [0.0, 1.5, 0.0]) / np.linalg.norm(p + [0.0, 1.5, 0.0])
    tris = [[c, rim[i + 1], rim[i], nrm(c), nrm(rim[i + 1]), nrm(rim[i])] for i in range(k)]
    return Mesh(np.array(tris))


def light_shapes():
    """id -> shape, cases A to G of the light-sampling tests."""
    quad = polygon([vec3(-1, 4.5, -1), vec3(1, 4.5, -1), vec3(1, 4.5, 1), vec3(-1, 4.5, 1)])
    inner2 = KdTree([cube().scale(vec3(.5, .3, .4)).translate(vec3(.3, 0, 0)),
                     sphere().scale(vec3(.2, .5, .3)).rotate_y(.6).translate(vec3(-.4, .1, 0))]).rotate_x(.3).translate(vec3(0, -.8, 0))
    inner1 = KdTree([sphere().scale(vec3(.4, .4, .4)).translate(vec3(-.6, 0, .2)), inner2]).scale(vec3(1.2, .8, 1)).translate(vec3(0, 1.5, 0))
    group = KdTree([sphere().translate(vec3(1.5, 0, 0)),
                    cube().scale(vec3(.05, 1, .8)).rotate_z(.7).translate(vec3(-1.5, .5, 0)),
                    _torus24().scale(vec3(.5, .5, .5)).translate(vec3(0, 0, 1.2)),
                    inner1]).rotate_y(.4).scale(vec3(1, 1, -1)).translate(vec3(0, 2, 0))
    return {
        "A": sphere(),
        "B": sphere().scale(vec3(.3, 1.2, .6)).rotate_x(.7).rotate_z(-.4).translate(vec3(.5, 1, -1)),
        "C": cube().scale(vec3(.6, .1, 1.5)).rotate_z(.3).rotate_y(1.1).translate(vec3(-2, 2.5, -.5)),
        "D": cube().scale(vec3(-.6, .4, 1)).rotate_y(.4).translate(vec3(1, 0, 0)),
        "E": quad,
        "F": _torus24().scale(vec3(.4, .9, .4)).rotate_x(.5).translate(vec3(0, 2.4, -1)),
        "G": group,
    }


def light_scene(shape, epsilon=False):
    sc = Scene()
    sc.add(Light.Object(Object(shape).material(Material.light(LIGHT_COLOR, LIGHT_EMIT))))
    if epsilon:
        sc.set_option("epsilon_policy", 1)
    return sc


def shared_table_scene(k, epsilon=False):
    """Case H: [Ambient, quad, mesh of k triangles]: 2 + k light triangles in one table."""
    sc = Scene()
    sc.add(Light.Ambient(vec3(0.05, 0.05, 0.05)))
    sc.add(Light.Object(Object(light_shapes()["E"]).material(Material.light(LIGHT_COLOR, LIGHT_EMIT))))
    sc.add(Light.Object(Object(fan_mesh(k).rotate_z(.2).translate(vec3(.5, -1.5, 0))).material(Material.light(LIGHT_COLOR, LIGHT_EMIT))))
    if epsilon:
        sc.set_option("epsilon_policy", 1)
    return sc


def positions(n, seed, extra=None):
    """Uniform in [-4, 4]^3, rounded to fp32 (the values both sides get), then `extra` rows."""
    p = np.random.default_rng(seed).uniform(-4.0, 4.0, size=(n, 3))
    if extra is not None:
        p = np.concatenate([p, extra])
    return p.astype(np.float32)


def structured_sphere_positions(seed):
    """For the bare unit sphere: local x exactly 0; x = z = 0 (straight above and below); on the +-x axis.  Never the centre."""
    rng = np.random.default_rng(seed)
    a = rng.uniform(-4.0, 4.0, size=(64, 3))
    a[:, 0] = 0.0
    a[::2, 0] = -0.0
    h = np.array([0.25, 0.9, 1.0, 1.5, 2.0, 3.0, 3.75, 4.0])
    z0 = np.zeros_like(h)
    b = np.concatenate([np.stack([z0, h, z0], 1), np.stack([z0, -h, z0], 1), np.stack([-z0, h, -z0], 1)])
    c = np.concatenate([np.stack([h, z0, z0], 1), np.stack([-h, z0, z0], 1)])
    return np.concatenate([a, b, c])


def sphere_leaf_matrices(shape, seed, n, rng_u32):
    """For every case 0..n-1: the composed matrix of the leaf the case samples if that leaf is a sphere, else None.  The leaf of a
    group follows from replaying the index draws, (word * count) >> 32 on the case's stream (rng_u32(seed, case, sample, n))."""
    out = []
    for i in range(n):
        m, s, k, words = np.eye(4), shape, 0, None
        while True:
            if s.matrix() is not None:
                m = m @ s.matrix()
            b = s.base()
            if not isinstance(b, KdTree):
                break
            if words is None:
                words = rng_u32(seed, i, 0, 8)
            s = b.shapes[(int(words[k]) * len(b.shapes)) >> 32]
            k += 1
        out.append(m if isinstance(b, Sphere) else None)
    return out


# ------------------------------------------------------------------ sky
def sky_images():
    rng = np.random.default_rng(11)
    ramp = np.zeros((4, 8, 3))
    ramp[..., 0] = np.arange(8)[None, :]          # first and last column differ: the seam shows
    ramp[..., 1] = np.arange(4)[:, None]
    ramp[..., 2] = 0.5
    imgs = {"1x1": rng.uniform(0.1, 2.0, (1, 1, 3)), "1x5": rng.uniform(0.1, 2.0, (5, 1, 3)), "6x1": rng.uniform(0.1, 2.0, (1, 6, 3)),
            "2x2": rng.uniform(0.1, 2.0, (2, 2, 3)), "7x5": rng.uniform(0.1, 2.0, (5, 7, 3)), "64x32": rng.uniform(0.0, 4.0, (32, 64, 3)),
            "ramp8x4": ramp}
    return imgs                                    # name "WxH" -> (H, W, 3)


def sky_scene(img, epsilon=False):
    sc = Scene()
    sc.environment = Environment.Hdri(img.shape[1], img.shape[0], img.reshape(-1, 3))
    if epsilon:
        sc.set_option("epsilon_policy", 1)
    return sc


def sky_directions():
    """Unnormalised directions of length 0.1 to 10, rounded to fp32: random ones, the poles with every sign of zero, near-pole tilts,
    both sides of the azimuth seam (-X, z = +-0 ... +-1e-1) and the texel centres of a 7 x 5 image."""
    rng = np.random.default_rng(5)
    d = [rng.normal(size=(4096, 3))]
    for y in (1.0, -1.0):
        d.append(np.array([[0.0, y, 0.0]]))
        d.append(np.array([[sx * 0.0, y, sz * 0.0] for sx in (1.0, -1.0) for sz in (1.0, -1.0)]))
        tilt = 10.0 ** np.arange(-7.0, -0.5, 0.5)
        ang = rng.uniform(0, 2 * np.pi, tilt.size)
        d.append(np.stack([tilt * np.cos(ang), np.full(tilt.size, y), tilt * np.sin(ang)], 1))
    zs = np.concatenate([[0.0], 10.0 ** np.arange(-30.0, 0.0, 1.0)])
    for s in (1.0, -1.0):
        for y in (0.0, 0.3, -0.8):
            d.append(np.stack([np.full(zs.size, -1.0), np.full(zs.size, y), s * zs], 1))
    w, h = 7, 5
    az = np.arange(w) / (w - 1) * 2 * np.pi - np.pi
    po = np.arange(h) / (h - 1) * np.pi
    aa, pp = np.meshgrid(az, po)
    d.append(np.stack([np.sin(pp) * np.cos(aa), np.cos(pp), np.sin(pp) * np.sin(aa)], -1).reshape(-1, 3))
    d = np.concatenate(d)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d *= 10.0 ** rng.uniform(-1.0, 1.0, (d.shape[0], 1))
    return d.astype(np.float32)
