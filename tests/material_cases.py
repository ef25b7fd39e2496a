"""Cases of the per-call material, bounce and camera tests (tests/test_gpu_device_materials.py, and their CPU counterparts in
test_oracle_kat.py): the materials, their (n, wo) inputs -- random ones and a table of structured ones --, the bsdf inputs, the
cameras, and what the reference alone says about which decisions fp32 cannot be asked to reproduce (the flags).  Nothing here looks
at the device."""
import ctypes as C
import functools
import math

import numpy as np

from oracle import pyoracle
from rpt_amd import Camera, Light, Material, Object, Scene, cube, plane, polygon, sphere, vec3

N, SEED = 4096, 7
ALBEDO = vec3(0.7, 0.5, 0.3)
EPS64 = 2.220446049250313e-16          # f64::EPSILON: nalgebra's rotation_between rotates only when |a x b| exceeds it


def materials():
    m = {"lambertian": Material.diffuse(ALBEDO)}
    for s in (0, 1, 6, 50, 1000):
        m[f"phong{s}"] = Material.specular(ALBEDO, float(s))
    m["mirror"] = Material.mirror()
    for name, ior in (("1.0", 1.0), ("1.05", 1.05), ("1.5", 1.5), ("2.4", 2.4), ("1over1.5", 1 / 1.5)):
        m[f"glass{name}"] = Material.transmissive(ior)
    return m


MATERIAL_NAMES = list(materials())
POLE_A = [1e-3, 1e-5, 1e-7, 1e-10, math.sin(math.pi), 1e-17, 1e-20, 1e-30]
POLE_A64 = [2.2e-16, 2.3e-16, 1e-200]          # both sides of the reference's threshold, and far below fp32's range
# Structured cases that sit on a decision's boundary on purpose (label prefix -> why); every other structured case must be unflagged.
BOUNDARY = {
    "k=+1e-06": "Snell's k placed at +1e-6, inside the |k| < 1e-5 flag",
    "k=-1e-06": "Snell's k placed at -1e-6, inside the |k| < 1e-5 flag",
    "wo.n=1e-06": "n.wo placed at the width of the bsdf flag (|n.wo| < 1e-6 after fp32 rounding, or not)",
    "ci=0": "n.wo = 0 exactly (axis vectors: the products are exact in every precision, the sign of zero decides)",
    "tangent": "n.wi or n.wo = +-0 exactly (axis normals: the products are exact in every precision, the sign of zero decides)",
}
BOUNDARY_OF = {("glass1.0", "wo.n=0.001"): "at ior 1 Snell's k is ci^2: 1e-6 here, inside the |k| < 1e-5 flag"}
EXACT_ZERO = ("ci=0", "tangent")                # flagged by the widths, yet decided exactly: compared like unflagged cases


def _unit(v):
    v = np.asarray(v, dtype=np.float64)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _tangent(n, rng):
    t = np.cross(n, rng.normal(size=3))
    return t / np.linalg.norm(t)


def _material_seed(name):
    return sum(map(ord, name))


def random_inputs(name):
    """N random unit (n, wo): above the surface for the opaque materials, on both sides for glass."""
    rng = np.random.default_rng(_material_seed(name))
    n, wo = _unit(rng.normal(size=(N, 3))), _unit(rng.normal(size=(N, 3)))
    if not name.startswith("glass"):
        wo = np.where((np.einsum("ij,ij->i", wo, n) < 0)[:, None], -wo, wo)
    return n, wo


def pole_vectors(f64):
    """(label, vector) of the pole family, as given: not normalised."""
    out = []
    for a in POLE_A + (POLE_A64 if f64 else []):
        for s in (1.0, -1.0):
            out += [(f"({a:g},{s:+g},0)", (a, s, 0.0)), (f"(0,{s:+g},{a:g})", (0.0, s, a)), (f"({a:g},{s:+g},-{a:g})", (a, s, -a))]
    return out


def structured_inputs(name, f64):
    """-> list of (label, n, wo).  See the module docstring of tests/test_gpu_device_materials.py for what each family is for."""
    rng = np.random.default_rng(1000 + _material_seed(name))
    mat = materials()[name]
    glass = mat.kind == Material.TRANSMISSIVE
    out = []
    axes = [np.roll([s, 0.0, 0.0], k) for k in range(3) for s in (1.0, -1.0)]
    for n in axes:                                                  # the six axis normals
        t1, t2 = np.roll(n, 1), np.roll(n, 2)
        wo = _unit(n + 0.5 * np.abs(t1) + 0.3 * np.abs(t2))
        out.append((f"axis{tuple(int(c) for c in n)}", n, wo))
        if glass:
            out.append((f"axis{tuple(int(c) for c in n)}inside", n, -wo))
    for label, v in pole_vectors(f64):                              # normals next to +-Y (Lambertian rotates +Y onto n)
        out.append((f"pole n={label}", np.array(v), _unit([0.3, 0.8 * v[1], 0.52])))
    for _ in range(8):                                              # wo = n, and grazing wo
        n = _unit(rng.normal(size=3))
        out.append(("wo=n", n, n.copy()))
        for c in (1e-3, 1e-6):
            out.append((f"wo.n={c:g}", n, math.sqrt(1 - c * c) * _tangent(n, rng) + c * n))
    if mat.kind == Material.PHONG:                                  # mirror direction +-Y and next to it (Phong rotates +Y onto it)
        for s in (1.0, -1.0):
            n = np.array([0.0, s, 0.0])
            out.append((f"mirror=(0,{s:+g},0)", n, n.copy()))
        for label, v in pole_vectors(f64):                          # n = +-Y, n.wo = 1: the mirror direction is (-a, +-1, ...) exactly
            out.append((f"pole mirror wo={label}", np.array([0.0, v[1], 0.0]), np.array(v)))
    if glass:
        ior = mat.ior
        for _ in range(8):
            n = _unit(rng.normal(size=3))
            out.append(("wo=-n", n, -n))
        for n in axes:                                              # ci = 0 exactly
            out.append(("ci=0", n, np.abs(np.roll(n, 1))))
        # Snell's k = 1 - eta^2 (1 - ci^2) at +-1e-3 and +-1e-6, from the side where eta >= 1 (inside for ior >= 1, outside below;
        # the other side has k > 0 everywhere, and at ior = 1 k = ci^2, so only the positive targets exist), 16 streams each
        eta = max(ior, 1.0 / ior)
        for k in (1e-3, -1e-3, 1e-6, -1e-6):
            ci2 = 1.0 - (1.0 - k) / (eta * eta)
            if not 0.0 <= ci2 <= 1.0:
                continue
            ci = math.sqrt(ci2)
            for _ in range(16):
                n = _unit(rng.normal(size=3))
                w = ci * n + math.sqrt(1.0 - ci2) * _tangent(n, rng)
                out.append((f"k={k:+g}", n, -w if ior >= 1.0 else w))
    return out


@functools.lru_cache(maxsize=None)
def inputs(name, f64):
    """-> n, wo (m, 3) float64 as both sides get them (rounded to fp32 unless f64), labels (m; '' for the random cases)."""
    n, wo = random_inputs(name)
    st = structured_inputs(name, f64)
    n = np.concatenate([n, np.array([s[1] for s in st])])
    wo = np.concatenate([wo, np.array([s[2] for s in st])])
    labels = np.array([""] * N + [s[0] for s in st])
    if not f64:
        n, wo = n.astype(np.float32).astype(np.float64), wo.astype(np.float32).astype(np.float64)
    for a in (n, wo, labels):
        a.setflags(write=False)
    return n, wo, labels


def is_boundary(labels, name=None):
    return np.array([any(l.startswith(p) for p in BOUNDARY) or (name, str(l)) in BOUNDARY_OF for l in labels])


def is_exact_zero(labels):
    return np.array([any(l.startswith(p) for p in EXACT_ZERO) for l in labels])


# ------------------------------------------------------------------ what the reference's formulas say (numpy, fp64)
def uniforms(seed, n_cases, count, sample=0):
    """The first `count` uniforms of streams (seed, i, sample), i < n_cases: (n_cases, count).  The oracle's uniform keeps the 23
    bits the device's does, so these are the device's draws too."""
    out = np.empty((n_cases, count))
    L = pyoracle.lib()
    for i in range(n_cases):
        L.orc_rng_uniform(C.c_uint64(seed), i, sample, count, out[i].ctypes.data_as(C.c_void_p))
    return out


def glass_terms(n, wo, ior):
    """Material::sample_f's Transmissive arm up to the decisions (src/material.rs:222-261): inside, ci, sr, eta, k, nn."""
    d = np.einsum("ij,ij->i", n, wo)
    inside = d < 0.0
    nn = np.where(inside[:, None], -n, n)
    ci = np.clip(np.einsum("ij,ij->i", wo, nn), 0.0, 1.0)
    ni, nt = np.where(inside, ior, 1.0), np.where(inside, 1.0, ior)
    r0 = ((ni - nt) / (ni + nt)) ** 2
    sr = np.clip(r0 + (1.0 - r0) * (1.0 - ci) ** 5, 0.0, 1.0)
    eta = ni / nt
    k = 1.0 - eta * eta * (1.0 - ci * ci)
    return dict(inside=inside, ci=ci, sr=sr, eta=eta, k=k, nn=nn)


def glass_outcomes(n, wo, ior):
    """The two directions the Transmissive arm can return: the mirror direction, and the refracted one with cos_t = sqrt(max(k, 0))."""
    g = glass_terms(n, wo, ior)
    reflect = 2.0 * np.einsum("ij,ij->i", n, wo)[:, None] * n - wo
    cos_t = np.sqrt(np.maximum(g["k"], 0.0))
    refract = g["eta"][:, None] * -wo + (g["eta"] * g["ci"] - cos_t)[:, None] * g["nn"]
    return reflect, refract, g


def sample_flags(name, n, wo, seed=SEED):
    """Cases whose sample_f decisions fp32 cannot be asked to reproduce (glass only): -> dict of `u_sr` (|u - sr| < 4e-6:
    reflect or not) and `k` (|k| < 1e-5: refract or None), from the reference's formulas and draws alone."""
    m = n.shape[0]
    none = np.zeros(m, bool)
    mat = materials()[name]
    if mat.kind != Material.TRANSMISSIVE:
        return dict(u_sr=none, k=none.copy())
    g = glass_terms(n, wo, mat.ior)
    u = uniforms(seed, m, 1)[:, 0]
    return dict(u_sr=np.abs(u - g["sr"]) < 4e-6, k=np.abs(g["k"]) < 1e-5)


def lobe_cosine(name, r2):
    """ct, st of the lobe direction sample_f draws from r2: Lambertian sqrt(r2), Phong r2^(1 / (shininess + 1)); ones elsewhere."""
    mat = materials()[name]
    if mat.kind == Material.LAMBERTIAN:
        ct = np.sqrt(r2)
    elif mat.kind == Material.PHONG:
        ct = np.power(r2, 1.0 / (mat.shininess + 1.0))
    else:
        ct = np.ones_like(r2)
    return ct, np.sqrt(np.maximum(1.0 - ct * ct, 0.0))


def sample_pdf(name, r2):
    """The pdf sample_f returns for the draw r2 (src/material.rs:173-220): cos(theta) / pi, (s + 1) / 2 pi cos(theta)^s, or 1."""
    mat = materials()[name]
    ct, _ = lobe_cosine(name, r2)
    if mat.kind == Material.LAMBERTIAN:
        return ct / math.pi
    if mat.kind == Material.PHONG:
        return (mat.shininess + 1.0) / (2.0 * math.pi) * np.power(ct, mat.shininess)
    return np.ones_like(r2)


def bsdf_flags(n, wo, wi):
    """|n.wi| or |n.wo| < 1e-6: the sign tests of Material::bsdf."""
    return (np.abs(np.einsum("ij,ij->i", n, wi)) < 1e-6) | (np.abs(np.einsum("ij,ij->i", n, wo)) < 1e-6)


def phong_cosine(n, wo, wi):
    """The lobe cosine of Material::bsdf's Phong arm: clamp(dot(-normalize(reflect(wi, n)), wo), 0, 1)."""
    r = wi - 2.0 * np.einsum("ij,ij->i", n, wi)[:, None] * n
    r = -r / np.linalg.norm(r, axis=1, keepdims=True)
    return np.clip(np.einsum("ij,ij->i", r, wo), 0.0, 1.0)


def bsdf_unsigned(name, n, wo, wi):
    """Material::bsdf where both sign tests pass, whatever the signs are: the other outcome of a flagged case (the first is zero)."""
    mat = materials()[name]
    m = n.shape[0]
    if mat.kind == Material.LAMBERTIAN:
        return np.broadcast_to(mat.albedo / math.pi, (m, 3)).copy()
    if mat.kind == Material.PHONG:
        c = phong_cosine(n, wo, wi)
        return (mat.albedo * ((mat.shininess + 2.0) / (2.0 * math.pi)))[None, :] * np.power(c, mat.shininess)[:, None]
    return np.ones((m, 3))


@functools.lru_cache(maxsize=None)
def bsdf_inputs(name, f64):
    """(n, wo, wi, labels) of the bsdf test besides the sampled directions: the random (n, wo) with N directions over the whole
    sphere, then for the six axis normals tangent-plane wi (wo above) and tangent-plane wo (wi above), the normal component
    +0.0 and -0.0 and the in-plane components of either sign: n.wi (n.wo) comes out as +0 or as -0."""
    rng = np.random.default_rng(2000 + _material_seed(name))
    n, wo = random_inputs(name)
    wi = _unit(rng.normal(size=(N, 3)))
    sn, swo, swi = [], [], []
    for k in range(3):
        for s in (1.0, -1.0):
            nrm = np.roll([s, 0.0, 0.0], k)
            above = _unit(nrm + 0.5 * np.abs(np.roll(nrm, 1)) + 0.3 * np.abs(np.roll(nrm, 2)))
            for z in (0.0, -0.0):
                for sa in (1.0, -1.0):
                    for sb in (1.0, -1.0):
                        t = np.roll([z, 0.6 * sa, 0.8 * sb], k)
                        sn += [nrm, nrm]
                        swo += [above, t]
                        swi += [t, above]
    n, wo, wi = np.concatenate([n, np.array(sn)]), np.concatenate([wo, np.array(swo)]), np.concatenate([wi, np.array(swi)])
    labels = np.array([""] * N + ["tangent"] * len(sn))
    if not f64:
        n, wo, wi = (a.astype(np.float32).astype(np.float64) for a in (n, wo, wi))
    for a in (n, wo, wi, labels):
        a.setflags(write=False)
    return n, wo, wi, labels


# ------------------------------------------------------------------ cameras
def cameras():
    """Pinhole and thin lens (aperture 1e-6, 0.05, 2; focal distance 0.1 and 10), fov 0.05 and 2.5, `up` orthogonal to the
    direction (look_at) and not."""
    tilted = _unit([0.3, -0.2, -1.0])
    return {
        "pinhole-narrow": Camera.look_at(vec3(1.0, 2.0, 8.0), vec3(0.0, 0.5, 0.0), vec3(0, 1, 0), 0.05),
        "pinhole-wide-skew": Camera(vec3(-3.0, 1.0, 4.0), tilted, vec3(0.1, 1.0, 0.2), 2.5),
        "lens1e-6-wide": Camera(vec3(0.5, 0.25, 2.0), vec3(0, 0, -1), vec3(0, 1, 0), 2.5, 1e-6, 10.0),
        "lens0.05-near-skew": Camera(vec3(1.0, -0.5, 1.5), tilted, vec3(0.1, 1.0, 0.2), 0.05, 0.05, 0.1),
        "lens2-wide": Camera.look_at(vec3(4.0, 3.0, 12.0), vec3(0.0, 0.0, 0.0), vec3(0, 1, 0), 2.5).focus(vec3(0.0, 0.0, 2.0), 2.0),
    }


CAMERA_NAMES = list(cameras())
FRAMES = [(33, 17), (17, 33), (1, 1), (64, 64)]
SAMPLES = [0, 1023]
LENS_DRAWS = 2 + 2 * 24        # jitter + up to 24 candidates: (1 - pi/4)^24 = 1e-16 of the pixels need more


def lens_flags(width, height, sample, seed=SEED):
    """Pixels where some candidate of the lens loop up to the accepted one has |x^2 + y^2 - 1| < 1e-6 (accept or redraw), from the
    reference's draws alone: x = -1 + 2 u.  -> (flagged, candidates drawn)."""
    u = uniforms(seed, width * height, LENS_DRAWS, sample)[:, 2:]
    x, y = -1.0 + 2.0 * u[:, 0::2], -1.0 + 2.0 * u[:, 1::2]
    r2 = x * x + y * y
    ok = r2 <= 1.0
    assert ok.any(axis=1).all()
    first = ok.argmax(axis=1)
    upto = np.arange(r2.shape[1])[None, :] <= first[:, None]
    return (upto & (np.abs(r2 - 1.0) < 1e-6)).any(axis=1), first + 1


# ------------------------------------------------------------------ the frame with faces turned upside down
def upside_down_scene(epsilon=False):
    """A Lambertian quad and a Phong cube turned with rotate_z(pi) over a floor, lit by a sphere light: the quad and the cube's
    lowest face look down with the normal (-sin(pi), -1, 0), sin(pi) = 1.2e-16.  -> scene, camera, probe rays (origins, directions:
    straight up onto the quad and onto the cube's lowest face)."""
    sc = Scene()
    sc.add(Object(plane(vec3(0, 1, 0), -1.0)).material(Material.diffuse(vec3(0.8, 0.8, 0.8))))
    quad = polygon([vec3(0.4, -1.5, -0.9), vec3(0.4, -1.5, 0.9), vec3(2.2, -1.5, 0.9), vec3(2.2, -1.5, -0.9)])   # faces +Y before the turn
    sc.add(Object(quad.rotate_z(math.pi)).material(Material.diffuse(vec3(0.9, 0.5, 0.3))))
    box = cube().scale(vec3(1.2, 0.8, 1.2)).rotate_y(0.4).translate(vec3(-1.3, -0.9, 0.0))
    sc.add(Object(box.rotate_z(math.pi)).material(Material.specular(vec3(0.4, 0.6, 0.9), 6.0)))
    lamp = sphere().scale(vec3(0.3, 0.3, 0.3)).translate(vec3(0.0, -0.2, 2.0))
    sc.add(Object(lamp.clone()).material(Material.light(vec3(1, 1, 1), 40.0)))
    sc.add(Light.Object(Object(lamp.clone()).material(Material.light(vec3(1, 1, 1), 40.0))))
    if epsilon:
        sc.set_option("epsilon_policy", 1)
    cam = Camera.look_at(vec3(0.0, -0.6, 6.0), vec3(0.0, 0.4, 0.0), vec3(0, 1, 0), 0.7)
    o = np.array([[-1.3, -0.9, 0.0], [1.3, -0.9, 0.0]])
    d = np.array([[0.0, 1.0, 0.0], [0.0, 1.0, 0.0]])
    return sc, cam, o, d
