"""Scenes and hand-made photon records for the photon-map tests (CPU only: numpy).

Every family is seeded and small (a few thousand records at most); positions, directions and powers are rounded to fp32 before either
side sees them, so the library's 48-byte records and the reference's fp64 lists hold the same numbers.

Scenes (y is up; every surface is Lambertian; the camera is a pinhole):
  A   an open floor polygon [-2, 2]^2 at y = 0 under a small light quad: no room shell, no plane;
  W   A with a 0.02-thick wall standing on the floor (the visibility family);
  B   a closed room [-2, 2] x [0, 4] x [-2, 2] of six polygons with an inner cube, the camera inside: the room shell;
  C   A with the floor as a `plane`;
  D   a bumpy_torus(40, 24) mesh over the floor of A: the mesh has a tree, the BVH kernel flavours run;
  Am, Bm   A and B in a homogeneous isotropic medium.

`family(name)` is a Case: scene, gather size K, surface and volume photon lists ((n, 10): position, direction, power, 0) and the
frames ((width, height, sample), ...) it is rendered at.  The surface families: control, few-*, dense, duplicates, pairs, line, outlier,
far, visibility, room, K-*, plane, torus, deep.  The volume families (beam x point map, kind 1): v-control, v-room, v-n1 .. v-n9,
v-coincident, v-behind, v-camera, v-block; `deep_volume()` is the deep comb as volume photons.  `radii_sets()` are position sets that
only go through the 10-NN radius kernel.  `restated(name)` / `answers(name, w, h, sample)` compute a family's reference once per process.

`tree_depth(positions)` emulates the map build far enough to count the inner nodes on the deepest path of the k-nearest tree:
morton_kernel's fp32 arithmetic, the stable sort, Karras' hierarchy with the index tie-break and pack_kernel's leaf collapse at 8."""
import functools

import numpy as np

from rpt_amd import Camera, Material, Medium, Mesh, Object, Scene, cube, plane, polygon, scenes, vec3

LEAF_MAX = 8            # kKnnLeaf
KNN_STACK = 64          # kKnnStack: the per-lane stack of the k-nearest walk
COOP_CAP = 256          # kCoopCap: candidates of the wave-level surface gather
CAND_CAP = 4096         # kCandCap: candidates of one 8x8 pixel block's beam estimate
FLOOR = 2.0
WALL_X, WALL_HALF = 0.3, 0.01
CUBE_AT, CUBE_SIZE = np.array([0.6, 0.4, -0.5]), 0.8
FOG = (0.02, 0.05)


def f32(a):
    return np.ascontiguousarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


# ------------------------------------------------------------------ scenes
def _quad(verts, towards):
    """A polygon whose normal points to the side of `towards`."""
    v = [np.asarray(p, dtype=np.float64) for p in verts]
    if np.dot(np.cross(v[1] - v[0], v[2] - v[0]), np.asarray(towards, dtype=np.float64) - v[0]) < 0:
        v = v[::-1]
    return polygon([vec3(*p) for p in v])


def _floor(y=0.0, s=FLOOR):
    return _quad([(-s, y, -s), (-s, y, s), (s, y, s), (s, y, -s)], (0.0, y + 1.0, 0.0))


def _light(y):
    return _quad([(-0.25, y, -0.25), (0.25, y, -0.25), (0.25, y, 0.25), (-0.25, y, 0.25)], (0.0, y - 1.0, 0.0))


def scene(name):
    """-> (Scene, Camera), a fresh pair per call (a Scene commits to a device once and keeps its options)."""
    sc = Scene()
    floor_m = Material.diffuse(vec3(0.75, 0.6, 0.45))
    grey = Material.diffuse(vec3(0.5, 0.55, 0.6))
    lamp = Material.light(vec3(1.0, 1.0, 1.0), 10.0)
    base = name.rstrip("m")
    if base == "B":
        s, h = FLOOR, 4.0
        mid = (0.0, 2.0, 0.0)
        sc.add(Object(_quad([(-s, 0, -s), (-s, 0, s), (s, 0, s), (s, 0, -s)], mid)).material(floor_m))
        sc.add(Object(_quad([(-s, h, -s), (-s, h, s), (s, h, s), (s, h, -s)], mid)).material(grey))
        sc.add(Object(_quad([(-s, 0, -s), (-s, h, -s), (s, h, -s), (s, 0, -s)], mid)).material(grey))
        sc.add(Object(_quad([(-s, 0, s), (-s, h, s), (s, h, s), (s, 0, s)], mid)).material(grey))
        sc.add(Object(_quad([(-s, 0, -s), (-s, h, -s), (-s, h, s), (-s, 0, s)], mid)).material(grey))
        sc.add(Object(_quad([(s, 0, -s), (s, h, -s), (s, h, s), (s, 0, s)], mid)).material(grey))
        sc.add(Object(cube().scale(vec3(CUBE_SIZE, CUBE_SIZE, CUBE_SIZE)).translate(vec3(*CUBE_AT))).material(grey))
        sc.add((_light(3.875), lamp))
        cam = Camera.look_at(vec3(0.0, 2.5, 1.75), vec3(0.25, 0.0, -0.5), vec3(0.0, 1.0, 0.0), 0.8)
    else:
        if base == "C":
            sc.add(Object(plane(vec3(0.0, 1.0, 0.0), 0.0)).material(floor_m))
        else:
            sc.add(Object(_floor()).material(floor_m))
        if base == "W":
            sc.add(Object(cube().scale(vec3(2.0 * WALL_HALF, 1.0, 2.0)).translate(vec3(WALL_X, 0.5, 0.0))).material(grey))
        if base == "D":
            mesh = Mesh(scenes.bumpy_torus(40, 24))
            sc.add(Object(mesh.scale(vec3(2.0, 2.0, 2.0)).translate(vec3(0.0, 0.5, 0.0))).material(grey))
        sc.add((_light(3.0), lamp))
        cam = Camera.look_at(vec3(0.0, 2.5, 4.5), vec3(0.0, 0.0, 0.0), vec3(0.0, 1.0, 0.0), 0.55)
    if name.endswith("m"):
        sc.add(Medium.homogeneous_isotropic(*FOG))
    return sc, cam


# ------------------------------------------------------------------ records
def photons(pos, rng, up=(0.0, 1.0, 0.0), direction=None, power=None):
    """(n, 10) photon list at `pos`: seeded directions in the hemisphere of `up` (at least 0.2 above its horizon), powers in
    [0.1, 1]^3, all rounded to fp32."""
    pos = np.asarray(pos, dtype=np.float64).reshape(-1, 3)
    n = len(pos)
    if direction is None:
        d = rng.normal(size=(n, 3))
        upv = np.asarray(up, dtype=np.float64)
        d -= (d @ upv)[:, None] * upv
        d += (np.abs(rng.normal(size=n)) + 0.2)[:, None] * upv
        direction = d / np.linalg.norm(d, axis=1, keepdims=True)
    if power is None:
        power = rng.uniform(0.1, 1.0, (n, 3))
    out = np.zeros((n, 10))
    out[:, :3], out[:, 3:6], out[:, 6:9] = pos, direction, power
    return f32(out)


def records(ph):
    """The library's 48-byte records of a photon list: (n, 12) float32 (position, radius 0; direction, 0; power, 0)."""
    ph = np.asarray(ph, dtype=np.float64).reshape(-1, 10)
    out = np.zeros((len(ph), 12), dtype=np.float32)
    out[:, 0:3], out[:, 4:7], out[:, 8:11] = ph[:, 0:3], ph[:, 3:6], ph[:, 6:9]
    return out


def lattice(rng, nx, nz, lo=-1.8, hi=1.8, jitter=0.3, y=0.0):
    gx, gz = np.meshgrid(np.linspace(lo, hi, nx), np.linspace(lo, hi, nz), indexing="ij")
    p = np.stack([gx.ravel(), np.full(nx * nz, y), gz.ravel()], axis=1)
    sx, sz = (hi - lo) / max(nx - 1, 1), (hi - lo) / max(nz - 1, 1)
    p[:, 0] += rng.uniform(-jitter, jitter, len(p)) * sx
    p[:, 2] += rng.uniform(-jitter, jitter, len(p)) * sz
    return p


def comb(copies):
    """The positions whose k-nearest tree is deep: `copies` points at the origin, 63 points with one coordinate (2^j + 0.5) q
    (j = 0 .. 20, q = one Morton cell) and the corner (E, E, E), E = 2097151 * 2^-12."""
    E = 2097151.0 * 2.0 ** -12
    q = E / 2097151.0
    pts = [[0.0, 0.0, 0.0]] * copies
    for j in range(21):
        for a in range(3):
            p = [0.0, 0.0, 0.0]
            p[a] = (2.0 ** j + 0.5) * q
            pts.append(p)
    pts.append([E, E, E])
    return np.array(pts)


# ------------------------------------------------------------------ the build, emulated
def morton_keys(pos):
    """morton_kernel: 63-bit keys from fp32 arithmetic."""
    f = np.float32
    P = np.ascontiguousarray(pos, dtype=np.float64).astype(f).reshape(-1, 3)
    lo, hi = P.min(axis=0), P.max(axis=0)
    ex = np.maximum(hi - lo, f(1e-30))
    s = f(2097151.0)
    cells = np.minimum(np.maximum(((P - lo) / ex).astype(f) * s, f(0.0)), s).astype(np.uint64)
    keys = np.zeros(len(P), dtype=np.uint64)
    for b in range(21):
        for a in range(3):
            keys |= ((cells[:, a] >> np.uint64(b)) & np.uint64(1)) << np.uint64(3 * b + (2 - a))
    return keys


def tree_depth(pos, leaf_max=LEAF_MAX):
    """Inner nodes on the deepest root-to-leaf path of the packed k-nearest tree of these positions (0 for fewer than 2)."""
    if len(pos) < 2:
        return 0
    k = [int(v) for v in np.sort(morton_keys(pos), kind="stable")]
    n = len(k)

    def delta(i, j):
        if k[i] != k[j]:
            return 64 - (k[i] ^ k[j]).bit_length()
        return 64 + 32 - (i ^ j).bit_length()

    best, stack = 0, [(0, n - 1, 0)]
    while stack:
        lo, hi, d = stack.pop()
        if lo == hi or (hi - lo + 1 <= leaf_max and d > 0):
            best = max(best, d)
            continue
        c = delta(lo, hi)
        a, b = lo, hi                                  # the split: the largest s in [lo, hi) with delta(lo, s) > c
        while b - a > 1:
            mid = (a + b) // 2
            if delta(lo, mid) > c:
                a = mid
            else:
                b = mid
        stack.append((lo, a, d + 1))
        stack.append((a + 1, hi, d + 1))
    return best


# ------------------------------------------------------------------ families
class Case:
    def __init__(self, name, scene_name, K, surface, volume=None, frames=((24, 24, 0),), note=""):
        self.name, self.scene_name, self.K = name, scene_name, K
        self.surface = np.asarray(surface, dtype=np.float64).reshape(-1, 10)
        self.volume = np.zeros((0, 10)) if volume is None else np.asarray(volume, dtype=np.float64).reshape(-1, 10)
        self.frames, self.note = tuple(frames), note

    def scene(self):
        return scene(self.scene_name)


K0 = 12
BOTH = ((24, 24, 0), (50, 37, 3))
DENSE_AT, DENSE_R = np.array([0.2, 0.0, 0.9]), 0.02
BLOCK_ROWS = (12, 13)


def _control(rng):
    return photons(lattice(rng, 60, 50), rng)


def _disc(rng, n, at, radius):
    a, r = rng.uniform(0.0, 2.0 * np.pi, n), radius * np.sqrt(rng.uniform(0.0, 1.0, n))
    return np.stack([at[0] + r * np.cos(a), np.full(n, at[1]), at[2] + r * np.sin(a)], axis=1)


def _comb_photons(rng, copies=4096):
    ph = photons(comb(copies), rng)
    ph[:copies, 3:9] = ph[0, 3:9]        # the copies at the origin are one payload
    return ph


def _surface_families():
    fam = []
    rng = np.random.default_rng(4101)
    control = _control(rng)
    fam.append(Case("control", "A", K0, control, frames=BOTH))
    few = photons(lattice(np.random.default_rng(4102), 4, 3, -0.9, 0.9), np.random.default_rng(4103))
    for n in (0, 1, 5, K0 - 1, K0):
        fam.append(Case(f"few-{n}", "A", K0, few[:n]))
    rng = np.random.default_rng(4104)
    dense = np.concatenate([_disc(rng, 2000, DENSE_AT, DENSE_R), lattice(rng, 20, 20)])
    fam.append(Case("dense", "A", 56, photons(dense, rng), frames=BOTH, note="a ball of more than kCoopCap candidates"))
    rng = np.random.default_rng(4105)
    base = photons(lattice(rng, 32, 32), rng)
    sites = photons(lattice(rng, 3, 3, -1.2, 1.2), rng)
    dup = [base] + [np.repeat(sites[i:i + 1], m, axis=0) for i, m in enumerate((2, 2, 2, K0, K0, K0, 3 * K0, 3 * K0, 3 * K0))]
    fam.append(Case("duplicates", "A", K0, np.concatenate(dup), note="groups of 2, K and 3K identical records"))
    rng = np.random.default_rng(4106)
    site = lattice(rng, 40, 40)
    h = 2.0 ** -6
    # (the lower one 2^-18 h farther from the floor: fp64 tells the two apart, a query point moved by 1e-5 swaps them)
    up, down = photons(site + [0.0, h, 0.0], rng), photons(site - [0.0, h * (1.0 + 2.0 ** -18), 0.0], rng)
    pairs = np.stack([up, down], axis=1).reshape(-1, 10)
    fam.append(Case("pairs", "A", K0 - 1, pairs, note="two payloads at all but the same distance from every floor point, K odd"))
    rng = np.random.default_rng(4107)
    line = np.stack([rng.uniform(-1.8, 1.8, 1000), np.zeros(1000), np.full(1000, 0.125)], axis=1)
    fam.append(Case("line", "A", K0, photons(line, rng), note="Morton keys on two degenerate extents"))
    rng = np.random.default_rng(4108)
    out = np.concatenate([lattice(rng, 40, 40), [[1.0e4, 0.0, 0.0]]])
    fam.append(Case("outlier", "A", K0, photons(out, rng), note="one photon at 1e4: the rest share a few Morton cells"))
    rng = np.random.default_rng(4109)
    far = lattice(rng, 25, 20, 0.0, 0.125) + [0.75, 0.0, 1.5]
    fam.append(Case("far", "A", K0, photons(far, rng), note="photons in one small patch only"))
    # visibility: photons on both sides of the wall within a gather radius, floating above the floor, arriving at and below the horizon
    rng = np.random.default_rng(4110)
    near_wall = np.stack([WALL_X + rng.choice([-1.0, 1.0], 600) * rng.uniform(WALL_HALF + 0.002, 0.08, 600), np.zeros(600),
                          rng.uniform(-0.9, 0.9, 600)], axis=1)
    floating = lattice(rng, 20, 20)
    floating[:, 1] = rng.uniform(0.0, 0.5, len(floating))
    vis = np.concatenate([photons(lattice(rng, 36, 36), rng), photons(near_wall, rng), photons(floating, rng)])
    flat = rng.choice(len(vis), 400, replace=False)
    vis[flat[:200], 4] = 0.0                                             # at the horizon of the floor's normal
    vis[flat[200:], 4] = -np.abs(vis[flat[200:], 4])                     # below it
    fam.append(Case("visibility", "W", K0, f32(vis)))
    rng = np.random.default_rng(4111)
    half = 0.5 * CUBE_SIZE
    off = rng.uniform(-half - 0.1, half + 0.1, (800, 2))
    off = off[np.abs(np.abs(off).max(axis=1) - half) > 0.03][:500]          # (not within 0.03 of the cube's side faces)
    under = np.stack([CUBE_AT[0] + off[:, 0], np.zeros(500), CUBE_AT[2] + off[:, 1]], axis=1)
    inside = under[:150] + [0.0, 0.3, 0.0]
    room = np.concatenate([photons(lattice(rng, 44, 44), rng), photons(under, rng), photons(inside, rng)])
    fam.append(Case("room", "B", K0, room, frames=BOTH, note="the room shell's shortcut; photons under and inside the inner cube"))
    for K in (1, 56, 57, 200):
        fam.append(Case(f"K-{K}", "A", K, control, note="57: the first gather with its lists in global memory"))
    fam.append(Case("plane", "C", K0, control))
    fam.append(Case("torus", "D", K0, control))
    rng = np.random.default_rng(4112)
    fam.append(Case("deep", "A", K0, _comb_photons(rng), note="the deep comb as a surface map: stackless searches"))
    return fam


def _volume_families():
    fam = []
    rng = np.random.default_rng(4201)
    floor = photons(lattice(rng, 20, 20), rng)
    K = 8

    def vol(pos, seed):
        r = np.random.default_rng(seed)
        return photons(pos, r)

    rng = np.random.default_rng(4202)
    box = np.stack([rng.uniform(-1.5, 1.5, 2000), rng.uniform(0.2, 2.0, 2000), rng.uniform(-1.5, 1.5, 2000)], axis=1)
    fam.append(Case("v-control", "Am", K, floor, vol(box, 1), frames=BOTH))
    fam.append(Case("v-room", "Bm", K, floor, vol(box, 2)))
    for n in range(1, 10):
        fam.append(Case(f"v-n{n}", "Am", K, floor, vol(box[:n] * [0.3, 0.5, 0.3], 3)))
    co = np.concatenate([np.repeat([[0.25, 0.75, 0.5]], 12, axis=0), box[:30]])
    fam.append(Case("v-coincident", "Am", K, floor, vol(co, 4), note="12 coincident photons: radius exactly 0, nothing added to a beam"))
    rng = np.random.default_rng(4203)
    behind = np.stack([rng.uniform(-1.0, 1.0, 300), rng.uniform(2.0, 3.5, 300), rng.uniform(4.6, 6.0, 300)], axis=1)
    below = np.stack([rng.uniform(-1.5, 1.5, 300), rng.uniform(-1.0, -0.05, 300), rng.uniform(-1.5, 1.5, 300)], axis=1)
    across = np.stack([rng.uniform(-1.5, 1.5, 600), rng.uniform(-0.03, 0.03, 600), rng.uniform(-1.5, 1.5, 600)], axis=1)
    fam.append(Case("v-behind", "Am", K, floor, vol(np.concatenate([behind, below, across, box[:300]]), 5),
                    note="photons behind the camera, beyond the first hit and straddling it"))
    eye = np.array([0.0, 2.5, 4.5])
    lone = np.concatenate([[eye + [0.125, -0.25, -0.5]], box[:9] * [0.2, 0.2, 0.2] + [0.0, 0.5, 0.0]])
    fam.append(Case("v-camera", "Am", K, floor, vol(lone, 6), note="an isolated photon whose sphere contains the camera"))
    # rows 12 and 13 of the pixel block (8..15, 8..15) of the 24 x 24 frame -- one strip of the block at the default "photon_parts" of 4:
    # 6,000 photons along the camera rays of its 16 pixels, each within 0.4 pixel of its ray, between 1.5 and 4 from the eye
    from oracle.pyoracle import camera_rays
    rng = np.random.default_rng(4204)
    cam = scene("Am")[1]
    rays = camera_rays(cam, 24, 24, sample=0, seed=0)
    pix = np.array([y * 24 + x for y in BLOCK_ROWS for x in range(8, 16)])
    which = rng.integers(0, len(pix), 6000)
    depth = rng.uniform(1.5, 4.0, 6000)
    pixel = 2.0 * np.tan(0.5 * cam.fov) / 24.0
    block = rays["o"][pix[which]] + depth[:, None] * rays["d"][pix[which]] + (0.4 * pixel * depth)[:, None] * rng.uniform(-1.0, 1.0, (6000, 3)) / np.sqrt(3.0)
    fam.append(Case("v-block", "Am", K, floor, vol(block, 7), note="more than kCandCap photons in the frustum of one strip of a pixel block"))
    return fam


@functools.lru_cache(maxsize=None)
def _families():
    return {c.name: c for c in _surface_families() + _volume_families()}


def family(name):
    return _families()[name]


SURFACE_NAMES = ("control", "few-0", "few-1", "few-5", "few-11", "few-12", "dense", "duplicates", "pairs", "line", "outlier", "far",
                 "visibility", "room", "K-1", "K-56", "K-57", "K-200", "plane", "torus", "deep")
VOLUME_NAMES = ("v-control", "v-room") + tuple(f"v-n{n}" for n in range(1, 10)) + ("v-coincident", "v-behind", "v-camera", "v-block")
NAMES = SURFACE_NAMES + VOLUME_NAMES
UNDECIDED_ON_PURPOSE = ("pairs",)


@functools.lru_cache(maxsize=None)
def deep_volume():
    """The deep comb as volume photons (with a few floor photons): the radii and the point x point gather must be right or refused."""
    rng = np.random.default_rng(4301)
    return Case("v-deep", "Am", 8, photons(lattice(rng, 10, 10), rng), _comb_photons(rng))


@functools.lru_cache(maxsize=None)
def radii_sets():
    """Position sets for the 10-NN radius kernel alone -> {name: (n, 3) fp32 values}."""
    out = {name: family(name).surface[:, :3] for name in ("control", "dense", "duplicates", "line", "outlier", "far")}
    for name in ("v-control", "v-coincident", "v-block") + tuple(f"v-n{n}" for n in range(1, 10)):
        out[name] = family(name).volume[:, :3]
    out["comb-16"] = f32(comb(16))          # 64 inner nodes on the deepest path: the deepest tree the walk's stack holds
    return out


# ------------------------------------------------------------------ the reference, once per process
@functools.lru_cache(maxsize=None)
def restated(name):
    from tests.photon_ref import Restated
    c = deep_volume() if name == "v-deep" else family(name)
    sc, cam = c.scene()
    return Restated(sc, cam, c.surface, c.volume, c.K)


@functools.lru_cache(maxsize=None)
def answers(name, width, height, sample):
    a = restated(name).sample(width, height, sample)
    for arr in (a.vals, a.bounds, a.sig, a.vals2, a.bounds2, a.sig2):
        if arr is not None:
            arr.setflags(write=False)
    return a
