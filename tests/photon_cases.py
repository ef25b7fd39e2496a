"""Scenes and hand-made photon records for the photon-map tests (CPU only: numpy).

Every family is seeded and small (a few thousand records at most); positions, directions and powers are rounded to fp32 before either
side sees them, so the library's 48-byte records and the reference's fp64 lists hold the same numbers.

Scenes (y is up; every surface is Lambertian; the camera is a pinhole):
  A   an open floor polygon [-2, 2]^2 at y = 0 under a small light quad: no room shell, no plane;
  W   A with a 0.02-thick wall standing on the floor (the visibility family);
  B   a closed room [-2, 2] x [0, 4] x [-2, 2] of six polygons with an inner cube, the camera inside: the room shell;
  C   A with the floor as a `plane`;
  D   a bumpy_torus(40, 24) mesh over the floor of A: the mesh has a tree, the BVH kernel flavours run;
  E   A with the veil of `veil_triangles()` between the eye and the floor (used as Ed);
  L   A seen through a thin lens (aperture 0.1, focused on the origin): the samples of a pixel start at different points (used as Lm);
  Am, Bm   A and B in a homogeneous isotropic medium;
  Ad, Wd   A and W in a denser one (sigma_t = 0.14): the sampled distance of the point x point estimate (mean 7) falls before the
           first hit (4 to 6 away) for about half of the pixels; in the fog of Am (sigma_t = 0.07, mean 14) it rarely does.

`family(name)` is a Case: scene, gather size K, surface and volume photon lists ((n, 10): position, direction, power, 0) and the
frames ((width, height, sample), ...) it is rendered at.  The surface families: control, few-*, dense, duplicates, pairs, line, outlier,
far, visibility, room, K-*, plane, torus, deep.  The volume families (beam x point map, kind 1): v-control, v-room, v-n1 .. v-n9,
v-coincident, v-behind, v-camera, v-block; `deep_volume()` is the deep comb as volume photons.  The families of the other two kinds of map carry their kind (`Case.kind`): p-* are
point x point maps (kind 0, volume gather size `Case.Kv`), b-* beam x beam maps (kind 2), whose volume list is (n, 10): end, start,
power, radius and whose records come from `beam_records`.  `radii_sets()` are position sets that
only go through the 10-NN radius kernel.  `restated(name)` / `answers(name, w, h, sample)` compute a family's reference once per process.

`tree_depth(positions)` emulates the map build far enough to count the inner nodes on the deepest path of the k-nearest tree:
morton_kernel's fp32 arithmetic, the stable sort, Karras' hierarchy with the index tie-break and pack_kernel's leaf collapse at 8."""
import functools

import numpy as np

from tests.photon_ref import word_uniform
from rpt_amd import Camera, Material, Medium, Mesh, Object, Scene, cube, plane, polygon, scenes, vec3

LEAF_MAX = 8            # kKnnLeaf
KNN_STACK = 64          # kKnnStack: the per-lane stack of the k-nearest walk
COOP_CAP = 256          # kCoopCap: candidates of the wave-level surface gather
CAND_CAP = 4096         # kCandCap: candidates of one 8x8 pixel block's beam estimate
FLOOR = 2.0
WALL_X, WALL_HALF = 0.3, 0.01
CUBE_AT, CUBE_SIZE = np.array([0.6, 0.4, -0.5]), 0.8
FOG = (0.02, 0.05)
FOG_DENSE = (0.04, 0.1)
EYE = np.array([0.0, 2.5, 4.5])      # the camera of every scene but B
ORACLE_BEAM_RADIUS = 3.0             # the reference's constant: only beams of this radius can be pinned to the oracle


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
    base = name.rstrip("md")
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
        if base == "E":
            sc.add(Object(Mesh(veil_triangles())).material(grey))
        if base == "D":
            mesh = Mesh(scenes.bumpy_torus(40, 24))
            sc.add(Object(mesh.scale(vec3(2.0, 2.0, 2.0)).translate(vec3(0.0, 0.5, 0.0))).material(grey))
        sc.add((_light(3.0), lamp))
        cam = Camera.look_at(vec3(0.0, 2.5, 4.5), vec3(0.0, 0.0, 0.0), vec3(0.0, 1.0, 0.0), 0.55)
        if base == "L":
            cam.focus(vec3(0.0, 0.0, 0.0), 0.1)
    if name.endswith("m"):
        sc.add(Medium.homogeneous_isotropic(*FOG))
    if name.endswith("d"):
        sc.add(Medium.homogeneous_isotropic(*FOG_DENSE))
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


def beams(start, end, radius, rng, power=None):
    """(n, 10) beam list: end, start, power in [0.1, 1]^3 (seeded), radius; all rounded to fp32."""
    start, end = np.asarray(start, dtype=np.float64).reshape(-1, 3), np.asarray(end, dtype=np.float64).reshape(-1, 3)
    n = len(start)
    out = np.zeros((n, 10))
    out[:, :3], out[:, 3:6], out[:, 9] = end, start, radius
    out[:, 6:9] = rng.uniform(0.1, 1.0, (n, 3)) if power is None else power
    return f32(out)


def beam_records(bm):
    """The library's 48-byte records of a beam list: (n, 12) float32 (end, radius; start, 0; power, 0)."""
    bm = np.asarray(bm, dtype=np.float64).reshape(-1, 10)
    out = np.zeros((len(bm), 12), dtype=np.float32)
    out[:, 0:3], out[:, 3], out[:, 4:7], out[:, 8:11] = bm[:, 0:3], bm[:, 9], bm[:, 3:6], bm[:, 6:9]
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
    def __init__(self, name, scene_name, K, surface, volume=None, frames=((24, 24, 0),), note="", kind=1, Kv=3):
        self.name, self.scene_name, self.K, self.kind, self.Kv = name, scene_name, K, kind, Kv
        self.surface = np.asarray(surface, dtype=np.float64).reshape(-1, 10)
        self.volume = np.zeros((0, 10)) if volume is None else np.asarray(volume, dtype=np.float64).reshape(-1, 10)
        self.frames, self.note = tuple(frames), note

    def scene(self):
        return scene(self.scene_name)

    def volume_records(self):
        return beam_records(self.volume) if self.kind == 2 else records(self.volume)


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


# ------------------------------------------------------------------ point x point maps (kind 0) and beam x beam maps (kind 2)
PIXEL_FRAME = (24, 24, 0)            # the frame whose camera rays the per-pixel constructions below are made for
VEIL_STEP = 2                        # the veil of scene "Ed" stands before every second pixel


@functools.lru_cache(maxsize=None)
def _pixel_rays(scene_name="Am"):
    from oracle.pyoracle import camera_rays
    cam = scene(scene_name)[1]
    w, h, s = PIXEL_FRAME
    r = camera_rays(cam, w, h, sample=s, seed=0)
    return r["o"], r["d"], r["next_word"]


def _frame_of(d):
    """Two unit vectors that complete each direction d to a right-handed orthogonal frame."""
    a = np.where(np.abs(d[:, 1:2]) < 0.9, [[0.0, 1.0, 0.0]], [[1.0, 0.0, 0.0]])
    e1 = np.cross(d, a)
    e1 /= np.linalg.norm(e1, axis=1, keepdims=True)
    return e1, np.cross(d, e1)


def veil_triangles():
    """One small triangle per chosen pixel of PIXEL_FRAME, facing the eye at the very distance the pixel's sample draws in the dense
    fog, 0.4 pixel wide: the point x point estimate's branch d < t is undecided there on purpose.  -> (n, 6, 3)."""
    o, d, word = _pixel_rays()
    dist = -np.log(word_uniform(word)) / (FOG_DENSE[0] + FOG_DENSE[1])
    pix = np.arange(0, len(o), VEIL_STEP)
    # (not nearer than 1: a triangle 0.4 pixel wide a few thousandths from the eye is a handful of fp32 steps across at these
    # coordinates -- the fp32 mesh is then another triangle than the fp64 one)
    pix = pix[(dist[pix] >= 1.0) & (dist[pix] < 8.0)]
    cam = scene("Am")[1]
    size = 0.4 * np.tan(0.5 * cam.fov) / PIXEL_FRAME[0] * dist[pix]
    e1, e2 = _frame_of(d[pix])
    c = o[pix] + dist[pix, None] * d[pix]
    tri = np.zeros((len(pix), 6, 3))
    for k, a in enumerate((0.5, 0.5 + 2.0 / 3.0, 0.5 + 4.0 / 3.0)):
        tri[:, k] = c + size[:, None] * (np.cos(np.pi * a) * e1 + np.sin(np.pi * a) * e2)
        tri[:, 3 + k] = -d[pix]
    return tri


def _bb_point(o, d, start, end):
    """The beam x beam estimate's geometry for one ray and one beam -> tq, beam_t, dist (src/photon.rs:503-593)."""
    b = (end - start) / np.linalg.norm(end - start)
    l = start - o
    u = np.cross(l, b)
    u /= np.linalg.norm(u)
    n = np.cross(b, u)
    n /= np.linalg.norm(n)
    tq = (n @ l) / (n @ d)
    qc = o + tq * d
    bt = b @ (qc - start)
    return tq, bt, np.linalg.norm(qc - (start + bt * b))


def _point_families():
    fam = []
    rng = np.random.default_rng(4401)
    floor = photons(lattice(rng, 20, 20), rng)
    K, KV = 8, 8

    def add(name, vol, scene_name="Ad", Kv=KV, frames=(PIXEL_FRAME,), note=""):
        fam.append(Case(name, scene_name, K, floor, vol, frames=frames, note=note, kind=0, Kv=Kv))

    rng = np.random.default_rng(4402)
    g = np.stack(np.meshgrid(np.linspace(-1.8, 1.8, 12), np.linspace(0.2, 2.6, 8), np.linspace(-1.8, 2.5, 12), indexing="ij"), axis=-1).reshape(-1, 3)
    control = photons(g + rng.uniform(-0.1, 0.1, g.shape), rng)
    add("p-control", control, frames=BOTH, note="a jittered 3-D lattice in the fogged scene")
    spread = control[::120]
    for n in (0, 1, KV - 1, KV, KV + 1):
        add(f"p-n{n}", spread[:n], note="an empty map gives 0 / 0 in the volume branch")
    add("p-coincident", np.repeat(control[500:501], KV, axis=0), note="K coincident photons are the whole map: every distance ties")
    sites = control[7::97][:6]
    ties = [control[::3]] + [np.repeat(sites[i:i + 1], m, axis=0) for i, m in enumerate((2, 2, KV, KV, 3 * KV, 3 * KV))]
    add("p-ties", np.concatenate(ties), note="groups of 2, K and 3K identical records: ties at the K-th distance")
    for kv in (1, 56, 57, 100):
        add(f"p-K{kv}", control, Kv=kv, note="57: the first gather with its lists in global memory")
    rng = np.random.default_rng(4403)
    ball = rng.normal(size=(1000, 3))
    ball = np.array([0.3, 1.2, 1.0]) + 0.03 * ball / np.linalg.norm(ball, axis=1, keepdims=True) * rng.uniform(0.0, 1.0, (1000, 1)) ** (1.0 / 3.0)
    add("p-clump", photons(np.concatenate([ball, control[::6, :3], [[1.0e4, 0.0, 0.0]]]), rng), note="a dense clump, a sparse lattice and one photon at 1e4")
    rng = np.random.default_rng(4404)
    wall = np.stack([WALL_X + rng.choice([-1.0, 1.0], 800) * rng.uniform(WALL_HALF + 0.002, 0.08, 800), rng.uniform(0.05, 0.95, 800),
                     rng.uniform(-0.9, 0.9, 800)], axis=1)
    add("p-wall", photons(np.concatenate([wall, control[::4, :3]]), rng), scene_name="Wd", note="photons on both sides of the thin wall: the volume gather has no visibility test")
    rng = np.random.default_rng(4405)
    behind = np.stack([rng.uniform(-1.0, 1.0, 300), rng.uniform(2.0, 3.5, 300), rng.uniform(4.6, 6.0, 300)], axis=1)
    add("p-behind", photons(np.concatenate([behind, control[::4, :3]]), rng), note="photons behind the eye")
    rng = np.random.default_rng(4406)
    add("p-deep16", _comb_photons(rng, 16), note="the comb with 16 origin copies: 64 inner nodes on the deepest path, the deepest tree the walk holds")
    add("p-edge", control, scene_name="Ed", note="a veil of triangles at the sampled distances: the branch d < t is undecided on purpose")
    return fam


def _beam_families():
    fam = []
    rng = np.random.default_rng(4501)
    floor = photons(lattice(rng, 20, 20), rng)
    K, R3 = 8, ORACLE_BEAM_RADIUS

    def add(name, bm, frames=(PIXEL_FRAME,), note="", scene_name="Am"):
        fam.append(Case(name, scene_name, K, floor, bm, frames=frames, note=note, kind=2))

    rng = np.random.default_rng(4502)
    n = 300
    start = np.array([0.0, 3.0, 0.0]) + rng.uniform(-0.25, 0.25, (n, 3)) * [1.0, 0.0, 1.0]
    dirs = rng.normal(size=(n, 3))
    dirs[:, 1] = -np.abs(dirs[:, 1])
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    end = start + dirs * rng.uniform(0.5, 3.0, (n, 1))
    control = beams(start, end, R3, rng)
    add("b-control", control, frames=BOTH, note="beams of the oracle's radius from under the light")
    thin = control.copy()
    thin[:, 9] = f32(rng.uniform(0.05, 0.3, n))
    add("b-thin", thin, frames=BOTH, note="radii 0.05 .. 0.3 from the record: against the restatement only")
    add("b-lens", control[:120], scene_name="Lm", note="a thin lens: with several samples per pixel the lanes' rays share no origin, "
        "form no packet and take beam_walk_batch")
    add("b-n0", control[:0])
    add("b-n1", control[:1])
    some = control[:60]
    o, d, _ = _pixel_rays()
    e1, e2 = _frame_of(d)
    rng = np.random.default_rng(4503)
    pix = rng.choice(len(o), 16, replace=False)
    depth = rng.uniform(2.0, 4.0, 16)
    on_ray = o[pix] + depth[:, None] * d[pix]
    first = np.arange(16) < 8
    s_ = np.where(first[:, None], on_ray, on_ray - 0.8 * e1[pix])
    e_ = np.where(first[:, None], on_ray + 0.8 * e1[pix], on_ray)
    add("b-ends", np.concatenate([beams(s_, e_, R3, rng), some]), note="beams that start (8) or end (8) on a pixel's own ray: beam_t at 0 and at the length")
    rng = np.random.default_rng(4504)
    pix = rng.choice(len(o), 12, replace=False)
    s_, e_ = np.zeros((12, 3)), np.zeros((12, 3))
    for i, p in enumerate(pix):
        at = o[p] + rng.uniform(2.0, 4.0) * d[p]
        lo_a, hi_a = 0.0, 6.0
        for _ in range(80):                                  # the offset at which the reference's own dist equals the radius
            mid = 0.5 * (lo_a + hi_a)
            c = at + mid * e1[p]
            if _bb_point(o[p], d[p], c - 2.0 * e2[p], c + 2.0 * e2[p])[2] < R3:
                lo_a = mid
            else:
                hi_a = mid
        c = at + lo_a * e1[p]
        s_[i], e_[i] = c - 2.0 * e2[p], c + 2.0 * e2[p]
    add("b-tangent", np.concatenate([beams(s_, e_, R3, rng), some]), note="beams at the radius from a pixel's own ray")
    rng = np.random.default_rng(4505)

    def seg(n, y0, y1):
        a = np.stack([rng.uniform(-1.5, 1.5, n), rng.uniform(*y0, n), rng.uniform(-1.5, 1.5, n)], axis=1)
        b = np.stack([a[:, 0] + rng.uniform(-0.8, 0.8, n), rng.uniform(*y1, n), a[:, 2] + rng.uniform(-0.8, 0.8, n)], axis=1)
        return a, b

    parts = [seg(60, (-1.5, -0.2), (-1.5, -0.2)), seg(60, (0.2, 0.8), (-0.8, -0.2)), seg(60, (0.3, 1.5), (0.3, 1.5))]
    add("b-hit", beams(np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]), R3, rng),
        note="beams beyond, across and in front of the floor")
    rng = np.random.default_rng(4506)

    def short(n, zlo, zhi):
        a = np.stack([rng.uniform(-1.0, 1.0, n), rng.uniform(1.5, 3.5, n), rng.uniform(zlo, zhi, n)], axis=1)
        v = rng.normal(size=(n, 3))
        return a, a + v / np.linalg.norm(v, axis=1, keepdims=True) * rng.uniform(0.5, 1.0, (n, 1))

    near, far = short(40, 4.8, 6.5), short(40, 9.5, 12.0)
    add("b-behind", np.concatenate([beams(near[0], near[1], R3, rng), beams(far[0], far[1], R3, rng), some]),
        note="beams behind the eye: 40 whose box holds the eye or reaches the forward ray, 40 whose box lies wholly behind")
    rng = np.random.default_rng(4507)
    axis = (np.zeros(3) - EYE) / np.linalg.norm(EYE)
    pix = rng.choice(len(o), 9, replace=False)
    s_, e_ = [], []
    for i, ang in enumerate((1e-3, 1e-2, 1e-1) * 3 + (1e-3, 1e-2, 1e-1)):
        dv = d[pix[i]] if i < 9 else axis
        f1, f2 = _frame_of(dv[None])
        b = dv + ang * f1[0]
        at = EYE + 2.0 * dv + 0.1 * f2[0]
        s_.append(at)
        e_.append(at + 1.5 * b / np.linalg.norm(b))
    add("b-parallel", np.concatenate([beams(s_, e_, R3, rng), some]), note="beams 1e-3, 1e-2 and 1e-1 rad from a pixel's ray (9) and from the view axis (3)")
    rng = np.random.default_rng(4508)
    a = np.stack([rng.uniform(-1.5, 1.5, 60), rng.uniform(0.2, 2.5, 60), rng.uniform(-1.5, 1.5, 60)], axis=1)
    b = a.copy()
    b[np.arange(60), np.arange(60) % 3] += rng.choice([-1.0, 1.0], 60) * rng.uniform(0.5, 2.0, 60)
    add("b-axis", beams(a, b, R3, rng), note="axis-aligned beams: a box without extent beyond the ends, exact zeros in its widening")
    add("b-long", np.concatenate([beams([[-500.0, 1.5, 0.3]], [[500.0, 1.2, -0.2]], R3, rng), control[:80]]), note="one beam of length 1000 among short ones")
    add("b-len0", np.concatenate([beams([[0.2, 1.0, 0.5]], [[0.2, 1.0, 0.5]], R3, rng), some]), note="a beam of length 0")
    add("b-eye", np.concatenate([beams([EYE + [0.0, 0.0, -2.0]], [EYE + [0.0, 0.0, -4.0]], R3, rng), some]), note="a beam whose line passes exactly through the eye")
    return fam


@functools.lru_cache(maxsize=None)
def _families():
    return {c.name: c for c in _surface_families() + _volume_families() + _point_families() + _beam_families()}


def family(name):
    return _families()[name]


SURFACE_NAMES = ("control", "few-0", "few-1", "few-5", "few-11", "few-12", "dense", "duplicates", "pairs", "line", "outlier", "far",
                 "visibility", "room", "K-1", "K-56", "K-57", "K-200", "plane", "torus", "deep")
VOLUME_NAMES = ("v-control", "v-room") + tuple(f"v-n{n}" for n in range(1, 10)) + ("v-coincident", "v-behind", "v-camera", "v-block")
NAMES = SURFACE_NAMES + VOLUME_NAMES
POINT_NAMES = ("p-control", "p-n0", "p-n1", "p-n7", "p-n8", "p-n9", "p-coincident", "p-ties", "p-K1", "p-K56", "p-K57", "p-K100", "p-clump",
               "p-wall", "p-behind", "p-deep16", "p-edge")
BEAM_NAMES = ("b-control", "b-thin", "b-lens", "b-n0", "b-n1", "b-ends", "b-tangent", "b-hit", "b-behind", "b-parallel", "b-axis", "b-long",
              "b-len0", "b-eye")
BEAM_NOT_PINNED = ("b-thin",)        # radii other than the oracle's constant
UNDECIDED_ON_PURPOSE = ("pairs", "p-edge")


@functools.lru_cache(maxsize=None)
def deep_volume(kind=1):
    """The deep comb as volume photons (with a few floor photons): the radii and the point x point gather must be right or refused.
    kind 0: the same lists as a point x point map ("p-deep72" to `restated` and `answers`)."""
    rng = np.random.default_rng(4301)
    return Case("v-deep" if kind == 1 else "p-deep72", "Am", 8, photons(lattice(rng, 10, 10), rng), _comb_photons(rng), kind=kind, Kv=3)


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
    c = deep_volume() if name == "v-deep" else deep_volume(0) if name == "p-deep72" else family(name)
    sc, cam = c.scene()
    return Restated(sc, cam, c.surface, c.volume, c.K, c.kind, c.Kv)


@functools.lru_cache(maxsize=None)
def answers(name, width, height, sample):
    a = restated(name).sample(width, height, sample)
    for arr in (a.vals, a.bounds, a.sig, a.vals2, a.bounds2, a.sig2):
        if arr is not None:
            arr.setflags(write=False)
    return a
