"""Camera paths one sample at a time: the scenes, the oracle's answers around the camera, and the rule (CPU only: numpy + the oracle).

A one-iteration render is a per-sample record: pixel p of a one-sample frame at sample offset s is the radiance of stream (seed, p, s)
and nothing else.  Four such frames of 48 x 48 are 9,216 camera paths.  A path decides things (which object, shadow test passed or
not, roulette, medium event or surface), and on a path that lies on such a boundary the library's fp32 (or fp64) arithmetic and the
oracle's may decide differently and both be right.  So, as tests/ray_cloud.py does for single rays, the oracle is asked about a small
cloud around the input -- here the camera's eye -- and the library's sample has to be one the cloud contains.

  mode     oracle policy   amplitude on the eye       b
  "fp32"   robust = 1      2e-6 (1 + max|eye|)        1e-3    (the project's per-pixel target, test_gpu_epsilon.py "north_star")
  "fp64"   robust = 0      1e-14 (1 + max|eye|)       1e-9    (the suite's fp64 bound on normals)

The cloud: the camera itself and 16 seeded perturbations of its eye; for the samples whose 17 answers disagree by more than b x scale,
48 more.  The rule, per sample:
  * scale = max(1e-3, the largest channel over the sample's cloud);
  * matched: all three channels within b x scale of one member;
  * decided: the 16 perturbed members agree within b x scale in every channel;
  * nothing may be NaN, infinite or negative, matched or not.
The caps (`caps`), per scene -- conditions, none of them derived from a GPU run:
  * fp32, and fp64 without a medium: at most 0.2 % of all samples unmatched;
  * fp64 in a medium (the literal policy's 1e-12 self-hit noise): at most 0.3 % of the decided samples unmatched;
  * strata (depth reached, how the path ended, clamp engaged or not -- read from the oracle's path record of the nominal camera; in
    fp64 with a medium over the decided samples): no stratum of at least 100 samples more than 2 % unmatched;
  * among the samples the oracle says were clamped: at most 1 % unmatched.
test_path_cloud_host.py shows with the oracle alone (the nominal answer left out of its own cloud) that the inputs stay below a
quarter of each cap, that the scenes exercise what they claim, and that the rule rejects wrong answers.

The issue's MonomialSurface scene is not among the scenes: the oracle has no monomial shape, so there is no reference for a path through
one ("Camera paths", records this and the other departures).

`restate` recomputes a sample from the record's per-level terms under another clamp rule: the wrong answers of the host test."""
import os

import numpy as np

from rpt_amd import Camera, KdTree, Light, Material, Medium, Mesh, Object, Scene, cube, hex_color, plane, polygon, scenes, sphere, vec3

MODES = {"fp32": {"robust": 1, "amp": 2e-6, "b": 1e-3}, "fp64": {"robust": 0, "amp": 1e-14, "b": 1e-9}}
SIZE, OFFSETS, SEED = 48, (0, 1, 2, 3), 6
N_FIRST, N_MORE = 16, 48
SCALE_FLOOR = 1e-3
FIREFLY_CLAMP = 100.0
CAP_ALL, CAP_DECIDED_IN_MEDIUM, CAP_STRATUM, CAP_CLAMPED, STRATUM_MIN = 2e-3, 3e-3, 2e-2, 1e-2, 100
N_TORUS = 192


# ------------------------------------------------------------------ scenes
def _materials(fog, lit, floor):
    sc = Scene()
    sc.add(Object(plane(vec3(0, 1, 0), 0.0)).material(Material.diffuse(hex_color(floor))))
    sc.add(Object(sphere().translate(vec3(-2.2, 1, 0))).material(Material.mirror()))
    sc.add(Object(sphere().scale(vec3(1, 1.3, 1)).translate(vec3(0, 1.3, 0))).material(Material.transmissive(1.5)))
    sc.add(Object(cube().scale(vec3(1.5, 1.5, 1.5)).rotate_y(0.6).translate(vec3(2.4, 0.75, 0.3))).material(
        Material.specular(hex_color(0xE7A94D), 8.0)))
    sc.add(Object(sphere().scale(vec3(0.6, 0.6, 0.6)).translate(vec3(0.8, 0.6, 2.0))).material(
        Material.metallic(hex_color(0x7CA3E7), 0.4)))
    if lit:
        quad = polygon([vec3(2, 5, -2), vec3(2, 5, 2), vec3(-2, 5, 2), vec3(-2, 5, -2)])
        sc.add((quad, Material.light(vec3(1, 1, 1), 12.0)))
        sc.add((cube().scale(vec3(0.5, 0.5, 0.5)).translate(vec3(-3.5, 2.5, 2.0)), Material.light(vec3(1.0, 0.6, 0.3), 30.0)))
        _lamp(sc, 0.4, vec3(3.5, 3.0, 2.5), 40.0)
        sc.add(Light.Ambient(vec3(0.02, 0.02, 0.03)))
        sc.add(Light.Point(vec3(5, 5, 5), vec3(0, 8, 0)))       # never passes the reference's test: contributes 0
        sc.add(Light.Directional(vec3(1, 1, 1), vec3(0, -1, 0)))
    sc.environment.color = np.array([0.05, 0.07, 0.1])
    if fog == "fog":
        sc.add(Medium.homogeneous_isotropic(0.01, 0.04))
    elif fog == "thin":       # extinction 0.004: a fifth of the distance samples lie beyond the background distance 400
        sc.add(Medium.homogeneous_isotropic(0.001, 0.003))
    elif fog == "glow":
        sc.add(Medium.colored_glowing_fog(0.02, 0.02))
    return sc, Camera.look_at(vec3(0.5, 3.0, 8.0), vec3(0, 1, 0), vec3(0, 1, 0), 0.6)


def _lamp(sc, radius, at, emittance):
    for wrap in (lambda o: o, Light.Object):
        sc.add(wrap(Object(sphere().scale(vec3(radius, radius, radius)).translate(at)).material(Material.light(vec3(0.4, 0.6, 1.0), emittance))))


def materials(fog=None):
    """The scene of test_gpu_parity.py's test_all_materials_lights_and_media_match_oracle: mirror, glass, Phong (shininess 8 and 0.4),
    Lambertian; quad, cube and sphere object lights with twins; ambient, point and directional lights; an environment colour."""
    return _materials(fog, True, 0xCCCCCC) + (4,)


def clamp(fog=None, torus=False):
    """The scene in which the firefly clamp works: the materials scene without its lights, an orange floor and one small, very bright
    sphere lamp just above it, six bounces.  torus: a 192-triangle mesh more, so that the kernel flavours with a tree run the scene."""
    sc, cam = _materials(fog, False, 0xCC8844)
    _lamp(sc, 0.1, vec3(-0.8, 0.3, 1.6), 4e5)
    if torus:
        mesh = Mesh(scenes.bumpy_torus(12, 8)).scale(vec3(0.5, 0.5, 0.5)).rotate_x(0.5).translate(vec3(-1.2, 0.8, 3.2))
        sc.add(Object(mesh).material(Material.diffuse(vec3(0.7, 0.7, 0.7))))
    return sc, cam, 6


def group_light():
    """A KdTree group as Light::Object and as its twin object (test_gpu_groups.py, test_group_as_object_light_matches_oracle)."""
    kids = [
        sphere().scale(vec3(0.3, 0.3, 0.3)).translate(vec3(-1.5, 2.5, 0.0)),
        cube().scale(vec3(0.5, 0.1, 0.5)).rotate_y(0.5).translate(vec3(1.5, 2.6, 0.3)),
        Mesh(scenes.bumpy_torus(4, 3)).scale(vec3(0.4, 0.4, 0.4)).translate(vec3(0.0, 2.4, -1.0)),
        KdTree([sphere().scale(vec3(0.2, 0.2, 0.2)).translate(vec3(0.0, 0.0, 1.0)),
                sphere().scale(vec3(0.15, 0.3, 0.15)).translate(vec3(0.6, 0.0, 1.2))]).translate(vec3(0.0, 2.3, 0.0)),
    ]
    glow = Material.light(vec3(1.0, 0.9, 0.7), 25.0)
    lamp = lambda: KdTree([k.clone() for k in kids]).rotate_z(0.1).translate(vec3(0.0, 0.2, 0.0))
    sc = Scene()
    sc.add(Object(lamp()).material(glow))
    sc.add(Light.Object(Object(lamp()).material(glow)))
    sc.add(Object(plane(vec3(0, 1, 0), -1.0)).material(Material.diffuse(vec3(0.8, 0.8, 0.8))))
    sc.add(Object(sphere().translate(vec3(0.0, 0.0, 0.0))).material(Material.specular(vec3(0.9, 0.5, 0.5), 0.3)))
    sc.add(Object(cube().translate(vec3(2.0, -0.5, 0.5))).material(Material.diffuse(vec3(0.3, 0.8, 0.4))))
    return sc, Camera.look_at(vec3(0.0, 1.5, 7.0), vec3(0.0, 1.0, 0.0), vec3(0, 1, 0), 0.9), 3


def _config(name):
    sc, cam, cfg = scenes.CONFIGS[name]()
    return sc, cam, cfg["max_bounces"]


# name -> (builder of (Scene, Camera, max_bounces), has a medium (C3 is the Cornell box in thin fog), the clamp works in it)
SCENES = {
    "materials": (lambda: materials(), False, False),
    "materials fog": (lambda: materials("fog"), True, False),
    "materials glow": (lambda: materials("glow"), True, False),
    "clamp": (lambda: clamp(), False, True),
    "clamp fog": (lambda: clamp("fog"), True, False),
    "clamp thin fog": (lambda: clamp("thin"), True, False),
    "clamp torus": (lambda: clamp(torus=True), False, True),
    "group light": (group_light, False, False),
    "C2": (lambda: _config("C2"), False, False),
    "C3": (lambda: _config("C3"), True, False),
}


def build(name):
    """-> a fresh (Scene, Camera, max_bounces) of SCENES[name] (a Scene is immutable once rendered, options are set before)."""
    return SCENES[name][0]()


# ------------------------------------------------------------------ the cloud
def _threads():
    return min(16, os.cpu_count() or 1)


def _moved(cam, eye):
    return Camera(eye, cam.direction, cam.up, cam.fov, cam.aperture, cam.focal_distance)


class Cloud:
    """The oracle's answers around the camera for the n = len(OFFSETS) * SIZE^2 samples of a scene, sample i = offset index * SIZE^2 +
    pixel.  first: (17, n, 3), member 0 the camera itself; again: the samples with a second pass, more: (len(again), 48, 3);
    rec: the path records of the camera itself; light_pass: per light, the vertices at which it passed its shadow test."""

    def __init__(self, name, mode, first, again, more, rec, light_pass):
        self.name, self.mode, self.first, self.again, self.more, self.rec, self.light_pass = name, mode, first, again, more, rec, light_pass
        self.medium, self.clamp_works = SCENES[name][1], SCENES[name][2]
        b = MODES[mode]["b"]
        top = first.max(axis=(0, 2))
        if len(again):
            top[again] = np.maximum(top[again], more.max(axis=(1, 2)))
        self.scale = np.maximum(SCALE_FLOOR, top)
        self.decided = ((first[1:].max(axis=0) - first[1:].min(axis=0)).max(axis=1) <= b * self.scale)
        self.clamped = rec["clamp"] != 0

    def __len__(self):
        return self.first.shape[1]

    @property
    def nominal(self):
        return self.first[0]


def cloud(name, mode, seed=11):
    from oracle.pyoracle import OracleScene
    cfg = MODES[mode]
    sc, cam, mb = build(name)
    osc = OracleScene(sc)
    n_pix = SIZE * SIZE
    rng = np.random.default_rng(seed)
    amp = cfg["amp"] * (1.0 + np.abs(cam.eye).max())
    first = np.empty((1 + N_FIRST, len(OFFSETS) * n_pix, 3))
    recs, light_pass = [], 0
    for j, off in enumerate(OFFSETS):
        rad, rec, lp = osc.render_paths(cam, SIZE, SIZE, mb, seed=SEED, sample_offset=off, robust=cfg["robust"], threads=_threads())
        first[0, j * n_pix:(j + 1) * n_pix] = rad
        recs.append(rec)
        light_pass = light_pass + lp
    eyes = cam.eye + amp * rng.uniform(-1.0, 1.0, (N_FIRST + N_MORE, 3))
    for m in range(N_FIRST):
        for j, off in enumerate(OFFSETS):
            first[1 + m, j * n_pix:(j + 1) * n_pix] = osc.render(_moved(cam, eyes[m]), SIZE, SIZE, 1, mb, seed=SEED, sample_offset=off,
                                                                 robust=cfg["robust"], threads=_threads())
    scale = np.maximum(SCALE_FLOOR, first.max(axis=(0, 2)))
    again = np.flatnonzero((first.max(axis=0) - first.min(axis=0)).max(axis=1) > cfg["b"] * scale)
    more = np.empty((len(again), N_MORE, 3))
    for j, off in enumerate(OFFSETS):
        sel = (again >= j * n_pix) & (again < (j + 1) * n_pix)
        pix = (again[sel] - j * n_pix).astype(np.uint32)
        if not len(pix):
            continue
        for m in range(N_MORE):
            more[sel, m] = osc.render(_moved(cam, eyes[N_FIRST + m]), SIZE, SIZE, 1, mb, seed=SEED, sample_offset=off, robust=cfg["robust"],
                                      threads=_threads(), pixels=pix)[pix]
    return Cloud(name, mode, first, again, more, np.concatenate(recs), np.asarray(light_pass))


_prepared = {}


def prepared(name, mode):
    """The cloud of a scene, computed once per process."""
    if (name, mode) not in _prepared:
        _prepared[(name, mode)] = cloud(name, mode)
    return _prepared[(name, mode)]


# ------------------------------------------------------------------ the rule
class Report:
    """unmatched, bad: (n,) bool (bad: NaN, infinite or negative); err: (n,) the distance to the nearest member (largest channel) / scale."""

    def __init__(self, unmatched, bad, err):
        self.unmatched, self.bad, self.err = unmatched, bad, err


def check(cl, got, leave_out_nominal=False):
    """The rule for every sample of Cloud `cl`; got: (n, 3), sample i = offset index * SIZE^2 + pixel.  leave_out_nominal: the cloud
    without the camera's own answer (the host test puts that answer to the rule)."""
    got = np.asarray(got, dtype=np.float64).reshape(-1, 3)
    assert len(got) == len(cl)
    b = MODES[cl.mode]["b"]
    with np.errstate(invalid="ignore"):
        members = cl.first[1:] if leave_out_nominal else cl.first
        err = np.abs(members - got[None]).max(axis=2).min(axis=0)
        if len(cl.again):
            err[cl.again] = np.minimum(err[cl.again], np.abs(cl.more - got[cl.again, None, :]).max(axis=2).min(axis=1))
        err = err / cl.scale
        bad = ~np.isfinite(got).all(axis=1) | (got < 0.0).any(axis=1)
        unmatched = ~(err <= b) | bad
    return Report(unmatched, bad, err)


def strata(cl):
    """-> {(depth, end, clamped): sample indices}."""
    key = cl.rec["depth"].astype(np.int64) * 8 + cl.rec["end"].astype(np.int64) * 2 + cl.clamped
    return {(int(k) // 8, int(k) % 8 // 2, bool(k % 2)): np.flatnonzero(key == k) for k in np.unique(key)}


def caps(cl, rep, fraction=1.0, title=""):
    """The caps of this module's header, each times `fraction` -> (figures, violations), and prints one line per figure."""
    held = cl.decided if (cl.mode == "fp64" and cl.medium) else np.ones(len(cl), bool)
    cap = CAP_DECIDED_IN_MEDIUM if (cl.mode == "fp64" and cl.medium) else CAP_ALL
    un = rep.unmatched & held
    fig = {"samples": len(cl), "held": int(held.sum()), "decided": int(cl.decided.sum()), "second pass": len(cl.again),
           "unmatched": int(un.sum()), "bad": int(rep.bad.sum()), "clamped": int(cl.clamped.sum()),
           "clamped unmatched": int((un & cl.clamped).sum()),
           "worst matched error": float(rep.err[~rep.unmatched].max()) if (~rep.unmatched).any() else 0.0}
    bad = []
    if fig["bad"]:
        bad.append(f"{fig['bad']} samples NaN, infinite or negative")
    if fig["unmatched"] > fraction * cap * fig["held"]:
        bad.append(f"{fig['unmatched']} of {fig['held']} unmatched, cap {fraction * cap:.2%}")
    if cl.clamp_works and fig["clamped unmatched"] > fraction * CAP_CLAMPED * fig["clamped"]:
        bad.append(f"{fig['clamped unmatched']} of {fig['clamped']} clamped samples unmatched, cap {fraction * CAP_CLAMPED:.2%}")
    worst = (-1.0, None)
    for key, idx in strata(cl).items():
        idx = idx[held[idx]]
        if len(idx) >= STRATUM_MIN:
            share = un[idx].mean()
            worst = max(worst, (float(share), key), key=lambda w: w[0])
            if share > fraction * CAP_STRATUM:
                bad.append(f"stratum (depth, end, clamped) = {key}: {int(un[idx].sum())} of {len(idx)} unmatched, cap {fraction * CAP_STRATUM:.2%}")
    fig["worst stratum"] = worst
    print(f"{title or cl.name} [{cl.mode}]: " + ", ".join(f"{k} {v:.3g}" if isinstance(v, float) else f"{k} {v}" for k, v in fig.items()))
    for line in bad:
        print("  " + line)
    return fig, bad


def show(cl, rep, got, n=6):
    for i in np.flatnonzero(rep.unmatched)[:n]:
        r = cl.rec[i]
        print(f"  sample {i} (offset {OFFSETS[i // (SIZE * SIZE)]}, pixel {i % (SIZE * SIZE)}) depth {r['depth']} end {r['end']} clamp {int(r['clamp']):#o} "
              f"{'decided' if cl.decided[i] else 'undecided'}: library {np.asarray(got[i]).tolist()!r} oracle {cl.nominal[i].tolist()!r} "
              f"err / scale {rep.err[i]:.3g}")


# ------------------------------------------------------------------ a sample restated under another clamp rule
def restate(cl, rule):
    """The radiance of every sample from the record's per-level terms d (what a level adds itself) and k (the factor on what the next level
    returns): radiance(level) = d + clamp(k * radiance(level + 1)) -> (n, 3), exact to rounding (k is the weight of unit radiance).
      "oracle"  the reference's rule: min(., 100) at every level without a medium, none with one;
      "none"    no clamp anywhere;
      "always"  min(., 100) with a medium too;
      "flat"    the forward form with the throughput forgotten: min over the levels of (P + 100) for (P + 100 Q), P the radiance gathered
                down to that level and Q the product of the k above it.
    Samples whose record overflowed (PATH_OVERFLOW) are returned as the oracle's own radiance."""
    d, k, levels = cl.rec["d"], cl.rec["k"], cl.rec["levels"]
    n, nl = d.shape[:2]
    clamp_on = {"oracle": not cl.medium, "none": False, "always": True, "flat": False}[rule]
    if rule == "flat":
        P, Q, bound = np.zeros((n, 3)), np.ones((n, 3)), np.full((n, 3), np.inf)
        for lv in range(nl):
            P = P + Q * d[:, lv]
            goes_on = (levels > lv + 1)[:, None]
            bound = np.where(goes_on, np.minimum(bound, P + FIREFLY_CLAMP), bound)
            Q = Q * k[:, lv]
        out = np.minimum(P, bound)
    else:
        out = np.zeros((n, 3))
        for lv in reversed(range(nl)):
            ind = k[:, lv] * out
            if clamp_on:
                ind = np.fmin(ind, FIREFLY_CLAMP)
            out = d[:, lv] + np.where((levels > lv + 1)[:, None], ind, 0.0)
    over = (cl.rec["flags"] & 4) != 0
    out[over] = cl.nominal[over]
    return out


def clamp_masks(rec, levels=12):
    """-> (n, levels) of the 3-bit channel masks in which a level's fmin(indirect, FIREFLY_CLAMP) took the clamp."""
    c = rec["clamp"].astype(np.uint64)
    return np.stack([((c >> np.uint64(3 * lv)) & np.uint64(7)).astype(np.int64) for lv in range(levels)], axis=1)
