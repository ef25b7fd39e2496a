"""What a path vertex calls besides the RNG, sample_f, bsdf and cast_ray, one call at a time against the fp64 oracle: light sampling
(sample_light_shape / illuminate_object of device_core.h and their fp64 twins in kernels_f64.hip), the sky lookup (env_color, both
modes) and the fog distance (stage_distance).  The rpt_debug_* hooks run the functions the render kernels run, on the committed scene;
the cases are in tests/sampler_cases.py.  Every test prints its figures before it asserts (pytest -s shows them)."""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import pyoracle
from oracle.pyoracle import OracleScene
from rpt_amd import Camera, Medium, Renderer, RptError, Scene
from tests import sampler_cases as cases

pytestmark = pytest.mark.gpu

N, SEED = 4096, 7
LIGHT_CASES = ["A", "B", "C", "D", "E", "F", "G", "H8-quad", "H8-mesh", "H9-quad", "H9-mesh"]


def _rng_u32(seed, pixel, sample, n):
    out = np.zeros(n, dtype=np.uint32)
    pyoracle.lib().orc_rng_u32(C.c_uint64(seed), pixel, sample, n, out.ctypes.data_as(C.c_void_p))
    return out


def _scene_of(case, epsilon):
    """-> scene, light index, the light's shape."""
    if case[0] == "H":
        sc = cases.shared_table_scene(6 if case[1] == "8" else 7, epsilon)
        li = 1 if case.endswith("quad") else 2
        return sc, li, sc.lights[li].object.shape
    shape = cases.light_shapes()[case]
    return cases.light_scene(shape, epsilon), 0, shape


@functools.lru_cache(maxsize=None)
def _reference(case):
    """Computed once per case and shared by the fp32 and the fp64 test: the fp32 positions, the oracle's answers on them, and the rim
    set of the sphere leaves (from the reference alone): sphere[i] = case i samples a sphere leaf, z[i] = the sample's local z =
    dot(M^-1 v_ref, normalize(M^-1 pos)) there."""
    sc, li, shape = _scene_of(case, False)
    extra = cases.structured_sphere_positions(1) if case == "A" else None
    pos = cases.positions(N, seed=sum(map(ord, case)), extra=extra)
    ref = OracleScene(sc).light_sample(li, pos.astype(np.float64), seed=SEED)
    n = pos.shape[0]
    sphere, z = np.zeros(n, bool), np.full(n, np.inf)
    for i, m in enumerate(cases.sphere_leaf_matrices(shape, SEED, n, _rng_u32)):
        if m is None:
            continue
        inv = np.linalg.inv(m)
        tl = inv[:3, :3] @ pos[i].astype(np.float64) + inv[:3, 3]
        vl = inv[:3, :3] @ ref["v"][i] + inv[:3, 3]
        sphere[i], z[i] = True, np.dot(vl, tl / np.linalg.norm(tl))
    for a in (pos, sphere, z, *ref.values()):
        a.setflags(write=False)
    return pos, ref, sphere, z


def _common_checks(case, got, ref, sphere, z):
    """Mode-independent: the same number of draws in every case, enough lit cases, a rim set of the expected size."""
    assert np.all(np.isfinite(ref["intensity"])) and all(np.all(np.isfinite(got[k])) for k in ("v", "nrm", "p", "intensity", "wi", "dist"))
    differ = np.flatnonzero(got["next_word"] != ref["next_word"])
    assert differ.size == 0, f"{case}: draw counts differ in cases {differ[:8]}"
    nonzero = np.any(ref["intensity"] != 0, axis=1).mean()
    rim = int((sphere & (z < 1 / 16)).sum())
    print(f"{case}: nonzero share {nonzero:.3f}, sphere-leaf cases {int(sphere.sum())}, rim cases {rim}")
    assert nonzero >= 0.3
    assert np.any(got["intensity"] != 0, axis=1).mean() >= 0.3
    if sphere.any():
        assert rim < 0.01 * sphere.sum()       # expected (1/16)^2 = 1/256 of them: r^2 is uniform on the disc
    if case in ("D", "G"):                     # mirrored: the reference divides by a signed area factor, and so must the device
        assert np.all(ref["p"] < 0) and np.all(got["p"] < 0) and np.all(got["intensity"] <= 0)


@pytest.mark.parametrize("case", LIGHT_CASES)
def test_light_sample_fp32_matches_oracle_per_call(case):
    """sample_light_shape / illuminate_object (fp32) against orc_light_sample, 4096 positions per light (A: + 104 structured ones that
    take the is_normal(nn.x) branch both ways).  next_word equal in every case.  Bounds: wi, nrm 5e-5 abs; dist 2e-5 (1 + |pos| / dist)
    rel; v 2e-5 (1 + |v|) abs; pdf 2e-4 rel; |dI| < 2e-4 |colour| / (dist^2 |p_ref|), colour = albedo * emittance (the emitter
    cosine's error bounded absolutely).  On the rim cases of sphere leaves (local z < 1/16, from the reference alone; z loses digits
    as 2^-24 / z^2 in 1 - dx^2 - dy^2) the bounds of v, nrm, pdf and intensity are multiplied by 1 / (16 z)^2; wi, dist and next_word
    hold unchanged there.  The multiplier stops growing at z = 2^-12 (2^16): below that 1 - dx^2 - dy^2 is under fp32's 2^-24
    and z is rounding alone; such a case (2^-24 of sphere cases) would still have to meet the capped bound.
    Measured on an MI355X, largest error / its bound per case (wi, dist, nrm, v, pdf, intensity); no draw-count difference anywhere:
      A .013 .006 .005 .007 .029 .002 (19 rim cases of 4200)   B .017 .005 .021 .004 .029 .003 (19 of 4096)
      C .004 .006 .001 .003 .000 .002   D .003 .004 .001 .003 .001 .002   E .005 .006 .000 .004 .000 .001
      F .007 .006 .004 .006 .002 .002   G .011 .008 .005 .004 .018 .002 (7 rim cases of 1757)
      H8-quad .004 .008 .000 .004 .000 .002   H8-mesh .002 .005 .002 .004 .002 .002
      H9-quad .004 .007 .000 .004 .000 .001   H9-mesh .005 .005 .002 .004 .002 .003
    The largest over all: pdf .029 (case 2452 of A and of B: the same draws), nrm .021, wi .017.
    Nonzero shares: A .900 (with the structured positions), B .969, C .446, D .467, E 1, F .412, G .696, H-quad 1, H-mesh .63-.65."""
    pos, ref, sphere, z = _reference(case)
    sc, li, _ = _scene_of(case, False)
    got = Renderer(sc, Camera()).debug_light_sample(li, pos, seed=SEED)
    _common_checks(case, got, ref, sphere, z)
    p64 = pos.astype(np.float64)
    g = {k: v.astype(np.float64) for k, v in got.items() if k != "next_word"}
    mult = np.where(sphere & (z < 1 / 16), 1.0 / (16.0 * np.maximum(z, 2.0 ** -12)) ** 2, 1.0)
    colour = np.linalg.norm(cases.LIGHT_COLOR * cases.LIGHT_EMIT)
    ratio = {
        "wi": np.abs(g["wi"] - ref["wi"]).max(axis=1) / 5e-5,
        "dist": np.abs(g["dist"] - ref["dist"]) / ref["dist"] / (2e-5 * (1 + np.linalg.norm(p64, axis=1) / ref["dist"])),
        "nrm": np.abs(g["nrm"] - ref["nrm"]).max(axis=1) / (5e-5 * mult),
        "v": np.abs(g["v"] - ref["v"]).max(axis=1) / (2e-5 * (1 + np.linalg.norm(ref["v"], axis=1)) * mult),
        "pdf": np.abs(g["p"] - ref["p"]) / np.abs(ref["p"]) / (2e-4 * mult),
        "intensity": np.linalg.norm(g["intensity"] - ref["intensity"], axis=1) / (2e-4 * colour / (ref["dist"] ** 2 * np.abs(ref["p"])) * mult),
    }
    print(f"{case}: error / bound: " + ", ".join(f"{k} {v.max():.3f} (case {int(v.argmax())})" for k, v in ratio.items()))
    for k, v in ratio.items():
        assert v.max() < 1.0, (case, k, int(v.argmax()), float(v.max()))


@pytest.mark.parametrize("case", LIGHT_CASES)
def test_light_sample_fp64_matches_oracle_per_call(case):
    """The reference-epsilon mode's sample_shape / sample_light_shape / illuminate_object against the same oracle call, same positions:
    next_word equal in every case, no rim exclusion.  The bound to hold was 1e-12 relative (test_fp64_closest_hit_with_rotations_within_1e12's); measured on an MI355X the largest
    difference of every output (v, nrm, p, intensity, wi, dist) is 0 in all eleven cases -- both sides do the same unfused fp64
    arithmetic on the same draws, and the device's sqrt and division are correctly rounded --, so the test asserts equality."""
    pos, ref, sphere, z = _reference(case)
    sc, li, _ = _scene_of(case, True)
    got = Renderer(sc, Camera()).debug_light_sample(li, pos.astype(np.float64), seed=SEED, f64=True)
    _common_checks(case, got, ref, sphere, z)
    worst = {k: np.abs(got[k] - ref[k]).max() for k in ("v", "nrm", "p", "intensity", "wi", "dist")}
    print(f"{case}: largest differences: " + ", ".join(f"{k} {v:.3e}" for k, v in worst.items()))
    for k in worst:
        assert np.array_equal(got[k], ref[k]), (case, k, worst[k])


def test_light_hooks_check_mode_and_light_kind():
    pos = np.zeros((1, 3))
    sc32, sc64 = cases.shared_table_scene(6), cases.shared_table_scene(6, epsilon=True)
    r32, r64 = Renderer(sc32, Camera()), Renderer(sc64, Camera())
    for r, f64 in ((r32, False), (r64, True)):
        with pytest.raises(RptError) as e:
            r.debug_light_sample(0, pos + 1, f64=f64)           # light 0 is the ambient light
        assert "rpt error -1" in str(e.value) and "Light::Object" in str(e.value)
        with pytest.raises(RptError):
            r.debug_light_sample(3, pos + 1, f64=f64)           # no such light
    for r, f64 in ((r32, True), (r64, False)):                  # the other mode's hook: RPT_ERR_STATE
        with pytest.raises(RptError) as e:
            r.debug_light_sample(1, pos + 1, f64=f64)
        assert "rpt error -2" in str(e.value) and "epsilon_policy" in str(e.value)
        with pytest.raises(RptError) as e:
            r.debug_env_color(pos + 1, f64=f64)
        assert "rpt error -2" in str(e.value)
    with pytest.raises(RptError) as e:
        r64.debug_medium_distance(4)
    assert "rpt error -1" in str(e.value) and "medium" in str(e.value)      # no medium: said before anything else
    fog64 = Scene()
    fog64.add(Medium.homogeneous_isotropic(0.02, 0.1))
    fog64.set_option("epsilon_policy", 1)
    with pytest.raises(RptError) as e:
        Renderer(fog64, Camera()).debug_medium_distance(4)
    assert "rpt error -2" in str(e.value)


# ------------------------------------------------------------------ sky
def _sky_reference(name):
    img = cases.sky_images()[name]
    d = cases.sky_directions()
    return img, d, OracleScene(cases.sky_scene(img)).env_color(d.astype(np.float64))


SKY_K32 = 2 * 1.49    # 2 x the largest k any image needs, measured on an MI355X (see the docstring)


@pytest.mark.parametrize("name", ["1x1", "1x5", "6x1", "2x2", "7x5", "64x32", "ramp8x4"])
def test_env_color_fp32_within_the_angle_model(name):
    """env_color (fp32) against orc_env_color.  The lookup is continuous except across the seam, so the colour error is bounded
    through the angles: d_az <= k 2^-22, d_polar <= k 2^-24 / max(sin polar, 2^-12),
    |d colour| <= range [(w - 1) d_az / 2 pi + (h - 1) d_polar / pi] + k 2^-24 |colour|, range = largest - smallest texel.
    k is measured against the oracle (never against the fp32 code) and the test holds 2 x that; above 32 it is a wrong lookup.
    No seam flips: both sides see the same sign of z.
    Measured on an MI355X, k per image: 1x1 0.46, 1x5 1.28, 6x1 1.26, 2x2 1.45, 7x5 1.28, 64x32 1.49, ramp8x4 0.42; every worst
    direction is one of the random ones, none near a pole or the seam.  The test holds k <= 2 x 1.49 = 2.98."""
    img, d, ref = _sky_reference(name)
    h, w = img.shape[:2]
    got = Renderer(cases.sky_scene(img), Camera()).debug_env_color(d).astype(np.float64)
    assert np.all(np.isfinite(got))
    u = d.astype(np.float64)
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    sin_polar = np.maximum(np.sqrt(np.maximum(1.0 - u[:, 1] ** 2, 0.0)), 2.0 ** -12)
    unit = (img.max() - img.min()) * ((w - 1) * 2.0 ** -22 / (2 * np.pi) + (h - 1) * 2.0 ** -24 / sin_polar / np.pi) \
        + 2.0 ** -24 * np.abs(ref).max(axis=1)
    k = np.abs(got - ref).max(axis=1) / unit
    print(f"sky {name}: k = {k.max():.2f} (direction {int(k.argmax())}: {d[int(k.argmax())]})")
    assert k.max() <= SKY_K32


@pytest.mark.parametrize("name", ["1x1", "1x5", "6x1", "2x2", "7x5", "64x32", "ramp8x4"])
def test_env_color_fp64_matches_oracle(name):
    """The reference-epsilon mode's env_color against orc_env_color: 1e-12 relative to the colour's largest component.
    Measured on an MI355X, largest relative difference per image: 1x1 0 (asserted equal: nothing is interpolated), 1x5 5.6e-16,
    6x1 1.5e-15, 2x2 5.6e-16, 7x5 2.7e-15, 64x32 1.6e-14, ramp8x4 1.1e-15: the device's atan2 / acos differ from the host's in
    the last bit and the fraction of a texel, (w - 1) az / 2 pi, carries that times the texel index.  Not 0, so the bound stays."""
    img, d, ref = _sky_reference(name)
    got = Renderer(cases.sky_scene(img, epsilon=True), Camera()).debug_env_color(d.astype(np.float64), f64=True)
    rel = np.abs(got - ref).max(axis=1) / np.abs(ref).max(axis=1)
    print(f"sky {name} fp64: largest relative difference {rel.max():.3e} (direction {int(rel.argmax())})")
    assert rel.max() < 1e-12
    if name == "1x1":
        assert np.array_equal(got, ref)


# ------------------------------------------------------------------ fog distance
FOG_K = 2 * 4.16      # 2 x the larger k of the two media, measured on an MI355X (see the docstring)


@pytest.mark.parametrize("kind,absorption,scattering", [(0, 0.02, 0.1), (1, 0.002, 0.004)])
def test_medium_distance_matches_oracle(kind, absorption, scattering):
    """stage_distance<true> -- dmed = -__logf(xi) / sigma_t and the search limit dmed (1 + 1e-6) -- against orc_medium_sample_d on the
    same 65,536 streams: e = |dmed sigma_t - (-ln xi)| <= k 2^-24 max(1, -ln xi), k = 2 x measured.  Independent of any
    measurement: t_limit is +inf exactly when dmed >= 400, else finite and strictly beyond dmed; the thin fog produces both kinds.
    Measured on an MI355X: k = 3.06 (homogeneous_isotropic(0.02, 0.1)) and 4.16 (colored_glowing_fog(0.002, 0.004)); the test
    holds k <= 2 x 4.16 = 8.32.  Where a fast log is weakest, xi > 0.99 (645 of the 65,536 draws), the largest relative error of
    dmed is 1.6e-7 and 2.2e-7; over all draws 2.0e-7 and 2.5e-7: v_log_f32 keeps its relative accuracy up to xi = 1 - 2^-24.
    The reference is one orc_medium_sample_d call per stream, the oracle's own Medium::sample_d (0.06 s per medium)."""
    n, seed = 65536, 3
    sc = Scene()
    sc.add(Medium.homogeneous_isotropic(absorption, scattering) if kind == 0 else Medium.colored_glowing_fog(absorption, scattering))
    dmed, lim = Renderer(sc, Camera()).debug_medium_distance(n, seed=seed)
    L = pyoracle.lib()
    ref = np.empty(n)
    dist, pdf, cdf = C.c_double(), C.c_double(), C.c_double()
    for i in range(n):
        L.orc_medium_sample_d(kind, absorption, scattering, C.c_uint64(seed), i, 0, C.byref(dist), C.byref(pdf), C.byref(cdf))
        ref[i] = dist.value
    sigma_t = absorption + scattering
    mlog = ref * sigma_t                                   # -ln xi
    assert np.all(np.isfinite(dmed)) and np.all(dmed > 0)
    far = dmed >= 400.0
    assert np.all(np.isposinf(lim[far])) and np.all(np.isfinite(lim[~far])) and np.all(lim[~far] > dmed[~far])
    if kind == 1:
        assert far.any() and (~far).any()                  # xi < 0.09 gives dmed > 400
    e = np.abs(dmed.astype(np.float64) * sigma_t - mlog)
    k = e / (2.0 ** -24 * np.maximum(1.0, mlog))
    near1 = mlog < -np.log(0.99)
    rel1 = (e[near1] / mlog[near1]).max()
    print(f"fog kind {kind}: k = {k.max():.2f} (case {int(k.argmax())}), xi > 0.99: {int(near1.sum())} cases, "
          f"largest relative error {rel1:.3e}; overall largest relative error {(e / mlog).max():.3e}")
    assert near1.sum() > 300
    assert k.max() <= FOG_K
