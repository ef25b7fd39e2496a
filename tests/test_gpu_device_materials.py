"""What every path vertex runs -- sample_f, bsdf, the bounce stage, cast_ray --, one call at a time against the fp64 oracle, in both
modes: sample_f / bsdf / rotate_from_y / cast_ray of device_core.h and of kernels_f64.hip, stage_bounce of kernels.hip.  The hooks
(rpt_debug_material_sample_f, rpt_debug_material_bsdf, rpt_debug_bounce, rpt_debug_material_f64, rpt_debug_material_bsdf_f64,
rpt_debug_camera_sample, rpt_debug_camera_sample_f64) run the functions the render kernels run; the cases are in
tests/material_cases.py, and tests/test_oracle_kat.py checks there what this module takes from them (the flags' budget, the numpy
restatements).  Every test prints its figures before it asserts (pytest -s shows them).

The structured cases, appended to the 4096 random (n, wo) of each material: the six axis normals; the pole family -- normals
(a, +-1, 0), (0, +-1, a), (a, +-1, -a), a from 1e-3 down to 1e-30 with sin(pi) among them (fp64: 2.2e-16 and 2.3e-16 too, on both
sides of the threshold of nalgebra's rotation_between, and 1e-200), given as they arrive, not normalised; for Phong the same family
on the mirror direction (n = +-Y, wo from the family) and the mirror direction +-Y itself --; wo = n and grazing wo; for glass normal
incidence from both sides, n.wo = 0, and Snell's k at +-1e-3 and +-1e-6 on 16 streams each.

fp32 bounds, from an error model of the device code, stated before anything was measured:
  wi   5e-5 absolute.  Phong: + min(1.8e-7 / st, 6e-4), st the lobe's sine: 1 - ct^2 is formed from a ct that __powf leaves 2 ulp
       (1.2e-7) off and loses 3.6e-7 absolutely, sqrt turns that into 3.6e-7 / (2 st), at most sqrt(3.6e-7).  Glass, refracted:
       + min(sqrt(dk), dk / (2 sqrt(k))), dk = 3e-7 eta^2: five roundings of terms up to eta^2 in k = 1 - eta^2 (1 - ci^2), through
       cos_t = sqrt(k).
  pdf  2e-4 relative.  Phong: + W(ct), W(c) = shininess (4e-7 / c + 2^-22 |log2 c|), the error of __powf's argument and of its
       exponent product; never below 1e-6 of the lobe's peak (shininess + 1) / 2 pi.
  f    1e-6 relative (a product of four fp32 factors).  Phong: + W(c), c the lobe cosine, never below 1e-6 of the peak
       albedo (shininess + 2) / 2 pi.
  k    the sum of its factors' bounds: k = |wi.n| f / pdf (/ 0.8), with |wi.n| off by the bound of wi times |n|_1.
  camera origin 2e-6 (1 + |eye| + aperture); direction 5e-6 + aperture / focal_distance * 2e-6, and for a lens
       + 2^-23 (|eye| + aperture) / focal_distance: focal - o subtracts two points of the eye's magnitude, each rounded to fp32.
Decisions (Some / None, reflect or refract, the bounce flag, the draws of the lens loop) equal the oracle's except on flagged
cases -- |u - sr| < 4e-6, |k| < 1e-5, |n.wi| or |n.wo| < 1e-6 (not where the products are exact: axis normals), a lens candidate
with |x^2 + y^2 - 1| < 1e-6 --, where the device must equal one of the reference's outcomes within the same bounds."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

from oracle import pyoracle
from oracle.pyoracle import OracleScene
from rpt_amd import Material, Medium, Renderer, _lib, api
from rpt_amd._lib import vp as _vp
from rpt_amd.api import hex_color, material_desc
from tests import material_cases as mc
from tests.util import rel_rms

pytestmark = pytest.mark.gpu

SEED = mc.SEED
FOG = Medium.homogeneous_isotropic(0.02, 0.1)


def _dot(a, b):
    return np.einsum("ij,ij->i", a, b)


def _absmax(a):
    return np.abs(a).reshape(a.shape[0], -1).max(axis=1)


def _report(title, ratios, labels):
    """Prints the largest error / bound per output and where it is; returns the outputs that exceed their bound."""
    parts, bad = [], []
    for k, r in ratios.items():
        r = np.where(np.isnan(r), np.inf, r)
        i = int(r.argmax())
        parts.append(f"{k} {r[i]:.3f} (case {i}{' ' + labels[i] if labels[i] else ''})")
        if not r[i] < 1.0:
            worst = np.flatnonzero(~(r < 1.0))
            bad.append(f"{k}: {worst.size} cases, e.g. " + ", ".join(f"{j} {labels[j]} {r[j]:.3g}" for j in worst[:6]))
    print(f"{title}: error / bound: " + ", ".join(parts))
    return bad


# ------------------------------------------------------------------ references (computed once per material and precision, shared)
@functools.lru_cache(maxsize=None)
def _ref_sample(name, f64):
    n, wo, labels = mc.inputs(name, f64)
    ref = pyoracle.material_sample(mc.materials()[name], n, wo, seed=SEED)
    for a in ref.values():
        a.setflags(write=False)
    return ref


@functools.lru_cache(maxsize=None)
def _draws(m):
    u = mc.uniforms(SEED, m, 4)
    u.setflags(write=False)
    return u


def _lobe(name, m, off):
    """ct, st of the sampled lobe direction from the reference's draws; `off`: draws the stage makes before sample_f."""
    return mc.lobe_cosine(name, _draws(m)[:, off + 1])


def _W(shin, c):
    if shin == 0:
        return np.zeros_like(c)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(c > 0, shin * (4e-7 / c + 2.0 ** -22 * np.abs(np.log2(c))), np.inf)


def _wi_bound(name, n, wo, refracted, off=0):
    """fp32 bound of a sampled direction (see the module docstring)."""
    mat = mc.materials()[name]
    b = np.full(n.shape[0], 5e-5)
    if mat.kind == Material.PHONG:
        _, st = _lobe(name, n.shape[0], off)
        with np.errstate(divide="ignore"):
            b = b + np.minimum(1.8e-7 / st, 6e-4)
    if mat.kind == Material.TRANSMISSIVE:
        g = mc.glass_terms(n, wo, mat.ior)
        dk = 3e-7 * g["eta"] ** 2
        with np.errstate(divide="ignore", invalid="ignore"):
            w = np.minimum(np.sqrt(dk), dk / (2.0 * np.sqrt(np.maximum(g["k"], 0.0))))
        b = b + np.where(refracted, w, 0.0)
    return b


def _pdf_bound(name, pdf_ref, off=0):
    mat = mc.materials()[name]
    if mat.kind != Material.PHONG:
        return 2e-4 * np.abs(pdf_ref)
    ct, _ = _lobe(name, pdf_ref.shape[0], off)
    with np.errstate(invalid="ignore"):
        b = np.abs(pdf_ref) * (2e-4 + _W(mat.shininess, ct))
    return np.maximum(np.where(np.isnan(b), 0.0, b), 1e-6 * (mat.shininess + 1.0) / (2.0 * math.pi))


def _f_bound(name, f_ref, n, wo, wi):
    """(m, 3) bound of a bsdf value; where the reference is zero the device must be."""
    mat = mc.materials()[name]
    if mat.kind != Material.PHONG:
        return 1e-6 * np.abs(f_ref)
    c = mc.phong_cosine(n, wo, wi)
    with np.errstate(invalid="ignore"):
        b = np.abs(f_ref) * (1e-6 + _W(mat.shininess, c))[:, None]
    floor = 1e-6 * mat.albedo * (mat.shininess + 2.0) / (2.0 * math.pi)
    return np.maximum(np.where(np.isnan(b), 0.0, b), np.where(np.any(f_ref != 0, axis=1)[:, None], floor[None, :], 0.0))


def _ratio(got, ref, bound):
    """max over components of |got - ref| / bound; 0 / 0 = 0, x / 0 = inf."""
    d = np.abs(np.asarray(got, np.float64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(d == 0, 0.0, d / bound)
    return r.reshape(r.shape[0], -1).max(axis=1)


def _sample_outcomes(name, n, wo, ref_some, ref_wi, us, live=None):
    """The outcomes sample_f may have on a device: the reference's own and, on flagged glass cases (|u - sr| < 4e-6, |k| < 1e-5;
    `us` is the draw compared with sr), the neighbouring ones.  -> list of (allowed, some, wi, refracted), the flagged mask."""
    m = n.shape[0]
    mat = mc.materials()[name]
    live = np.ones(m, bool) if live is None else live
    if mat.kind != Material.TRANSMISSIVE:
        return [(np.ones(m, bool), ref_some == 1, ref_wi, np.zeros(m, bool))], np.zeros(m, bool)
    reflect, refract, g = mc.glass_outcomes(n, wo, mat.ior)
    f_usr, f_k = (np.abs(us - g["sr"]) < 4e-6) & live, (np.abs(g["k"]) < 1e-5) & live
    yes, no = np.ones(m, bool), np.zeros(m, bool)
    outs = [(yes, ref_some == 1, ref_wi, (ref_some == 1) & ~(us < g["sr"])),
            (f_usr, yes, reflect, no),                                                  # reflect after all
            ((f_usr & (g["k"] >= 0)) | f_k, yes, refract, yes),                         # refract after all
            ((f_usr & (g["k"] < 0)) | f_k, no, np.zeros((m, 3)), no)]                   # None after all
    return outs, f_usr | f_k


# ------------------------------------------------------------------ sample_f and bsdf, fp32
def _fp32_sample_f(name, n, wo):
    m = n.shape[0]
    n32, wo32 = np.ascontiguousarray(n, np.float32), np.ascontiguousarray(wo, np.float32)
    wi, pdf, some = np.zeros((m, 3), np.float32), np.zeros(m, np.float32), np.zeros(m, np.int32)
    md = material_desc(mc.materials()[name], _lib.MaterialDesc)
    _lib.check(_lib.load().rpt_debug_material_sample_f(C.byref(md), m, _vp(n32), _vp(wo32), C.c_uint64(SEED), _vp(wi), _vp(pdf), _vp(some)))
    return some, wi, pdf


def _fp32_bsdf(name, n, wo, wi):
    a = [np.ascontiguousarray(x, np.float32) for x in (n, wo, wi)]
    f = np.zeros((n.shape[0], 3), np.float32)
    md = material_desc(mc.materials()[name], _lib.MaterialDesc)
    _lib.check(_lib.load().rpt_debug_material_bsdf(C.byref(md), n.shape[0], _vp(a[0]), _vp(a[1]), _vp(a[2]), _vp(f)))
    return f


@pytest.mark.parametrize("name", mc.MATERIAL_NAMES)
def test_sample_f_fp32_matches_oracle_per_call(name):
    """sample_f (fp32) through rpt_debug_material_sample_f against orc_material_sample on every case of the material: Some / None
    equal (flagged glass cases: one of the reference's outcomes), wi and pdf within the bounds of the module docstring, no NaN.
    (The draw counts are test_bounce_fp32_matches_oracle_per_call's.)
    Measured on an MI355X, largest error / bound (wi, pdf): lambertian .009 .001, phong0 .016 0, phong1 .021 .001, phong6 .041 .003,
    phong50 .063 .009, phong1000 .133 .065, mirror .005 0, glass1.0 .006 0, glass1.05 .372, glass1.5 .204, glass2.4 .233,
    glass1over1.5 .176 (each at a k = +1e-6 case; pdf 0).  No flagged case was decided the other way.
    With the rotation of the commit before (rotating whenever b.x^2 + b.z^2 > 0; measured once, with that threshold put back)
    Lambertian and every Phong fail here, on pole cases only.  The six cases with a = 1e-20, of either sign of Y, are NaN (s2 =
    1e-40 is a denormal that v_rsq_f32 takes for zero: 0 * inf).  With a = sin(pi) and a = 1e-17 the direction is finite and
    turned the other way, 0.67 to 2.0 off: Lambertian at the normals (a, -1, 0) and (a, -1, -a) (at (0, -1, a) the axis Y x b is X
    itself, so both rotations agree; next to +Y the rotation left out is nothing), Phong at all three mirror directions next to
    -Y (the reference's identity against a half-turn).  a = 1e-30 squares to zero and took the fallback already.  In fp64 the
    same build is wrong at y = -1 for every a from 2.2e-16 down to 1e-30 (Lambertian 9 cases, Phong 14), never NaN."""
    n, wo, labels = mc.inputs(name, False)
    m = n.shape[0]
    ref = _ref_sample(name, False)
    some, wi, pdf = _fp32_sample_f(name, n, wo)
    nan = np.flatnonzero(~(np.isfinite(wi).all(axis=1) & np.isfinite(pdf)))
    assert nan.size == 0, f"{name}: not finite in cases {nan[:8]} {labels[nan[:8]]}"
    outs, flagged = _sample_outcomes(name, n, wo, ref["some"], ref["wi"], _draws(m)[:, 0])
    best = np.full(m, np.inf)
    for allowed, o_some, o_wi, refr in outs:
        r = np.where(o_some, _ratio(wi, o_wi, _wi_bound(name, n, wo, refr)[:, None]), 0.0)
        best = np.where(allowed & ((some == 1) == o_some), np.minimum(best, r), best)
    other = (some != ref["some"])
    print(f"{name}: {m} cases, {int(flagged.sum())} flagged, {int((other & flagged).sum())} of them decided the other way")
    differ = np.flatnonzero(other & ~flagged)
    assert differ.size == 0, f"{name}: Some / None differs in cases {differ[:8]} {labels[differ[:8]]}"
    both = (ref["some"] == 1) & (some == 1)
    bad = _report(name, {"wi": best, "pdf": np.where(both, _ratio(pdf, ref["pdf"], _pdf_bound(name, ref["pdf"])), 0.0)}, labels)
    assert not bad, f"{name}: " + "; ".join(bad)


@pytest.mark.parametrize("name", mc.MATERIAL_NAMES)
def test_bsdf_fp32_matches_oracle_per_call(name):
    """bsdf (fp32) through rpt_debug_material_bsdf against orc_material_bsdf_n: at the oracle's sampled direction of every sample_f
    case, at 4096 directions over the whole sphere, and at tangent-plane wi and wo of the axis normals with +0.0 and -0.0 normal
    components (the sign of a zero decides: exact in every precision, so compared like any unflagged case).  Flagged cases
    (|n.wi| or |n.wo| < 1e-6) must equal zero or the value with both sign tests passed.
    Measured on an MI355X, largest error / bound: mirror, glass 0 (bit-equal to the rounded reference); lambertian, phong0 .040,
    phong1 .189, phong6 .281, phong50 .351, phong1000 .387; 2 to 6 flagged cases of about 8,000 per material."""
    mat = mc.materials()[name]
    n, wo, labels = mc.inputs(name, False)
    ref_s = _ref_sample(name, False)
    keep = ref_s["some"] == 1
    n2, wo2, wi2, labels2 = mc.bsdf_inputs(name, False)
    N_, WO = np.concatenate([n[keep], n2]), np.concatenate([wo[keep], wo2])
    WI = np.concatenate([ref_s["wi"][keep].astype(np.float32).astype(np.float64), wi2])
    LAB = np.concatenate([labels[keep], labels2])
    ref = pyoracle.material_bsdf(mat, N_, WO, WI)
    got = _fp32_bsdf(name, N_, WO, WI).astype(np.float64)
    assert np.all(np.isfinite(got))
    flagged = mc.bsdf_flags(N_, WO, WI) & ~mc.is_exact_zero(LAB)
    alt = mc.bsdf_unsigned(name, N_, WO, WI)
    r_own = _ratio(got, ref, _f_bound(name, ref, N_, WO, WI))
    r_zero = _ratio(got, np.zeros_like(ref), np.zeros_like(ref))
    r_alt = _ratio(got, alt, _f_bound(name, alt, N_, WO, WI))
    r = np.where(flagged, np.minimum(r_own, np.minimum(r_zero, r_alt)), r_own)
    print(f"{name}: {N_.shape[0]} cases, {int(flagged.sum())} flagged, nonzero share {np.any(ref != 0, axis=1).mean():.3f}")
    bad = _report(name, {"f": r}, LAB)
    assert not bad, f"{name}: " + "; ".join(bad)


# ------------------------------------------------------------------ the bounce stage, fp32
@functools.lru_cache(maxsize=None)
def _ref_bounce(name, fog):
    n, wo, _ = mc.inputs(name, False)
    ref = pyoracle.bounce(mc.materials()[name], n, -wo, max_bounces=3, depth=1, seed=SEED, medium=FOG if fog else None)
    for a in ref.values():
        a.setflags(write=False)
    return ref


@pytest.mark.parametrize("mode", ["plain", "fog"])
@pytest.mark.parametrize("name", mc.MATERIAL_NAMES)
def test_bounce_fp32_matches_oracle_per_call(name, mode):
    """stage_bounce<MEDIUM, false> at a surface event through rpt_debug_bounce against orc_bounce (the halves of the oracle's own
    trace_ray): `plain` is a scene without a medium (depth 1 of 3 bounces), `fog` one with a medium (roulette, pdf * 0.8).  The
    word after the stage is equal in EVERY case, flagged or not: this is the draw count of sample_f too.  The flag (the path goes
    on with a non-zero weight) equals the oracle's except on flagged cases and where the reference's weight is within its own
    bound of zero (fp32 may underflow there); wi and k within the bounds of the module docstring, on flagged cases against the
    outcome the device took.
    Measured on an MI355X: no draw-count difference anywhere, no flag decided the other way; largest error / bound (wi, k), plain
    then fog: lambertian .009 .002 / .006 .002, phong0 .018 .005 / .024 .005, phong1 .021 .005 / .019 .005, phong6 .041 .010 /
    .016 .005, phong50 .063 .034 / .052 .030, phong1000 .133 .165 / .086 .168, mirror .005 .001, glass .002-.003 .001."""
    mat = mc.materials()[name]
    fog = mode == "fog"
    n, wo, labels = mc.inputs(name, False)
    m = n.shape[0]
    rr, off = (0.8, 1) if fog else (1.0, 0)
    ref = _ref_bounce(name, fog)
    got = api.debug_bounce(mat, n, -wo, max_bounces=3, depth=1, seed=SEED, in_medium=fog)
    nan = np.flatnonzero(~(np.isfinite(got["wi"]).all(axis=1) & np.isfinite(got["k"]).all(axis=1)))
    assert nan.size == 0, f"{name}/{mode}: not finite in cases {nan[:8]} {labels[nan[:8]]}"
    differ = np.flatnonzero(got["next_word"] != ref["next_word"])
    assert differ.size == 0, f"{name}/{mode}: draw counts differ in cases {differ[:8]} {labels[differ[:8]]}"
    won = wo / np.linalg.norm(wo, axis=1, keepdims=True)                 # wo = -normalize(rd), as trace_ray forms it
    u = _draws(m)
    live = (u[:, 0] < 0.8) if fog else np.ones(m, bool)                  # the roulette: equal draws, an exact comparison
    assert np.array_equal(ref["cont"] == 1, live) or mat.kind == Material.TRANSMISSIVE
    pdf = mc.sample_pdf(name, u[:, off + 1])
    pb = _pdf_bound(name, pdf, off)
    outs, s_flagged = _sample_outcomes(name, n, won, np.where(ref["cont"] == 1, 1, 0), ref["wi"], u[:, off], live)
    g_on = got["flag"] == 1
    best = np.full(m, np.inf)
    best_wi, best_k = np.full(m, np.inf), np.full(m, np.inf)
    ref_flag = (ref["cont"] == 1) & np.any(ref["k"] != 0, axis=1)
    soft = s_flagged.copy()                                              # cases whose flag may go either way
    for allowed, goes, o_wi, refr in outs:
        goes = goes & live
        wb = _wi_bound(name, n, won, refr, off)
        bf = mc.bsdf_flags(n, won, o_wi) & goes
        soft |= bf & allowed
        dotn = np.abs(_dot(o_wi, n))
        for c_allowed, f in ((np.ones(m, bool), pyoracle.material_bsdf(mat, n, won, o_wi)), (bf, np.zeros((m, 3))),
                             (bf, mc.bsdf_unsigned(name, n, won, o_wi))):
            scale = (1.0 / (pdf * rr))[:, None]
            k = np.where(goes[:, None], dotn[:, None] * f * scale, 0.0)
            kb = (dotn[:, None] * _f_bound(name, f, n, won, o_wi) + np.abs(f) * (wb * np.abs(n).sum(axis=1))[:, None]) * scale \
                + np.abs(k) * (pb / pdf)[:, None]
            zeroish = ~goes | (np.abs(k) <= kb).all(axis=1)               # the weight may come out as zero: the flag goes with it
            soft |= allowed & c_allowed & goes & zeroish & np.any(k != 0, axis=1)
            r_wi = _ratio(got["wi"], o_wi, wb[:, None])
            r_k = _ratio(got["k"], k, kb)
            r_on = np.maximum(r_wi, r_k)
            fit = allowed & c_allowed & np.where(g_on, goes, zeroish)
            r = np.where(g_on, r_on, 0.0)
            better = fit & (r < best)
            best = np.where(better, r, best)
            best_wi = np.where(better, np.where(g_on, r_wi, 0.0), best_wi)
            best_k = np.where(better, np.where(g_on, r_k, 0.0), best_k)
    other = g_on != ref_flag
    print(f"{name}/{mode}: {m} cases, {int(ref_flag.sum())} paths go on, {int(soft.sum())} cases flagged or with a weight within its "
          f"bound of zero, {int((other & soft).sum())} of them decided the other way")
    differ = np.flatnonzero(other & ~soft)
    assert differ.size == 0, f"{name}/{mode}: the bounce flag differs in cases {differ[:8]} {labels[differ[:8]]}"
    bad = _report(f"{name}/{mode}", {"wi": best_wi, "k": best_k}, labels)
    assert not bad, f"{name}/{mode}: " + "; ".join(bad)


def test_bounce_fp32_medium_event_and_last_depth():
    """stage_bounce at a medium event (roulette, the phase sample of src/medium.rs:87-93, k = albedo * colour / 0.8) in the fog and
    in the glowing fog above y = 250, and at a surface at depth == max_bounces in a scene without a medium (no draw, no bounce).
    Bounds: wi 5e-5; k 4e-7 relative (three fp32 products of rounded factors).
    Measured on an MI355X, largest error / bound: wi .002, k .203 in the fog and 0 in the glowing fog."""
    mat = mc.materials()["lambertian"]
    n, wo, labels = mc.inputs("lambertian", False)
    m = n.shape[0]
    for medium, pos, colour in ((FOG, (0.0, 0.0, 0.0), hex_color(0xD2B48C)), (Medium.colored_glowing_fog(0.02, 0.03), (0.0, 300.0, 0.0), hex_color(0xFF0000))):
        ref = pyoracle.bounce(mat, n, -wo, seed=SEED, medium=medium, medium_event=True, position=pos)
        got = api.debug_bounce(mat, n, -wo, seed=SEED, in_medium=True, medium_event=True,
                               albedo_med=medium.scattering / (medium.absorption + medium.scattering), medium_color=colour)
        assert np.array_equal(got["next_word"], ref["next_word"])
        assert np.array_equal(got["flag"] == 1, (ref["cont"] == 1) & np.any(ref["k"] != 0, axis=1))
        assert 0.75 < (ref["cont"] == 1).mean() < 0.85
        bad = _report(f"medium event kind {medium.kind}", {"wi": _ratio(got["wi"], ref["wi"], 5e-5), "k": _ratio(got["k"], ref["k"], 4e-7 * np.abs(ref["k"]))}, labels)
        assert not bad, "; ".join(bad)
    ref = pyoracle.bounce(mat, n, -wo, max_bounces=3, depth=3, seed=SEED)
    got = api.debug_bounce(mat, n, -wo, max_bounces=3, depth=3, seed=SEED)
    first = _first_words(m)
    assert np.array_equal(got["next_word"], ref["next_word"]) and np.array_equal(ref["next_word"], first)
    assert not got["flag"].any() and not ref["cont"].any() and not got["k"].any() and not got["wi"].any()


def _first_words(m):
    out = np.zeros(m, dtype=np.uint32)
    for i in range(m):
        pyoracle.lib().orc_rng_u32(C.c_uint64(SEED), i, 0, 1, _vp(out[i:]))
    return out


# ------------------------------------------------------------------ sample_f and bsdf, reference-epsilon mode
# Largest differences measured on an MI355X: wi (absolute), pdf, f (relative).  Zero: the outputs equal the oracle's bit for bit (mirror
# and glass use + - * / sqrt only); elsewhere sin, cos, acos and pow are the device library's against the host's.  The f of
# test_bsdf_f64_matches_oracle_per_call stays below 4.2e-16 for every material.
F64_MEASURED = {
    "lambertian": (6.661e-16, 1.912e-15, 0.0), "phong0": (6.106e-16, 0.0, 0.0), "phong1": (7.078e-16, 2.688e-15, 9.596e-15),
    "phong6": (6.800e-16, 3.651e-15, 5.140e-15), "phong50": (1.221e-15, 6.236e-15, 1.794e-14),
    "phong1000": (2.331e-15, 1.114e-13, 3.333e-13), "mirror": (0.0, 0.0, 0.0), "glass1.0": (0.0, 0.0, 0.0),
    "glass1.05": (0.0, 0.0, 0.0), "glass1.5": (0.0, 0.0, 0.0), "glass2.4": (0.0, 0.0, 0.0), "glass1over1.5": (0.0, 0.0, 0.0),
}


def _f64_limits(name):
    """-> limits of wi (absolute), pdf, f (relative): twice the measured difference, zero where equality was measured; never above
    the mode's 1e-12."""
    return [2.0 * v for v in F64_MEASURED[name]]


@pytest.mark.parametrize("name", mc.MATERIAL_NAMES)
def test_material_f64_matches_oracle_per_call(name):
    """The reference-epsilon mode's sample_f, and its bsdf at the sampled direction, through rpt_debug_material_f64 against
    orc_material_sample on every case, fp64 inputs (the pole family with 2.2e-16, 2.3e-16 and 1e-200 too): next_word and Some / None
    equal in every case, nothing flagged; wi (absolute), pdf and f (relative) within the limits of F64_MEASURED, all below 1e-12."""
    mat = mc.materials()[name]
    n, wo, labels = mc.inputs(name, True)
    ref = _ref_sample(name, True)
    got = api.debug_material_f64(mat, n, wo, seed=SEED)
    assert all(np.all(np.isfinite(got[k])) for k in ("wi", "pdf", "f"))
    for key in ("next_word", "some"):
        differ = np.flatnonzero(got[key] != ref[key])
        assert differ.size == 0, f"{name}: {key} differs in cases {differ[:8]} {labels[differ[:8]]}"
    with np.errstate(divide="ignore", invalid="ignore"):
        d = {"wi": _absmax(got["wi"] - ref["wi"]),
             "pdf": np.where(ref["pdf"] != got["pdf"], np.abs(got["pdf"] - ref["pdf"]) / np.abs(ref["pdf"]), 0.0),
             "f": np.where(ref["f"] != got["f"], np.abs(got["f"] - ref["f"]) / np.abs(ref["f"]), 0.0).max(axis=1)}
    lim = dict(zip(("wi", "pdf", "f"), _f64_limits(name)))
    print(f"{name}: largest difference: " + ", ".join(f"{k} {v.max():.3e} (case {int(v.argmax())} {labels[int(v.argmax())]})" for k, v in d.items()))
    for k, v in d.items():
        assert lim[k] <= 1e-12 and np.all(v <= lim[k]), f"{name}: {k} {v.max():.3e} > {lim[k]:.3e} in case {int(v.argmax())} {labels[int(v.argmax())]}"


@pytest.mark.parametrize("name", mc.MATERIAL_NAMES)
def test_bsdf_f64_matches_oracle_per_call(name):
    """The mode's bsdf through rpt_debug_material_bsdf_f64 on the inputs of the fp32 bsdf test, unrounded: every sign decision
    equal, the values within the limit of F64_MEASURED for f."""
    mat = mc.materials()[name]
    n, wo, wi, labels = mc.bsdf_inputs(name, True)
    ref = pyoracle.material_bsdf(mat, n, wo, wi)
    got = api.debug_material_bsdf_f64(mat, n, wo, wi)
    assert np.array_equal(got == 0, ref == 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        d = np.where(ref != got, np.abs(got - ref) / np.abs(ref), 0.0).max(axis=1)
    lim = max(_f64_limits(name)[2], 2 * 4.2e-16) if mat.kind == Material.PHONG and mat.shininess > 0 else _f64_limits(name)[2]
    print(f"{name}: largest difference: f {d.max():.3e} (case {int(d.argmax())} {labels[int(d.argmax())]}), nonzero share {np.any(ref != 0, axis=1).mean():.3f}")
    assert lim <= 1e-12 and np.all(d <= lim)


# ------------------------------------------------------------------ the camera sample, both modes
@functools.lru_cache(maxsize=None)
def _ref_camera(name, w, h, sample):
    ref = pyoracle.camera_rays(mc.cameras()[name], w, h, sample=sample, seed=SEED)
    for a in ref.values():
        a.setflags(write=False)
    return ref


@pytest.mark.parametrize("name", mc.CAMERA_NAMES)
def test_camera_sample_fp32_matches_oracle_per_pixel(name):
    """render_kernel's camera sample (pixel_xn / pixel_yn, the two jitter draws, cast_ray with its lens loop) through
    rpt_debug_camera_sample against orc_camera_rays: every pixel of 33 x 17, 17 x 33, 1 x 1 and 64 x 64 frames, sample indices 0 and
    1023.  next_word equal in every pixel (no pixel of these frames is flagged: tests/test_oracle_kat.py), so the lens loop
    rejects what the reference rejects; origin and direction within the bounds of the module docstring.
    Measured on an MI355X, largest error / bound (origin, direction): pinhole-narrow 0 .022, pinhole-wide-skew 0 .027,
    lens1e-6-wide .005 .023, lens0.05-near-skew .011 .167, lens2-wide .016 .031."""
    cam = mc.cameras()[name]
    ob = 2e-6 * (1.0 + np.linalg.norm(cam.eye) + cam.aperture)
    db = 5e-6
    if cam.aperture > 0:
        db += cam.aperture / cam.focal_distance * 2e-6 + 2.0 ** -23 * (np.linalg.norm(cam.eye) + cam.aperture) / cam.focal_distance
    worst = {"o": 0.0, "d": 0.0}
    for w, h in mc.FRAMES:
        for sample in mc.SAMPLES:
            ref = _ref_camera(name, w, h, sample)
            got = api.debug_camera_sample(cam, w, h, sample=sample, seed=SEED)
            assert np.all(np.isfinite(got["o"])) and np.all(np.isfinite(got["d"]))
            differ = np.flatnonzero(got["next_word"] != ref["next_word"])
            assert differ.size == 0, f"{name} {w}x{h} sample {sample}: draw counts differ in pixels {differ[:8]}"
            ro, rd = _ratio(got["o"], ref["o"], ob), _ratio(got["d"], ref["d"], db)
            worst = {"o": max(worst["o"], ro.max()), "d": max(worst["d"], rd.max())}
            assert ro.max() < 1 and rd.max() < 1, f"{name} {w}x{h} sample {sample}: o {ro.max():.3f} (pixel {int(ro.argmax())}), d {rd.max():.3f} (pixel {int(rd.argmax())})"
    print(f"{name}: error / bound: o {worst['o']:.3f}, d {worst['d']:.3f} (bounds {ob:.2e}, {db:.2e})")


CAMERA_F64_EQUAL = True         # measured on an MI355X: every origin and direction equals the oracle's bit for bit


@pytest.mark.parametrize("name", mc.CAMERA_NAMES)
def test_camera_sample_f64_matches_oracle_per_pixel(name):
    """The reference-epsilon mode's camera sample through rpt_debug_camera_sample_f64 on the same frames: next_word equal in every
    pixel; direction within 1e-12 absolutely, origin within 1e-12 relatively -- and, as measured (+ - * / sqrt only), equal bit for bit."""
    cam = mc.cameras()[name]
    worst = {"o": 0.0, "d": 0.0}
    for w, h in mc.FRAMES:
        for sample in mc.SAMPLES:
            ref = _ref_camera(name, w, h, sample)
            got = api.debug_camera_sample(cam, w, h, sample=sample, seed=SEED, f64=True)
            assert np.array_equal(got["next_word"], ref["next_word"]), f"{name} {w}x{h} sample {sample}"
            do = _absmax(got["o"] - ref["o"]) / np.linalg.norm(ref["o"], axis=1)
            dd = _absmax(got["d"] - ref["d"])
            worst = {"o": max(worst["o"], do.max()), "d": max(worst["d"], dd.max())}
    print(f"{name}: largest difference: o {worst['o']:.3e} (relative), d {worst['d']:.3e}")
    assert worst["o"] <= 1e-12 and worst["d"] <= 1e-12
    if CAMERA_F64_EQUAL:
        assert worst["o"] == 0 and worst["d"] == 0


# ------------------------------------------------------------------ one frame with such normals per mode
def _upside_down(epsilon):
    sc, cam, o, d = mc.upside_down_scene(epsilon)
    r = Renderer(sc, cam).width(48).height(48).max_bounces(3).seed(4)
    t, obj, nrm = r.get_closest_hit_f64(o, d) if epsilon else r.get_closest_hit(o, d)
    print(f"normals of the faces turned upside down ({'fp64' if epsilon else 'fp32'}): objects {obj}, {nrm.tolist()}")
    assert list(obj) == [1, 2]
    # the faces' normals carry sin(pi) as the reference's do: below the rotation threshold, not zero
    assert np.all(np.abs(nrm[:, 1] + 1.0) < 1e-6) and np.all(np.abs(nrm[:, 0]) > 0) and np.all(np.abs(nrm[:, 0]) < mc.EPS64)
    got = r.sample_array(8)
    exp = OracleScene(sc).render(cam, 48, 48, 8, 3, seed=4, robust=0 if epsilon else 1)
    assert np.all(np.isfinite(got)) and exp.mean() > 0
    return got, exp


def test_frame_with_faces_turned_by_pi_matches_oracle_fp32():
    """A Lambertian quad and a Phong cube turned with rotate_z(pi) over a floor, 48 x 48 x 8 spp, 3 bounces, against the oracle at
    the same seed, at the tolerances of test_all_materials_lights_and_media_match_oracle (4e-3 relative RMS, mean within 2e-3).
    Both faces' normals arrive on the device as (-1.2246e-16, -1, 0).  Measured on an MI355X: 6.2e-8 relative RMS; with the
    rotation of the commit before 6.9e-3 (the other half-turn on the quad: other paths); the fp64 frame 3.6e-7 and 6.9e-3."""
    got, exp = _upside_down(False)
    print(f"rel RMS {rel_rms(got, exp):.3e}, mean {got.mean():.6f} vs {exp.mean():.6f}")
    assert rel_rms(got, exp) < 4e-3
    assert abs(got.mean() - exp.mean()) / exp.mean() < 2e-3


def test_frame_with_faces_turned_by_pi_matches_oracle_f64():
    """The same frame in the reference-epsilon mode against the oracle's literal policy, at the tolerances of test_gpu_epsilon.py's
    test_all_materials_shapes_and_both_media (5e-3 relative RMS, mean within 5e-4)."""
    got, exp = _upside_down(True)
    print(f"rel RMS {rel_rms(got, exp):.3e}, mean {got.mean():.6f} vs {exp.mean():.6f}")
    assert rel_rms(got, exp) < 5e-3
    assert abs(got.mean() - exp.mean()) < 5e-4 * exp.mean()
