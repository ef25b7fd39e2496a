"""The a-trous denoiser (rpt_denoise*), the parts that need no GPU: the numpy restatement of the definition (tests/denoise_ref.py)
against a pixel-by-pixel transcription of include/rpt_hip.h and on inputs where the definition is exact, the argument checks of the
new entry points that precede every device call, and the Python wrappers' refusals.

(RPT_ERR_STATE of rpt_buffer_mean_device / rpt_buffer_denoised_image -- fewer than two batches -- needs an rpt_buffer, which only a
device can hold: tests/test_gpu_denoise.py.)"""
import ctypes as C
import math
from fractions import Fraction

import numpy as np
import pytest

from rpt_amd import Camera, DenoiseParams, Denoiser, Renderer, Scene, _lib
from tests.denoise_ref import DEMODULATE, G, H, MATCH_ID, denoise_ref

NAN = float("nan")


def scalar_denoise(rgb, var, albedo, normal, depth, passes, flags, sc, sn, sd):
    """The definition, one pixel and one Python float operation at a time."""
    h, w = len(rgb), len(rgb[0])
    den = [[[(albedo[y][x][k] if flags & DEMODULATE and albedo[y][x][k] > 0.0 else 1.0) for k in range(3)] for x in range(w)] for y in range(h)]
    c = [[[rgb[y][x][k] / den[y][x][k] for k in range(3)] for x in range(w)] for y in range(h)]
    v = [[(var[y][x] if var is not None else 0.0) for x in range(w)] for y in range(h)]
    n = [[[(normal[y][x][k] if normal is not None else 0.0) for k in range(3)] for x in range(w)] for y in range(h)]
    z = [[(depth[y][x][0] if depth is not None else 0.0) for x in range(w)] for y in range(h)]
    ids = [[(depth[y][x][2] if depth is not None else 0.0) for x in range(w)] for y in range(h)]
    for i in range(passes):
        s = 1 << i
        c2, v2 = [[None] * w for _ in range(h)], [[None] * w for _ in range(h)]
        for y in range(h):
            for x in range(w):
                if sc > 0.0:
                    sv = sg = 0.0
                    for dy in (-1, 0, 1):
                        for dx in (-1, 0, 1):
                            if 0 <= y + dy < h and 0 <= x + dx < w:
                                sv = sv + (G[dy] * G[dx]) * v[y + dy][x + dx]
                                sg = sg + G[dy] * G[dx]
                    kp = 1.0 / ((sc * sc) * (sv / sg + 1e-12))
                Wt, Ct, Vt = 0.0, [0.0, 0.0, 0.0], 0.0
                for dy in (-2, -1, 0, 1, 2):
                    for dx in (-2, -1, 0, 1, 2):
                        qy, qx = y + s * dy, x + s * dx
                        if not (0 <= qy < h and 0 <= qx < w):
                            continue
                        xx = 0.0
                        if sc > 0.0:
                            e = [(c[qy][qx][k] - c[y][x][k]) * den[y][x][k] for k in range(3)]
                            xx = xx + ((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]) * kp
                        if sn > 0.0:
                            e = [(n[qy][qx][k] - n[y][x][k]) * (1.0 / sn) for k in range(3)]
                            xx = xx + ((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2])
                        if sd > 0.0:
                            e = (z[qy][qx] - z[y][x]) * (1.0 / (sd * float(s)))
                            xx = xx + e * e
                        if not xx < 4.0 or (flags & MATCH_ID and not ids[qy][qx] == ids[y][x]):
                            continue
                        t = 1.0 - xx * 0.25
                        t2 = t * t
                        wt = (t2 * t2) * (H[dy] * H[dx])
                        Wt = Wt + wt
                        Ct = [Ct[k] + wt * c[qy][qx][k] for k in range(3)]
                        Vt = Vt + (wt * wt) * v[qy][qx]
                if Wt > 0.0:
                    c2[y][x], v2[y][x] = [Ct[k] / Wt for k in range(3)], Vt / (Wt * Wt)
                else:
                    c2[y][x], v2[y][x] = c[y][x], v[y][x]
        c, v = c2, v2
    return (np.array([[[c[y][x][k] * den[y][x][k] for k in range(3)] for x in range(w)] for y in range(h)]).reshape(h, w, 3),
            np.array(v, dtype=np.float64).reshape(h, w))


def random_case(seed, w, h, ids=4):
    rng = np.random.default_rng(seed)
    rgb = rng.uniform(0.0, 2.0, (h, w, 3))
    var = rng.uniform(0.0, 0.05, (h, w))
    albedo = rng.choice([0.0, 0.25, 0.5, 0.9], (h, w, 3))
    normal = rng.normal(size=(h, w, 3)) * 0.2 + np.array([0.0, 0.0, 1.0])
    depth = np.stack([rng.uniform(1.0, 1.5, (h, w)), np.ones((h, w)), rng.integers(0, ids, (h, w)).astype(np.float64)], axis=-1)
    return rgb, var, albedo, normal, depth


def same(a, b):
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


SETTINGS = [
    dict(passes=3, flags=3, sigma_color=4.0, sigma_normal=0.5, sigma_depth=0.0),       # the defaults, one pass fewer
    dict(passes=2, flags=0, sigma_color=0.0, sigma_normal=0.0, sigma_depth=0.3),
    dict(passes=5, flags=2, sigma_color=2.0, sigma_normal=1.0, sigma_depth=0.5),
    dict(passes=1, flags=1, sigma_color=0.0, sigma_normal=0.0, sigma_depth=0.0),
]


@pytest.mark.parametrize("w,h", [(9, 7), (5, 3), (1, 1)])
@pytest.mark.parametrize("k", range(len(SETTINGS)))
def test_restatement_equals_the_definition_pixel_by_pixel(w, h, k):
    """Also the frames narrower than 2 s in both directions: 5 x 3 and 1 x 1 at 5 passes (setting 2), where every tap but the
    centre's row and column, or every tap but the centre, is outside the image."""
    s = SETTINGS[k]
    case = random_case(10 * k + w, w, h)
    got = denoise_ref(*case, **s)
    want = scalar_denoise(*[a.tolist() for a in case], s["passes"], s["flags"], s["sigma_color"], s["sigma_normal"], s["sigma_depth"])
    assert same(got[0], want[0]) and same(got[1], want[1])
    nulls = denoise_ref(case[0], None, None, None, None, passes=s["passes"], flags=0, sigma_color=0.0, sigma_normal=0.0, sigma_depth=0.0)
    want = scalar_denoise(case[0].tolist(), None, None, None, None, s["passes"], 0, 0.0, 0.0, 0.0)
    assert same(nulls[0], want[0]) and same(nulls[1], np.zeros((h, w)))
    if (w, h) == (1, 1):   # one tap: W = 9/64, C = 9/64 c, and the quotient of the two products is c again only up to rounding
        assert np.allclose(got[0], case[0], rtol=4e-16, atol=0.0)


def halves(w=12, h=8):
    rgb = np.ones((h, w, 3))
    rgb[:, w // 2:] = 2.0
    depth = np.zeros((h, w, 3))
    depth[..., 1] = 1.0
    depth[:, :w // 2, 2], depth[:, w // 2:, 2] = 1.0, 2.0
    return rgb, depth


def test_exact_inputs_two_half_frames():
    """With x = 0 every weight is a multiple of 1/256: W, C = W c and C / W are exact."""
    rgb, depth = halves()
    for passes in (1, 4):
        out, _ = denoise_ref(rgb, None, None, None, depth, passes=passes, flags=MATCH_ID, sigma_color=0.0, sigma_normal=0.0, sigma_depth=0.0)
        assert np.array_equal(out, rgb)                      # the id keeps the halves apart
        out, _ = denoise_ref(rgb, None, None, None, depth, passes=passes, flags=0, sigma_color=0.0, sigma_normal=0.0, sigma_depth=0.0)
        assert not np.array_equal(out, rgb)                  # without it and without a term: a blur across the edge
        assert np.array_equal(out[:, :2], rgb[:, :2]) if passes == 1 else True    # (two pixels from the edge: untouched by step 1)
        # the colour term with a zero variance keeps them apart as well: k_p = 1 / (16 * 1e-12), x = 6.25e10 across the edge
        out, v = denoise_ref(rgb, np.zeros(rgb.shape[:2]), None, None, depth, passes=passes, flags=0, sigma_color=4.0, sigma_normal=0.0,
                             sigma_depth=0.0)
        assert np.array_equal(out, rgb) and np.array_equal(v, np.zeros(rgb.shape[:2]))


def test_variance_of_a_constant_frame_is_sum_w2_over_sum_w_squared():
    """Pass 0 on a constant frame with unit variance and every term off: v' = sum w^2 / (sum w)^2 over the taps inside the image,
    exactly (w is a multiple of 1/256, w^2 of 1/65536, the sums and W W are exact, the division rounds once)."""
    w, h = 9, 8
    out, v = denoise_ref(np.full((h, w, 3), 0.5), np.ones((h, w)), None, None, None, passes=1, flags=0, sigma_color=0.0, sigma_normal=0.0,
                         sigma_depth=0.0)
    assert np.array_equal(out, np.full((h, w, 3), 0.5))

    def expect(x, y):
        ws = [Fraction(H[dy]) * Fraction(H[dx]) for dy in range(-2, 3) for dx in range(-2, 3) if 0 <= x + dx < w and 0 <= y + dy < h]
        return float(sum(q * q for q in ws) / sum(ws) ** 2)

    for (x, y) in [(4, 4), (2, 2), (0, 3), (1, 3), (4, 0), (4, 7), (8, 4), (0, 0), (8, 7), (1, 1), (7, 0)]:   # interior, edges, corners
        assert v[y, x] == expect(x, y), (x, y)
    assert v[4, 4] == (Fraction(70, 256) ** 2).__float__() and v[0, 0] < 1.0 and v[0, 0] > v[4, 4]
    # with the colour term on and that variance: vhat = 1 everywhere (sum g v / sum g with v = 1, exact), x = 0, the same result
    out2, v2 = denoise_ref(np.full((h, w, 3), 0.5), np.ones((h, w)), None, None, None, passes=1, flags=0, sigma_color=4.0, sigma_normal=0.0,
                           sigma_depth=0.0)
    assert np.array_equal(v2, v) and np.array_equal(out2, out)


@pytest.mark.parametrize("what", ["colour", "variance", "depth", "id"])
@pytest.mark.parametrize("pos", [(5, 4), (0, 0)])
def test_a_nan_pixel_keeps_its_value(what, pos):
    """A NaN colour (colour term on), variance (colour term on), depth (depth term on) or id (MATCH_ID) fails every test of the
    pixel's own taps: W = 0 and the pixel keeps c and v.  A NaN colour, depth or id fails the neighbours' tests of that tap as well:
    nothing of the pixel reaches another one.  A NaN variance does not: its pixel's colour passes the neighbours' tests and its NaN
    enters their V -- the definition as it stands, which the restatement and the kernels share."""
    x, y = pos
    rgb, var, albedo, normal, depth = random_case(3, 11, 9)
    rgb, depth = rgb * 0.01 + 0.5, depth.copy()              # close colours: taps are accepted
    depth[..., 2] = 1.0
    s = dict(passes=3, flags=MATCH_ID, sigma_color=4.0, sigma_normal=0.0, sigma_depth=5.0)
    if what == "colour":
        rgb[y, x, 1] = NAN
    elif what == "variance":
        var[y, x] = NAN
    elif what == "depth":
        depth[y, x, 0] = NAN
    else:
        depth[y, x, 2] = NAN
    out, v = denoise_ref(rgb, var, None, None, depth, **s)
    assert same(out[y, x], rgb[y, x]) and same(v[y, x], var[y, x])
    others = np.ones((9, 11), dtype=bool)
    others[y, x] = False
    if what == "variance":
        assert np.isfinite(out[others]).all() and np.isnan(v[others]).any()
        return
    assert np.isfinite(out[others]).all() and np.isfinite(v[others]).all()
    # what the pixel holds besides the NaN does not matter to anyone else
    rgb2 = rgb.copy()
    rgb2[y, x, 0], rgb2[y, x, 2] = 7.0, 0.125
    out2, v2 = denoise_ref(rgb2, var, None, None, depth, **s)
    assert same(out2[others], out[others]) and same(v2[others], v[others])
    # an infinite colour: inf - inf = NaN at the pixel's own tap, inf at the others'
    rgb3 = rgb.copy()
    rgb3[y, x, 0] = math.inf
    out3, v3 = denoise_ref(rgb3, var, None, None, np.where(np.isnan(depth), 1.0, depth), **s)
    assert same(out3[y, x], rgb3[y, x]) and np.isfinite(out3[others]).all()


# ---- the C ABI's checks
def _denoise(lib, fn, d, prm, planes):
    p = [a.ctypes.data_as(C.c_void_p) if a is not None else None for a in planes]
    args = [d, C.byref(prm) if prm is not None else None] + p
    return fn(*args, None) if fn is lib.rpt_denoise_device else fn(*args)


@pytest.mark.parametrize("device", [False, True])
def test_argument_checks_precede_every_device_call(device):
    """No denoiser exists and no GPU is needed: every refusal below is RPT_ERR_INVALID (-1), the parameters' and the planes' before the
    handle's."""
    lib = _lib.load()
    fn = lib.rpt_denoise_device if device else lib.rpt_denoise
    f = [np.zeros((4, 4, 3)) for _ in range(4)]
    rgb, albedo, normal, depth = f
    var, out, out_var = np.zeros((4, 4)), np.zeros((4, 4, 3)), np.zeros((4, 4))
    P = _lib.DenoiseParams
    full = [rgb, var, albedo, normal, depth, out, out_var]

    def err(prm, planes, text):
        assert _denoise(lib, fn, None, prm, planes) == -1
        assert text in lib.rpt_last_error(), lib.rpt_last_error()

    err(None, full, b"parameters")
    err(P(0, 3, 4.0, 0.5, 0.0), full, b"passes")
    err(P(9, 3, 4.0, 0.5, 0.0), full, b"passes")
    err(P(4, 4, 4.0, 0.5, 0.0), full, b"flag")
    err(P(4, 3, -1.0, 0.5, 0.0), full, b"sigma")
    err(P(4, 3, 4.0, NAN, 0.0), full, b"sigma")
    err(P(4, 3, 4.0, 0.5, math.inf), full, b"sigma")
    err(P(4, 3, 4.0, 0.5, 0.0), [None] + full[1:], b"null frame")
    err(P(4, 3, 4.0, 0.5, 0.0), full[:5] + [None, out_var], b"null frame")
    err(P(4, 0, 4.0, 0.0, 0.0), [rgb, None, None, None, None, out, None], b"sigma_color")
    err(P(4, 0, 0.0, 0.5, 0.0), [rgb, None, None, None, None, out, None], b"sigma_normal")
    err(P(4, 0, 0.0, 0.0, 0.5), [rgb, None, None, None, None, out, None], b"sigma_depth")
    err(P(4, 1, 0.0, 0.0, 0.0), [rgb, None, None, normal, depth, out, None], b"DEMODULATE")
    err(P(4, 2, 0.0, 0.0, 0.0), [rgb, None, albedo, normal, None, out, None], b"MATCH_ID")
    for k in (0, 2, 3, 4):
        err(P(4, 3, 4.0, 0.5, 0.5), full[:5] + [full[k], out_var], b"output")
    err(P(4, 3, 4.0, 0.5, 0.5), full[:5] + [out, var], b"output")
    err(P(4, 3, 4.0, 0.5, 0.5), full[:5] + [out, out], b"differ")
    # everything in order, nothing optional given: the next refusal is the handle
    err(P(1, 0, 0.0, 0.0, 0.0), [rgb, None, None, None, None, out, None], b"null denoiser")
    err(P(4, 3, 4.0, 0.5, 0.5), full, b"null denoiser")


def test_other_entry_points_check_their_arguments_without_a_gpu():
    lib = _lib.load()
    assert not lib.rpt_denoiser_create(0, 0, 8) and b"size" in lib.rpt_last_error()
    assert not lib.rpt_denoiser_create(0, 8, 0) and b"size" in lib.rpt_last_error()
    assert not lib.rpt_denoiser_create(0, 1 << 16, 1 << 15) and b"size" in lib.rpt_last_error()
    assert not lib.rpt_denoiser_create(-1, 8, 8) and b"device" in lib.rpt_last_error()
    assert not lib.rpt_denoiser_create(1 << 20, 8, 8) and b"device" in lib.rpt_last_error()
    lib.rpt_denoiser_destroy(None)
    buf = np.zeros(8)
    p = buf.ctypes.data_as(C.c_void_p)
    assert lib.rpt_buffer_mean_device(None, p, p, None) == -1 and b"null" in lib.rpt_last_error()
    prm = _lib.DenoiseParams(4, 3, 4.0, 0.5, 0.0)
    assert lib.rpt_buffer_denoised_image(None, None, C.byref(prm), p, p, p, p) == -1 and b"null" in lib.rpt_last_error()
    # the process option rpt_denoiser_create reads
    try:
        for v in (0, 1, 2, -1):
            assert lib.rpt_set_option(b"denoise_stage", v) == 0
        for v in (3, 4, -2, 16):
            assert lib.rpt_set_option(b"denoise_stage", v) == -1 and b"denoise_stage" in lib.rpt_last_error()
    finally:
        assert lib.rpt_set_option(b"denoise_stage", -1) == 0


def test_python_wrappers_refuse_before_the_device():
    p = DenoiseParams()
    assert (p.passes, p.flags, p.sigma_color, p.sigma_normal, p.sigma_depth) == (4, 3, 4.0, 0.5, 0.0)
    assert DenoiseParams(demodulate=False).flags == 2 and DenoiseParams(match_id=False).flags == 1
    d = p.desc()
    assert (d.passes, d.flags, d.sigma_color, d.sigma_normal, d.sigma_depth) == (4, 3, 4.0, 0.5, 0.0)
    with pytest.raises(ValueError):
        Denoiser(0, 8)
    with pytest.raises(ValueError):
        Denoiser(8, -1)
    r = Renderer(Scene(), Camera()).width(8).height(8).num_samples(8)
    with pytest.raises(ValueError, match="2 batches"):
        r.render_denoised(1)
    with pytest.raises(ValueError, match="num_samples"):
        r.render_denoised(9)
    with pytest.raises(ValueError, match="sharded"):
        Renderer(Scene(), Camera()).width(8).height(8).num_samples(8).shard(0, 2).render_denoised(4)
