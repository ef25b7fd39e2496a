"""The guided upsampling (rpt_upsample*), the parts that need no GPU: the numpy restatement of the definition (tests/upsample_ref.py)
against a pixel-by-pixel, tap-by-tap transcription of include/rpt_hip.h and on inputs where the definition is exact, NaN and inf,
the argument checks of the new entry points that precede every device call (through the library, and through
tests/host/upsample_harness.cpp over the HIP stubs: as a program of its own under AddressSanitizer + UBSan and plain; nothing loaded
into Python runs under a sanitizer), the Python wrappers' refusals, and the two quality conditions on the oracle's renders.

The quality scene is scenes.lampshade(), not scenes.spheres(): spheres() renders black under the reference's semantics (its only
light is a Light::Object that is no object), so every frame of it is zero and no reconstruction can be strictly closer to the
converged frame than replication is (0 against 0).  tools/upsample_quality.py on lampshade, s = 2, the defaults: 0.28 % of the pixels
take the fallback, RMS 24.31 levels against 31.04 for replication."""
import ctypes as C
import functools
import math
import os
import subprocess

import numpy as np
import pytest

from rpt_amd import Camera, DenoiseParams, Renderer, Scene, UpsampleParams, _lib, color_bytes, image_bytes_device, scenes, upsample
from tests.upsample_ref import DEMODULATE, MATCH_ID, mean_and_variance, oracle_planes, replicate, upsample_ref

NAN, INF = float("nan"), float("inf")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def scalar_upsample(lo_rgb, lo_var, lo_albedo, lo_normal, lo_depth, hi_albedo, hi_normal, hi_depth, s, r, flags, sn, sd):
    """The definition, one pixel, one tap and one Python float operation at a time -> (out, var, fallback) as nested lists."""
    h, w = len(lo_rgb), len(lo_rgb[0])
    H, W = s * h, s * w

    def den(albedo, y, x, k):
        return albedo[y][x][k] if flags & DEMODULATE and albedo[y][x][k] > 0.0 else 1.0

    def c_q(y, x):
        return [lo_rgb[y][x][k] / den(lo_albedo, y, x, k) for k in range(3)]

    def v_q(y, x):
        return lo_var[y][x] if lo_var is not None else 0.0

    out = [[None] * W for _ in range(H)]
    var = [[None] * W for _ in range(H)]
    fell = [[False] * W for _ in range(H)]
    for Y in range(H):
        for X in range(W):
            tx, ty = 2 * X + 1 - s, 2 * Y + 1 - s
            i0, j0 = math.floor(tx / (2 * s)), math.floor(ty / (2 * s))
            fx, fy = float(tx - 2 * s * i0) / float(2 * s), float(ty - 2 * s * j0) / float(2 * s)
            Ws, Cs, Vs = 0.0, [0.0, 0.0, 0.0], 0.0
            for dy in range(1 - r, r + 1):
                for dx in range(1 - r, r + 1):
                    qx, qy = i0 + dx, j0 + dy
                    if not (0 <= qx < w and 0 <= qy < h):
                        continue
                    g_dx = 1.0 - abs(fx - float(dx)) / float(r)
                    g_dy = 1.0 - abs(fy - float(dy)) / float(r)
                    if not (g_dx > 0.0 and g_dy > 0.0):
                        continue
                    x = 0.0
                    if sn > 0.0:
                        e = [(lo_normal[qy][qx][k] - hi_normal[Y][X][k]) * (1.0 / sn) for k in range(3)]
                        x = x + ((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2])
                    if sd > 0.0:
                        e = (lo_depth[qy][qx][0] - hi_depth[Y][X][0]) * (1.0 / (sd * float(s)))
                        x = x + e * e
                    if not x < 4.0 or (flags & MATCH_ID and not lo_depth[qy][qx][2] == hi_depth[Y][X][2]):
                        continue
                    t = 1.0 - x * 0.25
                    t2 = t * t
                    wgt = (t2 * t2) * (g_dy * g_dx)
                    c = c_q(qy, qx)
                    Ws = Ws + wgt
                    Cs = [Cs[k] + wgt * c[k] for k in range(3)]
                    Vs = Vs + (wgt * wgt) * v_q(qy, qx)
            with np.errstate(all="ignore"):
                if Ws > 0.0:
                    c, v = [float(np.float64(Cs[k]) / np.float64(Ws)) for k in range(3)], float(np.float64(Vs) / np.float64(Ws * Ws))
                else:
                    c, v, fell[Y][X] = c_q(Y // s, X // s), v_q(Y // s, X // s), True
            out[Y][X] = [c[k] * den(hi_albedo, Y, X, k) for k in range(3)]
            var[Y][X] = v
    return np.array(out, dtype=np.float64).reshape(H, W, 3), np.array(var, dtype=np.float64).reshape(H, W), np.array(fell).reshape(H, W)


def random_case(seed, w, h, s, ids=3):
    """lo_rgb, lo_var, lo_albedo, lo_normal, lo_depth, hi_albedo, hi_normal, hi_depth."""
    rng = np.random.default_rng(seed)

    def planes(hh, ww):
        albedo = rng.choice([0.0, 0.25, 0.5, 0.9], (hh, ww, 3))
        normal = rng.normal(size=(hh, ww, 3)) * 0.3 + np.array([0.0, 0.0, 1.0])
        depth = np.stack([rng.uniform(1.0, 1.5, (hh, ww)), np.ones((hh, ww)), rng.integers(0, ids, (hh, ww)).astype(np.float64)], axis=-1)
        return albedo, normal, depth

    lo = planes(h, w)
    hi = planes(s * h, s * w)
    return (rng.uniform(0.0, 2.0, (h, w, 3)), rng.uniform(0.0, 0.05, (h, w)), *lo, *hi)


def same(a, b):
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


SETTINGS = {
    "nothing": dict(flags=0, sigma_normal=0.0, sigma_depth=0.0),
    "normal alone": dict(flags=0, sigma_normal=0.7, sigma_depth=0.0),
    "depth alone": dict(flags=0, sigma_normal=0.0, sigma_depth=0.4),
    "demodulation alone": dict(flags=DEMODULATE, sigma_normal=0.0, sigma_depth=0.0),
    "id alone": dict(flags=MATCH_ID, sigma_normal=0.0, sigma_depth=0.0),
    "all": dict(flags=DEMODULATE | MATCH_ID, sigma_normal=0.7, sigma_depth=0.4),
}


@pytest.mark.parametrize("w,h", [(1, 1), (5, 3), (9, 7)])
@pytest.mark.parametrize("s", [2, 3, 4])
@pytest.mark.parametrize("r", [1, 2])
def test_restatement_equals_the_definition_tap_by_tap(w, h, s, r):
    for k, (name, kw) in enumerate(SETTINGS.items()):
        case = random_case(100 * k + 10 * s + r + w, w, h, s)
        got = upsample_ref(*case, scale=s, radius=r, return_fallback=True, **kw)
        want = scalar_upsample(*[a.tolist() for a in case], s, r, kw["flags"], kw["sigma_normal"], kw["sigma_depth"])
        assert same(got[0], want[0]) and same(got[1], want[1]) and same(got[2], want[2]), (name, w, h, s, r)
        if kw["flags"] == 0 and kw["sigma_normal"] == 0.0 and kw["sigma_depth"] == 0.0:
            nulls = upsample_ref(case[0], None, None, None, None, None, None, None, scale=s, radius=r, **kw)
            assert same(nulls[0], want[0]) and same(nulls[1], np.zeros((s * h, s * w)))
    if "id alone" in SETTINGS and (w, h) == (9, 7):
        assert want[2].sum() < want[2].size                      # (not every pixel falls back on random ids)


def test_exact_interior_weights_at_scale_2():
    """s = 2, r = 1, every term off: fx, fy are 1/4 or 3/4, the weights products of (1/4, 3/4) with Wsum = 1 exactly, so small-integer
    colours give exact outputs: the bilinear interpolation at pixel centres."""
    rng = np.random.default_rng(5)
    lo = rng.integers(0, 64, (4, 6, 3)).astype(np.float64)
    var = rng.integers(0, 64, (4, 6)).astype(np.float64)
    out, v = upsample_ref(lo, var, None, None, None, None, None, None, scale=2, radius=1, flags=0)
    for (X, Y) in [(1, 1), (2, 1), (5, 4), (6, 5), (10, 6), (3, 2)]:   # interior: i0 = (X - 1) // 2 >= 0 and i0 + 1 < w
        i0, j0 = (X - 1) // 2, (Y - 1) // 2
        gx = (0.75, 0.25) if (X - 1) % 2 == 0 else (0.25, 0.75)
        gy = (0.75, 0.25) if (Y - 1) % 2 == 0 else (0.25, 0.75)
        want = sum(gy[b] * gx[a] * lo[j0 + b, i0 + a] for b in range(2) for a in range(2))
        want_v = sum((gy[b] * gx[a]) ** 2 * var[j0 + b, i0 + a] for b in range(2) for a in range(2))
        assert np.array_equal(out[Y, X], want) and v[Y, X] == want_v, (X, Y)


def test_border_pixels_skip_exactly_the_taps_outside():
    """The first row and column have i0 = -1 (j0 = -1): only the taps at dx = 1 (dy = 1) are inside.  With one tap per axis left the
    quotient of the two products is the tap's colour up to rounding; with a constant row it is exact."""
    lo = np.zeros((3, 4, 3))
    lo[..., 0] = np.arange(4)[None, :] * 8.0                     # red = 8 x: constant down a column
    lo[..., 1] = np.arange(3)[:, None] * 8.0                     # green = 8 y
    out, _ = upsample_ref(lo, None, None, None, None, None, None, None, scale=2, radius=1, flags=0)
    # corner: one tap, weight 3/4 * 3/4: (9/16 c) / (9/16)
    assert np.array_equal(out[0, 0], lo[0, 0]) and np.array_equal(out[5, 7], lo[2, 3])
    # top edge, X = 3: i0 = 1, fx = 1/4: red = 3/4 * 8 + 1/4 * 16 = 10, only the row below the border counts: green = 0
    assert out[0, 3, 0] == 10.0 and out[0, 3, 1] == 0.0
    # left edge, Y = 2: j0 = 0, fy = 3/4: green = 1/4 * 0 + 3/4 * 8 = 6, red = the first column's 0
    assert out[2, 0, 1] == 6.0 and out[2, 0, 0] == 0.0
    # the same through the transcription, which skips by its own bounds test
    want = scalar_upsample(lo.tolist(), None, None, None, None, None, None, None, 2, 1, 0, 0.0, 0.0)
    assert same(out, want[0]) and not want[2].any()


@pytest.mark.parametrize("s", [2, 3, 4])
@pytest.mark.parametrize("r", [1, 2])
def test_one_low_resolution_pixel(s, r):
    """A 1 x 1 low-resolution frame: every full-resolution pixel has the one tap (or, where its id differs, the fallback to the same
    pixel): its value times den_p / den_q, up to the rounding of (w c) / w."""
    rng = np.random.default_rng(s + r)
    lo = np.array([[[0.5, 1.5, 0.25]]])
    lo_albedo = np.array([[[0.5, 0.25, 0.0]]])
    hi_albedo = rng.choice([0.0, 0.5, 0.8], (s, s, 3))
    lo_depth = np.array([[[1.0, 1.0, 2.0]]])
    hi_depth = np.ones((s, s, 3))
    hi_depth[..., 2] = rng.choice([2.0, 3.0], (s, s))
    hi_depth[0, 0, 2], hi_depth[-1, -1, 2] = 2.0, 3.0
    out, v, fb = upsample_ref(lo, np.array([[0.125]]), lo_albedo, None, lo_depth, hi_albedo, None, hi_depth, scale=s, radius=r, return_fallback=True)
    den_p = np.where(hi_albedo > 0.0, hi_albedo, 1.0)
    want = (lo[0, 0] / np.array([0.5, 0.25, 1.0])) * den_p
    assert np.allclose(out, want, rtol=4e-16, atol=0.0)
    assert np.array_equal(fb, hi_depth[..., 2] != 2.0) and fb[-1, -1] and not fb[0, 0]      # an id that matches no tap: the fallback
    assert np.array_equal(out[fb], want[fb])                                                  # which is exact
    assert np.allclose(v, 0.125, rtol=4e-16, atol=0.0) and np.array_equal(v[fb], np.full(int(fb.sum()), 0.125))


@pytest.mark.parametrize("what", ["colour", "variance", "normal", "depth", "lo id", "hi id"])
def test_nan_and_inf_follow_the_rules(what):
    """A NaN normal, depth or id fails the tap's tests (the tap is skipped; a full-resolution pixel whose own id or depth is NaN loses
    every tap and takes the fallback).  A NaN or inf colour or variance of an accepted tap enters C or V of the pixels that read the
    tap and of no other."""
    s, r = 2, 1
    case = [a.copy() for a in random_case(9, 6, 5, s, ids=1)]
    lo_rgb, lo_var, lo_albedo, lo_normal, lo_depth, hi_albedo, hi_normal, hi_depth = case
    lo_normal[:], hi_normal[:] = [0.0, 0.0, 1.0], [0.0, 0.0, 1.0]
    kw = dict(scale=s, radius=r, flags=MATCH_ID, sigma_normal=0.5, sigma_depth=5.0)
    clean, clean_v, fb0 = upsample_ref(*case, return_fallback=True, **kw)
    assert not fb0.any() and np.isfinite(clean).all()
    qx, qy = 2, 2
    reads = np.zeros((10, 12), dtype=bool)                       # the full-resolution pixels with (qx, qy) among their 2 x 2 taps
    reads[2 * qy - 1:2 * qy + 3, 2 * qx - 1:2 * qx + 3] = True
    for bad in (NAN, INF):
        c2 = [a.copy() for a in case]
        if what == "colour":
            c2[0][qy, qx, 1] = bad
        elif what == "variance":
            c2[1][qy, qx] = bad
        elif what == "normal":
            c2[3][qy, qx, 0] = bad
        elif what == "depth":
            c2[4][qy, qx, 0] = bad
        elif what == "lo id":
            c2[4][qy, qx, 2] = bad
        else:
            c2[7][5, 5, 2] = bad
        out, v, fb = upsample_ref(*c2, return_fallback=True, **kw)
        want = scalar_upsample(*[a.tolist() for a in c2], s, r, kw["flags"], kw["sigma_normal"], kw["sigma_depth"])
        assert same(out, want[0]) and same(v, want[1]) and same(fb, want[2])
        if what == "colour":
            assert not np.isfinite(out[reads][:, 1]).any() and np.isfinite(out[reads][:, [0, 2]]).all()
            assert same(out[~reads], clean[~reads]) and same(v, clean_v)
        elif what == "variance":
            assert not np.isfinite(v[reads]).any() and same(v[~reads], clean_v[~reads]) and same(out, clean)
        elif what == "hi id":
            assert fb[5, 5] and fb.sum() == 1                    # no tap matches: the pixel's own footprint (2, 2)
            assert same(out[5, 5], c2[0][2, 2]) and v[5, 5] == c2[1][2, 2]
        else:                                                    # the tap is skipped by all who read it; nobody falls back (other taps remain)
            assert np.isfinite(out).all() and np.isfinite(v).all() and not fb.any()
            assert same(out[~reads], clean[~reads]) and not same(out[reads], clean[reads])


# ---- the C ABI's checks, through the library (no GPU is needed: every refusal precedes every device call)
def _call(lib, device, prm, w, h, planes):
    p = [a.ctypes.data_as(C.c_void_p) if a is not None else None for a in planes]
    ref = C.byref(prm) if prm is not None else None
    return lib.rpt_upsample_device(ref, w, h, *p, None) if device else lib.rpt_upsample(0, ref, w, h, *p)


@pytest.mark.parametrize("device", [False, True])
def test_argument_checks_precede_every_device_call(device):
    lib = _lib.load()
    w, h = 4, 3
    lo = [np.zeros((h, w, 3)) for _ in range(4)]
    hi = [np.zeros((2 * h, 2 * w, 3)) for _ in range(3)]
    var, out, out_var = np.zeros((h, w)), np.zeros((2 * h, 2 * w, 3)), np.zeros((2 * h, 2 * w))
    full = [lo[0], var, lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], out, out_var]
    P = _lib.UpsampleParams

    def err(prm, planes, text, ww=w, hh=h):
        assert _call(lib, device, prm, ww, hh, planes) == -1
        assert text in lib.rpt_last_error(), lib.rpt_last_error()

    err(None, full, b"parameters")
    err(P(1, 1, 3, 0, 0.5, 0.0), full, b"scale")
    err(P(5, 0, 3, 0, 0.5, 0.0), full, b"scale")                 # (the scale before the radius)
    err(P(2, 0, 4, 0, 0.5, 0.0), full, b"radius")                # (the radius before the flags)
    err(P(2, 3, 3, 0, 0.5, 0.0), full, b"radius")
    err(P(2, 1, 4, 0, -1.0, 0.0), full, b"flag")                 # (the flags before the sigmas)
    err(P(2, 1, 3, 0, -1.0, 0.0), full, b"sigma", 0, 0)          # (the sigmas before the size)
    err(P(2, 1, 3, 0, 0.5, NAN), full, b"sigma")
    err(P(2, 1, 3, 0, INF, 0.0), full, b"sigma")
    err(P(2, 1, 3, 0, 0.5, 0.0), [None] * 10, b"empty", 0, h)    # (the size before the frames)
    err(P(2, 1, 3, 0, 0.5, 0.0), [None] * 10, b"empty", w, 0)
    err(P(2, 1, 3, 0, 0.5, 0.0), [None] * 10, b"too large", 1 << 31, 1)
    err(P(4, 1, 3, 0, 0.5, 0.0), [None] * 10, b"too large", 1, 1 << 30)
    err(P(2, 1, 3, 0, 0.5, 0.0), [None] * 10, b"too large", 1 << 15, 1 << 14)
    err(P(2, 1, 3, 0, 0.5, 0.5), [None] + full[1:], b"null frame")
    err(P(2, 1, 3, 0, 0.5, 0.5), full[:8] + [None, out_var], b"null frame")
    bare = [lo[0], None, None, None, None, None, None, None, out, None]

    def given(*idx):
        return [full[k] if k in idx else bare[k] for k in range(10)]

    err(P(2, 1, 3, 0, 0.5, 0.5), bare, b"sigma_normal > 0 needs the low")
    err(P(2, 1, 3, 0, 0.5, 0.5), given(3), b"sigma_normal > 0 needs the full")
    err(P(2, 1, 3, 0, 0.5, 0.5), given(3, 6), b"sigma_depth > 0 needs the low")
    err(P(2, 1, 3, 0, 0.5, 0.5), given(3, 6, 4), b"sigma_depth > 0 needs the full")
    err(P(2, 1, 3, 0, 0.5, 0.5), given(3, 6, 4, 7), b"DEMODULATE needs the low")
    err(P(2, 1, 3, 0, 0.5, 0.5), given(3, 6, 4, 7, 2), b"DEMODULATE needs the full")
    err(P(2, 1, 2, 0, 0.0, 0.0), given(7), b"MATCH_ID needs the low")
    err(P(2, 1, 2, 0, 0.0, 0.0), given(4), b"MATCH_ID needs the full")
    for k in range(8):
        err(P(2, 1, 3, 0, 0.5, 0.5), full[:8] + [full[k], out_var], b"output must not")
        err(P(2, 1, 3, 0, 0.5, 0.5), full[:8] + [out, full[k]], b"output must not")
    err(P(2, 1, 3, 0, 0.5, 0.5), full[:8] + [out, out], b"differ")


def test_other_entry_points_check_their_arguments_without_a_gpu():
    lib = _lib.load()
    buf = np.zeros(48)
    p = buf.ctypes.data_as(C.c_void_p)
    assert lib.rpt_image_bytes_device(None, 4, 4, p, None) == -1 and b"null" in lib.rpt_last_error()
    assert lib.rpt_image_bytes_device(p, 4, 4, None, None) == -1 and b"null" in lib.rpt_last_error()
    assert lib.rpt_image_bytes_device(p, 0, 4, p, None) == -1 and b"size" in lib.rpt_last_error()
    assert lib.rpt_image_bytes_device(p, 1 << 16, 1 << 15, p, None) == -1 and b"size" in lib.rpt_last_error()
    prm = _lib.UpsampleParams(2, 1, 0, 0, 0.0, 0.0)
    assert lib.rpt_buffer_upsampled_image(None, None, None, C.byref(prm), p, p, p, p, p, p, p) == -1 and b"null" in lib.rpt_last_error()


def test_python_wrappers_refuse_before_the_device():
    p = UpsampleParams()
    assert (p.scale, p.radius, p.flags, p.sigma_normal, p.sigma_depth) == (2, 1, 3, 1.0, 0.0)
    assert UpsampleParams(demodulate=False).flags == 2 and UpsampleParams(match_id=False).flags == 1
    d = UpsampleParams(scale=3, radius=2, sigma_depth=0.25).desc()
    assert (d.scale, d.radius, d.flags, d.sigma_normal, d.sigma_depth) == (3, 2, 3, 1.0, 0.25)
    with pytest.raises(ValueError, match="lo_rgb"):
        upsample(np.zeros((4, 4)))
    with pytest.raises(ValueError, match="scale"):
        upsample(np.zeros((4, 4, 3)), params=UpsampleParams(scale=5))
    with pytest.raises(ValueError, match="hi_normal"):
        upsample(np.zeros((4, 4, 3)), lo_normal=np.zeros((4, 4, 3)), hi_normal=np.zeros((4, 4, 3)))
    with pytest.raises(ValueError, match="empty"):
        image_bytes_device(1, 0, 4)
    r = Renderer(Scene(), Camera()).width(8).height(6).num_samples(8)
    with pytest.raises(ValueError, match="multiples"):
        r.render_upsampled(UpsampleParams(scale=4))
    with pytest.raises(ValueError, match="2 batches"):
        r.render_upsampled(batches=1)
    with pytest.raises(ValueError, match="num_samples"):
        r.render_upsampled(batches=9)
    with pytest.raises(ValueError, match="guide_samples"):
        r.render_upsampled(guide_samples=0)
    with pytest.raises(ValueError, match="sharded"):
        Renderer(Scene(), Camera()).width(8).height(8).num_samples(8).shard(0, 2).render_upsampled()
    from rpt_amd import AdaptiveParams
    with pytest.raises(ValueError, match="adaptive"):
        r.render_sequence([Camera()], upsample=UpsampleParams(), adaptive=AdaptiveParams())
    with pytest.raises(ValueError, match="multiples"):
        r.render_sequence([Camera()], upsample=UpsampleParams(scale=4))
    with pytest.raises(ValueError, match="UpsampleParams"):
        r.render_sequence([Camera()], upsample=DenoiseParams())


# ---- the host half over the HIP stubs, as a program of its own
SRC = os.path.join(ROOT, "tests", "host", "upsample_harness.cpp")
COMMON = ["-std=c++17", "-w", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + os.path.join(ROOT, "include")]


def _build_and_run(tmp_path, name, flags):
    exe = str(tmp_path / name)
    subprocess.check_call(["g++"] + flags + COMMON + [SRC, "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    p = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    print(p.stdout[-6000:])
    assert "FAILED" not in p.stdout, "\n".join(l for l in p.stdout.splitlines() if "FAILED" in l)
    assert p.returncode == 0, p.stderr[-2000:]
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr and "LeakSanitizer" not in p.stderr, p.stderr[-2000:]
    return p.stdout


def test_host_half_under_sanitizers_and_plain(tmp_path):
    a = _build_and_run(tmp_path, "upsample_asan", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer"])
    b = _build_and_run(tmp_path, "upsample_plain", ["-O1"])
    assert a == b and "failures=0" in a


# ---- the quality conditions on the oracle's renders
@functools.lru_cache(maxsize=None)
def oracle_case(name="lampshade", w=64, h=48, s=2):
    from oracle import pyoracle
    scene, cam, cfg = getattr(scenes, name)()
    osc = pyoracle.OracleScene(scene)
    batches = [osc.render(cam, w, h, 4, cfg["max_bounces"], seed=3, sample_offset=4 * k, robust=1) for k in range(4)]
    mean, var = mean_and_variance(batches)
    lo = oracle_planes(osc, scene, cam, w, h, 16, 3)
    hi = oracle_planes(osc, scene, cam, s * w, s * h, 1, 3)
    converged = osc.render(cam, s * w, s * h, 512, cfg["max_bounces"], seed=1234, robust=1).reshape(s * h, s * w, 3)
    return mean.reshape(h, w, 3), var.reshape(h, w), lo, hi, converged


def test_the_restatement_reconstructs_rather_than_falls_back():
    """s = 2 with the defaults on lampshade 64 x 48 -> 128 x 96 (the docstring above says why not spheres): at most 5 % of the pixels
    take the fallback, and the frame is closer to the oracle's 512-spp frame than s x s replication of the same low-resolution
    frame is."""
    mean, var, lo, hi, converged = oracle_case()
    p = UpsampleParams()
    out, _, fb = upsample_ref(mean, var, *lo, *hi, scale=p.scale, radius=p.radius, flags=p.flags, sigma_normal=p.sigma_normal,
                              sigma_depth=p.sigma_depth, return_fallback=True)
    want = color_bytes(converged).astype(np.float64)
    rms = lambda a: float(np.sqrt(np.mean((color_bytes(a).astype(np.float64) - want) ** 2)))  # noqa: E731
    print(f"lampshade 64 x 48 -> 128 x 96: fallback {100.0 * fb.mean():.2f} %, RMS {rms(out):.2f} levels, replication {rms(replicate(mean, 2)):.2f}")
    assert fb.mean() <= 0.05
    assert rms(out) < rms(replicate(mean, 2))
