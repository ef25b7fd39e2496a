"""Temporal accumulation (rpt_temporal_*), the parts that need no GPU: the numpy restatement of the definition
(tests/temporal_ref.py) against a pixel-by-pixel, tap-by-tap transcription of include/rpt_hip.h and on inputs where the definition is
exact; rpt_temporal_camera_record (a host function); the argument checks of every entry point, which precede every device call; the
Python wrappers' refusals; and the conditions on the analytic scene that keep the bit-for-bit tests of tests/test_gpu_temporal.py from
passing with the reprojection dead.

(RPT_ERR_STATE and the size checks of rpt_temporal_frame_image need an rpt_buffer, which only a device can hold:
tests/test_gpu_temporal.py.)"""
import ctypes as C
import math

import numpy as np
import pytest

from rpt_amd import Camera, DenoiseParams, Renderer, Scene, TemporalAccumulator, TemporalParams, _lib
from rpt_amd.api import camera_desc, temporal_camera_record
from tests.temporal_ref import EYES, FOV, MATCH_ID, TemporalRef, analytic_planes, camera_record, look_at_record, sequence

NAN, INF = float("nan"), float("inf")


def records(n=4):
    return [look_at_record(e, (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), FOV) for e in EYES[:n]]


def same(a, b):
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


# ---- the definition, one pixel, one tap and one Python float operation at a time
def div(a, b):
    try:
        return a / b
    except ZeroDivisionError:
        return NAN if (a == 0.0 or a != a) else math.copysign(INF, a) * math.copysign(1.0, b)


def dot3(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


class ScalarTemporal:
    def __init__(self, w, h):
        self.w, self.h, self.hist, self.rec = w, h, None, None

    def accumulate(self, rec, rgb, var, normal, depth, max_history, flags, depth_tol, normal_tol):
        w, h = self.w, self.h
        rec = [float(t) for t in rec]
        eye, direction, right, up, d = rec[0:3], rec[3:6], rec[6:9], rec[9:12], rec[12]
        dim = float(max(w, h))
        out = [[None] * w for _ in range(h)]
        out_v = [[None] * w for _ in range(h)]
        out_len = [[None] * w for _ in range(h)]
        new = [[None] * w for _ in range(h)]
        for y in range(h):
            for x in range(w):
                c_in = rgb[y][x]
                v_in = var[y][x] if var is not None else 0.0
                xn = (float(2 * x + 1) - float(w)) / dim
                yn = (float(2 * (h - y) - 1) - float(h)) / dim
                v = [(d * direction[k] + xn * right[k]) + yn * up[k] for k in range(3)]
                l = math.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
                cov = depth[y][x][1]
                hit = cov > 0.0
                zc = div(depth[y][x][0], cov)
                ident = depth[y][x][2]
                n = normal[y][x] if normal is not None else [0.0, 0.0, 0.0]
                B, Cs, V, L = 0.0, [0.0, 0.0, 0.0], 0.0, 0.0
                if self.hist is not None and hit:
                    p = self.rec
                    s = div(zc, l)
                    q = [(eye[k] + s * v[k]) - p[k] for k in range(3)]
                    zq = dot3(q, p[3:6])
                    if zq > 0.0:
                        u = div(dot3(q, p[6:9]) * p[12], zq)
                        ww = div(dot3(q, p[9:12]) * p[12], zq)
                        fx = ((u * dim + float(w)) - 1.0) * 0.5
                        fy = ((float(h) - 1.0) - ww * dim) * 0.5
                        if fx > -1.0 and fx < float(w) and fy > -1.0 and fy < float(h):
                            ix, iy = math.floor(fx), math.floor(fy)
                            ax, ay = fx - float(ix), fy - float(iy)
                            qq = dot3(q, q)
                            for j in (0, 1):
                                for i in (0, 1):
                                    tx, ty = ix + i, iy + j
                                    if not (0 <= tx < w and 0 <= ty < h):
                                        continue
                                    b = (ax if i else 1.0 - ax) * (ay if j else 1.0 - ay)
                                    hc, hv, hlen, hn, hz, hid = self.hist[ty][tx]
                                    if not hlen > 0.0:
                                        continue
                                    if flags & MATCH_ID and not hid == ident:
                                        continue
                                    if depth_tol > 0.0:
                                        r = hz * hz
                                        if not abs(r - qq) <= depth_tol * qq:
                                            continue
                                    if normal_tol > 0.0:
                                        e = [hn[k] - n[k] for k in range(3)]
                                        if not ((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]) <= normal_tol * normal_tol:
                                            continue
                                    B = B + b
                                    Cs = [Cs[k] + b * hc[k] for k in range(3)]
                                    V = V + (b * b) * hv
                                    L = L + b * hlen
                if B > 0.0:
                    hcol = [Cs[k] / B for k in range(3)]
                    hvar = V / (B * B)
                    hl = L / B
                    length = min(hl + 1.0, float(max_history))
                    a = 1.0 / length
                    o = [hcol[k] + (c_in[k] - hcol[k]) * a for k in range(3)]
                    om = 1.0 - a
                    ov = (om * om) * hvar + (a * a) * v_in
                else:
                    o, ov, length = list(c_in), v_in, 1.0
                out[y][x], out_v[y][x], out_len[y][x] = o, ov, length
                finite = hit and all(not (t - t != 0.0) for t in o + [ov])
                new[y][x] = (o, ov, length if finite else 0.0, list(n), zc, ident)
        self.hist, self.rec = new, rec
        return np.array(out).reshape(h, w, 3), np.array(out_v, dtype=np.float64).reshape(h, w), np.array(out_len, dtype=np.float64).reshape(h, w)


SETTINGS = [
    dict(max_history=16, flags=MATCH_ID, depth_tol=0.1, normal_tol=0.5),        # the defaults
    dict(max_history=2, flags=0, depth_tol=0.0, normal_tol=0.0),                # every test off
    dict(max_history=4, flags=MATCH_ID, depth_tol=0.0, normal_tol=0.0),
    dict(max_history=4, flags=0, depth_tol=0.02, normal_tol=0.0),
    dict(max_history=4, flags=0, depth_tol=0.0, normal_tol=0.2),
]


@pytest.mark.parametrize("w,h", [(1, 1), (5, 3), (33, 17)])
@pytest.mark.parametrize("k", range(len(SETTINGS)))
def test_restatement_equals_the_definition_pixel_by_pixel(w, h, k):
    s = SETTINGS[k]
    ref, scalar = TemporalRef(w, h), ScalarTemporal(w, h)
    took = 0
    for f, (rec, rgb, var, normal, depth) in enumerate(sequence(10 * k + w, w, h, records(3))):
        use_var = var if k != 1 else None
        use_normal = normal if s["normal_tol"] > 0.0 else None
        got = ref.accumulate(rec, rgb, use_var, use_normal, depth, **s)
        want = scalar.accumulate(rec, rgb.tolist(), use_var.tolist() if use_var is not None else None,
                                 use_normal.tolist() if use_normal is not None else None, depth.tolist(), **s)
        for a, b, name in zip(got, want, ("colour", "variance", "len")):
            assert same(a, b), (f, name)
        took += int(ref.last["took"].sum())
    if (w, h) == (33, 17):
        assert took > w * h                                             # most pixels of frames 1 and 2 reuse history


# ---- inputs on which the definition is exact
def flat_case(w=12, h=8, seed=5):
    rng = np.random.default_rng(seed)
    rec = records(1)[0]
    normal, depth = analytic_planes(rec, w, h)
    return rec, rng.uniform(0.0, 2.0, (h, w, 3)), rng.uniform(0.0, 0.05, (h, w)), normal, depth


def test_first_frame_and_frame_after_reset_pass_through():
    rec, rgb, var, normal, depth = flat_case()
    ref = TemporalRef(12, 8)
    for _ in range(2):
        out, v, length = ref.accumulate(rec, rgb, var, normal, depth)
        assert same(out, rgb) and same(v, var) and np.array_equal(length, np.ones((8, 12))) and ref.frames == 1
        out2, _, length2 = ref.accumulate(rec, rgb * 0.5, var, normal, depth)
        assert not same(out2, rgb * 0.5) and length2.max() == 2.0 and ref.frames == 2
        ref.reset()
        assert ref.frames == 0


def test_max_history_1_passes_through():
    rec, rgb, var, normal, depth = flat_case()
    ref = TemporalRef(12, 8)
    ref.accumulate(rec, rgb, var, normal, depth, max_history=1)
    out, v, length = ref.accumulate(rec, rgb * 0.25, var * 2.0, normal, depth, max_history=1)
    # len = 1, a = 1: hc + (rgb - hc) 1 is rgb only up to the rounding of the difference; the variance is (0 0) hv + (1 1) v_in
    assert ref.last["took"].all() and np.array_equal(length, np.ones((8, 12)))
    assert np.allclose(out, rgb * 0.25, rtol=0.0, atol=2.0 ** -51) and same(v, var * 2.0)
    # with the same frame again the difference is 0 and the pass-through is exact
    out, v, _ = ref.accumulate(rec, rgb * 0.25, var * 2.0, normal, depth, max_history=1)
    assert same(out, rgb * 0.25) and same(v, var * 2.0)


@pytest.mark.parametrize("bad", [NAN, INF])
def test_a_nan_or_inf_colour_never_outlives_its_frame(bad):
    rec, rgb, var, normal, depth = flat_case()
    ref = TemporalRef(12, 8)
    ref.accumulate(rec, rgb, var, normal, depth)
    rgb2 = rgb.copy()
    rgb2[3, 5, 1] = bad
    out, v, length = ref.accumulate(rec, rgb2, var, normal, depth)
    assert not np.isfinite(out[3, 5, 1]) and length[3, 5] == 2.0         # it appears in its own output, once
    others = np.ones((8, 12), dtype=bool)
    others[3, 5] = False
    assert np.isfinite(out[others]).all() and np.isfinite(v).all()
    out, v, length = ref.accumulate(rec, rgb, var, normal, depth)
    assert np.isfinite(out).all() and np.isfinite(v).all()
    assert length[3, 5] == 1.0 and same(out[3, 5], rgb[3, 5]) and (length[others] == 3.0).all()
    # the same for a variance that is not finite
    var2 = var.copy()
    var2[2, 2] = bad
    out, v, length = ref.accumulate(rec, rgb, var2, normal, depth)
    assert not np.isfinite(v[2, 2]) and np.isfinite(out).all()
    out, v, length = ref.accumulate(rec, rgb, var, normal, depth)
    assert length[2, 2] == 1.0 and np.isfinite(v).all()


def test_a_miss_pixel_never_lends_history():
    rec, rgb, var, normal, depth = flat_case()
    miss_depth, miss_normal = depth.copy(), normal.copy()
    miss_depth[4, 6], miss_normal[4, 6] = 0.0, 0.0
    ref = TemporalRef(12, 8)
    out, _, length = ref.accumulate(rec, rgb, var, miss_normal, miss_depth)
    assert same(out, rgb) and length[4, 6] == 1.0
    # the pixel is a hit in the next frame: its own record is the only tap with weight (the camera did not move), and holds nothing
    out, v, length = ref.accumulate(rec, rgb * 0.5, var, normal, depth)
    assert length[4, 6] == 1.0 and same(out[4, 6], rgb[4, 6] * 0.5) and not ref.last["took"][4, 6]
    assert (np.delete(length.reshape(-1), 4 * 12 + 6) == 2.0).all()
    # and a miss itself takes none
    out, v, length = ref.accumulate(rec, rgb, var, miss_normal, miss_depth)
    assert length[4, 6] == 1.0 and same(out[4, 6], rgb[4, 6]) and same(v[4, 6], var[4, 6])


# ---- the conditions on the analytic scene
def test_unmoved_camera_reprojects_every_pixel_onto_itself():
    w, h = 64, 48
    rec = records(1)[0]
    normal, depth = analytic_planes(rec, w, h)
    assert depth[..., 1].all() and set(np.unique(depth[..., 2])) == {1.0, 2.0}
    rng = np.random.default_rng(1)
    for max_history in (4, 16):
        ref = TemporalRef(w, h)
        for k in range(1, 8):
            _, _, length = ref.accumulate(rec, rng.uniform(0.0, 1.0, (h, w, 3)), None, normal, depth, max_history=max_history)
            assert np.abs(length - min(k, max_history)).max() <= 1e-9, k
            if k > 1:
                ys, xs = np.mgrid[0:h, 0:w]
                assert np.abs(ref.last["fx"] - xs).max() < 1e-12 and np.abs(ref.last["fy"] - ys).max() < 1e-12


def test_moved_camera_takes_history_at_95_percent_of_the_hit_pixels():
    w, h = 64, 48
    r0, r1 = records(2)
    ref = TemporalRef(w, h)
    rng = np.random.default_rng(2)
    n0, d0 = analytic_planes(r0, w, h)
    n1, d1 = analytic_planes(r1, w, h)
    ref.accumulate(r0, rng.uniform(0.0, 1.0, (h, w, 3)), None, n0, d0)
    _, _, length = ref.accumulate(r1, rng.uniform(0.0, 1.0, (h, w, 3)), None, n1, d1)
    hit, took = ref.last["hit"], ref.last["took"]
    ys, xs = np.mgrid[0:h, 0:w]
    shift = np.hypot(ref.last["fx"] - xs, ref.last["fy"] - ys)[took]
    print(f"moved camera: {int(took.sum())} of {int(hit.sum())} hit pixels take history, shifts up to {shift.max():.2f} px")
    assert hit.sum() == w * h and took.sum() >= 0.95 * hit.sum()
    assert shift.max() > 0.5 and (length[took] == 2.0).all() and (length[~took] == 1.0).all()


# ---- rpt_temporal_camera_record
def ulps(a, b):
    return abs(a - b) / math.ulp(b) if b != 0.0 else (0.0 if a == 0.0 else INF)


def test_camera_record_against_math():
    rng = np.random.default_rng(7)
    for k in range(50):
        eye, center = rng.normal(size=3) * 5.0, rng.normal(size=3)
        cam = Camera.look_at(eye, center, (0.0, 1.0, 0.0), float(rng.uniform(0.05, 3.0)))
        if k % 2:
            cam.direction = cam.direction * 3.0                        # neither normalised nor orthogonal: the record takes them as they are
            cam.up = cam.up + 0.1 * cam.direction
        got = temporal_camera_record(cam)
        want = camera_record(cam.eye, cam.direction, cam.up, cam.fov)
        assert got.shape == (13,)
        assert max(ulps(float(a), float(b)) for a, b in zip(got, want)) <= 4.0
        assert same(got[0:6], want[0:6]) and same(got[9:12], want[9:12])
    # axis-aligned cameras: exact
    for direction, up, right in [((0, 0, -1), (0, 1, 0), (1, 0, 0)), ((1, 0, 0), (0, 0, 1), (0, -1, 0)), ((0, -2, 0), (0, 0, 4), (-1, 0, 0))]:
        cam = Camera((1.5, -2.0, 3.0), direction, up, math.pi / 2)
        got = temporal_camera_record(cam)
        assert got[0:3].tolist() == [1.5, -2.0, 3.0] and got[3:6].tolist() == [float(t) for t in direction]
        assert got[6:9].tolist() == [float(t) for t in right] and got[9:12].tolist() == [float(t) for t in up]
        assert ulps(float(got[12]), 1.0) <= 4.0


def test_camera_record_refusals():
    lib = _lib.load()
    out = (C.c_double * 13)()

    def rc(cam):
        return lib.rpt_temporal_camera_record(C.byref(camera_desc(cam, _lib.CameraDesc)), out)

    assert rc(Camera()) == 0
    assert lib.rpt_temporal_camera_record(None, out) == -1 and b"null" in lib.rpt_last_error()
    assert lib.rpt_temporal_camera_record(C.byref(camera_desc(Camera(), _lib.CameraDesc)), None) == -1
    for field in ("eye", "direction", "up"):
        for bad in (NAN, INF, -INF):
            cam = Camera()
            getattr(cam, field)[1] = bad
            assert rc(cam) == -1 and b"finite" in lib.rpt_last_error(), (field, bad)
    for field in ("fov", "aperture", "focal_distance"):
        for bad in (NAN, INF):
            cam = Camera()
            setattr(cam, field, bad)
            assert rc(cam) == -1 and b"finite" in lib.rpt_last_error(), (field, bad)
    for fov in (0.0, -0.5, math.pi, 4.0):
        assert rc(Camera(fov=fov)) == -1 and b"fov" in lib.rpt_last_error(), fov
    assert rc(Camera(fov=3.14)) == 0 and rc(Camera(fov=1e-3)) == 0
    for direction, up in [((0, 0, -1), (0, 0, 2)), ((0, 0, 0), (0, 1, 0)), ((1, 1, 0), (-2, -2, 0))]:
        assert rc(Camera(direction=direction, up=up)) == -1 and b"cross" in lib.rpt_last_error()
    with pytest.raises(_lib.RptError, match="fov"):
        temporal_camera_record(Camera(fov=0.0))


# ---- the C ABI's checks
def _accumulate(lib, fn, t, prm, cam, planes):
    p = [a.ctypes.data_as(C.c_void_p) if a is not None else None for a in planes]
    args = [t, C.byref(prm) if prm is not None else None, C.byref(cam) if cam is not None else None] + p
    return fn(*args, None) if fn is lib.rpt_temporal_accumulate_device else fn(*args)


@pytest.mark.parametrize("device", [False, True])
def test_argument_checks_precede_every_device_call(device):
    """No accumulator exists and no GPU is needed: every refusal below is RPT_ERR_INVALID (-1), the parameters', the camera's and the
    planes' before the handle's."""
    lib = _lib.load()
    fn = lib.rpt_temporal_accumulate_device if device else lib.rpt_temporal_accumulate
    rgb, normal, depth, out = [np.zeros((4, 4, 3)) for _ in range(4)]
    var, out_var, out_len = [np.zeros((4, 4)) for _ in range(3)]
    P = _lib.TemporalParams
    cam = camera_desc(Camera(), _lib.CameraDesc)
    full = [rgb, var, normal, depth, out, out_var, out_len]
    ok = P(16, 1, 0.1, 0.5)

    def err(prm, camera, planes, text):
        assert _accumulate(lib, fn, None, prm, camera, planes) == -1
        assert text in lib.rpt_last_error(), lib.rpt_last_error()

    err(None, cam, full, b"parameters")
    err(P(0, 1, 0.1, 0.5), cam, full, b"max_history")
    err(P(4097, 1, 0.1, 0.5), cam, full, b"max_history")
    err(P(16, 2, 0.1, 0.5), cam, full, b"flag")
    err(P(16, 1, -0.1, 0.5), cam, full, b"tolerance")
    err(P(16, 1, NAN, 0.5), cam, full, b"tolerance")
    err(P(16, 1, 0.1, INF), cam, full, b"tolerance")
    err(P(16, 1, 0.1, -1.0), cam, full, b"tolerance")
    err(ok, None, full, b"null camera")
    err(ok, camera_desc(Camera(fov=0.0), _lib.CameraDesc), full, b"fov")
    err(ok, camera_desc(Camera(up=(0.0, 0.0, 1.0)), _lib.CameraDesc), full, b"cross")
    err(ok, cam, [None] + full[1:], b"null frame")
    err(ok, cam, full[:4] + [None, out_var, out_len], b"null frame")
    err(ok, cam, [rgb, var, normal, None, out, out_var, out_len], b"depth")
    err(ok, cam, [rgb, var, None, depth, out, out_var, out_len], b"normal_tol > 0")
    err(P(16, 1, 0.1, 0.0), cam, full, b"normal_tol == 0")
    for k in (0, 1, 2, 3):
        for slot in (4, 5, 6):
            planes = list(full)
            planes[slot] = full[k]
            err(ok, cam, planes, b"output")
    err(ok, cam, full[:4] + [out, out, out_len], b"differ")
    err(ok, cam, full[:4] + [out, out_var, out], b"differ")
    err(ok, cam, full[:4] + [out, out_var, out_var], b"differ")
    # everything in order, nothing optional given: the next refusal is the handle
    err(P(1, 0, 0.0, 0.0), cam, [rgb, None, None, depth, out, None, None], b"null accumulator")
    err(ok, cam, full, b"null accumulator")


def test_other_entry_points_check_their_arguments_without_a_gpu():
    lib = _lib.load()
    assert not lib.rpt_temporal_create(0, 0, 8) and b"size" in lib.rpt_last_error()
    assert not lib.rpt_temporal_create(0, 8, 0) and b"size" in lib.rpt_last_error()
    assert not lib.rpt_temporal_create(0, 1 << 16, 1 << 15) and b"size" in lib.rpt_last_error()
    assert not lib.rpt_temporal_create(-1, 8, 8) and b"device" in lib.rpt_last_error()
    assert not lib.rpt_temporal_create(1 << 20, 8, 8) and b"device" in lib.rpt_last_error()
    lib.rpt_temporal_destroy(None)
    n = C.c_uint32()
    assert lib.rpt_temporal_reset(None) == -1 and b"null" in lib.rpt_last_error()
    assert lib.rpt_temporal_frames(None, C.byref(n)) == -1 and b"null" in lib.rpt_last_error()
    # rpt_temporal_frame_image: the accumulation's parameters, the camera and the planes, the filter's, then the handles
    buf = np.zeros(8)
    p = buf.ctypes.data_as(C.c_void_p)
    q = np.zeros(8).ctypes.data_as(C.c_void_p)
    cam = camera_desc(Camera(), _lib.CameraDesc)
    T, D = _lib.TemporalParams, _lib.DenoiseParams
    dprm = D(4, 3, 4.0, 0.5, 0.0)

    def err(tprm, camera, planes, text, out=q):
        rc = lib.rpt_temporal_frame_image(None, C.byref(tprm) if tprm is not None else None, C.byref(camera) if camera is not None else None,
                                          None, None, C.byref(dprm), *planes, out)
        assert rc == -1 and text in lib.rpt_last_error(), lib.rpt_last_error()

    err(None, cam, [p, p, p], b"parameters")
    err(T(0, 1, 0.1, 0.5), cam, [p, p, p], b"max_history")
    err(T(16, 1, 0.1, 0.5), None, [p, p, p], b"null camera")
    err(T(16, 1, 0.1, 0.5), camera_desc(Camera(fov=4.0), _lib.CameraDesc), [p, p, p], b"fov")
    err(T(16, 1, 0.1, 0.5), cam, [p, None, p], b"normal_tol > 0")
    err(T(16, 1, 0.1, 0.5), cam, [p, p, None], b"depth")
    err(T(16, 1, 0.1, 0.5), cam, [p, p, p], b"null frame", out=None)
    err(T(16, 1, 0.1, 0.5), cam, [p, p, p], b"null accumulator")
    err(T(16, 1, 0.1, 0.0), cam, [None, None, p], b"null accumulator")       # normal_tol == 0: the plane is not read, given or not
    err(T(16, 1, 0.1, 0.0), cam, [None, p, p], b"null accumulator")


def test_python_wrappers_refuse_before_the_device():
    p = TemporalParams()
    assert (p.max_history, p.flags, p.depth_tol, p.normal_tol) == (16, 1, 0.1, 0.5)
    assert TemporalParams(match_id=False).flags == 0
    d = p.desc()
    assert (d.max_history, d.flags, d.depth_tol, d.normal_tol) == (16, 1, 0.1, 0.5)
    for kw in (dict(max_history=0), dict(max_history=4097), dict(depth_tol=-1.0), dict(normal_tol=NAN), dict(depth_tol=INF)):
        with pytest.raises(ValueError):
            TemporalParams(**kw)
    with pytest.raises(ValueError):
        TemporalAccumulator(0, 8)
    with pytest.raises(ValueError):
        TemporalAccumulator(8, -1)
    r = Renderer(Scene(), Camera()).width(8).height(8).num_samples(8)
    cams = [Camera(), Camera()]
    with pytest.raises(ValueError, match="2 batches"):
        r.render_sequence(cams, 1)
    with pytest.raises(ValueError, match="num_samples"):
        r.render_sequence(cams, 9)
    with pytest.raises(ValueError, match="TemporalParams"):
        r.render_sequence(cams, 4, temporal=DenoiseParams())
    with pytest.raises(ValueError, match="DenoiseParams"):
        r.render_sequence(cams, 4, denoise=TemporalParams())
    with pytest.raises(ValueError, match="sharded"):
        Renderer(Scene(), Camera()).width(8).height(8).num_samples(8).shard(0, 2).render_sequence(cams)
