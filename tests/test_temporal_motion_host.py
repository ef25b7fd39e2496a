"""Temporal accumulation of moving objects (rpt_temporal_motion_record, rpt_temporal_set_motion*), the parts that need no GPU: the
numpy restatement with a motion table (tests/temporal_motion_ref.py) against the one without (tests/temporal_ref.py) where no object
moves, and against a pixel-by-pixel, tap-by-tap transcription of include/rpt_hip.h with random affine records;
rpt_temporal_motion_record through the C ABI (the header's order bit for bit, exact inputs, numpy.linalg, every refusal); the
refusals of rpt_temporal_set_motion* that precede the handle; and the conditions on the moving analytic scene that keep the bit-for-bit
tests of tests/test_gpu_temporal_motion.py from passing with the motion map, or its normal half, dead."""
import ctypes as C
import math

import numpy as np
import pytest

from rpt_amd import Camera, Renderer, Scene, _lib, scenes
from rpt_amd.api import temporal_motion_record
from tests.temporal_motion_ref import (IDENTITY_RECORD, MotionRef, garbage_motion, motion_record, moving_sequence, random_matrix, random_records,
                                       rotation, scaling, translation)
from tests.temporal_ref import EYES, FOV, MATCH_ID, TemporalRef, garbage, look_at_record, sequence

NAN, INF = float("nan"), float("inf")
SIZES = [(1, 1), (5, 3), (33, 17), (64, 48)]


def records(n=4, moving=True):
    return [look_at_record(EYES[k if moving else 0], (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), FOV) for k in range(n)]


def same(a, b):
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


# ---- no motion: nothing differs
@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("planes", ["sequence", "garbage"])
def test_no_table_and_identity_table_equal_the_restatement_without_motion(w, h, planes):
    frames = (sequence if planes == "sequence" else garbage)(w + 3 * h, w, h, records(4))
    identity = np.tile(IDENTITY_RECORD, (3, 1))
    ref, none, ident = TemporalRef(w, h), MotionRef(w, h), MotionRef(w, h)
    for f, (rec, rgb, var, normal, depth) in enumerate(frames):
        want = ref.accumulate(rec, rgb, var, normal, depth)
        for name, got in (("no table", none.accumulate(rec, rgb, var, normal, depth)),
                          ("identity table", ident.accumulate(rec, rgb, var, normal, depth, motion=identity))):
            for a, b, what in zip(got, want, ("colour", "variance", "len")):
                assert same(a, b), (f, name, what)


# ---- the definition with a table, one pixel, one tap and one Python float operation at a time
def div(a, b):
    try:
        return a / b
    except ZeroDivisionError:
        return NAN if (a == 0.0 or a != a) else math.copysign(INF, a) * math.copysign(1.0, b)


def dot3(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


class ScalarMotion:
    def __init__(self, w, h):
        self.w, self.h, self.hist, self.rec = w, h, None, None

    def accumulate(self, rec, rgb, var, normal, depth, table, max_history, flags, depth_tol, normal_tol):
        w, h = self.w, self.h
        rec = [float(t) for t in rec]
        eye, direction, right, up, d = rec[0:3], rec[3:6], rec[6:9], rec[9:12], rec[12]
        dim = float(max(w, h))
        m = len(table) if table is not None else 0
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
                    P = [eye[k] + s * v[k] for k in range(3)]
                    nm = n
                    if m and ident >= 1.0 and ident <= float(m):
                        r = table[int(ident) - 1]
                        P = [((r[4 * k] * P[0] + r[4 * k + 1] * P[1]) + r[4 * k + 2] * P[2]) + r[4 * k + 3] for k in range(3)]
                        nm = [(r[12 + 3 * k] * n[0] + r[13 + 3 * k] * n[1]) + r[14 + 3 * k] * n[2] for k in range(3)]
                    q = [P[k] - p[k] for k in range(3)]
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
                                        r2 = hz * hz
                                        if not abs(r2 - qq) <= depth_tol * qq:
                                            continue
                                    if normal_tol > 0.0:
                                        e = [hn[k] - nm[k] for k in range(3)]
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
    dict(max_history=4, flags=0, depth_tol=0.0, normal_tol=0.0),                # every test off: a moved point is always taken
    dict(max_history=4, flags=0, depth_tol=0.0, normal_tol=0.7),                # the normal map alone decides
    dict(max_history=4, flags=MATCH_ID, depth_tol=0.3, normal_tol=0.0),
]


@pytest.mark.parametrize("w,h", [(5, 3), (33, 17)])
@pytest.mark.parametrize("k", range(len(SETTINGS)))
@pytest.mark.parametrize("m", [1, 3])
def test_restatement_equals_the_definition_pixel_by_pixel(w, h, k, m):
    s = SETTINGS[k]
    ref, scalar = MotionRef(w, h), ScalarMotion(w, h)
    took = 0
    for f, (rec, rgb, var, normal, depth) in enumerate(garbage_motion(7 * k + w + m, w, h, records(3), m)):
        table = random_records(100 * f + k + m, m) if f else None
        use_normal = normal if s["normal_tol"] > 0.0 else None
        got = ref.accumulate(rec, rgb, var, use_normal, depth, motion=table, **s)
        want = scalar.accumulate(rec, rgb.tolist(), var.tolist(), use_normal.tolist() if use_normal is not None else None, depth.tolist(),
                                 table.tolist() if table is not None else None, **s)
        for a, b, name in zip(got, want, ("colour", "variance", "len")):
            assert same(a, b), (f, name)
        if f and table is not None:
            ids = depth[..., 2]
            took += int((ref.last["took"] & (ids >= 1.0) & (ids <= float(m))).sum())
    if (w, h) == (33, 17) and k in (1, 2):
        assert took > 0                                                     # pixels with a record did take history


# ---- rpt_temporal_motion_record
def capi_record(cur, prev):
    lib = _lib.load()
    dp = C.POINTER(C.c_double)
    cur, prev = [np.ascontiguousarray(m, dtype=np.float64).reshape(16) for m in (cur, prev)]
    out = np.full(24, 7.0)
    rc = lib.rpt_temporal_motion_record(cur.ctypes.data_as(dp), prev.ctypes.data_as(dp), out.ctypes.data_as(dp))
    return rc, out


def test_motion_record_is_the_headers_order_bit_for_bit():
    rng = np.random.default_rng(11)
    for _ in range(200):
        cur, prev = random_matrix(rng), random_matrix(rng)
        rc, got = capi_record(cur, prev)
        assert rc == 0 and same(got, motion_record(cur, prev))
        assert same(temporal_motion_record(cur, prev), got)
        assert got[21:].tolist() == [0.0, 0.0, 0.0]


def test_motion_record_is_exact_on_exact_inputs():
    eye3 = np.eye(3).reshape(-1).tolist()
    # dyadic translations: A = I, t = prev_t - cur_t, G = I
    cur, prev = translation((0.5, -1.25, 3.0)), translation((2.0, 0.75, -0.125))
    rc, r = capi_record(cur, prev)
    assert rc == 0 and r[:12].reshape(3, 4)[:, :3].reshape(-1).tolist() == eye3 and r[:12].reshape(3, 4)[:, 3].tolist() == [1.5, 2.0, -3.125]
    assert r[12:21].tolist() == eye3
    # quarter turns about each axis, composed with a dyadic translation
    for axis in ((1, 0, 0), (0, 1, 0), (0, 0, 1)):
        turn = np.round(rotation(math.pi / 2, axis))
        cur, prev = translation((1.0, 2.0, -0.5)) @ turn, translation((0.25, 0.0, 4.0))
        rc, r = capi_record(cur, prev)
        want = prev @ np.linalg.inv(cur)
        assert rc == 0 and np.array_equal(r[:12].reshape(3, 4), want[:3]) and np.array_equal(r[12:21].reshape(3, 3), want[:3, :3])
    # a scale by 2: A_lin = 0.5 I, G = 2 I
    rc, r = capi_record(scaling(2.0), np.eye(4))
    assert rc == 0 and np.array_equal(r[:12].reshape(3, 4), 0.5 * np.eye(4)[:3]) and np.array_equal(r[12:21].reshape(3, 3), 2.0 * np.eye(3))


def test_equal_inputs_give_the_identity_record():
    rng = np.random.default_rng(3)
    for _ in range(20):
        m = random_matrix(rng)
        rc, r = capi_record(m, m.copy())
        assert rc == 0 and np.array_equal(r, IDENTITY_RECORD) and not np.signbit(r).any()
    assert np.array_equal(temporal_motion_record(None, None), IDENTITY_RECORD)
    assert np.array_equal(motion_record(None, None), IDENTITY_RECORD)
    assert same(temporal_motion_record(translation((1.0, 0.0, 0.0)), None), motion_record(translation((1.0, 0.0, 0.0)), None))


def test_motion_record_against_numpy_linalg():
    """Matrices composed as T . R . S with scales in [0.5, 2]: linear parts of condition <= 4 each, their product <= 16; a few dozen
    operations at 1.1e-16 each leave more than a decade below 1e-12 of the largest entry."""
    rng = np.random.default_rng(5)
    worst = 0.0
    for _ in range(300):
        cur, prev = random_matrix(rng), random_matrix(rng)
        rc, r = capi_record(cur, prev)
        a = prev @ np.linalg.inv(cur)
        g = np.linalg.inv(a[:3, :3]).T
        ea = np.abs(r[:12].reshape(3, 4) - a[:3]).max() / np.abs(a[:3]).max()
        eg = np.abs(r[12:21].reshape(3, 3) - g).max() / np.abs(g).max()
        worst = max(worst, ea, eg)
        assert rc == 0
    print(f"motion record against numpy.linalg: worst relative error {worst:.2e}")
    assert worst <= 1e-12


def test_motion_record_refusals():
    lib = _lib.load()
    ok = translation((1.0, 2.0, 3.0)) @ scaling(0.5)
    dp = C.POINTER(C.c_double)
    good = np.ascontiguousarray(ok).reshape(16)
    out = np.zeros(24)
    for args in ((None, good.ctypes.data_as(dp), out.ctypes.data_as(dp)), (good.ctypes.data_as(dp), None, out.ctypes.data_as(dp)),
                 (good.ctypes.data_as(dp), good.ctypes.data_as(dp), None)):
        assert lib.rpt_temporal_motion_record(*args) == -1 and b"null" in lib.rpt_last_error()
    for which in (0, 1):
        for at in (0, 3, 5, 11, 12, 15):
            for bad in (NAN, INF, -INF):
                mats = [ok.copy(), np.eye(4)]
                mats[which].reshape(-1)[at] = bad
                rc, _ = capi_record(*mats)
                assert rc == -1 and b"finite" in lib.rpt_last_error(), (which, at, bad)
                with pytest.raises(ValueError, match="finite"):
                    motion_record(*mats)
        for at, value in ((12, 0.5), (13, -1.0), (14, 1e-300), (15, 0.0), (15, 2.0)):
            mats = [ok.copy(), np.eye(4)]
            mats[which].reshape(-1)[at] = value
            rc, _ = capi_record(*mats)
            assert rc == -1 and b"bottom row" in lib.rpt_last_error(), (which, at)
            with pytest.raises(ValueError, match="bottom row"):
                motion_record(*mats)
    # a current matrix with no inverse (and an equal previous one: the determinant is asked for first)
    flat = scaling(1.0)
    flat[1, 1] = 0.0
    for prev in (np.eye(4), flat.copy()):
        rc, _ = capi_record(flat, prev)
        assert rc == -1 and b"current matrix" in lib.rpt_last_error()
        with pytest.raises(ValueError, match="current matrix"):
            motion_record(flat, prev)
    huge = scaling(1e200)
    rc, _ = capi_record(huge, np.eye(4))                                      # det = 1e600: not finite
    assert rc == -1 and b"current matrix" in lib.rpt_last_error()
    # a previous matrix that flattens the object: A has no inverse
    rc, _ = capi_record(ok, flat)
    assert rc == -1 and b"between the frames" in lib.rpt_last_error()
    with pytest.raises(ValueError, match="between the frames"):
        motion_record(ok, flat)
    rc, _ = capi_record(scaling(1e-60), scaling(1e60))                        # A = 1e120 I: det' = 1e360
    assert rc == -1 and b"between the frames" in lib.rpt_last_error()
    with pytest.raises(_lib.RptError, match="bottom row"):
        bad = np.eye(4)
        bad[3, 0] = 1.0
        temporal_motion_record(bad, None)


def test_set_motion_checks_its_arguments_before_the_handle():
    lib = _lib.load()
    dp = C.POINTER(C.c_double)
    table = np.tile(IDENTITY_RECORD, (3, 1))
    assert lib.rpt_temporal_set_motion(None, None, 2) == -1 and b"null motion records" in lib.rpt_last_error()
    assert lib.rpt_temporal_set_motion_device(None, None, 2) == -1 and b"null motion records" in lib.rpt_last_error()
    for at in range(21):
        for bad in (NAN, INF, -INF):
            t = table.copy()
            t[2, at] = bad
            assert lib.rpt_temporal_set_motion(None, t.ctypes.data_as(dp), 3) == -1 and b"finite" in lib.rpt_last_error(), at
    # the three padding doubles are never read
    t = table.copy()
    t[:, 21:] = NAN
    assert lib.rpt_temporal_set_motion(None, t.ctypes.data_as(dp), 3) == -1 and b"null accumulator" in lib.rpt_last_error()
    assert lib.rpt_temporal_set_motion(None, None, 0) == -1 and b"null accumulator" in lib.rpt_last_error()
    assert lib.rpt_temporal_set_motion_device(None, t.ctypes.data_as(C.c_void_p), 3) == -1 and b"null accumulator" in lib.rpt_last_error()


def test_render_sequence_refuses_scenes_that_do_not_match():
    r = Renderer(Scene(), Camera()).width(8).height(8).num_samples(8)
    cams = [Camera(), Camera()]
    a, b = scenes.simple_video(0)[0], scenes.simple_video(1)[0]
    with pytest.raises(ValueError, match="one Scene per camera"):
        r.render_sequence(cams, scenes=[a])
    with pytest.raises(ValueError, match="Scene objects"):
        r.render_sequence(cams, scenes=[a, None])
    short = scenes.simple_video(1)[0]
    short.objects.pop()
    with pytest.raises(ValueError, match="same base shape kinds"):
        r.render_sequence(cams, scenes=[a, short])
    swapped = scenes.simple_video(1)[0]
    swapped.objects[0], swapped.objects[1] = swapped.objects[1], swapped.objects[0]
    with pytest.raises(ValueError, match="same base shape kinds"):
        r.render_sequence(cams, scenes=[a, swapped])
    assert r.scene is not a and r.scene is not b


def test_simple_video_moves_the_cube_alone():
    s0, cam, cfg = scenes.simple_video(0)
    s3 = scenes.simple_video(3, step=0.25)[0]
    assert [o.shape.base().KIND for o in s0.objects] == [0, 1, 0, 0, 2] and cfg == {"width": 800, "height": 600, "spp": 100, "max_bounces": 1}
    assert s0.objects[1].shape.matrix()[2, 3] == 4.0 and s3.objects[1].shape.matrix()[2, 3] == 4.75
    for i in (0, 2, 3, 4):
        m0, m3 = s0.objects[i].shape.matrix(), s3.objects[i].shape.matrix()
        assert (m0 is None and m3 is None) or np.array_equal(m0, m3)
    r = temporal_motion_record(s3.objects[1].shape.matrix(), s0.objects[1].shape.matrix())
    assert np.abs(r[:12].reshape(3, 4) - np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, -0.75]])).max() < 1e-15


# ---- the conditions on the moving analytic scene (64 x 48, default parameters, frames 1 to 3)
def run(frames, tables):
    """-> per frame 1..3: (sphere pixels, those that took history, the median paint error over them)."""
    ref = MotionRef(64, 48)
    stats = []
    for f, fr in enumerate(frames):
        out, _, _ = ref.accumulate(fr["rec"], fr["rgb"], fr["var"], fr["normal"], fr["depth"], motion=tables[f])
        if f:
            took = ref.last["took"] & fr["sphere"]
            err = np.abs(out - fr["rgb"]).max(axis=-1)[took]
            stats.append((int(fr["sphere"].sum()), int(took.sum()), float(np.median(err)) if err.size else NAN))
    return stats


@pytest.mark.parametrize("moving", [False, True])
def test_condition_1_and_2_the_table_follows_the_sphere(moving):
    frames = moving_sequence(64, 48, records(4, moving), 0.4)
    with_table = run(frames, [fr["table"] for fr in frames])
    without = run(frames, [None] * 4)
    print(f"{'moving' if moving else 'fixed'} camera, spin 0.4, with the table (sphere pixels, took history, median paint error): {with_table}")
    print(f"{'moving' if moving else 'fixed'} camera, spin 0.4, without: {without}")
    for (n, took, err), (n0, took0, err0) in zip(with_table, without):
        assert n == n0 and n >= 250
        assert took >= 0.95 * n                                             # condition 1
        assert took0 <= 0.75 * n0                                           # condition 2
        assert err <= 0.1 * err0


def test_condition_3_the_normal_map_is_alive():
    frames = moving_sequence(64, 48, records(4, True), 0.8)
    full = run(frames, [fr["table"] for fr in frames])
    no_g = []
    for fr in frames:
        t = None
        if fr["table"] is not None:
            t = fr["table"].copy()
            t[:, 12:21] = IDENTITY_RECORD[12:21]
        no_g.append(t)
    dead = run(frames, no_g)
    print(f"moving camera, spin 0.8, the full record: {full}")
    print(f"moving camera, spin 0.8, G replaced by the identity: {dead}")
    for (n, took, _), (_, took0, _) in zip(full, dead):
        assert took >= 0.9 * n
        assert took0 <= 0.5 * n


# ---- the rendered sequence of tests/test_gpu_temporal_motion.py, first on the CPU: the oracle's closest hits through pixel centres
VIDEO_W, VIDEO_H = 64, 48
VIDEO = {4: dict(first=1, step=0.5), 8: dict(first=1, step=0.25)}            # n frames -> simple_video(first + f, step)


def video_scenes(n):
    return [scenes.simple_video(VIDEO[n]["first"] + f, VIDEO[n]["step"]) for f in range(n)]


@pytest.mark.parametrize("n", [4, 8])
def test_the_video_sequences_cube_is_large_enough_and_moves(n):
    """In every frame the cube covers at least 100 pixels of 64 x 48 and some point of it moves by at least one pixel; with the table
    at least 80 % of its pixels take history (the restatement on the oracle's planes)."""
    from oracle import pyoracle
    from rpt_amd import temporal_camera_record
    from tests.temporal_ref import pixel_rays
    w, h = VIDEO_W, VIDEO_H
    ref, prev, rows = MotionRef(w, h), None, []
    ys, xs = np.mgrid[0:h, 0:w]
    for f, (scene, cam, cfg) in enumerate(video_scenes(n)):
        rec = temporal_camera_record(cam)
        v, l = pixel_rays(rec, w, h)
        t, obj, nrm = pyoracle.OracleScene(scene).intersect(np.tile(rec[0:3], (w * h, 1)), (v / l[..., None]).reshape(-1, 3), robust=1)
        hit = obj >= 0
        depth = np.stack([np.where(hit, t, 0.0), hit.astype(np.float64), (obj + 1).astype(np.float64)], axis=1).reshape(h, w, 3)
        normal = np.where(hit[:, None], nrm, 0.0).reshape(h, w, 3)
        table = None
        if prev is not None:
            table = np.stack([temporal_motion_record(c.shape.matrix(), p.shape.matrix()) for c, p in zip(scene.objects, prev.objects)])
        ref.accumulate(rec, np.zeros((h, w, 3)), None, normal, depth, motion=table)
        cube = (obj == 1).reshape(h, w)
        assert cube.sum() >= 100, f
        if f:
            shift = np.hypot(ref.last["fx"] - xs, ref.last["fy"] - ys)[cube]
            took = int((ref.last["took"] & cube).sum())
            rows.append((int(cube.sum()), took, round(float(np.nanmax(shift)), 2)))
            assert np.nanmax(shift) >= 1.0 and took >= 0.8 * cube.sum(), f
        prev = scene
    print(f"simple_video, {n} frames, step {VIDEO[n]['step']}: (cube pixels, took history, largest shift in pixels) {rows}")
