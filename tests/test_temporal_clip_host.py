"""History clipping of the temporal accumulation (RPT_TEMPORAL_CLIP, rpt_temporal_set_clip), the parts that need no GPU: the numpy
restatement (tests/temporal_clip_ref.py) against a pixel-by-pixel, neighbour-by-neighbour transcription of include/rpt_hip.h in Python
floats; without the flag against tests/temporal_motion_ref.py bit for bit; exact inputs whose result the definition fixes; the
refusals of rpt_temporal_set_clip that precede the handle, TemporalParams and the two scenes; and the three quality conditions of
DESIGN.md section 4, "History clipping", on the oracle's renders (tools/temporal_clip_quality.py prints the whole grid)."""
import math

import numpy as np
import pytest

from rpt_amd import TemporalParams, _lib, scenes
from tests.temporal_clip_ref import (CLIP, CLIP_DEFAULTS, ClipRef, garbage_clip, oracle_sequence, quality_rows)
from tests.temporal_motion_ref import MotionRef, random_records
from tests.temporal_ref import EYES, FOV, MATCH_ID, analytic_planes, look_at_record

NAN, INF = float("nan"), float("inf")


def records(n=4, moving=True):
    return [look_at_record(EYES[k if moving else 0], (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), FOV) for k in range(n)]


def same(a, b):
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


# ---- the definition, one pixel, one tap, one neighbour and one Python float operation at a time
def div(a, b):
    try:
        return a / b
    except ZeroDivisionError:
        return NAN if (a == 0.0 or a != a) else math.copysign(INF, a) * math.copysign(1.0, b)


def dot3(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def fmax(a, b):
    return a if (a >= b or b != b) else b


def fmin(a, b):
    return a if (a <= b or b != b) else b


def is_finite(t):
    return not (t - t != 0.0)


class ScalarClip:
    def __init__(self, w, h):
        self.w, self.h, self.hist, self.rec = w, h, None, None
        self.clip = CLIP_DEFAULTS
        self.clipped = 0

    def accumulate(self, rec, rgb, var, normal, depth, table, max_history, flags, depth_tol, normal_tol):
        w, h = self.w, self.h
        rec = [float(t) for t in rec]
        eye, direction, right, up, d = rec[0:3], rec[3:6], rec[6:9], rec[9:12], rec[12]
        dim = float(max(w, h))
        m = len(table) if table is not None else 0
        radius, gamma, keep = self.clip
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
                    if flags & CLIP:
                        cnt, S, Q = 0.0, [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]
                        for dy in range(-radius, radius + 1):
                            for dx in range(-radius, radius + 1):
                                px, py = x + dx, y + dy
                                if not (0 <= px < w and 0 <= py < h):
                                    continue
                                c = rgb[py][px]
                                if not (is_finite(c[0]) and is_finite(c[1]) and is_finite(c[2])):
                                    continue
                                if flags & MATCH_ID and not depth[py][px][2] == ident:
                                    continue
                                cnt = cnt + 1.0
                                S = [S[k] + c[k] for k in range(3)]
                                Q = [Q[k] + c[k] * c[k] for k in range(3)]
                        if cnt > 0.0:
                            clipped = False
                            for k in range(3):
                                mk = S[k] / cnt
                                sk = fmax(Q[k] / cnt - mk * mk, 0.0)
                                sd = math.sqrt(sk)
                                lo, hi = mk - gamma * sd, mk + gamma * sd
                                t = fmin(fmax(hcol[k], lo), hi)
                                clipped = clipped or t != hcol[k]
                                hcol[k] = t
                            if clipped:
                                self.clipped += 1
                                if keep > 0:
                                    hl = fmin(hl, float(keep))
                    length = min(hl + 1.0, float(max_history))
                    a = 1.0 / length
                    o = [hcol[k] + (c_in[k] - hcol[k]) * a for k in range(3)]
                    om = 1.0 - a
                    ov = (om * om) * hvar + (a * a) * v_in
                else:
                    o, ov, length = list(c_in), v_in, 1.0
                out[y][x], out_v[y][x], out_len[y][x] = o, ov, length
                finite = hit and all(is_finite(t) for t in o + [ov])
                new[y][x] = (o, ov, length if finite else 0.0, list(n), zc, ident)
        self.hist, self.rec = new, rec
        return np.array(out).reshape(h, w, 3), np.array(out_v, dtype=np.float64).reshape(h, w), np.array(out_len, dtype=np.float64).reshape(h, w)


SETTINGS = [
    dict(max_history=16, flags=MATCH_ID | CLIP, depth_tol=0.1, normal_tol=0.0),
    dict(max_history=4, flags=CLIP, depth_tol=0.0, normal_tol=0.0),             # MATCH_ID off: every finite pixel of the window counts
    dict(max_history=8, flags=MATCH_ID | CLIP, depth_tol=0.0, normal_tol=2.5),
]
CLIPS = {1: (1, 0.5, 1), 2: (2, 1.0, 0), 3: (3, 0.25, 5)}


@pytest.mark.parametrize("w,h", [(5, 3), (33, 17)])
@pytest.mark.parametrize("radius", [1, 2, 3])
@pytest.mark.parametrize("k", range(len(SETTINGS)))
@pytest.mark.parametrize("m", [0, 3])
def test_restatement_equals_the_definition_pixel_by_pixel(w, h, radius, k, m):
    s = SETTINGS[k]
    ref, scalar = ClipRef(w, h), ScalarClip(w, h)
    ref.set_clip(*CLIPS[radius])
    scalar.clip = CLIPS[radius]
    took = clipped = 0
    for f, (rec, rgb, var, normal, depth) in enumerate(garbage_clip(11 * k + w + m + radius, w, h, records(3, moving=False), m)):
        table = random_records(100 * f + k + m, m) if f and m else None
        use_normal = normal if s["normal_tol"] > 0.0 else None
        got = ref.accumulate(rec, rgb, var, use_normal, depth, motion=table, **s)
        want = scalar.accumulate(rec, rgb.tolist(), var.tolist(), use_normal.tolist() if use_normal is not None else None, depth.tolist(),
                                 table.tolist() if table is not None else None, **s)
        for a, b, name in zip(got, want, ("colour", "variance", "len")):
            assert same(a, b), (f, name)
        took += int(ref.last["took"].sum())
        clipped += int(ref.last["clipped"].sum())
    assert clipped == scalar.clipped
    print(f"{w} x {h}, r {radius}, settings {k}, {m} records: {took} pixels took history, {clipped} were clipped")
    if (w, h) == (33, 17) and m == 0:
        assert took >= 100 and clipped >= 50                                # the step under test did run, and did change colours


# ---- without the flag nothing differs
@pytest.mark.parametrize("w,h", [(1, 1), (5, 3), (33, 17)])
@pytest.mark.parametrize("m", [0, 3])
def test_without_the_flag_every_output_equals_the_restatement_without_clipping(w, h, m):
    frames = garbage_clip(40 + w + m, w, h, records(4), m)
    plain, before, after = MotionRef(w, h), ClipRef(w, h), ClipRef(w, h)
    after.set_clip(3, 0.0, 0)
    for f, (rec, rgb, var, normal, depth) in enumerate(frames):
        table = random_records(7 * f + m, m) if f and m else None
        flags = (MATCH_ID, 0)[f % 2]
        want = plain.accumulate(rec, rgb, var, normal, depth, flags=flags, motion=table)
        for ref in (before, after):
            got = ref.accumulate(rec, rgb, var, normal, depth, flags=flags, motion=table)
            assert all(same(a, b) for a, b in zip(got, want)), f
            assert not ref.last["clipped"].any()


# ---- exact inputs
def constant_frames(w, h, colours, ids=None):
    """A fixed camera on the analytic scene, frame f one colour everywhere: every hit pixel reprojects onto itself."""
    rec = records(1)[0]
    normal, depth = analytic_planes(rec, w, h)
    if ids is not None:
        depth = depth.copy()
        depth[..., 2] = ids
    return [(rec, np.broadcast_to(np.array(c, dtype=np.float64), (h, w, 3)).copy(), np.full((h, w), 0.25), normal, depth) for c in colours]


@pytest.mark.parametrize("keep", [0, 1, 5])
@pytest.mark.parametrize("radius", [1, 3])
def test_a_constant_frame_over_another_constant_history_is_the_frame(keep, radius):
    """sd = 0: lo = hi = the frame's colour (dyadic, so that the window's mean is exact), the clamped history is the frame and so is the
    blend.  Three frames of history make hl 3: a clipped pixel keeps min(3, clip_history) of it (all of it at 0)."""
    w, h = 9, 7
    a, b = (0.75, 0.5, 0.25), (0.125, 2.0, 1.5)
    frames = constant_frames(w, h, [a, a, a, b])
    ref, plain = ClipRef(w, h), ClipRef(w, h)
    ref.set_clip(radius, 0.5, keep)
    for fr in frames[:3]:
        ref.accumulate(*fr)
        plain.accumulate(*fr)
    out, _, length = ref.accumulate(*frames[3], flags=MATCH_ID | CLIP)
    _, _, plain_length = plain.accumulate(*frames[3])
    took = ref.last["took"]
    assert took.sum() >= 0.9 * w * h and np.array_equal(ref.last["clipped"], took)
    assert np.array_equal(out, frames[3][1])
    assert np.array_equal(plain_length[took], np.full(int(took.sum()), 4.0))
    assert np.array_equal(length[took], np.full(int(took.sum()), 2.0 if keep == 1 else 4.0))


@pytest.mark.parametrize("w,h", [(5, 3), (33, 17)])
def test_a_huge_gamma_clips_nothing(w, h):
    """Finite colours, MATCH_ID off: every window holds at least four pixels of different colours, sd > 0, and 1e300 sd reaches past any
    history: all outputs equal the unclipped ones."""
    rng = np.random.default_rng(5)
    recs = records(4)
    ref, plain = ClipRef(w, h), ClipRef(w, h)
    ref.set_clip(2, 1e300, 1)
    for rec in recs:
        normal, depth = analytic_planes(rec, w, h)
        rgb, var = rng.uniform(0.0, 2.0, (h, w, 3)), rng.uniform(0.0, 0.05, (h, w))
        got = ref.accumulate(rec, rgb, var, normal, depth, flags=CLIP)
        want = plain.accumulate(rec, rgb, var, normal, depth, flags=0)
        assert all(same(a, b) for a, b in zip(got, want)) and not ref.last["clipped"].any()
    assert ref.last["took"].sum() >= 0.5 * w * h


def test_a_frame_of_one_pixel():
    """The window is the pixel itself: n = 1, sd = 0, the history is clamped to the frame."""
    frames = constant_frames(1, 1, [(0.3, 0.2, 0.1), (0.7, 0.1, 0.9), (math.nan, 0.1, 0.9), (0.2, 0.2, 0.2), (0.4, 0.4, 0.4)])
    for radius in (1, 2, 3):
        ref, scalar = ClipRef(1, 1), ScalarClip(1, 1)
        ref.set_clip(radius, 0.5, 1)
        scalar.clip = (radius, 0.5, 1)
        for f, (rec, rgb, var, normal, depth) in enumerate(frames):
            got = ref.accumulate(rec, rgb, var, normal, depth, flags=MATCH_ID | CLIP)
            want = scalar.accumulate(rec, rgb.tolist(), var.tolist(), normal.tolist(), depth.tolist(), None, 16, MATCH_ID | CLIP, 0.1, 0.5)
            assert all(same(a, b) for a, b in zip(got, want)), f
            assert f == 2 or same(got[0], rgb)
            # frame 1 clips; frame 2 is NaN: nothing counts, the history passes unclipped and NaN is blended in; frame 3 has no history
            assert (bool(ref.last["took"][0, 0]), bool(ref.last["clipped"][0, 0]), float(got[2][0, 0])) == \
                [(False, False, 1.0), (True, True, 2.0), (True, False, 3.0), (False, False, 1.0), (True, True, 2.0)][f]


def test_a_pixel_whose_neighbours_all_carry_other_ids():
    """With MATCH_ID its window holds itself alone (the history is clamped to its own colour); without, the whole window."""
    w, h = 7, 5
    ids = np.ones((h, w))
    ids[2, 3] = 7.0
    rng = np.random.default_rng(9)
    rec = records(1)[0]
    normal, depth = analytic_planes(rec, w, h)
    depth = depth.copy()
    depth[..., 2] = ids
    for flags in (MATCH_ID | CLIP, CLIP):
        ref = ClipRef(w, h)
        for f in range(3):
            rgb = rng.uniform(0.0, 2.0, (h, w, 3))
            out, _, length = ref.accumulate(rec, rgb, None, normal, depth, flags=flags)
        assert ref.last["took"][2, 3]
        if flags & MATCH_ID:
            assert np.array_equal(out[2, 3], rgb[2, 3]) and ref.last["clipped"][2, 3] and length[2, 3] == 2.0
        else:
            assert not np.array_equal(out[2, 3], rgb[2, 3])
        assert not np.array_equal(out[1, 1], rgb[1, 1])


def test_a_nan_id_counts_nothing_and_is_not_clipped():
    w, h = 5, 3
    frames = constant_frames(w, h, [(0.5, 0.5, 0.5), (1.0, 1.0, 1.0)], ids=np.where(np.arange(15).reshape(3, 5) == 7, NAN, 1.0))
    ref = ClipRef(w, h)
    for fr in frames:
        ref.accumulate(*fr, flags=CLIP)                                     # MATCH_ID off: the NaN id takes history and is clipped like the rest
    assert ref.last["took"][1, 2] and ref.last["clipped"][1, 2]
    ref = ClipRef(w, h)
    for fr in frames:
        ref.accumulate(*fr, flags=MATCH_ID | CLIP)                          # on: NaN == NaN is false for the taps already
    assert not ref.last["took"][1, 2] and ref.last["clipped"].sum() == ref.last["took"].sum() > 0


# ---- the setter, the parameters, the scenes
def test_set_clip_checks_its_arguments_in_order_and_before_the_handle():
    lib = _lib.load()
    for radius in (0, 4, 0xFFFFFFFF):
        assert lib.rpt_temporal_set_clip(None, radius, NAN, 5000) == -1 and b"radius" in lib.rpt_last_error()
    for gamma in (NAN, INF, -INF, -1e-300, -1.0):
        assert lib.rpt_temporal_set_clip(None, 1, gamma, 5000) == -1 and b"gamma" in lib.rpt_last_error()
    for keep in (4097, 0xFFFFFFFF):
        assert lib.rpt_temporal_set_clip(None, 3, 0.0, keep) == -1 and b"clip_history" in lib.rpt_last_error()
    for args in ((1, 0.0, 0), (3, 1e300, 4096), (2, -0.0, 1)):
        assert lib.rpt_temporal_set_clip(None, *args) == -1 and b"null accumulator" in lib.rpt_last_error()
    for ref_args in ((0, 0.5, 1), (4, 0.5, 1), (1, NAN, 1), (1, INF, 1), (1, -1.0, 1), (1, 0.5, 4097), (1, 0.5, -1)):
        with pytest.raises(ValueError):
            ClipRef(2, 2).set_clip(*ref_args)


@pytest.mark.parametrize("device", [False, True])
def test_the_flag_check_admits_the_two_flags_and_no_other(device):
    """No accumulator exists and no GPU is needed: with bit 1 (RPT_TEMPORAL_CLIP) set the next refusal is the handle's, as without
    it; every other bit is an unknown flag, with the two known ones or without."""
    import ctypes as C
    from rpt_amd import Camera
    from rpt_amd.api import camera_desc
    lib = _lib.load()
    fn = lib.rpt_temporal_accumulate_device if device else lib.rpt_temporal_accumulate
    rgb, normal, depth, out = [np.zeros((4, 4, 3)) for _ in range(4)]
    cam = camera_desc(Camera(), _lib.CameraDesc)
    planes = [a.ctypes.data_as(C.c_void_p) for a in (rgb, normal, depth, out)]

    def call(flags):
        prm = _lib.TemporalParams(16, flags, 0.1, 0.5)
        args = [None, C.byref(prm), C.byref(cam), planes[0], None, planes[1], planes[2], planes[3], None, None]
        return (fn(*args, None) if device else fn(*args)), lib.rpt_last_error()

    for flags in (0, 1, 2, 3):
        rc, text = call(flags)
        assert rc == -1 and b"null accumulator" in text, flags
    for flags in (4, 5, 6, 7, 8, 0x80000000, 0xFFFFFFFF):
        rc, text = call(flags)
        assert rc == -1 and b"unknown temporal flag" in text, flags


def test_temporal_params_carry_the_flag():
    p = TemporalParams()
    assert (p.max_history, p.flags, p.depth_tol, p.normal_tol, p.clip) == (16, 1, 0.1, 0.5, False)
    assert TemporalParams(clip=True).flags == 3 and TemporalParams(match_id=False, clip=True).flags == 2 == CLIP
    d = TemporalParams(clip=True).desc()
    assert (d.max_history, d.flags, d.depth_tol, d.normal_tol) == (16, 3, 0.1, 0.5)
    assert CLIP_DEFAULTS == (1, 0.5, 1)


def test_the_two_scenes_move_one_thing_each():
    for fn, moving, rest in ((scenes.sliding_shadow, 1, 5), (scenes.moving_light, 5, 1)):
        s0, cam, cfg = fn(0)
        s3 = fn(3)[0]
        assert [o.shape.base().KIND for o in s0.objects] == [0, 1, 0, 0, 2, 0] and cfg["max_bounces"] == 1
        assert len(s0.lights) == 2 and "CONFIGS" in dir(scenes) and fn not in scenes.CONFIGS.values()
        for i in range(6):
            m0, m3 = s0.objects[i].shape.matrix(), s3.objects[i].shape.matrix()
            assert ((m0 is None and m3 is None) or np.array_equal(m0, m3)) == (i != moving), i
        assert s0.objects[rest].shape.matrix()[:3, 3].tolist() == ([0.0, 4.0, 4.0] if rest == 5 else [0.4, -0.7, 4.0])
    assert scenes.sliding_shadow(2)[0].objects[1].shape.matrix()[:3, 3].tolist() == [-1.5 + 0.4 * 2, -0.7, 4.0]
    assert scenes.moving_light(2)[0].objects[5].shape.matrix()[:3, 3].tolist() == [-3.0 + 0.75 * 2, 4.0, 4.0]
    assert scenes.moving_light(2, step=0.5)[0].objects[5].shape.matrix()[0, 3] == -2.0


# ---- quality: directions, never thresholds ("History clipping")
@pytest.mark.parametrize("name", ["sliding_shadow", "moving_light"])
def test_quality_conditions_on_the_oracles_renders(name):
    frames, converged, earlier = oracle_sequence(getattr(scenes, name))
    n_static, n_changed, rows = quality_rows(frames, converged, earlier, [CLIP_DEFAULTS])
    alone, plain, clip = rows["alone"], rows["plain"], rows[CLIP_DEFAULTS]
    print(f"{name} (CPU: oracle + restatement), 64 x 48, 8 frames of 4 x 1 spp against 512 spp, RMS in 8-bit levels: changed mask "
          f"({n_changed} pixels) alone {alone[0]:.2f}, accumulated {plain[0]:.2f}, clipped {clip[0]:.2f}; static mask ({n_static}) alone "
          f"{alone[1]:.2f}, accumulated {plain[1]:.2f}, clipped {clip[1]:.2f}")
    assert n_changed >= 30
    assert clip[0] < plain[0]
    assert clip[1] < plain[1] and clip[1] < alone[1]
