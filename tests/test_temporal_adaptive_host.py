"""Adaptive sampling over a sequence on the host (no device): the restatements of tests/temporal_adaptive_ref.py against a
pixel-by-pixel, slot-by-slot transcription of include/rpt_hip.h; the two properties of the loop on random batches; what the C ABI and
the Python wrappers refuse before any device call; and the quality conditions of DESIGN.md section 4, "Adaptive sampling over a
sequence", on the oracle's renders."""
import copy
import ctypes as C
import functools
import math

import numpy as np
import pytest

from rpt_amd import AdaptiveParams, Camera, Renderer, Scene, TemporalParams, _lib
from tests import temporal_adaptive_ref as tar
from tests.adaptive_ref import RefBuffer, select, tile_grid
from tests.temporal_clip_ref import CLIP, ClipRef, garbage_clip
from tests.temporal_motion_ref import random_records
from tests.temporal_ref import MATCH_ID
from tests.test_temporal_clip_host import ScalarClip, records

NAN, INF = math.nan, math.inf
SENTINEL = -7.25


def same(a, b):
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


# ---- 1: the preview is steps 1 - 5 of the definition, in the listed tiles, and nothing else
SETTINGS = [
    dict(max_history=16, flags=MATCH_ID, depth_tol=0.1, normal_tol=0.0),
    dict(max_history=4, flags=CLIP, depth_tol=0.0, normal_tol=0.0),
    dict(max_history=8, flags=MATCH_ID | CLIP, depth_tol=0.0, normal_tol=2.5),
]
LISTS = {(5, 3): [None, [0], [], [7]], (33, 17): [None, [0], [1], [1, 0], [5, 1]]}           # 7 and 5: out of range


@pytest.mark.parametrize("w,h", [(5, 3), (33, 17)])
@pytest.mark.parametrize("k", range(len(SETTINGS)))
@pytest.mark.parametrize("m", [0, 3])
def test_preview_equals_the_definition_pixel_by_pixel(w, h, k, m):
    s = SETTINGS[k]
    ref, scalar = ClipRef(w, h), ScalarClip(w, h)
    ref.set_clip(2, 0.5, 1)
    scalar.clip = (2, 0.5, 1)
    took = 0
    for f, (rec, rgb, var, normal, depth) in enumerate(garbage_clip(23 * k + w + m, w, h, records(3, moving=False), m)):
        table = random_records(100 * f + k + m, m) if f and m else None
        use_normal = normal if s["normal_tol"] > 0.0 else None
        lists = [x.tolist() if x is not None else None for x in (rgb, var, use_normal, depth, table)]
        for tiles in LISTS[(w, h)]:
            got = tar.preview(ref, rec, rgb, var, use_normal, depth, tiles=tiles, fill=SENTINEL, motion=table, **s)
            twin = copy.deepcopy(scalar)                                    # the transcription's step 6 happens to a copy
            want = twin.accumulate(rec, lists[0], lists[1], lists[2], lists[3], lists[4], **s)
            tx, _ = tile_grid(w, h)
            for y in range(h):
                for x in range(w):
                    listed = tiles is None or (y // 32) * tx + x // 32 in tiles
                    for a, b in zip(got, want):
                        if listed:
                            assert same(np.asarray(a[y, x]), np.asarray(b[y, x])), (f, tiles, x, y)
                        else:
                            assert (np.asarray(a[y, x]) == SENTINEL).all(), (f, tiles, x, y)
        # the real accumulation moves both on
        a = ref.accumulate(rec, rgb, var, use_normal, depth, motion=table, **s)
        b = scalar.accumulate(rec, lists[0], lists[1], lists[2], lists[3], lists[4], **s)
        assert all(same(x, y) for x, y in zip(a, b))
        took += int(ref.last["took"].sum())
    if (w, h) == (33, 17) and m == 0:
        assert took >= 100


def test_preview_leaves_the_accumulator_untouched():
    w, h = 33, 17
    frames = garbage_clip(5, w, h, records(4, moving=False), 3)
    ref, twin = ClipRef(w, h), ClipRef(w, h)
    kw = dict(flags=MATCH_ID | CLIP, normal_tol=0.0)
    for f, (rec, rgb, var, normal, depth) in enumerate(frames):
        table = random_records(f, 3) if f else None
        before = copy.deepcopy(ref)
        for tiles in (None, [1], []):
            tar.preview(ref, rec, rgb, var, None, depth, tiles=tiles, motion=table, **kw)
        assert ref.frames == before.frames == f
        assert (ref.hist is None) == (before.hist is None)
        if ref.hist is not None:
            assert all(same(a, b) for a, b in zip(ref.hist, before.hist)) and same(ref.rec, before.rec)
        # ... and the accumulation behind any number of previews is the one of an accumulator that never previewed
        got = ref.accumulate(rec, rgb, var, None, depth, motion=table, **kw)
        want = twin.accumulate(rec, rgb, var, None, depth, motion=table, **kw)
        assert all(same(a, b) for a, b in zip(got, want))
    # without a frame: out = rgb, out_v = v_in, len = 1.0
    rec, rgb, var, normal, depth = frames[0]
    out, out_v, length = tar.preview(ClipRef(w, h), rec, rgb, var, None, depth, **kw)
    assert same(out, rgb) and same(out_v, var) and (length == 1.0).all()


# ---- 2: the tile errors of planes
def scalar_plane_errors(rgb, var, w, h, floor):
    tx_n, ty_n = tile_grid(w, h)
    out = np.zeros((ty_n, tx_n))
    for ty in range(ty_n):
        for tx in range(tx_n):
            a, inside = [0.0] * 1024, 0
            for j in range(1024):
                x, y = 32 * tx + (j & 31), 32 * ty + (j >> 5)
                if x < w and y < h:
                    inside += 1
                    c = [float(t) for t in rgb[y][x]]
                    yy = (c[0] + c[1]) + c[2]
                    den = yy * yy + floor * floor
                    a[j] = float(var[y][x]) / den                               # (floor > 0: den is never 0.0)
            s = 512
            while s >= 1:
                for j in range(s):
                    a[j] = a[j] + a[j + s]
                s //= 2
            out[ty, tx] = a[0] / float(inside)
    return out


@pytest.mark.parametrize("w,h", [(5, 3), (33, 17), (70, 40)])
def test_plane_errors_equal_the_definition_slot_by_slot(w, h):
    rng = np.random.default_rng(w * h)
    rgb, var = rng.uniform(0.0, 2.0, (h, w, 3)), rng.uniform(0.0, 0.1, (h, w))
    if w > 5:
        rgb[3, 4, 1], var[5, 6], var[2, 2], rgb[1, 33 % w, 0] = NAN, INF, 0.0, INF
    with np.errstate(all="ignore"):
        want = scalar_plane_errors(rgb.tolist(), var.tolist(), w, h, 0.05)
    assert same(tar.plane_tile_errors(rgb, var, 0.05), want)
    tx, ty = tile_grid(w, h)
    for tiles in ([0], [tx * ty - 1], list(range(0, tx * ty, 2)), [tx * ty, 0], []):
        got = tar.plane_tile_errors(rgb, var, 0.05, tiles=tiles, fill=SENTINEL)
        for t in range(tx * ty):
            assert same(got.reshape(-1)[t:t + 1], (want.reshape(-1)[t:t + 1] if t in tiles else np.array([SENTINEL]))), (tiles, t)


@pytest.mark.parametrize("w,h", [(5, 3), (33, 17), (96, 64)])
def test_plane_errors_of_the_buffers_mean_are_the_buffers_tile_errors(w, h):
    rng = np.random.default_rng(w + h)
    buf = RefBuffer(w, h)
    for _ in range(2):
        buf.add(rng.uniform(0.0, 1.5, (h, w, 3)))
    tx, ty = tile_grid(w, h)
    target = [(5, 3, 2)[t % 3] for t in range(tx * ty)]                            # 2, 3 and 5 batches per tile
    for r in range(3):
        buf.add_tiles(rng.uniform(0.0, 1.5, (h, w, 3)), [t for t in range(tx * ty) if target[t] - 2 > r])
    assert buf.tile_batches().reshape(-1).tolist() == target
    mean, var = buf.mean()
    assert same(tar.plane_tile_errors(mean, var, 0.07), buf.tile_errors(0.07))


def test_selection_among_a_list_keeps_the_lists_order():
    err = np.array([[0.1, 0.01, NAN], [0.3, 0.0625, 0.07]])
    counts = np.array([[2, 2, 2], [8, 3, 7]], dtype=np.uint32)
    assert tar.select_among(err, counts, 0.25, 8).tolist() == select(err, counts, 0.25, 8).tolist() == [0, 5]
    assert tar.select_among(err, counts, 0.25, 8, [5, 4, 3, 2, 0]).tolist() == [5, 0]
    assert tar.select_among(err, counts, 0.25, 8, [1, 2, 9]).tolist() == []
    assert tar.select_among(err, counts, 0.25, 8, []).dtype == np.uint32


# ---- 3: the loop on random batches
def noisy_batches(seed, w, h, sigma_by_tile):
    """batch_at(offset): a fixed picture plus noise whose width differs from tile to tile, a function of the offset alone."""
    base = np.random.default_rng(seed).uniform(0.2, 1.0, (h, w, 3))
    tx, ty = tile_grid(w, h)
    sig = np.repeat(np.repeat(np.asarray(sigma_by_tile, dtype=np.float64).reshape(ty, tx), 32, axis=0), 32, axis=1)[:h, :w]

    @functools.lru_cache(maxsize=None)
    def batch_at(offset):
        b = base + np.random.default_rng(1000 * seed + offset).normal(size=(h, w, 3)) * sig[..., None]
        b.setflags(write=False)
        return b
    return batch_at


W, H = 70, 40                                                                    # 3 x 2 tiles, the right and bottom ones partial
SIGMAS = [0.02, 0.2, 0.6, 0.05, 0.4, 0.1]
LOOP = dict(spp_per_batch=2, min_batches=2, max_batches=8, threshold=0.06, floor=0.05)


def planes_for_loop(seed):
    rec, _, _, normal, depth = garbage_clip(seed, W, H, records(1, moving=False))[0]
    depth = depth.copy()
    depth[..., 1] = 1.0                                                          # every pixel a hit
    depth[..., 2] = 1.0
    return rec, normal, depth


def test_loop_without_history_is_the_plain_adaptive_loop():
    batch_at = noisy_batches(3, W, H, SIGMAS)
    rec, normal, depth = planes_for_loop(1)
    buf, stats, last, lists = tar.adaptive_temporal_loop(batch_at, W, H, ClipRef(W, H), rec, None, depth, normal_tol=0.0, **LOOP)
    want, want_stats = tar.plain_adaptive_loop(batch_at, W, H, **LOOP)
    assert stats == want_stats
    assert same(buf.total, want.total) and same(buf.sumsq, want.sumsq) and same(buf.tile_batches(), want.tile_batches())
    counts = buf.tile_batches().reshape(-1)
    assert counts.min() == 2 and counts.max() == 8 and len(set(counts.tolist())) >= 3   # tiles stop early, late and never
    assert all(set(b.tolist()) <= set(a.tolist()) for a, b in zip(lists, lists[1:]))    # the active list only shrinks


@pytest.mark.parametrize("flags", [MATCH_ID, 0])
def test_accumulation_behind_the_loop_is_every_tiles_last_preview(flags):
    rec, normal, depth = planes_for_loop(2)
    ref = ClipRef(W, H)
    kw = dict(flags=flags, normal_tol=0.0, max_history=16)
    totals = []
    for f in range(4):
        batch_at = noisy_batches(10 + f, W, H, SIGMAS)
        before = copy.deepcopy(ref)
        buf, stats, last, lists = tar.adaptive_temporal_loop(batch_at, W, H, ref, rec, None, depth, sample_offset=16 * f, **kw, **LOOP)
        assert ref.frames == before.frames == f
        mean, var = buf.mean()
        after_loop = tar.preview(ref, rec, mean, var, None, depth, **kw)
        got = ref.accumulate(rec, mean, var, None, depth, **kw)
        counts = buf.counts()
        stopped = counts < LOOP["max_batches"]
        assert stopped.any()
        for a, b, c in zip(got, last, after_loop):
            assert same(a[stopped], b[stopped]) and same(a, c)
        totals.append(stats[1])
    # history carries the later frames: they render fewer tile-batches
    assert all(t <= totals[0] for t in totals[1:]) and sum(totals) < 4 * totals[0], totals


# ---- 4: what the C ABI refuses before any device call (handles are NULL or a scene that was never committed)
def _scene_cam_prm(w=80, h=72, shard_count=1):
    lib = _lib.load()
    s = lib.rpt_scene_create()
    cam = _lib.CameraDesc((0.0, 0.0, 10.0), (0.0, 0.0, -1.0), (0.0, 1.0, 0.0), 0.5, 0.0, 1.0)
    prm = _lib.RenderParams(w, h, 0.0, 2, 0, shard_count)
    return lib, s, cam, prm


def test_preview_checks_are_the_accumulations_and_precede_every_device_call():
    lib = _lib.load()
    cam = _lib.CameraDesc((0.0, 0.0, 10.0), (0.0, 0.0, -1.0), (0.0, 1.0, 0.0), 0.5, 0.0, 1.0)
    planes = [np.zeros(16) for _ in range(8)]
    rgb, var, normal, depth, tiles, out, out_v, out_len = [p.ctypes.data_as(C.c_void_p) for p in planes]
    T = _lib.TemporalParams

    def both(text, prm, cam_, args_acc):
        """the refusal of the accumulation is the preview's, with the list in order"""
        a = list(args_acc)
        p = C.byref(prm) if prm is not None else None
        c = C.byref(cam_) if cam_ is not None else None
        assert lib.rpt_temporal_accumulate_device(None, p, c, *a, None) == -1
        first = lib.rpt_last_error()
        assert text in first, first
        assert lib.rpt_temporal_preview_device(None, p, c, *a[:4], tiles, 1, *a[4:], None) == -1
        assert lib.rpt_last_error() == first

    ok = T(16, 1, 0.1, 0.5)
    full = (rgb, var, normal, depth, out, out_v, out_len)
    both(b"null temporal", None, cam, full)
    both(b"max_history", T(0, 1, 0.1, 0.5), cam, full)
    both(b"flag", T(16, 4, 0.1, 0.5), cam, full)
    both(b"tolerance", T(16, 1, -0.1, 0.5), cam, full)
    both(b"null camera", ok, None, full)
    both(b"null frame", ok, cam, (None, var, normal, depth, out, out_v, out_len))
    both(b"null frame", ok, cam, (rgb, var, normal, depth, None, out_v, out_len))
    both(b"depth plane", ok, cam, (rgb, var, normal, None, out, out_v, out_len))
    both(b"needs the normal", ok, cam, (rgb, var, None, depth, out, out_v, out_len))
    both(b"takes no normal", T(16, 1, 0.1, 0.0), cam, full)
    both(b"must not be one of the inputs", ok, cam, (rgb, var, normal, depth, rgb, out_v, out_len))
    both(b"outputs must differ", ok, cam, (rgb, var, normal, depth, out, out, out_len))
    both(b"null accumulator", ok, cam, full)
    both(b"RPT_TEMPORAL_CLIP", T(16, 3, 0.1, 0.5), cam, full)
    # the list: NULL with a count is refused behind the planes and before the handle; NULL with 0 and a list with 0 are lists
    assert lib.rpt_temporal_preview_device(None, C.byref(ok), C.byref(cam), rgb, var, normal, depth, None, 3, out, out_v, out_len, None) == -1
    assert b"null tile list" in lib.rpt_last_error()
    assert lib.rpt_temporal_preview_device(None, C.byref(ok), C.byref(cam), rgb, var, normal, depth, None, 3, out, out, out_len, None) == -1
    assert b"outputs must differ" in lib.rpt_last_error()
    for tl, n in ((None, 0), (tiles, 0)):
        assert lib.rpt_temporal_preview_device(None, C.byref(ok), C.byref(cam), rgb, var, normal, depth, tl, n, out, out_v, out_len, None) == -1
        assert b"null accumulator" in lib.rpt_last_error()
    assert not any(p.any() for p in planes)


def test_tile_error_checks_precede_every_device_call():
    lib = _lib.load()
    buf = np.zeros(16)
    p = buf.ctypes.data_as(C.c_void_p)
    for floor, text in ((0.0, b"floor"), (-1.0, b"floor"), (NAN, b"floor"), (INF, b"floor"), (0.1, b"null argument")):
        assert lib.rpt_temporal_tile_errors_device(None, p, p, floor, p, 1, p, None) == -1 and text in lib.rpt_last_error()
    assert not buf.any()


def test_loop_checks_precede_every_device_call():
    lib, s, cam, prm = _scene_cam_prm()
    try:
        P, T = _lib.AdaptiveParams, _lib.TemporalParams
        stats = (C.c_uint64 * 4)(9, 9, 9, 9)
        plane = np.zeros(16)
        d = plane.ctypes.data_as(C.c_void_p)
        ok_a, ok_t = P(4, 2, 4, 0, 0.1, 0.1), T(16, 1, 0.1, 0.5)

        def call(s_=s, cam_=cam, prm_=prm, a=ok_a, offset=0, t=ok_t, normal=d, depth=d):
            return lib.rpt_render_adaptive_temporal(s_, C.byref(cam_) if cam_ is not None else None, C.byref(prm_) if prm_ is not None else None,
                                                    C.byref(a) if a is not None else None, 1, offset, None, None,
                                                    C.byref(t) if t is not None else None, normal, depth, stats)

        def err(text, **kw):
            assert call(**kw) == -1
            assert text in lib.rpt_last_error(), lib.rpt_last_error()

        err(b"null argument", s_=None)
        err(b"null argument", cam_=None)
        err(b"null argument", prm_=None)
        err(b"null adaptive", a=None)
        err(b"spp_per_batch", a=P(0, 2, 4, 0, 0.1, 0.1))
        err(b"min_batches", a=P(4, 1, 4, 0, 0.1, 0.1))
        err(b"max_batches", a=P(4, 3, 2, 0, 0.1, 0.1))
        err(b"32 bits", a=P(1 << 20, 2, 1 << 13, 0, 0.1, 0.1))
        err(b"threshold", a=P(4, 2, 4, 0, NAN, 0.1))
        err(b"floor", a=P(4, 2, 4, 0, 0.1, 0.0))
        err(b"sample_offset", offset=0xFFFFFFFF - 15)                     # 16 samples from there do not fit
        err(b"sharded", prm_=_lib.RenderParams(80, 72, 0.0, 2, 0, 2))
        err(b"null buffer")                                                # ... and with a buffer the temporal checks follow (device tests)
        assert call(offset=0xFFFFFFFF - 16) == -1 and b"null buffer" in lib.rpt_last_error()
        assert list(stats) == [9, 9, 9, 9] and not plane.any()
    finally:
        lib.rpt_scene_destroy(s)


def test_python_wrappers_refuse_before_the_device():
    r = Renderer(Scene(), Camera()).width(80).height(72)
    p = AdaptiveParams(spp_per_batch=2, min_batches=2, max_batches=8)
    with pytest.raises(ValueError, match="AdaptiveParams"):
        r.sample_adaptive_temporal(TemporalParams(), None, None, {})
    with pytest.raises(ValueError, match="DeviceBuffer"):
        r.sample_adaptive_temporal(p, None, None, {})
    with pytest.raises(ValueError, match="AdaptiveParams"):
        r.render_sequence([Camera()], adaptive=TemporalParams())
    with pytest.raises(ValueError, match="return_tile_batches"):
        r.render_sequence([Camera()], return_tile_batches=True)
    with pytest.raises(ValueError, match="32 bits"):
        r.render_sequence([Camera()] * 3, adaptive=AdaptiveParams(spp_per_batch=1 << 16, min_batches=2, max_batches=1 << 15))
    with pytest.raises(ValueError, match="sharded"):
        Renderer(Scene(), Camera()).width(80).height(72).shard(0, 2).render_sequence([Camera()], adaptive=p)
    # num_samples and batches are not read with adaptive: num_samples(1) < batches is no refusal (a generator: nothing runs yet)
    assert r.num_samples(1).render_sequence([Camera()], adaptive=p) is not None
    with pytest.raises(ValueError, match="num_samples"):
        r.render_sequence([Camera()])


# ---- 5: the conditions on the oracle's renders (the device test asserts them on its own frames with the same settings)
def test_quality_conditions_on_the_oracles_renders():
    from oracle import pyoracle
    from rpt_amd import scenes, temporal_camera_record
    w, h = tar.QUALITY_W, tar.QUALITY_H
    scene, cam, cfg = getattr(scenes, tar.QUALITY_SCENE)(0)
    osc = pyoracle.OracleScene(scene)
    rec = temporal_camera_record(cam)
    batch_at, planes_at = tar.oracle_frame_inputs(osc, cam, cfg["max_bounces"], w, h, tar.QUALITY_SEED, tar.QUALITY_LOOP["spp_per_batch"],
                                                  tar.QUALITY_LOOP["min_batches"])
    ref, counts = ClipRef(w, h), []
    for f in range(tar.QUALITY_FRAMES + 1):
        if f == tar.QUALITY_FRAMES:
            ref.reset()
        normal, depth = planes_at(tar.frame_offset(f))
        buf, stats, _, _ = tar.adaptive_temporal_loop(batch_at, w, h, ref, rec, normal, depth, sample_offset=tar.frame_offset(f), **tar.QUALITY_LOOP)
        mean, var = buf.mean()
        ref.accumulate(rec, mean, var, normal, depth)
        counts.append(buf.tile_batches())
        assert stats[1] == int(buf.tile_batches().sum())
    plain = [tar.plain_adaptive_loop(batch_at, w, h, sample_offset=tar.frame_offset(f), **tar.QUALITY_LOOP)[0].tile_batches()
             for f in (0, tar.QUALITY_FRAMES)]
    totals = tar.check_conditions(counts[:-1], plain[0], counts[-1], plain[1])
    print(f"{tar.QUALITY_SCENE}(0) at {w} x {h}, oracle: tile batches per frame {[c.reshape(-1).tolist() for c in counts]}, totals {totals}")
    assert counts[0].reshape(-1).tolist() == [2, 3, 2, 8, 6, 8]                  # the counts DESIGN.md records
