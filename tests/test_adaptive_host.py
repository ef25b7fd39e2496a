"""Adaptive sampling by tile, the parts that need no GPU: the numpy restatement (tests/adaptive_ref.py) against a slot-by-slot
transcription of the definition in include/rpt_hip.h and on inputs where the definition is exact, the selection rule, the argument
checks of the new entry points that precede every device call, and the Python wrappers' refusals.

(RPT_ERR_STATE of rpt_render_adaptive -- a buffer that is not empty -- and the buffer's own checks need an rpt_buffer, which only a
device can hold: tests/test_gpu_adaptive.py.)"""
import ctypes as C
import math
from fractions import Fraction

import numpy as np
import pytest

from rpt_amd import AdaptiveParams, Camera, DenoiseParams, Renderer, Scene, _lib
from tests.adaptive_ref import RefBuffer, select, tile_errors, tile_grid

NAN, INF = float("nan"), float("inf")


def same(a, b):
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def random_buffer(seed, w, h, radius=0):
    """Batches on a grid of 2^-10 (the squares and the running sums are exact); the tiles end with 2, 3 and 5 batches side by side."""
    rng = np.random.default_rng(seed)
    buf = RefBuffer(w, h, radius)
    tx, ty = tile_grid(w, h)
    batch = lambda: rng.integers(0, 2048, (h, w, 3)) / 1024.0  # noqa: E731
    buf.add(batch())
    buf.add(batch())
    ids = np.arange(tx * ty)
    buf.add_tiles(batch(), ids[ids % 3 != 0][::-1])            # 3 batches, listed in descending order
    for _ in range(2):
        buf.add_tiles(batch(), ids[ids % 3 == 2])              # 5 batches
    return buf


def scalar_tile_errors(total, sumsq, counts, w, h, floor):
    """The definition, one slot and one Python float operation at a time."""
    tx_n, ty_n = tile_grid(w, h)
    out = [[None] * tx_n for _ in range(ty_n)]
    for ty in range(ty_n):
        for tx in range(tx_n):
            n = float(int(counts[ty][tx]))
            a, inside = [0.0] * 1024, 0
            for ry in range(32):
                for rx in range(32):
                    x, y = 32 * tx + rx, 32 * ty + ry
                    if x >= w or y >= h:
                        continue
                    inside += 1
                    m = [total[y][x][k] / n for k in range(3)]
                    ss = sumsq[y][x] - n * ((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2])
                    v = (ss if ss > 0.0 else 0.0) / (n - 1.0) / n      # fmax(ss, 0.0): 0.0 for a NaN ss as well
                    yy = (m[0] + m[1]) + m[2]
                    a[32 * ry + rx] = v / (yy * yy + floor * floor)
            s = 512
            while s >= 1:
                for j in range(s):
                    a[j] = a[j] + a[j + s]
                s //= 2
            out[ty][tx] = a[0] / float(inside)
    return np.array(out, dtype=np.float64)


@pytest.mark.parametrize("w,h", [(1, 1), (33, 33), (80, 72)])
def test_restatement_equals_the_definition_slot_by_slot(w, h):
    """1 x 1: one slot of 1024; 33 x 33: tiles of 32 x 32, 1 x 32, 32 x 1 and 1 x 1 pixels; 80 x 72: both edges clipped."""
    buf = random_buffer(w, w, h)
    counts = buf.tile_batches()
    tx, ty = tile_grid(w, h)
    assert counts.shape == (ty, tx) and (w == 1 or set(counts.reshape(-1).tolist()) == {2, 3, 5})
    for floor in (0.05, 1.0):
        got = buf.tile_errors(floor)
        want = scalar_tile_errors(buf.total.tolist(), buf.sumsq.tolist(), counts.tolist(), w, h, floor)
        assert same(got, want) and np.isfinite(got).all() and (got >= 0).all()
    assert (buf.tile_errors(0.05) > 0).any() or w == 1
    # the per-pixel mean and the variance of it with the pixel's own count
    rgb, var = buf.mean()
    n = buf.counts()
    for (x, y) in [(0, 0), (w - 1, h - 1), (w // 2, h // 2), (min(32, w - 1), 0), (0, min(32, h - 1))]:
        fn = float(n[y, x])
        m = [buf.total[y, x, k] / fn for k in range(3)]
        ss = buf.sumsq[y, x] - fn * ((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2])
        assert rgb[y, x].tolist() == m and var[y, x] == max(ss, 0.0) / (fn - 1.0) / fn


@pytest.mark.parametrize("radius", [0, 1, 2])
def test_restated_image_is_the_reference_s_window(radius):
    """get_filtered_color of src/buffer.rs:75-93 with a Vec per pixel: the window's samples summed, over their number."""
    w, h = 37, 40
    buf = random_buffer(7 + radius, w, h, radius)
    n = buf.counts()
    assert len(np.unique(n)) == 3
    f = buf.filtered()
    for (x, y) in [(0, 0), (36, 39), (31, 31), (32, 32), (33, 30), (5, 33), (36, 0)]:
        acc, count = [0.0, 0.0, 0.0], 0
        for i in range(max(x - radius, 0), x + radius + 1):
            for j in range(max(y - radius, 0), y + radius + 1):
                if i < w and j < h:
                    acc = [acc[k] + buf.total[j, i, k] for k in range(3)]
                    count += int(n[j, i])
        assert f[y, x].tolist() == [acc[k] / float(count) for k in range(3)]
    assert buf.image().shape == (h, w, 3) and buf.image().dtype == np.uint8


def test_exact_inputs():
    # a constant frame: every batch the same colour, v = 0, E = 0 whatever the counts
    buf = RefBuffer(80, 72)
    frame = np.full((72, 80, 3), 0.375)
    for _ in range(3):
        buf.add(frame)
    buf.add_tiles(frame, [0, 4, 8])
    e = buf.tile_errors(0.25)
    assert e.shape == (3, 3) and np.array_equal(e, np.zeros((3, 3))) and not np.signbit(e).any()
    # one tile of two-valued batches: two batches, grey a in the first and grey b in the second, the same for every pixel.
    # m = (a + b) / 2 per channel, sumsq = 3 (a^2 + b^2), ss = sumsq - 2 * 3 m^2 = 3 (a - b)^2 / 2, v = ss / 1 / 2, y = 3 m:
    # all exact in binary for a = 1/2, b = 1/4, and a_j is ONE rounded division, the same for the 1024 slots, so the tree sums are
    # a_j * 2^k, exact, and E = a_j * 1024 / 1024.
    a, b = Fraction(1, 2), Fraction(1, 4)
    buf = RefBuffer(32, 32)
    buf.add(np.full((32, 32, 3), float(a)))
    buf.add(np.full((32, 32, 3), float(b)))
    floor = Fraction(1, 8)
    m = (a + b) / 2
    v = (3 * (a * a + b * b) - 2 * 3 * m * m) / 1 / 2
    want = v / ((3 * m) ** 2 + floor * floor)
    got = buf.tile_errors(float(floor))
    assert got.shape == (1, 1) and got[0, 0] == float(want)            # float(Fraction) rounds once, as the division does
    assert float(v) == 3 * (0.25 ** 2) / 4
    # half the tile in the image: the same a_j in 512 slots, +0.0 in the others, over 512 pixels
    half = RefBuffer(32, 16)
    half.add(np.full((16, 32, 3), float(a)))
    half.add(np.full((16, 32, 3), float(b)))
    assert half.tile_errors(float(floor))[0, 0] == float(want)


def test_selection():
    err = np.array([[0.25, 0.0625, 0.5], [NAN, 1.0, 0.0626], [INF, 0.0, 0.0625000001]])
    counts = np.array([[4, 4, 4], [4, 8, 4], [4, 4, 7]], dtype=np.uint32)
    # E == threshold^2 is not selected (0.25^2 = 0.0625 exactly); NaN is not; +inf is; ids ascend
    assert select(err, counts, 0.25, 16).tolist() == [0, 2, 4, 5, 6, 8]
    assert select(err, counts, 0.25, 8).tolist() == [0, 2, 5, 6, 8]           # the cap: tile 4 holds max_batches
    assert select(err, counts, 0.25, 7).tolist() == [0, 2, 5, 6]
    assert select(err, counts, 0.25, 4).tolist() == []
    assert select(err, counts, 0.0, 16).tolist() == [0, 1, 2, 4, 5, 6, 8]     # 0 > 0 is false: a tile without noise is done
    assert select(err, counts, INF, 16).tolist() == []
    assert select(err, counts, 0.5, 16).tolist() == [2, 4, 6]
    assert select(err, counts, 0.25, 16).dtype == np.uint32


# ---- the C ABI's checks
def _scene_cam_prm(shard_count=1, w=80, h=72):
    lib = _lib.load()
    s = lib.rpt_scene_create()                                  # never committed: no device is touched
    cam = _lib.CameraDesc((0.0, 0.0, 10.0), (0.0, 0.0, -1.0), (0.0, 1.0, 0.0), 0.5, 0.0, 1.0)
    prm = _lib.RenderParams(w, h, 0.0, 2, 0, shard_count)
    return lib, s, cam, prm


@pytest.mark.parametrize("device", [False, True])
def test_tile_list_render_checks_precede_every_device_call(device):
    lib, s, cam, prm = _scene_cam_prm()
    try:
        out = np.zeros((72, 80, 3))
        tiles = np.array([0, 4, 8], dtype=np.uint32)
        fn = lib.rpt_render_sample_tiles_device if device else lib.rpt_render_sample_tiles

        def call(s_, cam_, prm_, it, tl, n, o):
            args = [s_, C.byref(cam_) if cam_ is not None else None, C.byref(prm_) if prm_ is not None else None, it, 1, 0,
                    tl.ctypes.data_as(C.c_void_p) if tl is not None else None, n, o.ctypes.data_as(C.c_void_p) if o is not None else None]
            return fn(*args, None) if device else fn(*args)

        def err(text, *a):
            assert call(*a) == -1
            assert text in lib.rpt_last_error(), lib.rpt_last_error()

        err(b"null", None, cam, prm, 4, tiles, 3, out)
        err(b"null", s, None, prm, 4, tiles, 3, out)
        err(b"null", s, cam, None, 4, tiles, 3, out)
        err(b"null output", s, cam, prm, 4, tiles, 3, None)
        err(b"null tile list", s, cam, prm, 4, None, 3, out)
        err(b"empty", s, cam, prm, 0, tiles, 3, out)
        err(b"empty", s, cam, _lib.RenderParams(0, 72, 0.0, 2, 0, 1), 4, tiles, 3, out)
        err(b"sharded", s, cam, _lib.RenderParams(80, 72, 0.0, 2, 0, 2), 4, tiles, 3, out)
        err(b"sharded", s, cam, _lib.RenderParams(80, 72, 0.0, 2, 1, 2), 4, tiles, 0, out)
        err(b"more tiles", s, cam, prm, 4, np.arange(10, dtype=np.uint32), 10, out)
        if not device:                                          # a host list is checked, a device list is trusted
            err(b"out of range", s, cam, prm, 4, np.array([0, 9], dtype=np.uint32), 2, out)
            err(b"out of range", s, cam, prm, 4, np.array([0xFFFFFFFF], dtype=np.uint32), 1, out)
            err(b"twice", s, cam, prm, 4, np.array([3, 5, 3], dtype=np.uint32), 3, out)
        # everything in order: the next refusal is the scene's state (RPT_ERR_STATE), also for an empty list
        assert call(s, cam, prm, 4, tiles, 3, out) == -2 and b"commit" in lib.rpt_last_error()
        assert call(s, cam, prm, 4, None, 0, out) == -2
        assert not out.any()
    finally:
        lib.rpt_scene_destroy(s)


def test_adaptive_parameter_checks_precede_every_device_call():
    lib, s, cam, prm = _scene_cam_prm()
    try:
        P = _lib.AdaptiveParams
        n = C.c_uint32(77)
        buf = np.zeros(16)
        p = buf.ctypes.data_as(C.c_void_p)
        stats = (C.c_uint64 * 4)()

        def err(text, prm_a):
            a = C.byref(prm_a) if prm_a is not None else None
            assert lib.rpt_buffer_refine_tiles(None, a, p, C.byref(n), None, None) == -1
            assert text in lib.rpt_last_error(), lib.rpt_last_error()
            assert lib.rpt_render_adaptive(s, C.byref(cam), C.byref(prm), a, 1, None, stats) == -1
            assert text in lib.rpt_last_error(), lib.rpt_last_error()

        err(b"null adaptive", None)
        err(b"spp_per_batch", P(0, 2, 4, 0, 0.1, 0.1))
        err(b"min_batches", P(4, 1, 4, 0, 0.1, 0.1))
        err(b"min_batches", P(4, 0, 4, 0, 0.1, 0.1))
        err(b"max_batches", P(4, 3, 2, 0, 0.1, 0.1))
        err(b"32 bits", P(1 << 20, 2, 1 << 13, 0, 0.1, 0.1))
        err(b"threshold", P(4, 2, 4, 0, -0.1, 0.1))
        err(b"threshold", P(4, 2, 4, 0, NAN, 0.1))
        err(b"floor", P(4, 2, 4, 0, 0.1, 0.0))
        err(b"floor", P(4, 2, 4, 0, 0.1, -1.0))
        err(b"floor", P(4, 2, 4, 0, 0.1, NAN))
        err(b"floor", P(4, 2, 4, 0, 0.1, INF))
        # parameters in order (+inf and 0 are thresholds): the next refusal is the handle
        for ok in (P(4, 2, 2, 0, INF, 0.1), P(1, 2, 9, 0, 0.0, 1e-3)):
            err(b"null", ok)
        assert n.value == 77
        ok = P(4, 2, 4, 0, 0.1, 0.1)
        assert lib.rpt_render_adaptive(None, C.byref(cam), C.byref(prm), C.byref(ok), 1, None, stats) == -1 and b"null" in lib.rpt_last_error()
        sharded = _lib.RenderParams(80, 72, 0.0, 2, 0, 2)
        assert lib.rpt_render_adaptive(s, C.byref(cam), C.byref(sharded), C.byref(ok), 1, None, stats) == -1
        assert b"sharded" in lib.rpt_last_error()
        # the buffer's entry points
        for floor, text in ((0.0, b"floor"), (-1.0, b"floor"), (NAN, b"floor"), (0.1, b"null")):
            assert lib.rpt_buffer_tile_errors_device(None, floor, p, None) == -1 and text in lib.rpt_last_error()
        assert lib.rpt_buffer_add_samples_tiles_device(None, p, p, 1, None) == -1 and b"null" in lib.rpt_last_error()
        assert lib.rpt_buffer_tile_batches(None, p, 16) == -1 and b"null" in lib.rpt_last_error()
    finally:
        lib.rpt_scene_destroy(s)


def test_python_wrappers_refuse_before_the_device():
    p = AdaptiveParams()
    d = p.desc()
    assert (d.spp_per_batch, d.min_batches, d.max_batches, d.threshold, d.floor) == (4, 4, 16, 0.05, 0.05)
    assert AdaptiveParams(threshold=INF).threshold == INF and AdaptiveParams(threshold=0).threshold == 0.0
    for bad in (dict(spp_per_batch=0), dict(min_batches=1), dict(min_batches=5, max_batches=4), dict(threshold=-1.0), dict(threshold=NAN),
                dict(floor=0.0), dict(floor=-2.0), dict(floor=NAN), dict(floor=INF), dict(spp_per_batch=1 << 20, max_batches=1 << 12)):
        with pytest.raises(ValueError):
            AdaptiveParams(**bad)
    r = Renderer(Scene(), Camera()).width(80).height(72)
    out = np.zeros((72, 80, 3))
    with pytest.raises(ValueError, match="outside"):
        r.sample_tiles_array(4, [0, 9], out)
    with pytest.raises(ValueError, match="outside"):
        r.sample_tiles_array(4, [-1], out)
    with pytest.raises(ValueError, match="twice"):
        r.sample_tiles_array(4, [2, 2], out)
    with pytest.raises(ValueError, match="out must be"):
        r.sample_tiles_array(4, [2], np.zeros((72, 80, 3), dtype=np.float32))
    with pytest.raises(ValueError, match="out must be"):
        r.sample_tiles_array(4, [2], np.zeros((72, 81, 3)))
    with pytest.raises(ValueError, match="out must be"):
        r.sample_tiles_array(4, [2], np.zeros((72, 80, 6))[..., ::2])
    with pytest.raises(ValueError, match="tiles listed"):
        r.sample_tiles_device(4, 1 << 20, 10, 1 << 21)
    with pytest.raises(ValueError, match="null"):
        r.sample_tiles_device(4, 0, 3, 1 << 21)
    with pytest.raises(ValueError, match="null"):
        r.sample_tiles_device(4, 1 << 20, 3, 0)
    sharded = Renderer(Scene(), Camera()).width(80).height(72).shard(0, 2)
    with pytest.raises(ValueError, match="sharded"):
        sharded.sample_tiles_array(4, [0], out)
    with pytest.raises(ValueError, match="sharded"):
        sharded.sample_tiles_device(4, 1 << 20, 1, 1 << 21)
    with pytest.raises(ValueError, match="sharded"):
        sharded.render_adaptive(p)
    with pytest.raises(ValueError, match="AdaptiveParams"):
        r.render_adaptive(DenoiseParams())
    with pytest.raises(ValueError, match="DenoiseParams"):
        r.render_adaptive(p, denoise=p)
    assert not out.any()
