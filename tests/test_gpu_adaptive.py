"""Adaptive sampling by tile on the device: tile-list renders against the full render, the buffer whose tiles hold different numbers
of batches and its tile errors and selection against the numpy restatement (tests/adaptive_ref.py), and the loop.  Equality is bit
for bit unless a test says otherwise.

Frames are 80 x 72: 3 x 3 tiles of 32 x 32 with the right and the bottom ones clipped.  Buffers are fed batches on a grid of 2^-10,
whose squares and running sums are exact, so that the buffer's sums do not depend on how buffer_add_kernel's expression is contracted
(tests/test_gpu_denoise.py does the same); what a tile batch of a RENDERED frame puts into a pixel is compared with what a full-frame
batch puts there, device against device, in the loop's tests."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

from rpt_amd import (AdaptiveParams, Camera, DenoiseParams, DeviceBuffer, Environment, Filter, Light, Material, Object, Renderer, RptError,
                     Scene, _lib, scenes, sphere, vec3)
from tests.adaptive_ref import RefBuffer, select, tile_grid

pytestmark = pytest.mark.gpu

W, H, SEED = 80, 72, 0xADA97
SENTINEL = -7.25                                                # no render writes a negative value
NAN, INF = float("nan"), float("inf")
LISTS = {"inner": [4], "corner": [8], "checker": [0, 2, 4, 6, 8], "descending": [8, 7, 6, 5, 4, 3, 2, 1, 0], "empty": []}


def torch():
    import torch as t
    return t


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(a, b):
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def tile_mask(tiles, w=W, h=H):
    tx_n, _ = tile_grid(w, h)
    m = np.zeros((h, w), dtype=bool)
    for t in tiles:
        ty, tx = divmod(int(t), tx_n)
        m[32 * ty:32 * ty + 32, 32 * tx:32 * tx + 32] = True
    return m


# ---- 1: tile-list renders
def _group_scene():
    from tests.test_gpu_features import _group_scene as g
    return g()


SCENES = {
    # name: (builder -> (scene, camera), reference-epsilon mode, options, samples)
    "cornell": (lambda: scenes.cornell()[:2], False, {}, 4),                                       # scan
    "lampshade": (lambda: scenes.lampshade()[:2], False, {}, 4),                                   # scan, in a medium
    "mesh": (lambda: scenes.mesh_in_fog(nu=32, nv=32)[:2], False, {}, 4),                          # C5-small: per-mesh trees
    "group": (_group_scene, False, {"scene_bvh_min": 4}, 8),                                       # a kd-tree group
    "fractal_spheres": (lambda: scenes.fractal_spheres(levels=2)[:2], False, {"scene_bvh_min": 4}, 4),   # the scene tree
    "cornell_f64": (lambda: scenes.cornell()[:2], True, {}, 4),
    "mesh_f64": (lambda: scenes.mesh_in_fog(nu=24, nv=24)[:2], True, {}, 4),                       # candidate tree
    # two blocks for 9 x 1024 x 3 items: every wave pulls many items; three chunks per pixel
    "cornell_capped": (lambda: scenes.cornell()[:2], False, {"max_blocks": 2, "chunk_spp": 2}, 6),
    "mesh_capped": (lambda: scenes.mesh_in_fog(nu=32, nv=32)[:2], False, {"max_blocks": 2, "chunk_spp": 2}, 6),
}


@functools.lru_cache(maxsize=None)
def renderer(name):
    build, f64, options, spp = SCENES[name]
    scene, cam = build()
    for k, v in options.items():
        scene.set_option(k, v)
    if f64:
        scene.set_option("epsilon_policy", 1)
    mb = 3
    return Renderer(scene, cam).width(W).height(H).max_bounces(mb).seed(SEED), spp


@functools.lru_cache(maxsize=None)
def full_render(name):
    r, spp = renderer(name)
    r._sample_offset = 3
    out = r.sample_array(spp).reshape(H, W, 3)
    out.setflags(write=False)
    assert np.isfinite(out).all() and (out >= 0).all() and out.max() > 0
    return out


def check_tiles(got, full, tiles, what):
    m = tile_mask(tiles)
    bad_in = int((bits(got)[m] != bits(full)[m]).sum())
    bad_out = int((got[~m] != SENTINEL).sum())
    print(f"{what}: {bad_in} values of the listed tiles differ from the full render, {bad_out} outside them were written")
    assert bad_in == 0 and bad_out == 0, what


@pytest.mark.parametrize("name", list(SCENES))
def test_tile_list_render_equals_the_full_render_and_touches_nothing_else(name):
    r, spp = renderer(name)
    full = full_render(name)
    if "capped" in name:
        assert r.chunking(spp)[1] == 3
    for what, tiles in LISTS.items():
        out = np.full((H, W, 3), SENTINEL)
        r._sample_offset = 3
        assert r.sample_tiles_array(spp, tiles, out) is out and r._sample_offset == 3 + spp
        check_tiles(out, full, tiles, f"{name}, {what}")


@pytest.mark.parametrize("name", ["lampshade", "mesh_f64"])
def test_device_lists_on_two_alternating_streams(name):
    t = torch()
    r, spp = renderer(name)
    full = full_render(name)
    lists = [[0, 2, 4, 6, 8], [7, 5, 3, 1]]
    d_lists = [t.tensor(ls, dtype=t.int32, device="cuda") for ls in lists]
    outs = [t.full((H * W * 3,), SENTINEL, dtype=t.float64, device="cuda") for _ in lists]
    streams = [t.cuda.Stream(), t.cuda.Stream()]
    t.cuda.synchronize()
    for i in range(4):                                          # the second round overwrites the first with the same bits
        k = i % 2
        r._sample_offset = 3
        r.sample_tiles_device(spp, d_lists[k].data_ptr(), len(lists[k]), outs[k].data_ptr(), streams[k].cuda_stream)
    r._sample_offset = 3
    r.sample_tiles_device(spp, 0, 0, outs[0].data_ptr(), streams[0].cuda_stream)     # n_tiles = 0: nothing is launched
    t.cuda.synchronize()
    for k in range(2):
        check_tiles(outs[k].cpu().numpy().reshape(H, W, 3), full, lists[k], f"{name}, stream {k}")


# ---- 2: the buffer with extra batches
def grid_batches(seed, w, h, n):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 2048, (h, w, 3)) / 1024.0 for _ in range(n)]


def build_buffers(w, h, radius, batches, plan):
    """plan: per batch None (full frame) or a tile list -> (DeviceBuffer, RefBuffer) fed alike."""
    t = torch()
    dev, ref = DeviceBuffer(w, h, Filter.Box(radius)), RefBuffer(w, h, radius)
    keep = []
    for b, tiles in zip(batches, plan):
        if tiles is None:
            dev.add_samples(b.reshape(-1, 3))
            ref.add(b)
            continue
        d_b = t.from_numpy(b.reshape(-1).copy()).cuda()
        d_t = t.tensor([int(x) for x in tiles], dtype=t.int32, device="cuda")
        keep += [d_b, d_t]
        t.cuda.synchronize()
        dev.add_samples_tiles_device(d_b.data_ptr(), d_t.data_ptr() if len(tiles) else 0, len(tiles))
        ref.add_tiles(b, tiles)
    t.cuda.synchronize()
    return dev, ref


def plan_235(w, h):
    """Tiles end with 2, 3 and 5 batches side by side."""
    tx, ty = tile_grid(w, h)
    ids = np.arange(tx * ty)
    if ids.size == 2:                                           # two tiles: 3 and 5 batches
        return [None, None, [1, 0], [1], [1]]
    return [None, None, ids[ids % 3 != 0][::-1].tolist(), ids[ids % 3 == 2].tolist(), ids[ids % 3 == 2].tolist()]


@pytest.mark.parametrize("w,h,radius", [(80, 72, 0), (80, 72, 1), (37, 23, 0), (37, 23, 1), (37, 23, 2)])
def test_buffer_with_extra_batches_equals_the_restatement(w, h, radius):
    dev, ref = build_buffers(w, h, radius, grid_batches(w + radius, w, h, 5), plan_235(w, h))
    counts = dev.tile_batches()
    assert counts.dtype == np.uint32 and np.array_equal(counts, ref.tile_batches()) and dev.batches == 2
    assert set(counts.reshape(-1).tolist()) == ({2, 3, 5} if w == 80 else {3, 5})
    rgb, var = dev.mean()
    want_rgb, want_var = ref.mean()
    # (sum = mean * n is not read back; on the grid the sums are exact and n is the restatement's: equal means are equal sums)
    assert same(rgb, want_rgb) and same(var, want_var) and var.max() > 0
    v, want_v = dev.variance(), ref.variance()
    print(f"{w} x {h}, radius {radius}: variance {v!r} against {want_v!r}")
    assert abs(v - want_v) <= 1e-12 * want_v
    got, want = dev.image(), ref.image()
    diff = np.abs(got.astype(int) - want.astype(int))
    print(f"{w} x {h}, radius {radius}: {int((diff != 0).sum())} of {diff.size} bytes differ, by at most {int(diff.max())}")
    # the same fp64 sums in the same order; pow() may differ in the last ulp, i.e. a byte may flip at an exact boundary (tests/test_gpu_buffer.py)
    assert got.shape == want.shape == (h, w, 3) and (got != want).mean() < 1e-3 and diff.max() <= 1


def test_buffer_without_tile_batches_is_unchanged():
    """The same full-frame batches into two buffers, one of which also receives an empty tile list: the kernels of a buffer without extra
    batches, the same image, variance and mean."""
    w, h = 37, 23
    batches = grid_batches(5, w, h, 3)
    a, ref = build_buffers(w, h, 1, batches, [None, None, None])
    b, _ = build_buffers(w, h, 1, batches + [batches[0]], [None, None, None, []])
    assert np.array_equal(a.tile_batches(), np.full((1, 2), 3)) and np.array_equal(b.tile_batches(), a.tile_batches())
    assert np.array_equal(a.image(), b.image()) and a.variance() == b.variance()
    assert all(same(x, y) for x, y in zip(a.mean(), b.mean())) and all(same(x, y) for x, y in zip(a.mean(), ref.mean()))
    with pytest.raises(ValueError, match="tiles listed"):
        a.add_samples_tiles_device(1 << 20, 1 << 21, 3)
    with pytest.raises(RptError, match="capacity"):
        out = np.zeros(1, dtype=np.uint32)
        _lib.check(_lib.load().rpt_buffer_tile_batches(a._h, out.ctypes.data_as(C.c_void_p), 1))


# ---- 3: tile errors and selection
def error_cases():
    cases = {}
    for (w, h) in [(80, 72), (37, 23), (1, 1)]:
        b = grid_batches(w, w, h, 5)
        cases[f"{w}x{h}"] = (w, h, b, plan_235(w, h) if w > 1 else [None, None, [0], None, [0]])
    b = grid_batches(9, W, H, 5)
    b[1][40, 50, 1] = NAN                                       # a NaN pixel in tile 4
    cases["nan"] = (W, H, b, plan_235(W, H))
    b = grid_batches(10, W, H, 5)
    for x in b:
        x[32:64, 0:32] = 0.0                                    # tile 3 all zero: v = 0, y = 0, a = 0 / floor^2
        x[0:32, 64:80] = 0.5                                    # tile 2 constant: E = 0 without being dark
    cases["zero"] = (W, H, b, plan_235(W, H))
    return cases


@pytest.mark.parametrize("name", ["80x72", "37x23", "1x1", "nan", "zero"])
def test_tile_errors_and_selection_equal_the_restatement(name):
    w, h, batches, plan = error_cases()[name]
    dev, ref = build_buffers(w, h, 0, batches, plan)
    counts = ref.tile_batches()
    for floor in (0.05, 1.0):
        got, want = dev.tile_errors(floor), ref.tile_errors(floor)
        bad = ~((got == want) | (np.isnan(got) & np.isnan(want)))
        print(f"{name}, floor {floor}: {int(bad.sum())} of {bad.size} tile errors differ; errors {want.reshape(-1).tolist()}")
        assert same(got, want)
    if name == "nan":
        assert np.isnan(want[1, 1]) and np.isfinite(np.delete(want.reshape(-1), 4)).all()
    if name == "zero":
        assert want[1, 0] == 0.0 and want[0, 2] == 0.0 and (np.delete(want.reshape(-1), [2, 3]) > 0).all()
    want = ref.tile_errors(0.05)
    finite = np.sort(want[np.isfinite(want) & (want > 0)])
    # thresholds below, between and above the tiles' errors (the comparison is with threshold * threshold, formed alike on both sides)
    thresholds = [0.0, math.sqrt(finite[0]) * 0.5, math.sqrt(finite[-1]) * 2.0, INF]
    thresholds += [math.sqrt(0.5 * (lo + hi)) for lo, hi in zip(finite[:-1], finite[1:])]
    thresholds += [math.sqrt(e) for e in finite[:2]]            # (about an error itself: either side, the same side on both)
    seen = set()
    for thr in thresholds:
        for cap in (9, 5, 3, 2):
            p = AdaptiveParams(spp_per_batch=1, min_batches=2, max_batches=cap, threshold=thr, floor=0.05)
            ids, err = dev.refine_tiles(p)
            expect = select(want, counts, thr, cap)
            assert ids.dtype == np.uint32 and np.array_equal(ids, expect), (thr, cap, ids, expect)
            assert same(err, want) and np.all(np.diff(ids.astype(np.int64)) > 0)
            seen.add(len(ids))
    assert 0 in seen and (w == 1 or len(seen) > 2)
    if name == "nan":
        assert 4 not in dev.refine_tiles(AdaptiveParams(1, 2, 9, 0.0, 0.05))[0]
    # fewer than two full-frame batches: RPT_ERR_STATE
    one, _ = build_buffers(w, h, 0, batches[:1], [None])
    with pytest.raises(RptError, match="2 full-frame"):
        one.tile_errors(0.05)
    with pytest.raises(RptError, match="2 full-frame"):
        one.refine_tiles(AdaptiveParams(1, 2, 9, 0.0, 0.05))
    with pytest.raises(ValueError, match="floor"):
        dev.tile_errors(0.0)


# ---- 4: the loop
LW = LH = 96
MIN_B, MAX_B, SPP_B, FLOOR = 2, 5, 2, 0.05
CORNERS = [0, 2, 6, 8]


def loop_scene():
    """Black environment, no medium, a diffuse sphere lit by a sphere light above it; the camera frames them so that at 96 x 96 the four
    corner tiles (and the left and right ones) see only the environment."""
    scene = Scene()
    scene.add(Object(sphere()).material(Material.diffuse(vec3(0.75, 0.5, 0.25))))
    lamp, glow = sphere().scale(vec3(0.3, 0.3, 0.3)).translate(vec3(0.0, 1.6, 0.5)), Material.light(vec3(1.0, 1.0, 1.0), 40.0)
    scene.add(Object(lamp.clone()).material(glow))              # a light is visible through its twin among the objects (scene.rs:57-75)
    scene.add(Light.Object(Object(lamp.clone()).material(glow)))
    scene.environment = Environment.Color(vec3(0.0, 0.0, 0.0))
    return scene, Camera(eye=vec3(0.0, 0.0, 10.0), direction=vec3(0.0, 0.0, -1.0), up=vec3(0.0, 1.0, 0.0), fov=1.0)


def loop_renderer(f64):
    scene, cam = loop_scene()
    if f64:
        scene.set_option("epsilon_policy", 1)
    return Renderer(scene, cam).width(LW).height(LH).max_bounces(3).seed(SEED)


@functools.lru_cache(maxsize=None)
def full_batches(f64):
    """k = MIN_B .. MAX_B full-frame batches -> {k: (mean, variance of the mean)}, and the restatement's tile errors after MIN_B."""
    r = loop_renderer(f64)
    buf, ref, out = DeviceBuffer(LW, LH), RefBuffer(LW, LH), {}
    for k in range(MAX_B):
        if k < MIN_B:                                           # the same frames into the restatement
            frame = r.sample_array(SPP_B)
            buf.add_samples(frame)
            ref.add(frame)
        else:
            r.sample(SPP_B, buf)
        if k + 1 >= MIN_B:
            out[k + 1] = buf.mean()
    for rgb, var in out.values():
        rgb.setflags(write=False)
        var.setflags(write=False)
    return out, ref.tile_errors(FLOOR)


def test_corner_tiles_see_only_the_black_environment():
    """Once, with the oracle on the CPU: every sample of a corner tile's pixels is exactly 0 for the seed used, in both modes' epsilon
    handling; a corner tile has E = 0 by construction.  The device agrees."""
    from oracle.pyoracle import OracleScene
    scene, cam = loop_scene()
    m = tile_mask(CORNERS, LW, LH)
    for robust in (1, 0):
        exp = OracleScene(scene).render(cam, LW, LH, MAX_B * SPP_B, 3, seed=SEED, robust=robust).reshape(LH, LW, 3)
        assert not exp[m].any() and exp[~m].max() > 0
    for f64 in (False, True):
        full, err = full_batches(f64)
        for rgb, var in full.values():
            assert not rgb[m].any() and not var[m].any()
        assert all(err.reshape(-1)[t] == 0.0 for t in CORNERS) and err[1, 1] > 0


def run_loop(f64, threshold):
    r, buf = loop_renderer(f64), DeviceBuffer(LW, LH)
    stats = r.sample_adaptive(AdaptiveParams(SPP_B, MIN_B, MAX_B, threshold, FLOOR), buf)
    return buf, stats


def check_against_full_batches(buf, stats, f64, what):
    full, _ = full_batches(f64)
    counts = buf.tile_batches()
    rgb, var = buf.mean()
    for t in range(9):
        n_t = int(counts.reshape(-1)[t])
        m = tile_mask([t], LW, LH)
        bad = int((bits(rgb)[m] != bits(full[n_t][0])[m]).sum()) + int((bits(var)[m] != bits(full[n_t][1])[m]).sum())
        print(f"{what}: tile {t} ended with {n_t} batches, {bad} values differ from {n_t} full-frame batches")
        assert bad == 0, (what, t)
    assert stats[3] == 9 and stats[1] == int(counts.sum()) and stats[2] == int((counts == MAX_B).sum())
    assert stats[0] == int(counts.max()) - MIN_B and buf.batches == MIN_B
    return counts


def test_loop_at_threshold_zero_and_infinity():
    full, _ = full_batches(False)
    buf, stats = run_loop(False, 0.0)
    counts = check_against_full_batches(buf, stats, False, "threshold 0")
    rgb, var = buf.mean()
    # a tile that stopped early had E = 0: here, all black (0 / n is 0 for every n), so the whole frame equals MAX_B full-frame batches
    assert same(rgb, full[MAX_B][0]) and same(var, full[MAX_B][1])
    assert counts[1, 1] == MAX_B and stats[0] == MAX_B - MIN_B and all(counts.reshape(-1)[t] == MIN_B for t in CORNERS)
    buf, stats = run_loop(False, INF)
    rgb, var = buf.mean()
    assert same(rgb, full[MIN_B][0]) and same(var, full[MIN_B][1])
    assert np.array_equal(buf.tile_batches(), np.full((3, 3), MIN_B)) and stats == (0, 9 * MIN_B, 0, 9)


@pytest.mark.parametrize("f64", [False, True])
def test_loop_between_the_corner_tiles_and_the_centre_tile(f64):
    _, err = full_batches(f64)
    e_centre = float(err[1, 1])
    assert e_centre > 0
    threshold = math.sqrt(e_centre) * 0.5                       # between the corner tiles' 0 and the centre tile's error after MIN_B
    buf, stats = run_loop(f64, threshold)
    counts = check_against_full_batches(buf, stats, f64, f"f64={f64}, threshold {threshold:.4f}")
    print(f"f64={f64}: centre error {e_centre:.6f} after {MIN_B} batches, tile batches {counts.reshape(-1).tolist()}, stats {stats}")
    assert all(counts.reshape(-1)[t] == MIN_B for t in CORNERS)   # the pair that keeps this test from passing vacuously
    assert counts[1, 1] > MIN_B
    # the buffer's read-outs work on unequal counts
    assert buf.image().shape == (LH, LW, 3) and np.isfinite(buf.variance())


def test_render_adaptive_returns_an_image_and_the_counts():
    _, err = full_batches(False)
    p = AdaptiveParams(SPP_B, MIN_B, MAX_B, math.sqrt(float(err[1, 1])) * 0.5, FLOOR)
    img, counts = loop_renderer(False).render_adaptive(p)
    assert img.shape == (LH, LW, 3) and img.dtype == np.uint8 and img.max() > 0
    assert counts.shape == (3, 3) and counts.min() == MIN_B and counts.max() > MIN_B
    den, counts2 = loop_renderer(False).render_adaptive(p, denoise=DenoiseParams())
    assert den.shape == (LH, LW, 3) and den.dtype == np.uint8 and den.max() > 0 and np.array_equal(counts2, counts)
    m = tile_mask(CORNERS, LW, LH)
    assert not img[m].any() and not den[m].any()


# ---- 5: RPT_ERR_STATE and the other refusals that need a buffer
def test_render_adaptive_refuses_a_used_or_mismatched_buffer():
    r = loop_renderer(False)
    p = AdaptiveParams(SPP_B, MIN_B, MAX_B, INF, FLOOR)
    buf = DeviceBuffer(LW, LH)
    r.sample(1, buf)
    with pytest.raises(RptError, match="-2.*empty buffer"):
        r.sample_adaptive(p, buf)
    with pytest.raises(RptError, match="dimension"):
        r.sample_adaptive(p, DeviceBuffer(LW, LH + 1))
    fresh = DeviceBuffer(LW, LH)
    assert r.sample_adaptive(p, fresh) == (0, 9 * MIN_B, 0, 9)
    with pytest.raises(RptError, match="-2.*empty buffer"):      # ... and now it is used
        r.sample_adaptive(p, fresh)
