"""Adaptive sampling over a sequence on the device (rpt_temporal_preview_device, rpt_temporal_tile_errors_device,
rpt_render_adaptive_temporal) against the numpy restatement in tests/temporal_adaptive_ref.py.  Equality is bit for bit unless a test
says otherwise; pixels and entries that a call must not write keep a sentinel.  tests/test_temporal_adaptive_host.py shows that the
restatement is the definition and chooses, on the CPU, the settings of the conditions asserted in the last section on the device's own
frames."""
import ctypes as C
import functools

import numpy as np
import pytest

from rpt_amd import (AdaptiveParams, DeviceBuffer, Renderer, RptError, TemporalAccumulator, TemporalParams, _lib, color_bytes, scenes,
                     temporal_camera_record, temporal_motion_record)
from rpt_amd.api import camera_desc
from tests import temporal_adaptive_ref as tar
from tests.adaptive_ref import RefBuffer, tile_grid
from tests.temporal_clip_ref import ClipRef, garbage_clip
from tests.temporal_motion_ref import moving_sequence, random_records
from tests.temporal_ref import analytic_cameras, sequence

pytestmark = pytest.mark.gpu

SENTINEL = -7.25
SIZES = [(1, 1), (5, 3), (33, 17), (64, 48), (96, 64)]


def same(a, b):
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def ref_kw(p):
    return dict(max_history=p.max_history, flags=p.flags, depth_tol=p.depth_tol, normal_tol=p.normal_tol)


def tile_lists(w, h):
    """every tile, one tile, the last (partial) tile, alternating tiles, an id out of range among valid ones, an empty list"""
    tx, ty = tile_grid(w, h)
    n = tx * ty
    lists = [None, [0], [n - 1], list(range(0, n, 2)), [n] + ([0] if n > 1 else []), [0xFFFFFFFF], []]
    if n > 2:
        lists.append(list(range(n - 1, -1, -1)))                                  # every tile, descending
    return lists


# ---- 1: the preview against the restatement, after 0, 1 and 3 accumulated frames
def fixed_cameras(n=4):
    return [analytic_cameras(1)[0]] * n


def case_inputs(case, w, h):
    """-> (cameras, frames [(rec, rgb, var, normal, depth)], tables or None, TemporalParams, clip settings or None)"""
    fixed, moving = fixed_cameras(), analytic_cameras(4)
    rec_f, rec_m = [temporal_camera_record(c) for c in fixed], [temporal_camera_record(c) for c in moving]
    seed = 7 * w + h
    if case == "match_id":
        return fixed, garbage_clip(seed, w, h, rec_f), None, TemporalParams(normal_tol=0.0), None
    if case == "no_flag":
        return fixed, garbage_clip(seed + 1, w, h, rec_f), None, TemporalParams(match_id=False, depth_tol=0.0, normal_tol=2.5), None
    if case == "clip_alone":
        return fixed, garbage_clip(seed + 2, w, h, rec_f), None, TemporalParams(match_id=False, depth_tol=0.0, normal_tol=2.5, clip=True), (1, 0.5, 1)
    if case == "clip_r2":
        return fixed, garbage_clip(seed + 3, w, h, rec_f), None, TemporalParams(normal_tol=0.0, clip=True), (2, 1.0, 0)
    if case == "clip_r3":
        return fixed, garbage_clip(seed + 4, w, h, rec_f), None, TemporalParams(normal_tol=0.0, clip=True), (3, 0.25, 5)
    if case in ("motion1", "motion3", "motion70"):
        m = int(case[6:])
        frames = garbage_clip(seed + m, w, h, rec_f, m=m)                           # ids 0 .. m + 2: some lie past the table
        tables = [None] + [random_records(10 * f + m, m) for f in (1, 2, 3)]
        return fixed, frames, tables, TemporalParams(depth_tol=0.5, normal_tol=0.0, clip=(m == 3)), (2, 0.5, 1) if m == 3 else None
    if case == "analytic":                                                          # NaN and inf colours, misses and foreign ids sprinkled in
        return moving, sequence(seed + 5, w, h, rec_m), None, TemporalParams(clip=True), (1, 0.5, 1)
    if case == "moving_sphere":
        frames = moving_sequence(w, h, rec_m, 0.4)
        return (moving, [(fr["rec"], fr["rgb"], fr["var"], fr["normal"], fr["depth"]) for fr in frames], [fr["table"] for fr in frames],
                TemporalParams(), None)
    raise KeyError(case)


CASES = ["match_id", "no_flag", "clip_alone", "clip_r2", "clip_r3", "motion1", "motion3", "motion70", "analytic", "moving_sphere"]


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("case", CASES)
def test_preview_equals_the_restatement(w, h, case):
    cams, frames, tables, p, clip = case_inputs(case, w, h)
    acc, ref = TemporalAccumulator(w, h), ClipRef(w, h)
    if clip is not None:
        acc.set_clip(*clip)
        ref.set_clip(*clip)
    took = 0
    for f, (cam, (rec, rgb, var, normal, depth)) in enumerate(zip(cams, frames)):
        normal = normal if p.normal_tol > 0.0 else None
        table = tables[f] if tables is not None else None
        if table is not None:
            acc.set_motion(table)
        if f in (0, 1, 3):
            full = tar.preview(ref, rec, rgb, var, normal, depth, motion=table, **ref_kw(p))
            for tiles in tile_lists(w, h):
                got = acc.preview(cam, rgb, var, normal, depth, params=p, tiles=tiles, fill=SENTINEL)
                m = tar.tile_mask(tiles, w, h)
                want = (np.where(m[..., None], full[0], SENTINEL), np.where(m, full[1], SENTINEL), np.where(m, full[2], SENTINEL))
                for k, name in enumerate(("colour", "variance", "len")):
                    assert same(got[k], want[k]), (case, f, tiles, name)
            assert acc.frames == f
        got = acc.accumulate(cam, rgb, var, normal, depth, params=p, return_variance=True, return_length=True)
        want = ref.accumulate(rec, rgb, var, normal, depth, motion=table, **ref_kw(p))
        assert all(same(got[k], want[k]) for k in range(3)), (case, f)           # behind the previews: the table was still there
        took += int(ref.last["took"].sum())
    acc.close()
    if (w, h) == (96, 64) and case not in ("moving_sphere",):
        assert took >= 1000, took


def test_preview_with_null_planes_and_null_outputs():
    import torch
    w, h = 33, 17
    cams = fixed_cameras()
    frames = garbage_clip(79, w, h, [temporal_camera_record(c) for c in cams])
    acc, ref = TemporalAccumulator(w, h), ClipRef(w, h)
    p = TemporalParams(clip=True, normal_tol=0.0)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    tiles = torch.tensor([1], dtype=torch.int32, device="cuda")
    for f, (cam, (rec, rgb, var, normal, depth)) in enumerate(zip(cams, frames)):
        want = tar.preview(ref, rec, rgb, None, None, depth, tiles=[1], fill=SENTINEL, **ref_kw(p))
        d_rgb, d_depth = up(rgb), up(depth)
        out = torch.full((h * w * 3,), SENTINEL, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        acc.preview_device(cam, d_rgb.data_ptr(), 0, 0, d_depth.data_ptr(), out.data_ptr(), 0, 0, params=p, d_tiles=tiles.data_ptr(), n_tiles=1)
        torch.cuda.synchronize()
        assert same(out.cpu().numpy().reshape(h, w, 3), want[0]), f
        got = acc.preview(cam, rgb, None, None, depth, params=p, fill=SENTINEL)
        assert all(same(a, b) for a, b in zip(got, tar.preview(ref, rec, rgb, None, None, depth, **ref_kw(p))))
        acc.accumulate(cam, rgb, None, None, depth, params=p)
        ref.accumulate(rec, rgb, None, None, depth, **ref_kw(p))
    acc.close()


# ---- 2: what a preview leaves alone
def test_previews_change_nothing_and_the_table_is_consumed_once():
    w, h = 64, 48
    cams = analytic_cameras(4)
    frames = moving_sequence(w, h, [temporal_camera_record(c) for c in cams], 0.8)
    a, twin, ref = TemporalAccumulator(w, h), TemporalAccumulator(w, h), ClipRef(w, h)
    p = TemporalParams(clip=True)
    for f, (cam, fr) in enumerate(zip(cams, frames)):
        args = (fr["rgb"], fr["var"], fr["normal"], fr["depth"])
        for t in (a, twin):
            t.set_motion(fr["table"])
        for n in range(f + 1):                                                   # 1, 2, 3, 4 previews
            a.preview(cam, *args, params=p, tiles=[n % 4] if n else None)
            assert a.frames == f
        got = a.accumulate(cam, *args, params=p, return_variance=True, return_length=True)
        never = twin.accumulate(cam, *args, params=p, return_variance=True, return_length=True)
        want = ref.accumulate(fr["rec"], *args, motion=fr["table"], **ref_kw(p))
        assert all(same(got[k], never[k]) and same(got[k], want[k]) for k in range(3)), f
        assert a.frames == twin.frames == f + 1
    # the table of the last frame is gone: a preview and an accumulation of the same planes now see none
    fr, cam = frames[-1], cams[-1]
    args = (fr["rgb"], fr["var"], fr["normal"], fr["depth"])
    assert not same(tar.preview(ref, fr["rec"], *args, motion=fr["table"], **ref_kw(p))[0], tar.preview(ref, fr["rec"], *args, **ref_kw(p))[0])
    assert all(same(x, y) for x, y in zip(a.preview(cam, *args, params=p), tar.preview(ref, fr["rec"], *args, **ref_kw(p))))
    got = a.accumulate(cam, *args, params=p, return_variance=True, return_length=True)
    want = ref.accumulate(fr["rec"], *args, **ref_kw(p))
    assert all(same(got[k], want[k]) for k in range(3))
    for t in (a, twin):
        t.close()


def test_set_motion_while_the_previous_call_is_queued():
    """A preview and an accumulation of frame 1 (with its table) are queued behind a render that takes milliseconds on the same stream;
    frame 2's table is set and frame 2 previewed and accumulated while they still wait.  Everything equals the restatement."""
    import torch
    w, h = 64, 48
    cams = analytic_cameras(3)
    frames = moving_sequence(w, h, [temporal_camera_record(c) for c in cams], 0.8)
    ref = ClipRef(w, h)
    want_pv, want = [], []
    for fr in frames:
        args = (fr["rec"], fr["rgb"], fr["var"], fr["normal"], fr["depth"])
        want_pv.append(tar.preview(ref, *args, motion=fr["table"]))
        want.append(ref.accumulate(*args, motion=fr["table"]))
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    dev = [[up(fr[k]) for k in ("rgb", "var", "normal", "depth")] for fr in frames]
    new = lambda: (torch.zeros(h * w * 3, dtype=torch.float64, device="cuda"), torch.zeros(h * w, dtype=torch.float64, device="cuda"),  # noqa: E731
                   torch.zeros(h * w, dtype=torch.float64, device="cuda"))
    outs, pvs = [new() for _ in frames], [new() for _ in frames]
    scene, cam, cfg = scenes.lampshade()
    r = Renderer(scene, cam).width(96).height(96).max_bounces(cfg["max_bounces"]).seed(1)
    big = torch.zeros(96 * 96 * 3, dtype=torch.float64, device="cuda")
    r.sample_device(1, big.data_ptr())                                   # commit and warm up outside the queue
    stream, other = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    acc = TemporalAccumulator(w, h)

    def queue(f, st):
        ptrs = [t.data_ptr() for t in dev[f]]
        acc.preview_device(cams[f], *ptrs, *[t.data_ptr() for t in pvs[f]], stream_ptr=st.cuda_stream)
        acc.accumulate_device(cams[f], *ptrs, *[t.data_ptr() for t in outs[f]], stream_ptr=stream.cuda_stream)

    queue(0, stream)
    r.sample_device(4096, big.data_ptr(), stream.cuda_stream)            # 3.5 ms on the stream (tests/test_gpu_call_sequences.py)
    acc.set_motion(frames[1]["table"])
    queue(1, stream)
    acc.set_motion(frames[2]["table"])
    queue(2, other)                                                      # the preview on another stream: ordered through the event
    torch.cuda.synchronize()
    for f in range(3):
        for got, exp in ((outs[f], want[f]), (pvs[f], want_pv[f])):
            g = [t.cpu().numpy() for t in got]
            assert same(g[0].reshape(h, w, 3), exp[0]) and same(g[1].reshape(h, w), exp[1]) and same(g[2].reshape(h, w), exp[2]), f
    acc.close()
    scene.close()


def test_two_accumulators_on_two_alternating_streams():
    import torch
    w, h = 64, 48
    cams = analytic_cameras(4)
    recs = [temporal_camera_record(c) for c in cams]
    fa, fb = sequence(81, w, h, recs), garbage_clip(82, w, h, [recs[0]] * 4, m=3)
    tb = [None] + [random_records(60 + f, 3) for f in (1, 2, 3)]
    pa, pb = TemporalParams(clip=True), TemporalParams(max_history=5, match_id=False, depth_tol=0.5, normal_tol=0.0, clip=True)
    ra, rb = ClipRef(w, h), ClipRef(w, h)
    rb.set_clip(3, 0.25, 0)
    la, lb = [0, 3], [2, 1]
    wa, wb = [], []
    for f in range(4):
        wa.append(tar.preview(ra, *fa[f], tiles=la, fill=SENTINEL, **ref_kw(pa)))
        ra.accumulate(*fa[f], **ref_kw(pa))
        wb.append(tar.preview(rb, fb[f][0], fb[f][1], None, None, fb[f][4], tiles=lb, fill=SENTINEL, motion=tb[f], **ref_kw(pb)))
        rb.accumulate(fb[f][0], fb[f][1], None, None, fb[f][4], motion=tb[f], **ref_kw(pb))
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    da, db = [[up(a) for a in fr[1:]] for fr in fa], [[up(a) for a in fr[1:]] for fr in fb]
    new = lambda n: torch.full((n,), SENTINEL, dtype=torch.float64, device="cuda")  # noqa: E731
    oa = [(new(h * w * 3), new(h * w), new(h * w)) for _ in range(4)]
    ob = [(new(h * w * 3), new(h * w), new(h * w)) for _ in range(4)]
    scratch = (new(h * w * 3), new(h * w * 3))
    ta, tb_d = torch.tensor(la, dtype=torch.int32, device="cuda"), torch.tensor(lb, dtype=torch.int32, device="cuda")
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    a, b = TemporalAccumulator(w, h), TemporalAccumulator(w, h)
    b.set_clip(3, 0.25, 0)
    for f in range(4):
        sa, sb = (s1, s2) if f % 2 == 0 else (s2, s1)
        rgb, var, normal, depth = da[f]
        a.preview_device(cams[f], rgb.data_ptr(), var.data_ptr(), normal.data_ptr(), depth.data_ptr(), *[t.data_ptr() for t in oa[f]], params=pa,
                         d_tiles=ta.data_ptr(), n_tiles=2, stream_ptr=sa.cuda_stream)
        a.accumulate_device(cams[f], rgb.data_ptr(), var.data_ptr(), normal.data_ptr(), depth.data_ptr(), scratch[0].data_ptr(), params=pa,
                            stream_ptr=sb.cuda_stream)
        rgb, var, normal, depth = db[f]
        if tb[f] is not None:
            b.set_motion(tb[f])
        b.preview_device(cams[0], rgb.data_ptr(), 0, 0, depth.data_ptr(), *[t.data_ptr() for t in ob[f]], params=pb, d_tiles=tb_d.data_ptr(),
                         n_tiles=2, stream_ptr=sb.cuda_stream)
        b.accumulate_device(cams[0], rgb.data_ptr(), 0, 0, depth.data_ptr(), scratch[1].data_ptr(), params=pb, stream_ptr=sa.cuda_stream)
    torch.cuda.synchronize()
    for f in range(4):
        for outs, want in ((oa, wa), (ob, wb)):
            got = [t.cpu().numpy() for t in outs[f]]
            assert same(got[0].reshape(h, w, 3), want[f][0]) and same(got[1].reshape(h, w), want[f][1]) and same(got[2].reshape(h, w), want[f][2]), f
    for t in (a, b):
        t.close()


# ---- 3: the tile errors of planes
@pytest.mark.parametrize("w,h", SIZES)
def test_plane_errors_equal_the_restatement(w, h):
    rng = np.random.default_rng(3 * w + h)
    rgb, var = rng.uniform(0.0, 2.0, (h, w, 3)), rng.uniform(0.0, 0.1, (h, w))
    acc = TemporalAccumulator(w, h)
    planes = [(rgb, var)]
    if w > 5:
        bad_rgb, bad_var = rgb.copy(), var.copy()
        bad_rgb[3, 4, 1], bad_var[5, 6], bad_rgb[1, w - 1, 0], bad_var[h - 1, 0] = np.nan, np.inf, np.inf, np.nan
        planes += [(bad_rgb, bad_var), (rgb, np.zeros((h, w)))]                   # NaN and inf; zero variance
    for a, v in planes:
        for tiles in tile_lists(w, h):
            got = acc.tile_errors(a, v, 0.05, tiles=tiles, fill=SENTINEL)
            assert same(got, tar.plane_tile_errors(a, v, 0.05, tiles=tiles, fill=SENTINEL)), tiles
    assert not acc.tile_errors(rgb, np.zeros((h, w)), 0.05).any()
    acc.close()


@pytest.mark.parametrize("w,h", [(33, 17), (96, 64), (100, 70)])
def test_plane_errors_of_the_buffers_mean_are_the_buffers_tile_errors(w, h):
    import torch
    rng = np.random.default_rng(w + h)
    buf, ref, acc = DeviceBuffer(w, h), RefBuffer(w, h), TemporalAccumulator(w, h)
    for _ in range(2):
        b = rng.uniform(0.0, 1.5, (h, w, 3))
        buf.add_samples(b)
        ref.add(b)
    assert same(acc.tile_errors(*buf.mean(), 0.07), buf.tile_errors(0.07))        # no tile batch yet
    tx, ty = tile_grid(w, h)
    target = [(5, 3, 2)[t % 3] for t in range(tx * ty)]                            # 2, 3 and 5 batches per tile
    for r in range(3):
        b = rng.uniform(0.0, 1.5, (h, w, 3))
        ids = [t for t in range(tx * ty) if target[t] - 2 > r]
        d_b = torch.from_numpy(b.reshape(-1)).cuda()
        d_ids = torch.tensor(ids + [0], dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        buf.add_samples_tiles_device(d_b.data_ptr(), d_ids.data_ptr(), len(ids))
        torch.cuda.synchronize()
        ref.add_tiles(b, ids)
    assert buf.tile_batches().reshape(-1).tolist() == target
    mean, var = buf.mean()
    got = acc.tile_errors(mean, var, 0.07)
    assert same(got, buf.tile_errors(0.07))
    # (the restatement's sums of squares differ from the device's in the last place on values like these; on planes it agrees:)
    assert same(got, tar.plane_tile_errors(mean, var, 0.07)) and np.allclose(got, ref.tile_errors(0.07), rtol=1e-12, atol=0.0)
    acc.close()
    buf.close()


# ---- 4: the loop on rendered scenes, 96 x 64, four frames, both render modes
W, H, FRAMES, SEED = tar.QUALITY_W, tar.QUALITY_H, tar.QUALITY_FRAMES, tar.QUALITY_SEED
LOOP = tar.QUALITY_LOOP
SPAN = LOOP["max_batches"] * LOOP["spp_per_batch"]


def tables_of(seq):
    return [None] + [np.stack([temporal_motion_record(c.shape.matrix(), p.shape.matrix()) for c, p in zip(cur[0].objects, prev[0].objects)])
                     for prev, cur in zip(seq, seq[1:])]


def frames_of(name, moving, f64, n=FRAMES):
    seq = [getattr(scenes, name)(f if moving else 0) for f in range(n)]
    if f64:
        for scene, _, _ in seq:
            scene.set_option("epsilon_policy", 1)
    return seq, (tables_of(seq) if moving else [None] * n)


class DeviceSums:
    """RefBuffer's interface over a DeviceBuffer: the sums are the device's own (its sum of squares is compiled as the render kernels'
    file is, and differs from numpy's in the last place), so the restated loop is driven by exactly the planes the device's loop sees;
    the preview, the tile errors of planes, the selection and the loop's logic stay numpy."""

    def __init__(self, w, h):
        self.w, self.h, self.buf = w, h, DeviceBuffer(w, h)

    def add(self, batch):
        self.buf.add_samples(np.ascontiguousarray(batch))

    def add_tiles(self, batch, tiles):
        import torch
        d_b = torch.from_numpy(np.array(batch, dtype=np.float64).reshape(-1)).cuda()          # (a copy: the batch is read-only)
        d_ids = torch.from_numpy(np.concatenate([np.asarray(tiles, dtype=np.uint32), np.zeros(1, np.uint32)]).view(np.int32)).cuda()
        torch.cuda.synchronize()
        self.buf.add_samples_tiles_device(d_b.data_ptr(), d_ids.data_ptr(), len(tiles))
        torch.cuda.synchronize()

    def mean(self):
        return self.buf.mean()

    def tile_batches(self):
        return self.buf.tile_batches()

    def tile_errors(self, floor):
        return self.buf.tile_errors(floor)

    def counts(self):
        return np.repeat(np.repeat(self.tile_batches(), 32, axis=0), 32, axis=1)[:self.h, :self.w]


def device_batches(r):
    """batch_at(offset) by the device: the full-frame batch of LOOP's spp at that sample offset."""
    @functools.lru_cache(maxsize=None)
    def batch_at(offset):
        r._sample_offset = offset
        b = r.sample_array(LOOP["spp_per_batch"]).reshape(H, W, 3)
        b.setflags(write=False)
        return b
    return batch_at


def run_frames(name, moving, f64, p, clip=None, reset_before=(), max_blocks=0, n=FRAMES):
    """The device's loop, frame by frame, against the restated loop driven by the device's own full-frame batches; every frame is
    finished by an accumulation that is compared too -> per frame (tile batches, stats, the plain loop's tile batches)."""
    seq, tables = frames_of(name, moving, f64, n)
    acc, ref = TemporalAccumulator(W, H), ClipRef(W, H)
    if clip is not None:
        acc.set_clip(*clip)
        ref.set_clip(*clip)
    params = AdaptiveParams(**LOOP)
    rows, held = [], 0
    for f, ((scene, cam, cfg), table) in enumerate(zip(seq, tables)):
        if f in reset_before:
            acc.reset()
            ref.reset()
            held = 0
        if max_blocks:
            scene.set_option("max_blocks", max_blocks)
        r = Renderer(scene, cam).width(W).height(H).max_bounces(cfg["max_bounces"]).seed(SEED)
        offset = f * SPAN
        planes = r.features_array(LOOP["min_batches"] * LOOP["spp_per_batch"], albedo=False, sample_offset=offset)
        normal, depth = planes["normal"], planes["depth"]
        rec = temporal_camera_record(cam)
        acc.set_motion(table)
        buf = DeviceBuffer(W, H)
        stats = r.sample_adaptive_temporal(params, buf, acc, planes, p, sample_offset=offset)
        assert acc.frames == held
        batch_at = device_batches(r)
        want, want_stats, last, lists = tar.adaptive_temporal_loop(batch_at, W, H, ref, rec, normal, depth, sample_offset=offset, motion=table,
                                                                   buffer=DeviceSums(W, H), **LOOP, **ref_kw(p))
        mean, var = buf.mean()
        w_mean, w_var = want.mean()
        print(f"{name} f64={f64} frame {f}: tile batches {buf.tile_batches().reshape(-1).tolist()}, stats {stats}; restated "
              f"{want.tile_batches().reshape(-1).tolist()}, {want_stats}")
        assert np.array_equal(buf.tile_batches(), want.tile_batches()) and stats == want_stats, f
        assert same(mean, w_mean) and same(var, w_var), f
        assert buf.batches == LOOP["min_batches"]
        plain = tar.plain_adaptive_loop(batch_at, W, H, sample_offset=offset, buffer=DeviceSums(W, H), **LOOP)[0]
        # the loop accumulated nothing and left the table: the accumulation that finishes the frame
        got = acc.accumulate(cam, mean, var, normal, depth, params=p, return_variance=True, return_length=True)
        exp = ref.accumulate(rec, mean, var, normal, depth, motion=table, **ref_kw(p))
        assert all(same(got[k], exp[k]) for k in range(3)), f
        if not p.clip:
            stopped = want.counts() < LOOP["max_batches"]
            assert all(same(got[k][stopped], last[k][stopped]) for k in range(3)), f
        held += 1
        rows.append((buf.tile_batches(), stats, plain.tile_batches(), plain, buf))
        scene.close()
    acc.close()
    return rows


@pytest.mark.parametrize("f64", [False, True])
def test_loop_equals_the_restated_loop_and_meets_the_conditions(f64):
    """scenes.sliding_shadow(0) at rest: the settings chosen on the CPU; frame 4 follows a reset."""
    rows = run_frames(tar.QUALITY_SCENE, False, f64, TemporalParams(), reset_before=(FRAMES,), n=FRAMES + 1)
    counts = [row[0] for row in rows]
    totals = tar.check_conditions(counts[:FRAMES], rows[0][2], counts[FRAMES], rows[FRAMES][2])
    print(f"f64={f64}: tile batches per frame {totals}, behind the reset {int(counts[FRAMES].sum())}")
    # frame 0 and the frame behind the reset: the plain loop's buffer, bit for bit; frame 0 also by rpt_render_adaptive itself
    for f in (0, FRAMES):
        assert all(same(a, b) for a, b in zip(rows[f][4].mean(), rows[f][3].mean())), f
    scene, cam, cfg = getattr(scenes, tar.QUALITY_SCENE)(0)
    if f64:
        scene.set_option("epsilon_policy", 1)
    own = DeviceBuffer(W, H)
    stats = Renderer(scene, cam).width(W).height(H).max_bounces(cfg["max_bounces"]).seed(SEED).sample_adaptive(AdaptiveParams(**LOOP), own)
    assert stats == rows[0][1] and np.array_equal(own.tile_batches(), counts[0])
    assert all(same(a, b) for a, b in zip(own.mean(), rows[0][4].mean()))
    scene.close()


@pytest.mark.parametrize("f64", [False, True])
def test_loop_with_a_motion_table(f64):
    run_frames("simple_video", True, f64, TemporalParams())
    # (simple_video's point light lights nothing, scenes.py: every tile stops at min_batches.  The same under a light that does:)
    rows = run_frames("sliding_shadow", True, f64, TemporalParams())
    assert any(int(row[0].max()) > LOOP["min_batches"] for row in rows[1:])


@pytest.mark.parametrize("f64", [False, True])
def test_loop_with_clipping_and_a_moving_shadow(f64):
    rows = run_frames("sliding_shadow", True, f64, TemporalParams(clip=True), clip=(1, 0.5, 1))
    assert any(int(row[0].max()) > LOOP["min_batches"] for row in rows)


def test_loop_on_a_capped_grid():
    rows = run_frames(tar.QUALITY_SCENE, False, False, TemporalParams(), max_blocks=5, n=2)
    free = run_frames(tar.QUALITY_SCENE, False, False, TemporalParams(), n=2)
    assert all(np.array_equal(a[0], b[0]) and all(same(x, y) for x, y in zip(a[4].mean(), b[4].mean())) for a, b in zip(rows, free))


def test_render_sequence_with_adaptive_equals_the_restatement():
    seq, tables = frames_of("sliding_shadow", True, False)
    p, params = TemporalParams(clip=True), AdaptiveParams(**LOOP)
    ref, want, want_counts = ClipRef(W, H), [], []
    for f, ((scene, cam, cfg), table) in enumerate(zip(seq, tables)):
        r = Renderer(scene, cam).width(W).height(H).max_bounces(cfg["max_bounces"]).seed(SEED)
        planes = r.features_array(LOOP["min_batches"] * LOOP["spp_per_batch"], albedo=False, sample_offset=f * SPAN)
        rec = temporal_camera_record(cam)
        buf, _, _, _ = tar.adaptive_temporal_loop(device_batches(r), W, H, ref, rec, planes["normal"], planes["depth"], sample_offset=f * SPAN,
                                                  motion=table, buffer=DeviceSums(W, H), **LOOP, **ref_kw(p))
        out, _, _ = ref.accumulate(rec, *buf.mean(), planes["normal"], planes["depth"], motion=table, **ref_kw(p))
        want.append(color_bytes(out))
        want_counts.append(buf.tile_batches())
    own, cam0, cfg = scenes.sliding_shadow(0)
    r = Renderer(own, cam0).width(W).height(H).max_bounces(cfg["max_bounces"]).seed(SEED).num_samples(1)
    got = list(r.render_sequence([s[1] for s in seq], temporal=p, scenes=[s[0] for s in seq], adaptive=params, return_tile_batches=True))
    assert len(got) == FRAMES
    for f, (img, counts) in enumerate(got):
        assert np.array_equal(img, want[f]) and np.array_equal(counts, want_counts[f]), f
    plain = list(r.render_sequence([s[1] for s in seq], temporal=p, scenes=[s[0] for s in seq], adaptive=params))
    assert all(np.array_equal(a, b[0]) for a, b in zip(plain, got))
    for s in seq:
        s[0].close()
    own.close()


# ---- 5: the refusals that need handles
def test_refusals_that_need_a_buffer_and_an_accumulator():
    import torch
    scene, cam, cfg = scenes.sliding_shadow(0)
    r = Renderer(scene, cam).width(W).height(H).max_bounces(cfg["max_bounces"]).seed(SEED)
    host = r.features_array(4, albedo=False)
    keep = {k: torch.from_numpy(np.array(v).reshape(-1)).cuda() for k, v in host.items()}
    planes = {k: t.data_ptr() for k, t in keep.items()}                          # device pointers: the C ABI's own checks are reached
    torch.cuda.synchronize()
    p = AdaptiveParams(**dict(LOOP, threshold=float("inf")))
    acc = TemporalAccumulator(W, H)
    used = DeviceBuffer(W, H)
    r.sample(1, used)
    with pytest.raises(RptError, match="-2.*empty buffer"):
        r.sample_adaptive_temporal(p, used, acc, planes, sample_offset=0)
    with pytest.raises(RptError, match="dimension"):
        r.sample_adaptive_temporal(p, DeviceBuffer(W, H + 1), acc, planes, sample_offset=0)
    small = TemporalAccumulator(W, H - 1)
    with pytest.raises(RptError, match="different sizes"):
        r.sample_adaptive_temporal(p, DeviceBuffer(W, H), small, planes, sample_offset=0)
    with pytest.raises(RptError, match="depth plane"):
        r.sample_adaptive_temporal(p, DeviceBuffer(W, H), acc, {"normal": planes["normal"]}, sample_offset=0)
    with pytest.raises(RptError, match="needs the normal"):
        r.sample_adaptive_temporal(p, DeviceBuffer(W, H), acc, {"depth": planes["depth"]}, sample_offset=0)
    fresh = DeviceBuffer(W, H)
    assert r.sample_adaptive_temporal(p, fresh, acc, planes, sample_offset=0) == (0, 6 * LOOP["min_batches"], 0, 6)
    assert acc.frames == 0
    # the lists of the two device entry points
    lib = _lib.load()
    d = torch.zeros(W * H * 10, dtype=torch.float64, device="cuda")
    ids = torch.zeros(8, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    base, n = d.data_ptr(), W * H * 8
    tp, cd = TemporalParams(normal_tol=0.0).desc(), camera_desc(cam, _lib.CameraDesc)
    v = C.c_void_p
    assert lib.rpt_temporal_preview_device(acc._h, C.byref(tp), C.byref(cd), v(base), None, None, v(base + 3 * n), v(ids.data_ptr()), 7,
                                           v(base + 6 * n), None, None, None) == -1 and b"more tiles" in lib.rpt_last_error()
    assert lib.rpt_temporal_tile_errors_device(acc._h, v(base), v(base + 3 * n), 0.05, None, 2, v(base + 4 * n), None) == -1
    assert b"null tile list" in lib.rpt_last_error()
    assert lib.rpt_temporal_tile_errors_device(acc._h, v(base), v(base + 3 * n), 0.05, v(ids.data_ptr()), 7, v(base + 4 * n), None) == -1
    assert b"more tiles" in lib.rpt_last_error()
    torch.cuda.synchronize()
    assert not d.cpu().numpy().any()
    for t in (acc, small):
        t.close()
    scene.close()
