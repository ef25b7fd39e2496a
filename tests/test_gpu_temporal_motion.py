"""Temporal accumulation of moving objects (rpt_temporal_set_motion*) on the device against the numpy restatement of the definition
in tests/temporal_motion_ref.py.  Equality is bit for bit -- colour, variance and history length of every frame of a sequence --
unless a test says otherwise.  The cameras reach the device as rpt_camera and the restatement as the record
rpt_temporal_camera_record makes of them; the tables reach both as the same doubles.

tests/test_temporal_motion_host.py shows on the same moving scene that the restatement follows the object (with the table 284 of 285
sphere pixels take history, without it 167, with the normal map dead 100 of 293), and that the cube of the rendered sequence is large
enough and moves; the counts are asserted here again on what the device was compared with."""
import functools

import numpy as np
import pytest

from rpt_amd import (DenoiseParams, Denoiser, DeviceBuffer, Renderer, RptError, TemporalAccumulator, TemporalParams, color_bytes, scenes,
                     temporal_camera_record, temporal_motion_record)
from tests.denoise_ref import denoise_ref
from tests.temporal_motion_ref import IDENTITY_RECORD, MotionRef, garbage_motion, moving_sequence, random_records
from tests.temporal_ref import TemporalRef, analytic_cameras, sequence

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (5, 3), (33, 17), (64, 48)]


def same(a, b):
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def ref_kw(p):
    return dict(max_history=p.max_history, flags=p.flags, depth_tol=p.depth_tol, normal_tol=p.normal_tol)


def check(cams, frames, tables, w, h, what, **kw):
    """The host entry point with set_motion(tables[f]) before frame f, against the restatement -> per frame the restatement's outputs,
    its `last` and the frame's id plane.  frames: (record, rgb, var, normal, depth)."""
    p = TemporalParams(**kw)
    acc, ref, outs = TemporalAccumulator(w, h), MotionRef(w, h), []
    for f, (cam, (rec, rgb, var, normal, depth)) in enumerate(zip(cams, frames)):
        normal = normal if p.normal_tol > 0.0 else None
        if tables[f] is not None:
            acc.set_motion(tables[f])
        got = acc.accumulate(cam, rgb, var, normal, depth, params=p, return_variance=True, return_length=True)
        want = ref.accumulate(rec, rgb, var, normal, depth, motion=tables[f], **ref_kw(p))
        for k, name in enumerate(("colour", "variance", "len")):
            bad = ~((got[k] == want[k]) | (np.isnan(got[k]) & np.isnan(want[k])))
            print(f"{what}, frame {f}: {name}: {int(bad.sum())} of {bad.size} values differ; {int(ref.last['took'].sum())} pixels took history")
        assert all(same(got[k], want[k]) for k in range(3)), (what, f)
        outs.append((want, ref.last, depth[..., 2]))
    acc.close()
    return outs


def as_tuples(frames):
    return [(fr["rec"], fr["rgb"], fr["var"], fr["normal"], fr["depth"]) for fr in frames]


# ---- 1: the moving analytic scene
@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("spin", [0.4, 0.8])
@pytest.mark.parametrize("moving", [False, True])
def test_moving_analytic_scene_equals_the_restatement(w, h, spin, moving):
    cams = analytic_cameras(4)
    if not moving:
        cams = [cams[0]] * 4
    frames = moving_sequence(w, h, [temporal_camera_record(c) for c in cams], spin)
    outs = check(cams, as_tuples(frames), [fr["table"] for fr in frames], w, h, f"moving scene {w} x {h}, spin {spin}, camera {'moving' if moving else 'fixed'}")
    if (w, h) == (64, 48):
        for fr, (_, last, _) in list(zip(frames, outs))[1:]:
            took, n = int((last["took"] & fr["sphere"]).sum()), int(fr["sphere"].sum())
            assert took >= (0.95 if spin == 0.4 else 0.9) * n, (took, n)  # conditions 1 and 3 of the host tests, on what the device equals


# ---- 2: planes that belong to no scene, random affine records
@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("m", [1, 3, 70])
def test_garbage_planes_and_random_records_equal_the_restatement(w, h, m):
    cams = analytic_cameras(4)
    frames = garbage_motion(600 + w + m, w, h, [temporal_camera_record(c) for c in cams], m)
    tables = [None] + [random_records(10 * f + m, m) for f in (1, 2, 3)]
    what = f"garbage {w} x {h}, {m} records"
    check(cams, frames, tables, w, h, what + ", every test on", depth_tol=0.5, normal_tol=1.5)
    outs = check(cams, frames, tables, w, h, what + ", normal_tol 0 and no normal plane", normal_tol=0.0)
    outs += check(cams, frames, tables, w, h, what + ", match_id off", match_id=False, depth_tol=0.0, normal_tol=2.0)
    if (w, h) == (64, 48):
        with_record = sum(int((last["took"] & (ids >= 1.0) & (ids <= float(m))).sum()) for _, last, ids in outs)
        past = sum(int((last["took"] & (ids > float(m))).sum()) for _, last, ids in outs)
        print(f"{what}: {with_record} pixels with a record and {past} past the table took history")
        assert with_record > 20 and past > 20


# ---- 3: identity and one-shot
def test_identity_table_none_and_no_call_give_the_same_bits():
    w, h = 33, 17
    cams = analytic_cameras(4)
    frames = sequence(700, w, h, [temporal_camera_record(c) for c in cams])
    a, b, c, ref = [TemporalAccumulator(w, h) for _ in range(3)] + [TemporalRef(w, h)]
    identity = np.tile(IDENTITY_RECORD, (3, 1))
    for cam, (rec, rgb, var, normal, depth) in zip(cams, frames):
        a.set_motion(identity)
        b.set_motion(identity)
        b.set_motion(None)
        want = ref.accumulate(rec, rgb, var, normal, depth)
        for acc in (a, b, c):
            got = acc.accumulate(cam, rgb, var, normal, depth, return_variance=True, return_length=True)
            assert all(same(got[k], want[k]) for k in range(3))
    for acc in (a, b, c):
        acc.close()


def test_a_table_is_consumed_by_one_call():
    w, h = 64, 48
    cams = analytic_cameras(4)
    frames = moving_sequence(w, h, [temporal_camera_record(c) for c in cams], 0.4)
    planes = lambda fr: (fr["rgb"], fr["var"], fr["normal"], fr["depth"])  # noqa: E731
    acc, ref = TemporalAccumulator(w, h), MotionRef(w, h)
    t1, t3 = frames[1]["table"], frames[3]["table"]
    # set before the first frame (consumed there, where nothing is looked up) and before frame 1; frame 2 gets none
    applied = [None, t1, None]
    for f in range(3):
        if f < 2:
            acc.set_motion(t1)
        got = acc.accumulate(cams[f], *planes(frames[f]), return_variance=True, return_length=True)
        want = ref.accumulate(frames[f]["rec"], *planes(frames[f]), motion=applied[f])
        assert all(same(got[k], want[k]) for k in range(3)), f
    stale = MotionRef(w, h)
    for f in range(3):
        other = stale.accumulate(frames[f]["rec"], *planes(frames[f]), motion=t1 if f else None)
    assert not same(other[0], want[0])                                   # a table that outlived its frame would have shown
    # a refused call leaves the table for the next one
    acc.set_motion(t3)
    with pytest.raises(RptError, match="normal_tol"):
        acc.accumulate(cams[3], frames[3]["rgb"], None, None, frames[3]["depth"])
    got = acc.accumulate(cams[3], *planes(frames[3]), return_variance=True, return_length=True)
    want = ref.accumulate(frames[3]["rec"], *planes(frames[3]), motion=t3)
    assert all(same(got[k], want[k]) for k in range(3))
    # a reset drops it
    acc.set_motion(t3)
    acc.reset()
    ref.reset()
    for f in (2, 3):
        got = acc.accumulate(cams[f], *planes(frames[f]), return_variance=True, return_length=True)
        want = ref.accumulate(frames[f]["rec"], *planes(frames[f]))
        assert all(same(got[k], want[k]) for k in range(3)), f
    with pytest.raises(RptError, match="finite"):
        bad = t3.copy()
        bad[1, 7] = np.inf
        acc.set_motion(bad)
    with pytest.raises(ValueError):
        acc.set_motion(np.zeros((2, 23)))
    acc.close()


# ---- 4: entry points and streams
def test_entry_points_agree_and_streams_are_ordered():
    import torch
    w, h = 64, 48
    cams = analytic_cameras(4)
    recs = [temporal_camera_record(c) for c in cams]
    fa = moving_sequence(w, h, recs, 0.4)
    fb = garbage_motion(800, w, h, recs, 3)
    ta = [fr["table"] for fr in fa]
    tb = [random_records(40 + f, 3) for f in range(4)]
    pa, pb = TemporalParams(), TemporalParams(max_history=3, match_id=False, depth_tol=0.5, normal_tol=0.0)
    ra, rb = MotionRef(w, h), MotionRef(w, h)
    wa = [ra.accumulate(fr["rec"], fr["rgb"], fr["var"], fr["normal"], fr["depth"], motion=ta[f], **ref_kw(pa)) for f, fr in enumerate(fa)]
    wb = [rb.accumulate(fr[0], fr[1], fr[2], None, fr[4], motion=tb[f] if f else None, **ref_kw(pb)) for f, fr in enumerate(fb)]
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    da = [[up(fr[k]) for k in ("rgb", "var", "normal", "depth")] for fr in fa]
    db = [[up(a) for a in fr[1:]] for fr in fb]
    dta = [up(t) if t is not None else None for t in ta]
    new = lambda n: torch.full((n,), 7.0, dtype=torch.float64, device="cuda")  # noqa: E731
    oa = [(new(h * w * 3), new(h * w), new(h * w)) for _ in fa]
    oa2 = [(new(h * w * 3), new(h * w), new(h * w)) for _ in fa]
    ob = [(new(h * w * 3), new(h * w), new(h * w)) for _ in fb]
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    a, a2, b = TemporalAccumulator(w, h), TemporalAccumulator(w, h), TemporalAccumulator(w, h)
    # a: host tables, a2: the same tables as device tables, b: other tables; each one's calls alternate between two streams
    for f in range(4):
        sa, sb = (s1, s2) if f % 2 == 0 else (s2, s1)
        rgb, var, normal, depth = da[f]
        a.set_motion(ta[f])
        a.accumulate_device(cams[f], rgb.data_ptr(), var.data_ptr(), normal.data_ptr(), depth.data_ptr(), oa[f][0].data_ptr(), oa[f][1].data_ptr(),
                            oa[f][2].data_ptr(), params=pa, stream_ptr=sa.cuda_stream)
        if dta[f] is not None:
            a2.set_motion_device(dta[f].data_ptr(), 2)
        a2.accumulate_device(cams[f], rgb.data_ptr(), var.data_ptr(), normal.data_ptr(), depth.data_ptr(), oa2[f][0].data_ptr(), oa2[f][1].data_ptr(),
                             oa2[f][2].data_ptr(), params=pa, stream_ptr=sb.cuda_stream)
        rgb, var, normal, depth = db[f]
        if f:
            scratch = tb[f].copy()
            b.set_motion(scratch)
            scratch[:] = np.nan                                          # the caller's array is free as soon as set_motion returns
        b.accumulate_device(cams[f], rgb.data_ptr(), var.data_ptr(), 0, depth.data_ptr(), ob[f][0].data_ptr(), 0, ob[f][2].data_ptr(),
                            params=pb, stream_ptr=sb.cuda_stream)
    torch.cuda.synchronize()
    host = TemporalAccumulator(w, h)
    for f in range(4):
        for outs in (oa, oa2):
            got = [t.cpu().numpy() for t in outs[f]]
            assert same(got[0].reshape(h, w, 3), wa[f][0]) and same(got[1].reshape(h, w), wa[f][1]) and same(got[2].reshape(h, w), wa[f][2]), f
        got = [t.cpu().numpy() for t in ob[f]]
        assert same(got[0].reshape(h, w, 3), wb[f][0]) and same(got[2].reshape(h, w), wb[f][2]), f
        fr = fa[f]
        host.set_motion(ta[f])
        again = host.accumulate(cams[f], fr["rgb"], fr["var"], fr["normal"], fr["depth"], params=pa, return_variance=True, return_length=True)
        assert all(same(again[k], wa[f][k]) for k in range(3))
    for t in (a, a2, b, host):
        t.close()


def test_set_motion_while_the_previous_call_is_queued():
    """Frame 1 (with its table) is queued behind a render that takes milliseconds on the same stream; frame 2's table is set and frame 2
    queued while frame 1 still waits.  Both frames equal the restatement: frame 1 read its own table."""
    import torch
    w, h = 64, 48
    cams = analytic_cameras(3)
    frames = moving_sequence(w, h, [temporal_camera_record(c) for c in cams], 0.8)
    ref = MotionRef(w, h)
    want = [ref.accumulate(fr["rec"], fr["rgb"], fr["var"], fr["normal"], fr["depth"], motion=fr["table"]) for fr in frames]
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    dev = [[up(fr[k]) for k in ("rgb", "var", "normal", "depth")] for fr in frames]
    outs = [(torch.zeros(h * w * 3, dtype=torch.float64, device="cuda"), torch.zeros(h * w, dtype=torch.float64, device="cuda"),
             torch.zeros(h * w, dtype=torch.float64, device="cuda")) for _ in frames]
    scene, cam, cfg = scenes.lampshade()
    r = Renderer(scene, cam).width(96).height(96).max_bounces(cfg["max_bounces"]).seed(1)
    big = torch.zeros(96 * 96 * 3, dtype=torch.float64, device="cuda")
    r.sample_device(1, big.data_ptr())                                   # commit and warm up outside the queue
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    acc = TemporalAccumulator(w, h)

    def queue(f):
        rgb, var, normal, depth = dev[f]
        acc.accumulate_device(cams[f], rgb.data_ptr(), var.data_ptr(), normal.data_ptr(), depth.data_ptr(), outs[f][0].data_ptr(), outs[f][1].data_ptr(),
                              outs[f][2].data_ptr(), stream_ptr=stream.cuda_stream)

    queue(0)
    r.sample_device(4096, big.data_ptr(), stream.cuda_stream)            # 3.5 ms on the stream (tests/test_gpu_call_sequences.py)
    acc.set_motion(frames[1]["table"])
    queue(1)
    acc.set_motion(frames[2]["table"])
    queue(2)
    torch.cuda.synchronize()
    for f in range(3):
        got = [t.cpu().numpy() for t in outs[f]]
        assert same(got[0].reshape(h, w, 3), want[f][0]) and same(got[1].reshape(h, w), want[f][1]) and same(got[2].reshape(h, w), want[f][2]), f
    assert not same(frames[1]["table"], frames[2]["table"])
    acc.close()
    scene.close()


# ---- 5: rendered frames: examples/simple_video.rs at 64 x 48
W, H = 64, 48
VIDEO = {4: dict(first=1, step=0.5), 8: dict(first=1, step=0.25)}            # as tests/test_temporal_motion_host.py checks on the CPU
CUBE_ID = 2.0


def video(n):
    return [scenes.simple_video(VIDEO[n]["first"] + f, VIDEO[n]["step"]) for f in range(n)]


def tables_of(seq):
    return [None] + [np.stack([temporal_motion_record(c.shape.matrix(), p.shape.matrix()) for c, p in zip(cur[0].objects, prev[0].objects)])
                     for prev, cur in zip(seq, seq[1:])]


@functools.lru_cache(maxsize=None)
def rendered(f64, n_frames, spp, seed=3):
    """Per frame 4 batches of spp samples of that frame's scene in a DeviceBuffer, at the sample offsets that follow the previous
    frame's, and the feature planes of the same samples -> [(camera, buffer, planes, mean, variance, table)]."""
    seq = video(n_frames)
    frames = []
    for f, ((scene, cam, cfg), table) in enumerate(zip(seq, tables_of(seq))):
        if f64:
            scene.set_option("epsilon_policy", 1)
        r = Renderer(scene, cam).width(W).height(H).max_bounces(cfg["max_bounces"]).seed(seed)
        r._sample_offset = f * 4 * spp
        planes = r.features_array(4 * spp)
        buf = DeviceBuffer(W, H)
        for _ in range(4):
            r.sample(spp, buf)
        rgb, var = buf.mean()
        for a in (rgb, var, *planes.values()):
            a.setflags(write=False)
        frames.append((cam, buf, planes, rgb, var, table))
        scene.close()
    return frames


@pytest.mark.parametrize("f64", [False, True])
def test_rendered_frames(f64):
    frames = rendered(f64, 4, 4)
    acc, plain, filtered = [TemporalAccumulator(W, H) for _ in range(3)]
    denoiser, ref = Denoiser(W, H), MotionRef(W, H)
    p = TemporalParams()
    images, images_filtered = [], []
    for f, (cam, buf, planes, rgb, var, table) in enumerate(frames):
        for t in (acc, plain, filtered):
            t.set_motion(table)
        got = acc.accumulate(cam, rgb, var, planes["normal"], planes["depth"], return_variance=True, return_length=True)
        want = ref.accumulate(temporal_camera_record(cam), rgb, var, planes["normal"], planes["depth"], motion=table, **ref_kw(p))
        cube = planes["depth"][..., 2] == CUBE_ID
        took = ref.last["took"] & cube
        print(f"simple_video f64={f64}, frame {f}: {int(took.sum())} of {int(cube.sum())} cube pixels take history")
        assert all(same(got[k], want[k]) for k in range(3)), f
        assert cube.sum() >= 100
        if f:
            assert took.sum() >= 0.8 * cube.sum()
        img = buf.temporal_image(plain, cam, planes)
        assert np.array_equal(img, color_bytes(want[0])), f
        images.append(img)
        den, _ = denoise_ref(want[0], want[1], planes["albedo"], planes["normal"], planes["depth"])
        img = buf.temporal_image(filtered, cam, planes, denoiser=denoiser)
        assert np.array_equal(img, color_bytes(den)), f
        images_filtered.append(img)
    # Renderer.render_sequence(cameras, scenes=...) is this composition, and leaves its own scene alone
    seq = video(4)
    if f64:
        for scene, _, _ in seq:
            scene.set_option("epsilon_policy", 1)
    own, cam0, cfg = scenes.simple_video(0)
    r = Renderer(own, cam0).width(W).height(H).max_bounces(cfg["max_bounces"]).seed(3).num_samples(16)
    got = list(r.render_sequence([s[1] for s in seq], 4, scenes=[s[0] for s in seq]))
    assert r.scene is own and len(got) == 4 and all(np.array_equal(a, b) for a, b in zip(got, images))
    seq2 = video(4)
    if f64:
        for scene, _, _ in seq2:
            scene.set_option("epsilon_policy", 1)
    got = list(r.render_sequence([s[1] for s in seq2], 4, denoise=DenoiseParams(), scenes=[s[0] for s in seq2]))
    assert all(np.array_equal(a, b) for a, b in zip(got, images_filtered))
    with pytest.raises(ValueError, match="one Scene per camera"):
        r.render_sequence([cam0, cam0], scenes=[seq[0][0]])
    short = scenes.simple_video(2)[0]
    short.objects.pop()
    with pytest.raises(ValueError, match="same base shape kinds"):
        r.render_sequence([cam0, cam0], scenes=[scenes.simple_video(1)[0], short])
    for s in seq + seq2:
        s[0].close()
    for t in (acc, plain, filtered, denoiser):
        t.close()


# ---- 6: quality.  A condition, not a tolerance: after eight frames of 4 x 1 spp the accumulated frame is closer, over the cube's
# pixels, to a converged one than the last frame alone.  (tools/temporal_motion_quality.py: the restatement on the oracle's renders;
# DESIGN.md section 4, "Moving objects", has the ratios.)  The ratio without a table is printed, not asserted: a one-colour object
# hides misplaced history.
def test_accumulated_frame_is_closer_to_the_converged_one_over_the_cube():
    frames = rendered(False, 8, 1)
    with_table, without = TemporalAccumulator(W, H), TemporalAccumulator(W, H)
    for cam, buf, planes, rgb, var, table in frames:
        with_table.set_motion(table)
        accumulated = buf.temporal_image(with_table, cam, planes)
        blind = buf.temporal_image(without, cam, planes)
    cam, buf, planes, rgb, var, table = frames[-1]
    alone = buf.image()
    scene, _, cfg = video(8)[-1]
    converged = Renderer(scene, cam).width(W).height(H).max_bounces(cfg["max_bounces"]).seed(1234).num_samples(512).render()
    scene.close()
    cube = planes["depth"][..., 2] == CUBE_ID
    rms = lambda a: float(np.sqrt(np.mean((a.astype(np.float64) - converged.astype(np.float64))[cube] ** 2)))  # noqa: E731
    print(f"quality, simple_video 64 x 48, 8 frames of 4 x 1 spp against 512 spp over the cube's {int(cube.sum())} pixels: RMS {rms(alone):.2f} -> "
          f"{rms(accumulated):.2f} levels with the table, ratio {rms(accumulated) / rms(alone):.3f}; without a table {rms(blind):.2f}, "
          f"ratio {rms(blind) / rms(alone):.3f}")
    assert rms(accumulated) < rms(alone)
    for t in (with_table, without):
        t.close()
