"""History clipping of the temporal accumulation (RPT_TEMPORAL_CLIP, rpt_temporal_set_clip) on the device against the numpy
restatement of the definition in tests/temporal_clip_ref.py.  Equality is bit for bit -- colour, variance and history length of every
frame of a four-frame sequence -- unless a test says otherwise.  Sizes: 1 x 1; 5 x 3 (the window is larger than the image); 16 x 17 and
17 x 16 (one row or column of a second block, whose other threads idle at the barrier); 33 x 17; 64 x 48; each at r = 1, 2, 3.

tests/test_temporal_clip_host.py shows that the restatement is the definition (neighbour by neighbour) and that on such planes the
step runs and changes colours; the counts are asserted here again on what the device was compared with.  The last section renders
scenes.sliding_shadow and scenes.moving_light in both modes and asserts the three quality conditions of DESIGN.md section 4, "History
clipping", on the device's frames."""
import functools

import numpy as np
import pytest

from rpt_amd import (DeviceBuffer, Renderer, RptError, TemporalAccumulator, TemporalParams, color_bytes, scenes, temporal_camera_record,
                     temporal_motion_record)
from tests.temporal_clip_ref import (CLIP_DEFAULTS, ClipRef, garbage_clip, quality_masks, rms_levels)
from tests.temporal_motion_ref import moving_sequence, random_records
from tests.temporal_ref import analytic_cameras, garbage, sequence

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (5, 3), (16, 17), (17, 16), (33, 17), (64, 48)]
CLIPS = {1: (1, 0.5, 1), 2: (2, 1.0, 0), 3: (3, 0.25, 5)}                     # clip_history 1, 0 and 5


def same(a, b):
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def ref_kw(p):
    return dict(max_history=p.max_history, flags=p.flags, depth_tol=p.depth_tol, normal_tol=p.normal_tol)


def check(cams, frames, tables, w, h, what, clip, on=None, **kw):
    """The host entry point against the restatement, frame by frame; clip: the settings or None (set_clip is never called); on: per
    frame whether the flag is set (default: always) -> (pixels that took history, pixels that were clipped)."""
    acc, ref = TemporalAccumulator(w, h), ClipRef(w, h)
    if clip is not None:
        acc.set_clip(*clip)
        ref.set_clip(*clip)
    took = clipped = 0
    for f, (cam, (rec, rgb, var, normal, depth)) in enumerate(zip(cams, frames)):
        p = TemporalParams(clip=on[f] if on is not None else True, **kw)
        normal = normal if p.normal_tol > 0.0 else None
        if tables is not None and tables[f] is not None:
            acc.set_motion(tables[f])
        got = acc.accumulate(cam, rgb, var, normal, depth, params=p, return_variance=True, return_length=True)
        want = ref.accumulate(rec, rgb, var, normal, depth, motion=tables[f] if tables is not None else None, **ref_kw(p))
        for k, name in enumerate(("colour", "variance", "len")):
            bad = ~((got[k] == want[k]) | (np.isnan(got[k]) & np.isnan(want[k])))
            print(f"{what}, frame {f}: {name}: {int(bad.sum())} of {bad.size} values differ")
        assert all(same(got[k], want[k]) for k in range(3)), (what, f)
        took += int(ref.last["took"].sum())
        clipped += int(ref.last["clipped"].sum())
    acc.close()
    print(f"{what}: {took} pixels took history, {clipped} were clipped")
    return took, clipped


def fixed_cameras(n=4):
    return [analytic_cameras(1)[0]] * n


# ---- 1: planes that belong to no scene
@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("radius", [1, 2, 3])
def test_garbage_planes_equal_the_restatement(w, h, radius):
    cams = fixed_cameras()
    recs = [temporal_camera_record(c) for c in cams]
    what = f"garbage {w} x {h}, r {radius}"
    frames = garbage_clip(900 + w + 3 * h + radius, w, h, recs)
    t1 = check(cams, frames, None, w, h, what + ", both flags", CLIPS[radius], normal_tol=0.0)
    t2 = check(cams, frames, None, w, h, what + ", the flag alone", CLIPS[radius], match_id=False, depth_tol=0.0, normal_tol=2.5)
    moved = garbage_clip(950 + w + radius, w, h, recs, m=3)
    tables = [None] + [random_records(10 * f + radius, 3) for f in (1, 2, 3)]
    check(cams, moved, tables, w, h, what + ", a motion table", CLIPS[radius], depth_tol=0.5, normal_tol=0.0)
    # the garbage planes of tests/test_gpu_temporal.py under a moving camera (three ids, any depth and coverage)
    moving = analytic_cameras(4)
    check(moving, garbage(500 + w + radius, w, h, [temporal_camera_record(c) for c in moving]), None, w, h, what + ", any depth", CLIPS[radius],
          depth_tol=0.0, normal_tol=0.0)
    if (w, h) == (64, 48):
        assert min(t1[0], t2[0]) >= 1000 and min(t1[1], t2[1]) >= 500        # the step ran, and changed colours


# ---- 2: the analytic scene of tests/test_gpu_temporal.py, with NaN and inf colours, misses and foreign ids sprinkled in
@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("radius", [1, 2, 3])
def test_analytic_scene_equals_the_restatement(w, h, radius):
    cams = analytic_cameras(4)
    recs = [temporal_camera_record(c) for c in cams]
    what = f"analytic scene {w} x {h}, r {radius}"
    took, clipped = check(cams, sequence(300 + w + radius, w, h, recs), None, w, h, what, CLIPS[radius])
    frames = moving_sequence(w, h, recs, 0.4)
    rng = np.random.default_rng(w + radius)
    tuples = [(fr["rec"], fr["rgb"] + rng.normal(size=(h, w, 3)) * 0.05, fr["var"], fr["normal"], fr["depth"]) for fr in frames]
    check(cams, tuples, [fr["table"] for fr in frames], w, h, what + ", the moving sphere", CLIPS[radius])
    if (w, h) == (64, 48):
        assert took >= 5000 and clipped >= 1000


# ---- 3: the flag and the settings
def test_the_flag_toggled_between_the_frames_of_a_sequence():
    w, h = 33, 17
    cams = fixed_cameras()
    frames = garbage_clip(77, w, h, [temporal_camera_record(c) for c in cams])
    for on in ([False, True, False, True], [True, False, True, True]):
        took, clipped = check(cams, frames, None, w, h, f"flag {on}", (2, 0.5, 1), on=on, normal_tol=0.0)
        assert clipped >= 100


def test_the_flag_with_set_clip_never_called_uses_the_defaults():
    w, h = 33, 17
    cams = analytic_cameras(4)
    frames = sequence(78, w, h, [temporal_camera_record(c) for c in cams])
    took, clipped = check(cams, frames, None, w, h, "defaults", None)
    assert clipped >= 100 and ClipRef(w, h).clip == CLIP_DEFAULTS == (1, 0.5, 1)


def test_null_variance_and_normal_planes():
    w, h = 17, 16
    cams = fixed_cameras()
    frames = [(rec, rgb, None, None, depth) for rec, rgb, var, normal, depth in garbage_clip(79, w, h, [temporal_camera_record(c) for c in cams])]
    acc, ref = TemporalAccumulator(w, h), ClipRef(w, h)
    p = TemporalParams(clip=True, normal_tol=0.0)
    for f, (cam, (rec, rgb, var, normal, depth)) in enumerate(zip(cams, frames)):
        got = acc.accumulate(cam, rgb, None, None, depth, params=p, return_variance=True, return_length=True)
        want = ref.accumulate(rec, rgb, None, None, depth, **ref_kw(p))
        assert all(same(got[k], want[k]) for k in range(3)), f
        assert same(acc.accumulate(cam, rgb, None, None, depth, params=TemporalParams(max_history=1, clip=True, normal_tol=0.0)),
                    ref.accumulate(rec, rgb, None, None, depth, **ref_kw(TemporalParams(max_history=1, clip=True, normal_tol=0.0)))[0])
    acc.close()


def test_settings_persist_over_a_reset_and_bad_ones_are_refused():
    w, h = 16, 17
    cams = fixed_cameras()
    frames = garbage_clip(80, w, h, [temporal_camera_record(c) for c in cams])
    acc, ref = TemporalAccumulator(w, h), ClipRef(w, h)
    acc.set_clip(3, 0.25, 0)
    ref.set_clip(3, 0.25, 0)
    for bad in ((0, 0.5, 1), (4, 0.5, 1), (1, float("nan"), 1), (1, float("inf"), 1), (1, -1.0, 1), (1, 0.5, 4097)):
        with pytest.raises(RptError):
            acc.set_clip(*bad)
    p = TemporalParams(clip=True, normal_tol=0.0)
    for f, (cam, (rec, rgb, var, normal, depth)) in enumerate(zip(cams, frames)):
        if f == 2:
            acc.reset()
            ref.reset()
        got = acc.accumulate(cam, rgb, var, None, depth, params=p, return_variance=True, return_length=True)
        want = ref.accumulate(rec, rgb, var, None, depth, **ref_kw(p))
        assert all(same(got[k], want[k]) for k in range(3)), f
    assert ref.last["clipped"].sum() >= 30
    acc.close()


# ---- 4: the device entry point; two accumulators with different settings on two alternating streams
def test_entry_points_agree_and_streams_are_ordered():
    import torch
    w, h = 64, 48
    cams = analytic_cameras(4)
    recs = [temporal_camera_record(c) for c in cams]
    fa = sequence(81, w, h, recs)
    fb = garbage_clip(82, w, h, [recs[0]] * 4, m=3)
    tb = [None] + [random_records(60 + f, 3) for f in (1, 2, 3)]
    pa, pb = TemporalParams(clip=True), TemporalParams(max_history=5, match_id=False, depth_tol=0.5, normal_tol=0.0, clip=True)
    ra, rb = ClipRef(w, h), ClipRef(w, h)
    rb.set_clip(3, 0.25, 0)
    wa = [ra.accumulate(*fr, **ref_kw(pa)) for fr in fa]
    wb = [rb.accumulate(fr[0], fr[1], None, None, fr[4], motion=tb[f], **ref_kw(pb)) for f, fr in enumerate(fb)]
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    da = [[up(a) for a in fr[1:]] for fr in fa]
    db = [[up(a) for a in fr[1:]] for fr in fb]
    new = lambda n: torch.full((n,), 7.0, dtype=torch.float64, device="cuda")  # noqa: E731
    oa = [(new(h * w * 3), new(h * w), new(h * w)) for _ in fa]
    ob = [(new(h * w * 3), new(h * w), new(h * w)) for _ in fb]
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    a, b = TemporalAccumulator(w, h), TemporalAccumulator(w, h)
    b.set_clip(3, 0.25, 0)
    for f in range(4):
        sa, sb = (s1, s2) if f % 2 == 0 else (s2, s1)
        rgb, var, normal, depth = da[f]
        a.accumulate_device(cams[f], rgb.data_ptr(), var.data_ptr(), normal.data_ptr(), depth.data_ptr(), oa[f][0].data_ptr(), oa[f][1].data_ptr(),
                            oa[f][2].data_ptr(), params=pa, stream_ptr=sa.cuda_stream)
        rgb, var, normal, depth = db[f]
        if tb[f] is not None:
            b.set_motion(tb[f])
        b.accumulate_device(cams[0], rgb.data_ptr(), 0, 0, depth.data_ptr(), ob[f][0].data_ptr(), ob[f][1].data_ptr(), ob[f][2].data_ptr(),
                            params=pb, stream_ptr=sb.cuda_stream)
    torch.cuda.synchronize()
    host = TemporalAccumulator(w, h)
    for f in range(4):
        for outs, want in ((oa, wa), (ob, wb)):
            got = [t.cpu().numpy() for t in outs[f]]
            assert same(got[0].reshape(h, w, 3), want[f][0]) and same(got[1].reshape(h, w), want[f][1]) and same(got[2].reshape(h, w), want[f][2]), f
        again = host.accumulate(cams[f], *fa[f][1:], params=pa, return_variance=True, return_length=True)
        assert all(same(again[k], wa[f][k]) for k in range(3))
    assert ra.last["clipped"].sum() >= 500 and rb.last["clipped"].sum() >= 500
    for t in (a, b, host):
        t.close()


# ---- 5: rendered frames and quality: scenes.sliding_shadow and scenes.moving_light at 64 x 48, 8 frames of 4 x 1 spp, seed 3
W, H, FRAMES, BATCHES = 64, 48, 8, 4


def tables_of(seq):
    return [None] + [np.stack([temporal_motion_record(c.shape.matrix(), p.shape.matrix()) for c, p in zip(cur[0].objects, prev[0].objects)])
                     for prev, cur in zip(seq, seq[1:])]


def sequence_of(name, f64):
    seq = [getattr(scenes, name)(f) for f in range(FRAMES)]
    if f64:
        for scene, _, _ in seq:
            scene.set_option("epsilon_policy", 1)
    return seq


@functools.lru_cache(maxsize=None)
def rendered(name, f64):
    """Per frame 4 batches of 1 spp in a DeviceBuffer at the sample offsets that follow the previous frame's, the feature planes of
    the same samples -> ([(camera, buffer, planes, mean, variance, table)], the converged 8-bit frames of the last scene and of the
    scene two earlier: 512 spp with another seed)."""
    seq = sequence_of(name, f64)
    frames, converged = [], {}
    for f, ((scene, cam, cfg), table) in enumerate(zip(seq, tables_of(seq))):
        r = Renderer(scene, cam).width(W).height(H).max_bounces(cfg["max_bounces"]).seed(3)
        r._sample_offset = f * BATCHES
        planes = r.features_array(BATCHES)
        buf = DeviceBuffer(W, H)
        for _ in range(BATCHES):
            r.sample(1, buf)
        rgb, var = buf.mean()
        for a in (rgb, var, *planes.values()):
            a.setflags(write=False)
        frames.append((cam, buf, planes, rgb, var, table))
        if f in (FRAMES - 3, FRAMES - 1):
            converged[f] = Renderer(scene, cam).width(W).height(H).max_bounces(cfg["max_bounces"]).seed(1234).num_samples(512).render()
        scene.close()
    return frames, converged[FRAMES - 1], converged[FRAMES - 3]


@pytest.mark.parametrize("f64", [False, True])
@pytest.mark.parametrize("name", ["sliding_shadow", "moving_light"])
def test_rendered_scenes_equal_the_restatement_and_meet_the_quality_conditions(name, f64):
    frames, converged, earlier = rendered(name, f64)
    acc, clip_img, plain_img = [TemporalAccumulator(W, H) for _ in range(3)]
    ref, ref_plain = ClipRef(W, H), ClipRef(W, H)
    p, plain = TemporalParams(clip=True), TemporalParams()
    images = []
    for f, (cam, buf, planes, rgb, var, table) in enumerate(frames):
        for t in (acc, clip_img, plain_img):
            t.set_motion(table)
        rec = temporal_camera_record(cam)
        got = acc.accumulate(cam, rgb, var, planes["normal"], planes["depth"], params=p, return_variance=True, return_length=True)
        want = ref.accumulate(rec, rgb, var, planes["normal"], planes["depth"], motion=table, **ref_kw(p))
        want_plain = ref_plain.accumulate(rec, rgb, var, planes["normal"], planes["depth"], motion=table, **ref_kw(plain))
        assert all(same(got[k], want[k]) for k in range(3)), f
        img = buf.temporal_image(clip_img, cam, planes, p)
        assert np.array_equal(img, color_bytes(want[0])), f
        images.append(img)
        img_plain = buf.temporal_image(plain_img, cam, planes, plain)
        assert np.array_equal(img_plain, color_bytes(want_plain[0])), f
    # Renderer.render_sequence(.., temporal=TemporalParams(clip=True), scenes=..) is this composition with the accumulator's defaults
    seq = sequence_of(name, f64)
    own, cam0, cfg = getattr(scenes, name)(0)
    r = Renderer(own, cam0).width(W).height(H).max_bounces(cfg["max_bounces"]).seed(3).num_samples(BATCHES)
    got = list(r.render_sequence([s[1] for s in seq], BATCHES, temporal=p, scenes=[s[0] for s in seq]))
    assert len(got) == FRAMES and all(np.array_equal(a, b) for a, b in zip(got, images))
    for s in seq:
        s[0].close()
    own.close()
    # quality: directions, never thresholds
    static, changed = quality_masks([fr[2]["depth"][..., 2] for fr in frames], converged, earlier)
    alone = color_bytes(frames[-1][3])
    rows = {k: (rms_levels(im, converged, changed), rms_levels(im, converged, static)) for k, im in (("alone", alone), ("plain", img_plain), ("clip", img))}
    print(f"{name} f64={f64} (device), 64 x 48, 8 frames of 4 x 1 spp against 512 spp, RMS in 8-bit levels (changed mask, static mask): "
          f"{int(changed.sum())} changed and {int(static.sum())} static pixels; alone {rows['alone'][0]:.2f} {rows['alone'][1]:.2f}, "
          f"accumulated {rows['plain'][0]:.2f} {rows['plain'][1]:.2f}, clipped {rows['clip'][0]:.2f} {rows['clip'][1]:.2f}; "
          f"{int(ref.last['clipped'].sum())} pixels clipped in the last frame")
    assert changed.sum() >= 30
    assert rows["clip"][0] < rows["plain"][0]
    assert rows["clip"][1] < rows["plain"][1] and rows["clip"][1] < rows["alone"][1]
    for t in (acc, clip_img, plain_img):
        t.close()
