"""Temporal accumulation (rpt_temporal_*) on the device against the numpy restatement of the definition in tests/temporal_ref.py.
Equality is bit for bit -- colour, variance and history length of every frame of a sequence; the frames after the first pin the
records the device stored -- unless a test says otherwise.  The cameras reach the device as rpt_camera and the restatement as the
record rpt_temporal_camera_record makes of them (a host function), so no test depends on two tan implementations agreeing.

tests/test_temporal_host.py shows on the same analytic scene that the restatement reprojects (an unmoved camera maps every pixel onto
itself, a moved one takes history at 3066 of 3072 pixels); the counts are asserted here again on what the device was compared with."""
import functools

import numpy as np
import pytest

from rpt_amd import (DenoiseParams, Denoiser, DeviceBuffer, Renderer, RptError, TemporalAccumulator, TemporalParams, color_bytes, scenes,
                     temporal_camera_record)
from tests.denoise_ref import denoise_ref
from tests.temporal_ref import TemporalRef, analytic_cameras, analytic_planes, arc_cameras, garbage, sequence

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")
SIZES = [(1, 1), (5, 3), (33, 17), (64, 48)]


def same(a, b):
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def ref_kw(p):
    return dict(max_history=p.max_history, flags=p.flags, depth_tol=p.depth_tol, normal_tol=p.normal_tol)


def frames_of(make, seed, w, h, n=4):
    """-> the cameras and make()'s frames for their records."""
    cams = analytic_cameras(n)
    return cams, make(seed, w, h, [temporal_camera_record(c) for c in cams])


def check(cams, frames, w, h, what, use_var=True, **kw):
    """The host entry point, frame by frame, against the restatement -> the restatement's accumulator and its outputs."""
    p = TemporalParams(**kw)
    acc, ref, outs = TemporalAccumulator(w, h), TemporalRef(w, h), []
    assert acc.frames == 0
    for f, (cam, (rec, rgb, var, normal, depth)) in enumerate(zip(cams, frames)):
        var = var if use_var else None
        normal = normal if p.normal_tol > 0.0 else None
        got = acc.accumulate(cam, rgb, var, normal, depth, params=p, return_variance=True, return_length=True)
        want = ref.accumulate(rec, rgb, var, normal, depth, **ref_kw(p))
        for k, name in enumerate(("colour", "variance", "len")):
            bad = ~((got[k] == want[k]) | (np.isnan(got[k]) & np.isnan(want[k])))
            print(f"{what}, frame {f}: {name}: {int(bad.sum())} of {bad.size} values differ; {int(ref.last['took'].sum())} pixels took history")
        assert all(same(got[k], want[k]) for k in range(3)), (what, f)
        assert acc.frames == f + 1
        outs.append((want, ref.last))
    acc.close()
    return outs


# ---- 1: the analytic scene over four frames of a moving camera, random radiance and variance, every size
@pytest.mark.parametrize("w,h", SIZES)
def test_analytic_scene_equals_the_restatement(w, h):
    cams, frames = frames_of(sequence, 100 + w, w, h)
    outs = check(cams, frames, w, h, f"analytic {w} x {h}")
    if (w, h) == (64, 48):
        for (out, v, length), last in outs[1:]:
            assert last["took"].sum() > 0.85 * w * h                    # (the sprinkled misses, ids and NaNs take some away)
        assert abs(outs[-1][0][2].max() - 4.0) < 1e-9


# ---- 2: planes that belong to no scene
@pytest.mark.parametrize("w,h", SIZES)
def test_random_garbage_planes_equal_the_restatement(w, h):
    cams, frames = frames_of(garbage, 200 + w, w, h)
    outs = check(cams, frames, w, h, f"garbage {w} x {h}", depth_tol=0.0, normal_tol=0.0, match_id=False)
    check(cams, frames, w, h, f"garbage {w} x {h}, every test on", depth_tol=0.5, normal_tol=1.5)
    if (w, h) == (64, 48):
        assert sum(int(last["took"].sum()) for _, last in outs) > 100   # some of it lands inside the frame


# ---- 3: each test and flag alone, NULL var, max_history 1, 2 and 16
SETTINGS = {
    "defaults": dict(),
    "nothing": dict(match_id=False, depth_tol=0.0, normal_tol=0.0),
    "id alone": dict(match_id=True, depth_tol=0.0, normal_tol=0.0),
    "depth alone": dict(match_id=False, depth_tol=0.02, normal_tol=0.0),
    "normal alone": dict(match_id=False, depth_tol=0.0, normal_tol=0.2),
    "no id match": dict(match_id=False),
    "max_history 1": dict(max_history=1),
    "max_history 2": dict(max_history=2),
    "max_history 16": dict(max_history=16),
    "max_history 4096": dict(max_history=4096),
}


@pytest.mark.parametrize("name", list(SETTINGS))
def test_tests_flags_and_history_lengths(name):
    w, h = 33, 17
    cams, frames = frames_of(sequence, 300, w, h)
    outs = check(cams, frames, w, h, name, **SETTINGS[name])
    check(cams, frames, w, h, name + ", no variance", use_var=False, **SETTINGS[name])
    cap = SETTINGS[name].get("max_history", 16)
    assert abs(outs[-1][0][2].max() - min(4.0, cap)) < 1e-9 and outs[-1][1]["took"].sum() > w * h // 2


def test_optional_outputs_and_reset():
    """The outputs do not depend on which optional outputs are asked for; a reset forgets the history."""
    w, h = 33, 17
    cams, frames = frames_of(sequence, 301, w, h)
    a, b, ref = TemporalAccumulator(w, h), TemporalAccumulator(w, h), TemporalRef(w, h)
    for cam, (rec, rgb, var, normal, depth) in zip(cams, frames):
        full = a.accumulate(cam, rgb, var, normal, depth, return_variance=True, return_length=True)
        bare = b.accumulate(cam, rgb, var, normal, depth)
        assert same(full[0], bare) and same(bare, ref.accumulate(rec, rgb, var, normal, depth)[0])
    a.reset()
    ref.reset()
    assert a.frames == 0 and b.frames == 4
    rec, rgb, var, normal, depth = frames[1]
    out, v, length = a.accumulate(cams[1], rgb, var, normal, depth, return_variance=True, return_length=True)
    assert same(out, rgb) and same(v, var) and (length == 1.0).all() and a.frames == 1
    ref.accumulate(rec, rgb, var, normal, depth)
    rec, rgb, var, normal, depth = frames[2]
    got = a.accumulate(cams[2], rgb, var, normal, depth, return_variance=True, return_length=True)
    want = ref.accumulate(rec, rgb, var, normal, depth)
    assert all(same(got[k], want[k]) for k in range(3)) and got[2].max() == 2.0
    with pytest.raises(RptError, match="normal_tol"):
        a.accumulate(cams[2], rgb, var, None, depth)
    with pytest.raises(RptError, match="normal_tol"):
        a.accumulate(cams[2], rgb, var, normal, depth, params=TemporalParams(normal_tol=0.0))
    assert a.frames == 2                                                # a refused call leaves the history alone
    a.close()
    b.close()


# ---- 4: NaN and inf
@pytest.mark.parametrize("what", ["colour", "variance", "depth", "coverage", "id"])
def test_nan_and_inf_pixels(what):
    """Frames 0 and 1 share a camera, so a pixel's own record is the tap that carries the weight; the spots have ids of their own
    in both frames, so the neighbours' records (weights of 1e-13, fx is x only up to rounding) are refused and what the spot takes
    in frame 1 is what its own record of frame 0 lends: nothing."""
    w, h = 64, 48
    cams = analytic_cameras(2)
    cams = [cams[0], cams[0], cams[1]]
    recs = [temporal_camera_record(c) for c in cams]
    frames = [list(f) for f in sequence(400, w, h, recs)]
    normal0, depth0 = analytic_planes(recs[0], w, h)
    spots = [(33, 20), (0, 0), (63, 47), (16, 15)]                      # interior, two corners, a block corner
    for k, (x, y) in enumerate(spots):
        bad = NAN if k % 2 == 0 else INF
        for f in (0, 1):
            rec, rgb, var, normal, depth = frames[f]
            rgb[y, x], var[y, x], normal[y, x], depth[y, x] = 0.5, 0.01, normal0[y, x], depth0[y, x]
            depth[y, x, 2] = 50.0 + k
        rec, rgb, var, normal, depth = frames[0]
        if what == "colour":
            rgb[y, x, k % 3] = bad
        elif what == "variance":
            var[y, x] = bad
        elif what == "depth":
            depth[y, x, 0] = bad
        elif what == "coverage":
            depth[y, x, 1] = bad
        else:
            depth[y, x, 2] = bad if bad != bad else 77.0                # (an infinite id is an id like another)
    outs = check(cams, frames, w, h, f"NaN / inf {what}")
    (out0, v0, len0), _ = outs[0]
    (out1, v1, len1), last1 = outs[1]
    for k, (x, y) in enumerate(spots):
        if what == "colour":
            assert not np.isfinite(out0[y, x]).all()                    # in its own output, once
        if what == "variance":
            assert not np.isfinite(v0[y, x])
        assert len1[y, x] == 1.0 and not last1["took"][y, x], (what, x, y)         # nothing outlives the frame
        assert same(out1[y, x], np.full(3, 0.5)) and v1[y, x] == 0.01
    # and the control: the same spots with nothing bad take their own history
    frames[0][1][:], frames[0][2][:] = np.nan_to_num(frames[0][1], nan=0.5, posinf=0.5), np.nan_to_num(frames[0][2], nan=0.01, posinf=0.01)
    for k, (x, y) in enumerate(spots):
        frames[0][4][y, x] = depth0[y, x]
        frames[0][4][y, x, 2] = 50.0 + k
    (_, _, len1), last1 = check(cams, frames, w, h, f"NaN / inf {what}, control")[1]
    assert all(len1[y, x] == 2.0 and last1["took"][y, x] for x, y in spots)


# ---- 5: entry points and streams
def test_host_and_device_entries_agree_and_streams_are_ordered():
    import torch
    w, h = 64, 48
    cams, fa = frames_of(sequence, 500, w, h)
    _, fb = frames_of(garbage, 501, w, h)
    pa, pb = TemporalParams(), TemporalParams(max_history=3, match_id=False, depth_tol=0.5, normal_tol=0.0)
    ra, rb = TemporalRef(w, h), TemporalRef(w, h)
    wa = [ra.accumulate(*f, **ref_kw(pa)) for f in fa]
    wb = [rb.accumulate(f[0], f[1], f[2], None, f[4], **ref_kw(pb)) for f in fb]
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    da = [[up(a) for a in f[1:]] for f in fa]
    db = [[up(a) for a in f[1:]] for f in fb]
    new = lambda n: torch.full((n,), 7.0, dtype=torch.float64, device="cuda")  # noqa: E731
    oa = [(new(h * w * 3), new(h * w), new(h * w)) for _ in fa]
    ob = [(new(h * w * 3), new(h * w), new(h * w)) for _ in fb]
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    a, b = TemporalAccumulator(w, h), TemporalAccumulator(w, h)
    # two accumulators on two streams; each one's calls alternate between the streams and wait for their own predecessor
    for f in range(4):
        sa, sb = (s1, s2) if f % 2 == 0 else (s2, s1)
        rgb, var, normal, depth = da[f]
        a.accumulate_device(cams[f], rgb.data_ptr(), var.data_ptr(), normal.data_ptr(), depth.data_ptr(), oa[f][0].data_ptr(), oa[f][1].data_ptr(),
                            oa[f][2].data_ptr(), params=pa, stream_ptr=sa.cuda_stream)
        rgb, var, normal, depth = db[f]
        b.accumulate_device(cams[f], rgb.data_ptr(), var.data_ptr(), 0, depth.data_ptr(), ob[f][0].data_ptr(), 0, ob[f][2].data_ptr(),
                            params=pb, stream_ptr=sb.cuda_stream)
    torch.cuda.synchronize()
    assert a.frames == b.frames == 4
    host = TemporalAccumulator(w, h)
    for f in range(4):
        got = [t.cpu().numpy() for t in oa[f]]
        assert same(got[0].reshape(h, w, 3), wa[f][0]) and same(got[1].reshape(h, w), wa[f][1]) and same(got[2].reshape(h, w), wa[f][2]), f
        got = [t.cpu().numpy() for t in ob[f]]
        assert same(got[0].reshape(h, w, 3), wb[f][0]) and float(got[1].min()) == float(got[1].max()) == 7.0     # NULL: not written
        assert same(got[2].reshape(h, w), wb[f][2]), f
        # the host entry point: the same bits
        rec, rgb, var, normal, depth = fa[f]
        again = host.accumulate(cams[f], rgb, var, normal, depth, params=pa, return_variance=True, return_length=True)
        assert all(same(again[k], wa[f][k]) for k in range(3))
    with pytest.raises(RptError, match="output"):                       # an output that is an input
        a.accumulate_device(cams[0], da[0][0].data_ptr(), da[0][1].data_ptr(), da[0][2].data_ptr(), da[0][3].data_ptr(), da[0][0].data_ptr())
    for t in (a, b, host):
        t.close()


# ---- 6: rendered frames
W = H = 64
CORNELL_DISTANCE = 1080.0     # from the eye of scenes._cornell_camera to the middle of the box


@functools.lru_cache(maxsize=None)
def rendered(name, f64, n_frames, spp, seed=3, step=0.02):
    """n_frames cameras on a small arc; per frame 4 batches of spp samples in a DeviceBuffer at the sample offsets that follow the
    previous frame's, and the feature planes of the same samples -> [(camera, buffer, planes, mean, variance)]."""
    scene, cam, cfg = getattr(scenes, name)()
    if f64:
        scene.set_option("epsilon_policy", 1)
    cams = arc_cameras(cam, n_frames, CORNELL_DISTANCE, step)
    r = Renderer(scene, cams[0]).width(W).height(H).max_bounces(cfg["max_bounces"]).seed(seed)
    frames = []
    for c in cams:
        r.camera = c
        planes = r.features_array(4 * spp)                              # of the samples the next calls trace
        buf = DeviceBuffer(W, H)
        for _ in range(4):
            r.sample(spp, buf)
        rgb, var = buf.mean()
        for a in (rgb, var, *planes.values()):
            a.setflags(write=False)
        frames.append((c, buf, planes, rgb, var))
    return frames


@pytest.mark.parametrize("name,f64", [("cornell", False), ("cornell", True), ("lampshade", False), ("lampshade", True)])
def test_rendered_frames(name, f64):
    frames = rendered(name, f64, 3, 4)
    acc, plain, filtered = [TemporalAccumulator(W, H) for _ in range(3)]
    denoiser, ref = Denoiser(W, H), TemporalRef(W, H)
    p = TemporalParams()
    for f, (cam, buf, planes, rgb, var) in enumerate(frames):
        got = acc.accumulate(cam, rgb, var, planes["normal"], planes["depth"], return_variance=True, return_length=True)
        want = ref.accumulate(temporal_camera_record(cam), rgb, var, planes["normal"], planes["depth"], **ref_kw(p))
        took, hit = ref.last["took"], ref.last["hit"]
        print(f"{name} f64={f64}, frame {f}: {int(took.sum())} of {int(hit.sum())} hit pixels take history, mean len {want[2].mean():.2f}")
        assert all(same(got[k], want[k]) for k in range(3)), f
        if f:
            assert took.sum() > 0.8 * hit.sum()
        # rpt_temporal_frame_image: the same frame as bytes, without and with the filter (which takes the accumulated variance)
        img = buf.temporal_image(plain, cam, planes)
        assert img.shape == (H, W, 3) and img.dtype == np.uint8
        assert np.array_equal(img, color_bytes(want[0])), f
        den, _ = denoise_ref(want[0], want[1], planes["albedo"], planes["normal"], planes["depth"])
        img = buf.temporal_image(filtered, cam, planes, denoiser=denoiser)
        assert np.array_equal(img, color_bytes(den)), f
    assert acc.frames == plain.frames == filtered.frames == 3
    for t in (acc, plain, filtered, denoiser):
        t.close()


def test_frame_image_refusals():
    cam, buf, planes, rgb, var = rendered("cornell", False, 3, 4)[0]
    acc = TemporalAccumulator(W, H)
    with pytest.raises(RptError, match="normal"):
        buf.temporal_image(acc, cam, {"depth": planes["depth"]})
    with pytest.raises(RptError, match="depth"):
        buf.temporal_image(acc, cam, {"normal": planes["normal"]})
    with pytest.raises(RptError, match="albedo"):                       # the filter's own needs
        buf.temporal_image(acc, cam, {"normal": planes["normal"], "depth": planes["depth"]}, denoiser=Denoiser(W, H))
    with pytest.raises(ValueError):
        buf.temporal_image(acc, cam, {"colour": planes["albedo"]})
    small, one = TemporalAccumulator(5, 3), DeviceBuffer(W, H)
    with pytest.raises(RptError, match="sizes"):
        buf.temporal_image(small, cam, planes)
    with pytest.raises(RptError, match="sizes"):
        buf.temporal_image(acc, cam, planes, denoiser=Denoiser(5, 3))
    one.add_samples(np.zeros((H * W, 3)))
    with pytest.raises(RptError, match="2 batches"):                    # RPT_ERR_STATE
        one.temporal_image(acc, cam, planes)
    assert acc.frames == 0 and small.frames == 0
    # normal_tol == 0: the accumulation takes no normal plane, whether the caller has one or not
    img = buf.temporal_image(acc, cam, {"depth": planes["depth"]}, TemporalParams(normal_tol=0.0))
    assert np.array_equal(img, color_bytes(rgb)) and acc.frames == 1


# ---- 7: quality.  A condition, not a tolerance: after eight frames of 4 x 1 spp the accumulated frame is closer to a converged one
# than the last frame alone.  (tools/temporal_quality.py --cpu: the restatement on the oracle's renders satisfies it; DESIGN.md
# section 4, "Temporal accumulation", has both ratios.)
@pytest.mark.parametrize("name", ["cornell", "lampshade"])
def test_accumulated_frame_is_closer_to_the_converged_one(name):
    frames = rendered(name, False, 8, 1)
    acc, acc2, denoiser = TemporalAccumulator(W, H), TemporalAccumulator(W, H), Denoiser(W, H)
    for cam, buf, planes, rgb, var in frames:
        accumulated = buf.temporal_image(acc, cam, planes)
        both = buf.temporal_image(acc2, cam, planes, denoiser=denoiser)
    cam, buf, planes, rgb, var = frames[-1]
    alone = buf.image()                                                  # Filter::Box(0): color_bytes of the last frame's mean
    filtered = buf.denoised_image(denoiser, planes)
    scene, _, cfg = getattr(scenes, name)()
    make = lambda c, seed, spp: Renderer(scene, c).width(W).height(H).max_bounces(cfg["max_bounces"]).seed(seed).num_samples(spp)  # noqa: E731
    converged = make(cam, 1234, 512).render()
    rms = lambda a: float(np.sqrt(np.mean((a.astype(np.float64) - converged.astype(np.float64)) ** 2)))  # noqa: E731
    print(f"quality, {name} 64 x 64, 8 frames of 4 x 1 spp against 512 spp: RMS {rms(alone):.2f} -> {rms(accumulated):.2f} levels, "
          f"ratio {rms(accumulated) / rms(alone):.3f}; denoise alone {rms(filtered):.2f}, accumulate + denoise {rms(both):.2f}, "
          f"ratio {rms(both) / rms(filtered):.3f}")
    assert rms(accumulated) < rms(alone)
    # Renderer.render_sequence is this composition
    seq = list(make(cam, 3, 4).render_sequence([f[0] for f in frames], 4))
    assert len(seq) == 8 and np.array_equal(seq[-1], accumulated)
    seq = list(make(cam, 3, 4).render_sequence([f[0] for f in frames], 4, denoise=DenoiseParams()))
    assert np.array_equal(seq[-1], both)
    for t in (acc, acc2, denoiser):
        t.close()
