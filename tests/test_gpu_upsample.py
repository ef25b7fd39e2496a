"""The guided upsampling (rpt_upsample*, rpt_image_bytes_device, rpt_buffer_upsampled_image, Renderer.render_upsampled and
render_sequence(upsample=..)) on the device against the numpy restatement of the definition in tests/upsample_ref.py.  Frames and
variances are compared bit for bit.  Bytes are equal to color_bytes of the restated frame, every one of them, as in
tests/test_gpu_temporal.py.

Low-resolution sizes: 1 x 1, 5 x 3, 33 x 17 (no 32 x 8 block divides s times it) and 32 x 24 (every scale's frame is whole blocks).
Every test runs under a time limit of its own: a step that hangs ends the process instead of letting the next one start."""
import faulthandler
import functools

import numpy as np
import pytest

from rpt_amd import (DenoiseParams, Denoiser, DeviceBuffer, Renderer, RptError, TemporalParams, UpsampleParams, color_bytes, image_bytes_device,
                     scenes, temporal_camera_record, temporal_motion_record, upsample, upsample_device)
from tests.denoise_ref import denoise_ref
from tests.temporal_motion_ref import MotionRef
from tests.upsample_ref import replicate, upsample_ref

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")
SIZES = [(1, 1), (5, 3), (33, 17), (32, 24)]
NAMES = ("albedo", "normal", "depth")


@pytest.fixture(autouse=True)
def time_limit():
    faulthandler.dump_traceback_later(120, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def garbage(seed, w, h, s):
    """lo_rgb, lo_var, lo_albedo, lo_normal, lo_depth, hi_albedo, hi_normal, hi_depth: regions with three ids, noise on top."""
    rng = np.random.default_rng(seed)

    def planes(hh, ww, k):
        ys, xs = np.mgrid[0:hh, 0:ww]
        region = (xs // (3 * k) + 2 * (ys // (2 * k))) % 3
        albedo = rng.choice([0.0, 0.25, 0.5, 0.9], (3, 3))[region]
        albedo[rng.uniform(size=(hh, ww)) < 0.1] = 0.0
        normal = rng.normal(size=(3, 3))[region] * 0.5 + rng.normal(size=(hh, ww, 3)) * 0.2
        depth = np.stack([2.0 + 0.5 * region + rng.normal(size=(hh, ww)) * 0.1, rng.choice([0.5, 1.0], (hh, ww)),
                          np.where(rng.uniform(size=(hh, ww)) < 0.1, 7.0, region.astype(np.float64))], axis=-1)
        return albedo, normal, depth

    lo = planes(h, w, 1)
    hi = planes(s * h, s * w, s)
    return (rng.uniform(0.0, 2.0, (h, w, 3)), rng.uniform(0.0, 0.05, (h, w)), *lo, *hi)


def same(a, b):
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def ref_of(case, p, **kw):
    return upsample_ref(*case, scale=p.scale, radius=p.radius, flags=p.flags, sigma_normal=p.sigma_normal, sigma_depth=p.sigma_depth, **kw)


def device_entry(case, p, want_var=True, stream=None):
    """rpt_upsample_device on torch tensors -> (out, out_var or None), outputs prefilled with 7."""
    import torch
    h, w = case[0].shape[:2]
    s = p.scale
    dev = [torch.from_numpy(np.ascontiguousarray(a)).cuda() if a is not None else None for a in case]
    out = torch.full((s * h, s * w, 3), 7.0, dtype=torch.float64, device="cuda")
    out_var = torch.full((s * h, s * w), 7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    upsample_device(w, h, *[t.data_ptr() if t is not None else 0 for t in dev], out.data_ptr(), out_var.data_ptr() if want_var else 0, params=p,
                    stream_ptr=stream.cuda_stream if stream is not None else 0)
    torch.cuda.synchronize()
    return out.cpu().numpy(), out_var.cpu().numpy()


def check(case, p, what):
    """Host entry and device entry against the restatement -> the restatement's (out, var)."""
    ref = ref_of(case, p)
    got = upsample(*case, params=p, return_variance=True)
    got_d = device_entry(case, p)
    for name, g in (("host entry", got), ("device entry", got_d)):
        for k, plane in enumerate(("colour", "variance")):
            bad = ~((g[k] == ref[k]) | (np.isnan(g[k]) & np.isnan(ref[k])))
            print(f"{what}, {name}: {plane}: {int(bad.sum())} of {bad.size} values differ")
    assert same(got[0], ref[0]) and same(got[1], ref[1]), what
    assert same(got_d[0], ref[0]) and same(got_d[1], ref[1]), what
    return ref


def bytes_match(got, frame, what):
    """got: (h, w, 3) uint8 of the device; frame: the restated fp64 frame."""
    want = color_bytes(frame)
    assert got.shape == want.shape and got.dtype == np.uint8
    diff = np.abs(got.astype(int) - want.astype(int))
    print(f"{what}: {int((diff != 0).sum())} of {diff.size} bytes differ, by at most {int(diff.max())}")
    assert np.array_equal(got, want), what


# (given planes: indices into the case) each term and flag alone, all together, nothing (every optional plane NULL)
SETTINGS = {
    "nothing": (dict(demodulate=False, match_id=False, sigma_normal=0.0, sigma_depth=0.0), (0,)),
    "variance alone": (dict(demodulate=False, match_id=False, sigma_normal=0.0, sigma_depth=0.0), (0, 1)),
    "normal alone": (dict(demodulate=False, match_id=False, sigma_normal=0.7, sigma_depth=0.0), (0, 1, 3, 6)),
    "depth alone": (dict(demodulate=False, match_id=False, sigma_normal=0.0, sigma_depth=0.4), (0, 1, 4, 7)),
    "id alone": (dict(demodulate=False, match_id=True, sigma_normal=0.0, sigma_depth=0.0), (0, 1, 4, 7)),
    "demodulation alone": (dict(demodulate=True, match_id=False, sigma_normal=0.0, sigma_depth=0.0), (0, 1, 2, 5)),
    "all": (dict(demodulate=True, match_id=True, sigma_normal=0.7, sigma_depth=0.4), tuple(range(8))),
    "all planes given, the defaults": (dict(), tuple(range(8))),
}


# ---- 1 + 2: garbage planes, every size, scale, radius and setting; NULL planes
@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("s", [2, 3, 4])
@pytest.mark.parametrize("r", [1, 2])
def test_garbage_planes_equal_the_restatement(w, h, s, r):
    case = garbage(1000 * s + 100 * r + w, w, h, s)
    fell = 0
    for name, (kw, given) in SETTINGS.items():
        p = UpsampleParams(scale=s, radius=r, **kw)
        sub = [a if k in given else None for k, a in enumerate(case)]
        check(sub, p, f"{w} x {h}, s {s}, r {r}, {name}")
        fell += int(ref_of(sub, p, return_fallback=True)[2].sum())
    if (w, h) == (33, 17):
        assert fell > 0                                         # the fallback is exercised (ids that match no tap)


def test_null_out_var_leaves_the_frame_alone():
    case = garbage(5, 33, 17, 3)
    p = UpsampleParams(scale=3, radius=2, sigma_normal=0.7, sigma_depth=0.4)
    ref = ref_of(case, p)
    out, untouched = device_entry(case, p, want_var=False)
    assert same(out, ref[0]) and float(untouched.min()) == 7.0 and float(untouched.max()) == 7.0
    assert same(upsample(*case, params=p), ref[0])
    with pytest.raises(RptError, match="needs the full-resolution normal"):
        upsample(*case[:6], None, case[7], params=p)
    with pytest.raises(RptError, match="output must not"):
        import torch
        t = torch.zeros(33 * 17 * 9 * 3, dtype=torch.float64, device="cuda")
        upsample_device(33, 17, t.data_ptr(), 0, 0, 0, 0, 0, 0, 0, t.data_ptr(), 0, params=UpsampleParams(scale=3, demodulate=False, match_id=False,
                                                                                                      sigma_normal=0.0))


# ---- 3: NaN and inf
@pytest.mark.parametrize("what", ["colour", "variance", "normal", "depth", "id", "albedo"])
def test_nan_and_inf_pixels(what):
    s, w, h = 2, 33, 17
    case = [a.copy() for a in garbage(21, w, h, s)]
    spots = [(16, 8), (0, 0), (32, 16), (15, 3)]                 # low-resolution pixels: interior, two corners, a block corner
    for k, (x, y) in enumerate(spots):
        bad = NAN if k % 2 == 0 else INF
        if what == "colour":
            case[0][y, x, k % 3] = bad
        elif what == "variance":
            case[1][y, x] = bad
        elif what == "normal":
            case[3][y, x, k % 3] = bad
            case[6][s * y, s * x, k % 3] = bad
        elif what == "depth":
            case[4][y, x, 0] = bad
            case[7][s * y + 1, s * x, 0] = bad
        elif what == "id":
            case[4][y, x, 2] = bad
            case[7][s * y, s * x + 1, 2] = bad
        else:
            case[2][y, x, k % 3] = bad
            case[5][s * y, s * x, k % 3] = bad
    for r in (1, 2):
        out, v = check(case, UpsampleParams(scale=s, radius=r, sigma_normal=0.7, sigma_depth=0.4), f"NaN / inf {what}, r {r}")
        if what in ("normal", "depth", "id"):                    # a bad guide value skips taps; it never reaches a colour
            assert np.isfinite(out).all() and np.isfinite(v).all()


# ---- 4: streams
def test_two_calls_on_two_alternating_streams():
    import torch
    ps = [UpsampleParams(scale=2, radius=1, sigma_normal=0.7), UpsampleParams(scale=4, radius=2, sigma_depth=0.4),
          UpsampleParams(scale=3, radius=2, demodulate=False), UpsampleParams(scale=2, radius=2, match_id=False, sigma_normal=0.3)]
    cases = [garbage(40 + k, 33, 17, p.scale) for k, p in enumerate(ps)]
    refs = [ref_of(c, p) for c, p in zip(cases, ps)]
    dev = [[torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in c] for c in cases]
    outs = [(torch.full((17 * p.scale, 33 * p.scale, 3), 7.0, dtype=torch.float64, device="cuda"),
             torch.full((17 * p.scale, 33 * p.scale), 7.0, dtype=torch.float64, device="cuda")) for p in ps]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]         # (torch's streams are non-blocking)
    torch.cuda.synchronize()
    for k, p in enumerate(ps):
        upsample_device(33, 17, *[t.data_ptr() for t in dev[k]], outs[k][0].data_ptr(), outs[k][1].data_ptr(), params=p,
                        stream_ptr=streams[k % 2].cuda_stream)
    torch.cuda.synchronize()
    for k, (o, v) in enumerate(outs):
        assert same(o.cpu().numpy(), refs[k][0]) and same(v.cpu().numpy(), refs[k][1]), k


# ---- 5: bytes
def test_image_bytes_device_is_color_bytes():
    import torch
    rng = np.random.default_rng(51)
    frame = rng.uniform(-0.2, 1.3, (45, 70, 3))
    frame[0, 0], frame[3, 5, 1], frame[44, 69, 2], frame[7, 7, 0] = [0.0, 1.0, 0.5], NAN, INF, -INF
    t = torch.from_numpy(frame).cuda()
    torch.cuda.synchronize()
    bytes_match(image_bytes_device(t.data_ptr(), 70, 45), frame, "image_bytes_device, default stream")
    s = torch.cuda.Stream()
    bytes_match(image_bytes_device(t.data_ptr(), 70, 45, stream_ptr=s.cuda_stream), frame, "image_bytes_device, a stream of its own")
    with pytest.raises(RptError, match="null"):
        image_bytes_device(0, 70, 45)


@functools.lru_cache(maxsize=None)
def rendered(name, f64, w, h, s, seed=3, guide=1):
    """4 batches x 4 spp of a scene at w x h in a DeviceBuffer, the low-resolution planes of the same 16 samples, the full-resolution
    planes of `guide` samples -> buffer, lo planes, hi planes, mean, variance."""
    scene, cam, cfg = getattr(scenes, name)()
    if f64:
        scene.set_option("epsilon_policy", 1)
    r = Renderer(scene, cam).width(w).height(h).max_bounces(cfg["max_bounces"]).seed(seed)
    lo = r.features_array(16, sample_offset=0)
    hi = Renderer(scene, cam).width(s * w).height(s * h).max_bounces(cfg["max_bounces"]).seed(seed).features_array(guide, sample_offset=0)
    buf = DeviceBuffer(w, h)
    for _ in range(4):
        r.sample(4, buf)
    rgb, var = buf.mean()
    for a in (rgb, var, *lo.values(), *hi.values()):
        a.setflags(write=False)
    return buf, lo, hi, rgb, var


def restated(rgb, var, lo, hi, p, denoise=None, **kw):
    """The composition rpt_buffer_upsampled_image runs: (filter at the low resolution) -> upsample."""
    if denoise is not None:
        rgb, var = denoise_ref(rgb, var, lo["albedo"], lo["normal"], lo["depth"], passes=denoise.passes, flags=denoise.flags,
                               sigma_color=denoise.sigma_color, sigma_normal=denoise.sigma_normal, sigma_depth=denoise.sigma_depth)
    return ref_of((rgb, var, *[lo[k] for k in NAMES], *[hi[k] for k in NAMES]), p, **kw)


@pytest.mark.parametrize("s", [2, 3])
def test_buffer_upsampled_image_with_and_without_the_low_resolution_filter(s):
    w, h = 35, 23
    buf, lo, hi, rgb, var = rendered("cornell", False, w, h, s)
    p = UpsampleParams(scale=s)
    bytes_match(buf.upsampled_image(lo, hi, p), restated(rgb, var, lo, hi, p)[0], f"upsampled_image, s {s}")
    dp = DenoiseParams(passes=2)
    den = Denoiser(w, h)
    bytes_match(buf.upsampled_image(lo, hi, p, den, dp), restated(rgb, var, lo, hi, p, dp)[0], f"upsampled_image, s {s}, filtered at the low resolution")
    with pytest.raises(RptError, match="sizes"):
        buf.upsampled_image(lo, hi, p, Denoiser(5, 3), dp)
    with pytest.raises(RptError, match="needs the full-resolution normal"):
        buf.upsampled_image(lo, {"albedo": hi["albedo"], "depth": hi["depth"]}, p)
    with pytest.raises(ValueError):
        buf.upsampled_image(lo, {"albedo": lo["albedo"]}, UpsampleParams(scale=s, match_id=False, sigma_normal=0.0))
    empty = DeviceBuffer(w, h)
    empty.add_samples(np.zeros((w * h, 3)))
    with pytest.raises(RptError, match="2 batches"):            # RPT_ERR_STATE
        empty.upsampled_image(lo, hi, p)


# ---- 6: rendered frames of both modes through Renderer.render_upsampled
@pytest.mark.parametrize("name,f64", [("cornell", False), ("cornell", True), ("lampshade", False), ("lampshade", True)])
def test_render_upsampled_is_the_restatement_on_the_device_s_own_frames(name, f64):
    w, h, s = 32, 24, 2
    buf, lo, hi, rgb, var = rendered(name, f64, w, h, s)
    scene, cam, cfg = getattr(scenes, name)()
    if f64:
        scene.set_option("epsilon_policy", 1)
    r = Renderer(scene, cam).width(s * w).height(s * h).max_bounces(cfg["max_bounces"]).seed(3).num_samples(16)
    p = UpsampleParams()
    frame, _, fb = restated(rgb, var, lo, hi, p, return_fallback=True)
    assert np.isfinite(frame).all() and fb.mean() < 0.5
    bytes_match(r.render_upsampled(), frame, f"render_upsampled {name} f64={f64}")
    assert (r.width_, r.height_) == (s * w, s * h)
    dp = DenoiseParams(passes=3)
    bytes_match(r.render_upsampled(p, 4, dp), restated(rgb, var, lo, hi, p, dp)[0], f"render_upsampled {name} f64={f64}, filtered")


# ---- 7: sequences
def test_render_sequence_with_upsample_equals_the_restatement():
    """Three frames of scenes.simple_video at 32 x 24 -> 64 x 48: the restated upsampled frame and variance of every frame fed to
    tests/temporal_motion_ref.py with the full-resolution normal and depth planes and the frame's motion table."""
    w, h, s, spp = 32, 24, 2, 4
    W, H = s * w, s * h
    seq = [scenes.simple_video(1 + f, 0.5) for f in range(3)]
    tables = [None] + [np.stack([temporal_motion_record(c.shape.matrix(), q.shape.matrix()) for c, q in zip(cur[0].objects, prev[0].objects)])
                       for prev, cur in zip(seq, seq[1:])]
    p, tp, ref = UpsampleParams(), TemporalParams(), MotionRef(W, H)
    want, want_filtered, ref2 = [], [], MotionRef(W, H)
    for f, ((scene, cam, cfg), table) in enumerate(zip(seq, tables)):
        lo_r = Renderer(scene, cam).width(w).height(h).max_bounces(cfg["max_bounces"]).seed(3)
        hi_r = Renderer(scene, cam).width(W).height(H).max_bounces(cfg["max_bounces"]).seed(3)
        lo = lo_r.features_array(4 * spp, sample_offset=f * 4 * spp)
        hi = hi_r.features_array(1, sample_offset=f * 4 * spp)
        lo_r._sample_offset = f * 4 * spp
        buf = DeviceBuffer(w, h)
        for _ in range(4):
            lo_r.sample(spp, buf)
        rgb, var = buf.mean()
        up, up_var = restated(rgb, var, lo, hi, p)
        kw = dict(max_history=tp.max_history, flags=tp.flags, depth_tol=tp.depth_tol, normal_tol=tp.normal_tol)
        acc = ref.accumulate(temporal_camera_record(cam), up, up_var, hi["normal"], hi["depth"], motion=table, **kw)
        want.append(acc[0])
        acc = ref2.accumulate(temporal_camera_record(cam), up, up_var, hi["normal"], hi["depth"], motion=table, **kw)
        want_filtered.append(denoise_ref(acc[0], acc[1], hi["albedo"], hi["normal"], hi["depth"])[0])
        if f:
            print(f"frame {f}: {int(ref.last['took'].sum())} of {W * H} pixels take history")
            assert ref.last["took"].sum() > 0                   # (the accumulation is not vacuous; half the frame is sky, which has no history)
        buf.close()
    own, cam0, cfg = scenes.simple_video(0)
    r = Renderer(own, cam0).width(W).height(H).max_bounces(cfg["max_bounces"]).seed(3).num_samples(4 * spp)
    got = list(r.render_sequence([q[1] for q in seq], 4, scenes=[q[0] for q in seq], upsample=p))
    assert r.scene is own and r.camera is cam0 and len(got) == 3
    for f in range(3):
        bytes_match(got[f], want[f], f"render_sequence(upsample), frame {f}")
    seq2 = [scenes.simple_video(1 + f, 0.5) for f in range(3)]
    got = list(r.render_sequence([q[1] for q in seq2], 4, denoise=DenoiseParams(), scenes=[q[0] for q in seq2], upsample=p))
    for f in range(3):
        bytes_match(got[f], want_filtered[f], f"render_sequence(upsample, denoise), frame {f}")
    for q in seq + seq2:
        q[0].close()


# ---- 8: quality.  Conditions, not tolerances (tests/test_upsample_host.py holds the restatement to the same two on the oracle's frames)
def test_the_device_s_frames_reconstruct_rather_than_fall_back():
    """scenes.lampshade() (tests/test_upsample_host.py says why not spheres) at 64 x 48 -> 128 x 96, s = 2 with the defaults: at
    most 5 % of the pixels take the fallback, and the upsampled frame is closer to the 512-spp full-resolution frame than s x s
    replication of the same low-resolution frame is."""
    w, h, s = 64, 48, 2
    buf, lo, hi, rgb, var = rendered("lampshade", False, w, h, s)
    p = UpsampleParams()
    _, _, fb = restated(rgb, var, lo, hi, p, return_fallback=True)
    got = buf.upsampled_image(lo, hi, p)
    scene, cam, cfg = scenes.lampshade()
    make = lambda seed, spp: Renderer(scene, cam).width(s * w).height(s * h).max_bounces(cfg["max_bounces"]).seed(seed).num_samples(spp)  # noqa: E731
    converged = make(1234, 512).render().astype(np.float64)
    rms = lambda a: float(np.sqrt(np.mean((a.astype(np.float64) - converged) ** 2)))  # noqa: E731
    plain = color_bytes(replicate(rgb, s))
    print(f"quality, lampshade 64 x 48 -> 128 x 96, 4 batches x 4 spp against 512 spp: fallback {100.0 * fb.mean():.2f} %, RMS {rms(got):.2f} levels, "
          f"replication {rms(plain):.2f}")
    assert fb.mean() <= 0.05
    assert rms(got) < rms(plain)
    # Renderer.render_upsampled is this composition
    assert np.array_equal(make(3, 16).render_upsampled(), got)
