"""The a-trous denoiser (rpt_denoise*, rpt_buffer_mean_device, rpt_buffer_denoised_image) on the device against the numpy restatement
of the definition in tests/denoise_ref.py.  Equality is bit for bit, for the colour and for the output variance, unless a test says
otherwise.

Frames are 70 x 45 as in tests/test_gpu_features.py: 5 x 3 blocks of 16 x 16 pixels, clipped on both edges; at 5 passes the +-32
taps of step 16 are clipped on every side.  Every comparison runs with "denoise_stage" 0 (the taps gathered from global memory),
1 and 2 (the passes of step <= 1, <= 2 stage their tile and halo in LDS)."""
import functools

import numpy as np
import pytest

from rpt_amd import DenoiseParams, Denoiser, DeviceBuffer, Renderer, RptError, _lib, color_bytes, scenes
from tests.denoise_ref import denoise_ref

pytestmark = pytest.mark.gpu

W, H = 70, 45
STAGES = (0, 1, 2)
NAN, INF = float("nan"), float("inf")


@functools.lru_cache(maxsize=None)
def denoiser(w, h, stage, copy=0):
    """One denoiser per frame size and "denoise_stage" (the option is read at rpt_denoiser_create), shared by the tests."""
    lib = _lib.load()
    _lib.check(lib.rpt_set_option(b"denoise_stage", stage))
    try:
        return Denoiser(w, h)
    finally:
        _lib.check(lib.rpt_set_option(b"denoise_stage", -1))


def frames(seed, w=W, h=H):
    """Seeded frame, variance and planes: regions of 9 x 7 pixels with five ids, a colour and a normal of their own, noise on top."""
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:h, 0:w]
    region = (xs // 9 + 2 * (ys // 7)) % 5
    albedo = rng.uniform(0.1, 0.9, (5, 3))[region]
    albedo[rng.uniform(size=(h, w)) < 0.05] = 0.0                       # den = 1 there
    var = rng.uniform(0.0, 0.02, (h, w)) * rng.choice([0.0, 1.0, 4.0], (h, w))
    rgb = albedo * rng.uniform(0.5, 1.5, (5, 1))[region] + rng.normal(size=(h, w, 3)) * np.sqrt(var)[..., None]
    normal = rng.normal(size=(5, 3))[region] * 0.5 + rng.normal(size=(h, w, 3)) * 0.05
    depth = np.stack([2.0 + 0.02 * xs + 0.5 * region + rng.normal(size=(h, w)) * 0.01, rng.choice([0.5, 1.0], (h, w)),
                      region.astype(np.float64)], axis=-1)
    return rgb, var, albedo, normal, depth


def same(a, b):
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def check(case, what, w=W, h=H, **kw):
    """The device's result for every stage setting against the restatement -> the restatement's."""
    p = DenoiseParams(**kw)
    ref = denoise_ref(*case, passes=p.passes, flags=p.flags, sigma_color=p.sigma_color, sigma_normal=p.sigma_normal, sigma_depth=p.sigma_depth)
    for stage in STAGES:
        got = denoiser(w, h, stage).denoise(*case, params=p, return_variance=True)
        for k, name in enumerate(("colour", "variance")):
            bad = ~((got[k] == ref[k]) | (np.isnan(got[k]) & np.isnan(ref[k])))
            print(f"{what}, denoise_stage {stage}: {name}: {int(bad.sum())} of {bad.size} values differ")
        assert same(got[0], ref[0]) and same(got[1], ref[1]), (what, stage)
    return ref


# ---- 1: random frames, 1 to 5 passes, every term and flag on
@pytest.mark.parametrize("passes", [1, 2, 3, 4, 5])
def test_random_frames_equal_the_restatement(passes):
    case = frames(passes)
    out, var = check(case, f"{passes} passes", passes=passes, sigma_depth=0.4)
    assert np.isfinite(out).all() and not same(out, case[0])
    assert var.mean() < case[1].mean()                                  # it is a filter


# ---- 2: each term alone, all together, each flag off, the optional planes NULL
SETTINGS = {
    "colour alone": (dict(demodulate=False, match_id=False, sigma_color=4.0, sigma_normal=0.0, sigma_depth=0.0), (0, 1)),
    "normal alone": (dict(demodulate=False, match_id=False, sigma_color=0.0, sigma_normal=0.5, sigma_depth=0.0), (0, 3)),
    "depth alone": (dict(demodulate=False, match_id=False, sigma_color=0.0, sigma_normal=0.0, sigma_depth=0.4), (0, 4)),
    "id alone": (dict(demodulate=False, match_id=True, sigma_color=0.0, sigma_normal=0.0, sigma_depth=0.0), (0, 4)),
    "demodulation alone": (dict(demodulate=True, match_id=False, sigma_color=0.0, sigma_normal=0.0, sigma_depth=0.0), (0, 2)),
    "nothing": (dict(demodulate=False, match_id=False, sigma_color=0.0, sigma_normal=0.0, sigma_depth=0.0), (0,)),
    "all": (dict(sigma_depth=0.4), (0, 1, 2, 3, 4)),
    "defaults": (dict(), (0, 1, 2, 3, 4)),
    "no demodulation": (dict(demodulate=False, sigma_depth=0.4), (0, 1, 3, 4)),
    "no id match": (dict(match_id=False, sigma_depth=0.4), (0, 1, 2, 3, 4)),
    "a variance without the colour term": (dict(sigma_color=0.0), (0, 1, 2, 3, 4)),
}


@pytest.mark.parametrize("name", list(SETTINGS))
def test_terms_flags_and_null_planes(name):
    kw, given = SETTINGS[name]
    case = frames(11)
    check([a if k in given else None for k, a in enumerate(case)], name, passes=3, **kw)


# ---- 3: frames narrower than the taps
@pytest.mark.parametrize("w,h", [(5, 3), (1, 1), (17, 16)])
def test_tiny_frames(w, h):
    check(frames(w, w, h), f"{w} x {h}", w, h, passes=5, sigma_depth=0.4)


# ---- 4: NaN and inf
@pytest.mark.parametrize("what", ["colour", "variance", "depth", "id"])
def test_nan_and_inf_pixels(what):
    rgb, var, albedo, normal, depth = [a.copy() for a in frames(21)]
    spots = [(33, 20), (0, 0), (69, 44), (16, 15)]                     # interior, two corners, a block corner
    for k, (x, y) in enumerate(spots):
        bad = NAN if k % 2 == 0 else INF
        if what == "colour":
            rgb[y, x, k % 3] = bad
        elif what == "variance":
            var[y, x] = bad
        elif what == "depth":
            depth[y, x, 0] = bad
        else:
            depth[y, x, 2] = bad if bad != bad else 77.0               # (an infinite id is an id like another)
    out, v = check((rgb, var, albedo, normal, depth), f"NaN / inf {what}", passes=4, sigma_depth=0.4)
    den = np.where(albedo > 0.0, albedo, 1.0)
    for k, (x, y) in enumerate(spots):
        if k % 2 == 0:                                                 # NaN: the pixel keeps c and v; c den is rgb again up to the two roundings
            keep = np.isfinite(rgb[y, x])
            assert np.allclose(out[y, x][keep], rgb[y, x][keep], rtol=5e-16, atol=0.0), (what, x, y)
            assert same(out[y, x][~keep], (rgb[y, x] / den[y, x] * den[y, x])[~keep])
            assert same(v[y, x], var[y, x])


# ---- 5: streams
def test_two_denoisers_and_two_streams():
    import torch
    cases = [frames(31), frames(32), frames(33)]
    params = [DenoiseParams(passes=3), DenoiseParams(passes=5, sigma_depth=0.4), DenoiseParams(passes=2, match_id=False)]
    refs = [denoise_ref(*c, passes=p.passes, flags=p.flags, sigma_color=p.sigma_color, sigma_normal=p.sigma_normal, sigma_depth=p.sigma_depth)
            for c, p in zip(cases, params)]
    dev = [[torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in c] for c in cases]
    outs = [(torch.full((H * W * 3,), 7.0, dtype=torch.float64, device="cuda"), torch.full((H * W,), 7.0, dtype=torch.float64, device="cuda"))
            for _ in cases]
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    for stage in STAGES:
        a, b = denoiser(W, H, stage), denoiser(W, H, stage, copy=1)
        assert a is not b
        # two denoisers on two streams, then the first one again on the other stream: it waits for its own first call
        a.denoise_device(*[t.data_ptr() for t in dev[0]], outs[0][0].data_ptr(), outs[0][1].data_ptr(), params=params[0], stream_ptr=s1.cuda_stream)
        b.denoise_device(*[t.data_ptr() for t in dev[1]], outs[1][0].data_ptr(), outs[1][1].data_ptr(), params=params[1], stream_ptr=s2.cuda_stream)
        a.denoise_device(*[t.data_ptr() for t in dev[2]], outs[2][0].data_ptr(), outs[2][1].data_ptr(), params=params[2], stream_ptr=s2.cuda_stream)
        torch.cuda.synchronize()
        for k, (o, v) in enumerate(outs):
            assert same(o.cpu().numpy().reshape(H, W, 3), refs[k][0]) and same(v.cpu().numpy().reshape(H, W), refs[k][1]), (stage, k)
            o.fill_(7.0)
            v.fill_(7.0)
        torch.cuda.synchronize()
    # the variance output is optional; the frame does not depend on it
    a = denoiser(W, H, 0)
    a.denoise_device(*[t.data_ptr() for t in dev[0]], outs[0][0].data_ptr(), 0, params=params[0])
    torch.cuda.synchronize()
    assert same(outs[0][0].cpu().numpy().reshape(H, W, 3), refs[0][0]) and float(outs[0][1].min()) == 7.0
    with pytest.raises(RptError):                                       # an output that is an input
        a.denoise_device(*[t.data_ptr() for t in dev[0]], dev[0][0].data_ptr(), 0, params=params[0])


# ---- 6: real inputs
@functools.lru_cache(maxsize=None)
def rendered(name, f64, w=W, h=H, seed=3):
    """4 batches x 4 spp of a scene in a DeviceBuffer and the feature planes of the same 16 samples -> buffer, planes, mean, variance."""
    scene, cam, cfg = getattr(scenes, name)()
    if f64:
        scene.set_option("epsilon_policy", 1)
    r = Renderer(scene, cam).width(w).height(h).max_bounces(cfg["max_bounces"]).seed(seed)
    planes = r.features_array(16, sample_offset=0)
    buf = DeviceBuffer(w, h)
    for _ in range(4):
        r.sample(4, buf)
    rgb, var = buf.mean()
    for a in (rgb, var, *planes.values()):
        a.setflags(write=False)
    return buf, planes, rgb, var


@pytest.mark.parametrize("name,f64", [("cornell", False), ("cornell", True), ("lampshade", False), ("lampshade", True), ("monomial_glass", True)])
def test_rendered_frames(name, f64):
    buf, planes, rgb, var = rendered(name, f64)
    assert buf.batches == 4 and np.isfinite(rgb).all() and (var >= 0).all() and var.max() > 0
    if name == "monomial_glass":
        print("monomial_glass: NaN depths", int(np.isnan(planes["depth"][..., 0]).sum()))
    case = (rgb, var, planes["albedo"], planes["normal"], planes["depth"])
    check(case, f"{name} f64={f64}")                                                     # the defaults
    check(case, f"{name} f64={f64}, depth term", sigma_depth=0.5, passes=5)              # (monomial_glass: where a hit carries a NaN depth it freezes its pixel; the count is printed, 0 at this size and seed)


def test_buffer_mean_equals_numpy():
    """Batches on a grid of 2^-10: the squares, their sums and the running sums are exact, so the buffer's sums do not depend on how
    its kernels round them, and what rpt_buffer_mean_device adds is the stated order of operations."""
    rng = np.random.default_rng(41)
    for n in (2, 3, 4):
        buf = DeviceBuffer(W, H)
        batches = [rng.integers(0, 2048, (H * W, 3)) / 1024.0 for _ in range(n)]
        for k, b in enumerate(batches):
            if k == 1:
                with pytest.raises(RptError, match="2 batches"):        # RPT_ERR_STATE
                    buf.mean()
                with pytest.raises(RptError, match="2 batches"):
                    buf.denoised_image(denoiser(W, H, 0), {}, DenoiseParams(demodulate=False, match_id=False, sigma_normal=0.0))
            buf.add_samples(b)
        rgb, var = buf.mean()
        total, sumsq = np.zeros((H * W, 3)), np.zeros(H * W)
        for b in batches:
            total = total + b
            sumsq = sumsq + ((b[:, 0] * b[:, 0] + b[:, 1] * b[:, 1]) + b[:, 2] * b[:, 2])
        fn = float(n)
        mean = total / fn
        ss = sumsq - fn * ((mean[:, 0] * mean[:, 0] + mean[:, 1] * mean[:, 1]) + mean[:, 2] * mean[:, 2])
        want = np.fmax(ss, 0.0) / (fn - 1.0) / fn
        assert same(rgb, mean.reshape(H, W, 3)) and same(var, want.reshape(H, W))
        assert var.max() > 0
        # the mean of the per-pixel variances is Buffer::variance / n up to the rounding of the sums
        assert abs(var.mean() * n - buf.variance()) <= 1e-12 * buf.variance()
    with pytest.raises(RptError, match="sizes"):
        buf.denoised_image(denoiser(5, 3, 0), {}, DenoiseParams(demodulate=False, match_id=False, sigma_normal=0.0))


@pytest.mark.parametrize("name", ["cornell", "lampshade"])
def test_denoised_image_is_color_bytes_of_the_restatement(name):
    buf, planes, rgb, var = rendered(name, False)
    ref, _ = denoise_ref(rgb, var, planes["albedo"], planes["normal"], planes["depth"])
    want = color_bytes(ref)
    for stage in STAGES:
        got = buf.denoised_image(denoiser(W, H, stage), planes)
        assert got.shape == want.shape == (H, W, 3) and got.dtype == np.uint8
        diff = np.abs(got.astype(int) - want.astype(int))
        print(f"{name}, denoise_stage {stage}: {int((diff != 0).sum())} of {diff.size} bytes differ, by at most {int(diff.max())}")
        # the same fp64 frame; pow() may differ in the last ulp, i.e. a byte may flip at an exact boundary (tests/test_gpu_buffer.py)
        assert (got != want).mean() < 1e-3 and diff.max() <= 1
    with pytest.raises(RptError, match="normal"):
        buf.denoised_image(denoiser(W, H, 0), {"albedo": planes["albedo"], "depth": planes["depth"]})
    with pytest.raises(ValueError):
        buf.denoised_image(denoiser(W, H, 0), {"colour": planes["albedo"]})


# ---- 7: quality.  A condition, not a tolerance: the filtered image is closer to a converged one than the noisy image is.
@pytest.mark.parametrize("name", ["cornell", "lampshade"])
def test_filtered_image_is_closer_to_the_converged_one(name):
    w = h = 64
    buf, planes, rgb, var = rendered(name, False, w, h, seed=3)
    noisy = buf.image()                                                  # Filter::Box(0): color_bytes of the mean
    filtered = buf.denoised_image(denoiser(w, h, -1), planes)
    scene, cam, cfg = getattr(scenes, name)()
    make = lambda seed, spp: Renderer(scene, cam).width(w).height(h).max_bounces(cfg["max_bounces"]).seed(seed).num_samples(spp)  # noqa: E731
    converged = make(1234, 512).render()
    rms = lambda a: float(np.sqrt(np.mean((a.astype(np.float64) - converged.astype(np.float64)) ** 2)))  # noqa: E731
    print(f"quality, {name} 64 x 64, 4 batches x 4 spp against 512 spp: RMS {rms(noisy):.2f} -> {rms(filtered):.2f} levels, "
          f"ratio {rms(filtered) / rms(noisy):.3f}")
    assert rms(filtered) < rms(noisy)
    # Renderer.render_denoised is this composition
    assert np.array_equal(make(3, 16).render_denoised(4), filtered)
