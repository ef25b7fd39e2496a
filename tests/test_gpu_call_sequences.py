"""One committed scene through mixed call sequences and streams.

A committed scene keeps its buffers between calls -- the tile lists and their key, two launch sets (slab, work counter, events),
the host entry points' frame, the counters, the feature pass's slab, the timing ring, the specialised scan kernel, the photon map
with its camera-pass scratch -- and reuses them in place.  Every other test of the suite builds a scene per result; here

  1. "a result does not depend on the scene's past": a list of steps (an entry point with every parameter, seed and sample offset
     set explicitly) runs on ONE scene in order and in two written-out permutations, with two Renderer objects on the one scene
     used in turn; every result must be bit-equal to the same call on a freshly built and committed scene (computed once per scene
     and step, cached for the module; a call the scene refuses must be refused in the sequence as well).  The rest of the suite pins
     the fresh-scene call to the oracle;
  2. "a result does not depend on what the scene still has queued": device entry points on torch.cuda.Stream() streams (they are
     non-blocking), nothing waiting between the calls of a group, one synchronize at the end; every frame bit-equal to the lone call
     on a fresh scene.  Within a group all frames have the same tiles_x: a launch that read another call's tile list would write
     wrong pixels of its own frame, never outside it.  tests/test_host_call_sequences.py checks the same property on a CPU
     against a model of the streams, deterministically; this is the check that the model describes the runtime;
  3. the other objects with state: a DeviceBuffer with read-outs between its additions, one Denoiser through changing passes, flags
     and planes."""
import functools

import numpy as np
import pytest

from rpt_amd import AdaptiveParams, Camera, DenoiseParams, Denoiser, DeviceBuffer, Light, Renderer, RptError, scenes
from rpt_amd import _lib
from tests.util import random_rays

pytestmark = pytest.mark.gpu

SEED = 11
REFUSED = ("refused",)
MARKER = -7.25


class Case:
    def __init__(self, name, build, eps, center, radius, options=None):
        self.name, self.build, self.eps, self.center, self.radius, self.options = name, build, eps, np.array(center, dtype=np.float64), radius, options or {}

    def fresh(self):
        """-> (scene, camera, max_bounces, index of the first Light::Object or 0), the scene not yet committed."""
        scene, cam, cfg = self.build()
        for k, v in self.options.items():
            scene.set_option(k, v)
        if self.eps:
            scene.set_option("epsilon_policy", 1)
        light = next((i for i, l in enumerate(scene.lights) if l.kind == Light.OBJECT), 0)
        return scene, cam, cfg["max_bounces"], light


ROOM = ((278.0, 273.0, 280.0), 270.0)
CASES = {c.name: c for c in (
    Case("cornell", scenes.cornell, False, *ROOM),                                        # scan, no medium
    Case("lampshade", scenes.lampshade, False, *ROOM),                                    # scan in a medium: shell, tail cull, shadow form
    Case("mesh", lambda: scenes.mesh_in_fog(24, 24), False, (0.0, 0.0, 0.0), 2.0),        # per-mesh tree, detached shadow queries
    Case("fractal", lambda: scenes.fractal_spheres(3), False, (0.0, 0.0, 0.0), 2.0, {"scene_bvh_min": 4}),   # scene tree
    Case("cornell_eps", scenes.cornell, True, *ROOM),
    Case("lampshade_eps", scenes.lampshade, True, *ROOM),
    Case("mesh_eps", lambda: scenes.mesh_in_fog(24, 24), True, (0.0, 0.0, 0.0), 2.0),     # candidate tree
    Case("beamphoton", scenes.lampshade_beamphoton, False, *ROOM),                        # (the photon chain's scenes)
    Case("beamphoton_eps", scenes.lampshade_beamphoton, True, *ROOM),
)}
SEQUENCE_CASES = ["cornell", "lampshade", "mesh", "fractal", "cornell_eps", "lampshade_eps", "mesh_eps"]


class Ctx:
    """What a step gets: the renderer to use, and the case's camera, bounces, light and geometry."""

    def __init__(self, case, scene, cam, bounces, light):
        self.case, self.scene, self.cam, self.bounces, self.light = case, scene, cam, bounces, light
        self.renderers = [Renderer(scene, cam), Renderer(scene, cam)]    # two objects, one handle
        self.r = self.renderers[0]

    def set(self, w, h, offset=0, shard=(0, 1), cam=None, bounces=None, exposure=0.0):
        r = self.r
        r.camera = cam or self.cam
        r.width(w).height(h).exposure_value(exposure).max_bounces(self.bounces if bounces is None else bounces).seed(SEED).shard(*shard)
        r.gather_size(12).gather_size_volume(3).watts(100.0 * 5000)
        r._sample_offset = offset
        return r


def attempt(fn):
    try:
        return fn()
    except RptError:
        return REFUSED


def same(a, b):
    """Bit-equality of two results: arrays (NaN equal to NaN), numbers, strings, and tuples / dicts of them."""
    if isinstance(a, dict):
        return isinstance(b, dict) and sorted(a) == sorted(b) and all(same(a[k], b[k]) for k in a)
    if isinstance(a, (tuple, list)):
        return isinstance(b, (tuple, list)) and len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")
    return type(a) is type(b) and a == b


# ---- the steps
def s_render(w, h, spp, offset=0, shard=(0, 1)):
    return lambda c: attempt(lambda: c.set(w, h, offset, shard).sample_array(spp))


def s_features(c):
    return attempt(lambda: c.set(96, 96).features_array(4, sample_offset=0))


def s_tiles(c):
    out = np.full(96 * 96 * 3, MARKER)
    return attempt(lambda: c.set(96, 96).sample_tiles_array(8, [4, 0, 8], out))


def s_closest_hit(c):
    o, d = random_rays(np.random.default_rng(7), 4096, c.case.center, 1.5 * c.case.radius)
    r = c.set(96, 96)
    return attempt(lambda: r.get_closest_hit(o, d)), attempt(lambda: r.get_closest_hit_f64(o, d))


def s_light_hooks(c):
    rng = np.random.default_rng(5)
    pos = c.case.center + rng.uniform(-0.5, 0.5, (1024, 3)) * c.case.radius
    d = rng.normal(size=(1024, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    dist = rng.uniform(0.1, 2.0, 1024) * c.case.radius
    r = c.set(96, 96)
    return (attempt(lambda: r.debug_light_sample(c.light, pos, seed=3, f64=c.case.eps)),
            attempt(lambda: r.debug_shadow_test(c.light, pos, d, dist)))


def s_other_camera(c):
    right = np.cross(c.cam.direction, c.cam.up)
    cam = Camera(c.cam.eye + 0.1 * c.case.radius * right, c.cam.direction, c.cam.up, 0.8 * c.cam.fov)
    return attempt(lambda: c.set(64, 64, cam=cam, bounces=0, exposure=1.5).sample_array(4))


def s_counters(c):
    c.scene.set_option("counters", 1)
    try:
        r = c.set(64, 64)
        return attempt(lambda: (r.sample_array(4), r.counters()))
    finally:
        c.scene.set_option("counters", 0)


def s_max_blocks(c):
    c.scene.set_option("max_blocks", 5)
    try:
        return attempt(lambda: c.set(96, 96).sample_array(8))
    finally:
        c.scene.set_option("max_blocks", 0)


STEPS = [
    ("render 96x96", s_render(96, 96, 8)),                        # 0
    ("render 96x32", s_render(96, 32, 8)),                        # 1: fewer tiles, the same buffers
    ("render 33x17", s_render(33, 17, 3)),                        # 2: a clipped tile, another chunking
    ("shard 0/2", s_render(96, 96, 8, shard=(0, 2))),             # 3
    ("shard 1/2", s_render(96, 96, 8, shard=(1, 2))),             # 4
    ("render 160x96", s_render(160, 96, 40, offset=8)),           # 5: the slab grows, several chunks
    ("features", s_features),                                     # 6
    ("tile list", s_tiles),                                       # 7
    ("render 96x96", s_render(96, 96, 8)),                        # 8: step 0 again
    ("closest hit", s_closest_hit),                               # 9
    ("light hooks", s_light_hooks),                               # 10
    ("other camera", s_other_camera),                             # 11
    ("counters", s_counters),                                     # 12
    ("max_blocks", s_max_blocks),                                 # 13
]
# numpy.random.default_rng(20261019).permutation(14), twice
ORDERS = {
    "in order": list(range(14)),
    "permutation 1": [1, 12, 10, 11, 3, 2, 4, 6, 7, 8, 0, 9, 13, 5],
    "permutation 2": [13, 12, 10, 4, 3, 8, 11, 2, 7, 0, 6, 5, 1, 9],
}


def freeze(x):
    if isinstance(x, np.ndarray):
        x.setflags(write=False)
    elif isinstance(x, dict):
        for v in x.values():
            freeze(v)
    elif isinstance(x, (tuple, list)):
        for v in x:
            freeze(v)
    return x


@functools.lru_cache(maxsize=None)
def expected(case_name, step_name):
    """The step on a scene that has done nothing else."""
    case = CASES[case_name]
    c = Ctx(case, *case.fresh())
    fn = next(f for n, f in STEPS if n == step_name)
    out = freeze(fn(c))
    c.scene.close()
    return out


def check_flavour(case, c):
    st = c.r.scene_stats()
    name = case.name
    if name.startswith(("cornell", "lampshade")):
        assert st["bvh_nodes"] == 0 and st["scene_bvh"] == 0 and st["shell_faces"] > 0, st
        if name == "lampshade":
            assert c.r.shadow_scan_info(c.light)["shadow_form"] == 1
    if name == "mesh":
        assert st["bvh_nodes"] > 0 and st["scene_bvh"] == 0, st
    if name == "fractal":
        assert st["scene_bvh"] != 0, st
    if name == "mesh_eps":
        assert c.r.f64_mesh_tree_info()["render_uses_trees"] == 1
    # what a flavour refuses is refused, the rest is computed
    hit32, hit64 = expected(name, "closest hit")
    assert (hit64 if case.eps else hit32) is not REFUSED
    sample, shadow = expected(name, "light hooks")
    if name in ("cornell", "lampshade"):
        assert sample is not REFUSED and shadow is not REFUSED
    if name == "fractal":                                     # no Light::Object
        assert sample is REFUSED and shadow is REFUSED
    if case.eps:
        assert sample is not REFUSED and shadow is REFUSED    # the shadow query is the fp32 scan's
    for step in ("render 96x96", "render 33x17", "shard 1/2", "render 160x96", "features", "tile list", "other camera", "counters", "max_blocks"):
        assert expected(name, step) is not REFUSED, step
    tiles = expected(name, "tile list").reshape(96, 96, 3)
    assert (tiles[32:64, 0:32] == MARKER).all() and not (tiles[0:32, 0:32] == MARKER).any()   # tile 3 kept, tile 0 rendered
    assert same(expected(name, "counters")[1]["samples"], 64 * 64 * 4)


@pytest.mark.parametrize("order", list(ORDERS))
@pytest.mark.parametrize("name", SEQUENCE_CASES)
def test_a_result_does_not_depend_on_the_scenes_past(name, order):
    case = CASES[name]
    c = Ctx(case, *case.fresh())
    if order == "in order":
        check_flavour(case, c)
    bad = []
    for k, i in enumerate(ORDERS[order]):
        step, fn = STEPS[i]
        c.r = c.renderers[k % 2 if order == "permutation 1" else 0]
        got = fn(c)
        if not same(got, expected(name, step)):
            bad.append(f"{step} (position {k})")
    print(f"{name}, {order}: {len(bad)} of {len(STEPS)} steps differ from the fresh scene's: {bad}")
    c.scene.close()
    assert not bad, bad


# ---- the photon chain: map, camera pass, path render, camera pass at another size, a smaller map, camera pass
def photon_chain(c, kind, only=None):
    """The chain's results; `only` = k: result k alone, on a scene that has just built the map that result needs."""
    def build(n):
        return lambda: tuple(c.set(48, 48).photon_map_build(n, kind)[k] for k in ("surface", "volume", "shot"))
    chain = [
        (None, build(5000)),
        (5000, lambda: c.set(48, 48).photon_sample_array(8)),
        (None, lambda: c.set(96, 96).sample_array(8)),
        (5000, lambda: c.set(96, 32, offset=8).photon_sample_array(8)),
        (None, build(1200)),
        (1200, lambda: c.set(48, 48).photon_sample_array(8)),
    ]
    if only is None:
        return [attempt(fn) for _, fn in chain]
    need, fn = chain[only]
    if need:
        attempt(build(need))
    return attempt(fn)


@pytest.mark.parametrize("name", ["beamphoton", "cornell", "beamphoton_eps", "cornell_eps"])
def test_photon_passes_do_not_depend_on_the_scenes_past(name):
    case, kind = CASES[name], Renderer.PHOTON_POINT_BEAM         # the estimator both modes have
    want = []
    for k in range(6):
        c = Ctx(case, *case.fresh())
        want.append(photon_chain(c, kind, only=k))
        c.scene.close()
    assert not any(w is REFUSED for w in want), name
    assert want[0][0] + want[0][1] > want[4][0] + want[4][1] > 0                        # 5,000 and 1,200 photons: maps of different sizes
    assert not same(want[1], want[5])
    c = Ctx(case, *case.fresh())
    got = photon_chain(c, kind)
    c.scene.close()
    bad = [k for k in range(6) if not same(got[k], want[k])]
    print(f"{name}: chain results that differ from the fresh scene's: {bad}")
    assert not bad, bad


# ---- in flight
# A: the launch that must still be running while the next calls are prepared.  lampshade(), 96 x 96, more samples rather than more
# pixels.  Its lone launch, measured with the "timing" option on an MI355X (render kernel, ms): fp32 1.4 / 2.0 / 3.5 / 5.9 at
# 1,024 / 2,048 / 4,096 / 8,192 samples; reference-epsilon mode 3.0 / 4.8 / 7.3 / 11.8 at 256 / 512 / 1,024 / 2,048.  Preparing a
# call takes the host some tens of microseconds.
A_SPP = 4096         # fp32: 3.5 ms
A_SPP_EPS = 1024     # reference-epsilon mode: 7.3 ms


PREPARE = {"photon map": lambda c: c.set(48, 48).photon_map_build(5000, Renderer.PHOTON_POINT_BEAM)}


@functools.lru_cache(maxsize=None)
def lone(case_name, call, prepare=None):
    """One device call alone on a fresh scene (after PREPARE[prepare]) -> its frame or planes."""
    case = CASES[case_name]
    c = Ctx(case, *case.fresh())
    if prepare:
        PREPARE[prepare](c)
    out = run_group(c, [call], [None])[0]
    c.scene.close()
    out.setflags(write=False)
    return out


def run_group(c, calls, streams, host_after=None):
    """Queues `calls` (kind, w, h, spp, offset, shard) on the given torch streams (None: the null stream) without waiting, then
    synchronises once -> the frames.  host_after = (position, call): a host entry point called right after that position."""
    import torch
    keep, host = [], None
    for kind, w, h, spp, offset, shard in calls:                  # a frame per call: planes for a feature pass, else a marked frame
        n = w * h * 3
        keep.append(torch.zeros(3 * n, dtype=torch.float64, device="cuda") if kind == "features"
                    else torch.full((n,), MARKER, dtype=torch.float64, device="cuda"))
    tiles = torch.tensor([4, 0, 8], dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    for k, ((kind, w, h, spp, offset, shard), st) in enumerate(zip(calls, streams)):
        r = c.set(w, h, offset, shard)
        ptr = st.cuda_stream if st is not None else 0
        f, n = keep[k], w * h * 3
        if kind == "sample":
            r.sample_device(spp, f.data_ptr(), ptr)
        elif kind == "features":
            r.features_device(spp, f.data_ptr(), f.data_ptr() + 8 * n, f.data_ptr() + 16 * n, ptr, sample_offset=offset)
        elif kind == "tiles":
            r.sample_tiles_device(spp, tiles.data_ptr(), 3, f.data_ptr(), ptr)
        elif kind == "photon":
            r.photon_sample_device(spp, f.data_ptr(), ptr)
        if host_after is not None and host_after[0] == k:
            _, w2, h2, spp2, offset2, shard2 = host_after[1]
            host = c.set(w2, h2, offset2, shard2).sample_array(spp2)
    torch.cuda.synchronize()
    return [f.cpu().numpy() for f in keep] + ([host] if host is not None else [])


def check_group(case_name, calls, streams, host_after=None, prepare=None):
    case = CASES[case_name]
    c = Ctx(case, *case.fresh())
    if prepare:
        PREPARE[prepare](c)
    got = run_group(c, calls, streams, host_after)
    c.scene.close()
    bad = []
    for k, call in enumerate(calls):
        want = lone(case_name, call, prepare)
        diff = int((got[k] != want).sum())
        assert (want != MARKER).any()
        if diff:
            bad.append((k, call[0], diff, want.size))
    if host_after is not None:
        want = expected_host(case_name, host_after[1])
        if not same(got[-1], want):
            bad.append(("host", int((got[-1] != want).sum())))
    print(f"{case_name}: calls whose frame differs from the lone call's (position, kind, values, of): {bad}")
    assert not bad, bad


def expected_host(case_name, call):
    case = CASES[case_name]
    c = Ctx(case, *case.fresh())
    _, w, h, spp, offset, shard = call
    out = c.set(w, h, offset, shard).sample_array(spp)
    c.scene.close()
    return out


def group_a(spp):
    return [("sample", 96, 96, spp, 0, (0, 1)), ("sample", 96, 32, 8, 3, (0, 1)), ("sample", 96, 96, 8, 5, (1, 2))]


def test_one_stream_three_frames_queued():
    import torch
    s = torch.cuda.Stream()
    check_group("lampshade", group_a(A_SPP), [s, s, s])


def test_one_stream_three_frames_queued_in_the_reference_epsilon_mode():
    import torch
    s = torch.cuda.Stream()
    check_group("lampshade_eps", group_a(A_SPP_EPS), [s, s, s])


def test_two_streams_in_turn_two_sizes():
    import torch
    s, t = torch.cuda.Stream(), torch.cuda.Stream()
    a, b, sh = group_a(A_SPP)
    check_group("lampshade", [a, b, sh, a, b], [s, t, s, t, s])


def test_a_host_call_while_a_device_call_is_queued():
    import torch
    s = torch.cuda.Stream()
    a, b, sh = group_a(A_SPP)
    check_group("lampshade", [a, sh], [s, s], host_after=(0, b))


def test_mixed_entry_points_queued_on_two_streams():
    import torch
    s, t = torch.cuda.Stream(), torch.cuda.Stream()
    calls = [("sample", 96, 96, A_SPP, 0, (0, 1)), ("features", 96, 32, 4, 0, (0, 1)), ("tiles", 96, 96, 8, 2, (0, 1)),
             ("photon", 96, 32, 8, 0, (0, 1)), ("sample", 96, 96, 8, 5, (1, 2)), ("features", 96, 96, 4, 1, (1, 2)),
             ("photon", 96, 96, 8, 4, (0, 2))]
    check_group("beamphoton", calls, [s, t, s, t, s, t, s], prepare="photon map")


# ---- the other objects with state
def test_device_buffer_read_outs_between_additions_change_nothing():
    """add_samples, add_samples_tiles_device, mean, tile_errors, refine_tiles, image and variance interleaved on one buffer: every
    read-out equals that of a second buffer that received the additions alone (and reads only then)."""
    import torch
    w, h = 70, 45                                                  # 3 x 2 tiles, the last column and row clipped
    rng = np.random.default_rng(3)
    batches = [rng.uniform(0.0, 2.0, (w * h, 3)) for _ in range(4)]
    tile_frames = [torch.from_numpy(rng.uniform(0.0, 2.0, w * h * 3)).cuda() for _ in range(2)]
    lists = [torch.tensor(l, dtype=torch.int32, device="cuda") for l in ([5, 0, 2], [1, 5])]
    torch.cuda.synchronize()
    params = AdaptiveParams(spp_per_batch=1, min_batches=2, max_batches=4, threshold=0.05, floor=0.05)

    def additions(b, upto, read):
        """The additions in their order, the first `upto` of them; read(b, k) after addition k."""
        ops = [lambda: b.add_samples(batches[0]), lambda: b.add_samples(batches[1]),
               lambda: b.add_samples_tiles_device(tile_frames[0].data_ptr(), lists[0].data_ptr(), 3),
               lambda: b.add_samples(batches[2]),
               lambda: b.add_samples_tiles_device(tile_frames[1].data_ptr(), lists[1].data_ptr(), 2),
               lambda: b.add_samples(batches[3])]
        for k, op in enumerate(ops[:upto]):
            op()
            torch.cuda.synchronize()
            read(b, k)

    def read_all(b):
        ids, err = b.refine_tiles(params)
        return (b.mean(), b.tile_errors(0.05), ids, err, b.image(), b.variance(), b.tile_batches(), b.batches)

    busy = DeviceBuffer(w, h)
    seen = {}
    additions(busy, 6, lambda b, k: seen.__setitem__(k, read_all(b)) if k >= 1 else None)
    bad = []
    for k in range(1, 6):
        quiet = DeviceBuffer(w, h)
        additions(quiet, k + 1, lambda b, i: None)
        if not same(seen[k], read_all(quiet)):
            bad.append(k)
        quiet.close()
    busy.close()
    print(f"device buffer: additions after which the read-outs differ: {bad}")
    assert not bad
    assert seen[5][6].max() == 6 and seen[5][6].min() == 4 and seen[5][7] == 4     # tile 5 got both tile batches, tiles 3 and 4 none


def _denoise_frames(seed, w, h):
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:h, 0:w]
    region = (xs // 9 + 2 * (ys // 7)) % 5
    albedo = rng.uniform(0.1, 0.9, (5, 3))[region]
    var = rng.uniform(0.0, 0.02, (h, w))
    rgb = albedo * rng.uniform(0.5, 1.5, (5, 1))[region] + rng.normal(size=(h, w, 3)) * np.sqrt(var)[..., None]
    normal = rng.normal(size=(5, 3))[region] * 0.5 + rng.normal(size=(h, w, 3)) * 0.05
    depth = np.stack([2.0 + 0.02 * xs + 0.5 * region, np.ones((h, w)), region.astype(np.float64)], axis=-1)
    return rgb, var, albedo, normal, depth


@pytest.mark.parametrize("stage", [0, -1])
def test_one_denoiser_through_changing_passes_flags_and_planes(stage):
    """Passes 5 -> 1 -> 3, flags changed, NULL planes then real ones, on one object: each result bit-equal to a fresh denoiser's."""
    w, h = 70, 45
    lib = _lib.load()

    def make():
        _lib.check(lib.rpt_set_option(b"denoise_stage", stage))
        try:
            return Denoiser(w, h)
        finally:
            _lib.check(lib.rpt_set_option(b"denoise_stage", -1))
    full, other = _denoise_frames(1, w, h), _denoise_frames(2, w, h)
    nulls = [full[0], full[1], None, None, None]
    calls = [
        (full, dict(passes=5, sigma_depth=0.4)),
        (other, dict(passes=1, sigma_depth=0.4)),
        (full, dict(passes=3, demodulate=False, match_id=False)),
        (nulls, dict(passes=3, demodulate=False, match_id=False, sigma_normal=0.0)),
        (other, dict(passes=3, sigma_depth=0.4)),
        (full, dict(passes=5, sigma_depth=0.4)),
    ]
    one = make()
    got = [one.denoise(*case, params=DenoiseParams(**kw), return_variance=True) for case, kw in calls]
    one.close()
    bad = []
    for k, (case, kw) in enumerate(calls):
        d = make()
        if not same(got[k], d.denoise(*case, params=DenoiseParams(**kw), return_variance=True)):
            bad.append(k)
        d.close()
    print(f"denoise_stage {stage}: calls that differ from a fresh denoiser's: {bad}")
    assert not bad
    assert same(got[0], got[5]) and not same(got[0][0], got[2][0])
