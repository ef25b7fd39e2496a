"""First-hit feature planes (rpt_render_features*) on the device, in both modes, against the numpy restatement of the contract in
tests/feature_ref.py -- a composition of hooks that other modules check against the oracle call by call -- and against
tolerance-free properties of their own.  Equality is bit for bit unless a test says otherwise.

Frames are 70 x 45: 3 x 2 tiles of 32 x 32, clipped on both edges, no multiple of the 8 x 8 pixels of a wave; 10 samples in chunks
of 4 (three chunks, the last one ragged), sample offset 5, a seed of its own."""
import ctypes as C
import functools

import numpy as np
import pytest

from rpt_amd import (Buffer, Camera, DeviceBuffer, Environment, KdTree, Light, Material, Object, Renderer, Scene, _lib, cube, plane,
                     scenes, shard_pixels, sphere, vec3)
from tests.feature_ref import feature_planes, feature_samples, reduce_samples

pytestmark = pytest.mark.gpu

W, H, SPP, CHUNK, OFFSET, SEED = 70, 45, 10, 4, 5, 0x5EED0F17
PLANES = ("albedo", "normal", "depth")


def _hdri_spheres():
    scene, _, _ = scenes.spheres()
    # C1's camera raised to the horizon, so that the upper half of the frame misses; it keeps the lens (cast_ray draws from the unit disc)
    cam = Camera.look_at(vec3(0.7166, -9.2992, 2.8803), vec3(0.8673, 0.2095, 2.6), vec3(0.0, 0.0, 1.0), 0.6911).focus(vec3(0.1, -2.0, 0.6), 0.15)
    assert cam.aperture > 0
    texels = np.arange(8 * 4 * 3, dtype=np.float64).reshape(4, 8, 3) / 64.0 + 0.125   # 8 x 4 distinct texels
    scene.environment = Environment.Hdri(8, 4, texels)
    return scene, cam


def _group_scene():
    """A kd-tree group between two plain objects: in the reference-epsilon mode its leaves are records of their own."""
    scene = Scene()
    scene.add(Object(plane(vec3(0.0, 1.0, 0.0), -1.0)).material(Material.diffuse(vec3(0.5, 0.25, 0.125))))
    kids = [sphere().scale(vec3(0.4, 0.4, 0.4)).translate(vec3(-1.0 + 0.5 * i, -0.3 + 0.2 * i, 0.0)) for i in range(4)]
    kids.append(cube().rotate_y(0.4).scale(vec3(0.5, 0.5, 0.5)).translate(vec3(1.4, 0.2, 0.5)))
    scene.add(Object(KdTree(kids).translate(vec3(0.0, 0.1, 0.0))).material(Material.specular(vec3(0.25, 0.75, 0.5), 0.3)))
    scene.add(Object(sphere().scale(vec3(0.6, 0.6, 0.6)).translate(vec3(0.0, 1.2, -1.0))).material(Material.mirror()))
    scene.add(Light.Ambient(vec3(0.1, 0.1, 0.1)))
    scene.environment = Environment.Color(vec3(0.2, 0.3, 0.4))
    return scene, Camera(eye=vec3(0.0, 0.5, 6.0), direction=vec3(0.0, 0.0, -1.0), up=vec3(0.0, 1.0, 0.0), fov=0.8)


def _furnace(rho):
    from tests.test_oracle_kat import furnace_scene
    return furnace_scene(rho, 0.25)


BUILDERS = {
    "cornell": lambda: scenes.cornell()[:2],                                   # scan, room shell, object light
    "lampshade": lambda: scenes.lampshade()[:2],                               # a medium, which the pass ignores
    "spheres_hdri": _hdri_spheres,                                             # planes + misses -> the environment's texels; a lens
    "mesh": lambda: scenes.mesh_in_fog(nu=24, nv=24)[:2],                      # per-mesh tree (fp32), candidate tree (fp64)
    "fractal_spheres": lambda: scenes.fractal_spheres(levels=2)[:2],           # with scene_bvh_min = 4: the scene tree
    "fractal_meshes": lambda: scenes.fractal_meshes(levels=2, nu=12, nv=8)[:2],   # instancing + scene tree
    "monomial": lambda: scenes.monomial_glass()[:2],                           # MONO
    "group": _group_scene,
    "furnace": lambda: _furnace(0.75),
}
OPTIONS = {"fractal_spheres": {"scene_bvh_min": 4}, "fractal_meshes": {"scene_bvh_min": 4}}


def make(name, f64, chunk=CHUNK, w=W, h=H, **options):
    """A renderer on a fresh scene (options are read at commit; a committed scene is immutable)."""
    scene, cam = BUILDERS[name]()
    for k, v in {**OPTIONS.get(name, {}), **options}.items():
        scene.set_option(k, v)
    scene.set_option("chunk_spp", chunk)
    if f64:
        scene.set_option("epsilon_policy", 1)
    return Renderer(scene, cam).width(w).height(h).seed(SEED)


def run(r, spp=SPP, offset=OFFSET, **kw):
    return r.features_array(spp, sample_offset=offset, **kw)


@functools.lru_cache(maxsize=None)
def case(name, f64):
    """(planes of the pass, planes of the restatement) of one scene in one mode, computed once for every test that reads them."""
    r = make(name, f64)
    got = run(r)
    ref = feature_planes(r, SPP, SEED, OFFSET, f64)
    for d in (got, ref):
        for a in d.values():
            a.setflags(write=False)
    return got, ref


def same(a, b):
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def check_planes(got, ref, what):
    for k in PLANES:
        bad = ~((got[k] == ref[k]) | (np.isnan(got[k]) & np.isnan(ref[k])))
        print(f"{what}: {k}: {int(bad.sum())} of {bad.size} values differ, coverage mean {ref['depth'][..., 1].mean():.3f}")
    for k in PLANES:
        assert same(got[k], ref[k]), (what, k)


# ---- 1: the fp32 flavours against the restatement
@pytest.mark.parametrize("name", ["cornell", "lampshade", "spheres_hdri", "mesh", "fractal_spheres", "fractal_meshes", "monomial"])
def test_fp32_planes_equal_the_restatement(name):
    got, ref = case(name, False)
    assert 0.0 < ref["depth"][..., 1].mean()                      # the frame sees the scene
    if name in ("spheres_hdri", "monomial"):
        assert ref["depth"][..., 1].min() == 0.0                  # ... and the environment
    check_planes(got, ref, name)
    r = make(name, False)
    stats = r.scene_stats()
    if name.startswith("fractal"):
        assert stats["scene_bvh"] != 0
    if name == "fractal_meshes":
        assert stats["instances"] > 0
    if name == "mesh":
        assert stats["bvh_nodes"] > 0 and stats["scene_bvh"] == 0
    for k in PLANES:                                               # each plane requested alone, the others NULL
        alone = run(r, **{p: p == k for p in PLANES})
        assert list(alone) == [k] and same(alone[k], ref[k]), (name, k)


# ---- 2: the reference-epsilon mode against its restatement
@pytest.mark.parametrize("name", ["cornell", "lampshade", "mesh", "monomial", "group"])
def test_f64_planes_equal_the_restatement(name):
    got, ref = case(name, True)
    assert 0.0 < ref["depth"][..., 1].mean()
    check_planes(got, ref, name + " (reference-epsilon)")
    if name == "group":
        ids = np.unique(ref["depth"][..., 2])
        print("group: ids", ids)
        assert ids.max() > 3                                       # records beyond the scene's three objects: the group's leaves
    if name == "mesh":
        assert make(name, True).f64_mesh_tree_info()["render_uses_trees"] == 1     # the TREE flavour ran
        r = make(name, True, f64_mesh_tree_min=0)
        assert r.f64_mesh_tree_info()["render_uses_trees"] == 0
        scan = run(r)
        for k in PLANES:
            assert same(scan[k], got[k]), k                        # tree on and off: the same planes


# ---- 3: chunking and offsets
@pytest.mark.parametrize("f64", [False, True])
def test_chunking_and_offsets(f64):
    per_sample = objs = None
    for chunk in (1, 4, 16):
        r = make("cornell", f64, chunk=chunk)
        assert r.chunking(SPP) == (min(chunk, SPP), -(-SPP // min(chunk, SPP)))
        if per_sample is None:
            per_sample, objs = feature_samples(r, SPP, SEED, OFFSET, f64)   # the samples do not depend on the chunking
        mean = reduce_samples(per_sample, r.chunking(SPP)[0]).reshape(H, W, 8)
        got = run(r)
        assert same(got["albedo"], mean[..., 0:3]) and same(got["normal"], mean[..., 3:6]), chunk
        assert same(got["depth"][..., 0:2], mean[..., 6:8]), chunk
        assert same(got["depth"][..., 2], (objs[0] + 1).reshape(H, W).astype(np.float64)), chunk
    r = make("cornell", f64)
    ten, one = run(r, 10, 0, albedo=False, normal=False)["depth"], run(r, 1, 0, albedo=False, normal=False)["depth"]
    assert same(ten[..., 2], one[..., 2])                          # the id is that of the call's first sample
    assert same(one[..., 1], (one[..., 2] > 0).astype(np.float64))
    hits = ten[..., 1] * 10.0
    assert np.array_equal(hits, np.round(hits)) and hits.min() >= 0 and hits.max() <= 10


# ---- 4: sharding
@pytest.mark.parametrize("f64", [False, True])
def test_shards_add_up_to_the_frame(f64):
    whole, _ = case("cornell", f64)
    r = make("cornell", f64)
    total = {k: np.zeros((H, W, 3)) for k in PLANES}
    for rank in range(3):
        part = run(r.shard(rank, 3))
        owned = np.zeros(W * H, dtype=bool)
        owned[shard_pixels(W, H, rank, 3)] = True
        assert owned.any() and not owned.all()
        for k in PLANES:
            flat = part[k].reshape(-1, 3)
            assert np.array_equal(flat[~owned], np.zeros_like(flat[~owned])), (rank, k)
            assert same(flat[owned], whole[k].reshape(-1, 3)[owned]), (rank, k)
            total[k] = total[k] + part[k]
    for k in PLANES:
        assert same(total[k], whole[k]), k


# ---- 5: the device variant and what carries a plane
def test_device_variant_and_plumbing():
    import torch
    whole, _ = case("cornell", False)
    r = make("cornell", False)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    first = [torch.full((H * W * 3,), 7.0, dtype=torch.float64, device="cuda") for _ in PLANES]
    second = [torch.full((H * W * 3,), 9.0, dtype=torch.float64, device="cuda") for _ in PLANES]
    torch.cuda.synchronize()
    # two passes back to back on two streams: the second waits for the first (one feature scratch per scene)
    r.features_device(SPP, *[t.data_ptr() for t in first], stream_ptr=s1.cuda_stream, sample_offset=OFFSET)
    r.features_device(SPP, *[t.data_ptr() for t in second], stream_ptr=s2.cuda_stream, sample_offset=OFFSET)
    torch.cuda.synchronize()
    for k, a, b in zip(PLANES, first, second):
        assert same(a.cpu().numpy().reshape(H, W, 3), whole[k]), k
        assert same(b.cpu().numpy().reshape(H, W, 3), whole[k]), k
    # a single plane, the others null
    only = torch.zeros(H * W * 3, dtype=torch.float64, device="cuda")
    r.features_device(SPP, 0, only.data_ptr(), None, stream_ptr=s1.cuda_stream, sample_offset=OFFSET)
    torch.cuda.synchronize()
    assert same(only.cpu().numpy().reshape(H, W, 3), whole["normal"])
    # a plane is a frame: rpt_buffer_add_samples_device takes it ...
    dev, host = DeviceBuffer(W, H), Buffer(W, H)
    for _ in range(2):
        dev.add_samples_device(first[0].data_ptr(), s1.cuda_stream)
        host.add_samples(whole["albedo"])
    s1.synchronize()
    assert dev.batches == 2 and np.array_equal(dev.image(), host.image())
    # ... and so do rpt_frame_pack_device / rpt_frame_unpack_device, shard by shard
    lib = _lib.load()
    for k, t in zip(PLANES, first):
        back = torch.zeros_like(t)
        for rank in range(3):
            tiles = _lib.check(lib.rpt_shard_tiles(W, H, rank, 3, None, 0))
            packed = torch.zeros(max(tiles, 1) * 3072, dtype=torch.float64, device="cuda")
            _lib.check(lib.rpt_frame_pack_device(W, H, rank, 3, C.c_void_p(t.data_ptr()), C.c_void_p(packed.data_ptr()), None))
            _lib.check(lib.rpt_frame_unpack_device(W, H, rank, 3, C.c_void_p(packed.data_ptr()), C.c_void_p(back.data_ptr()), None))
        torch.cuda.synchronize()
        assert same(back.cpu().numpy().reshape(H, W, 3), whole[k]), k


# ---- 6: independence from the render
@pytest.mark.parametrize("f64", [False, True])
def test_pass_and_render_do_not_touch_each_other(f64):
    import torch
    whole, _ = case("lampshade", f64)
    r = make("lampshade", f64).max_bounces(3)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    frames = [torch.zeros(H * W * 3, dtype=torch.float64, device="cuda") for _ in range(4)]
    planes = [torch.zeros(H * W * 3, dtype=torch.float64, device="cuda") for _ in PLANES]
    torch.cuda.synchronize()

    def render(i):   # the same samples every time, on alternating streams
        r._sample_offset = 0
        r.sample_device(4, frames[i].data_ptr(), streams[i % 2].cuda_stream)

    render(0)
    render(1)
    r.features_device(SPP, *[t.data_ptr() for t in planes], stream_ptr=streams[0].cuda_stream, sample_offset=OFFSET)
    render(2)
    render(3)
    torch.cuda.synchronize()
    base = frames[0].cpu().numpy()
    assert np.isfinite(base).all() and base.max() > 0
    for f in frames[1:]:
        assert np.array_equal(f.cpu().numpy(), base)
    for k, t in zip(PLANES, planes):
        assert same(t.cpu().numpy().reshape(H, W, 3), whole[k]), k
    # what the pass ignores: max_bounces, exposure_value, the render kernels' grid options
    other = make("lampshade", f64, max_blocks=3, blocks_per_cu=1).max_bounces(7).exposure_value(2.5)
    got = run(other)
    for k in PLANES:
        assert same(got[k], whole[k]), k


# ---- 7: meaning, without the restatement
@pytest.mark.parametrize("f64", [False, True])
def test_planes_mean_what_they_say(f64):
    rho = 0.75                                                     # exact in binary: sums of it are exact, and so is their mean
    got, _ = case("furnace", f64)
    cov, ids = got["depth"][..., 1], got["depth"][..., 2]
    assert np.array_equal(cov, np.ones((H, W)))                    # a closed box around the camera
    assert np.array_equal(got["albedo"], np.full((H, W, 3), rho))
    assert np.array_equal(ids, np.round(ids)) and ids.min() >= 1 and ids.max() <= 6
    assert (got["depth"][..., 0] > 0).all()
    # every sample of these pixels hits the wall z = -10 (object 4, normal +z): the mean of equal unit normals
    back = ids == 5
    length = np.linalg.norm(got["normal"], axis=-1)
    inner = back & np.roll(back, 1, 0) & np.roll(back, -1, 0) & np.roll(back, 1, 1) & np.roll(back, -1, 1)
    flat = inner & (np.abs(got["normal"][..., 2] - 1.0) < 1e-3)
    print(f"furnace f64={f64}: {int(flat.sum())} pixels on the back wall, |n| - 1 within {np.abs(length[flat] - 1.0).max():.3e}")
    assert flat.sum() > 100
    assert np.abs(length[flat] - 1.0).max() <= (1e-12 if f64 else 1e-6)
    # ids elsewhere: a valid object index + 1, or 0 for a miss
    for name in ("cornell", "monomial"):
        planes, _ = case(name, f64)
        n_objects = len(BUILDERS[name]()[0].objects)
        i = planes["depth"][..., 2]
        assert np.array_equal(i, np.round(i)) and i.min() >= 0 and i.max() <= n_objects
        assert (planes["depth"][..., 1][i == 0] < 1).all()         # the first sample missed


# ---- 8: the two modes agree
# Both modes draw the same words and round the rays differently, so a silhouette pixel may see another object in its first sample
# and a few samples may change sides.  Measured on the MI355X at 96 x 72 x 16 (the test prints both figures): no pixel's id and no
# coverage value differs in either scene -- 0 of 6,912 pixels, largest coverage difference 0.0.  Asserted at three times that, which
# is still 0: at this size the two modes see the same objects sample by sample.
MODES_AGREE = {   # scene: (fraction of pixels whose ids differ, largest difference of the coverage planes), as measured
    "cornell": (0.0, 0.0),
    "monomial": (0.0, 0.0),
}


@pytest.mark.parametrize("name", ["cornell", "monomial"])
def test_modes_agree(name):
    w, h, spp = 96, 72, 16
    a = make(name, False, chunk=0, w=w, h=h).features_array(spp, albedo=False, normal=False)["depth"]
    b = make(name, True, chunk=0, w=w, h=h).features_array(spp, albedo=False, normal=False)["depth"]
    id_fraction = float((a[..., 2] != b[..., 2]).mean())
    cov = float(np.nanmax(np.abs(a[..., 1] - b[..., 1])))
    print(f"modes agree, {name}: ids differ in {id_fraction:.6f} of the pixels ({int((a[..., 2] != b[..., 2]).sum())}), "
          f"coverage differs by at most {cov:.6f}")
    bound_ids, bound_cov = MODES_AGREE[name]
    assert id_fraction <= 3 * bound_ids and cov <= 3 * bound_cov
