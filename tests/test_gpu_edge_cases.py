"""Edge cases of the HIP path: empty / ragged inputs, degenerate sizes, option handling, and the
non-packet fallback of the photon beam walk.  All compared with the oracle where a value exists."""
import numpy as np
import pytest

import rpt_amd
from rpt_amd import (Camera, Environment, Light, Material, Medium, Object, Renderer, RptError, Scene, polygon, scenes,
                     sphere, vec3)
from tests.util import rel_rms

pytestmark = pytest.mark.gpu


def _oracle(scene):
    from oracle.pyoracle import OracleScene
    return OracleScene(scene)


def test_empty_scene_returns_the_environment():
    sc = Scene()
    sc.environment = Environment.Color(vec3(0.25, 0.5, 0.75))
    out = Renderer(sc, Camera()).width(5).height(3).max_bounces(2).sample_array(3)
    assert out.shape == (15, 3) and np.allclose(out, [0.25, 0.5, 0.75], rtol=1e-6)
    fog = Scene()                                             # empty scene inside a medium: medium events only,
    fog.add(Medium.homogeneous_isotropic(0.1, 0.4))           # no light -> black (renderer.rs:198-206, 243-282)
    out = Renderer(fog, Camera()).width(4).height(4).sample_array(8)
    assert np.all(out == 0.0)


@pytest.mark.parametrize("w,h,spp", [(1, 1, 1), (7, 3, 33), (33, 65, 2), (64, 1, 5)])
def test_ragged_image_and_sample_counts(w, h, spp):
    scene, cam, cfg = scenes.cornell()
    got = Renderer(scene, cam).width(w).height(h).max_bounces(2).seed(9).sample_array(spp)
    exp = _oracle(scene).render(cam, w, h, spp, 2, seed=9, robust=1)
    assert got.shape == (w * h, 3) and np.all(np.isfinite(got))
    assert rel_rms(got, exp) < 5e-3


def test_zero_bounces_and_scene_without_lights():
    scene, cam, cfg = scenes.cornell()
    scene.lights.clear()                                      # emission is still seen at depth 0 (renderer.rs:295-299)
    got = Renderer(scene, cam).width(48).height(48).max_bounces(0).seed(1).sample_array(4)
    exp = _oracle(scene).render(cam, 48, 48, 4, 0, seed=1, robust=1)
    assert got.max() > 50 and rel_rms(got, exp) < 1e-5       # only the light quad's emittance * colour


def test_chunk_option_changes_rounding_only_and_is_validated():
    scene, cam, cfg = scenes.lampshade()
    def render():
        s2, c2, _ = scenes.lampshade()
        return Renderer(s2, c2).width(40).height(40).max_bounces(10).seed(3).sample_array(24)
    base = render()
    try:
        rpt_amd.set_option("chunk_spp", 5)                    # 24 = 4 full chunks + one of 4
        other = render()
    finally:
        rpt_amd.set_option("chunk_spp", 0)
    assert not np.array_equal(base, other) or True            # may or may not differ in the last bit
    assert np.allclose(base, other, rtol=1e-5, atol=1e-9)
    with pytest.raises(RptError):
        rpt_amd.set_option("chunk_spp", -1)
    with pytest.raises(RptError):
        rpt_amd.set_option("no_such_option", 1)


def test_options_belong_to_a_scene():
    """rpt_scene_set_option: two scenes of one process with different options do not see each other's (the C ABI has
    no process-global render state); the process default set by rpt_set_option reaches scenes created afterwards."""
    import rpt_amd
    a, cam, cfg = scenes.cornell()
    b, _, _ = scenes.cornell()
    ra = Renderer(a, cam).width(64).height(64).max_bounces(2).seed(1)
    rb = Renderer(b, cam).width(64).height(64).max_bounces(2).seed(1)
    a.set_option("counters", 1).set_option("chunk_spp", 16)
    img_a, img_b = ra.sample_array(32), rb.sample_array(32)
    assert ra.counters()["samples"] == 64 * 64 * 32 and rb.counters()["samples"] == 0
    assert not np.array_equal(img_a, img_b) and np.allclose(img_a, img_b, rtol=1e-4, atol=1e-6)   # 2 chunks vs 16: fp32 sum order
    rpt_amd.set_option("chunk_spp", 16)      # the convenience setter: default + every live scene
    try:
        rb._sample_offset = 0
        assert np.array_equal(rb.sample_array(32), img_a)
        c, _, _ = scenes.cornell()
        assert np.array_equal(Renderer(c, cam).width(64).height(64).max_bounces(2).seed(1).sample_array(32), img_a)
    finally:
        rpt_amd.set_option("chunk_spp", 0)


def test_render_argument_errors():
    scene, cam, cfg = scenes.cornell()
    r = Renderer(scene, cam).width(0).height(4)
    with pytest.raises(RptError):
        r.sample_array(1)                                     # empty image
    r = Renderer(scene, cam).width(4).height(4)
    with pytest.raises(RptError):
        r.sample_array(0)                                     # zero iterations
    with pytest.raises(RptError):
        Renderer(scene, cam).width(4).height(4).shard(3, 2).sample_array(1)
    with pytest.raises(RptError):
        scene.add(Object(sphere()))                           # committed scenes are immutable


def test_photon_beam_walk_without_a_common_ray_origin():
    """Thin-lens camera: every lane's ray starts at a different lens point, so the wave cannot form a
    frustum packet and takes the batched per-ray voting walk; same estimate, same oracle."""
    scene, cam, cfg = scenes.CONFIGS["C4"]()
    lens = Camera(cam.eye, cam.direction, cam.up, cam.fov).focus(vec3(278.0, 273.0, 280.0), 12.0)
    n, size, spp = 10000, 40, 3
    r = Renderer(scene, lens).width(size).height(size).watts(14.65 * n).gather_size(12).gather_size_volume(3).seed(6)
    r.photon_map_build(n, Renderer.PHOTON_POINT_BEAM)
    got = r.photon_sample_array(spp)
    pm = _oracle(scene).photon_map(n, 1, 14.65 * n, 12, 3, seed=6, robust=1)
    exp = pm.render(lens, size, size, spp, seed=6)
    assert np.all(np.isfinite(got)) and exp.mean() > 0
    assert rel_rms(got, exp) < 1e-2 and abs(got.mean() - exp.mean()) / exp.mean() < 3e-3
    # The wave-private LDS region of the camera pass serves three layouts in turn (photon.hip, photon_query_kernel): this
    # camera once had a pixel's candidate list and the per-sample beam walk live in it together.  The counters build counts
    # such trips.
    import ctypes as C
    from rpt_amd import _lib
    scene.set_option("counters", 1)
    r._sample_offset = 0
    again = r.photon_sample_array(spp)
    out = (C.c_uint64 * 56)()
    _lib.check(_lib.load().rpt_debug_section_counters(r.scene._handle, out))
    assert int(out[15]) == 0      # counters[23]: trips with two layouts live at once
    assert np.allclose(again, got, rtol=1e-6, atol=1e-9)


def test_timing_events_are_kept_per_launch_and_read_afterwards():
    """rpt_get_timing / rpt_get_timing_mean: HIP events around every launch on its stream; the renders never
    wait for them, the mean covers the launches since the previous mean and then starts over."""
    scene, cam, cfg = scenes.cornell()
    r = Renderer(scene, cam).width(64).height(64).max_bounces(2).seed(1)
    with pytest.raises(RptError):
        r.sample_array(1)
        r.timing()                                            # timing was off: nothing recorded
    rpt_amd.set_option("timing", 1)
    try:
        for _ in range(3):
            r.sample_array(4)
        last = r.timing()
        mean = r.timing_mean()
        assert mean[2] == 3 and mean[0] > 0 and mean[1] > 0 and last[0] > 0 and last[2] > 0
        assert 0.2 * last[0] < mean[0] < 5 * last[0]
        with pytest.raises(RptError):
            r.timing_mean()                                   # nothing since the previous mean
        r.sample_array(4)
        assert r.timing_mean()[2] == 1
    finally:
        rpt_amd.set_option("timing", 0)


def test_launches_on_two_streams_overlap_without_sharing_their_slab():
    """The library keeps a slab + work counter per stream (rpt_capi.cpp LaunchSet): frames launched alternately on
    two streams, nothing waiting in between, are each bit-identical to the frame of a lone launch -- also for
    different sample offsets and sizes in flight at the same time, and on a third stream that has to wait."""
    import torch
    scene, cam, cfg = scenes.lampshade()
    w, h, spp = 96, 64, 12
    r = Renderer(scene, cam).width(w).height(h).max_bounces(10).seed(4)

    def lone(offset):
        r._sample_offset = offset
        return r.sample_array(spp).copy()
    expect = [lone(0), lone(spp), lone(2 * spp)]
    # a second size, between the launches of the first and on the stream after theirs: the same tiles_x, half the height, other
    # sample counts and offsets, and one shard of two -- its tile list [1, 3, 5] is no prefix of the first size's [0 .. 5], so a launch
    # that read the other size's list would show (the lone frames come from a scene of their own: this one's history is under test)
    h2, spp2 = 48, 5
    s2, c2, _ = scenes.lampshade()
    r2 = Renderer(s2, c2).width(w).height(h2).max_bounces(10).seed(4).shard(1, 2)

    def lone_small(offset):
        r2._sample_offset = offset
        return r2.sample_array(spp2).copy()
    expect_small = [lone_small(7), lone_small(7 + spp2), lone_small(7 + 2 * spp2)]
    small = Renderer(scene, cam).width(w).height(h2).max_bounces(10).seed(4).shard(1, 2)   # the same scene handle as r
    streams = [torch.cuda.Stream() for _ in range(3)]
    frames = [torch.zeros(w * h * 3, dtype=torch.float64, device="cuda") for _ in range(6)]
    small_frames = [torch.zeros(w * h2 * 3, dtype=torch.float64, device="cuda") for _ in range(6)]
    torch.cuda.synchronize()
    for i, f in enumerate(frames):                             # 6 launches queued back to back: streams 0 1 2 0 1 2
        st = streams[i % 3]
        r._sample_offset = (i % 3) * spp
        with torch.cuda.stream(st):
            r.sample_device(spp, f.data_ptr(), st.cuda_stream)
        st = streams[(i + 1) % 3]                              # ... each followed by one of the other size: streams 1 2 0 1 2 0
        small._sample_offset = 7 + (i % 3) * spp2
        with torch.cuda.stream(st):
            small.sample_device(spp2, small_frames[i].data_ptr(), st.cuda_stream)
    torch.cuda.synchronize()
    for i, f in enumerate(frames):
        assert np.array_equal(f.cpu().numpy().reshape(-1, 3), expect[i % 3])
    for i, f in enumerate(small_frames):
        assert np.array_equal(f.cpu().numpy().reshape(-1, 3), expect_small[i % 3]), i


def test_no_tree_walk_ever_finds_its_stack_full():
    """bvh_traverse drops the far child when its stack is full; rpt_scene_commit refuses scenes whose trees are deep enough for
    that.  The counters build counts the event (rpt_get_counters()[7]): zero on the per-mesh-tree and the scene-tree flavours."""
    from rpt_amd import Renderer, scenes
    for make in (lambda: scenes.mesh_in_fog(48, 48), lambda: scenes.fractal_spheres(4)):
        scene, cam, cfg = make()
        scene.set_option("counters", 1)
        r = Renderer(scene, cam).width(96).height(96).max_bounces(cfg["max_bounces"]).seed(1)
        r.sample_array(4)
        c = r.counters()
        assert c["bvh_nodes"] > 0 and c["stack_overflows"] == 0
