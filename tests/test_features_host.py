"""First-hit feature planes, the parts that need no GPU: the summation order of the interface as tests/feature_ref.py restates it,
the argument checks of rpt_render_features* that precede every device call, and the Python methods."""
import ctypes as C

import numpy as np
import pytest

from rpt_amd import Camera, Renderer, Scene, _lib
from rpt_amd.api import camera_desc
from tests.feature_ref import reduce_samples

# fp64 sums of these depend on the order: 1 is lost next to 2^53 unless the two large terms cancel first
BIG = 2.0 ** 53


def test_reduction_is_chunked_in_sample_order():
    x = np.array([BIG, 1.0, 1.0, -BIG])[:, None]
    assert BIG + 1.0 == BIG and 1.0 - BIG == -(BIG - 1.0) != -BIG
    # one chunk, in sample order: ((BIG + 1) + 1) - BIG = 0, both ones lost
    assert reduce_samples(x, 4)[0] == 0.0
    # chunks of 1: the chunk sums added in chunk order, the same additions
    assert reduce_samples(x, 1)[0] == 0.0
    # chunks of 2: (BIG + 1) + (1 - BIG) = BIG - (BIG - 1) = 1, one of them kept
    assert reduce_samples(x, 2)[0] == 1.0 / 4.0
    # chunks of 3, the last one ragged: ((BIG + 1) + 1) + (-BIG) = 0
    assert reduce_samples(x, 3)[0] == 0.0
    # the samples in another order: ((-BIG + 1) + 1) + BIG = 2, both kept
    assert reduce_samples(x[::-1], 4)[0] == 2.0 / 4.0


def test_reduction_divides_and_keeps_shapes():
    rng = np.random.default_rng(5)
    x = rng.uniform(-1, 1, size=(10, 7, 8))
    got = reduce_samples(x, 4)
    assert got.shape == (7, 8)
    want = (((x[0] + x[1]) + x[2]) + x[3]) + (((x[4] + x[5]) + x[6]) + x[7]) + (x[8] + x[9])
    assert np.array_equal(got, want / 10.0)                     # a division, not a multiplication by 0.1
    assert np.array_equal(reduce_samples(x[:1], 4), x[0])       # one sample, one chunk
    third = np.full((3, 1), 1.0)
    assert reduce_samples(third, 2)[0] == 1.0                   # 3 / 3, where 3 * (1 / 3) would do as well: the shape of the call only
    assert np.signbit(reduce_samples(np.array([[-0.0], [-0.0]]), 1)[0]) == False   # noqa: E712  (sums start from +0.0)


def _call(lib, scene, cam, prm, iterations, planes, device=False):
    fn = lib.rpt_render_features_device if device else lib.rpt_render_features
    args = [scene, cam, prm, iterations, C.c_uint64(1), 0] + [p.ctypes.data_as(C.c_void_p) if p is not None else None for p in planes]
    return fn(*args, None) if device else fn(*args)


@pytest.mark.parametrize("device", [False, True])
def test_argument_checks_precede_every_device_call(device):
    """No scene is committed and no GPU is needed: each refusal is RPT_ERR_INVALID (-1)."""
    lib = _lib.load()
    h = lib.rpt_scene_create()
    try:
        cam = C.byref(camera_desc(Camera(), _lib.CameraDesc))
        prm = C.byref(_lib.RenderParams(8, 8, 0.0, 0, 0, 1))
        plane = np.zeros((8, 8, 3))
        assert _call(lib, h, cam, prm, 4, [None, None, None], device) == -1
        assert _call(lib, None, cam, prm, 4, [plane, plane, plane], device) == -1
        assert _call(lib, h, None, prm, 4, [plane, None, None], device) == -1
        assert _call(lib, h, cam, None, 4, [None, plane, None], device) == -1
        assert _call(lib, h, cam, prm, 0, [None, None, plane], device) == -1
        assert b"empty render" in lib.rpt_last_error()
        # with everything in order the next refusal is the call order: the scene is not committed
        assert _call(lib, h, cam, prm, 4, [plane, None, None], device) == -2
    finally:
        lib.rpt_scene_destroy(h)


def test_python_methods_reject_an_empty_request():
    r = Renderer(Scene(), Camera()).width(8).height(8)
    with pytest.raises(ValueError):
        r.features_array(4, albedo=False, normal=False, depth=False)
    with pytest.raises(ValueError):
        r.features_device(4, 0, 0, 0)
    with pytest.raises(ValueError):
        r.features_device(4, None, None, None, stream_ptr=0)
