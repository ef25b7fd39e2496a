"""rpt_debug_shadow_test, rpt_shadow_scan_info, rpt_debug_distance_pair and the option "shadow_scan", without a GPU: what the caller
got wrong is RPT_ERR_INVALID (-1) and is said before the scene's state; a well-formed call on a scene that was never committed is
RPT_ERR_STATE (-2).  And the integer identity behind the light-triangle sampler's rejection test, on the CPU."""
import ctypes as C

import numpy as np

from rpt_amd import Material, _lib, sphere, vec3
from rpt_amd.api import material_desc, shape_desc


def _scene_with_an_ambient_and_an_object_light(lib):
    h = lib.rpt_scene_create()
    col = np.array([1.0, 1.0, 1.0])
    assert lib.rpt_scene_add_light_ambient(h, col.ctypes.data_as(C.POINTER(C.c_double))) == 0
    sd, keep = shape_desc(sphere().translate(vec3(0, 3, 0)), _lib.ShapeDesc)
    md = material_desc(Material.light(vec3(1, 1, 1), 5.0), _lib.MaterialDesc)
    assert lib.rpt_scene_add_light_object(h, C.byref(sd), C.byref(md)) >= 0
    return h


def test_shadow_test_hook_validates_its_arguments_without_a_gpu():
    lib = _lib.load()
    h = _scene_with_an_ambient_and_an_object_light(lib)
    try:
        p = np.zeros(16).ctypes.data
        # rpt_debug_shadow_test(scene, light, n, origins, dirs, dist, out_flag, out_t)
        assert lib.rpt_debug_shadow_test(None, 1, 1, p, p, p, p, p) == -1
        for k in range(5):                                                       # each array in turn
            args = [p] * 5
            args[k] = None
            assert lib.rpt_debug_shadow_test(h, 1, 1, *args) == -1 and b"null" in lib.rpt_last_error()
        assert lib.rpt_debug_shadow_test(h, 0, 1, p, p, p, p, p) == -1 and b"Light::Object" in lib.rpt_last_error()   # the ambient light
        assert lib.rpt_debug_shadow_test(h, 2, 1, p, p, p, p, p) == -1                                                # no such light
        assert lib.rpt_debug_shadow_test(h, 1, 1, p, p, p, p, p) == -2 and b"commit" in lib.rpt_last_error()
        out = (C.c_uint32 * 4)()
        assert lib.rpt_shadow_scan_info(None, 1, out) == -1 and lib.rpt_shadow_scan_info(h, 1, None) == -1
        assert lib.rpt_shadow_scan_info(h, 0, out) == -1 and b"Light::Object" in lib.rpt_last_error()
        assert lib.rpt_shadow_scan_info(h, 1, out) == -2 and b"commit" in lib.rpt_last_error()
    finally:
        lib.rpt_scene_destroy(h)


def test_distance_pair_hook_validates_its_arguments_without_a_gpu():
    lib = _lib.load()
    p = np.zeros(16).ctypes.data
    # rpt_debug_distance_pair(sigma_t, k0, n, out_new, out_guarded)
    assert lib.rpt_debug_distance_pair(0.003, 0, 1, None, p) == -1 and b"null" in lib.rpt_last_error()
    assert lib.rpt_debug_distance_pair(0.003, 0, 1, p, None) == -1 and b"null" in lib.rpt_last_error()
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        assert lib.rpt_debug_distance_pair(bad, 0, 1, p, p) == -1 and b"sigma_t" in lib.rpt_last_error()
    assert lib.rpt_debug_distance_pair(0.003, 1 << 23, 1, p, p) == -1 and b"23 bits" in lib.rpt_last_error()
    assert lib.rpt_debug_distance_pair(0.003, (1 << 23) - 1, 2, p, p) == -1 and b"23 bits" in lib.rpt_last_error()
    assert lib.rpt_debug_distance_pair(0.003, 5, (1 << 23) - 4, p, p) == -1
    assert lib.rpt_debug_distance_pair(0.003, (1 << 23) - 1, 0, p, p) == 0                  # nothing to do
    assert lib.rpt_debug_distance_pair(0.003, 0, 0, p, p) == 0


def test_the_option_has_its_name():
    lib = _lib.load()
    h = lib.rpt_scene_create()
    try:
        assert lib.rpt_scene_set_option(h, b"shadow_scan", 0) == 0 and lib.rpt_scene_set_option(h, b"shadow_scan", 1) == 0
        assert lib.rpt_scene_set_option(h, b"shadow_scans", 1) < 0                          # (an unknown name is an error)
    finally:
        lib.rpt_scene_destroy(h)


def test_rejection_by_carry_is_rejection_by_sum():
    """Mesh::sample redraws while u + v > 1; on the draws' words a, b (u = (2 (a >> 9) + 1) 2^-24) that is (a >> 9) + (b >> 9) >= 2^23.
    The sampler tests the carry of (a & ~511) + (b & ~511) out of 32 bits instead: the masked words are 512 (a >> 9) and
    512 (b >> 9), so their sum reaches 2^32 exactly when the sum of the shifted ones reaches 2^23."""
    rng = np.random.default_rng(7)
    a = rng.integers(0, 1 << 32, size=10_000_000, dtype=np.uint64)
    b = rng.integers(0, 1 << 32, size=10_000_000, dtype=np.uint64)
    edge = np.array([0, 1, 511, 512, 513, (1 << 31) - 512, (1 << 31) - 1, 1 << 31, (1 << 31) + 511, (1 << 31) + 512,
                     (1 << 32) - 1024, (1 << 32) - 513, (1 << 32) - 512, (1 << 32) - 1], dtype=np.uint64)
    ea, eb = (g.ravel() for g in np.meshgrid(edge, edge))
    # pairs on both sides of the boundary ku + kv = 2^23, with every combination of low bits at their extremes
    ku = rng.integers(0, 1 << 23, size=4096, dtype=np.uint64)
    low = np.array([0, 1, 255, 510, 511], dtype=np.uint64)
    ba, bb = [], []
    for d in (-2, -1, 0, 1, 2):
        kv = ((1 << 23) + d - ku.astype(np.int64))
        ok = (kv >= 0) & (kv < (1 << 23))
        for la in low:
            for lb in low:
                ba.append((ku[ok] << np.uint64(9)) | la)
                bb.append((kv[ok].astype(np.uint64) << np.uint64(9)) | lb)
    a = np.concatenate([a, ea, np.concatenate(ba)])
    b = np.concatenate([b, eb, np.concatenate(bb)])
    mask = np.uint64(0xFFFFFE00)
    carry = ((a & mask) + (b & mask)) >= np.uint64(1 << 32)
    by_sum = ((a >> np.uint64(9)) + (b >> np.uint64(9))) >= np.uint64(1 << 23)
    # the device forms the carry with a 32-bit add: the same thing as the wrapped sum being smaller than an operand
    wrapped = ((a & mask) + (b & mask)) & np.uint64(0xFFFFFFFF)
    assert np.array_equal(carry, wrapped < (a & mask))
    assert carry.any() and (~carry).any()
    assert np.array_equal(carry, by_sum)
