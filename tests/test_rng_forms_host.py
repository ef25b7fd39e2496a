"""The integer identities behind the leaner draw forms (device_core.h, RPT_RNG_FORMS), stated in numpy, and the argument checks of the hook that runs
the forms on the device: no GPU.

  roulette   uniform() < 0.8f on the draw's word: float32(2k+1) 2^-24 < float32(0.8)  <=>  word < 0xCCCCCC00, k = word >> 9
  one mask   (a & ~511) + b carries out of 32 bits exactly when (a & ~511) + (b & ~511) does, i.e. when ku + kv >= 2^23
  step       xoshiro128+ with the intermediate values substituted (three xor3 and one xor) is the reference's eight assignments"""
import numpy as np

T_08 = 0xCCCCCC00
M32 = np.uint64(0xFFFFFFFF)


def test_roulette_threshold_for_every_draw():
    k = np.arange(1 << 23, dtype=np.uint32)
    u = (2 * k + 1).astype(np.float32) * np.float32(2.0 ** -24)
    assert u.dtype == np.float32
    below = u < np.float32(0.8)
    for low in (0, 511):
        word = (k << np.uint32(9)) | np.uint32(low)
        assert np.array_equal(below, word < np.uint32(T_08)), low
    # the fp64 path reads the same draw as a double and compares it with the double 0.8: the same cut
    assert np.array_equal((2 * k.astype(np.float64) + 1) * 2.0 ** -24 < 0.8, below)
    assert below.sum() == T_08 >> 9 and np.float32(0.8) == np.float32(13421773 * 2.0 ** -24)


def _carries(a, b):
    """(carry out of (a & ~511) + (b & ~511), carry out of (a & ~511) + b, ku + kv >= 2^23) for uint32 words a, b."""
    a, b = a.astype(np.uint64), b.astype(np.uint64)
    am, bm = a & np.uint64(0xFFFFFE00), b & np.uint64(0xFFFFFE00)
    return (am + bm) >> np.uint64(32) != 0, (am + b) >> np.uint64(32) != 0, (a >> np.uint64(9)) + (b >> np.uint64(9)) >= (1 << 23)


def test_one_mask_carry_identity():
    rng = np.random.default_rng(7)
    a = rng.integers(0, 1 << 32, 10 ** 7, dtype=np.uint64).astype(np.uint32)
    b = rng.integers(0, 1 << 32, 10 ** 7, dtype=np.uint64).astype(np.uint32)
    both, one, reject = _carries(a, b)
    assert np.array_equal(both, one) and np.array_equal(one, reject)
    assert 0.45 < reject.mean() < 0.55
    # corners: ku + kv around 2^23, low nine bits all clear or all set on either side
    ku = np.concatenate([np.arange(0, 1 << 23, 4099, dtype=np.int64), np.array([0, 1, (1 << 22) - 1, 1 << 22, (1 << 23) - 2, (1 << 23) - 1])])
    seen = set()
    for total in ((1 << 23) - 2, (1 << 23) - 1, 1 << 23, (1 << 23) + 1):
        kv = total - ku
        ok = (kv >= 0) & (kv < (1 << 23))
        for la in (0, 511):
            for lb in (0, 511):
                wa = ((ku[ok] << 9) | la).astype(np.uint32)
                wb = ((kv[ok] << 9) | lb).astype(np.uint32)
                both, one, reject = _carries(wa, wb)
                assert np.array_equal(both, one) and np.array_equal(one, reject), (total, la, lb)
                assert np.all(reject == (total >= (1 << 23))), (total, la, lb)
                seen.add(bool(reject[0]))
    assert seen == {False, True}


def _rotl(x, r):
    return ((x << np.uint64(r)) | (x >> np.uint64(32 - r))) & M32


def _step_ref(s0, s1, s2, s3):
    r = (s0 + s3) & M32
    t = (s1 << np.uint64(9)) & M32
    s2 = s2 ^ s0
    s3 = s3 ^ s1
    s1 = s1 ^ s2
    s0 = s0 ^ s3
    s2 = s2 ^ t
    s3 = _rotl(s3, 11)
    return r, (s0, s1, s2, s3)


def _step_new(a, b, c, d):
    x3 = lambda x, y, z: x ^ y ^ z  # noqa: E731
    r = (a + d) & M32
    t = (b << np.uint64(9)) & M32
    return r, (x3(a, d, b), x3(b, c, a), x3(c, a, t), _rotl(d ^ b, 11))


def test_step_identity():
    rng = np.random.default_rng(11)
    state = tuple(rng.integers(0, 1 << 32, 10 ** 6, dtype=np.uint64) for _ in range(4))
    # states with few bits set and with all of them set: every term of every xor is seen alone
    edge = np.array([0, 1, 1 << 22, 1 << 23, 1 << 31, 0xFFFFFFFF], dtype=np.uint64)
    grid = np.stack(np.meshgrid(edge, edge, edge, edge, indexing="ij")).reshape(4, -1)
    state = tuple(np.concatenate([s, g]) for s, g in zip(state, grid))
    ref, new = state, state
    for _ in range(4):      # a few steps in a row: the new state feeds the next output
        r_ref, ref = _step_ref(*ref)
        r_new, new = _step_new(*new)
        assert np.array_equal(r_ref, r_new)
        for x, y in zip(ref, new):
            assert np.array_equal(x, y)


def test_draw_forms_hook_validates_its_arguments_without_a_gpu():
    import ctypes as C

    from rpt_amd import _lib
    from rpt_amd.api import DRAW_FORM_WORDS
    lib = _lib.load()
    buf = (C.c_uint32 * DRAW_FORM_WORDS)()
    p = C.cast(buf, C.c_void_p)
    assert lib.rpt_debug_draw_forms(C.c_uint64(0), 1, None, p) == -1 and b"null" in lib.rpt_last_error()
    assert lib.rpt_debug_draw_forms(C.c_uint64(0), 1, p, None) == -1 and b"null" in lib.rpt_last_error()
    assert lib.rpt_debug_draw_forms(C.c_uint64(0), (1 << 20) + 1, p, p) == -1 and b"2^20" in lib.rpt_last_error()
    assert lib.rpt_debug_draw_forms(C.c_uint64(0), 0, p, p) == 0                      # nothing to do
