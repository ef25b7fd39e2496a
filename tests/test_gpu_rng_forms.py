"""The leaner draw forms on the device (device_core.h, RPT_RNG_FORMS): the generator's step against the oracle's generator word for
word, every changed draw form against the form it replaces (rpt_debug_draw_forms) and against the draws worked out on the host from
the oracle's words, and frames that must not depend on the grid.  Bit equality throughout; the two oracle bounds are the ones
test_render_matches_oracle_same_seed asserts for C2 and C3."""
import ctypes as C

import numpy as np
import pytest

from rpt_amd import Renderer, scenes
from rpt_amd import _lib
from rpt_amd.api import DRAW_FORM_WORDS, debug_draw_forms
from tests.util import rel_rms

pytestmark = pytest.mark.gpu

N_WORDS = 4096
SEEDS = (0, 1, 2 ** 63, 2 ** 64 - 1)
PIXELS = (0, 1, 2 ** 20 - 1, 2 ** 32 - 1)
SAMPLES = (0, 1, 255, 2 ** 32 - 1)


def _oracle_words(oracle_lib, seed, pixel, sample, n):
    exp = np.zeros(n, dtype=np.uint32)
    oracle_lib.orc_rng_u32(C.c_uint64(seed), pixel, sample, n, exp.ctypes.data_as(C.c_void_p))
    return exp


@pytest.mark.parametrize("seed", SEEDS)
def test_step_matches_the_oracles_generator(oracle_lib, seed):
    lib = _lib.load()
    for pixel in PIXELS:
        for sample in SAMPLES:
            got = np.zeros(N_WORDS, dtype=np.uint32)
            _lib.check(lib.rpt_debug_rng_u32(C.c_uint64(seed), pixel, sample, N_WORDS, got.ctypes.data_as(C.c_void_p)))
            exp = _oracle_words(oracle_lib, seed, pixel, sample, N_WORDS)
            assert exp.any() and np.array_equal(got, exp), (seed, pixel, sample)


def _host_forms(words):
    """The 274 words of rpt_debug_draw_forms for one lane from its stream's words.  fp64 holds a + (b - a) u exactly for these
    widths (24-bit a, 48-bit product, less than 53 bits from the top of one to the bottom of the other), so the one rounding to
    fp32 is the fma's."""
    out = np.zeros(DRAW_FORM_WORDS, dtype=np.uint32)
    k = (words >> np.uint32(9)).astype(np.int64)
    u = (2 * k[:64] + 1).astype(np.float64) * 2.0 ** -24
    for f, h in enumerate((np.float32(1.0), np.float32(1.0) / np.float32(64.0), np.float32(1.0) / np.float32(1024.0),
                           np.float32(1.0) / np.float32(3000.0))):
        a, b = -np.float64(h), np.float64(h)
        out[64 * f:64 * f + 64] = (a + (b - a) * u).astype(np.float32).view(np.uint32)
    below = (2 * k[:64] + 1).astype(np.float32) * np.float32(2.0 ** -24) < np.float32(0.8)
    for j in range(64):
        out[256 + j // 32] |= np.uint32(int(below[j]) << (j % 32))
    at, pairs = 0, 0
    while pairs < 8:
        ku, kv = k[at], k[at + 1]
        at += 2
        if ku + kv >= 1 << 23:      # `while u + v > 1 { redraw }`
            continue
        out[258 + 2 * pairs], out[259 + 2 * pairs] = ku, kv
        pairs += 1
    return out


def test_draw_forms_match_their_reference_forms(oracle_lib):
    n, seed = 1 << 20, 5
    new, ref = debug_draw_forms(seed, n)
    assert new.shape == (DRAW_FORM_WORDS, n)
    for lo, hi, what in ((0, 64, "range(-1, 1)"), (64, 128, "range(-1/64, 1/64)"), (128, 192, "range(-1/1024, 1/1024)"),
                         (192, 256, "range(-1/3000, 1/3000)"), (256, 258, "roulette"), (258, 274, "triangle pairs")):
        diff = int((new[lo:hi] != ref[lo:hi]).sum())
        print(f"{what}: {diff} of {(hi - lo) * n} words differ")
        assert diff == 0, what
    # ... and both are the draws of the oracle's stream, worked out on the host, for lanes across the range
    for lane in (0, 1, 63, 64, 255, 256, 4097, n // 2 + 3, n - 1):
        words = _oracle_words(oracle_lib, seed, lane, 0, 256)
        exp = _host_forms(words)
        assert np.array_equal(new[:, lane], exp), lane
    # the draws are draws: ranges inside their interval, roulette near 0.8, pairs accepted
    r = new[:64].view(np.float32)
    assert r.min() > -1.0 and r.max() < 1.0 and abs(float(r.mean())) < 1e-3
    inv = new[192:256].view(np.float32)
    assert np.abs(inv).max() < np.float32(1.0) / np.float32(3000.0)
    bits = np.unpackbits(new[256:258].view(np.uint8)).mean()
    assert abs(bits - 0.8) < 1e-3
    assert np.all(new[258:274:2].astype(np.int64) + new[259:274:2] < 1 << 23)


@pytest.mark.parametrize("name,tol", [("C3", 3e-3), ("C2", 2e-3)])
def test_frames_do_not_depend_on_the_grid(name, tol):
    """64x64x8 on the default grid (every lane at most one item) and on one block (16 or more items per lane): the same frame, inside
    the bound of test_render_matches_oracle_same_seed for the scene."""
    from oracle.pyoracle import OracleScene
    scene, cam, cfg = scenes.CONFIGS[name]()
    size, spp = 64, 8
    r = Renderer(scene, cam).width(size).height(size).max_bounces(cfg["max_bounces"]).seed(3)
    _, n_chunks = r.chunking(spp)
    n_items = ((size + 31) // 32) ** 2 * 1024 * n_chunks
    scene.set_option("timing", 1)
    frames = []
    try:
        for cap in (0, 1):
            scene.set_option("max_blocks", cap)
            r._sample_offset = 0
            frames.append(r.sample_array(spp))
            blocks = r.timing()[2]
            print(f"{name}: max_blocks {cap} -> {blocks} blocks, {n_items} items, {n_items / (blocks * 256):.2f} per lane")
            if cap == 0:
                assert n_items <= blocks * 256, (name, "not the isolated launch", n_items, blocks)
            else:
                assert blocks == cap and n_items >= 8 * blocks * 256, (name, "too few items per lane", n_items, blocks)
    finally:
        scene.set_option("max_blocks", 0)
    assert np.all(np.isfinite(frames[0])) and frames[0].mean() > 0
    assert np.array_equal(frames[0], frames[1]), name
    exp = OracleScene(scene).render(cam, size, size, spp, cfg["max_bounces"], seed=3, robust=1)
    err = rel_rms(frames[0], exp)
    print(f"{name}: rel. RMS against the oracle {err:.3e} (bound {tol:g})")
    assert err < tol, (name, err)
