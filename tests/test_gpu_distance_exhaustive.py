"""The medium distance -ln(xi) / sigma_t of the render kernels (medium_distance in kernels.hip: the bare v_log_f32 and the two-word
product with ln 2, written out) against the guarded formula it replaced, -__logf(xi) * inv_sigma_t, kept as it was
(medium_distance_guarded): for EVERY draw xi = (2 k + 1) 2^-24, k = 0 .. 2^23 - 1, and the extinction of C3 and of C4, the two are
the same 32 bits.  The reference is the guarded formula, not the new code; no draw is left out."""
import numpy as np
import pytest

from rpt_amd import scenes
from rpt_amd.api import debug_distance_pair

pytestmark = pytest.mark.gpu

N_DRAWS = 1 << 23


def _sigma_t(make):
    """absorption + scattering of the scene's medium, added in fp32 as the kernels add them."""
    scene = make()[0]
    (m,) = scene.media
    return np.float32(m.absorption) + np.float32(m.scattering)


@pytest.mark.parametrize("name", ["C3", "C4"])
def test_every_draw_gives_the_guarded_formulas_bits(name):
    sigma_t = _sigma_t(scenes.CONFIGS[name])
    new, guarded = debug_distance_pair(sigma_t, 0, N_DRAWS)
    assert new.shape == (N_DRAWS,) and guarded.shape == (N_DRAWS,)
    # the reference is what it should be: -ln(xi) / sigma_t, positive, finite, falling with k (a loose bound: it only has to show that
    # the guarded column is the logarithm -- v_log_f32 is good to about 1e-7 of log2(xi), which near xi = 1 is an absolute error)
    k = np.arange(0, N_DRAWS, 4099, dtype=np.int64)
    exact = -np.log((2.0 * k + 1.0) * 2.0 ** -24) / np.float64(sigma_t)
    assert np.all(np.isfinite(guarded)) and np.all(guarded > 0)
    assert np.all(np.abs(guarded[k] - exact) <= 1e-5 * exact + 1e-6 / np.float64(sigma_t))
    assert np.all(np.diff(guarded[k]) < 0)
    differ = np.flatnonzero(new.view(np.uint32) != guarded.view(np.uint32))
    print(f"{name}: sigma_t {float(sigma_t)!r}, {N_DRAWS} draws, {differ.size} differ"
          + (f", first k = {int(differ[0])}: {new[differ[0]]!r} against {guarded[differ[0]]!r}" if differ.size else ""))
    assert differ.size == 0


def test_a_window_of_draws_is_the_same_slice():
    """k0 > 0: the hook's window is draws k0 .. k0 + n - 1 (the last draw included)."""
    sigma_t = _sigma_t(scenes.CONFIGS["C3"])
    full = debug_distance_pair(sigma_t, N_DRAWS - 4096, 4096)
    part = debug_distance_pair(sigma_t, N_DRAWS - 100, 100)
    assert np.array_equal(part[0].view(np.uint32), full[0][-100:].view(np.uint32))
    assert np.array_equal(part[1].view(np.uint32), full[1][-100:].view(np.uint32))
    exact = -np.log((2.0 * (N_DRAWS - 1) + 1.0) * 2.0 ** -24) / np.float64(sigma_t)
    assert abs(float(part[1][-1]) - exact) <= 1e-5 * exact + 1e-6 / np.float64(sigma_t)
