"""Point x point (RPT_PHOTON_MAP, kind 0) and beam x beam (RPT_PHOTON_BEAM_BEAM, kind 2) maps built from hand-made records, pixel
by pixel, through the C ABI -- the fp32 mode only: the reference-epsilon mode refuses rpt_photon_map_from_records.

Every pixel of every p-* and b-* family of tests/photon_cases.py is compared with the fp64 brute-force restatement of
tests/photon_ref.py (`Restated(kind=0 / 2)`) under that module's rule: the cloud around the query -- for kind 0 the sampled distance
moves too --, decided and undecided pixels, the fp32 bounds stated in its docstring.  The settings are those of
tests/test_gpu_photon_records.py under which these kinds' values could differ: the default, one surface search per lane, a grid of
three blocks.  "photon_block_lists" builds candidate lists for the beam x point estimate alone; "photon_parts" does cut the work items of
every kind into strips, but what it changes -- the order of a pixel's beam x point terms, where the surface gather's carried radius and
anchor start afresh -- is a starting guess of an exact search and no per-pixel value of kind 0 or 2.  DESIGN.md ("Point x point and beam x beam
maps from hand-made records") holds the family table, the measured error / bound and the mutation counts.

b-eye -- a beam whose line passes exactly through the eye -- is NaN in all 576 pixels of the reference (l x b = 0, its tests are
rejections that a NaN passes); visit_beam's tests are written the same way and the device's 576 pixels are NaN too.  b-lens looks
through a thin lens: with several samples per pixel the lanes' rays share no origin and the walk falls back to beam_walk_batch, which
the counters build shows."""
import ctypes as C

import numpy as np
import pytest

from tests import photon_cases as pc
from tests import photon_ref as pr
from tests import test_gpu_photon_records as base

pytestmark = pytest.mark.gpu

SETTINGS = {k: base.SETTINGS[k] for k in ("default", "coop-off", "blocks-3")}
XFAIL = {}
NAMES = pc.POINT_NAMES + pc.BEAM_NAMES


def _apply_rule(name, setting, frames):
    case = pc.family(name)
    r = base._build(case, options=SETTINGS[setting])
    bad = 0
    for w, h, s in frames:
        got = base._frame(r, w, h, s)
        n_bad, worst = pr.report(f"{name} [{setting}] {w}x{h} sample {s}", pc.answers(name, w, h, s), got)
        bad += n_bad
    assert bad == 0


def _params(names, settings):
    out = []
    for name in names:
        for setting in settings:
            marks = [pytest.mark.xfail(strict=True, reason=XFAIL[(name, setting)])] if (name, setting) in XFAIL else []
            out.append(pytest.param(name, setting, marks=marks, id=f"{name}-{setting}"))
    return out


@pytest.mark.parametrize("name,setting", _params(NAMES, ["default"]))
def test_every_pixel_of_a_family_under_the_default_settings(name, setting):
    """Every frame of the family: 24 x 24, and 50 x 37 (clipped 8 x 8 blocks, another sample offset) for the controls."""
    _apply_rule(name, setting, pc.family(name).frames)


@pytest.mark.parametrize("name,setting", _params(NAMES, [s for s in SETTINGS if s != "default"]))
def test_every_pixel_of_a_family_under_each_setting(name, setting):
    """One surface search per lane, a grid of three blocks: each against the reference, not against the default."""
    _apply_rule(name, setting, pc.family(name).frames[:1])


@pytest.mark.parametrize("name", ["p-control", "b-control"])
def test_a_ragged_frame_on_three_blocks(name):
    """50 x 37 under max_blocks 3: clipped pixel blocks, many work items per block."""
    _apply_rule(name, "blocks-3", pc.family(name).frames[1:])


@pytest.mark.parametrize("name", ["p-control", "p-wall", "p-edge", "p-K57", "p-K100", "b-control", "b-thin", "b-lens"])
def test_seventy_samples_per_pixel(name):
    """More than a wave of samples per pixel (two trips, the second partly filled; every lane keeps a list of its own -- in LDS, and
    in global memory for p-K57 and p-K100): the mean of 70 samples against the mean of the 70 restated ones, each with its cloud's
    widened range; one family per scene and kind.  b-lens: the lanes' rays have origins of their own, the beams come through
    beam_walk_batch."""
    w, h, n = 5, 5, 70
    case = pc.family(name)
    r = base._build(case, width=w, height=h)
    got = base._frame(r, w, h, 0, n)
    v, lo, hi = pc.restated(name).mean(w, h, n)
    width = np.maximum(hi - lo, 1e-300)
    excess = np.maximum(np.maximum(lo - got, got - hi), 0.0) / width
    print(f"{name}: 70 samples, {w}x{h}: largest distance from the range / its width {excess.max():.3g}; relative width of the range "
          f"{np.nanmax(width / np.maximum(np.abs(v), 1e-300)):.3g}")
    assert np.all(np.isfinite(got)) and np.all(got >= lo) and np.all(got <= hi)
    assert np.abs(v).max() > 0


def _fallbacks(name, samples):
    """Trips of the camera pass whose rays formed no packet and walked the beams through beam_walk_batch (counters build, [20])."""
    from rpt_amd import _lib
    case = pc.family(name)
    r = base._build(case, options={"counters": 1})
    base._frame(r, 24, 24, 0, samples)
    out = (C.c_uint64 * 56)()
    _lib.check(_lib.load().rpt_debug_section_counters(r.scene._handle, out))
    print(name, samples, "samples:", int(out[12]), "trips through beam_walk_batch")
    return int(out[12])


def test_the_thin_lens_reaches_the_batch_walk():
    """Four samples per pixel through the lens: every trip's lanes start at different points, no trip forms a packet.  A pinhole's
    always do, and so does a single live lane."""
    assert _fallbacks("b-lens", 4) > 0
    assert _fallbacks("b-lens", 1) == 0
    assert _fallbacks("b-control", 4) == 0
