"""Photon maps built from hand-made records (rpt_photon_map_from_records), estimate by estimate, through the C ABI.

With hand-made photons a one-sample camera pass is a deterministic function of the camera ray: every pixel of every family of
tests/photon_cases.py is compared with the fp64 brute-force restatement of tests/photon_ref.py under that module's rule (the cloud
around the query, decided and undecided pixels, the stated fp32 bound) -- under the default settings and under each setting that takes
another path through photon.hip, every one against the reference itself.  The 10-NN radii of the beam x point map are compared with
the brute-force values at 1e-5 relative (exact zeros stay exact).  A tree deeper than the k-nearest walk's stack yields the right radii
or a refusal that names the depth, never a wrong radius.

What these families found is in DESIGN.md ("Photon maps from hand-made records"): wrong radii on a deep tree, NaN pixels from a photon
of radius 0, and every photon at the K-th distance summed by the wave-level gather are fixed.  One defect is kept as a strict expected
failure with its figures:
  * v-camera -- both beam forms that share the eye as origin replace exp(-sigma_t s) by exp(-sigma_t |c|) (1 + sigma_t (|c| - s)); for
    a sphere that holds the camera |c| - s is not small: 102 of 576 pixels 1e-4 below the reference, 20.6 times the stated bound."""
import ctypes as C

import numpy as np
import pytest

from rpt_amd import Renderer, RptError
from tests import photon_cases as pc
from tests import photon_ref as pr

pytestmark = pytest.mark.gpu

SETTINGS = {
    "default": {},
    "coop-off": {"photon_coop_gather": 0},
    "lists-off": {"photon_block_lists": 0},
    "parts-1": {"photon_parts": 1},
    "parts-8": {"photon_parts": 8},
    "blocks-3": {"max_blocks": 3},
}
COUNTERS = {"terms without a scan": 1, "overfull walks": 4, "lanes searching one by one": 11}   # tools/photon_gather_counters.py
# (family, setting) -> reason; see the module docstring
_EXP = ("the beam estimate's first-order exp(sigma_t (|c| - s)) next to a sphere that holds the camera: 102 of 576 pixels 1e-4 relative "
        "below the reference (error / bound 20.6), under every setting")
XFAIL = {("v-camera", s): _EXP for s in SETTINGS}


def _upload(ph, rec=None):
    import torch
    rec = pc.records(ph) if rec is None else rec
    if len(rec) == 0:
        return None, 0
    t = torch.from_numpy(rec).to(torch.device("cuda", 0)).contiguous()
    return t, t.data_ptr()


def _build(case, kind=None, options=None, width=24, height=24):
    """A renderer over a fresh scene with the case's maps built from its records (kind: the case's own unless given)."""
    import torch
    sc, cam = case.scene()
    for k, v in (options or {}).items():
        sc.set_option(k, v)
    kind = case.kind if kind is None else kind
    r = Renderer(sc, cam).width(width).height(height).gather_size(case.K).gather_size_volume(case.Kv).seed(0)
    ts, ps = _upload(case.surface)
    tv, pv = _upload(case.volume, case.volume_records())
    torch.cuda.synchronize()
    st = r.photon_map_from_records(max(len(case.surface) + len(case.volume), 1), kind, ps, len(case.surface), pv, len(case.volume))
    assert (st["surface"], st["volume"]) == (len(case.surface), len(case.volume))
    del ts, tv
    return r


def _frame(r, w, h, sample, n=1):
    r.width(w).height(h)
    r._sample_offset = sample
    return r.photon_sample_array(n)


def _apply_rule(name, setting, frames):
    case = pc.family(name)
    r = _build(case, options=SETTINGS[setting])
    bad = 0
    for w, h, s in frames:
        got = _frame(r, w, h, s)
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


@pytest.mark.parametrize("name,setting", _params(pc.NAMES, ["default"]))
def test_every_pixel_of_a_family_under_the_default_settings(name, setting):
    """Every frame of the family (24 x 24; 50 x 37 with clipped 8 x 8 blocks and another sample offset for the larger families)."""
    _apply_rule(name, setting, pc.family(name).frames)


@pytest.mark.parametrize("name,setting", _params(pc.NAMES, [s for s in SETTINGS if s != "default"]))
def test_every_pixel_of_a_family_under_each_setting(name, setting):
    """One search per lane, no block candidate lists, one and eight strips per pixel block, a grid of three blocks: each against the
    reference, not against the default."""
    _apply_rule(name, setting, pc.family(name).frames[:1])


@pytest.mark.parametrize("name", ["control", "room", "plane", "torus", "v-control", "v-room"])
def test_seventy_samples_per_pixel(name):
    """More than a wave of samples per pixel (two trips, the second partly filled), the guessed radius carried from pixel to pixel: the
    mean of 70 samples against the mean of the 70 restated ones, each with its cloud's widened range."""
    w, h, n = 5, 5, 70
    case = pc.family(name)
    r = _build(case, width=w, height=h)
    got = _frame(r, w, h, 0, n)
    v, lo, hi = pc.restated(name).mean(w, h, n)
    width = np.maximum(hi - lo, 1e-300)
    excess = np.maximum(np.maximum(lo - got, got - hi), 0.0) / width
    print(f"{name}: 70 samples, {w}x{h}: largest distance from the range / its width {excess.max():.3g}; relative width of the range "
          f"{np.nanmax(width / np.maximum(np.abs(v), 1e-300)):.3g}")
    assert np.all(np.isfinite(got)) and np.all(got >= lo) and np.all(got <= hi)
    assert np.abs(v).max() > 0


def _counters(name):
    from rpt_amd import _lib
    case = pc.family(name)
    r = _build(case, options={"counters": 1})
    for w, h, s in case.frames[:1]:
        _frame(r, w, h, s, 4)
    out = (C.c_uint64 * 56)()
    _lib.check(_lib.load().rpt_debug_section_counters(r.scene._handle, out))
    got = {k: int(out[i]) for k, i in COUNTERS.items()}
    print(name, got)
    return got


def test_counters_show_the_intended_paths():
    """The wave-level counters of the camera pass (counters build): the dense disc overfills the wave's candidate list and hands over
    to one search per lane; the far family searches lane by lane; in the room the shell's shortcut adds terms without a visibility
    scan, and a scene with a plane never does."""
    dense = _counters("dense")
    assert dense["overfull walks"] > 0 and dense["lanes searching one by one"] > 0
    assert _counters("far")["lanes searching one by one"] > 0
    assert _counters("room")["terms without a scan"] > 0
    assert _counters("plane")["terms without a scan"] == 0


def _radii_case(pos):
    vol = np.zeros((len(pos), 10))
    vol[:, :3] = pos
    vol[:, 4] = 1.0
    vol[:, 6:9] = 0.5
    return pc.Case("radii", "Am", 8, np.zeros((0, 10)), vol)


@pytest.mark.parametrize("name", sorted(pc.radii_sets()))
def test_radii_equal_the_brute_force_values(name):
    """knn_radius_kernel through photon_map_download(1): 1e-5 relative (the bound of test_c4_at_its_configured_one_million_photons);
    where the reference is exactly 0 (ten or more coincident photons) so is the device's.  comb-16 is the deepest tree the walk's
    stack holds (64 inner nodes on a path)."""
    pos = pc.radii_sets()[name]
    r = _build(_radii_case(pos))
    got = r.photon_map_download(1)
    assert np.array_equal(got[:, :3].astype(np.float64), pos)
    exp = pr.knn_radii(pos)
    zero = exp == 0.0
    rel = np.abs(got[~zero, 9] - exp[~zero]) / exp[~zero]
    print(f"{name}: {len(pos)} photons, {int(zero.sum())} radii exactly 0, largest relative error {rel.max() if len(rel) else 0.0:.2e}")
    assert np.all(got[zero, 9] == 0.0)
    assert np.all(rel <= 1e-5)


@pytest.mark.parametrize("kind", [1, 0])
def test_a_tree_deeper_than_the_walks_stack_is_right_or_refused(kind):
    """The deep comb as volume photons: 72 inner nodes on the deepest path, the walk's stack holds 64.  Kind 1 runs the radius kernel,
    kind 0 the point x point volume gather, both through knn_walk.  Either the map is refused with RPT_ERR_UNSUPPORTED and a message
    that names the tree depth, or the values are right -- every origin copy's radius is exactly 0, and every pixel of the camera pass
    obeys the rule against the restatement of its own kind (tests/test_gpu_photon_estimates.py holds the families of kind 0 and 2)."""
    case = pc.deep_volume(kind)
    try:
        r = _build(case)
    except RptError as e:
        msg = str(e)
        print(msg)
        assert "rpt error -4" in msg and "depth" in msg and str(pc.tree_depth(case.volume[:, :3])) in msg
        return
    if kind == 1:
        got = r.photon_map_download(1)
        exp = pr.knn_radii(case.volume[:, :3])
        zero = exp == 0.0
        assert zero.sum() == 4096 and np.all(got[zero, 9] == 0.0)
        assert np.all(np.abs(got[~zero, 9] - exp[~zero]) <= 1e-5 * exp[~zero])
    n_bad, _ = pr.report(case.name, pc.answers(case.name, 24, 24, 0), _frame(r, 24, 24, 0))
    assert n_bad == 0
