"""The inputs of test_gpu_path_cloud.py, pinned with the oracle alone (tests/path_cloud.py): the scenes allow the caps, they exercise
what they claim to, and the rule with its caps rejects wrong answers.  No GPU.

Measured here with the camera's own answer left out of its cloud, unmatched of held samples (fp32: all 9,216; fp64 in a medium: the
decided ones) -- fp32: 0 on every scene but the clamp scene in fog, 1 (0.011 %).  fp64: materials 0, in fog 2 of 6,302 (0.03 %), in the
glowing fog 2 of 5,940; clamp 0, in fog 2 of 5,901, with the torus 0; group light 0; C2 1 of 9,216; C3 0 of 9,178.  Decided shares in fp64 in a
medium: 68 %, 64 %, 64 % and, in C3's thin fog, 99.6 %.  The worst stratum: 0.27 % (fp32, clamp scene in fog, depth 7) and 0.34 % (fp64, glowing
fog, depth 5).
The clamp scene: 807 of 9,216 samples clamped (797 with the torus), 81 in exactly one channel, 329 (333) at a level deeper than the first
bounce, 230 (233) at two levels of one path.

What the scenes cannot show, and where it is shown instead: in the materials scene's fog (extinction 0.05) a miss beyond the background
distance 400 has probability e^-20, so "the environment only beyond 400" is exercised there from the near side only (every miss is followed
by a medium event) and from the far side by C3, whose thin fog leaves 4,604 of 9,216 paths ending in such a miss, and by the clamp scene
in a fog of extinction 0.004 (2,905 far misses, 5,349 samples with a medium event; fp32 2 unmatched, fp64 0 of 7,739 decided).  With a medium a path
ends by roulette, not by max_bounces, so "every depth ends paths" is asked up to depth 4 there.  Ambient lights have no shadow test, and
the materials scene's point and directional light never pass the reference's (test_gpu_parity.py says so of the first): "every light
passes" is asked of the object lights."""
import numpy as np
import pytest

from rpt_amd import Light
from tests import path_cloud as pc

MODES = ["fp32", "fp64"]
CASES = [(name, mode) for mode in MODES for name in pc.SCENES]
CLAMP_SCENES = [name for name, s in pc.SCENES.items() if s[2]]
FAR_MISS_SCENES = ("clamp thin fog", "C3")          # thin fog: a distance sample can lie beyond the background distance


@pytest.mark.parametrize("name,mode", CASES)
def test_the_inputs_allow_a_quarter_of_every_cap(name, mode):
    cl = pc.prepared(name, mode)
    assert len(cl) == len(pc.OFFSETS) * pc.SIZE ** 2 == 9216 and cl.first.shape == (17, 9216, 3) and cl.more.shape == (len(cl.again), 48, 3)
    assert cl.medium == bool(pc.build(name)[0].media)
    assert np.all(np.isfinite(cl.first)) and np.all(cl.first >= 0.0) and np.all(np.isfinite(cl.more)) and np.all(cl.more >= 0.0)
    rep = pc.check(cl, cl.nominal, leave_out_nominal=True)
    fig, bad = pc.caps(cl, rep, fraction=0.25)
    assert not bad, bad
    if mode == "fp64" and cl.medium:
        assert fig["decided"] >= 0.6 * len(cl)
    # the camera's own answer in its own cloud: matched everywhere, at distance 0
    rep = pc.check(cl, cl.nominal)
    assert not rep.unmatched.any() and rep.err.max() == 0.0
    # the second pass ran for every sample that is not decided
    assert np.all(np.isin(np.flatnonzero(~cl.decided), cl.again))
    # the Phong exponents stay at 50 or below (a direction error of 1e-6 under cos^n)
    assert all(o.material_.shininess <= 50.0 for o in pc.build(name)[0].objects)


@pytest.mark.parametrize("name", list(pc.SCENES))
def test_the_record_restates_the_radiance_and_both_policies_walk_the_same_kinds_of_path(name):
    for mode in MODES:
        cl = pc.prepared(name, mode)
        again = pc.restate(cl, "oracle")
        assert np.all(np.abs(again - cl.nominal) <= 1e-12 * cl.scale[:, None])
        rec = cl.rec
        assert np.all(rec["levels"] == rec["depth"] + 1) and np.all(rec["end"] <= 2)
        assert np.array_equal((rec["flags"] & 4) != 0, rec["depth"] >= 16)
        if not cl.medium:
            assert rec["depth"].max() == pc.build(name)[2] and not (rec["flags"] & 3).any()
        if not cl.clamp_works:
            assert not cl.clamped.any()            # (with a medium the reference does not clamp)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", CLAMP_SCENES)
def test_the_clamp_works_in_the_clamp_scenes(name, mode):
    cl = pc.prepared(name, mode)
    m = pc.clamp_masks(cl.rec)
    channels = np.array([bin(v).count("1") for v in range(8)])[m]
    assert cl.clamped.sum() >= 300
    assert (channels.sum(axis=1) == 1).sum() >= 50            # exactly one channel
    assert (m[:, 1:] != 0).any(axis=1).sum() >= 30            # deeper than the first bounce
    assert ((m != 0).sum(axis=1) >= 2).sum() >= 10            # at two levels of one path
    # the same scene in fog: the reference does not clamp, and more than a few samples lie above what a clamp would leave
    fog = pc.prepared("clamp fog", mode)
    assert not fog.clamped.any() and (np.abs(pc.restate(fog, "always") - fog.nominal).max(axis=1) > 1e-2 * fog.scale).sum() >= 100


@pytest.mark.parametrize("name,mode", CASES)
def test_depths_media_and_lights_are_exercised(name, mode):
    cl = pc.prepared(name, mode)
    sc, cam, mb = pc.build(name)
    ends = np.bincount(cl.rec["depth"], minlength=mb + 1)
    assert np.all(ends[:(min(mb, 4) if cl.medium else mb) + 1] >= 30), ends
    if cl.medium:
        assert ((cl.rec["flags"] & 1) != 0).sum() >= 200
        if name in FAR_MISS_SCENES:
            assert ((cl.rec["flags"] & 2) != 0).sum() >= 100
        else:               # extinction 0.04-0.05: every miss is followed by a medium event
            assert not (cl.rec["flags"] & 2).any() and not (cl.rec["end"] == 0).any()
    tested = [i for i, l in enumerate(sc.lights) if l.kind == Light.OBJECT]
    assert tested and len(cl.light_pass) == len(sc.lights)
    assert all(cl.light_pass[i] >= 50 for i in tested), cl.light_pass


def _fails(cl, got, title):
    rep = pc.check(cl, got)
    return rep, pc.caps(cl, rep, title=f"{cl.name}, {title}")[1]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["materials", "materials fog", "clamp", "clamp torus", "C2"])
def test_the_rule_rejects_what_is_wrong(name, mode):
    cl = pc.prepared(name, mode)
    b = pc.MODES[mode]["b"]
    nominal = cl.nominal
    inside = pc.check(cl, nominal, leave_out_nominal=True)
    firm = cl.decided & ~inside.unmatched & (nominal.max(axis=1) >= pc.SCALE_FLOOR)     # a value of its own, held by 16 other answers
    assert firm.sum() >= 4000
    # scaled by 1 +- 5 b: every firm sample is rejected; by 1 + b / 4: none
    for s in (1.0 + 5.0 * b, 1.0 - 5.0 * b):
        rep, bad = _fails(cl, nominal * s, f"scaled by {s!r}")
        assert np.all(rep.unmatched[firm]) and bad
    assert not pc.check(cl, nominal * (1.0 + 0.25 * b)).unmatched.any()
    # the neighbouring stream: sample offset + 1
    n_pix = pc.SIZE ** 2
    other = np.roll(nominal, -n_pix, axis=0)
    differs = firm & (np.abs(other - nominal).max(axis=1) > 3.0 * b * cl.scale)
    rep, bad = _fails(cl, other, "the neighbouring stream")
    assert differs.sum() >= 3000 and np.all(rep.unmatched[differs]) and bad
    # NaN, infinite, negative: one sample is enough
    for v in (np.nan, np.inf, -1e-6):
        got = nominal.copy()
        got[1234, 1] = v
        rep, bad = _fails(cl, got, f"one sample {v}")
        assert rep.bad[1234] and rep.unmatched[1234] and rep.bad.sum() == 1 and bad


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", CLAMP_SCENES)
def test_the_rule_rejects_a_wrong_clamp(name, mode):
    cl = pc.prepared(name, mode)
    b = pc.MODES[mode]["b"]
    inside = pc.check(cl, cl.nominal, leave_out_nominal=True)
    firm = cl.decided & ~inside.unmatched
    m = pc.clamp_masks(cl.rec)
    # no clamp at all: only clamped samples move, and nearly all of them
    got = pc.restate(cl, "none")
    moved = np.abs(got - cl.nominal).max(axis=1) > 3.0 * b * cl.scale
    rep, bad = _fails(cl, got, "no clamp")
    assert not moved[~cl.clamped].any() and moved.sum() >= 0.9 * cl.clamped.sum()
    assert np.all(rep.unmatched[moved & firm]) and any("clamped samples" in line for line in bad)
    # the clamp at 100 for 100 Q: moves paths clamped below the first bounce, among them some whose throughput there is below 1
    got = pc.restate(cl, "flat")
    moved = np.abs(got - cl.nominal).max(axis=1) > 3.0 * b * cl.scale
    deeper = (m[:, 1:] != 0).any(axis=1)
    rep, bad = _fails(cl, got, "clamp at 100 for 100 Q")
    assert not moved[~deeper].any() and moved.sum() >= 100
    assert (moved & (got > cl.nominal + 3.0 * b * cl.scale[:, None]).any(axis=1)).sum() >= 30      # Q < 1: the loose bound lets more through
    assert np.all(rep.unmatched[moved & firm]) and any("clamped samples" in line for line in bad)
    # a clamp in fog, where the reference has none
    fog = pc.prepared("clamp fog", mode)
    got = pc.restate(fog, "always")
    moved = np.abs(got - fog.nominal).max(axis=1) > 3.0 * b * fog.scale
    rep, bad = _fails(fog, got, "a clamp in fog")
    assert moved.sum() >= 100 and bad
