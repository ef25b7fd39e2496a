"""The photon-map restatement (tests/photon_ref.py) and its inputs (tests/photon_cases.py), pinned with the oracle alone: CPU only.

  * the restatement equals the oracle's camera pass over the same photon lists (`photon_map_from_photons(...).render`, one sample per
    pixel) to 1e-12 relative in every pixel of every family, and its radii equal the oracle's;
  * the reference alone meets the caps on undecided pixels: at most 5 % per family, at least 10 % in the family made to be undecided;
  * each family is what it claims to be;
  * the same for the point x point (kind 0) and beam x beam (kind 2) maps: every p-* and b-* family but those whose beams do not have
    the oracle's radius 3 is pinned to the oracle (which proves the stream and the draw of the sampled distance); every p-* family in
    the dense fog has at least a quarter of its pixels in each branch."""
import numpy as np
import pytest

from tests import photon_cases as pc
from tests import photon_ref as pr


def _oracle_map(name):
    c = pc.deep_volume() if name == "v-deep" else pc.deep_volume(0) if name == "p-deep72" else pc.family(name)
    r = pc.restated(name)
    return r.osc.photon_map_from_photons(max(len(c.surface) + len(c.volume), 1), c.kind, 100.0, c.K, c.Kv, c.surface, c.volume, robust=1), c, r


def _rel(a, b):
    with np.errstate(invalid="ignore", divide="ignore"):
        d = np.abs(a - b) / np.maximum(np.abs(b).max(axis=1, keepdims=True), 1e-300)
    same = (np.isnan(a) & np.isnan(b)) | (np.isinf(a) & (a == b))
    return np.where(same, 0.0, d)


@pytest.mark.parametrize("name", pc.NAMES + ("v-deep",))
def test_restatement_equals_the_oracle_in_every_pixel(name):
    pm, c, r = _oracle_map(name)
    for w, h, s in c.frames:
        exp = pm.render(r.camera, w, h, 1, seed=0, sample_offset=s)
        got = pc.answers(name, w, h, s).value
        err = _rel(got, exp)
        lit = np.isfinite(exp).all(axis=1) & (np.abs(exp).max(axis=1) > 0)
        print(f"{name} {w}x{h} sample {s}: lit pixels {int(lit.sum())} of {len(exp)}, largest relative difference {np.nanmax(err):.2e}")
        assert not np.isnan(err).any() and err.max() <= 1e-12
        if name != "few-0":
            assert lit.mean() > 0.2


@pytest.mark.parametrize("name", sorted(pc.radii_sets()) + ["v-deep"])
def test_radii_equal_the_oracle(name):
    from oracle.pyoracle import OracleScene
    pos = pc.deep_volume().volume[:, :3] if name == "v-deep" else pc.radii_sets()[name]
    vol = np.zeros((len(pos), 10))
    vol[:, :3] = pos
    vol[:, 4] = 1.0
    pm = OracleScene(pc.scene("Am")[0]).photon_map_from_photons(len(pos), 1, 100.0, 8, 3, np.zeros((0, 10)), vol, robust=1)
    exp, got = pm.photons(1)[:, 9], pr.knn_radii(pos)
    assert np.array_equal(got == 0.0, exp == 0.0)
    nz = exp > 0
    assert np.all(np.abs(got[nz] - exp[nz]) <= 1e-12 * exp[nz])


@pytest.mark.parametrize("name", pc.NAMES)
def test_undecided_pixels_stay_within_their_caps(name):
    c = pc.family(name)
    for w, h, s in c.frames:
        a = pc.answers(name, w, h, s)
        share = float((~a.decided).mean())
        print(f"{name} {w}x{h} sample {s}: {100.0 * share:.2f} % undecided")
        if name in pc.UNDECIDED_ON_PURPOSE:
            assert share >= 0.10
        else:
            assert share <= 0.05


def _hit_points(name, w, h, s):
    r = pc.restated(name)
    o, d = r.rays(w, h, s)
    t, obj, _ = r.osc.intersect(o, d, robust=1)
    return (o + t[:, None] * d)[obj >= 0]


def test_dense_has_a_ball_with_more_candidates_than_the_wave_gather_holds():
    c = pc.family("dense")
    x = _hit_points("dense", 24, 24, 0)
    _, d2 = pr._nearest(c.surface[:, :3], x, c.K)
    r2 = d2.max(axis=1)
    inside = (((x[:, None, :] - c.surface[None, :, :3]) ** 2).sum(axis=2) <= r2[:, None]).sum(axis=1)
    near = np.sqrt(((x - pc.DENSE_AT) ** 2).sum(axis=1)) < 0.3
    # a pixel's first search radius is sqrt(2) times the previous pixel's: next to the disc that ball holds the whole disc
    wide = (((x[:, None, :] - c.surface[None, :, :3]) ** 2).sum(axis=2) <= 2.0 * r2[:, None]).sum(axis=1)
    print(f"dense: photons within the K-th distance up to {inside.max()}, within sqrt(2) of it up to {wide.max()}")
    assert near.any() and wide.max() > pc.COOP_CAP


def test_far_needs_more_than_seven_doublings():
    c = pc.family("far")
    x = _hit_points("far", 24, 24, 0)
    _, d2 = pr._nearest(c.surface[:, :3], x, c.K)
    r = np.sqrt(d2.max(axis=1))
    first = r.min()                                                    # the radius of a query inside the corner
    within = (np.sqrt(((x[:, None, :] - c.surface[None, :, :3]) ** 2).sum(axis=2)) <= 2.0 ** 7 * first).sum(axis=1)
    print(f"far: radii {first:.4f} .. {r.max():.3f}; fewest photons within 2^7 x the smallest {within.min()}")
    assert within.min() < c.K


def test_tree_depths():
    """The emulated k-nearest tree is deeper than the walk's stack for the deep comb alone."""
    assert pc.tree_depth(pc.comb(1)) == 56 and pc.tree_depth(pc.comb(16)) == 64 and pc.tree_depth(pc.comb(512)) == 69
    assert pc.tree_depth(pc.family("deep").surface[:, :3]) == 72 > pc.KNN_STACK
    assert pc.tree_depth(pc.deep_volume().volume[:, :3]) == 72
    rng = np.random.default_rng(0)
    assert pc.tree_depth(rng.uniform(0.0, 1.0, (20000, 3))) == 14
    for name in pc.NAMES:
        if name == "deep":
            continue
        c = pc.family(name)
        for pos in (c.surface[:, :3], c.volume[:, :3]):
            assert pc.tree_depth(pos) < pc.KNN_STACK, name
    for name, pos in pc.radii_sets().items():
        assert pc.tree_depth(pos) <= pc.KNN_STACK, name


def test_block_family_overfills_a_strip_list():
    """More volume photons than kCandCap reach into the frustum of pixel rows 12 and 13 of the block (8..15, 8..15)."""
    c = pc.family("v-block")
    r = pc.restated("v-block")
    o, d = r.rays(24, 24, 0)
    pix = np.array([y * 24 + x for y in pc.BLOCK_ROWS for x in range(8, 16)])
    otc = c.volume[None, :, :3] - o[pix][:, None, :]
    disk = (otc * d[pix][:, None, :]).sum(axis=2)
    dist2 = (otc ** 2).sum(axis=2) - disk ** 2
    reached = ((disk > 0) & (dist2 < r.radius[None, :] ** 2)).any(axis=0)
    assert reached.sum() > pc.CAND_CAP


def test_records_hold_the_lists_bit_for_bit():
    c = pc.family("visibility")
    rec = pc.records(c.surface)
    assert rec.dtype == np.float32 and rec.shape == (len(c.surface), 12) and rec.nbytes == 48 * len(c.surface)
    assert np.array_equal(rec[:, [0, 1, 2, 4, 5, 6, 8, 9, 10]].astype(np.float64), c.surface[:, :9])


def test_the_rule_accepts_its_own_reference_and_rejects_a_photon_too_many():
    a = pc.answers("control", 24, 24, 0)
    failed, ratio = pr.check(a, a.value)
    assert not failed.any() and ratio.max() == 0.0
    lit = np.abs(a.value).max(axis=1) > 0
    off = a.value * np.where(lit, 1.0 + 1.0 / pc.K0, 1.0)[:, None]      # about one photon term too many in a sum of K
    failed, _ = pr.check(a, off)
    assert failed[lit & a.decided].all()


# ------------------------------------------------------------------ point x point and beam x beam maps
PINNED = tuple(n for n in pc.POINT_NAMES + pc.BEAM_NAMES if n not in pc.BEAM_NOT_PINNED) + ("p-deep72",)


@pytest.mark.parametrize("name", PINNED)
def test_restatement_of_the_other_kinds_equals_the_oracle_in_every_pixel(name):
    """Kind 0 and kind 2 against `photon_map_from_photons(kind, robust=1).render`, one sample per pixel: 1e-12 relative, non-finite
    values of the same kind."""
    pm, c, r = _oracle_map(name)
    assert c.kind in (0, 2) and (c.kind == 0 or np.all(c.volume[:, 9] == pc.ORACLE_BEAM_RADIUS))
    for w, h, s in c.frames:
        exp = pm.render(r.camera, w, h, 1, seed=0, sample_offset=s)
        got = pc.answers(name, w, h, s).value
        err = _rel(got, exp)
        odd = ~np.isfinite(exp).all(axis=1)
        print(f"{name} {w}x{h} sample {s}: {int(odd.sum())} non-finite pixels of {len(exp)}, largest relative difference {np.nanmax(err):.2e}")
        assert not np.isnan(err).any() and err.max() <= 1e-12


@pytest.mark.parametrize("name", pc.POINT_NAMES + pc.BEAM_NAMES)
def test_undecided_pixels_of_the_other_kinds_stay_within_their_caps(name):
    c = pc.family(name)
    for w, h, s in c.frames:
        a = pc.answers(name, w, h, s)
        share = float((~a.decided).mean())
        print(f"{name} {w}x{h} sample {s}: {100.0 * share:.2f} % undecided")
        if name in pc.UNDECIDED_ON_PURPOSE:
            assert share >= 0.10
        else:
            assert share <= 0.05


@pytest.mark.parametrize("name", pc.POINT_NAMES)
def test_point_families_reach_both_branches(name):
    """At least a quarter of the pixels draw a distance before the first hit, at least a quarter beyond it."""
    c = pc.family(name)
    r = pc.restated(name)
    for w, h, s in c.frames:
        o, d = r.rays(w, h, s)
        dist, _ = r.distances(w, h, s)
        t, obj, _ = r.osc.intersect(o, d, robust=1)
        vol = (obj < 0) | (dist < t)
        print(f"{name} {w}x{h} sample {s}: {100.0 * vol.mean():.1f} % of the pixels in the volume branch")
        assert 0.25 <= vol.mean() <= 0.75


@pytest.mark.parametrize("name", ["b-lens", "p-K57"])
def test_seventy_sample_means_equal_the_oracle(name):
    """The 5 x 5 mean of 70 samples that the GPU test uses, against the oracle's own 70-sample render: for b-lens every sample has
    its own origin on the lens."""
    pm, c, r = _oracle_map(name)
    exp = pm.render(r.camera, 5, 5, 70, seed=0)
    got, lo, hi = r.mean(5, 5, 70)
    err = _rel(got, exp)
    print(f"{name}: 70 samples, 5x5: largest relative difference {err.max():.2e}")
    assert err.max() <= 1e-12 and np.all(lo <= got) and np.all(got <= hi)
    if name == "b-lens":
        o, _ = r.rays(5, 5, 0)
        o1, _ = r.rays(5, 5, 1)
        assert np.abs(o - o1).max() > 1e-3


def test_beam_records_hold_the_lists_bit_for_bit():
    c = pc.family("b-thin")
    rec = c.volume_records()
    assert rec.dtype == np.float32 and rec.shape == (len(c.volume), 12)
    assert np.array_equal(rec[:, [0, 1, 2, 4, 5, 6, 8, 9, 10, 3]].astype(np.float64), c.volume)
    assert np.all(rec[:, [7, 11]] == 0)


def test_the_families_of_the_other_kinds_are_what_they_claim():
    """b-ends: beam_t of the made beams is at 0 / at the length on their own pixel's ray; b-tangent: dist at the radius; b-behind: the
    far beams' boxes lie behind the eye; b-len0 / b-eye: the degenerate records; kind-0 trees are within the walk's stack."""
    o, d, _ = pc._pixel_rays()
    ends = pc.family("b-ends").volume[:16]
    tang = pc.family("b-tangent").volume[:12]

    for k, b in enumerate(ends):
        g = np.array([pc._bb_point(o[i], d[i], b[3:6], b[0:3]) for i in range(len(o))])
        ln = np.linalg.norm(b[0:3] - b[3:6])
        edge = np.abs(g[:, 1] - (0.0 if k < 8 else ln)) + g[:, 2]
        assert edge.min() < 1e-5
    for b in tang:
        g = np.array([pc._bb_point(o[i], d[i], b[3:6], b[0:3]) for i in range(len(o))])
        assert np.abs(g[:, 2] - b[9]).min() < 1e-5
    far = pc.family("b-behind").volume[40:80]
    assert np.all(np.minimum(far[:, 2], far[:, 5]) - 3.0 > pc.EYE[2])
    z = pc.family("b-len0").volume[0]
    assert np.array_equal(z[0:3], z[3:6])
    e = pc.family("b-eye").volume[0]
    assert np.all(np.cross(e[3:6] - pc.EYE, e[0:3] - e[3:6]) == 0.0)
    for name in pc.POINT_NAMES:
        assert pc.tree_depth(pc.family(name).volume[:, :3]) <= pc.KNN_STACK, name
    assert pc.tree_depth(pc.family("p-deep16").volume[:, :3]) == pc.KNN_STACK
