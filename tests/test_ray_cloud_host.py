"""The inputs of test_gpu_structured_rays.py, pinned with the oracle alone (tests/ray_cloud.py): the GPU tests cannot pass by leaving
rays undecided, and the rule they apply rejects what it should.  No GPU.

Undecided shares measured here (17-answer clouds, the amplitudes of ray_cloud.MODES), fp32 / fp64, in per cent: axis-parallel lattices
0.04 / 0.03, one zero component 0.4 / 0.4, torus centroids 0.8 / 0.4, cones other than x 1: 0 / 0, surface origins with |cos| >= 0.2:
2.2 / 1.9, random 0.2 / 0.2; torus vertices 32 / 20, box planes 37 / 37, box edges 82 / 82, cone x 1: 100 / 100, room edges 94 / 94; all
rays 5.3 / 4.9 (the rays just in front of surfaces, whose t the cloud spreads by more than b_t, are most of that).  The torus's edge
midpoints are 11.8 / 6.7 per cent undecided: its vertex normals are smooth, so object, t and normal
are continuous across an edge that faces the ray, and such a ray is decided with good reason; only edges on a silhouette are not.  "The
edges" that must be undecided for at least a tenth are therefore the box's twelve; of the torus's only some are asked for."""
import numpy as np
import pytest

from tests import ray_cloud as rc

MODES = ["fp32", "fp64"]


def _share(cl, family, names, prefix):
    sel = np.array([n.startswith(prefix) for n in names])[family]
    assert sel.sum() > 0, prefix
    return 1.0 - cl.decided[sel].mean()


@pytest.mark.parametrize("mode", MODES)
def test_every_ray_is_a_valid_ray_of_one_family(mode):
    p = rc.prepared(mode)
    o, d = p["o"], p["d"]
    assert 30000 <= len(o) <= 50000
    assert np.all(np.isfinite(o)) and np.all(np.isfinite(d))
    assert np.all(np.abs(np.linalg.norm(d, axis=1) - 1.0) < (1e-6 if mode == "fp32" else 1e-14))
    assert np.all(np.abs(o) < 5.001)                                      # inside the room
    if mode == "fp32":
        assert np.array_equal(o, o.astype(np.float32).astype(np.float64)) and np.array_equal(d, d.astype(np.float32).astype(np.float64))
    member = np.zeros(len(o), dtype=int)
    for g in rc.GROUPS:
        member += np.array([n.startswith(g) for n in p["names"]])[p["family"]]
    assert np.all(member == 1)
    # both signs of zero are there, and the one-zero families hold exactly one zero
    axis = np.array([n.startswith("axis") for n in p["names"]])[p["family"]]
    zeros = d[axis] == 0.0
    assert np.all(zeros.sum(axis=1) == 2)
    assert np.signbit(d[axis][zeros]).sum() == zeros.sum() // 2
    one = np.array([n.startswith("one zero") for n in p["names"]])[p["family"]]
    assert np.all((d[one] == 0.0).sum(axis=1) == 1)


@pytest.mark.parametrize("mode", MODES)
def test_interior_families_are_decided_and_boundary_families_are_not(mode):
    p = rc.prepared(mode)
    cl, family, names = p["cloud"], p["family"], p["names"]
    rc.print_table(f"{mode}: the oracle alone", rc.table(cl, family, names, groups=rc.GROUPS))
    for g in rc.INTERIOR:
        assert _share(cl, family, names, g) <= 0.05, g
    assert 1.0 - cl.decided.mean() <= 0.10
    for g in rc.BOUNDARY:
        assert _share(cl, family, names, g) >= 0.10, g
    assert _share(cl, family, names, "torus edges") > 0.03
    # the second pass ran for every ray whose first 17 answers name different objects, and for no other
    differ = (cl.obj != cl.obj[:, :1]).any(axis=1)
    assert np.array_equal(np.flatnonzero(differ), cl.again) and cl.obj2.shape == (len(cl.again), 17 + 26 + 26 + 32 + 2 * rc.N_OBJECTS_BISECTED * rc.N_BISECTIONS)
    assert 100 < len(cl.again) and not cl.decided[cl.again].any()


@pytest.mark.parametrize("mode", MODES)
def test_every_object_and_the_miss_are_decided_answers(mode):
    cl = rc.prepared(mode)["cloud"]
    first = cl.obj[:, 0]
    for i, name in enumerate(rc.OBJECTS):
        assert (cl.decided & (first == i)).sum() >= 100, name
    assert (cl.decided & (first < 0)).sum() >= 1000
    assert np.all(np.isposinf(cl.t[first < 0, 0]))


@pytest.mark.parametrize("variant", ["lattice", "scan"])
def test_the_other_scenes_keep_the_shares(variant):
    """The 64 small spheres are hit, and neither they nor the 32-triangle torus change the picture."""
    p = rc.prepared("fp32", variant)
    cl, family, names = p["cloud"], p["family"], p["names"]
    for g in ("axis", "one zero", "surface steep", "random"):
        assert _share(cl, family, names, g) <= 0.05, g
    assert 1.0 - cl.decided.mean() <= 0.10
    first = cl.obj[:, 0]
    for i, name in enumerate(rc.OBJECTS):
        assert (cl.decided & (first == i)).sum() >= 100, name
    if variant == "lattice":
        assert (cl.decided & (first >= 10)).sum() >= 100 and len(np.unique(first[first >= 10])) >= 16


@pytest.mark.parametrize("mode", MODES)
def test_the_rule_accepts_the_oracle_and_rejects_what_is_wrong(mode, capsys):
    p = rc.prepared(mode)
    cl, family, names = p["cloud"], p["family"], p["names"]
    cfg = rc.MODES[mode]
    obj, t, nrm = cl.obj[:, 0].copy(), cl.t[:, 0].copy(), cl.nrm[:, 0].copy()
    nrm[obj < 0] = 0.0
    rep = rc.check(cl, obj, t, nrm, mode, family, names)
    assert not rep.failed.any()
    assert np.nanmax(rep.t_err) == 0.0 and np.nanmax(rep.n_err) == 0.0
    hits = cl.decided & (obj >= 0)
    assert hits.sum() > 30000
    # the neighbouring object
    rep = rc.check(cl, np.where(obj >= 0, (obj + 1) % len(rc.OBJECTS), obj), t, nrm, mode, family, names, layout="wrong object", show=1)
    assert np.all(rep.failed[hits])
    assert "wrong object" in capsys.readouterr().out
    # a hit where everything misses, a miss where everything hits, a miss with a finite t
    rep = rc.check(cl, np.where(obj < 0, 0, -1), np.where(obj < 0, 1.0, np.inf), nrm, mode, show=0)
    assert np.all(rep.failed[cl.decided])
    rep = rc.check(cl, obj, np.where(obj < 0, 1.0, t), nrm, mode, show=0)
    assert np.all(rep.failed[obj < 0]) and not rep.failed[obj >= 0].any()
    # t off by five bounds, either way
    for s in (1.0 + 5.0 * cfg["b_t"], 1.0 - 5.0 * cfg["b_t"]):
        rep = rc.check(cl, obj, t * s, nrm, mode, show=0)
        assert np.all(rep.failed[hits])
    rep = rc.check(cl, obj, t * (1.0 + 0.5 * cfg["b_t"]), nrm, mode, show=0)
    assert not rep.failed.any()
    # a flipped normal, and one off by two bounds in one component
    rep = rc.check(cl, obj, t, -nrm, mode, show=0)
    assert np.all(rep.failed[hits])
    rep = rc.check(cl, obj, t, nrm + np.array([0.0, 2.0 * cfg["b_n"], 0.0]), mode, show=0)
    assert np.all(rep.failed[hits])
    # NaN anywhere
    bad_t, bad_n = t.copy(), nrm.copy()
    bad_t[::7] = np.nan
    bad_n[::5, 1] = np.nan
    assert np.all(rc.check(cl, obj, bad_t, nrm, mode, show=0).failed[::7])
    assert np.all(rc.check(cl, obj, t, bad_n, mode, show=0).failed[::5])


def test_an_undecided_ray_accepts_each_of_its_answers_and_no_other():
    p = rc.prepared("fp32")
    cl = p["cloud"]
    room = np.array([n.startswith("room edges") for n in p["names"]])[p["family"]]
    obj, t, nrm = cl.obj[:, 0].copy(), cl.t[:, 0].copy(), cl.nrm[:, 0].copy()
    nrm[obj < 0] = 0.0
    tried = 0
    for row in np.flatnonzero(np.isin(cl.again, np.flatnonzero(room))):
        i = cl.again[row]
        seen = np.unique(cl.obj2[row])
        for ob in seen:
            k = np.flatnonzero(cl.obj2[row] == ob)[-1]
            obj[i], t[i], nrm[i] = ob, cl.t2[row, k], (cl.nrm2[row, k] if ob >= 0 else 0.0)
            assert not rc.check(cl, obj, t, nrm, "fp32", show=0).failed[i]
        absent = [ob for ob in range(len(rc.OBJECTS)) if ob not in seen][0]
        obj[i] = absent
        assert rc.check(cl, obj, t, nrm, "fp32", show=0).failed[i]
        obj[i], t[i], nrm[i] = cl.obj[i, 0], cl.t[i, 0], (cl.nrm[i, 0] if cl.obj[i, 0] >= 0 else 0.0)
        tried += 1
        if tried == 5:
            break
    assert tried == 5
