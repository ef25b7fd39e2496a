"""The photon shooting pass chain by chain, in both modes: photon_shoot_kernel<MEDIUM, BVH, WRITE> (photon.hip) and
photon_shoot_f64_kernel<MEDIUM, WRITE, LDSTAB> (kernels_f64.hip) with the count pass, the prefix sums and the write pass of shoot_range,
against the oracle's chains of the same photons.  The rule, the error model and what a cloud is: tests/photon_chain_ref.py; the scenes:
tests/photon_chain_cases.py; tests/test_photon_chain_host.py checks on the oracle alone what this module takes from them.  The library's
per-photon record counts come from rpt_debug_photon_chain_counts (scene option "photon_keep_counts").  fp32 chains are read after
rpt_photon_shoot (the raw records), reference-epsilon chains after rpt_photon_map_build (rpt_photon_map_download in shooting order and
rpt_debug_photon_positions64).  Every test prints its figures before it asserts (pytest -s shows them).

Measured on an MI355X at the first run (the table is in DESIGN.md, "Photon shooting, chain by chain"): every case passed; in fp32 the
largest error / bound is 1.3e-3 for a position (mesh), 0.19 for a direction (a volume record of the fog, after a medium scatter's 7 u)
and 0.26 for a power (the rounding of the stored value against 2 u at a chain's first record); in the reference-epsilon mode the fp64
surface positions reach 5.5e-5 of their bound and everything stored as a float reaches 0.92 to 0.999 of a bound whose largest term is
that rounding.  No photon of any family had other record counts than the oracle's own chain."""
import functools

import numpy as np
import pytest

from rpt_amd import Camera, Renderer, RptError
from tests import photon_chain_cases as cases
from tests import photon_chain_ref as pcr

pytestmark = pytest.mark.gpu


def _records(r, which):
    """The raw records of the last photon_shoot -> (n, 12) float32: pos_r, dir, pow."""
    import torch
    from rpt_amd.dist import _view
    ptr, n = r.photon_records(which)
    return _view(ptr, n, torch.device("cuda", r.device_)).cpu().numpy().copy().view(np.float32).reshape(n, 12)


def _shoot(family, mode, kind, cap=0, shard=None, keep=1):
    """-> dict: cnt_s, cnt_v, surface (n, 10) fp64 (position, direction or beam start, power, radius slot), volume, stats."""
    a = cases.shoot_args(family, kind)
    sc = cases.scene(family)
    sc.set_option("photon_keep_counts", keep)
    sc.set_option("max_blocks", cap)
    if mode == "fp64":
        sc.set_option("epsilon_policy", 1)
    r = Renderer(sc, Camera()).watts(a["watts"]).seed(cases.SEED)
    rank, count = shard if shard else (a["shard_rank"], a["shard_count"])
    n = a["n"] if not shard else 1
    if mode == "fp32":
        totals = r.photon_shoot(a["photon_count"], kind, rank, count)
        raw = [_records(r, w) for w in (0, 1)]
        out = [np.concatenate([x[:, 0:3], x[:, 4:7], x[:, 8:11], x[:, 3:4]], axis=1).astype(np.float64) for x in raw]
        pad = [np.concatenate([x[:, 7], x[:, 11]]) for x in raw]
        assert all(np.all(p == 0) for p in pad)                      # the unused lanes of a raw record
        stats = {"surface": totals[0], "volume": totals[1], "shoot_blocks": None}      # (the map's stats exist once it is built)
    else:
        stats = r.photon_map_build(a["photon_count"], kind)
        totals = (stats["surface"], stats["volume"])
        out = [r.photon_map_download(w).astype(np.float64) for w in (0, 1)]
        out[0][:, 0:3] = r.photon_positions64()
    res = {"surface": out[0], "volume": out[1], "totals": totals, "stats": stats, "renderer": r, "bvh_nodes": r.scene_stats()["bvh_nodes"]}
    if keep:
        res["cnt_s"], res["cnt_v"] = r.photon_chain_counts(n)
    return res


@functools.lru_cache(maxsize=None)
def _uncapped(family, mode, kind):
    res = _shoot(family, mode, kind)
    del res["renderer"]
    for k in ("surface", "volume", "cnt_s", "cnt_v"):
        res[k].setflags(write=False)
    return res


@pytest.mark.parametrize("family,mode,kind", cases.cases())
def test_shooting_pass_matches_oracle_chain_by_chain(family, mode, kind):
    """The rule of tests/photon_chain_ref.py on every photon of the family: counts, then every record inside its cloud's range widened
    by the bound; beam-beam volume records also carry radius 3."""
    ref = pcr.reference_for(family, mode, kind)
    got = _uncapped(family, mode, kind)
    assert got["totals"] == (len(got["surface"]), len(got["volume"]))
    if family == "mesh":
        assert got["bvh_nodes"] > 0                                   # the mesh has a tree of its own: the BVH instantiation
    fails, worst, info = pcr.check(ref, got["cnt_s"], got["cnt_v"], got["surface"], got["volume"])
    pcr.report(f"{family} {mode} kind {kind}", worst, info)
    ns, nv = ref.counts()
    print(f"    records: {len(got['surface'])} surface / {len(got['volume'])} volume, the oracle's chains {ns.sum()} / {nv.sum()}; "
          f"photons with other counts than the oracle's own chain: {int(((got['cnt_s'] != ns) | (got['cnt_v'] != nv)).sum())}")
    assert not fails, fails[:12]
    if kind == 2:
        assert len(got["volume"]) >= cases.MIN_BEAMS and np.all(got["volume"][:, 9] == 3.0)
    elif mode == "fp32":
        assert np.all(got["volume"][:, 9] == 0.0)
    assert np.all(got["surface"][:, 9] == 0.0)


@pytest.mark.parametrize("family,mode", [(f, m) for f, (modes, kinds) in cases.FAMILIES.items() for m in modes])
def test_capped_grids_shoot_the_same_bits(family, mode):
    """max_blocks = 3 and = 1 (4,096 photons are 16 blocks: every thread strides, or every wave takes many batches) against the
    uncapped launch: arrays and counts bit for bit."""
    kind = cases.FAMILIES[family][1][0]
    want = _uncapped(family, mode, kind)
    for cap in (3, 1):
        got = _shoot(family, mode, kind, cap=cap)
        if mode == "fp64":
            assert got["stats"]["shoot_blocks"] == cap and want["stats"]["shoot_blocks"] == 16
        for k in ("cnt_s", "cnt_v", "surface", "volume"):
            assert np.array_equal(got[k], want[k]), (cap, k)


@pytest.mark.parametrize("family,mode,kind", [("flat", "fp32", 1), ("fog", "fp32", 1), ("fog", "fp32", 2), ("fog", "fp64", 0), ("many", "fp64", 1)])
def test_counts_hook_adds_up_and_indexes_the_arrays(family, mode, kind):
    """sum(counts) == the stats, and exclusive_cumsum(counts)[i] is where photon i's records begin: in fp32, three photons shot
    alone (shard_count = photon_count, shard_rank = i) give the slices of the full arrays bit for bit."""
    got = _uncapped(family, mode, kind)
    assert got["cnt_s"].sum() == got["stats"]["surface"] == len(got["surface"])
    assert got["cnt_v"].sum() == got["stats"]["volume"] == len(got["volume"])
    if mode != "fp32":
        return
    a = cases.shoot_args(family, kind)
    os_, ov_ = pcr._excl(got["cnt_s"].astype(np.int64)), pcr._excl(got["cnt_v"].astype(np.int64))
    busy = np.flatnonzero((got["cnt_s"] > 0) & ((got["cnt_v"] > 0) | (got["cnt_v"].sum() == 0)))
    for i in (0, int(busy[len(busy) // 2]), a["n"] - 1):
        one = _shoot(family, mode, kind, shard=(i, a["photon_count"]))
        assert (one["cnt_s"][0], one["cnt_v"][0]) == (got["cnt_s"][i], got["cnt_v"][i]) == (len(one["surface"]), len(one["volume"]))
        assert np.array_equal(one["surface"], got["surface"][os_[i]:os_[i] + got["cnt_s"][i]])
        assert np.array_equal(one["volume"], got["volume"][ov_[i]:ov_[i] + got["cnt_v"][i]])


def test_counts_are_kept_on_request_only():
    """Without the option the hook has nothing (RPT_ERR_STATE) and the shooting pass stores the same records."""
    want = _uncapped("fog", "fp32", 1)
    got = _shoot("fog", "fp32", 1, keep=0)
    assert np.array_equal(got["surface"], want["surface"]) and np.array_equal(got["volume"], want["volume"])
    with pytest.raises(RptError):
        got["renderer"].photon_chain_counts(cases.N_PHOTONS)
    fresh = Renderer(cases.scene("flat").set_option("photon_keep_counts", 1), Camera())
    fresh.scene._commit(0)
    with pytest.raises(RptError):
        fresh.photon_chain_counts(1)                                  # nothing shot yet
