"""The chain-by-chain rule for the photon shooting pass (tests/photon_chain_ref.py) on the oracle alone: the hook reproduces the map
build, the families of tests/photon_chain_cases.py meet the conditions the rule needs before anything runs on a device, the rule
accepts the oracle's own chains and rejects chains that are subtly wrong.  No GPU."""
import numpy as np
import pytest

from oracle.pyoracle import OracleScene
from tests import photon_chain_cases as cases
from tests import photon_chain_ref as pcr
from tests.ray_cloud import MODES


@pytest.mark.parametrize("kind", [0, 1, 2])
@pytest.mark.parametrize("robust", [0, 1])
def test_chains_without_amplitude_are_the_map_build(kind, robust):
    """orc_photon_chains with amp = 0 against orc_photon_map_build: the same lists bit for bit, whole and as a slice."""
    osc = OracleScene(cases.scene("fog"))
    n, watts = 3000, 48000.0
    pm = osc.photon_map(n, kind, watts, 20, 3, seed=9, robust=robust)
    ch = osc.photon_chains(n, kind, watts, seed=9, robust=robust, n=n, verts=True)
    for which, name, cnt in ((0, "surface", "ns"), (1, "volume", "nv")):
        exp = pm.photons(which)[:, :9]
        assert len(exp) > (20 if kind == 2 and which == 1 else 1000)
        assert np.array_equal(exp, ch[name][:, :9]) and ch[cnt].sum() == len(exp)
    assert ch["nrows"].sum() == len(ch["rows"]) and np.all(ch["rows"][pcr._excl(ch["nrows"]), 0] == 3)
    assert (ch["rows"][:, 5] == 1).sum() == ch["ns"].sum() and (ch["rows"][:, 5] == 2).sum() == ch["nv"].sum()
    part = osc.photon_chains(n, kind, watts, seed=9, robust=robust, first=1000, n=500)
    os_, ov_ = pcr._excl(ch["ns"]), pcr._excl(ch["nv"])
    assert np.array_equal(part["surface"], ch["surface"][os_[1000]:os_[1500]]) and np.array_equal(part["volume"], ch["volume"][ov_[1000]:ov_[1500]])
    assert np.array_equal(part["sig"], ch["sig"][1000:1500])
    idx = np.array([7, 2999, 1234], dtype=np.uint64)
    pick = osc.photon_chains(n, kind, watts, seed=9, robust=robust, indices=idx)
    assert np.array_equal(pick["sig"], ch["sig"][idx.astype(int)]) and np.array_equal(pick["ns"], ch["ns"][idx.astype(int)])


def test_a_displaced_chain_keeps_its_streams():
    """amp > 0 moves the rays, not the draws: the records move by about the amplitude, and a member is a function of its seed."""
    osc = OracleScene(cases.scene("fog"))
    a = osc.photon_chains(4096, 1, 65536.0, seed=cases.SEED, robust=1, n=512)
    b = osc.photon_chains(4096, 1, 65536.0, seed=cases.SEED, robust=1, n=512, amp=2e-6, cloud_seed=3)
    c = osc.photon_chains(4096, 1, 65536.0, seed=cases.SEED, robust=1, n=512, amp=2e-6, cloud_seed=3)
    d = osc.photon_chains(4096, 1, 65536.0, seed=cases.SEED, robust=1, n=512, amp=2e-6, cloud_seed=4)
    assert np.array_equal(b["volume"], c["volume"]) and np.array_equal(b["sig"], c["sig"])
    same = a["sig"] == b["sig"]
    assert same.mean() > 0.9
    keep = np.repeat(same & (d["sig"] == a["sig"]), a["nv"])
    va, vb, vd = a["volume"][keep], b["volume"][np.repeat(same & (d["sig"] == a["sig"]), b["nv"])], d["volume"][np.repeat(same & (d["sig"] == a["sig"]), d["nv"])]
    step = np.abs(va[:, :3] - vb[:, :3]).max()
    assert 0 < step < 1e-3 and not np.array_equal(vb, vd)


@pytest.mark.parametrize("family,mode,kind", cases.cases())
def test_families_meet_the_conditions_of_the_rule(family, mode, kind):
    """Per family, on the oracle alone: at least 85 % (fp32 amplitude) or 95 % (fp64 amplitude) of the chains are decided, every kind of
    record the family is there to exercise is stored at least 1,000 times (kept beams: 300), and what the family is named for happens."""
    ref = pcr.reference_for(family, mode, kind)
    ns, nv = ref.counts()
    rows = ref.members[0]["rows"]
    share = ref.decided.mean()
    print(f"{family} {mode} kind {kind}: decided {share:.4f}, {ns.sum()} surface and {nv.sum()} volume records, longest chain {int((ns + nv).max())}")
    assert share >= (0.85 if mode == "fp32" else 0.95)
    need_s, need_v = cases.EXERCISES[family]
    assert ns.sum() >= need_s and nv.sum() >= (min(need_v, cases.MIN_BEAMS) if kind == 2 else need_v)
    assert len(ns) == cases.shoot_args(family, kind)["n"] and len(ns) % 256 == 0 and len(ns) >= 16 * 256
    for groups in ref.groups.values():
        assert sum(len(g["surface"]) for g in groups.values()) == pcr.N_FIRST + 1 + pcr.N_MORE
    surf = rows[rows[:, 0] == 2]
    if family == "objects":
        kinds = np.bincount(surf[:, 6].astype(int), minlength=4)
        assert np.all(kinds[1:] >= 80)                                          # Phong, mirror and glass vertices
        assert (surf[:, 2] == 2).sum() >= 10                                    # sample_f None: total internal reflection
        assert ((surf[:, 2] == 0) & (surf[:, 7] <= 0) & (surf[:, 5] == 1)).sum() >= 100    # a stored vertex with wi.n <= 0
    if family in ("fog", "glow", "glow low"):
        assert nv.sum() / len(nv) > (4.0 if kind != 2 else 0.0) and (rows[:, 2] == 3).sum() >= 1000
    if family.startswith("glow"):
        hi = rows[rows[:, 0] == 1, 1]
        assert (hi.sum() >= 1000 and (hi == 0).sum() >= 1000) if family == "glow" else hi.sum() == 0
    if family == "sphere light":
        em = rows[pcr._excl(ref.members[0]["nrows"])]
        assert (em[:, 10] < 0.1).sum() >= 4 and em[:, 9].min() < 1.0           # emitter normals next to the pole; sphere samples
    if family == "many":
        assert len(cases.scene(family).objects) > 32


@pytest.mark.parametrize("family,mode,kind", cases.cases())
def test_rule_accepts_the_oracle_rounded_to_fp32(family, mode, kind):
    ref = pcr.reference_for(family, mode, kind)
    fails, worst, info = pcr.check(ref, *pcr.as_device(ref.members[0], mode))
    pcr.report(f"{family} {mode} kind {kind} (the oracle's own chains as floats)", worst, info)
    assert not fails, fails[:10]
    # the chain is a member of its cloud: what is left is the rounding to float, half an ulp against bounds of 2 u and more (in the
    # reference-epsilon mode the rounding IS the bound's largest term, 2^-24 |value|)
    assert max(v[0] for v in worst.values()) < (0.5 if mode == "fp32" else 1.0)


def _tamper(mode, kind, family="fog"):
    ref = pcr.reference_for(family, mode, kind)
    cs, cv, s, v = pcr.as_device(ref.members[0], mode)
    return ref, cs.astype(np.int64), cv.astype(np.int64), s.copy(), v.copy()


def _first_photon(ref, cs, cv, min_s=0, min_v=0):
    return int(np.flatnonzero(ref.decided & (cs >= min_s) & (cv >= min_v))[0])


@pytest.mark.parametrize("mode", ["fp32", "fp64"])
def test_rule_rejects_records_swapped_inside_a_chain(mode):
    ref, cs, cv, s, v = _tamper(mode, 1)
    i = _first_photon(ref, cs, cv, min_v=2)
    o = pcr._excl(cv)[i]
    v[[o, o + 1]] = v[[o + 1, o]]
    fails, _, _ = pcr.check(ref, cs, cv, s, v)
    assert fails and all(f"photon {i} " in f for f in fails)


@pytest.mark.parametrize("mode", ["fp32", "fp64"])
def test_rule_rejects_chains_shifted_by_one_photon(mode):
    ref, cs, cv, s, v = _tamper(mode, 1)
    ns0, nv0 = cs[0], cv[0]
    cs, cv = np.roll(cs, -1), np.roll(cv, -1)
    s, v = np.roll(s, -ns0, axis=0), np.roll(v, -nv0, axis=0)
    fails, _, _ = pcr.check(ref, cs, cv, s, v)
    assert len(fails) > 10


@pytest.mark.parametrize("mode", ["fp32", "fp64"])
def test_rule_rejects_a_power_off_by_a_thousandth_from_the_third_vertex_on(mode):
    """Every chain's records from its third vertex on carry (1 + 1e-3) x the power: each such decided chain is named."""
    ref, cs, cv, s, v = _tamper(mode, 1, "flat")
    within = np.arange(len(s)) - np.repeat(pcr._excl(cs), cs)
    s[within >= 2, 6:9] *= 1.0 + 1e-3
    fails, worst, _ = pcr.check(ref, cs, cv, s, v)
    assert fails and worst["surface power"][0] > 1.0 and worst["surface position"][0] < 0.5 and worst["surface power"][2] >= 2
    # ... and a single record of a single chain is enough
    ref, cs, cv, s, v = _tamper(mode, 1, "flat")
    i = _first_photon(ref, cs, cv, min_s=3)
    s[pcr._excl(cs)[i] + 2, 6:9] *= 1.0 + 1e-3
    fails, _, _ = pcr.check(ref, cs, cv, s, v)
    assert len(fails) == 1 and f"photon {i} record 2: surface power" in fails[0]


@pytest.mark.parametrize("mode", ["fp32", "fp64"])
def test_rule_rejects_a_volume_record_in_the_surface_array(mode):
    ref, cs, cv, s, v = _tamper(mode, 1)
    i = _first_photon(ref, cs, cv, min_v=1)
    os_, ov_ = pcr._excl(cs)[i], pcr._excl(cv)[i]
    s = np.insert(s, os_ + cs[i], v[ov_ + cv[i] - 1], axis=0)
    v = np.delete(v, ov_ + cv[i] - 1, axis=0)
    cs[i] += 1
    cv[i] -= 1
    fails, _, _ = pcr.check(ref, cs, cv, s, v)
    assert len(fails) == 2 and all(f"photon {i} (decided)" in f for f in fails)


@pytest.mark.parametrize("mode", ["fp32", "fp64"])
def test_rule_rejects_a_dropped_last_record(mode):
    ref, cs, cv, s, v = _tamper(mode, 1)
    i = _first_photon(ref, cs, cv, min_s=1)
    s = np.delete(s, pcr._excl(cs)[i] + cs[i] - 1, axis=0)
    cs[i] -= 1
    fails, _, _ = pcr.check(ref, cs, cv, s, v)
    assert len(fails) == 1 and f"photon {i} (decided)" in fails[0]
    # the counts left as they were: the arrays no longer add up
    ref, cs, cv, s, v = _tamper(mode, 1)
    fails, _, _ = pcr.check(ref, cs, cv, s[:-1], v)
    assert fails


@pytest.mark.parametrize("mode", ["fp32", "fp64"])
def test_rule_rejects_a_kept_beam_without_its_boost_or_out_of_order(mode):
    ref, cs, cv, s, v = _tamper(mode, 2)
    i = _first_photon(ref, cs, cv, min_v=1)
    o = pcr._excl(cv)[i]
    assert v[o, 6:9].min() > 0
    v[o, 6:9] /= 1000.0
    fails, _, _ = pcr.check(ref, cs, cv, s, v)
    assert len(fails) == 1 and f"photon {i} record 0: volume power" in fails[0]
    # the beam's start (direction slots) replaced by the direction the photon came from
    ref, cs, cv, s, v = _tamper(mode, 2)
    plain = pcr.reference_for("fog", mode, 1).members[0]
    assert np.array_equal(plain["ns"][:4096], ref.members[0]["ns"][:4096])           # the same chains, thinned
    v[o, 3:6] = -v[o, 3:6]
    fails, _, _ = pcr.check(ref, cs, cv, s, v)
    assert len(fails) == 1 and "volume direction" in fails[0]
    assert cv.sum() >= cases.MIN_BEAMS and cv.sum() < 0.002 * plain["nv"].sum() * 16
    # the thinning draws taken one vertex late: the record kept is the volume vertex after the one the reference keeps
    ref, cs, cv, s, v = _tamper(mode, 2)
    pv, po = plain["volume"], pcr._excl(plain["nv"])
    done = False
    for i in np.flatnonzero(ref.decided[:4096] & (cv[:4096] == 1)):
        o = pcr._excl(cv)[i]
        j = np.flatnonzero(np.all(pv[po[i]:po[i] + plain["nv"][i], :3].astype(np.float32) == v[o, :3].astype(np.float32), axis=1))
        assert j.size == 1                                                            # the kept beam ends at a vertex of the plain chain
        if j[0] + 1 < plain["nv"][i]:
            late = pv[po[i] + j[0] + 1]
            v[o] = np.concatenate([late[:3], pv[po[i] + j[0], :3], 1000.0 * late[6:9]]).astype(np.float32)
            done = True
            break
    assert done
    fails, _, _ = pcr.check(ref, cs, cv, s, v)
    assert fails and all(f"photon {i} record 0: volume" in f for f in fails)


def test_an_undecided_chain_is_held_to_one_of_its_signatures():
    """An undecided chain of the fp32 fog: the library may answer with any member's chain, not with a mixture of two."""
    ref, cs, cv, s, v = _tamper("fp32", 1)
    pick = None
    for i, groups in ref.groups.items():
        shapes = {(g["ns"], g["nv"]) for g in groups.values()}
        if len(shapes) >= 2:
            pick = i
            break
    assert pick is not None
    other = next(g for g in ref.groups[pick].values() if (g["ns"], g["nv"]) != (cs[pick], cv[pick]))
    os_, ov_ = pcr._excl(cs)[pick], pcr._excl(cv)[pick]
    s2 = np.concatenate([s[:os_], other["surface"][0].astype(np.float32).astype(np.float64), s[os_ + cs[pick]:]])
    v2 = np.concatenate([v[:ov_], other["volume"][0].astype(np.float32).astype(np.float64), v[ov_ + cv[pick]:]])
    cs2, cv2 = cs.copy(), cv.copy()
    cs2[pick], cv2[pick] = other["ns"], other["nv"]
    fails, _, _ = pcr.check(ref, cs2, cv2, s2, v2)
    assert not fails, fails
    cs3 = cs.copy()
    cs3[pick] += 7                                   # counts no member has
    s3 = np.insert(s, [os_] * 7, s[0], axis=0)
    fails, _, _ = pcr.check(ref, cs3, cv, s3, v)
    assert len(fails) == 1 and "fit no signature" in fails[0]


def test_counts_hook_validates_its_arguments_without_a_gpu():
    """rpt_debug_photon_chain_counts and its option refuse what they must before anything touches a device."""
    import ctypes as C
    from rpt_amd import _lib
    lib = _lib.load()
    h = lib.rpt_scene_create()
    try:
        out = np.zeros(4, dtype=np.uint32)
        ptr = out.ctypes.data_as(C.c_void_p)
        assert lib.rpt_scene_set_option(h, b"photon_keep_counts", 2) != 0 and lib.rpt_scene_set_option(h, b"photon_keep_counts", -1) != 0
        assert lib.rpt_scene_set_option(h, b"photon_keep_counts", 1) == 0
        assert lib.rpt_debug_photon_chain_counts(None, 0, ptr, 4) != 0 and lib.rpt_debug_photon_chain_counts(h, 0, None, 4) != 0
        assert lib.rpt_debug_photon_chain_counts(h, 2, ptr, 4) != 0
        rc = lib.rpt_debug_photon_chain_counts(h, 0, ptr, 4)          # no shooting pass yet: RPT_ERR_STATE
        assert rc == -2 and not out.any()
    finally:
        lib.rpt_scene_destroy(h)
