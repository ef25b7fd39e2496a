"""Moving spheres, the parts that need no GPU.

  * rpt_sphere_records_host (rpt_amd/csrc/scene_update_core.h run once on the host) against the numpy restatement of
    tests/scene_update_ref.py, bit for bit: 2,000 random (r, c, p) with r in [1e-3, 1e3] and coordinates in +-1e4, and hand-made cases
    (c = 0, c = p, c on an axis, r = 1, negative zero, coordinates at 1e-30 and 1e30); the motion record also against
    rpt_temporal_motion_record of the two matrices through the C ABI.
  * tests/host/scene_update_harness.cpp, a stand-alone program over malloc-backed HIP stubs that drives the real rpt_capi.cpp and
    rpt_scene_update.cpp, built plain and under AddressSanitizer + UBSan (no failure, no report, the same output): the same cases
    against a fresh flatten of a scene with that sphere in both modes (arena bytes), every refusal in the stated order, the life cycle, a list replaced after a move,
    moved scenes against fresh commits with the kernels' lane functions run serially, and the refit's host preparation, whose dumped
    tables this file checks with numpy on a 70-sphere scene (the height lists are a child-before-parent order; fixed boxes plus movable
    boxes reproduce every committed node box exactly before any move and after a move onto the same places).

No GPU, no oracle; nothing loaded into Python runs under a sanitizer."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from rpt_amd import _lib
from rpt_amd.api import temporal_motion_record
from tests import scene_update_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "scene_update_harness.cpp")
COMMON = ["-std=c++17", "-w", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + os.path.join(ROOT, "include")]

HAND = [
    (1.0, (0.0, 0.0, 0.0), (1.0, 2.0, 3.0)),          # c = 0, r = 1
    (0.5, (1.0, 2.0, 3.0), (1.0, 2.0, 3.0)),          # c = p: the identity record
    (2.0, (0.0, 5.0, 0.0), (0.0, 0.0, 0.0)),          # c on an axis
    (0.15, (-3.0, 0.0, 0.0), (0.0, 0.0, 4.0)),
    (1.0, (-0.0, 0.0, -0.0), (0.0, 0.0, 0.0)),        # negative zero, and equal to p as numbers
    (0.3, (-0.0, 1.0, -0.0), (0.0, -1.0, 0.0)),
    (0.3, (1e-30, -1e-30, 1e-30), (0.0, 0.0, 0.0)),
    (0.3, (1e30, -1e30, 1e30), (1.0, 1.0, 1.0)),
    (1e-3, (1e30, 1e-30, -0.0), (1e30, 1e-30, 0.0)),
    (1e3, (1e4, -1e4, 1e4), (-1e4, 1e4, -1e4)),
    (0.15, (0.125, 0.09, -0.375), (0.125, 4.5, -0.375)),   # a marble at rest in the glass, and where it fell from
]


def cases():
    rng = np.random.default_rng(20260)
    n = 2000
    r = 10.0 ** rng.uniform(-3.0, 3.0, n)
    c, p = rng.uniform(-1e4, 1e4, (n, 3)), rng.uniform(-1e4, 1e4, (n, 3))
    out = [(float(r[i]), tuple(c[i]), tuple(p[i])) for i in range(n)]
    return out + HAND


def host_records(r, c, p):
    lib = _lib.load()
    scan, shade, item, pbox = (np.zeros(k, dtype=np.float32) for k in (12, 12, 6, 8))
    inv, nrm, motion = np.zeros(12), np.zeros(9), np.zeros(24)
    cull = np.zeros(1, dtype=ref.CULL)
    c, p = np.array(c, dtype=np.float64), np.array(p, dtype=np.float64)
    rc = lib.rpt_sphere_records_host(float(r), c.ctypes.data_as(C.POINTER(C.c_double)), p.ctypes.data_as(C.POINTER(C.c_double)), _lib.vp(scan),
                                     _lib.vp(shade), _lib.vp(item), _lib.vp(pbox), _lib.vp(inv), _lib.vp(nrm), _lib.vp(cull), _lib.vp(motion))
    return rc, dict(scan=scan, shade=shade, item=item, pbox=pbox, inv=inv, nrm=nrm, cull=cull[0], motion=motion)


def same(a, b):
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()


def test_host_records_equal_the_restatement_bit_for_bit():
    bad = []
    for i, (r, c, p) in enumerate(cases()):
        rc, got = host_records(r, c, p)
        want = ref.sphere_records(r, c)
        motion = ref.sphere_motion_record(r, c, p)
        shade = np.zeros(12, dtype=np.float32)
        shade[[0, 5, 10]] = want["shade_n"]
        shade[7] = 1.0
        nrm = np.zeros(9)
        nrm[[0, 4, 8]] = want["nrm"]
        checks = {
            "scan": same(got["scan"], want["scan"]), "shade": same(got["shade"], shade),
            "item": same(got["item"], np.concatenate([want["item_lo"], want["item_hi"]])),
            "pbox": same(got["pbox"], np.concatenate([want["pbox_lo"], [np.float32(0)], want["pbox_hi"], [np.float32(0)]]).astype(np.float32)),
            "inv": same(got["inv"], want["inv"]), "nrm": same(got["nrm"], nrm),
            "cull": same(got["cull"]["lo"], want["cull_lo"]) and same(got["cull"]["hi"], want["cull_hi"]) and int(got["cull"]["unbounded"]) == want["unbounded"]
                    and int(got["cull"]["slab_test"]) == 0,
            "motion": (rc == 0 and motion is not None and same(got["motion"], motion)) or (rc != 0 and motion is None),
        }
        bad += [(i, r, c, k) for k, ok in checks.items() if not ok]
    assert not bad, bad[:10]


def test_motion_record_is_rpt_temporal_motion_record_of_the_two_matrices():
    for r, c, p in cases()[::7] + HAND:
        rc, got = host_records(r, c, p)
        assert rc == 0
        want = temporal_motion_record(ref.matrix(r, c), ref.matrix(r, p))
        assert same(got["motion"], np.asarray(want, dtype=np.float64).reshape(-1)), (r, c, p)
    # matrices that compare equal: the exact identity record, whatever the signs of their zeros
    for r, c, p in (HAND[1], HAND[4], HAND[8]):
        assert same(host_records(r, c, p)[1]["motion"], ref.IDENTITY_RECORD)


def test_the_hand_made_cases_reach_what_they_are_for():
    """The restatement itself: an unbounded cull box where fp32 cannot hold it, exact zeros off the diagonal, N = r^2 / r^3."""
    big = ref.sphere_records(1e3, (3.40282e38, 0.0, 0.0))
    assert big["unbounded"] == 1 and not big["cull_lo"].any() and not big["cull_hi"].any()
    rc, got = host_records(1e3, (3.40282e38, 0.0, 0.0), (0.0, 0.0, 0.0))
    assert int(got["cull"]["unbounded"]) == 1 and not got["cull"]["lo"].any() and not got["cull"]["hi"].any()
    rec = ref.sphere_records(0.15, (0.3, -0.2, 0.1))
    scan = rec["scan"].reshape(3, 4)
    assert all(scan[i, j] == 0.0 and not np.signbit(scan[i, j]) for i in range(3) for j in range(3) if i != j)   # the y-rotation bits stay
    r = np.float64(0.15)
    assert rec["nrm"] == (r * r) / (r * (r * r)) and rec["nrm"] != 1.0 / r   # (for this r the two differ in the last bit)


# ---- the harness
def _build_and_run(tmp_path, name, flags, cases_file, dumps):
    exe = str(tmp_path / name)
    subprocess.check_call(["g++"] + flags + COMMON + [SRC, "-o", exe])
    os.makedirs(dumps, exist_ok=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    p = subprocess.run([exe, cases_file, dumps], capture_output=True, text=True, env=env, timeout=900)
    print(p.stdout[-8000:])
    assert "MISMATCH" not in p.stdout, "\n".join(l for l in p.stdout.splitlines() if "MISMATCH" in l)[:4000]
    assert p.returncode == 0, p.stderr[-2000:]
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-2000:]
    return p.stdout


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    if not os.path.exists("/opt/rocm/include/hip/hip_runtime_api.h"):
        pytest.skip("HIP headers not installed")
    tmp = tmp_path_factory.mktemp("scene_update")
    cases_file = str(tmp / "cases.bin")
    np.array([[r, *c, *p] for r, c, p in cases()], dtype=np.float64).tofile(cases_file)
    san = _build_and_run(tmp, "san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer"], cases_file, str(tmp / "dump_san"))
    plain = _build_and_run(tmp, "plain", ["-O1"], cases_file, str(tmp / "dump"))
    assert san == plain
    return plain.splitlines(), str(tmp / "dump")


@pytest.mark.timeout(1800)
def test_records_equal_a_fresh_flatten_in_both_modes(harness):
    lines, _ = harness
    assert f"flatten cases={len(cases())} mismatches=0" in lines
    assert lines[-1] == "total mismatches=0"


def test_every_refusal_in_the_stated_order(harness):
    lines, _ = harness
    got = {}
    for l in lines:
        if l.startswith("refusal ") and ": rc=" in l:
            what, rest = l[len("refusal "):].split(": rc=", 1)
            rc, msg = rest.split(" ", 1)
            got[what] = (int(rc), msg)
    INVALID, STATE, UNSUPPORTED = -1, -2, -4
    want = {
        "null scene": (INVALID, "null scene"), "null list": (INVALID, "null object list"), "before commit": (STATE, "rpt_scene_commit"),
        "move before commit": (STATE, "rpt_scene_commit"), "move with no list": (STATE, "rpt_scene_set_movable_spheres must be called first"),
        "move_device with no list": (STATE, "rpt_scene_set_movable_spheres must be called first"),
        "index out of range": (INVALID, "names object 99"), "listed twice": (INVALID, "object 1 is listed twice"),
        "group": (UNSUPPORTED, "is a group"), "plane": (INVALID, "object 0 is not a sphere"), "cube": (INVALID, "object 2 is not a sphere"),
        "light twin": (UNSUPPORTED, "twin of a Light::Object"), "no transform": (INVALID, "has no transform"),
        "off-diagonal": (INVALID, "non-zero off-diagonal"), "not uniform": (INVALID, "does not scale uniformly"),
        "negative radius": (INVALID, "must be finite and > 0"), "radius without a motion record": (INVALID, "admits no motion record"),
        "bottom row": (INVALID, "bottom row of the transform of object 10"), "centre not finite": (INVALID, "centre of object 11 is not finite"),
        # the list (fine, cube): the first bad entry in list order is the one that is named
        "order: the first bad entry is named": (INVALID, "object 2 is not a sphere"),
        "fine": (0, "-"), "null centres": (INVALID, "null centres"), "null device centres": (INVALID, "null centres"),
        "records: unknown array": (INVALID, "unknown array"), "records: fp64 array of an fp32 scene": (STATE, "epsilon_policy = 1"),
        "records: buffer too small": (INVALID, "too small"),
    }
    for what, (rc, part) in want.items():
        assert what in got, what
        assert got[what][0] == rc and part in got[what][1], (what, got[what])
    assert "refusal scene: objects 0 1 2 3 4 5 6 7 8 9 10 11 commit=0" in lines   # the scene takes all twelve objects: every refusal above is the list's own


def test_the_life_cycle_over_stubs(harness):
    lines, _ = harness
    assert "lifecycle before set: scan bound present" in lines
    assert "lifecycle set: rc=0 scan bound absent groups=0" in lines          # the diagnostics a moved sphere would make stale are gone
    assert "lifecycle set again: rc=0 listed=1 moves=0" in lines               # a second call replaces the list
    assert "lifecycle move on a stream: rc=0 moves=1 photon map stale=1 launches=1" in lines
    assert "lifecycle table: sphere=2 object=3 centre=7 8 9" in lines           # the table holds the new centre
    assert "lifecycle destroyed" in lines


def test_moved_scenes_equal_fresh_commits(harness):
    lines, _ = harness
    updates = [l for l in lines if l.startswith("update ")]
    assert len(updates) == 18 and all(l.endswith("mismatches=0") for l in updates), updates
    assert any("65:" in l and "eps=1" in l and "groups=3" in l and "tree_nodes=31" in l for l in updates)   # cull32 groups on both sides of a boundary, and a tree
    assert any("33:" in l and "eps=1" in l and "groups=2" in l for l in updates)
    assert any("25, none" in l and "listed=0" in l for l in updates)


def test_a_second_list_starts_where_the_first_left_the_spheres(harness):
    """set, move, set with another list, move, four lists in turn on the 70-sphere scene with its tree, in both modes: the records equal a
    fresh commit's, a listed sphere's motion row starts at the centre an earlier list left it at, and a sphere that was moved and then
    dropped from the list stays inside its leaf's refitted box."""
    lines, _ = harness
    assert not [l for l in lines if l.startswith("relist") and ("MISMATCH" in l or "failed" in l)]
    for eps in (0, 1):
        assert any(l.startswith(f"relist eps={eps} lists=4 tree_nodes=") and l.endswith("mismatches=0") and "tree_nodes=0 " not in l for l in lines)


def test_refit_preparation_against_numpy(harness):
    lines, dumps = harness
    assert any(l.startswith("refit set=0 same=0 move=0 listed=47 ") for l in lines), lines[-3:]

    def load(name, dtype):
        return np.fromfile(os.path.join(dumps, name), dtype=dtype)

    nodes = load("nodes_committed.bin", ref.NODE)
    entries, order = load("entries.bin", ref.ENTRY), load("order.bin", "<u4")
    raw = load("raw_committed.bin", "<f4").reshape(-1, 2, 4)[:, :, :3]
    items = load("items_committed.bin", "<f4").reshape(-1, 2, 4)
    assert len(nodes) >= 35 and len(entries) == 2 * len(nodes) and len(order) == len(nodes) and len(items) == 47
    ref.check_order(entries, order)
    # leaves hold movable spheres, fixed items, or both; inner entries exist
    kinds = [(int(e["a"]) == ref.INNER, int(e["a"]) not in (ref.NONE, ref.INNER), bool(np.isfinite(e["lo"][0]))) for e in entries]
    assert any(k[0] for k in kinds) and any(k[1] and k[2] for k in kinds) and any(k[1] and not k[2] for k in kinds) and any(not k[0] and not k[1] for k in kinds)
    listed = sorted(int(m) for e in entries for m in (e["a"], e["b"]) if int(e["a"]) != ref.INNER and int(m) != ref.NONE)
    assert listed == list(range(47))   # every movable sphere is in exactly one leaf
    # before any move: fixed boxes + movable boxes reproduce every committed bound and every committed node box, bit for bit
    got_raw, got_boxes = ref.refit(entries, order, items)
    assert same(got_raw, raw)
    assert same(got_boxes, ref.node_boxes(nodes))
    # a move onto the same places changes no byte of the nodes
    assert same(load("nodes_same.bin", ref.NODE), nodes)
    # a move: the boxes are the refit of the moved item boxes; the topology words stay
    moved = load("nodes_moved.bin", ref.NODE)
    items_moved = load("items_moved.bin", "<f4").reshape(-1, 2, 4)
    assert not same(items_moved, items)
    raw_m, boxes_m = ref.refit(entries, order, items_moved)
    assert same(boxes_m, ref.node_boxes(moved)) and same(raw_m, load("raw_moved.bin", "<f4").reshape(-1, 2, 4)[:, :, :3])
    assert same(moved["e0"], nodes["e0"]) and same(moved["e1"], nodes["e1"]) and not same(ref.node_boxes(moved), ref.node_boxes(nodes))
