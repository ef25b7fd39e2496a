"""What the primary scans of a medium test before they scan (option "scan_cull"), on a CPU: tests/host/scan_cull_harness.cpp commits
C3, C2 and four synthetic scenes through the real rpt_capi.cpp and prints SceneView::scan_tail (the box the scan tests before its
tail), scan_bound, scan_groups and scan_always (what the counters build classifies wave trips by) next to every scanned record's box.

  * the tail box holds every box, rectangle and triangle record -- the exact extents of the boxes, the others' with a margin -- and
    no more than their union needs; C3's is the lampshade under the ceiling and reaches y = 618, above the room;
  * a scene without such records has no cull; a plane or more than 64 records do not prevent it (they are not in the tail);
  * every record's box lies inside the box of its group, every group's box and the shell inside the bound; the group masks and the
    always-tested mask partition the records; at most four groups; a box that is most of the bound is in no group;
  * a scene with a plane and a scene with 65 scanned records have no bound and no groups;
  * with the option off the boxes are the same and the scans are not culled.

No GPU, no oracle."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "scan_cull_harness.cpp")
NAMES = ("C3", "C2", "plane", "many", "big", "notail")


def _box(s):
    f = [float(x) for x in s.split(",")]
    return f[:3], f[3:]


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    if not os.path.exists("/opt/rocm/include/hip/hip_runtime_api.h"):
        pytest.skip("HIP headers not installed")
    exe = str(tmp_path_factory.mktemp("scan_cull") / "harness")
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-std=c++17", "-w",
                           "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + os.path.join(ROOT, "include"), SRC, "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1")
    p = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert p.returncode == 0, p.stdout[-1000:] + p.stderr[-2000:]
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-2000:]
    out = {}
    for l in p.stdout.splitlines():
        f = l.split()
        d = dict(kv.split("=", 1) for kv in f[1:])
        out[(f[0], int(d["on"]))] = d
    assert sorted(out) == sorted((n, on) for n in NAMES for on in (0, 1))
    return out


def _inside(inner, outer):
    (ilo, ihi), (olo, ohi) = inner, outer
    return all(olo[a] <= ilo[a] and ihi[a] <= ohi[a] for a in range(3))


def _groups(d):
    return [(int(d[f"gmask{g}"], 16), _box(d[f"gbox{g}"])) for g in range(int(d["n_groups"]))]


def _tail_records(d):
    first = int(d["n_sph"]) + int(d["n_cub"])
    return range(first, int(d["n"]))


@pytest.mark.parametrize("name", ["C3", "C2", "plane", "big"])
def test_the_tail_box_holds_every_record_behind_the_shell(lines, name):
    d = lines[(name, 1)]
    assert d["enabled"] == "1"
    tail = _box(d["tail"])
    recs = [_box(d[f"rec{i}"]) for i in _tail_records(d)]
    assert recs
    for r in recs:
        assert _inside(r, tail), (name, r, tail)
    # ... and is their union, up to the margin of the rectangles and triangles (1e-4 of the scene's extent: below 0.1 in these scenes)
    for a in range(3):
        assert min(r[0][a] for r in recs) - tail[0][a] < 0.1 and tail[1][a] - max(r[1][a] for r in recs) < 0.1
    # a rectangle or a triangle on the tail's boundary lies strictly inside it: a ray in the plane of its edge must not graze the box
    first = int(d["n_sph"]) + int(d["n_cub"]) + int(d["n_aabb"])
    for i in range(first, int(d["n"])):
        rlo, rhi = _box(d[f"rec{i}"])
        assert all(tail[0][a] < rlo[a] and rhi[a] < tail[1][a] for a in range(3)), (name, i)


def test_c3_tail_is_the_lampshade_and_sticks_out_of_the_room(lines):
    d = lines[("C3", 1)]
    assert (d["n_cub"], d["n_aabb"], d["n_rect"], d["has_shell"]) == ("2", "4", "1", "1")
    (tlo, thi), (slo, shi), (blo, bhi) = _box(d["tail"]), _box(d["shell"]), _box(d["bound"])
    assert (tlo, thi) == ([203.0, 478.0, 219.5], [353.0, 618.0, 344.5])
    assert shi[1] == pytest.approx(548.9) and bhi[1] == 618.0                  # the shades stick out of the room
    assert blo[0] == slo[0] and bhi[0] == shi[0] and blo[2] == slo[2] and bhi[2] == shi[2]


def test_a_scene_without_tail_records_is_not_culled_and_many_records_are_no_obstacle(lines):
    assert lines[("notail", 1)]["enabled"] == "0"
    d = lines[("many", 1)]
    assert d["enabled"] == "1" and int(d["n"]) == 65 and d["scene_bvh"] == "0"
    (tlo, thi) = _box(d["tail"])
    # 64 unit boxes on a 9 x 8 grid of pitch 3 (exact) and the light's rectangle at y = 40 (with its margin)
    assert tlo == pytest.approx([-1.0, -0.5, -1.0], abs=0.01) and thi == pytest.approx([24.5, 40.0, 1.0], abs=0.01)
    assert tlo[1] == -0.5 and thi[0] == 24.5 and thi[1] > 40.0 and tlo[0] < -1.0


@pytest.mark.parametrize("name", ["C3", "C2", "big"])
def test_every_record_lies_in_its_group_and_in_the_bound(lines, name):
    d = lines[(name, 1)]
    n, bound, groups, always = int(d["n"]), _box(d["bound"]), _groups(d), int(d["always"], 16)
    assert 1 <= len(groups) <= 4
    seen = always
    for mask, box in groups:
        assert mask and not (mask & seen), "a record is in two groups, or in a group and always tested"
        seen |= mask
        assert _inside(box, bound)
        for i in range(n):
            if (mask >> i) & 1:
                assert _inside(_box(d[f"rec{i}"]), box), (name, i)
    assert seen == (1 << n) - 1, "every record is in a group or always tested"
    for i in range(n):
        assert _inside(_box(d[f"rec{i}"]), bound), (name, i)
    assert _inside(_box(d["tail"]), bound)
    if d["has_shell"] == "1":
        assert _inside(_box(d["shell"]), bound)


def test_c3_groups_follow_the_scene(lines):
    d = lines[("C3", 1)]
    assert int(d["always"], 16) == 0                                            # the shell has no record number: nothing else is large
    masks = sorted(m for m, _ in _groups(d))
    assert masks[:2] == [0b01, 0b10]                                            # each tall box by itself
    assert masks[2] | masks[3] == 0b1111100 and len(masks) == 4                 # the shades and the light's rectangle share two groups


def test_a_box_that_is_most_of_the_bound_is_always_tested(lines):
    d = lines[("big", 1)]
    assert int(d["n_aabb"]) == 7 and int(d["n_sph"]) == 1 and int(d["n_tri"]) == 1
    always = int(d["always"], 16)
    assert always == 1 << int(d["n_sph"])                                       # the first box record (after the sphere)
    assert all(not (m & always) for m, _ in _groups(d))


@pytest.mark.parametrize("name", ["plane", "many"])
def test_scenes_with_a_plane_or_more_than_64_records_have_no_bound_and_no_groups(lines, name):
    d = lines[(name, 1)]
    assert d["scene_bvh"] == "0"
    assert (int(d["n_pln"]) > 0) if name == "plane" else (int(d["n"]) == 65)
    assert d["n_groups"] == "0" and int(d["always"], 16) == 0
    lo, hi = _box(d["bound"])
    assert lo[0] > hi[0]                                                        # "no bound"


@pytest.mark.parametrize("name", NAMES)
def test_option_off_keeps_the_boxes_and_disables_the_cull(lines, name):
    on, off = lines[(name, 1)], lines[(name, 0)]
    assert off["enabled"] == "0"
    for k in on:
        if k not in ("on", "enabled"):
            assert on[k] == off[k], k
