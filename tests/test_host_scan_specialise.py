"""Commit-time scan specialisation (option "scan_specialise") on a CPU: tests/host/scan_specialise_harness.cpp commits C3, C2 and
two synthetic scenes through the real rpt_capi.cpp with the option on and off and prints the marks the unmasked scans read.

  * C3: both cubes are marked as rotations about the vertical axis, its four shade boxes form the pairs (right, left) with the
    y and z slabs in common and (front, back) with x and y in common; C2: its cube and its sphere are marked;
  * a cube rotated about x, a sheared one and one with 1e-30 where the zero belongs are not marked; a y-rotated sphere is;
  * two boxes whose upper y planes differ in the last bit share z only, an identical pair shares all three, a last box without
    a partner nothing;
  * with the option off nothing is marked, and every scanned array (hence record order and hit codes) and the lights' twin code
    ranges are the same bytes either way.

No GPU, no oracle."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "scan_specialise_harness.cpp")


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    if not os.path.exists("/opt/rocm/include/hip/hip_runtime_api.h"):
        pytest.skip("HIP headers not installed")
    exe = str(tmp_path_factory.mktemp("scan_specialise") / "harness")
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
        d["shared"] = [int(x) for x in d["shared"].split(",") if x]
        d["boxes"] = [[[int(w, 16) for w in half.split(".")] for half in b.split(":")] for b in d["boxes"].split(",") if b]
        out[(f[0], int(d["on"]))] = d
    assert sorted(out) == sorted((n, on) for n in ("C3", "C2", "mixed", "lastbit") for on in (0, 1))
    return out


def test_c3_and_c2_records_are_marked(lines):
    c3 = lines[("C3", 1)]
    assert (c3["n_sph"], c3["n_cub"], c3["n_aabb"]) == ("0", "2", "4")
    assert int(c3["cub_yrot"], 16) == 0b11 and int(c3["sph_yrot"], 16) == 0
    assert c3["shared"] == [0b110, 0, 0b011, 0]          # (right, left): y and z;  (front, back): x and y
    c2 = lines[("C2", 1)]
    assert (c2["n_sph"], c2["n_cub"], c2["n_aabb"]) == ("1", "1", "0")
    assert int(c2["cub_yrot"], 16) == 1 and int(c2["sph_yrot"], 16) == 1


def test_only_exact_vertical_axis_rotations_are_marked(lines):
    m = lines[("mixed", 1)]
    assert (m["n_sph"], m["n_cub"]) == ("1", "4")
    # cubes in scene order: about y, about x, sheared, about y with 1e-30 in place of a zero
    assert int(m["cub_yrot"], 16) == 0b0001
    assert int(m["sph_yrot"], 16) == 1


def test_slabs_are_shared_only_when_bit_equal_and_only_within_a_pair(lines):
    d = lines[("lastbit", 1)]
    assert d["n_aabb"] == "5"
    (lo0, hi0), (lo1, hi1) = d["boxes"][0], d["boxes"][1]
    assert lo0[1] == lo1[1] and hi1[1] == hi0[1] + 1     # the upper y planes are neighbouring fp32 values
    assert lo0[2] == lo1[2] and hi0[2] == hi1[2] and lo0[0] != lo1[0]
    assert d["shared"] == [0b100, 0, 0b111, 0, 0]


@pytest.mark.parametrize("name", ["C3", "C2", "mixed", "lastbit"])
def test_option_off_marks_nothing_and_changes_no_record(lines, name):
    on, off = lines[(name, 1)], lines[(name, 0)]
    assert int(off["sph_yrot"], 16) == 0 and int(off["cub_yrot"], 16) == 0 and not any(off["shared"])
    assert on["records"] == off["records"] and on["boxes"] == off["boxes"]       # record order, hence hit codes
    assert on["twins"] == off["twins"] and on["twins"]                            # twin code ranges of the lights
