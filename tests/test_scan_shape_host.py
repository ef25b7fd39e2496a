"""The scan JIT's host half on a CPU: tests/host/scan_shape_harness.cpp commits C3, C2 and variations of C3 through the real
rpt_capi.cpp and prints the shape a specialised kernel would be compiled for, cache keys, a cache file's round trip and -- where
libhiprtc can be opened here -- the result of compiling C3's and C2's shapes.

  * the shape of C3 and of C2 is the counts and flags of the committed view, field for field;
  * another size, angle and place of an object keeps the shape; one more record of any kind, a general rotation where a y-rotation
    was, or "scan_cull" off changes it;
  * the cache key changes with one byte of the program text, of an included file, of the options, and with the compiler's version;
  * the query and the option check their arguments;
  * a cache file is written whole or not at all and a truncated one is refused;
  * the compiled kernels carry the AOT kernel's mangled names and stay within its 80 VGPRs.

No GPU, no oracle."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "scan_shape_harness.cpp")
C3 = "0,2,0,4,0,1,0,0,1,1,0x0ull,0x3ull;medium=1"
C2 = "1,1,0,0,0,1,0,0,1,1,0x1ull,0x1ull;medium=0"


@pytest.fixture(scope="module")
def out(tmp_path_factory):
    if not os.path.exists("/opt/rocm/include/hip/hip_runtime_api.h"):
        pytest.skip("HIP headers not installed")
    d = tmp_path_factory.mktemp("scan_shape")
    exe = str(d / "harness")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-w", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                           "-I" + os.path.join(ROOT, "include"), SRC, "-o", exe, "-ldl"])
    p = subprocess.run([exe, os.path.join(ROOT, "rpt_amd", "csrc"), str(d)], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    res = {"shape": {}, "query": {}, "compile": {}}
    for line in p.stdout.splitlines():
        f = line.split()
        if f[0] in ("shape", "query"):
            res[f[0]][f[1]] = dict(kv.split("=", 1) for kv in f[2:] if "=" in kv)
        elif f[0] == "compile":
            res["compile"][f[1]] = line
        else:
            res[f[0]] = dict(kv.split("=", 1) for kv in f[1:] if "=" in kv) or f[1:]
    return res


def test_shape_is_the_committed_views_counts(out):
    for name, want in (("C3", C3), ("C2", C2)):
        s = out["shape"][name]
        assert s["in_scope"] == "1" and s["shape"] == s["view"] == want, (name, s)


def test_record_values_are_not_part_of_the_shape(out):
    assert out["shape"]["C3_moved"]["shape"] == C3


@pytest.mark.parametrize("name,field", [("C3_plus_sphere", 0), ("C3_plus_cube", 1), ("C3_plus_plane", 2), ("C3_plus_box", 3), ("C3_plus_rect_x", 4),
                                        ("C3_plus_rect_y", 5), ("C3_plus_rect_z", 6), ("C3_plus_triangle", 7), ("C3_no_cull", 9),
                                        ("C3_general_rotation", 11)])
def test_counts_and_flags_are(out, name, field):
    s = out["shape"][name]
    assert s["shape"] == s["view"] and s["shape"] != C3
    got, base = s["shape"].split(";")[0].split(","), C3.split(";")[0].split(",")
    assert got[field] != base[field], (name, got)
    if field <= 7:
        assert int(got[field]) == int(base[field]) + 1
    if name == "C3_general_rotation":
        assert got[11] == "0x2ull"                       # the first cube is no y-rotation any more; the count stayed
        assert got[:11] == base[:11]


def test_cache_key_follows_every_byte(out):
    k = out["key"]
    assert k["base"] == k["again"] and len(k["base"]) == 32
    assert len({k["base"], k["text"], k["header"], k["options"], k["version"], k["c2"]}) == 6, k
    assert out["sources"] == ["kernels.hip", "kernels.h", "gpu_layout.h", "device_core.h"] or sorted(out["sources"]) == sorted(
        ["kernels.hip", "kernels.h", "gpu_layout.h", "device_core.h"])


def test_option_and_query_check_their_arguments(out):
    o = out["options"]
    assert (o["uncommitted"], o["set0"], o["set2"], o["set3"], o["setneg"]) == ("-2", "0", "0", "-1", "-1")
    q = out["query"]["C3"]
    assert (q["rc"], q["state"], q["text"]) == ("0", "1", C3)            # idle before any render, and the shape is known
    assert (q["null_scene"], q["null_out"], q["capacity_without_buffer"]) == ("-1", "-1", "-1")
    assert q["short"] == "0" and q["short_text"] == C3[:3]               # truncated, terminated


def test_cache_file_round_trip(out):
    c = out["cache"]
    assert (c["write"], c["read"], c["same"], c["truncated_read"], c["unwritable_write"]) == ("1", "1", "1", "0", "0"), c


@pytest.mark.parametrize("name,medium", [("C3", "1"), ("C2", "0")])
def test_shapes_compile_within_the_register_budget(out, name, medium):
    line = out["compile"][name]
    if " failed: hiprtc not available" in line:
        pytest.skip("libhiprtc cannot be opened on this machine")
    assert " ok " in line, line
    f = dict(kv.split("=", 1) for kv in line.split()[3:])
    assert f["lowered"] == f"_ZN4rptg13render_kernelILb{medium}ELi0ELb0ELb0ELi0ELb0EEEvNS_10RenderArgsE"
    assert f["resources"] == "1" and 0 < int(f["vgprs"]) <= 80, line
    print(name, line)
