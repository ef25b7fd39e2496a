"""The scan JIT's structure block on a CPU: tests/host/scene_struct_harness.cpp commits C3, C2 and variations of C3 through the real
rpt_capi.cpp and prints the structure a specialised kernel would be compiled with, the cache key of its program and -- where
libhiprtc can be opened here -- the resources of C3's and C2's code objects with and without the block.

  * C3's and C2's structure, field for field; other colours, sizes and places (C3_values) keep string and key;
  * one material kind, one light's shape, one pair's common slabs, one more light: each changes string and key; so does the
    medium's kind once its group, which is outside the default, is switched on;
  * more lights than the block describes: the lights group reads from the view, the others stay;
  * a group switched off (RPT_SCAN_STRUCT_GROUPS) leaves none of its fields in the string;
  * the program is the shape block as it was, the structure block, the include and the instantiation's name, so that the medium keys it too;
  * the compiled kernels stay within the shape-only build's VGPRs and scratch and are no larger.

The harness runs once plain and once under AddressSanitizer and UBSan (a stand-alone program: no preloading).  No GPU, no oracle."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "scene_struct_harness.cpp")
LIGHT = "1:object/mesh/twin/60000000-60000000"          # the quad on the ceiling: a mesh light whose twin is rectangle record 0
C3 = "groups=lights+tables+mats+pairs;lights=" + LIGHT + ";mats=0x1;medium_kind=view;hdri=view;pairs=0x1e"
C2 = "groups=lights+tables+mats+pairs;lights=" + LIGHT + ";mats=0x1;medium_kind=view;hdri=view;pairs=0x0"


def _run(tmp, name, flags):
    exe = str(tmp / name)
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-w", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                           "-I" + os.path.join(ROOT, "include"), SRC, "-o", exe, "-ldl"] + flags)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="halt_on_error=1")
    env.pop("RPT_SCAN_STRUCT_GROUPS", None)
    p = subprocess.run([exe, os.path.join(ROOT, "rpt_amd", "csrc")], capture_output=True, text=True, timeout=900, env=env)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-2000:]
    res = {"struct": {}, "groups": {}, "compile": {}, "program": []}
    lines = p.stdout.splitlines()
    for i, line in enumerate(lines):
        f = line.split()
        if f[0] == "struct":
            res["struct"][f[1]] = dict(kv.split("=", 1) for kv in f[2:] if "=" in kv)
        elif f[0] == "groups":
            res["groups"][int(f[1])] = f[2].split("=", 1)[1]
        elif f[0] == "compile":
            res["compile"][f[1]] = line
        elif f[0] == "program":
            res["program"] = [line[len("program "):]] + lines[i + 1:i + 4]
    return res


@pytest.fixture(scope="module")
def out(tmp_path_factory):
    if not os.path.exists("/opt/rocm/include/hip/hip_runtime_api.h"):
        pytest.skip("HIP headers not installed")
    return _run(tmp_path_factory.mktemp("scene_struct"), "harness", [])


def test_structure_of_c3_and_c2(out):
    for name, want in (("C3", C3), ("C2", C2)):
        s = out["struct"][name]
        assert s["in_scope"] == "1" and s["structure"] == s["query"] == want and s["query_rc"] == "0", (name, s)
    s = out["struct"]["C3"]
    assert (s["short_rc"], s["short"], s["null"]) == ("0", C3[:7], "-1")     # truncated and terminated; a null buffer is refused


def test_record_values_are_not_part_of_it(out):
    a, b = out["struct"]["C3"], out["struct"]["C3_values"]
    assert a["structure"] == b["structure"] and a["shape"] == b["shape"] and a["key"] == b["key"]


@pytest.mark.parametrize("name,field,value,same_shape", [("C3_one_mirror", "mats", "0x5", True), ("C3_sphere_light", "lights", "1:object/sphere/xf/twin/0-0", False),
                                                         ("C3_other_slabs", "pairs", "0x1c", True), ("C3_plus_ambient", "lights", "2" + LIGHT[1:] + "|ambient", True)])
def test_one_change_of_structure_changes_string_and_key(out, name, field, value, same_shape):
    a, b = out["struct"]["C3"], out["struct"][name]
    fa, fb = (dict(kv.split("=", 1) for kv in x["structure"].split(";")) for x in (a, b))
    assert fb[field] == value and fa[field] != value, fb
    assert {k for k in fa if fa[k] != fb[k]} == {field}, (fa, fb)
    assert (a["shape"] == b["shape"]) == same_shape
    assert a["key"] != b["key"] and len(b["key"]) == 32


def test_the_group_outside_the_default_is_a_switch(out):
    """The medium's kind and the HDRI's absence did not pass the acceptance rule: "view" by default, constants with every group switched on."""
    a, b, c = out["struct"]["C3"], out["struct"]["C3_all_groups"], out["struct"]["C3_glowing_fog_all_groups"]
    assert b["structure"] == "groups=lights+tables+mats+small+pairs;lights=" + LIGHT + ";mats=0x1;medium_kind=0;hdri=0;pairs=0x1e"
    assert c["structure"] == b["structure"].replace("medium_kind=0", "medium_kind=1")
    assert len({a["key"], b["key"], c["key"]}) == 3 and a["shape"] == b["shape"] == c["shape"]


def test_more_lights_than_the_block_describes(out):
    s = out["struct"]["C3_six_lights"]
    assert s["structure"] == "groups=tables+mats+pairs;lights=view;mats=0x1;medium_kind=view;hdri=view;pairs=0x1e", s
    assert s["key"] != out["struct"]["C3"]["key"]


def test_a_group_switched_off_leaves_no_field(out):
    g = out["groups"]
    assert g[0] == "groups=none;lights=view;mats=view;medium_kind=view;hdri=view;pairs=view"
    assert g[1] == "groups=lights;lights=" + LIGHT + ";mats=view;medium_kind=view;hdri=view;pairs=view"
    assert g[2] == "groups=tables;lights=view;mats=view;medium_kind=view;hdri=view;pairs=view"
    assert g[4] == "groups=mats;lights=view;mats=0x1;medium_kind=view;hdri=view;pairs=view"
    assert g[8] == "groups=small;lights=view;mats=view;medium_kind=0;hdri=0;pairs=view"
    assert g[16] == "groups=pairs;lights=view;mats=view;medium_kind=view;hdri=view;pairs=0x1e"


def test_program_is_shape_block_structure_block_include(out):
    p = out["program"]
    assert p[0] == "#define RPT_SCAN_SHAPE 0,2,0,4,0,1,0,0,1,1,0x0ull,0x3ull"
    assert p[1] == "#define RPT_SCENE_STRUCT 23,1,111u,0u,0u,0u,1610612736u,0u,0u,0u,1610612736u,0u,0u,0u,1,0,0,0x1eull"
    assert p[2] == '#include "kernels.hip"'
    assert p[3] == "// rptg::render_kernel<true, 0, false, false, 0, false>"        # the medium is in neither block: the name keys it
    assert all(s["begins_with_shape_block"] == "1" for s in out["struct"].values())


def test_the_medium_keys_the_code_object(out):
    """Every count, flag and structure field alike, one scene in fog and one not: two instantiations, two keys."""
    a, b = out["struct"]["C3"], out["struct"]["C3_no_medium"]
    assert a["structure"] == b["structure"] and a["shape"].split(";")[0] == b["shape"].split(";")[0]
    assert (a["shape"].split(";")[1], b["shape"].split(";")[1]) == ("medium=1", "medium=0")
    assert a["key"] != b["key"]


@pytest.mark.parametrize("name,medium,max_scratch", [("C3", "1", 24), ("C2", "0", 0)])
def test_structure_compiles_within_the_shape_only_budget(out, name, medium, max_scratch):
    """The resource rule: no more VGPRs and no more scratch than the code object of the shape block alone (80 / 24 B and 79-80 / 0 as the
    device reports them for C3 and C2), and no larger."""
    line, base = out["compile"][name], out["compile"][name + "_shape_only"]
    if " failed: hiprtc not available" in line:
        pytest.skip("libhiprtc cannot be opened on this machine")
    assert " ok " in line and " ok " in base, (line, base)
    f, b = (dict(kv.split("=", 1) for kv in x.split()[3:]) for x in (line, base))
    print(name, line, "|", base)
    assert f["lowered"] == b["lowered"] == f"_ZN4rptg13render_kernelILb{medium}ELi0ELb0ELb0ELi0ELb0EEEvNS_10RenderArgsE"
    assert f["resources"] == "1" and 0 < int(f["vgprs"]) <= int(b["vgprs"]) <= 80, line
    assert int(f["scratch"]) <= int(b["scratch"]) <= max_scratch, line
    assert 0 < int(f["text_bytes"]) < int(b["text_bytes"]), line


def test_the_harness_under_asan_and_ubsan(tmp_path, out):
    res = _run(tmp_path, "harness_san", ["-fsanitize=address,undefined", "-fno-omit-frame-pointer"])
    assert res["struct"] == out["struct"] and res["groups"] == out["groups"]
