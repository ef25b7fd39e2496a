"""Camera paths against the oracle, one sample at a time, in both modes (tests/path_cloud.py has the scenes, the rule and the caps;
test_path_cloud_host.py pins them with the oracle alone).

The path loop of render_kernel and render_f64_kernel joins pieces that each have a test of their own; what it decides itself -- what
is added at which depth, surface or medium event, the environment in fog only beyond the background distance, the product of the
weights, and the reference's nested firefly clamp restated as a forward running bound -- moves a frame's relative RMS by less than
the frame tests allow, and no small scene of theirs makes the clamp engage.  Here every run is four one-sample frames of 48 x 48 at
the sample offsets the oracle used: 9,216 paths, each of which must be an answer the oracle gives in a small neighbourhood of the
camera, within the caps of path_cloud.caps overall, per stratum (depth, end, clamped) and among the clamped samples.

Every run asserts through scene_stats(), scan_jit_info(), counters() or f64_mesh_tree_info() that the layout is the one it names.
The library is compared with itself only where DESIGN.md states bit identity: "scan_specialise" 1 = 0, "counters" 1 = 0, and the
scan JIT's kernel = the AOT one.  Each test prints its figures ("Camera paths", has them)."""
import os

import numpy as np
import pytest

from rpt_amd import Renderer
from tests import path_cloud as pc

pytestmark = pytest.mark.gpu

N_PIX = pc.SIZE ** 2


@pytest.fixture(scope="module", autouse=True)
def jit_cache(tmp_path_factory):
    """The scan JIT's cache directory is the module's own: "scan_jit" = 1 finds nothing there, 2 compiles."""
    old = {k: os.environ.get(k) for k in ("RPT_JIT_CACHE", "RPT_HIPRTC_LIB")}
    os.environ["RPT_JIT_CACHE"] = str(tmp_path_factory.mktemp("path_cloud_jit_cache"))
    os.environ.pop("RPT_HIPRTC_LIB", None)
    yield
    for k, v in old.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v


def _scan(st):
    return st["scene_bvh"] == 0 and st["bvh_nodes"] == 0 and st["instances"] == 0


def _mesh_tree(st):
    return st["scene_bvh"] == 0 and st["bvh_tris"] == pc.N_TORUS and st["bvh_nodes"] > 0


# what scene_stats() must say of a scene under the default options
DEFAULT_CLAIM = {
    "materials": _scan, "materials fog": _scan, "materials glow": _scan, "clamp": _scan, "clamp fog": _scan, "clamp thin fog": _scan,
    "clamp torus": _mesh_tree,
    "group light": _scan,                         # (its flavour: the layout "group flavour" below)
    "C2": lambda st: _scan(st) and st["shell_faces"] == 5, "C3": lambda st: _scan(st) and st["shell_faces"] == 5,
}
# option set -> (options, scenes, claim on (scene name, scene_stats, scan_jit_info, counters) after the four frames)
VARIED = ("clamp", "clamp fog", "clamp thin fog", "clamp torus", "materials fog")
JIT_SCOPE = ("clamp", "clamp fog", "clamp thin fog", "materials fog")          # linear-scan scenes without group lights


def _jit_runs(name, jit):
    return jit["state"] == "active" and jit["launches"] == len(pc.OFFSETS) if name in JIT_SCOPE else jit["state"] != "active" and jit["launches"] == 0


LAYOUTS = {
    "default": ({}, tuple(pc.SCENES), lambda name, st, jit, cnt: DEFAULT_CLAIM[name](st) and cnt["samples"] == 0),
    "scan_specialise 0": ({"scan_specialise": 0}, VARIED, lambda name, st, jit, cnt: DEFAULT_CLAIM[name](st)),
    "scan_jit 0": ({"scan_jit": 0}, VARIED, lambda name, st, jit, cnt: jit["state"] == "off" and jit["launches"] == 0),
    "scan_jit 2": ({"scan_jit": 2}, VARIED, lambda name, st, jit, cnt: _jit_runs(name, jit)),
    # (C2 and C3 have the room: 5 shell faces by default, asserted above; the other scenes have a floor plane and no shell to take away)
    "room_shell 0": ({"room_shell": 0}, ("C2", "C3"), lambda name, st, jit, cnt: st["shell_faces"] == 0 and st["scene_bvh"] == 0),
    "counters 1": ({"counters": 1}, VARIED, lambda name, st, jit, cnt: DEFAULT_CLAIM[name](st) and cnt["samples"] == N_PIX and cnt["vertices"] > N_PIX),
    "scene tree": ({"scene_bvh_min": 2}, VARIED,
                   lambda name, st, jit, cnt: st["scene_bvh"] == (2 if name == "clamp torus" else 1) and st["scene_bvh_prims"] >= 5),
    "scene tree, meshes inside": ({"scene_bvh_min": 2, "scene_tree_meshes": 1}, ("clamp torus",),
                                  lambda name, st, jit, cnt: st["scene_bvh"] == 1 and st["scene_bvh_prims"] >= 5 and st["bvh_tris"] == pc.N_TORUS),
    # a group as Light::Object runs the kernel flavour that has no counters build: the option leaves its counters at zero
    "group flavour": ({"counters": 1}, ("group light",), lambda name, st, jit, cnt: _scan(st) and cnt["samples"] == 0 and "GROUPS" in jit["reason"]),
}
RUNS = [(layout, name) for layout, (_, names, _) in LAYOUTS.items() for name in names]
_frames = {}


def _four_frames(r):
    """Four consecutive one-sample calls of a fresh renderer: sample offsets 0, 1, 2, 3 as in iterative_render (test_gpu_parity.py,
    test_sample_offset_and_exposure_follow_iterative_render) -> (4 * N_PIX, 3)."""
    assert pc.OFFSETS == tuple(range(len(pc.OFFSETS)))
    return np.concatenate([np.asarray(r.sample_array(1)).reshape(N_PIX, 3) for _ in pc.OFFSETS])


def _fp32(layout, name):
    """The 9,216 samples of a scene under a layout, once per process; asserts the layout."""
    if (layout, name) not in _frames:
        options, _, claim = LAYOUTS[layout]
        sc, cam, mb = pc.build(name)
        for k, v in options.items():
            sc.set_option(k, v)
        r = Renderer(sc, cam).width(pc.SIZE).height(pc.SIZE).max_bounces(mb).seed(pc.SEED)
        got = _four_frames(r)
        st, jit, cnt = r.scene_stats(), r.scan_jit_info(), r.counters()
        print(f"{name}, {layout}: {st}\n  scan JIT: {jit['state']}, launches {jit['launches']}, {jit['reason']}; counters {cnt}")
        assert claim(name, st, jit, cnt), (layout, name, st, jit, cnt)
        _frames[(layout, name)] = got
    return _frames[(layout, name)]


def _hold(cl, got, title):
    rep = pc.check(cl, got)
    fig, bad = pc.caps(cl, rep, title=title)
    if bad:
        pc.show(cl, rep, got)
    assert not bad, bad


# ------------------------------------------------------------------ fp32
@pytest.mark.parametrize("layout,name", RUNS)
def test_fp32_paths_sample_by_sample(layout, name):
    _hold(pc.prepared(name, "fp32"), _fp32(layout, name), f"{name}, {layout}")


@pytest.mark.parametrize("name", VARIED)
def test_fp32_layouts_agree_where_the_design_says_bit_for_bit(name):
    base = _fp32("default", name).view(np.uint64)
    for layout in ("scan_specialise 0", "counters 1", "scan_jit 0", "scan_jit 2"):
        other = _fp32(layout, name).view(np.uint64)
        differ = np.flatnonzero((other != base).any(axis=1))
        assert len(differ) == 0, (layout, len(differ), differ[:8])


def test_fp32_group_flavour_ignores_the_counters_option():
    assert np.array_equal(_fp32("group flavour", "group light").view(np.uint64), _fp32("default", "group light").view(np.uint64))


# ------------------------------------------------------------------ reference-epsilon mode
F64_RUNS = [(name, None) for name in pc.SCENES] + [("clamp torus", 1)]


@pytest.mark.parametrize("name,tree_min", F64_RUNS)
def test_fp64_paths_sample_by_sample(name, tree_min):
    sc, cam, mb = pc.build(name)
    sc.set_option("epsilon_policy", 1)
    if tree_min is not None:
        sc.set_option("f64_mesh_tree_min", tree_min)
    r = Renderer(sc, cam).width(pc.SIZE).height(pc.SIZE).max_bounces(mb).seed(pc.SEED)
    info = r.f64_mesh_tree_info()
    print(f"{name}, f64_mesh_tree_min {tree_min}: {info}")
    assert info["tree_min"] == (64 if tree_min is None else tree_min)
    # the torus (192 triangles) has a candidate tree; no other mesh of these scenes reaches 64 triangles
    assert (info["meshes"], info["triangles"]) == ((1, pc.N_TORUS) if name == "clamp torus" else (0, 0))
    assert info["render_uses_trees"] == 1 or name != "clamp torus"
    got = _four_frames(r)
    _hold(pc.prepared(name, "fp64"), got, f"{name}, reference-epsilon mode, f64_mesh_tree_min {tree_min}")
