"""MonomialSurface without a GPU: the public descriptors (kind 5, height / exp in plane_normal, the 200-byte rpt_shape_desc),
transforms and KdTree children, and the fp64 restatement of tests/monomial_ref.py on known cases."""
import ctypes as C
import math

import numpy as np

from rpt_amd import KdTree, MonomialSurface, Transformed, monomial_surface, sphere, vec3
from rpt_amd import _lib
from rpt_amd.api import shape_desc
from tests.monomial_ref import closest_hit, intersect_local, intersect_world


def test_descriptor_of_the_shape():
    assert C.sizeof(_lib.ShapeDesc) == 200
    for name, off in [("kind", 0), ("has_transform", 4), ("transform", 8), ("plane_normal", 136), ("plane_value", 160),
                      ("tris", 168), ("n_tris", 176), ("children", 184), ("n_children", 192)]:
        assert getattr(_lib.ShapeDesc, name).offset == off
    s = monomial_surface(2.0, 4.0)
    assert isinstance(s, MonomialSurface) and (s.height, s.exp) == (2.0, 4.0)
    d, _ = shape_desc(s, _lib.ShapeDesc)
    assert d.kind == 5 and d.has_transform == 0
    assert list(d.plane_normal) == [2.0, 4.0, 0.0]


def test_transforms_and_kdtree_children():
    s = monomial_surface(-0.5, 3.0).scale(vec3(2.0, 1.0, 0.5)).rotate_y(0.3).translate(vec3(1.0, 2.0, 3.0))
    assert isinstance(s, Transformed) and isinstance(s.base(), MonomialSurface)
    c, sn = math.cos(0.3), math.sin(0.3)
    rot = np.array([[c, 0, sn, 0], [0, 1, 0, 0], [-sn, 0, c, 0], [0, 0, 0, 1]])
    exp = np.array([[1, 0, 0, 1], [0, 1, 0, 2], [0, 0, 1, 3], [0, 0, 0, 1.0]]) @ rot @ np.diag([2.0, 1.0, 0.5, 1.0])
    assert np.allclose(s.matrix(), exp, atol=1e-15)
    g = KdTree([s, sphere()]).translate(vec3(0.0, -1.0, 0.0))
    d, keep = shape_desc(g, _lib.ShapeDesc)
    assert d.kind == 4 and d.n_children == 2 and d.has_transform == 1
    child = d.children[0]
    assert child.kind == 5 and child.has_transform == 1 and list(child.plane_normal)[:2] == [-0.5, 3.0]
    assert np.allclose(np.array(child.transform[:]).reshape(4, 4), exp)
    # the group's bounds are its children's boxes merged: the transformed local box [-1, min(0, h), -1]..[1, max(0, h), 1]
    corners = np.array([[x, y, z, 1.0] for x in (-1, 1) for y in (-0.5, 0.0) for z in (-1, 1)]) @ exp.T
    lo, hi = corners[:, :3].min(axis=0), corners[:, :3].max(axis=0)
    assert np.all(lo < hi)


def test_restatement_known_cases():
    ok, t, n = intersect_local([[0.5, 3.0, 0.3]], [[0.0, -1.0, 0.0]], 2.0, 1e-12)   # straight down onto y = 2 (0.34)^2
    assert ok[0] and abs(t[0] - 2.7688) < 1e-12
    assert n[0][1] > 0.0   # two-sided: the normal faces the ray
    ok, t, _ = intersect_local([[0.9, -1.0, 0.1]], [[0.0, 1.0, 0.0]], 2.0, 1e-12)   # deriv2 = -0: Newton steps to infinity
    assert ok[0] and np.isnan(t[0])
    d = np.array([[1e-9, 1.0, 0.0]])
    d /= np.linalg.norm(d)
    ok, _, _ = intersect_local([[0.9, -1.0, 0.1]], d, 2.0, 1e-12)                   # tilted by 1e-9: a miss (surface at y ~ 1.35)
    assert not ok[0]
    ok, _, _ = intersect_local([[0.5, 3.0, 0.3]], [[0.0, -1.0, 0.0]], 2.0, 1e-12, rec_time=[2.0])   # a closer record stays
    assert not ok[0]
    ok, _, _ = intersect_local([[2.0, 3.0, 0.0]], [[0.0, -1.0, 0.0]], 2.0, 1e-12)   # outside x^2 + z^2 <= 1
    assert not ok[0]


def test_restatement_under_a_transform_and_in_scene_order():
    m = np.array([[2.0, 0, 0, 1.0], [0, 0.5, 0, -1.0], [0, 0, 2.0, 0.0], [0, 0, 0, 1.0]])
    ok, t, n = intersect_world([[1.5, 5.0, 0.5]], [[0.0, -1.0, 0.0]], 2.0, 1e-12, m)
    # local ray: origin (0.25, 12, 0.25), direction (0, -2, 0); local hit at y = 2 (0.125)^2 = 0.03125
    assert ok[0] and abs(t[0] - (12.0 - 0.03125) / 2.0) < 1e-12
    assert abs(np.linalg.norm(n[0]) - 1.0) < 1e-15
    # two copies at the same place: an equal time replaces the record (monomial_surface.rs:85), so the later one wins
    tt, obj, _ = closest_hit([[0.5, 3.0, 0.3]], [[0.0, -1.0, 0.0]], [(2.0, None), (2.0, None)])
    assert obj[0] == 1 and abs(tt[0] - 2.7688) < 1e-12
