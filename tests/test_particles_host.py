"""The particle systems without a GPU: the numpy restatement (tests/particles_ref.py) against the line-by-line transcription of the
reference's Rust; the library's host functions (rpt_particles_integrate_host, rpt_particles_derivative_host,
rpt_monomial_closest_point, rpt_particles_display_positions_host) against the restatement, bit for bit, counters included; the
branches the hand-made states of tests/particles_cases.py claim; the reference's own unit tests; every refusal in its order; the
Python mirrors."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from rpt_amd import (MarblesSystem, MonomialSurface, ParticleState, RptError, SimpleCircleSystem, SolidGravitySystem, _lib,
                     monomial_surface, scenes)
from rpt_amd._lib import ParticlesParams, vp

from . import particles_cases as pc
from . import particles_ref as ref

STEP = 1.0 / 10000.0
KINDS = (ref.CIRCLE, ref.GRAVITY, ref.MARBLES)


def same(a, b):
    return np.array_equal(ref.bits(a), ref.bits(b))


def host_integrate(kind, pos, vel, time, step, n=None, radius=pc.R, height=pc.HEIGHT):
    pos, vel = np.array(pos, dtype=np.float64).reshape(-1, 3), np.array(vel, dtype=np.float64).reshape(-1, 3)
    prm, cnt = ParticlesParams(kind, len(pos) if n is None else n, radius, height), (C.c_uint64 * 8)()
    rc = _lib.load().rpt_particles_integrate_host(C.byref(prm), vp(pos), vp(vel), time, step, cnt)
    return rc, pos, vel, list(cnt)


def all_states():
    out = [(name, pos, vel) for name, pos, vel in pc.family_states()]
    for n in (1, 2, 3, 25):
        out.append((f"random-{n}", *pc.random_state(n, 40 + n)))
    return out


def test_the_hand_made_states_take_the_branches_they_claim():
    for name, (pos, claim) in pc.FAMILIES.items():
        pos = np.array(pos, dtype=np.float64)
        for vel in (np.zeros_like(pos), pc.velocities(len(pos))):
            (_, acc), cnt, m = ref.derivative(ref.MARBLES, pc.R, pc.HEIGHT, pos, vel)
            assert {k for k in pc.MASKS if m[k].any()} == claim, name
            if name in ("origin", "coincident"):
                assert np.isnan(acc).all(), name
            else:
                assert np.isfinite(acc).all(), name
            if name == "axis":
                assert np.isnan(m["closest"][0, 0]) and np.isnan(m["closest"][0, 2])
            if name == "inside":
                assert ((pc.R - 0.06) - pos[0, 1]) / pc.R >= 0.0 and ref.length(pos)[0] <= 0.1      # the table would push; it is off
    moving = pc.velocities(1)
    (_, a0), _, _ = ref.derivative(ref.MARBLES, pc.R, pc.HEIGHT, [[0.5, 0.395, 0.0]], np.zeros((1, 3)))
    (_, a1), _, _ = ref.derivative(ref.MARBLES, pc.R, pc.HEIGHT, [[0.5, 0.395, 0.0]], moving)
    (_, a2), _, _ = ref.derivative(ref.MARBLES, pc.R, pc.HEIGHT, [[0.3, 5.0, 0.2]], moving)
    assert not same(a1 - a0, a2 - np.array([[0.0, -1.0, 0.0]]))                                     # the band's nv^3 term is not multiplied by zero


def test_restatement_equals_the_transcription():
    for kind in KINDS:
        for name, pos, vel in all_states():
            (dp, dv), cnt, _ = ref.derivative(kind, pc.R, pc.HEIGHT, pos, vel)
            tp, tv, tc = ref.t_derivative(kind, pc.R, pc.HEIGHT, pos.tolist(), vel.tolist())
            assert same(dp, np.array(tp)) and same(dv, np.array(tv)) and [int(x) for x in cnt] == tc, (kind, name)
    for i, (name, pos, vel) in enumerate(all_states()):
        kind, steps = KINDS[i % 3] if not name.startswith("random") else ref.MARBLES, 1 + i % 5
        time = steps * STEP * (1.0 - 2.0 ** -30)
        a, b = ref.rk4_integrate(kind, pc.R, pc.HEIGHT, pos, vel, time, STEP), ref.t_rk4_integrate(kind, pc.R, pc.HEIGHT, pos, vel, time, STEP)
        assert same(a[0], b[0]) and same(a[1], b[1]) and np.array_equal(a[2], b[2]) and int(a[2][0]) == 4 * steps, (kind, name)
    for p in ([0.3, 0.7, -0.2], [0.0, 3.0, 0.0], [0.0, 0.0, 0.0], [1e-13, 0.0, 0.0], [5.0, -1.0, 2.0], [math.nan, 1.0, 0.0], [1e200, 1.0, 0.0]):
        assert same(ref.closest_point(2.0, [p])[0], np.array(ref.t_closest_point(2.0, p))), p
        assert same(ref.closest_point(1.0, [p], precise=True)[0], np.array(ref.t_closest_point(1.0, p, 10000))), p


def test_host_functions_equal_the_restatement_bit_for_bit():
    lib = _lib.load()
    for kind in KINDS:
        for i, (name, pos, vel) in enumerate(all_states()):
            prm = ParticlesParams(kind, len(pos), pc.R, pc.HEIGHT)
            dp, dv, cnt = np.zeros_like(pos), np.zeros_like(pos), (C.c_uint64 * 8)()
            assert lib.rpt_particles_derivative_host(C.byref(prm), vp(pos), vp(vel), vp(dp), vp(dv), cnt) == 0
            (ep, ev), ec, _ = ref.derivative(kind, pc.R, pc.HEIGHT, pos, vel)
            assert same(dp, ep) and same(dv, ev) and list(cnt)[:6] == [int(x) for x in ec], (kind, name)
            steps = 1 + i % 5
            time = steps * STEP * (1.0 - 2.0 ** -30)
            rc, gp, gv, gc = host_integrate(kind, pos, vel, time, STEP)
            ep, ev, ec = ref.rk4_integrate(kind, pc.R, pc.HEIGHT, pos, vel, time, STEP)
            assert rc == 0 and same(gp, ep) and same(gv, ev) and gc == [int(x) for x in ec] + [0, 0], (kind, name, steps)


def test_one_full_frame_from_the_touching_state():
    pos, vel = pc.touching_state()
    ep, ev, ec = pc.full_frame_reference()
    rc, gp, gv, gc = host_integrate(ref.MARBLES, pos, vel, 1.0 / 16.0, STEP)
    assert rc == 0 and same(gp, ep) and same(gv, ev) and np.isfinite(ep).all()
    assert gc[:6] == [int(x) for x in ec] and gc[0] == 4 * 625 and all(x > 0 for x in gc[:6]), gc   # marbles touch each other, the glass and the table
    assert same(MarblesSystem(pc.R).display_positions(gp), ref.display_positions(pc.R, pc.HEIGHT, ep))


def test_closest_point_and_display_positions_equal_the_restatement():
    rng = np.random.default_rng(5)
    pts = np.concatenate([rng.uniform(-1.5, 1.5, (200, 3)), [[0, 3, 0], [0, 0, 0], [1e-13, 0, 0], [0, 0, 1e-11], [0.5, 0.125, 0], [7, 9, -3], [np.nan, 0, 1], [np.inf, 1, 0]]])
    for height in (2.0, 1.0, -0.5):
        surf = MonomialSurface(height, 4.0)
        coarse, fine = ref.closest_point(height, pts), ref.closest_point(height, pts, precise=True)
        for p, c, f in zip(pts, coarse, fine):
            assert same(surf.closest_point(p), c) and same(surf.closest_point_precise(p), f), p
    pos = np.concatenate([pts[:60], [[0, 3, 0], [0, 0, 0], [0.5, 0.2, 0.0], [3, -5, 0], [np.nan, np.nan, np.nan]]])
    assert same(MarblesSystem(pc.R).display_positions(pos), ref.display_positions(pc.R, pc.HEIGHT, pos))
    assert ref.display_positions(pc.R, pc.HEIGHT, [[3, -5, 0]])[0, 1] == pc.R - 0.06
    assert ref.display_positions(pc.R, pc.HEIGHT, [[np.nan] * 3])[0, 1] == pc.R - 0.06                # f64::max: the operand that is not NaN


def test_the_references_unit_tests():
    # monomial_closest_point_works (height 1): the closest point to a point ON the surface is within 0.03 of it
    surf = monomial_surface(1.0, 4.0)
    zs = [1.0, -1.0, 0.00001, -0.00001, 0.0, 1e-13, 1e-12, 1e-11, 1e-10] + [s * i / 10000.0 for i in range(1, 10000, 7) for s in (1, -1)]
    for x, z in [(0.23234, 0.723423), (0.12323, -0.23423)] + [(0.0, z) for z in zs]:
        pt = np.array([x, (x ** 2 + z ** 2) ** 2, z])
        assert np.linalg.norm(pt - surf.closest_point(pt)) < 0.03, (x, z)
    # rk4_works: the circle returns after tau, and is at (-1, 0, 0) after pi
    for device_free_time, where in ((math.tau, [1.0, 0.0, 0.0]), (math.pi, [-1.0, 0.0, 0.0])):
        s = ParticleState([[1.0, 0.0, 0.0]])
        SimpleCircleSystem().rk4_integrate(s, device_free_time, 0.005, device=None)
        assert np.linalg.norm(s.pos[0] - where) < 1e-3 and (s.vel == 0.0).all()


def test_the_remainder_step():
    c, last = ref.step_sequence(1.0 / 16.0, 1.0 / 10000.0)
    assert (c, last) == (624, 9.999999999924044e-05)
    pos, vel = pc.random_state(3, 1)
    rc, gp, gv, gc = host_integrate(ref.MARBLES, pos, vel, 1.0 / 16.0, STEP)
    ep, ev, _ = ref.rk4_steps(ref.MARBLES, pc.R, pc.HEIGHT, pos, vel, [STEP] * 624 + [last])
    assert rc == 0 and gc[0] == 4 * 625 and same(gp, ep) and same(gv, ev)
    wrong, _, _ = ref.rk4_steps(ref.MARBLES, pc.R, pc.HEIGHT, pos, vel, [STEP] * 625)
    assert not same(wrong, ep)
    rc, gp, _, gc = host_integrate(ref.CIRCLE, [[1.0, 2.0, 3.0]], [[0.0] * 3], 0.0, STEP)                 # time 0: one step of size 0
    assert rc == 0 and gc[0] == 4 and same(gp, [[1.0, 2.0, 3.0]])


def test_every_refusal_in_its_order():
    lib = _lib.load()
    pos, vel = pc.random_state(2, 1)

    def why():
        return lib.rpt_last_error().decode()

    def integ(prm, p, v, time, step):
        return lib.rpt_particles_integrate_host(C.byref(prm) if prm else None, p, v, time, step, (C.c_uint64 * 8)())
    good = ParticlesParams(ref.MARBLES, 2, pc.R, pc.HEIGHT)
    # the parameters first, in the header's order, whatever else is wrong with the call
    for prm, word in ((None, "null particle parameters"), (ParticlesParams(3, 2, pc.R, 2.0), "kind"), (ParticlesParams(-1, 2, pc.R, 2.0), "kind"),
                      (ParticlesParams(2, 0, pc.R, 2.0), "1..256"), (ParticlesParams(2, 257, pc.R, 2.0), "1..256"),
                      (ParticlesParams(2, 2, math.nan, 2.0), "finite"), (ParticlesParams(1, 2, 1.0, math.inf), "finite"),
                      (ParticlesParams(2, 2, 0.0, 2.0), "radius > 0"), (ParticlesParams(2, 2, -1.0, 2.0), "radius > 0")):
        assert integ(prm, None, None, -1.0, 0.0) == -1 and word in why(), word
        assert lib.rpt_particles_create(0, C.byref(prm) if prm else None) is None and word in why(), word
        assert lib.rpt_particles_display_positions_host(C.byref(prm) if prm else None, None, None) == -1 and word in why(), word
    assert integ(ParticlesParams(ref.GRAVITY, 2, 0.0, 0.0), vp(pos.copy()), vp(vel.copy()), STEP, STEP) == 0   # the radius of another system may be 0
    # then time, step and the length of the sequence, then the state
    for time, step, word in ((-1.0, 0.0, "time"), (math.nan, 1.0, "time"), (math.inf, 1.0, "time"), (1.0, 0.0, "step"), (1.0, -1.0, "step"),
                             (1.0, math.nan, "step"), (1.0, math.inf, "step"), (1048577.0, 1.0, "2^20"), (1.0, 1e-300, "2^20")):
        assert integ(good, None, None, time, step) == -1 and word in why(), (time, step)
        assert lib.rpt_particles_integrate(None, time, step, None) == -1 and word in why(), (time, step)      # ... before the handle
    assert integ(good, None, None, 1.0, 1.0) == -1 and "null state" in why()
    assert lib.rpt_particles_integrate(None, 1.0, 1.0, None) == -1 and "null particle system" in why()
    assert lib.rpt_particles_display_positions_host(C.byref(ParticlesParams(ref.GRAVITY, 2, 0.0, 0.0)), vp(pos), vp(pos.copy())) == -4
    assert lib.rpt_monomial_closest_point(math.nan, (C.c_double * 3)(), 0, (C.c_double * 3)()) == -1
    assert lib.rpt_monomial_closest_point(2.0, None, 0, (C.c_double * 3)()) == -1
    for fn in (lib.rpt_particles_state, lib.rpt_particles_set_state):
        assert fn(None, vp(pos), vp(vel)) == -1 and "null particle system" in why()
    assert lib.rpt_particles_display_positions(None, vp(pos)) == -1 and lib.rpt_particles_counters(None, (C.c_uint64 * 8)()) == -1
    with pytest.raises(RptError):
        MarblesSystem(0.0).time_derivative(ParticleState(pos))
    # state values that are not finite are accepted
    weird = [[math.nan, 1.0, 0.0], [0.3, math.inf, 0.0]]
    rc, gp, gv, _ = host_integrate(ref.MARBLES, weird, [[0.0] * 3] * 2, STEP, STEP)
    ep, ev, _ = ref.rk4_integrate(ref.MARBLES, pc.R, pc.HEIGHT, weird, [[0.0] * 3] * 2, STEP, STEP)
    assert rc == 0 and np.isnan(gp[0, 0]) and same(gp, ep) and same(gv, ev)                            # NaN propagates as defined


def test_python_mirrors():
    a, b = ParticleState([[1.0, 2.0, 3.0]], [[0.5, 0.25, 0.125]]), ParticleState([[3.0, 2.0, 1.0]])
    s = (a + b) * 2.0 / 4.0
    assert s.pos.tolist() == [[2.0, 2.0, 2.0]] and s.vel.tolist() == [[0.25, 0.125, 0.0625]] and len(s) == 1
    pos, vel = pc.random_state(5, 2)
    for system, kind in ((SimpleCircleSystem(), ref.CIRCLE), (SolidGravitySystem(), ref.GRAVITY), (MarblesSystem(pc.R), ref.MARBLES)):
        d = system.time_derivative(ParticleState(pos, vel))
        (ep, ev), _, _ = ref.derivative(kind, pc.R, 2.0, pos, vel)
        assert same(d.pos, ep) and same(d.vel, ev)
        st = ParticleState(pos, vel)
        assert system.rk4_integrate(st, 3.5 * STEP, STEP, device=None) is st
        ep, ev, _ = ref.rk4_integrate(kind, pc.R, 2.0, pos, vel, 3.5 * STEP, STEP)
        assert same(st.pos, ep) and same(st.vel, ev)
    init = scenes.marbles_initial()
    assert len(init) == 25 and (init.vel == 0).all() and ((init.pos[:, 1] >= 4.0) & (init.pos[:, 1] < 6.0)).all()
    assert init.pos[7].tolist()[::2] == [1 / 5.0 - 0.375, 2 / 5.0 - 0.375] and same(init.pos, scenes.marbles_initial().pos)
    scene, cam, cfg = scenes.marbles(MarblesSystem(0.15).display_positions(init.pos))
    assert len(scene.objects) == 27 and cfg == {"width": 800, "height": 600, "spp": 2000, "max_bounces": 9}


def test_cpp_mirror_host_rk4_equals_the_library(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "mirror")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-ffp-contract=off", "-I" + os.path.join(root, "include"),
                           os.path.join(root, "tests", "host", "particles_mirror_check.cpp"), "-o", exe, "-L" + os.path.join(root, "rpt_amd"),
                           "-lrpt_hip", "-Wl,-rpath," + os.path.join(root, "rpt_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout.startswith("1 "), out.stdout + out.stderr
    x = float(out.stdout.split()[1])
    assert abs(x + 1.0) < 1e-3                                   # rk4_works: at (-1, 0, 0) after pi
