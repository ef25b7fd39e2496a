"""rpt_particles_batch_* on the device, through the C ABI: every system of a batch against what it is alone -- the numpy restatement
of include/rpt_hip.h (tests/particles_ref.py) or rpt_particles_integrate_host -- bit for bit: state, display positions and the six
defined counters per system; the launch rule; streams; the refusals; and marbles_field_sequence through Renderer.render_sequence."""
import ctypes as C

import numpy as np
import pytest

from rpt_amd import _lib
from rpt_amd._lib import ParticlesParams, vp

from . import particles_batch_cases as bc
from . import particles_cases as pc
from . import particles_ref as ref
from .particles_batch_cases import STEP, time_of

pytestmark = pytest.mark.gpu
LAUNCH = 256                       # RK4 steps per kernel launch of one round, at most
SCALE = 2                          # ... divided by rounds x this (include/rpt_hip.h)
INVALID, UNSUPPORTED = -1, -4


class Batch:
    def __init__(self, systems):
        self.lib = _lib.load()
        self.ns = [len(s[1]) for s in systems]
        self.first = np.concatenate([[0], np.cumsum(self.ns)])
        self.total = int(self.first[-1])
        prm = (ParticlesParams * len(systems))(*[ParticlesParams(k, len(p), r, h) for k, p, _, r, h in systems])
        self.h = self.lib.rpt_particles_batch_create(0, prm, len(systems))
        assert self.h, self.lib.rpt_last_error()
        pos, vel = np.concatenate([s[1] for s in systems]), np.concatenate([s[2] for s in systems])
        assert self.lib.rpt_particles_batch_set_state(self.h, vp(pos), vp(vel)) == 0

    def set_system_state(self, i, pos, vel):
        pos, vel = np.ascontiguousarray(pos, dtype=np.float64), np.ascontiguousarray(vel, dtype=np.float64)
        assert self.lib.rpt_particles_batch_set_system_state(self.h, i, vp(pos), vp(vel)) == 0

    def integrate(self, time, step=STEP, stream=None):
        assert self.lib.rpt_particles_batch_integrate(self.h, time, step, C.c_void_p(stream)) == 0, self.lib.rpt_last_error()

    def split(self, a):
        return [a[self.first[i]:self.first[i + 1]] for i in range(len(self.ns))]

    def state(self):
        pos, vel = np.zeros((self.total, 3)), np.zeros((self.total, 3))
        assert self.lib.rpt_particles_batch_state(self.h, vp(pos), vp(vel)) == 0
        return self.split(pos), self.split(vel)

    def display(self):
        out = np.zeros((self.total, 3))
        assert self.lib.rpt_particles_batch_display_positions(self.h, vp(out)) == 0, self.lib.rpt_last_error()
        return self.split(out)

    def counters(self):
        out = (C.c_uint64 * (8 * len(self.ns)))()
        assert self.lib.rpt_particles_batch_counters(self.h, out) == 0
        return [[int(x) for x in out[8 * i:8 * i + 8]] for i in range(len(self.ns))]

    def info(self):
        out = (C.c_uint64 * 8)()
        assert self.lib.rpt_particles_batch_info(self.h, out) == 0
        return [int(x) for x in out]

    def close(self):
        self.lib.rpt_particles_batch_destroy(self.h)


def same(a, b):
    return np.array_equal(ref.bits(a), ref.bits(b))


def run_batch(systems, time):
    b = Batch(systems)
    try:
        b.integrate(time)
        return b.state() + (b.counters(), b.info())
    finally:
        b.close()


def check_batch(systems, time, expected, name, launches=1):
    gp, gv, gc, info = run_batch(systems, time)
    for s, (ep, ev, ec) in enumerate(expected):
        assert same(gp[s], ep) and same(gv[s], ev), (name, s, np.argwhere(ref.bits(gp[s]) != ref.bits(ep))[:4].tolist())
        assert gc[s][:6] == list(ec)[:6] and gc[s][6] == launches and gc[s][7] == 0, (name, s, gc[s], ec)
    return gc, info


def run_single(kind, pos, vel, radius, height, time):
    lib = _lib.load()
    prm = ParticlesParams(kind, len(pos), radius, height)
    h = lib.rpt_particles_create(0, C.byref(prm))
    assert h, lib.rpt_last_error()
    try:
        gp, gv, gc = np.zeros_like(pos), np.zeros_like(pos), (C.c_uint64 * 8)()
        assert lib.rpt_particles_set_state(h, vp(pos), vp(vel)) == 0 and lib.rpt_particles_integrate(h, time, STEP, None) == 0
        assert lib.rpt_particles_state(h, vp(gp), vp(gv)) == 0 and lib.rpt_particles_counters(h, gc) == 0
        return gp, gv, [int(x) for x in gc]
    finally:
        lib.rpt_particles_destroy(h)


def test_a_batch_of_one_equals_the_single_handle_for_each_kind():
    for kind, n in ((ref.CIRCLE, 3), (ref.GRAVITY, 7), (ref.MARBLES, 25), (ref.MARBLES, 70)):
        sys_ = bc.system(kind, *pc.random_state(n, 30 + n))
        time = time_of(1 + (n + kind) % 5)
        sp, sv, sc = run_single(*sys_, time)
        gp, gv, gc, info = run_batch([sys_], time)
        assert same(gp[0], sp) and same(gv[0], sv) and gc[0] == sc, (kind, n, gc, sc)          # all eight: one launch each
        assert info[1] == 1 and info[2] == LAUNCH // SCALE and info[4] == n and info[5] == n


def test_three_systems_of_mixed_kinds_and_sizes_match_the_restatement():
    systems = bc.mixed_three()
    for steps in (1, 4):
        time = time_of(steps)
        gc, _ = check_batch(systems, time, bc.by_restatement(systems, time), f"mixed {steps}")
        assert gc[0][1] > 0 and gc[1][1:6] == [0] * 5 and gc[2][0] == 4 * steps


def test_the_staging_decision_of_a_batch_changes_no_bits():
    # n_max = 256: nobody stages, though 1 and 56 would on their own; then (1, 56) stages and (57, 256) does not
    systems = bc.sizes([1, 56, 57, 256])
    time = time_of(3)
    alone = pc.cached("batch_sizes_alone", lambda: bc.by_host_function(systems, time))
    _, info = check_batch(systems, time, alone, "all four")
    assert info[4] == 256
    _, lo = check_batch(systems[:2], time, alone[:2], "(1, 56)")
    _, hi = check_batch(systems[2:], time, alone[2:], "(57, 256)")
    assert lo[4] == 56 and hi[4] == 256 and lo[3] > info[3] == hi[3]          # 56 pays for its pair forces in LDS, 57 does not
    # ... and the restatement agrees with the host function on the small ones
    for got, exp in zip(alone[:2], bc.by_restatement(systems[:2], time)):
        assert same(got[0], exp[0]) and same(got[1], exp[1]) and got[2] == exp[2]


def test_the_families_as_one_batch_reach_every_branch():
    systems = bc.families()
    total = np.zeros(6, dtype=np.uint64)
    for steps in (1, 3):
        time = time_of(steps)
        gc, _ = check_batch(systems, time, pc.cached(("batch_families", steps), lambda: bc.by_restatement(systems, time)), f"families {steps}")
        total += np.array([c[:6] for c in gc], dtype=np.uint64).sum(axis=0)
    assert (total > 0).all(), total                       # every branch ran on the device


def test_more_systems_than_the_device_holds_at_once():
    systems = bc.many_small(1025)
    time = time_of(3)
    _, info = check_batch(systems, time, bc.by_host_function(systems, time), "1,025 small")
    assert info[1] == -(-1025 // info[0]) and info[4] == 3 and info[5] == 2 * 513 + 3 * 512


def test_heavy_blocks_side_by_side():
    # 40 systems of n = 256: with LDS sized for the batch the device takes one or two a CU, so this is one round.  It checks heavy
    # blocks next to each other, not rounds.
    systems = bc.heavy(40)
    time = time_of(2)
    check_batch(systems, time, bc.by_host_function(systems, time), "40 x 256")


def test_rounds_shorten_the_launches():
    # MARBLES, GRAVITY and CIRCLE in turn: the host function's 520 steps of 1,025 systems stay within seconds
    systems = bc.many_small(1025, kinds=(ref.MARBLES, ref.GRAVITY, ref.CIRCLE, ref.GRAVITY), seed=8)
    time = time_of(520)
    b = Batch(systems)
    try:
        resident = b.info()[0]
        rounds = -(-1025 // resident)
        steps_per_launch = max(1, LAUNCH // (rounds * SCALE))
        assert b.info()[1] == rounds and b.info()[2] == steps_per_launch
    finally:
        b.close()
    check_batch(systems, time, bc.by_host_function(systems, time), "520 steps", launches=-(-520 // steps_per_launch))


def test_two_batches_on_two_alternating_streams():
    import torch
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    sys_a, sys_b = bc.mixed_three(), bc.sizes([2, 64, 5], seed=50)
    a, b = Batch(sys_a), Batch(sys_b)
    try:
        for k in range(4):
            a.integrate(3 * STEP, STEP, (sa, sb)[k % 2].cuda_stream)
            b.integrate(3 * STEP, STEP, (sb, sa)[k % 2].cuda_stream)
        for batch, systems in ((a, sys_a), (b, sys_b)):
            gp, gv = batch.state()
            for s, (kind, p, v, radius, height) in enumerate(systems):
                for _ in range(4):
                    p, v, _ = ref.rk4_integrate(kind, radius, height, p, v, 3 * STEP, STEP)
                assert same(gp[s], p) and same(gv[s], v), s
    finally:
        a.close()
        b.close()


def test_set_system_state_while_an_integrate_is_queued_behind_a_render():
    import torch
    from rpt_amd import Renderer, scenes
    scene, cam, cfg = scenes.lampshade()
    st = torch.cuda.Stream()
    out = torch.zeros(128 * 128 * 3, dtype=torch.float64, device="cuda:0")
    r = Renderer(scene, cam).width(128).height(128).max_bounces(cfg["max_bounces"]).seed(1)
    systems = bc.mixed_three()
    p1, v1 = pc.random_state(7, 9)
    b = Batch(systems)
    try:
        r.sample_device(16, out.data_ptr(), st.cuda_stream)
        b.integrate(5 * STEP, STEP, st.cuda_stream)          # queued behind the render
        b.set_system_state(1, p1, v1)                        # ordered behind the integrate: it must not be overwritten by it
        b.integrate(2 * STEP, STEP, st.cuda_stream)
        gp, gv = b.state()
        for s, (kind, p, v, radius, height) in enumerate(systems):
            if s == 1:
                p, v = p1, v1
            else:
                p, v, _ = ref.rk4_integrate(kind, radius, height, p, v, 5 * STEP, STEP)
            p, v, _ = ref.rk4_integrate(kind, radius, height, p, v, 2 * STEP, STEP)
            assert same(gp[s], p) and same(gv[s], v), s
        evaluations = 4 * (ref.step_sequence(5 * STEP, STEP)[0] + ref.step_sequence(2 * STEP, STEP)[0] + 2)
        assert [c[0] for c in b.counters()] == [evaluations] * 3
        torch.cuda.synchronize()
    finally:
        b.close()


def test_display_positions_of_a_batch_of_the_families():
    systems = bc.families() + [bc.system(ref.MARBLES, pc.random_state(256, 3)[0], np.zeros((256, 3)), radius=0.12, height=2.5)]
    b = Batch(systems)
    try:
        for s, (got, (_, pos, _, radius, height)) in enumerate(zip(b.display(), systems)):
            assert same(got, ref.display_positions(radius, height, pos)), s
        assert b.counters()[0][6] == 1
    finally:
        b.close()


def test_marbles_field_sequence_renders_the_restatements_frames():
    from rpt_amd import ParticleState, Renderer, scenes
    time = 5 * STEP
    offsets = scenes.marbles_field_offsets((2, 1), 3.0)
    start = [(np.array([[0.5, 0.2, 0.0], [0.7, 0.21, 0.0], [-0.3, 0.6, 0.2]]), pc.velocities(3, 1)),          # three marbles per glass
             (np.array([[0.05, 0.05, 0.0], [0.45, 0.3, 0.1], [0.2, 0.5, -0.3]]), pc.velocities(3, 2))]
    states, shown = start, []
    for _ in range(3):
        shown.append([ref.display_positions(pc.R, pc.HEIGHT, p) + np.array([ox, 0.0, oz]) for (p, _), (ox, oz) in zip(states, offsets)])
        states = [ref.rk4_integrate(ref.MARBLES, pc.R, pc.HEIGHT, p, v, time, STEP)[:2] for p, v in states]

    def render(seq):
        seq = list(seq)
        scene, cam, cfg = scenes.marbles_field(shown[0], offsets)
        r = Renderer(scene, cam).width(48).height(32).max_bounces(cfg["max_bounces"]).seed(3).num_samples(8)
        return [np.array(f) for f in r.render_sequence([c for _, c in seq], batches=2, scenes=[s for s, _ in seq])]

    got = render(scenes.marbles_field_sequence(3, grid=(2, 1), spacing=3.0, time=time, states=[ParticleState(p, v) for p, v in start]))
    exp = render([scenes.marbles_field(p, offsets)[:2] for p in shown])
    assert len(got) == 3 and all(np.array_equal(a, b) for a, b in zip(got, exp))
    assert got[0].shape == (32, 48, 3) and got[0].any() and not np.array_equal(got[0], got[2])


def test_every_refusal_by_code_and_message():
    lib = _lib.load()

    def said(word):
        return word in lib.rpt_last_error().decode()

    good = [ParticlesParams(ref.MARBLES, 3, pc.R, pc.HEIGHT), ParticlesParams(ref.GRAVITY, 2, 0.0, 0.0), ParticlesParams(ref.MARBLES, 1, pc.R, pc.HEIGHT)]
    arr = (ParticlesParams * 3)(*good)
    assert not lib.rpt_particles_batch_create(0, None, 3) and said("null particle parameters")
    assert not lib.rpt_particles_batch_create(0, arr, 0) and said("1..4096")
    assert not lib.rpt_particles_batch_create(0, arr, 4097) and said("1..4096")
    for field, value, word in (("n", 0, "1..256"), ("n", 257, "1..256"), ("kind", 3, "kind"), ("radius", float("nan"), "finite"), ("height", float("inf"), "finite")):
        bad = (ParticlesParams * 3)(*good)
        setattr(bad[1], field, value)
        bad[2].radius = 0.0                                # a later bad system is not the one that is named
        assert not lib.rpt_particles_batch_create(0, bad, 3) and said("system 1:") and said(word), (field, lib.rpt_last_error())
    bad = (ParticlesParams * 3)(*good)
    bad[2].radius = 0.0
    assert not lib.rpt_particles_batch_create(0, bad, 3) and said("system 2:") and said("radius > 0")
    assert not lib.rpt_particles_batch_create(99, arr, 3) and said("device")
    h = lib.rpt_particles_batch_create(0, arr, 3)
    assert h, lib.rpt_last_error()
    try:
        buf, cnt = np.zeros((6, 3)), (C.c_uint64 * 24)()
        for time, step, word in ((-1.0, 1.0, "time"), (float("inf"), 1.0, "time"), (1.0, 0.0, "step"), (1.0, float("nan"), "step"), (1048577.0, 1.0, "2^20")):
            assert lib.rpt_particles_batch_integrate(h, time, step, None) == INVALID and said(word)
            assert lib.rpt_particles_batch_integrate(None, time, step, None) == INVALID and said(word)       # before the handle
        assert lib.rpt_particles_batch_integrate(None, 1.0, 1.0, None) == INVALID and said("null particle ensemble")
        assert lib.rpt_particles_batch_set_state(h, None, None) == INVALID and said("null positions")
        assert lib.rpt_particles_batch_set_state(None, vp(buf), None) == INVALID and said("ensemble")
        assert lib.rpt_particles_batch_set_system_state(h, 0, None, None) == INVALID and said("null positions")
        assert lib.rpt_particles_batch_set_system_state(h, 3, vp(buf), None) == INVALID and said("system index out of range")
        assert lib.rpt_particles_batch_set_system_state(None, 0, vp(buf), None) == INVALID and said("ensemble")
        assert lib.rpt_particles_batch_state(h, None, None) == INVALID and said("null outputs")
        assert lib.rpt_particles_batch_state(None, vp(buf), None) == INVALID and said("ensemble")
        assert lib.rpt_particles_batch_state_device(h, None, None, None) == INVALID and said("null outputs")
        assert lib.rpt_particles_batch_display_positions(h, None) == INVALID and said("null output")
        assert lib.rpt_particles_batch_display_positions(None, vp(buf)) == INVALID and said("ensemble")
        assert lib.rpt_particles_batch_display_positions(h, vp(buf)) == UNSUPPORTED and said("marbles systems only")
        assert lib.rpt_particles_batch_counters(h, None) == INVALID and said("null output")
        assert lib.rpt_particles_batch_counters(None, cnt) == INVALID and said("ensemble")
        assert lib.rpt_particles_batch_info(h, None) == INVALID and said("null output")
        assert lib.rpt_particles_batch_counters(h, cnt) == 0 and list(cnt) == [0] * 24          # no refused call launched anything
    finally:
        lib.rpt_particles_batch_destroy(h)
