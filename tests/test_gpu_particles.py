"""rpt_particles_* on the device against the numpy restatement of include/rpt_hip.h (tests/particles_ref.py), bit for bit: state,
display positions and the six defined counters, through the C ABI; the host function next to the kernel; the launch split; streams;
and the marbles sequence through Renderer.render_sequence."""
import ctypes as C

import numpy as np
import pytest

from rpt_amd import _lib
from rpt_amd._lib import ParticlesParams, vp

from . import particles_cases as pc
from . import particles_ref as ref

pytestmark = pytest.mark.gpu
STEP = 1.0 / 10000.0
LAUNCH = 256                       # RK4 steps per kernel launch, at most


def launches(steps):
    return -(-steps // LAUNCH)


class Handle:
    def __init__(self, kind, pos, vel, radius=pc.R, height=pc.HEIGHT):
        self.lib = _lib.load()
        self.n = len(pos)
        self.prm = ParticlesParams(kind, self.n, radius, height)
        self.h = self.lib.rpt_particles_create(0, C.byref(self.prm))
        assert self.h, self.lib.rpt_last_error()
        self.set_state(pos, vel)

    def set_state(self, pos, vel):
        pos, vel = np.ascontiguousarray(pos, dtype=np.float64), np.ascontiguousarray(vel, dtype=np.float64)
        assert self.lib.rpt_particles_set_state(self.h, vp(pos), vp(vel)) == 0

    def integrate(self, time, step, stream=None):
        assert self.lib.rpt_particles_integrate(self.h, time, step, C.c_void_p(stream)) == 0, self.lib.rpt_last_error()

    def state(self):
        pos, vel = np.zeros((self.n, 3)), np.zeros((self.n, 3))
        assert self.lib.rpt_particles_state(self.h, vp(pos), vp(vel)) == 0
        return pos, vel

    def display(self):
        out = np.zeros((self.n, 3))
        assert self.lib.rpt_particles_display_positions(self.h, vp(out)) == 0, self.lib.rpt_last_error()
        return out

    def counters(self):
        out = (C.c_uint64 * 8)()
        assert self.lib.rpt_particles_counters(self.h, out) == 0
        return [int(x) for x in out]

    def close(self):
        self.lib.rpt_particles_destroy(self.h)


def same(a, b):
    return np.array_equal(ref.bits(a), ref.bits(b))


def run_device(kind, pos, vel, time, step, **kw):
    h = Handle(kind, pos, vel, **kw)
    try:
        h.integrate(time, step)
        return h.state() + (h.counters(),)
    finally:
        h.close()


def check(kind, pos, vel, steps, name):
    # `steps` steps of STEP: a time just short of steps * STEP makes the loop's last step the remainder
    time = steps * STEP * (1.0 - 2.0 ** -30)
    c, _ = ref.step_sequence(time, STEP)
    assert c + 1 == steps
    gp, gv, gc = run_device(kind, pos, vel, time, STEP)
    ep, ev, ec = ref.rk4_integrate(kind, pc.R, pc.HEIGHT, pos, vel, time, STEP)
    assert same(gp, ep) and same(gv, ev), (name, steps, np.argwhere(ref.bits(gp) != ref.bits(ep))[:4].tolist())
    assert gc[:6] == [int(x) for x in ec] and gc[6] == 1 and gc[7] == 0, (name, gc, ec)
    return gc


def test_families_match_the_restatement_and_reach_every_branch():
    total = np.zeros(6, dtype=np.uint64)
    for i, (name, pos, vel) in enumerate(pc.family_states()):
        total += np.array(check(ref.MARBLES, pos, vel, 1 + i % 5, name)[:6], dtype=np.uint64)
    assert (total > 0).all(), total                       # every branch ran on the device


# 56 | 57: up to 56 particles the kernel stages the pair forces in LDS, above it every lane computes its own
@pytest.mark.parametrize("n", [1, 2, 3, 25, 56, 57, 63, 64, 65, 70, 256])
def test_random_states_match_the_restatement(n):
    for kind in (ref.CIRCLE, ref.GRAVITY, ref.MARBLES):
        pos, vel = pc.random_state(n, 100 + n)
        check(kind, pos, vel, 1 + (n + kind) % 5, f"kind {kind} n {n}")


def test_gravity_and_circle_families():
    for name, pos, vel in pc.family_states():
        if name.startswith(("pair_contact", "coincident", "free_fall")):
            for kind in (ref.CIRCLE, ref.GRAVITY):
                check(kind, pos, vel, 3, name)


def test_full_frame_from_the_touching_state():
    pos, vel = pc.touching_state()
    ep, ev, ec = pc.full_frame_reference()
    gp, gv, gc = run_device(ref.MARBLES, pos, vel, 1.0 / 16.0, STEP)
    assert same(gp, ep) and same(gv, ev)
    assert gc[:6] == [int(x) for x in ec] and all(x > 0 for x in gc[:6]) and gc[0] == 2500 and gc[6] == launches(625), gc


def test_several_launches_equal_one_host_call_and_the_device_equals_the_host_function():
    lib = _lib.load()
    pos, vel = pc.touching_state()
    time = 1030 * STEP * (1.0 - 2.0 ** -30)
    assert ref.step_sequence(time, STEP)[0] + 1 == 1030
    gp, gv, gc = run_device(ref.MARBLES, pos, vel, time, STEP)
    hp, hv, hc = pos.copy(), vel.copy(), (C.c_uint64 * 8)()
    prm = ParticlesParams(ref.MARBLES, 25, pc.R, pc.HEIGHT)
    assert lib.rpt_particles_integrate_host(C.byref(prm), vp(hp), vp(hv), time, STEP, hc) == 0
    assert same(gp, hp) and same(gv, hv) and gc[:6] == list(hc)[:6] and gc[6] == launches(1030) == 5 and gc[0] == 4 * 1030, (gc, list(hc))
    for kind, n in ((ref.GRAVITY, 7), (ref.CIRCLE, 3), (ref.MARBLES, 70)):
        pos, vel = pc.random_state(n, 5)
        gp, gv, gc = run_device(kind, pos, vel, 4.5 * STEP, STEP)
        hp, hv = pos.copy(), vel.copy()
        prm = ParticlesParams(kind, n, pc.R, pc.HEIGHT)
        assert lib.rpt_particles_integrate_host(C.byref(prm), vp(hp), vp(hv), 4.5 * STEP, STEP, hc) == 0
        assert same(gp, hp) and same(gv, hv) and gc[:6] == list(hc)[:6]


def _frames_reference(frames):
    def run():
        pos, vel = pc.dropped_state()
        out = []
        for _ in range(frames):
            pos, vel, _ = ref.rk4_integrate(ref.MARBLES, pc.R, pc.HEIGHT, pos, vel, 1.0 / 16.0, STEP)
            out.append((pos, vel, ref.display_positions(pc.R, pc.HEIGHT, pos)))
        return out
    return pc.cached(("frames", frames), run)


def test_eight_chained_frames_and_their_display_positions():
    pos, vel = pc.dropped_state()
    h = Handle(ref.MARBLES, pos, vel)
    try:
        for f, (ep, ev, ed) in enumerate(_frames_reference(8)):
            h.integrate(1.0 / 16.0, STEP)
            gp, gv = h.state()
            assert same(gp, ep) and same(gv, ev), f
            assert same(h.display(), ed), f
        c = h.counters()
        assert c[0] == 8 * 2500 and c[6] == 8 * (launches(625) + 1) and c[3] > 0, c
    finally:
        h.close()


def test_display_positions_of_the_families():
    for name, pos, vel in pc.family_states():
        h = Handle(ref.MARBLES, pos, vel)
        try:
            assert same(h.display(), ref.display_positions(pc.R, pc.HEIGHT, pos)), name
        finally:
            h.close()
    pos, _ = pc.random_state(256, 3)
    h = Handle(ref.MARBLES, pos, np.zeros_like(pos))
    try:
        assert same(h.display(), ref.display_positions(pc.R, pc.HEIGHT, pos))
    finally:
        h.close()
    lib = _lib.load()
    g = Handle(ref.GRAVITY, pos[:3], pos[:3])
    try:
        out = np.zeros((3, 3))
        assert lib.rpt_particles_display_positions(g.h, vp(out)) == -4        # RPT_ERR_UNSUPPORTED
    finally:
        g.close()


def test_two_handles_on_two_alternating_streams():
    import torch
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    pa, va = pc.random_state(25, 1)
    pb, vb = pc.random_state(64, 2)
    ha, hb = Handle(ref.MARBLES, pa, va), Handle(ref.MARBLES, pb, vb)
    try:
        for k in range(4):
            ha.integrate(3 * STEP, STEP, (sa, sb)[k % 2].cuda_stream)
            hb.integrate(3 * STEP, STEP, (sb, sa)[k % 2].cuda_stream)
        for h, p, v in ((ha, pa, va), (hb, pb, vb)):
            for _ in range(4):
                p, v, _ = ref.rk4_integrate(ref.MARBLES, pc.R, pc.HEIGHT, p, v, 3 * STEP, STEP)
            gp, gv = h.state()
            assert same(gp, p) and same(gv, v)
    finally:
        ha.close()
        hb.close()


def test_set_state_while_an_integrate_is_queued_behind_a_render():
    import torch
    from rpt_amd import Renderer, scenes
    scene, cam, cfg = scenes.lampshade()
    st = torch.cuda.Stream()
    out = torch.zeros(128 * 128 * 3, dtype=torch.float64, device="cuda:0")
    r = Renderer(scene, cam).width(128).height(128).max_bounces(cfg["max_bounces"]).seed(1)
    p0, v0 = pc.random_state(25, 8)
    p1, v1 = pc.random_state(25, 9)
    h = Handle(ref.MARBLES, p0, v0)
    try:
        r.sample_device(16, out.data_ptr(), st.cuda_stream)
        h.integrate(5 * STEP, STEP, st.cuda_stream)         # queued behind the render
        h.set_state(p1, v1)                                 # ordered behind the integrate: it must not be overwritten by it
        h.integrate(2 * STEP, STEP, st.cuda_stream)
        gp, gv = h.state()
        ep, ev, _ = ref.rk4_integrate(ref.MARBLES, pc.R, pc.HEIGHT, p1, v1, 2 * STEP, STEP)
        assert same(gp, ep) and same(gv, ev)
        assert h.counters()[0] == 4 * (ref.step_sequence(5 * STEP, STEP)[0] + ref.step_sequence(2 * STEP, STEP)[0] + 2)
        torch.cuda.synchronize()
    finally:
        h.close()


def test_marbles_sequence_renders_the_restatements_frames():
    from rpt_amd import ParticleState, Renderer, scenes
    pos, vel = pc.dropped_state()
    frames = _frames_reference(8)[:2]
    shown = [ref.display_positions(pc.R, pc.HEIGHT, pos)] + [f[2] for f in frames]

    def render(seq):
        seq = list(seq)
        scene, cam, cfg = scenes.marbles(shown[0])
        r = Renderer(scene, cam).width(64).height(48).max_bounces(cfg["max_bounces"]).seed(3).num_samples(4)
        return [np.array(f) for f in r.render_sequence([c for _, c in seq], batches=2, scenes=[s for s, _ in seq])]

    got = render(scenes.marbles_sequence(3, state=ParticleState(pos, vel)))
    exp = render([scenes.marbles(p)[:2] for p in shown])
    assert len(got) == 3 and all(np.array_equal(a, b) for a, b in zip(got, exp))
    assert got[0].shape == (48, 64, 3) and got[0].any()
