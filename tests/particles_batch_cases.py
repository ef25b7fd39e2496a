"""States for the ensemble tests (tests/test_gpu_particles_batch.py): batches put together from tests/particles_cases.py's states, and
what each system of a batch must come out as -- the numpy restatement (tests/particles_ref.py) for a few steps of small systems,
rpt_particles_integrate_host (the same text, compiled) where numpy would take too long."""
import ctypes as C

import numpy as np

from rpt_amd import _lib
from rpt_amd._lib import ParticlesParams, vp

from . import particles_cases as pc
from . import particles_ref as ref

STEP = 1.0 / 10000.0


def time_of(steps):
    """A time just short of steps * STEP: the loop's last step is the remainder, `steps` steps in all."""
    time = steps * STEP * (1.0 - 2.0 ** -30)
    assert ref.step_sequence(time, STEP)[0] + 1 == steps
    return time


def system(kind, pos, vel, radius=pc.R, height=pc.HEIGHT):
    return (kind, np.ascontiguousarray(pos, dtype=np.float64), np.ascontiguousarray(vel, dtype=np.float64), radius, height)


def mixed_three():
    """MARBLES n = 25, GRAVITY n = 7, CIRCLE n = 3: the particle offsets 0, 25, 32 are multiples of nothing."""
    return [system(ref.MARBLES, *pc.touching_state()), system(ref.GRAVITY, *pc.random_state(7, 21)), system(ref.CIRCLE, *pc.random_state(3, 22))]


def sizes(ns, seed=40):
    """MARBLES systems of the given sizes, with heights and radii of their own."""
    return [system(ref.MARBLES, *pc.random_state(n, seed + n), radius=0.15 - 0.01 * (i % 3), height=2.0 + 0.25 * (i % 2)) for i, n in enumerate(ns)]


def families():
    return [system(ref.MARBLES, pos, vel) for _, pos, vel in pc.family_states()]


def many_small(count=1025, kinds=(ref.MARBLES,), seed=7):
    """`count` systems of n = 2 or 3 (alternating), random states."""
    rng = np.random.default_rng(seed)
    out = []
    for s in range(count):
        n = 2 + s % 2
        pos = rng.uniform([-0.4, 0.0, -0.4], [0.4, 0.8, 0.4], (n, 3))
        out.append(system(kinds[s % len(kinds)], pos, rng.uniform(-1.0, 1.0, (n, 3))))
    return out


def heavy(count=40):
    """`count` MARBLES systems of n = 256, every one with a state of its own."""
    return [system(ref.MARBLES, *pc.random_state(256, 60 + s)) for s in range(count)]


def by_restatement(systems, time):
    """[(pos, vel, counters[6])] from tests/particles_ref.py, one system at a time."""
    out = []
    for kind, pos, vel, radius, height in systems:
        p, v, c = ref.rk4_integrate(kind, radius, height, pos, vel, time, STEP)
        out.append((p, v, [int(x) for x in c]))
    return out


def by_host_function(systems, time):
    """[(pos, vel, counters[6])] from rpt_particles_integrate_host on each system alone; equal systems are computed once."""
    lib = _lib.load()
    done, out = {}, []
    for kind, pos, vel, radius, height in systems:
        key = (kind, pos.tobytes(), vel.tobytes(), radius, height)
        if key not in done:
            p, v, c = pos.copy(), vel.copy(), (C.c_uint64 * 8)()
            prm = ParticlesParams(kind, len(pos), radius, height)
            assert lib.rpt_particles_integrate_host(C.byref(prm), vp(p), vp(v), time, STEP, c) == 0
            done[key] = (p, v, [int(x) for x in c][:6])
        out.append(done[key])
    return out
