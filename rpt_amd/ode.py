"""The reference's src/ode/: ParticleState, the ParticleSystem trait's three systems and their RK4 integration, over the
rpt_particles_* entry points of include/rpt_hip.h, which states the arithmetic as an order of fp64 operations.  With a device the
integration runs in a HIP kernel (one workgroup, the time loop inside); `device=None` runs the same text serially on the host.
The two give the same bits.  ParticleEnsemble integrates many independent systems in one launch, a workgroup each."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import ParticlesParams, vp as _vp

CIRCLE, GRAVITY, MARBLES = 0, 1, 2


def _arr(a, n=None):
    a = np.ascontiguousarray(a, dtype=np.float64).reshape(-1, 3)
    if n is not None and len(a) != n:
        raise ValueError(f"expected {n} vectors, got {len(a)}")
    return a


class ParticleState:
    """Positions and velocities, n x 3 each (ode/particle_state.rs), with the reference's `+`, `* f64` and `/ f64`."""

    def __init__(self, pos, vel=None):
        self.pos = _arr(pos).copy()
        self.vel = np.zeros_like(self.pos) if vel is None else _arr(vel, len(self.pos)).copy()

    def __len__(self):
        return len(self.pos)

    def copy(self):
        return ParticleState(self.pos, self.vel)

    def __add__(self, other):
        return ParticleState(self.pos + other.pos, self.vel + other.vel)

    def __mul__(self, f):
        return ParticleState(self.pos * float(f), self.vel * float(f))

    def __truediv__(self, f):
        return ParticleState(self.pos / float(f), self.vel / float(f))


class ParticleSystem:
    """One of the library's three systems (a system of the caller's own integrates on the host: rpt.hpp's template)."""
    KIND = None
    radius = 0.0
    height = 0.0

    def params(self, n):
        return ParticlesParams(self.KIND, int(n), float(self.radius), float(self.height))

    def time_derivative(self, state):
        """The derivative of `state` as a ParticleState (a host function)."""
        out = ParticleState(np.zeros_like(state.pos))
        prm = self.params(len(state))
        _lib.check(_lib.load().rpt_particles_derivative_host(C.byref(prm), _vp(state.pos), _vp(state.vel), _vp(out.pos), _vp(out.vel), None))
        return out

    def rk4_integrate(self, state, time, step, device=0):
        """Advances `state` in place by `time` in steps of `step` (ParticleSystem::rk4_integrate) and returns it."""
        if device is None:
            prm = self.params(len(state))
            cnt = (C.c_uint64 * 8)()
            _lib.check(_lib.load().rpt_particles_integrate_host(C.byref(prm), _vp(state.pos), _vp(state.vel), float(time), float(step), cnt))
            return state
        sim = ParticleSimulator(self, state, device=device)
        try:
            sim.integrate(time, step)
            state.pos, state.vel = sim.state()
        finally:
            sim.close()
        return state


class SimpleCircleSystem(ParticleSystem):
    KIND = CIRCLE


class SolidGravitySystem(ParticleSystem):
    """Solid gravity objects in space."""
    KIND = GRAVITY


class MarblesSystem(ParticleSystem):
    """Marbles of one radius and the monomial glass y = height (x^2 + z^2)^2 on a table (the reference's height: 2)."""
    KIND = MARBLES

    def __init__(self, radius, height=2.0):
        self.radius = float(radius)
        self.height = float(height)

    def display_positions(self, pos):
        """Where marbles.rs:77-83 draws marbles at `pos` (a host function)."""
        pos = _arr(pos)
        out = np.zeros_like(pos)
        prm = self.params(len(pos))
        _lib.check(_lib.load().rpt_particles_display_positions_host(C.byref(prm), _vp(pos), _vp(out)))
        return out


class ParticleSimulator:
    """A system's state on a device (rpt_particles).  The calls of one simulator are ordered whatever their streams."""

    def __init__(self, system, state, device=0):
        self.system = system
        self.n = len(state)
        prm = system.params(self.n)
        self._h = _lib.load().rpt_particles_create(int(device), C.byref(prm))
        if not self._h:
            _lib.check(-1)
        self.set_state(state)

    def set_state(self, state):
        pos, vel = _arr(state.pos, self.n), _arr(state.vel, self.n)
        _lib.check(_lib.load().rpt_particles_set_state(self._h, _vp(pos), _vp(vel)))

    def state(self):
        """(pos, vel) as new arrays; synchronous."""
        pos, vel = np.zeros((self.n, 3)), np.zeros((self.n, 3))
        _lib.check(_lib.load().rpt_particles_state(self._h, _vp(pos), _vp(vel)))
        return pos, vel

    def state_device(self):
        """The device addresses of the simulator's own position and velocity arrays."""
        p, v = C.c_void_p(), C.c_void_p()
        _lib.check(_lib.load().rpt_particles_state_device(self._h, C.byref(p), C.byref(v)))
        return p.value, v.value

    def integrate(self, time, step, stream=None):
        """Asynchronous, on `stream` (a hipStream_t as an integer; None: the default stream)."""
        _lib.check(_lib.load().rpt_particles_integrate(self._h, float(time), float(step), C.c_void_p(stream)))

    def display_positions(self):
        out = np.zeros((self.n, 3))
        _lib.check(_lib.load().rpt_particles_display_positions(self._h, _vp(out)))
        return out

    def display_positions_device(self, stream=None):
        """The display positions left in the simulator's own device array: its address (n x 3 doubles, valid until close()).
        Asynchronous on `stream`, ordered like integrate."""
        d = C.c_void_p()
        _lib.check(_lib.load().rpt_particles_display_positions_device(self._h, C.byref(d), C.c_void_p(stream)))
        return d.value

    def counters(self):
        """Derivative evaluations, pair contacts, surface band / push, table band / push, launches, 0."""
        out = (C.c_uint64 * 8)()
        _lib.check(_lib.load().rpt_particles_counters(self._h, out))
        return [int(x) for x in out]

    def close(self):
        if self._h:
            _lib.load().rpt_particles_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ParticleEnsemble:
    """Many independent systems on a device, integrated in one launch, one workgroup each (rpt_particles_batch).  `systems` and
    `states` are lists of equal length: system i (a MarblesSystem, SolidGravitySystem or SimpleCircleSystem, of any size and
    parameters) with its ParticleState.  Every system comes out with the bits it would have alone; the calls of one ensemble are
    ordered whatever their streams."""

    def __init__(self, systems, states, device=0):
        systems, states = list(systems), list(states)
        if len(systems) != len(states):
            raise ValueError(f"{len(systems)} systems but {len(states)} states")
        self.systems = systems
        self.sizes = [len(s) for s in states]
        self.first = np.concatenate([[0], np.cumsum(self.sizes)]).astype(np.int64)
        prm = (ParticlesParams * max(1, len(systems)))(*[sy.params(n) for sy, n in zip(systems, self.sizes)])
        self._h = _lib.load().rpt_particles_batch_create(int(device), prm, len(systems))
        if not self._h:
            _lib.check(-1)
        pos = np.concatenate([_arr(s.pos) for s in states])
        vel = np.concatenate([_arr(s.vel) for s in states])
        _lib.check(_lib.load().rpt_particles_batch_set_state(self._h, _vp(pos), _vp(vel)))

    def __len__(self):
        return len(self.sizes)

    def _split(self, a):
        return [a[self.first[i]:self.first[i + 1]].copy() for i in range(len(self.sizes))]

    def set_state(self, i, state):
        """Replaces system i's state (ordered behind what the ensemble has queued)."""
        if not 0 <= i < len(self.sizes):
            raise IndexError(f"system {i} of {len(self.sizes)}")
        pos, vel = _arr(state.pos, self.sizes[i]), _arr(state.vel, self.sizes[i])
        _lib.check(_lib.load().rpt_particles_batch_set_system_state(self._h, int(i), _vp(pos), _vp(vel)))

    def states(self):
        """A list of ParticleState, one per system; synchronous."""
        total = int(self.first[-1])
        pos, vel = np.zeros((total, 3)), np.zeros((total, 3))
        _lib.check(_lib.load().rpt_particles_batch_state(self._h, _vp(pos), _vp(vel)))
        return [ParticleState(p, v) for p, v in zip(self._split(pos), self._split(vel))]

    def state_device(self):
        """The device addresses of the concatenated position and velocity arrays and of the uint32 first-particle indices."""
        p, v, f = C.c_void_p(), C.c_void_p(), C.c_void_p()
        _lib.check(_lib.load().rpt_particles_batch_state_device(self._h, C.byref(p), C.byref(v), C.byref(f)))
        return p.value, v.value, f.value

    def integrate(self, time, step, stream=None):
        """Advances every system by `time` in steps of `step`.  Asynchronous, on `stream` (a hipStream_t as an integer; None: the
        default stream)."""
        _lib.check(_lib.load().rpt_particles_batch_integrate(self._h, float(time), float(step), C.c_void_p(stream)))

    def display_positions(self):
        """A list of (n_i, 3) arrays: where marbles.rs draws each system's marbles (every system a MarblesSystem)."""
        out = np.zeros((int(self.first[-1]), 3))
        _lib.check(_lib.load().rpt_particles_batch_display_positions(self._h, _vp(out)))
        return self._split(out)

    def display_positions_device(self, stream=None):
        """Every system's display positions left in the ensemble's own device array, the systems concatenated: its address
        (sum(n) x 3 doubles, valid until close()).  Asynchronous on `stream`, ordered like integrate."""
        d = C.c_void_p()
        _lib.check(_lib.load().rpt_particles_batch_display_positions_device(self._h, C.byref(d), C.c_void_p(stream)))
        return d.value

    def counters(self):
        """One list of eight per system: ParticleSimulator.counters' slots, launches counted for the ensemble."""
        out = (C.c_uint64 * (8 * len(self.sizes)))()
        _lib.check(_lib.load().rpt_particles_batch_counters(self._h, out))
        return [[int(x) for x in out[8 * i:8 * i + 8]] for i in range(len(self.sizes))]

    def info(self):
        """Resident blocks R, rounds, steps per launch, dynamic LDS bytes per block, the largest n, the number of particles, and the
        tuning (threads per block, lanes per particle)."""
        out = (C.c_uint64 * 8)()
        _lib.check(_lib.load().rpt_particles_batch_info(self._h, out))
        keys = ("resident_blocks", "rounds", "launch_steps", "lds_bytes", "n_max", "particles", "block", "lanes")
        return dict(zip(keys, (int(x) for x in out)))

    def close(self):
        if self._h:
            _lib.load().rpt_particles_batch_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
