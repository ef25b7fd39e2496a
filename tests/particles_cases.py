"""Hand-made marble states (r = 0.15, height = 2) for the particle tests, each with the branches it claims to take; the claim is
asserted from the restatement's masks by tests/test_particles_host.py (no GPU), so the GPU tests run states that are known to reach
the code they are meant for."""
import numpy as np

from . import particles_ref as ref

R, HEIGHT = 0.15, 2.0

# name -> (positions, the set of masks that fire for some particle: contact, surface_band, surface_push, table_band, table_push)
FAMILIES = {
    "free_fall": ([[0.3, 5.0, 0.2]], set()),
    "pair_contact": ([[0.5, 5.0, 0.0], [0.7, 5.0, 0.0]], {"contact"}),
    "surface_band": ([[0.5, 0.395, 0.0]], {"surface_band"}),
    "surface_push": ([[0.5, 0.2, 0.0]], {"surface_push"}),
    "table_band": ([[3.0, 0.1, 0.0]], {"table_band"}),
    "table_push": ([[3.0, 0.05, 0.0]], {"table_push"}),
    "inside": ([[0.05, 0.05, 0.0]], {"surface_push"}),                 # length <= 0.1: the table term is off
    "axis": ([[0.0, 3.0, 0.0]], set()),                                # NaN closest point, no surface force
    "origin": ([[0.0, 0.0, 0.0]], {"surface_push"}),                   # closest = the point, L = 0, ratio = 1, NaN normal
    "coincident": ([[0.4, 5.0, 0.1], [0.4, 5.0, 0.1]], {"contact"}),   # NaN
    "every_term": ([[0.5, 0.1, 0.0], [0.7, 0.1, 0.0]], {"contact", "surface_push", "table_band"}),
}
MASKS = ("contact", "surface_band", "surface_push", "table_band", "table_push")


def velocities(n, seed=7):
    return np.random.default_rng(seed).uniform(-0.5, 0.5, (n, 3))


def family_states():
    """(name, pos, vel): every family at rest and moving."""
    out = []
    for name, (pos, _) in FAMILIES.items():
        pos = np.array(pos, dtype=np.float64)
        out.append((name + "-rest", pos, np.zeros_like(pos)))
        out.append((name + "-moving", pos, velocities(len(pos))))
    return out


def random_state(n, seed):
    """Marbles thrown into the glass's neighbourhood, close enough together that some touch."""
    rng = np.random.default_rng(seed)
    side = max(0.4, 0.22 * n ** (1.0 / 3.0))
    pos = rng.uniform([-side, 0.0, -side], [side, 2.0 * side, side], (n, 3))
    return pos, rng.uniform(-1.0, 1.0, (n, 3))


def touching_state():
    """25 marbles: twenty in the glass on marbles.rs's grid (0.2 apart: neighbours overlap), five in a row on the table."""
    rng = np.random.default_rng(11)
    pos = [[(i // 5) / 5.0 - 0.375, 0.12 + 0.1 * (i % 4) + 0.05 * rng.random(), (i % 5) / 5.0 - 0.375] for i in range(20)]
    pos += [[1.3 + 0.25 * k, 0.085 + 0.01 * k, 0.3] for k in range(5)]
    return np.array(pos), rng.uniform(-0.2, 0.2, (25, 3))


def dropped_state(n=25, seed=123):
    """The start of the sequence, lowered so that the marbles reach the glass within a few frames."""
    rng = np.random.default_rng(seed)
    pos = [[(i // 5) / 5.0 - 0.375, 0.6 + 0.5 * rng.random(), (i % 5) / 5.0 - 0.375] for i in range(n)]
    return np.array(pos), np.zeros((n, 3))


_cache = {}


def cached(key, fn):
    """One reference per session and key, shared by the tests that need it."""
    if key not in _cache:
        _cache[key] = fn()
    return _cache[key]


def full_frame_reference():
    pos, vel = touching_state()
    return cached("full_frame", lambda: ref.rk4_integrate(ref.MARBLES, R, HEIGHT, pos, vel, 1.0 / 16.0, 1.0 / 10000.0))
