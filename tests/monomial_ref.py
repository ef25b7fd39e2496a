"""fp64 restatement of the reference's MonomialSurface::intersect (src/shape/monomial_surface.rs:22-107), written for the
tests: numpy float64 arithmetic is IEEE with no fused multiply-adds, and every expression below keeps the cited line's operation
order, so on the same local ray it gives the reference's bits.  Vectorised over rays (each element follows its own path).

  * `intersect_local` -- one surface in its own space, against a record time per ray (+inf: the empty record);
  * `intersect_world` -- the same under Transformed<T> (src/shape.rs:128-138): the ray mapped by M^-1 (not renormalised, so t
    is shared), the normal mapped by normalize(M^-T n);
  * `sphere_world` -- Sphere::intersect (src/shape/sphere.rs:14-46) under Transformed<T>, for scenes that put other objects
    into or in front of a surface;
  * `closest_hit` -- Renderer::get_closest_hit (src/renderer.rs:416-425) over a list of such shapes, in scene order.
"""
import numpy as np


def _box(o, d, height):
    # BoundingBox::intersect (src/kdtree.rs:56-71) of p_min = (-1, 0, -1), p_max = (1, height, 1) (monomial_surface.rs:181-187);
    # f64::min / f64::max return the other operand of a NaN, as np.fmin / np.fmax do
    lo, hi = (-1.0, 0.0, -1.0), (1.0, height, 1.0)
    a, b = [], []
    for k in range(3):
        t1 = (lo[k] - o[:, k]) / d[:, k]
        t2 = (hi[k] - o[:, k]) / d[:, k]
        a.append(np.fmin(t1, t2))
        b.append(np.fmax(t1, t2))
    return np.fmax(np.fmax(a[0], a[1]), a[2]), np.fmin(np.fmin(b[0], b[1]), b[2])


def intersect_local(o, d, height, t_min, rec_time=None):
    """-> (hit, t, normal): whether the surface replaces a record of time `rec_time` (default +inf), and what it writes."""
    o = np.asarray(o, dtype=np.float64).reshape(-1, 3)
    d = np.asarray(d, dtype=np.float64).reshape(-1, 3)
    n = o.shape[0]
    rec = np.full(n, np.inf) if rec_time is None else np.asarray(rec_time, dtype=np.float64)
    h = float(height)
    with np.errstate(all="ignore"):
        b_min, b_max = _box(o, d, h)
        ok = ~(np.fmax(b_min, t_min) > np.fmin(b_max, rec))                                   # :23-26

        def dist(t):                                                                          # :27-32
            x = o[:, 0] + t * d[:, 0]
            y = o[:, 1] + t * d[:, 1]
            z = o[:, 2] + t * d[:, 2]
            s = x * x + z * z
            return y - h * (s * s)

        c0 = o[:, 0] * o[:, 0] + o[:, 2] * o[:, 2]                                             # :33-35
        c1 = 2. * (o[:, 0] * d[:, 0] + o[:, 2] * d[:, 2])
        c2 = d[:, 0] * d[:, 0] + d[:, 2] * d[:, 2]

        def deriv(t):                                                                         # :36-42
            dy = 2. * c0 * c1 + 2. * t * (c1 * c1 + 2. * c0 * c2) + 3. * (t * t) * 2. * c1 * c2 + 4. * (t * t * t) * c2 * c2
            return d[:, 1] - h * dy

        def deriv2(t):                                                                        # :43-48
            dy = 2. * (c1 * c1 + 2. * c0 * c2) + 3. * 2. * t * 2. * c1 * c2 + 4. * 3. * (t * t) * c2 * c2
            return -h * dy

        tmin = np.full(n, float(t_min))
        maximize = dist(tmin) < 0.0                                                           # :50
        cur = (b_min + b_max) / 2.                                                            # :52-61
        going = maximize.copy()
        for _ in range(10):
            going &= ~(dist(cur) > 0.)
            step = deriv(cur) / deriv2(cur)
            cur = np.where(going, cur - step, cur)
        t_max = np.where(maximize, cur, 10000.)                                               # :65-71
        ok &= ~(maximize & (t_max < tmin))
        ok &= (dist(tmin) < 0.0) != (dist(t_max) < 0.0)                                       # :72-74
        l, r = tmin.copy(), t_max.copy()
        for _ in range(60):                                                                   # :75-84
            m = (l + r) / 2.0
            up = (dist(m) >= 0.0) == maximize
            r = np.where(up, m, r)
            l = np.where(up, l, m)
        ok &= ~(r > rec)                                                                      # :85-87
        px, py, pz = o[:, 0] + r * d[:, 0], o[:, 1] + r * d[:, 1], o[:, 2] + r * d[:, 2]      # Ray::at, src/shape.rs:60-62
        ok &= ~(px * px + pz * pz > 1.0)                                                      # :88-92
        s = px * px + pz * pz                                                                 # :95-99
        nv = np.stack([h * 4.0 * px * s, np.full(n, -1.0), h * 4.0 * pz * s], axis=1)
        nv = _normalize(nv)
        flip = (nv[:, 0] * d[:, 0] + nv[:, 1] * d[:, 1] + nv[:, 2] * d[:, 2]) > 0.0         # :101-104
        nv = np.where(flip[:, None], -nv, nv)
    del py
    return ok, r, nv


def _normalize(v):
    ln = np.sqrt(v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2])
    return v / ln[:, None]


def inverse_rows(m):
    """M^-1 of a 4x4 transform.  The tests that compare bits use matrices whose inverse is exact (translations, power-of-two
    scales): this one is exact for them."""
    return np.linalg.inv(np.asarray(m, dtype=np.float64))


def intersect_world(o, d, height, t_min, m=None, rec_time=None):
    """Transformed<MonomialSurface> (src/shape.rs:128-138); m = None: the bare surface."""
    o = np.asarray(o, dtype=np.float64).reshape(-1, 3)
    d = np.asarray(d, dtype=np.float64).reshape(-1, 3)
    if m is None:
        return intersect_local(o, d, height, t_min, rec_time)
    inv = inverse_rows(m)
    with np.errstate(all="ignore"):
        ol = np.stack([inv[i, 0] * o[:, 0] + inv[i, 1] * o[:, 1] + inv[i, 2] * o[:, 2] + inv[i, 3] for i in range(3)], axis=1)
        dl = np.stack([inv[i, 0] * d[:, 0] + inv[i, 1] * d[:, 1] + inv[i, 2] * d[:, 2] for i in range(3)], axis=1)
        ok, t, nl = intersect_local(ol, dl, height, t_min, rec_time)
        nt = inv[:3, :3].T   # normal_transform = (linear part)^-T = (M^-1 linear part)^T
        nw = np.stack([nt[i, 0] * nl[:, 0] + nt[i, 1] * nl[:, 1] + nt[i, 2] * nl[:, 2] for i in range(3)], axis=1)
        nw = _normalize(nw)
    return ok, t, nw


def sphere_world(o, d, t_min, m=None, rec_time=None):
    """Sphere::intersect (src/shape/sphere.rs:14-46, the unit sphere) under Transformed<T> -> (hit, t, normal), same conventions as
    intersect_world."""
    o = np.asarray(o, dtype=np.float64).reshape(-1, 3)
    d = np.asarray(d, dtype=np.float64).reshape(-1, 3)
    n = o.shape[0]
    rec = np.full(n, np.inf) if rec_time is None else np.asarray(rec_time, dtype=np.float64)
    inv = np.eye(4) if m is None else inverse_rows(m)
    with np.errstate(all="ignore"):
        if m is None:
            ol, dl = o, d
        else:
            ol = np.stack([inv[i, 0] * o[:, 0] + inv[i, 1] * o[:, 1] + inv[i, 2] * o[:, 2] + inv[i, 3] for i in range(3)], axis=1)
            dl = np.stack([inv[i, 0] * d[:, 0] + inv[i, 1] * d[:, 1] + inv[i, 2] * d[:, 2] for i in range(3)], axis=1)
        a = dl[:, 0] * dl[:, 0] + dl[:, 1] * dl[:, 1] + dl[:, 2] * dl[:, 2]          # :16-18
        b = dl[:, 0] * ol[:, 0] + dl[:, 1] * ol[:, 1] + dl[:, 2] * ol[:, 2]
        c = (ol[:, 0] * ol[:, 0] + ol[:, 1] * ol[:, 1] + ol[:, 2] * ol[:, 2]) - 1.0
        disc = b * b - a * c                                                          # :20-23
        ok = ~np.signbit(disc)
        sq = np.sqrt(disc)
        t_minus = (-b - sq) / a                                                       # :25-36
        t_plus = (-b + sq) / a
        t = np.where(t_minus < t_min, t_plus, t_minus)
        ok &= ~(t < t_min)
        ok &= t < rec                                                                 # :39
        nl = _normalize(ol + t[:, None] * dl)                                         # :41, Ray::at
        if m is not None:
            nt = inv[:3, :3].T
            nl = _normalize(np.stack([nt[i, 0] * nl[:, 0] + nt[i, 1] * nl[:, 1] + nt[i, 2] * nl[:, 2] for i in range(3)], axis=1))
    return ok, t, nl


def closest_hit(o, d, surfaces, t_min=1e-12):
    """Renderer::get_closest_hit over `surfaces` in scene order: (height, matrix or None) for a monomial surface, ("sphere",
    matrix or None) for a sphere.  Each one replaces the record when its own test says so (for a monomial surface an equal or
    NaN time included).  -> (t, object index or -1, normal)."""
    o = np.asarray(o, dtype=np.float64).reshape(-1, 3)
    n = o.shape[0]
    t = np.full(n, np.inf)
    obj = np.full(n, -1, dtype=np.int32)
    nrm = np.zeros((n, 3))
    for k, (height, m) in enumerate(surfaces):
        if isinstance(height, str):
            ok, tk, nk = sphere_world(o, d, t_min, m, rec_time=t)
        else:
            ok, tk, nk = intersect_world(o, d, height, t_min, m, rec_time=t)
        t = np.where(ok, tk, t)
        obj = np.where(ok, k, obj)
        nrm = np.where(ok[:, None], nk, nrm)
    return t, obj, nrm
