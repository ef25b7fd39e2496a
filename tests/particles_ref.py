"""The particle systems of include/rpt_hip.h ("particle systems": closest_point*, the three systems' derivatives, rk4_integrate, the
display positions) twice over:

  * restated in numpy -- one array operation per rounded fp64 operation of the header, in its order, vectorised over particles and
    candidates; the partner loop stays a loop, since its order IS the definition.  Returns the six counters and, per derivative
    evaluation, the branch masks;
  * transcribed into plain Python floats line by line after the reference's Rust (loops over i, j < i and the candidates), with the
    header's one stated departure (sqrt(x x + z z) for f64::hypot).

numpy never contracts a product into a sum, and Python's float is the IEEE double, so both are exact statements of the header."""
import math

import numpy as np

CIRCLE, GRAVITY, MARBLES = 0, 1, 2
NO_WIN = 1e18


def bits(a):
    """The values as bit patterns, every NaN as one pattern: equal bits <=> equal finite values and NaNs in the same places."""
    a = np.ascontiguousarray(a, dtype=np.float64)
    return np.where(np.isnan(a), np.uint64(0x7FF8000000000000), a.view(np.uint64))


def length(v):
    return np.sqrt((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2])


def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def step_sequence(time, step):
    """(number of steps of `step`, the last step)."""
    t, c = float(time), 0
    while t > step:
        t = t - step
        c += 1
    return c, t


def closest_point(height, P, precise=False):
    P = np.asarray(P, dtype=np.float64).reshape(-1, 3)
    n = 10000 if precise else 100
    with np.errstate(all="ignore"):
        trivial = length(P) < 1e-12
        px = np.sqrt(P[:, 0] * P[:, 0] + P[:, 2] * P[:, 2])
        py = P[:, 1]
        xf = np.arange(-n, n + 1).astype(np.float64) / float(n)
        yc = height * ((xf * xf) * (xf * xf))
        a = px[:, None] - xf[None, :]
        b = py[:, None] - yc[None, :]
        d = a * a + b * b
        valid = d < NO_WIN
        w = np.argmin(np.where(valid, d, np.inf), axis=1)        # the first of the smallest: the strict scan's winner
        win = np.where(valid.any(axis=1), xf[w], -1.0)
        ux = P[:, 0] / px
        uz = P[:, 2] / px
        X = win * ux
        Z = win * uz
        s = X * X + Z * Z
        out = np.stack([X, height * (s * s), Z], axis=1)
    return np.where(trivial[:, None], P, out)


def _pairs(pos):
    """d[p, q], len[p, q], below[p, q] (q < p), other[p, q] (q != p)."""
    n = len(pos)
    idx = np.arange(n)
    below = idx[None, :] < idx[:, None]
    other = idx[None, :] != idx[:, None]
    d = np.where(below[:, :, None], pos[:, None, :] - pos[None, :, :], pos[None, :, :] - pos[:, None, :])
    return d, length(d), below, other


def derivative(kind, radius, height, pos, vel):
    """((dpos, dvel), counters[6], masks)."""
    pos = np.asarray(pos, dtype=np.float64).reshape(-1, 3)
    vel = np.asarray(vel, dtype=np.float64).reshape(-1, 3)
    n = len(pos)
    cnt = np.zeros(6, dtype=np.uint64)
    cnt[0] = 1
    masks = {}
    with np.errstate(all="ignore"):
        if kind == CIRCLE:
            dpos = np.stack([-pos[:, 1], pos[:, 0], np.zeros(n)], axis=1)
            return (dpos, np.zeros((n, 3))), cnt, masks
        d, ln, below, other = _pairs(pos)
        direction = d / ln[:, :, None]
        if kind == GRAVITY:
            s = 1.0 / (ln * ln) - 0.0001 * (1.0 / (ln * ((ln * ln) * (ln * ln))))
            f = direction * s[:, :, None]
            acc = np.zeros((n, 3))
            for q in range(n):
                acc = np.where(other[:, q, None], np.where(below[:, q, None], acc - f[:, q], acc + f[:, q]), acc)
            return (vel.copy(), acc), cnt, masks
        r = float(radius)
        two_r = 2.0 * r
        contact = (ln < two_r) & other
        c = (two_r - ln) / r
        f = ((-direction) * 5.0) * c[:, :, None]
        damp = vel * 0.5
        acc = np.tile(np.array([0.0, -1.0, 0.0]), (n, 1))
        for q in range(n):
            t = np.where(below[:, q, None], acc - f[:, q], acc + f[:, q])
            t = t - damp
            acc = np.where(contact[:, q, None], t, acc)
        masks["contact"] = contact
        cnt[1] = np.count_nonzero(contact & below)
        # surface
        C = closest_point(height, pos)
        v = pos - C
        L = length(v)
        nrm = v / L[:, None]
        ratio = (r - L) / r
        nv = dot(vel, nrm)
        band = (-0.1 < ratio) & (ratio < 0.0)
        push = ~band & (ratio >= 0.0)
        acc = np.where(band[:, None], acc - (30.0 * nrm) * ((nv * nv) * nv)[:, None], acc)
        acc = np.where(push[:, None], acc + (100.0 * nrm) * ratio[:, None], acc)
        masks["surface_band"], masks["surface_push"], masks["closest"] = band, push, C
        # table
        tn = np.array([0.0, 1.0, 0.0])
        tr = ((r - 0.06) - pos[:, 1]) / r
        tv = (vel[:, 0] * 0.0 + vel[:, 1] * 1.0) + vel[:, 2] * 0.0
        on = length(pos) > 0.1
        tband = on & (-0.1 < tr) & (tr < 0.0)
        tpush = on & ~tband & (tr >= 0.0)
        acc = np.where(tband[:, None], acc - (20.0 * tn)[None, :] * tv[:, None], acc)
        acc = np.where(tpush[:, None], acc + (300000.0 * tn)[None, :] * tr[:, None], acc)
        masks["table_band"], masks["table_push"] = tband, tpush
        # air
        acc = acc - vel / 5.0
        cnt[2:6] = [np.count_nonzero(m) for m in (band, push, tband, tpush)]
    return (vel.copy(), acc), cnt, masks


def rk4_steps(kind, radius, height, pos, vel, steps):
    """The given sequence of step sizes.  -> (pos, vel, counters[6])."""
    pos = np.array(pos, dtype=np.float64).reshape(-1, 3)
    vel = np.array(vel, dtype=np.float64).reshape(-1, 3)
    cnt = np.zeros(6, dtype=np.uint64)

    def f(p, v):
        nonlocal cnt
        k, c, _ = derivative(kind, radius, height, p, v)
        cnt = cnt + c
        return k

    with np.errstate(all="ignore"):
        for h in steps:
            hh = h / 2.0
            k1 = f(pos, vel)
            k2 = f(pos + k1[0] * hh, vel + k1[1] * hh)
            k3 = f(pos + k2[0] * hh, vel + k2[1] * hh)
            k4 = f(pos + k3[0] * h, vel + k3[1] * h)
            h6 = h / 6.0
            pos = pos + (((k1[0] + k2[0] * 2.0) + k3[0] * 2.0) + k4[0]) * h6
            vel = vel + (((k1[1] + k2[1] * 2.0) + k3[1] * 2.0) + k4[1]) * h6
    return pos, vel, cnt


def rk4_integrate(kind, radius, height, pos, vel, time, step):
    c, last = step_sequence(time, step)
    return rk4_steps(kind, radius, height, pos, vel, [step] * c + [last])


def display_positions(radius, height, pos):
    pos = np.asarray(pos, dtype=np.float64).reshape(-1, 3)
    with np.errstate(all="ignore"):
        C = closest_point(height, pos, precise=True)
        v = pos - C
        ln = length(v)
        moved = C + ((v / ln[:, None]) * radius) * 1.05
        out = np.where((ln < radius * 1.05)[:, None], moved, pos)
        lo = radius - 0.06
        y = out[:, 1]
        out[:, 1] = np.where(np.isnan(y), lo, np.where(y >= lo, y, lo))
    return out


# ------------------------------------------------------------------------------------------------ the transcription
def _sub(a, b):
    return [a[0] - b[0], a[1] - b[1], a[2] - b[2]]


def _len(v):
    return math.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _div(a, b):
    """IEEE division (Python raises where IEEE answers)."""
    try:
        return a / b
    except ZeroDivisionError:
        if a != a or a == 0.0:
            return math.nan
        return math.copysign(math.inf, a) * math.copysign(1.0, b)


def _normalize(v):
    ln = _len(v)
    return [_div(v[0], ln), _div(v[1], ln), _div(v[2], ln)]


def t_closest_point(height, point, n=100):
    if _len(point) < 1e-12:
        return list(point)
    px = math.sqrt(point[0] * point[0] + point[2] * point[2])
    py = point[1]
    res = (1e18, -1.0)
    for x in range(-n, n + 1):
        xf = x / float(n)
        yc = height * ((xf * xf) * (xf * xf))
        dist2 = (px - xf) * (px - xf) + (py - yc) * (py - yc)
        if dist2 < res[0]:
            res = (dist2, xf)
    ux, uz = _div(point[0], px), _div(point[2], px)
    xz = (res[1] * ux, res[1] * uz)
    s = xz[0] * xz[0] + xz[1] * xz[1]
    return [xz[0], height * (s * s), xz[1]]


def t_derivative(kind, radius, height, pos, vel):
    """-> (dpos, dvel, counters[6]) as lists."""
    n = len(pos)
    cnt = [1, 0, 0, 0, 0, 0]
    if kind == CIRCLE:
        return [[-p[1], p[0], 0.0] for p in pos], [[0.0, 0.0, 0.0] for _ in pos], cnt
    if kind == GRAVITY:
        acc = [[0.0, 0.0, 0.0] for _ in range(n)]
        for i in range(n):
            for j in range(i):
                d = _sub(pos[i], pos[j])
                direction = _normalize(d)
                ln = _len(d)
                s = _div(1.0, ln * ln) - 0.0001 * _div(1.0, ln * ((ln * ln) * (ln * ln)))
                force = [direction[k] * s for k in range(3)]
                for k in range(3):
                    acc[j][k] = acc[j][k] + force[k]
                    acc[i][k] = acc[i][k] - force[k]
        return [list(v) for v in vel], acc, cnt
    r = radius
    acc = [[0.0, -1.0, 0.0] for _ in range(n)]
    for i in range(n):
        for j in range(i):
            d = _sub(pos[i], pos[j])
            direction = _normalize(d)
            ln = _len(d)
            if ln < 2.0 * r:
                c = _div(2.0 * r - ln, r)
                force = [((-direction[k]) * 5.0) * c for k in range(3)]
                cnt[1] += 1
                for k in range(3):
                    acc[j][k] = acc[j][k] + force[k]
                    acc[j][k] = acc[j][k] - vel[j][k] * 0.5
                    acc[i][k] = acc[i][k] - force[k]
                    acc[i][k] = acc[i][k] - vel[i][k] * 0.5
    for i in range(n):
        closest = t_closest_point(height, pos[i])
        vec = _sub(pos[i], closest)
        normal = _normalize(vec)
        ratio = _div(r - _len(vec), r)
        nv = _dot(vel[i], normal)
        if -0.1 < ratio and ratio < 0.0:
            for k in range(3):
                acc[i][k] = acc[i][k] - (30.0 * normal[k]) * ((nv * nv) * nv)
            cnt[2] += 1
        elif ratio >= 0.0:
            for k in range(3):
                acc[i][k] = acc[i][k] + (100.0 * normal[k]) * ratio
            cnt[3] += 1
    for i in range(n):
        normal = [0.0, 1.0, 0.0]
        ratio = _div((r - 0.06) - pos[i][1], r)
        nv = (vel[i][0] * 0.0 + vel[i][1] * 1.0) + vel[i][2] * 0.0
        if _len(pos[i]) > 0.1:
            if -0.1 < ratio and ratio < 0.0:
                for k in range(3):
                    acc[i][k] = acc[i][k] - (20.0 * normal[k]) * nv
                cnt[4] += 1
            elif ratio >= 0.0:
                for k in range(3):
                    acc[i][k] = acc[i][k] + (300000.0 * normal[k]) * ratio
                cnt[5] += 1
    for i in range(n):
        for k in range(3):
            acc[i][k] = acc[i][k] - vel[i][k] / 5.0
    return [list(v) for v in vel], acc, cnt


def t_rk4_integrate(kind, radius, height, pos, vel, time, step):
    """-> (pos, vel, counters[6]) as numpy arrays."""
    pos = [[float(x) for x in p] for p in np.asarray(pos, dtype=np.float64).reshape(-1, 3)]
    vel = [[float(x) for x in p] for p in np.asarray(vel, dtype=np.float64).reshape(-1, 3)]
    n = len(pos)
    cnt = [0] * 6

    def f(p, v):
        dp, dv, c = t_derivative(kind, radius, height, p, v)
        for k in range(6):
            cnt[k] += c[k]
        return dp, dv

    def axpy(s, k, a):
        return [[s[i][c] + k[i][c] * a for c in range(3)] for i in range(n)]

    def one(h):
        nonlocal pos, vel
        k1 = f(pos, vel)
        k2 = f(axpy(pos, k1[0], h / 2.0), axpy(vel, k1[1], h / 2.0))
        k3 = f(axpy(pos, k2[0], h / 2.0), axpy(vel, k2[1], h / 2.0))
        k4 = f(axpy(pos, k3[0], h), axpy(vel, k3[1], h))
        new = []
        for s, w in ((pos, 0), (vel, 1)):
            new.append([[s[i][c] + (((k1[w][i][c] + k2[w][i][c] * 2.0) + k3[w][i][c] * 2.0) + k4[w][i][c]) * (h / 6.0) for c in range(3)]
                        for i in range(n)])
        pos, vel = new

    t = float(time)
    while t > step:
        one(step)
        t -= step
    one(t)
    return np.array(pos).reshape(-1, 3), np.array(vel).reshape(-1, 3), np.array(cnt, dtype=np.uint64)
