"""The moving-object part of the temporal accumulation of include/rpt_hip.h restated in numpy, next to tests/temporal_ref.py:
motion_record is rpt_temporal_motion_record in the header's order of fp64 operations (Python floats: IEEE, each operation rounded on
its own), MotionRef is TemporalRef.accumulate with `motion=`, an (m, 24) table or None.  The kernel's output is compared with
MotionRef bit for bit (tests/test_gpu_temporal_motion.py); MotionRef is compared with TemporalRef and with a pixel-by-pixel
transcription of the header text (tests/test_temporal_motion_host.py).

The moving analytic scene: the wall z = 0 (id 1) and a sphere (id 2) with object-to-world M_f = T((0, 0, 1) + f (0.25, 0.1, 0.1)) .
R_y(spin f) . S(0.7), seen through pixel centres as temporal_ref.analytic_planes sees its scene; the radiance is a "paint" fixed in the
sphere's own coordinates, 0.5 + 0.5 x (the hit point in the unit sphere's coordinates), and 0.3 on the wall: history taken from another
material point shows as a colour error."""
import math

import numpy as np

from tests.temporal_ref import MATCH_ID, TemporalRef, pixel_rays

MOTION_DOUBLES = 24
IDENTITY_RECORD = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], dtype=np.float64)


def _cofactors(m):
    """The header's nine cofactors k (inverse = k / det) and the determinant of a 3 x 3 list of Python floats."""
    k = [[m[1][1] * m[2][2] - m[1][2] * m[2][1], m[0][2] * m[2][1] - m[0][1] * m[2][2], m[0][1] * m[1][2] - m[0][2] * m[1][1]],
         [m[1][2] * m[2][0] - m[1][0] * m[2][2], m[0][0] * m[2][2] - m[0][2] * m[2][0], m[0][2] * m[1][0] - m[0][0] * m[1][2]],
         [m[1][0] * m[2][1] - m[1][1] * m[2][0], m[0][1] * m[2][0] - m[0][0] * m[2][1], m[0][0] * m[1][1] - m[0][1] * m[1][0]]]
    return k, (m[0][0] * k[0][0] + m[0][1] * k[1][0]) + m[0][2] * k[2][0]


def motion_record(cur, prev):
    """rpt_temporal_motion_record -> 24 doubles, or ValueError where the function returns RPT_ERR_INVALID.  None: the identity."""
    cur, prev = [[float(t) for t in np.asarray(np.eye(4) if m is None else m, dtype=np.float64).reshape(16)] for m in (cur, prev)]
    if not all(math.isfinite(t) for t in cur + prev):
        raise ValueError("a matrix value is not finite")
    for m in (cur, prev):
        if m[12:] != [0.0, 0.0, 0.0, 1.0]:
            raise ValueError("the bottom row must be 0 0 0 1")
    c = [[cur[4 * i + j] for j in range(3)] for i in range(3)]
    k, det = _cofactors(c)
    if det == 0.0 or not math.isfinite(det):
        raise ValueError("the current matrix has no inverse")
    if cur == prev:
        return IDENTITY_RECORD.copy()
    inv = [[k[i][j] / det for j in range(3)] for i in range(3)]
    u = [-((inv[i][0] * cur[3] + inv[i][1] * cur[7]) + inv[i][2] * cur[11]) for i in range(3)]
    out = [0.0] * MOTION_DOUBLES
    a = [[0.0] * 3 for _ in range(3)]
    for i in range(3):
        p = prev[4 * i:4 * i + 4]
        for j in range(3):
            a[i][j] = out[4 * i + j] = (p[0] * inv[0][j] + p[1] * inv[1][j]) + p[2] * inv[2][j]
        out[4 * i + 3] = ((p[0] * u[0] + p[1] * u[1]) + p[2] * u[2]) + p[3]
    k, det = _cofactors(a)
    if det == 0.0 or not math.isfinite(det):
        raise ValueError("the map between the frames has no inverse")
    for i in range(3):
        for j in range(3):
            out[12 + 3 * i + j] = k[j][i] / det
    return np.array(out, dtype=np.float64)


# ---- matrices
def translation(v):
    m = np.eye(4)
    m[:3, 3] = v
    return m


def rotation(angle, axis):
    a = np.asarray(axis, dtype=np.float64)
    x, y, z = a / np.linalg.norm(a)
    c, s = math.cos(angle), math.sin(angle)
    m = np.eye(4)
    m[:3, :3] = [[c + x * x * (1 - c), x * y * (1 - c) - z * s, x * z * (1 - c) + y * s],
                 [y * x * (1 - c) + z * s, c + y * y * (1 - c), y * z * (1 - c) - x * s],
                 [z * x * (1 - c) - y * s, z * y * (1 - c) + x * s, c + z * z * (1 - c)]]
    return m


def scaling(s):
    return np.diag([s, s, s, 1.0])


def random_matrix(rng):
    """T . R . S with a translation in [-2, 2]^3, any rotation about a random axis and a uniform scale in [0.5, 2]."""
    return translation(rng.uniform(-2.0, 2.0, 3)) @ rotation(rng.uniform(0.0, 2.0 * math.pi), rng.normal(size=3)) @ scaling(rng.uniform(0.5, 2.0))


def random_records(seed, m):
    """m records of random affine motions -> (m, 24).  Every odd one is between two unrelated matrices (the point lands anywhere, the
    tests mostly fail); every even one is a small step (a turn of up to 0.05 rad, a scale change of up to 2 %, a shift of up to 0.05)
    from a random matrix, so that pixels with a record do take history."""
    rng = np.random.default_rng(seed)
    recs = []
    for k in range(m):
        prev = random_matrix(rng)
        if k % 2 == 0:
            step = translation(rng.uniform(-0.05, 0.05, 3)) @ rotation(rng.uniform(-0.05, 0.05), rng.normal(size=3)) @ scaling(rng.uniform(0.98, 1.02))
            cur = step @ prev
        else:
            cur = random_matrix(rng)
        recs.append(motion_record(cur, prev))
    return np.stack(recs)


# ---- the moving analytic scene
RADIUS = 0.7


def sphere_matrix(f, spin):
    return translation(np.array([0.0, 0.0, 1.0]) + f * np.array([0.25, 0.1, 0.1])) @ rotation(spin * f, (0.0, 1.0, 0.0)) @ scaling(RADIUS)


def moving_planes(rec, w, h, m_sphere):
    """-> normal, depth (as analytic_planes: one camera sample through each pixel centre), paint (h, w, 3) and the sphere's mask."""
    rec = np.asarray(rec, dtype=np.float64)
    v, l = pixel_rays(rec, w, h)
    dirs = v / l[..., None]
    eye = rec[0:3]
    centre = m_sphere[:3, 3]
    with np.errstate(all="ignore"):
        oc = eye - centre
        bq = dirs @ oc
        disc = bq * bq - (oc @ oc - RADIUS * RADIUS)
        ts = np.where(disc > 0.0, -bq - np.sqrt(np.maximum(disc, 0.0)), np.inf)
        ts = np.where(ts > 0.0, ts, np.inf)
        tw = np.where(dirs[..., 2] != 0.0, -eye[2] / dirs[..., 2], np.inf)
        tw = np.where(tw > 0.0, tw, np.inf)
    t = np.minimum(ts, tw)
    hit = np.isfinite(t)
    sphere = hit & (ts <= tw)
    point = eye + np.where(hit, t, 0.0)[..., None] * dirs
    normal = np.where(sphere[..., None], (point - centre) / RADIUS, np.array([0.0, 0.0, 1.0]))
    normal = np.where(hit[..., None], normal, 0.0)
    depth = np.stack([np.where(hit, t, 0.0), hit.astype(np.float64), np.where(hit, np.where(sphere, 2.0, 1.0), 0.0)], axis=-1)
    inv = np.linalg.inv(m_sphere)
    local = point @ inv[:3, :3].T + inv[:3, 3]
    paint = np.where(sphere[..., None], 0.5 + 0.5 * local, 0.3)
    paint = np.where(hit[..., None], paint, 0.0)
    return normal, depth, paint, sphere


def moving_sequence(w, h, recs, spin):
    """Per camera record f: dict(rec, rgb, var, normal, depth, sphere, table) with table the (2, 24) motion table of frame f against
    frame f - 1 (wall: identity; None for f = 0), built by motion_record."""
    frames = []
    for f, rec in enumerate(recs):
        m = sphere_matrix(f, spin)
        normal, depth, paint, sphere = moving_planes(rec, w, h, m)
        table = np.stack([IDENTITY_RECORD, motion_record(m, sphere_matrix(f - 1, spin))]) if f else None
        frames.append(dict(rec=np.asarray(rec, dtype=np.float64), rgb=paint, var=np.full((h, w), 0.01), normal=normal, depth=depth,
                           sphere=sphere, table=table))
    return frames


def garbage_motion(seed, w, h, recs, m):
    """temporal_ref.garbage's tuples (record, radiance, variance, normal, depth) with ids that run from 0 to m + 2 and a NaN id here
    and there: ids inside the table, the two ends of it, ids past it and misses."""
    rng = np.random.default_rng(seed)
    frames = []
    for rec in recs:
        rgb = rng.normal(size=(h, w, 3)) * 3.0
        var = rng.uniform(0.0, 1.0, (h, w))
        normal = rng.normal(size=(h, w, 3))
        cov = rng.choice([0.0, 0.25, 0.5, 1.0, math.nan], (h, w), p=[0.1, 0.2, 0.2, 0.45, 0.05])
        ids = rng.integers(0, m + 3, (h, w)).astype(np.float64)
        ids = np.where(rng.uniform(size=(h, w)) < 0.03, math.nan, ids)
        depth = np.stack([rng.uniform(-2.0, 14.0, (h, w)) * np.where(cov > 0.0, cov, 1.0), cov, ids], axis=-1)
        frames.append((rec, rgb, var, normal, depth))
    return frames


class MotionRef(TemporalRef):
    """TemporalRef with the motion table of the call: accumulate(.., motion=(m, 24) array or None)."""

    def accumulate(self, rec, rgb, var, normal, depth, max_history=16, flags=MATCH_ID, depth_tol=0.1, normal_tol=0.5, motion=None):
        w, h = self.w, self.h
        rec = np.asarray(rec, dtype=np.float64).copy()
        rgb = np.asarray(rgb, dtype=np.float64).reshape(h, w, 3)
        depth = np.asarray(depth, dtype=np.float64).reshape(h, w, 3)
        v_in = np.asarray(var, dtype=np.float64).reshape(h, w) if var is not None else np.zeros((h, w))
        n = np.asarray(normal, dtype=np.float64).reshape(h, w, 3) if normal is not None else np.zeros((h, w, 3))
        if motion is not None:
            motion = np.asarray(motion, dtype=np.float64).reshape(-1, MOTION_DOUBLES)
        fw, fh, dim = float(w), float(h), float(max(w, h))
        with np.errstate(all="ignore"):
            cov = depth[..., 1]
            hit = cov > 0.0
            zc = depth[..., 0] / cov
            ident = depth[..., 2]
            B, C, V, L = np.zeros((h, w)), np.zeros((h, w, 3)), np.zeros((h, w)), np.zeros((h, w))
            fx = fy = np.full((h, w), np.nan)
            if self.hist is not None:
                hc, hv, hlen, hn, hz, hid = self.hist
                p = self.rec
                v, l = pixel_rays(rec, w, h)
                s = zc / l
                P = np.stack([rec[k] + s * v[..., k] for k in range(3)], axis=-1)
                nm = n
                if motion is not None and len(motion):
                    has = (ident >= 1.0) & (ident <= float(len(motion)))
                    o = np.where(has, ident, 1.0).astype(np.uint32) - 1
                    r = motion[o]                                           # (h, w, 24)
                    moved = np.stack([((r[..., 4 * k] * P[..., 0] + r[..., 4 * k + 1] * P[..., 1]) + r[..., 4 * k + 2] * P[..., 2]) + r[..., 4 * k + 3]
                                      for k in range(3)], axis=-1)
                    turned = np.stack([(r[..., 12 + 3 * k] * n[..., 0] + r[..., 13 + 3 * k] * n[..., 1]) + r[..., 14 + 3 * k] * n[..., 2]
                                       for k in range(3)], axis=-1)
                    P = np.where(has[..., None], moved, P)
                    nm = np.where(has[..., None], turned, n)
                q = np.stack([P[..., k] - p[k] for k in range(3)], axis=-1)

                def dot(a):
                    return (q[..., 0] * a[0] + q[..., 1] * a[1]) + q[..., 2] * a[2]

                zq = dot(p[3:6])
                valid = hit & (zq > 0.0)
                u = (dot(p[6:9]) * p[12]) / zq
                ww = (dot(p[9:12]) * p[12]) / zq
                fx = ((u * dim + fw) - 1.0) * 0.5
                fy = ((fh - 1.0) - ww * dim) * 0.5
                valid = valid & (fx > -1.0) & (fx < fw) & (fy > -1.0) & (fy < fh)
                flx, fly = np.floor(fx), np.floor(fy)
                ax, ay = fx - flx, fy - fly
                ix = np.where(valid, flx, 0.0).astype(np.int64)
                iy = np.where(valid, fly, 0.0).astype(np.int64)
                qq = (q[..., 0] * q[..., 0] + q[..., 1] * q[..., 1]) + q[..., 2] * q[..., 2]
                for j in (0, 1):
                    for i in (0, 1):
                        tx, ty = ix + i, iy + j
                        ok = valid & (tx >= 0) & (tx < w) & (ty >= 0) & (ty < h)
                        cx, cy = np.clip(tx, 0, w - 1), np.clip(ty, 0, h - 1)
                        b = (ax if i else 1.0 - ax) * (ay if j else 1.0 - ay)
                        ok = ok & (hlen[cy, cx] > 0.0)
                        if flags & MATCH_ID:
                            ok = ok & (hid[cy, cx] == ident)
                        if depth_tol > 0.0:
                            r2 = hz[cy, cx] * hz[cy, cx]
                            ok = ok & (np.abs(r2 - qq) <= depth_tol * qq)
                        if normal_tol > 0.0:
                            e = hn[cy, cx] - nm
                            ok = ok & (((e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]) <= normal_tol * normal_tol)
                        B = np.where(ok, B + b, B)
                        C = np.where(ok[..., None], C + b[..., None] * hc[cy, cx], C)
                        V = np.where(ok, V + (b * b) * hv[cy, cx], V)
                        L = np.where(ok, L + b * hlen[cy, cx], L)
            took = B > 0.0
            hcol = C / B[..., None]
            hvar = V / (B * B)
            hl = L / B
            length = np.where(took, np.minimum(hl + 1.0, float(max_history)), 1.0)
            a = 1.0 / length
            out = np.where(took[..., None], hcol + (rgb - hcol) * a[..., None], rgb)
            om = 1.0 - a
            out_v = np.where(took, (om * om) * hvar + (a * a) * v_in, v_in)
            finite = ~((out_v - out_v) != 0.0)
            for k in range(3):
                finite = finite & ~((out[..., k] - out[..., k]) != 0.0)
            stored = np.where(hit & finite, length, 0.0)
        self.hist = (out.copy(), out_v.copy(), stored, n.copy(), zc.copy(), ident.copy())
        self.rec = rec
        self.frames += 1
        self.last = dict(fx=fx, fy=fy, took=took, hit=hit)
        return out, out_v, length
