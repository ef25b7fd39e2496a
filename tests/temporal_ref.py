"""The temporal accumulation of include/rpt_hip.h (rpt_temporal_*) restated in numpy: the same fp64 operations in the same order, each
rounded on its own (numpy's elementwise ufuncs: IEEE add, multiply, divide, sqrt, no contraction), vectorised over the frame.  The
kernel's output is compared with this bit for bit (tests/test_gpu_temporal.py); this is compared with a pixel-by-pixel transcription
of the header text (tests/test_temporal_host.py).

Cameras enter as records -- the 13 doubles eye, direction, right, up, d of rpt_temporal_camera_record -- so that nothing depends on
two tan implementations agreeing."""
import math

import numpy as np

MATCH_ID = 1


def camera_record(eye, direction, up, fov):
    """The record by Python's math, in the order the header states: right = normalize(cross(direction, up)), d = 1 / tan(fov / 2)."""
    e, dr, u = [[float(t) for t in v] for v in (eye, direction, up)]
    c = [dr[1] * u[2] - dr[2] * u[1], dr[2] * u[0] - dr[0] * u[2], dr[0] * u[1] - dr[1] * u[0]]
    ln = math.sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2])
    return np.array(e + dr + [t / ln for t in c] + u + [1.0 / math.tan(fov / 2.0)], dtype=np.float64)


def look_at_record(eye, center, up, fov):
    """Camera::look_at (src/camera.rs:44-56) -> record."""
    eye, center, up = [np.asarray(v, dtype=np.float64) for v in (eye, center, up)]
    direction = center - eye
    direction = direction / np.linalg.norm(direction)
    up = up - np.dot(up, direction) * direction
    up = up / np.linalg.norm(up)
    return camera_record(eye, direction, up, fov)


def pixel_rays(rec, w, h):
    """Step 1 of the definition: v (h, w, 3) and l (h, w) of the pixel centres."""
    rec = np.asarray(rec, dtype=np.float64)
    direction, right, up, d = rec[3:6], rec[6:9], rec[9:12], rec[12]
    dim = float(max(w, h))
    xs, ys = np.arange(w, dtype=np.int64), np.arange(h, dtype=np.int64)
    xn = ((2 * xs + 1).astype(np.float64) - float(w)) / dim
    yn = ((2 * (h - ys) - 1).astype(np.float64) - float(h)) / dim
    v = np.stack([(d * direction[k] + xn[None, :] * right[k]) + yn[:, None] * up[k] for k in range(3)], axis=-1)
    l = np.sqrt((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2])
    return v, l


def analytic_planes(rec, w, h):
    """The normal and depth planes of the analytic scene of the tests as one camera sample through each pixel centre gives them: the
    wall z = 0 with id 1 (normal +z) and the sphere of radius 0.7 at (0, 0, 1) with id 2; a ray that reaches neither is a miss
    (n = 0, depth = (0, 0, 0)).  -> normal (h, w, 3), depth (h, w, 3) = (distance, 1, id)."""
    rec = np.asarray(rec, dtype=np.float64)
    v, l = pixel_rays(rec, w, h)
    dirs = v / l[..., None]
    eye = rec[0:3]
    centre, radius = np.array([0.0, 0.0, 1.0]), 0.7
    with np.errstate(all="ignore"):
        oc = eye - centre
        bq = dirs @ oc
        disc = bq * bq - (oc @ oc - radius * radius)
        ts = np.where(disc > 0.0, -bq - np.sqrt(np.maximum(disc, 0.0)), np.inf)
        ts = np.where(ts > 0.0, ts, np.inf)
        tw = np.where(dirs[..., 2] != 0.0, -eye[2] / dirs[..., 2], np.inf)
        tw = np.where(tw > 0.0, tw, np.inf)
    t = np.minimum(ts, tw)
    hit = np.isfinite(t)
    sphere = hit & (ts <= tw)
    point = eye + np.where(hit, t, 0.0)[..., None] * dirs
    normal = np.where(sphere[..., None], (point - centre) / radius, np.array([0.0, 0.0, 1.0]))
    normal = np.where(hit[..., None], normal, 0.0)
    depth = np.stack([np.where(hit, t, 0.0), hit.astype(np.float64), np.where(hit, np.where(sphere, 2.0, 1.0), 0.0)], axis=-1)
    return normal, depth


# ---- the inputs the tests share
FOV = math.pi / 6
EYES = [(0.0, 0.0, 10.0), (0.3, 0.1, 9.8), (0.55, 0.25, 9.5), (0.7, 0.2, 9.3)]      # all looking at the origin


def analytic_cameras(n=4):
    from rpt_amd import Camera
    return [Camera.look_at(e, (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), FOV) for e in EYES[:n]]


def arc_cameras(camera, n, distance, step=0.02):
    """n cameras on a small arc: `camera`'s eye turned by k * step radians about the axis `up` through the point `distance` ahead of
    it, looking at that point."""
    from rpt_amd import Camera
    eye, up = np.asarray(camera.eye, dtype=np.float64), np.asarray(camera.up, dtype=np.float64)
    direction = np.asarray(camera.direction, dtype=np.float64)
    direction, up = direction / np.linalg.norm(direction), up / np.linalg.norm(up)
    centre = eye + distance * direction
    side = np.cross(direction, up)
    cams = []
    for k in range(n):
        a = k * step
        cams.append(Camera.look_at(centre - distance * (math.cos(a) * direction + math.sin(a) * side), centre, up, camera.fov))
    return cams


def sequence(seed, w, h, recs):
    """Per record of a moving camera: (record, radiance, variance, normal, depth) on the analytic scene with random radiance and
    variance, coverage 0.5 or 1, and a few misses, foreign ids, NaN and inf colours, variances and depths sprinkled in (the frame
    after must not take them)."""
    rng = np.random.default_rng(seed)
    frames = []
    for f, rec in enumerate(recs):
        normal, depth = analytic_planes(rec, w, h)
        depth = depth.copy()
        depth[..., 1] = rng.choice([0.5, 1.0], (h, w))                  # coverage < 1: depth[0] is the mean over all samples
        depth[..., 0] *= depth[..., 1]
        rgb = rng.uniform(0.0, 2.0, (h, w, 3))
        var = rng.uniform(0.0, 0.05, (h, w))
        for k in range(max(1, w * h // 12)):
            x, y = int(rng.integers(0, w)), int(rng.integers(0, h))
            what = (k + f) % 6
            if what == 0:
                depth[y, x], normal[y, x] = 0.0, 0.0                    # a miss
            elif what == 1:
                depth[y, x, 2] = 7.0
            elif what == 2:
                rgb[y, x, k % 3] = math.nan if k % 2 else math.inf
            elif what == 3:
                var[y, x] = math.inf if k % 2 else math.nan
            elif what == 4:
                depth[y, x, 0] = math.nan if k % 2 else math.inf
            else:
                depth[y, x, 1] = math.nan
        frames.append((rec, rgb, var, normal, depth))
    return frames


def garbage(seed, w, h, recs):
    """The same tuple per record with planes that belong to no scene: any depth, coverage (0 and NaN among them), id and normal."""
    rng = np.random.default_rng(seed)
    frames = []
    for rec in recs:
        rgb = rng.normal(size=(h, w, 3)) * 3.0
        var = rng.uniform(0.0, 1.0, (h, w))
        normal = rng.normal(size=(h, w, 3))
        cov = rng.choice([0.0, 0.25, 0.5, 1.0, math.nan], (h, w), p=[0.1, 0.2, 0.2, 0.45, 0.05])
        depth = np.stack([rng.uniform(-2.0, 14.0, (h, w)) * np.where(cov > 0.0, cov, 1.0), cov, rng.integers(0, 3, (h, w)).astype(np.float64)],
                         axis=-1)
        frames.append((rec, rgb, var, normal, depth))
    return frames


class TemporalRef:
    """The accumulator: the history records of the last frame (c, v, len, n, z, id as arrays) and its camera record."""

    def __init__(self, w, h):
        self.w, self.h = int(w), int(h)
        self.reset()

    def reset(self):
        self.hist, self.rec, self.frames = None, None, 0
        self.last = None

    def accumulate(self, rec, rgb, var, normal, depth, max_history=16, flags=MATCH_ID, depth_tol=0.1, normal_tol=0.5):
        """-> (out (h, w, 3), out_v (h, w), len (h, w)).  self.last keeps fx, fy and the mask of the pixels that took history."""
        w, h = self.w, self.h
        rec = np.asarray(rec, dtype=np.float64).copy()
        rgb = np.asarray(rgb, dtype=np.float64).reshape(h, w, 3)
        depth = np.asarray(depth, dtype=np.float64).reshape(h, w, 3)
        v_in = np.asarray(var, dtype=np.float64).reshape(h, w) if var is not None else np.zeros((h, w))
        n = np.asarray(normal, dtype=np.float64).reshape(h, w, 3) if normal is not None else np.zeros((h, w, 3))
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
                q = np.stack([(rec[k] + s * v[..., k]) - p[k] for k in range(3)], axis=-1)

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
                            r = hz[cy, cx] * hz[cy, cx]
                            ok = ok & (np.abs(r - qq) <= depth_tol * qq)
                        if normal_tol > 0.0:
                            e = hn[cy, cx] - n
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
