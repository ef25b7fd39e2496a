"""The history clipping of the temporal accumulation (RPT_TEMPORAL_CLIP, rpt_temporal_set_clip) restated in numpy, next to
tests/temporal_ref.py and tests/temporal_motion_ref.py: ClipRef is MotionRef with the flag CLIP and the accumulator's three settings
(set_clip: radius, gamma, history; kept over reset, as the C ABI keeps them).  The whole accumulation is restated here, with the new
step between the taps and the blend, so that "without the flag nothing differs" is a statement about two restatements
(tests/test_temporal_clip_host.py) and not a delegation.  The kernel's output is compared with ClipRef bit for bit
(tests/test_gpu_temporal_clip.py); ClipRef is compared with a pixel-by-pixel, neighbour-by-neighbour transcription of the header text.

fmax_ and fmin_ are the header's: the operand that is not NaN; of two that compare equal, the first."""
import math

import numpy as np

from tests.temporal_motion_ref import MOTION_DOUBLES, MotionRef
from tests.temporal_ref import MATCH_ID, pixel_rays

CLIP = 2
CLIP_DEFAULTS = (1, 0.5, 1)


def fmax_(a, b):
    return np.where((a >= b) | (b != b), a, b)


def fmin_(a, b):
    return np.where((a <= b) | (b != b), a, b)


def window_sums(rgb, ident, radius, match):
    """The window of the definition for every pixel at once -> n (h, w), S (h, w, 3), Q (h, w, 3): dy outer, dx inner, pixels outside
    the image skipped, a pixel counted iff its three values are finite and (match) its id equals the centre's."""
    h, w = ident.shape
    r = int(radius)
    with np.errstate(all="ignore"):
        fin = ~((rgb - rgb) != 0.0).any(axis=-1)
    pad_rgb = np.zeros((h + 2 * r, w + 2 * r, 3))
    pad_rgb[r:r + h, r:r + w] = rgb
    pad_ok = np.zeros((h + 2 * r, w + 2 * r), dtype=bool)
    pad_ok[r:r + h, r:r + w] = fin
    pad_id = np.full((h + 2 * r, w + 2 * r), math.nan)
    pad_id[r:r + h, r:r + w] = ident
    n, S, Q = np.zeros((h, w)), np.zeros((h, w, 3)), np.zeros((h, w, 3))
    with np.errstate(all="ignore"):
        for dy in range(-r, r + 1):
            for dx in range(-r, r + 1):
                ys, xs = slice(r + dy, r + dy + h), slice(r + dx, r + dx + w)
                ok = pad_ok[ys, xs]
                if match:
                    ok = ok & (pad_id[ys, xs] == ident)
                c = np.where(ok[..., None], pad_rgb[ys, xs], 0.0)
                n = np.where(ok, n + 1.0, n)
                S = np.where(ok[..., None], S + c, S)
                Q = np.where(ok[..., None], Q + c * c, Q)
    return n, S, Q


class ClipRef(MotionRef):
    """MotionRef with RPT_TEMPORAL_CLIP: accumulate(.., flags=MATCH_ID | CLIP) uses the settings of set_clip.  self.last gains
    `clipped`, the mask of the pixels whose history colour the clamp changed."""

    def __init__(self, w, h):
        super().__init__(w, h)
        self.clip = CLIP_DEFAULTS

    def set_clip(self, radius=1, gamma=0.5, history=1):
        radius, gamma, history = int(radius), float(gamma), int(history)
        if not 1 <= radius <= 3 or not gamma >= 0.0 or math.isinf(gamma) or not 0 <= history <= 4096:
            raise ValueError("set_clip: radius 1..3, gamma finite and >= 0, history 0..4096")
        self.clip = (radius, gamma, history)

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
                    r = motion[o]
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
            clipped = np.zeros((h, w), dtype=bool)
            if flags & CLIP:
                # between 4 and 5: clamp the history colour to the current frame's window around the pixel itself
                radius, gamma, keep = self.clip
                cnt, S, Q = window_sums(rgb, ident, radius, bool(flags & MATCH_ID))
                some = took & (cnt > 0.0)
                m = S / cnt[..., None]
                sq = fmax_(Q / cnt[..., None] - m * m, 0.0)
                sd = np.sqrt(sq)
                lo, hi = m - gamma * sd, m + gamma * sd
                new = fmin_(fmax_(hcol, lo), hi)
                clipped = some & (new != hcol).any(axis=-1)
                hcol = np.where(some[..., None], new, hcol)
                if keep > 0:
                    hl = np.where(clipped, fmin_(hl, float(keep)), hl)
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
        self.last = dict(fx=fx, fy=fy, took=took, hit=hit, clipped=clipped)
        return out, out_v, length


def garbage_clip(seed, w, h, recs, m=0):
    """temporal_ref.garbage's tuples (record, radiance, variance, normal, depth) for the clipping tests: three ids (1..3; 0..m + 2
    with a motion table of m records), a NaN id here and there, NaN and inf colours sprinkled in, and coverage mostly 1 so that many
    pixels take history.  The camera barely moves between the records the tests pass, so the depths of one pixel agree across frames
    often enough for the depth test to pass where it is on."""
    rng = np.random.default_rng(seed)
    frames = []
    ids0 = rng.integers(0 if m else 1, (m + 3) if m else 4, (h, w)).astype(np.float64)
    z0 = rng.uniform(8.0, 11.0, (h, w))
    for rec in recs:
        rgb = rng.normal(size=(h, w, 3)) * 3.0
        for value in (math.nan, math.inf, -math.inf):
            bad, k = rng.uniform(size=(h, w)) < 0.03, int(rng.integers(0, 3))
            rgb[..., k] = np.where(bad, value, rgb[..., k])
        var = rng.uniform(0.0, 1.0, (h, w))
        normal = rng.normal(size=(h, w, 3))
        cov = rng.choice([0.0, 0.5, 1.0, math.nan], (h, w), p=[0.05, 0.15, 0.77, 0.03])
        ids = np.where(rng.uniform(size=(h, w)) < 0.2, rng.integers(0, m + 3 if m else 4, (h, w)).astype(np.float64), ids0)
        ids = np.where(rng.uniform(size=(h, w)) < 0.04, math.nan, ids)
        depth = np.stack([z0 * np.where(cov > 0.0, cov, 1.0), cov, ids], axis=-1)
        frames.append((rec, rgb, var, normal, depth))
    return frames


# ---- the quality measurement of DESIGN.md section 4, "History clipping" (CPU: the oracle's renders; the device test renders its own)
QUALITY_W, QUALITY_H, QUALITY_FRAMES, QUALITY_BATCHES, QUALITY_SEED, QUALITY_REF_SEED = 64, 48, 8, 4, 3, 1234
CUBE_ID, LIGHT_ID = 2.0, 6.0
CHANGED_LEVELS = 16


def quality_masks(id_planes, converged_last, converged_earlier):
    """static: pixels that keep one id in all frames, not the cube's or the light's; changed: static pixels whose converged 8-bit frame
    differs by >= 16 levels in some channel from the converged frame two scenes earlier."""
    ids = np.stack(id_planes)
    static = (ids == ids[0]).all(axis=0) & (ids[0] != CUBE_ID) & (ids[0] != LIGHT_ID)
    diff = np.abs(converged_last.astype(np.int64) - converged_earlier.astype(np.int64)).max(axis=-1)
    return static, static & (diff >= CHANGED_LEVELS)


def rms_levels(image8, converged8, mask):
    return float(np.sqrt(np.mean((image8.astype(np.float64) - converged8.astype(np.float64))[mask] ** 2)))


def oracle_sequence(scene_fn, spp=512):
    """The sequence scene_fn(0..7) at 64 x 48 by the oracle: per frame the mean and the variance of the mean of 4 batches of 1 spp
    (seed 3, sample offsets 4 f + k, as rpt_buffer_mean_device forms them), the feature planes of the same camera samples, the camera
    record and the motion table from the scenes' matrices -> (frames [(rec, rgb, var, normal, depth, table)], converged 8-bit frame of
    the last scene at `spp` with another seed, the same of the scene two earlier)."""
    from oracle import pyoracle
    from rpt_amd import color_bytes, temporal_camera_record, temporal_motion_record
    w, h, nb = QUALITY_W, QUALITY_H, QUALITY_BATCHES
    frames, prev, converged = [], None, {}
    for f in range(QUALITY_FRAMES):
        scene, cam, cfg = scene_fn(f)
        osc = pyoracle.OracleScene(scene)
        total, sumsq, feat, first = np.zeros((w * h, 3)), np.zeros(w * h), np.zeros((w * h, 5)), None
        for k in range(nb):
            b = osc.render(cam, w, h, 1, cfg["max_bounces"], seed=QUALITY_SEED, sample_offset=f * nb + k, robust=1)
            total = total + b
            sumsq = sumsq + ((b[:, 0] * b[:, 0] + b[:, 1] * b[:, 1]) + b[:, 2] * b[:, 2])
            cs = pyoracle.camera_rays(cam, w, h, sample=f * nb + k, seed=QUALITY_SEED)
            t, obj, nrm = osc.intersect(cs["o"], cs["d"], robust=1)
            hit = obj >= 0
            feat += np.concatenate([np.where(hit[:, None], nrm, 0.0), np.where(hit, t, 0.0)[:, None], hit[:, None].astype(np.float64)], axis=1)
            first = obj if first is None else first
        fn = float(nb)
        mean = total / fn
        var = np.fmax(sumsq - fn * ((mean[:, 0] * mean[:, 0] + mean[:, 1] * mean[:, 1]) + mean[:, 2] * mean[:, 2]), 0.0) / (fn - 1.0) / fn
        feat = feat / fn
        depth = np.stack([feat[:, 3], feat[:, 4], (first + 1).astype(np.float64)], axis=1).reshape(h, w, 3)
        table = None
        if prev is not None:
            table = np.stack([temporal_motion_record(c.shape.matrix(), p.shape.matrix()) for c, p in zip(scene.objects, prev.objects)])
        frames.append((temporal_camera_record(cam), mean.reshape(h, w, 3), var.reshape(h, w), feat[:, 0:3].reshape(h, w, 3), depth, table))
        if f in (QUALITY_FRAMES - 3, QUALITY_FRAMES - 1):
            converged[f] = color_bytes(osc.render(cam, w, h, spp, cfg["max_bounces"], seed=QUALITY_REF_SEED, robust=1).reshape(h, w, 3))
        prev = scene
    return frames, converged[QUALITY_FRAMES - 1], converged[QUALITY_FRAMES - 3]


def quality_rows(frames, converged, earlier, settings):
    """-> (static count, changed count, {name: (rms over changed, rms over static)}) with names "alone", "plain" and one per
    (radius, gamma, history) of `settings`, all by ClipRef on `frames` with the default parameters."""
    from rpt_amd import color_bytes
    w, h = QUALITY_W, QUALITY_H
    static, changed = quality_masks([fr[4][..., 2] for fr in frames], converged, earlier)

    def run(flags, clip=None):
        ref = ClipRef(w, h)
        if clip is not None:
            ref.set_clip(*clip)
        for rec, rgb, var, normal, depth, table in frames:
            out, _, _ = ref.accumulate(rec, rgb, var, normal, depth, flags=flags, motion=table)
        return color_bytes(out)

    both = lambda img: (rms_levels(img, converged, changed), rms_levels(img, converged, static))  # noqa: E731
    rows = {"alone": both(color_bytes(frames[-1][1])), "plain": both(run(MATCH_ID))}
    for s in settings:
        rows[tuple(s)] = both(run(MATCH_ID | CLIP, s))
    return int(static.sum()), int(changed.sum()), rows
