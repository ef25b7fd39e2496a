"""The guided upsampling of include/rpt_hip.h (rpt_upsample*) restated in numpy: one array operation per rounded fp64 operation of the
definition, in its order.  A skipped tap goes through np.where, never through a multiplication by 0 (0 * NaN is NaN), and there is
no `**`.  tests/test_upsample_host.py holds this restatement to a pixel-by-pixel transcription of the definition and to the cases in
which the definition is exact; tests/test_gpu_upsample.py compares the kernel with it bit for bit."""
import numpy as np

from tests.denoise_ref import sq3

DEMODULATE, MATCH_ID = 1, 2


def positions(n_hi, s):
    """-> (i0, f) of the n_hi full-resolution coordinates on one axis: integers, then one division."""
    t = 2 * np.arange(n_hi, dtype=np.int64) + 1 - s
    i0 = t // (2 * s)                                            # floor division
    return i0, (t - 2 * s * i0).astype(np.float64) / float(2 * s)


def upsample_ref(lo_rgb, lo_var, lo_albedo, lo_normal, lo_depth, hi_albedo, hi_normal, hi_depth, scale=2, radius=1,
                 flags=DEMODULATE | MATCH_ID, sigma_normal=0.0, sigma_depth=0.0, return_fallback=False):
    """-> (out_rgb, out_var): (s h, s w, 3) and (s h, s w); with return_fallback also the (s h, s w) mask of the pixels whose Wsum is
    not > 0."""
    with np.errstate(all="ignore"):
        lo_rgb = np.asarray(lo_rgb, dtype=np.float64)
        h, w = lo_rgb.shape[:2]
        s, r = int(scale), int(radius)
        H, W = s * h, s * w
        if flags & DEMODULATE:
            den_q = np.where(np.asarray(lo_albedo) > 0.0, lo_albedo, 1.0)
            den_p = np.where(np.asarray(hi_albedo) > 0.0, hi_albedo, 1.0)
        else:
            den_q, den_p = np.ones((h, w, 3)), np.ones((H, W, 3))
        c = lo_rgb / den_q
        v = np.array(lo_var, dtype=np.float64) if lo_var is not None else np.zeros((h, w))
        i0, fx = positions(W, s)
        j0, fy = positions(H, s)
        a_n = 1.0 / sigma_normal if sigma_normal > 0.0 else None
        a_z = 1.0 / (sigma_depth * float(s)) if sigma_depth > 0.0 else None
        Wsum, C, V = np.zeros((H, W)), np.zeros((H, W, 3)), np.zeros((H, W))
        for dy in range(1 - r, r + 1):
            qy = j0 + dy
            g_dy = 1.0 - np.abs(fy - float(dy)) / float(r)
            for dx in range(1 - r, r + 1):
                qx = i0 + dx
                g_dx = 1.0 - np.abs(fx - float(dx)) / float(r)
                ok = (((qy >= 0) & (qy < h) & (g_dy > 0.0))[:, None] & ((qx >= 0) & (qx < w) & (g_dx > 0.0))[None, :])
                iy, ix = np.clip(qy, 0, h - 1)[:, None], np.clip(qx, 0, w - 1)[None, :]   # (some pixel of the image where not ok)
                x = np.zeros((H, W))
                if sigma_normal > 0.0:
                    x = x + sq3((np.asarray(lo_normal)[iy, ix] - hi_normal) * a_n)
                if sigma_depth > 0.0:
                    e = (np.asarray(lo_depth)[iy, ix][..., 0] - np.asarray(hi_depth)[..., 0]) * a_z
                    x = x + e * e
                ok = ok & (x < 4.0)
                if flags & MATCH_ID:
                    ok = ok & (np.asarray(lo_depth)[iy, ix][..., 2] == np.asarray(hi_depth)[..., 2])
                t = 1.0 - x * 0.25
                t2 = t * t
                wgt = (t2 * t2) * (g_dy[:, None] * g_dx[None, :])
                Wsum = np.where(ok, Wsum + wgt, Wsum)
                C = np.where(ok[..., None], C + wgt[..., None] * c[iy, ix], C)
                V = np.where(ok, V + (wgt * wgt) * v[iy, ix], V)
        fallback = ~(Wsum > 0.0)
        own_y, own_x = (np.arange(H) // s)[:, None], (np.arange(W) // s)[None, :]
        cc = np.where(fallback[..., None], c[own_y, own_x], C / Wsum[..., None])
        vv = np.where(fallback, v[own_y, own_x], V / (Wsum * Wsum))
        out = cc * den_p
        return (out, vv, fallback) if return_fallback else (out, vv)


def oracle_planes(osc, scene, cam, w, h, samples, seed, offset=0):
    """albedo, normal, depth of `samples` camera samples from `offset` on at w x h, as rpt_render_features defines them, from the
    oracle's closest hits (osc: the scene's pyoracle.OracleScene) -> three (h, w, 3) arrays."""
    from oracle import pyoracle
    colors = np.array([o.material_.color() for o in scene.objects], dtype=np.float64).reshape(-1, 3)
    acc, first = np.zeros((w * h, 8)), None
    for s in range(samples):
        cs = pyoracle.camera_rays(cam, w, h, sample=offset + s, seed=seed)
        t, obj, nrm = osc.intersect(cs["o"], cs["d"], robust=1)
        hit = obj >= 0
        a = np.zeros((w * h, 3))
        a[hit] = colors[obj[hit]]
        if not hit.all():
            a[~hit] = osc.env_color(cs["d"][~hit])
        acc += np.concatenate([a, np.where(hit[:, None], nrm, 0.0), np.where(hit, t, 0.0)[:, None], hit[:, None].astype(np.float64)], axis=1)
        first = obj if first is None else first
    mean = acc / float(samples)
    depth = np.stack([mean[:, 6], mean[:, 7], (first + 1).astype(np.float64)], axis=1)
    return mean[:, 0:3].reshape(h, w, 3), mean[:, 3:6].reshape(h, w, 3), depth.reshape(h, w, 3)


def mean_and_variance(batches):
    """The per-pixel mean of (n_pixels, 3) batches and the variance of that mean, as rpt_buffer_mean_device orders them."""
    total, sumsq = np.zeros(batches[0].shape), np.zeros(batches[0].shape[0])
    for b in batches:
        total = total + b
        sumsq = sumsq + ((b[:, 0] * b[:, 0] + b[:, 1] * b[:, 1]) + b[:, 2] * b[:, 2])
    fn = float(len(batches))
    mean = total / fn
    var = np.fmax(sumsq - fn * ((mean[:, 0] * mean[:, 0] + mean[:, 1] * mean[:, 1]) + mean[:, 2] * mean[:, 2]), 0.0) / (fn - 1.0) / fn
    return mean, var


def replicate(lo, scale):
    """Plain s x s replication of a low-resolution array: what the upsampling has to beat."""
    return np.repeat(np.repeat(np.asarray(lo), scale, axis=0), scale, axis=1)
