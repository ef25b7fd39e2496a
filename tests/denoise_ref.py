"""The a-trous filter of include/rpt_hip.h (rpt_denoise*) restated in numpy: one array operation per rounded fp64 operation of the
definition, in its order.  A skipped tap goes through np.where, never through a multiplication by 0 (0 * NaN is NaN), and there is
no `**`.  tests/test_denoise_host.py holds this restatement to a pixel-by-pixel transcription of the definition and to the cases in
which the definition is exact; tests/test_gpu_denoise.py compares the kernels with it bit for bit."""
import numpy as np

DEMODULATE, MATCH_ID = 1, 2
G = {-1: 0.25, 0: 0.5, 1: 0.25}
H = {-2: 0.0625, -1: 0.25, 0: 0.375, 1: 0.25, 2: 0.0625}


def shifted(a, ox, oy):
    """-> (inside, values): values[y, x] = a[y + oy, x + ox] where that pixel is inside the image (elsewhere some pixel of the image:
    np.where drops it)."""
    h, w = a.shape[:2]
    ys, xs = np.arange(h) + oy, np.arange(w) + ox
    inside = ((ys >= 0) & (ys < h))[:, None] & ((xs >= 0) & (xs < w))[None, :]
    return inside, a[np.clip(ys, 0, h - 1)[:, None], np.clip(xs, 0, w - 1)[None, :]]


def sq3(e):
    """(e0 e0 + e1 e1) + e2 e2 of an (h, w, 3) array."""
    return (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]


def prepare(rgb, var, albedo, normal, depth, flags):
    """-> den, c, v, n, z, ids: the set-up per pixel."""
    rgb = np.asarray(rgb, dtype=np.float64)
    h, w = rgb.shape[:2]
    den = np.where(np.asarray(albedo) > 0.0, albedo, 1.0) if flags & DEMODULATE else np.ones((h, w, 3))
    c = rgb / den
    v = np.array(var, dtype=np.float64) if var is not None else np.zeros((h, w))
    n = np.asarray(normal, dtype=np.float64) if normal is not None else np.zeros((h, w, 3))
    z = np.asarray(depth, dtype=np.float64)[..., 0] if depth is not None else np.zeros((h, w))
    ids = np.asarray(depth, dtype=np.float64)[..., 2] if depth is not None else np.zeros((h, w))
    return den, c, v, n, z, ids


def denoise_pass(c, v, den, n, z, ids, step, flags, sigma_color, sigma_normal, sigma_depth):
    """One pass at `step` -> (c', v')."""
    h, w = v.shape
    if sigma_color > 0.0:
        sv, sg = np.zeros((h, w)), np.zeros((h, w))
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                inside, vq = shifted(v, dx, dy)
                gg = G[dy] * G[dx]
                sv = np.where(inside, sv + gg * vq, sv)
                sg = np.where(inside, sg + gg, sg)
        vhat = sv / sg
        kp = 1.0 / ((sigma_color * sigma_color) * (vhat + 1e-12))
    a_n = 1.0 / sigma_normal if sigma_normal > 0.0 else None
    a_z = 1.0 / (sigma_depth * float(step)) if sigma_depth > 0.0 else None
    W, C, V = np.zeros((h, w)), np.zeros((h, w, 3)), np.zeros((h, w))
    for dy in (-2, -1, 0, 1, 2):
        for dx in (-2, -1, 0, 1, 2):
            inside, cq = shifted(c, step * dx, step * dy)
            x = np.zeros((h, w))
            if sigma_color > 0.0:
                x = x + sq3((cq - c) * den) * kp
            if sigma_normal > 0.0:
                x = x + sq3((shifted(n, step * dx, step * dy)[1] - n) * a_n)
            if sigma_depth > 0.0:
                e = (shifted(z, step * dx, step * dy)[1] - z) * a_z
                x = x + e * e
            ok = inside & (x < 4.0)
            if flags & MATCH_ID:
                ok = ok & (shifted(ids, step * dx, step * dy)[1] == ids)
            t = 1.0 - x * 0.25
            t2 = t * t
            wt = (t2 * t2) * (H[dy] * H[dx])
            W = np.where(ok, W + wt, W)
            C = np.where(ok[..., None], C + wt[..., None] * cq, C)
            V = np.where(ok, V + (wt * wt) * shifted(v, step * dx, step * dy)[1], V)
    keep = ~(W > 0.0)
    return np.where(keep[..., None], c, C / W[..., None]), np.where(keep, v, V / (W * W))


def denoise_ref(rgb, var, albedo, normal, depth, passes=4, flags=DEMODULATE | MATCH_ID, sigma_color=4.0, sigma_normal=0.5, sigma_depth=0.0):
    """-> (out, out_var): (h, w, 3) and (h, w)."""
    with np.errstate(all="ignore"):
        den, c, v, n, z, ids = prepare(rgb, var, albedo, normal, depth, flags)
        for i in range(passes):
            c, v = denoise_pass(c, v, den, n, z, ids, 1 << i, flags, sigma_color, sigma_normal, sigma_depth)
        return c * den, v
