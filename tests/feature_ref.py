"""The contract of rpt_render_features* (include/rpt_hip.h) restated in numpy, from hooks the suite checks against the oracle one call
at a time: the camera sample (debug_camera_sample), the closest hit (get_closest_hit / get_closest_hit_f64), the environment's colour
(debug_env_color) and Material.color() of the Python scene.  A helper, not a test: tests/test_gpu_features.py compares the feature
pass with this composition, tests/test_features_host.py checks the reduction on synthetic samples."""
import numpy as np

from rpt_amd import KdTree, api


def reduce_samples(per_sample, chunk_spp):
    """The summation order of the interface: per_sample (S, ...) float64 -> mean over the S samples.  Samples are cut into chunks of
    chunk_spp (the last one ragged); a chunk is summed in sample order from +0.0, the chunk sums are added in chunk order from +0.0,
    and the total is divided by float(S)."""
    per_sample = np.asarray(per_sample, dtype=np.float64)
    n = per_sample.shape[0]
    total = np.zeros(per_sample.shape[1:], dtype=np.float64)
    for first in range(0, n, chunk_spp):
        part = np.zeros(per_sample.shape[1:], dtype=np.float64)
        for s in range(first, min(n, first + chunk_spp)):
            part = part + per_sample[s]
        total = total + part
    return total / np.float64(n)


def _leaves(shape):
    base = shape.base()
    return sum(_leaves(k) for k in base.shapes) if isinstance(base, KdTree) else 1


def record_colors(scene, f64):
    """Material.color() per object index as the closest-hit hooks report it: fp32 mode one entry per scene object, the colour rounded
    to float; reference-epsilon mode one entry per record -- a group's leaves are records of their own, in depth-first order, with
    the group's material -- in fp64."""
    if not f64:
        return np.array([o.material_.color() for o in scene.objects], dtype=np.float32).reshape(-1, 3).astype(np.float64)
    rows = []
    for o in scene.objects:
        rows += [o.material_.color()] * _leaves(o.shape)
    return np.array(rows, dtype=np.float64).reshape(-1, 3)


def feature_samples(renderer, iterations, seed, sample_offset, f64):
    """Per sample s and pixel: (a rgb, n xyz, z, c) as float64, shape (iterations, h * w, 8), and the object index of every sample,
    shape (iterations, h * w)."""
    w, h = renderer.width_, renderer.height_
    colors = record_colors(renderer.scene, f64)
    out = np.zeros((iterations, w * h, 8), dtype=np.float64)
    objs = np.zeros((iterations, w * h), dtype=np.int64)
    for s in range(iterations):
        cs = api.debug_camera_sample(renderer.camera, w, h, sample=sample_offset + s, seed=seed, f64=f64)
        t, obj, nrm = renderer.get_closest_hit_f64(cs["o"], cs["d"]) if f64 else renderer.get_closest_hit(cs["o"], cs["d"])
        hit = obj >= 0
        a = np.zeros((w * h, 3), dtype=np.float64)
        a[hit] = colors[obj[hit]]
        if not hit.all():
            a[~hit] = renderer.debug_env_color(cs["d"][~hit], f64=f64).astype(np.float64)
        out[s, :, 0:3] = a
        out[s, :, 3:6] = np.where(hit[:, None], nrm.astype(np.float64), 0.0)
        out[s, :, 6] = np.where(hit, t.astype(np.float64), 0.0)
        out[s, :, 7] = hit
        objs[s] = obj
    return out, objs


def feature_planes(renderer, iterations, seed, sample_offset, f64):
    """-> dict of albedo, normal, depth, (h, w, 3) float64 each, of the unsharded frame, under the chunking the scene reports."""
    w, h = renderer.width_, renderer.height_
    chunk_spp, n_chunks = renderer.chunking(iterations)
    assert n_chunks == -(-iterations // chunk_spp)
    per_sample, objs = feature_samples(renderer, iterations, seed, sample_offset, f64)
    mean = reduce_samples(per_sample, chunk_spp)
    depth = np.stack([mean[:, 6], mean[:, 7], (objs[0] + 1).astype(np.float64)], axis=1)
    return {"albedo": mean[:, 0:3].reshape(h, w, 3), "normal": mean[:, 3:6].reshape(h, w, 3), "depth": depth.reshape(h, w, 3)}
