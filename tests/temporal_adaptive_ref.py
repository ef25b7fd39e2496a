"""Adaptive sampling over a sequence (include/rpt_hip.h: rpt_temporal_preview_device, rpt_temporal_tile_errors_device,
rpt_render_adaptive_temporal) restated in numpy on top of tests/temporal_clip_ref.py and tests/adaptive_ref.py:
  preview             a deep copy of the accumulator's restatement (ClipRef) accumulates the frame; the outputs are masked to the
                      listed tiles; the original is untouched: no history, no frame count, and the caller still holds the table;
  plane_tile_errors   adaptive_ref.tile_errors' tree with the pixel's terms taken from planes;
  select_among        adaptive_ref.select among a list, the ids in the list's order;
  adaptive_temporal_loop
                      the loop over a callable that returns a full-frame batch per sample offset, with RefBuffer.add_tiles.
The kernels are compared with these bit for bit (tests/test_gpu_temporal_adaptive.py); tests/test_temporal_adaptive_host.py holds them
to a pixel-by-pixel, slot-by-slot transcription of the header text.

Test infrastructure: not part of the product."""
import copy

import numpy as np

from tests.adaptive_ref import TILE, RefBuffer, tile_grid, tile_pixels


def tile_mask(tiles, w, h):
    """(h, w) bool: the in-image pixels of the listed tiles (None: every pixel); an id out of range lists nothing."""
    if tiles is None:
        return np.ones((h, w), dtype=bool)
    tx, ty = tile_grid(w, h)
    m = np.zeros((h, w), dtype=bool)
    for t in tiles:
        if 0 <= int(t) < tx * ty:
            ys, xs = tile_pixels(t, w, h)
            m[ys, xs] = True
    return m


def preview(ref, rec, rgb, var, normal, depth, tiles=None, fill=np.nan, **kw):
    """-> (out, out_v, len) of ref.accumulate(rec, rgb, var, normal, depth, **kw) in the listed tiles, `fill` elsewhere; `ref` (a
    ClipRef, or any of the restatements it derives from) is left as it was."""
    twin = copy.deepcopy(ref)
    out, out_v, length = twin.accumulate(rec, rgb, var, normal, depth, **kw)
    m = tile_mask(tiles, ref.w, ref.h)
    return np.where(m[..., None], out, fill), np.where(m, out_v, fill), np.where(m, length, fill)


def plane_tile_errors(rgb, var, floor, tiles=None, fill=np.nan):
    """E_t of the listed tiles (None: of every tile) -> (tiles_y, tiles_x), `fill` in the other entries: y = (rgb_0 + rgb_1) + rgb_2,
    a_j = var / (y y + floor floor), +0.0 in the slots outside the image, halving strides 512 .. 1, over double(in-image pixels)."""
    h, w = var.shape
    tx_n, ty_n = tile_grid(w, h)
    floor = float(floor)
    with np.errstate(all="ignore"):
        y = (rgb[..., 0] + rgb[..., 1]) + rgb[..., 2]
        a = var / (y * y + floor * floor)
    slots = np.zeros((ty_n * TILE, tx_n * TILE))
    slots[:h, :w] = a
    t = slots.reshape(ty_n, TILE, tx_n, TILE).transpose(0, 2, 1, 3).reshape(ty_n, tx_n, TILE * TILE).copy()
    s = TILE * TILE // 2
    with np.errstate(all="ignore"):
        while s >= 1:
            t[..., :s] = t[..., :s] + t[..., s:2 * s]
            s //= 2
        inside = np.minimum(TILE, w - TILE * np.arange(tx_n))[None, :] * np.minimum(TILE, h - TILE * np.arange(ty_n))[:, None]
        err = t[..., 0] / inside.astype(np.float64)
    if tiles is None:
        return err
    out = np.full((ty_n, tx_n), fill, dtype=np.float64)
    for i in tiles:
        if 0 <= int(i) < tx_n * ty_n:
            out.reshape(-1)[int(i)] = err.reshape(-1)[int(i)]
    return out


def select_among(errors, tile_counts, threshold, max_batches, tiles=None):
    """The listed ids (None: every id) whose tile has E_t > threshold threshold (false for NaN) and n_t < max_batches, in the list's
    order."""
    thr2 = float(threshold) * float(threshold)
    e, n = np.asarray(errors).reshape(-1), np.asarray(tile_counts).reshape(-1)
    ids = range(e.size) if tiles is None else [int(t) for t in tiles]
    with np.errstate(invalid="ignore"):
        return np.array([t for t in ids if 0 <= t < e.size and e[t] > thr2 and n[t] < int(max_batches)], dtype=np.uint32)


def adaptive_temporal_loop(batch_at, w, h, ref, rec, normal, depth, spp_per_batch, min_batches, max_batches, threshold, floor, sample_offset=0,
                           buffer=None, **kw):
    """rpt_render_adaptive_temporal: batch_at(offset) -> the full-frame batch of spp_per_batch samples at that sample offset, (h, w, 3);
    ref: the accumulator's restatement, left as it was; kw: accumulate's (max_history, flags, depth_tol, normal_tol, motion); buffer:
    an empty buffer with RefBuffer's add / add_tiles / mean / tile_batches (default: a RefBuffer).
    -> (RefBuffer, stats, (out, out_v, len) of every tile's last preview, the active lists round by round)."""
    buf = buffer if buffer is not None else RefBuffer(w, h)
    for k in range(min_batches):
        buf.add(batch_at(sample_offset + k * spp_per_batch))
    tx, ty = tile_grid(w, h)
    active, lists = None, []
    rounds, tile_batches = 0, min_batches * tx * ty
    last = (np.full((h, w, 3), np.nan), np.full((h, w), np.nan), np.full((h, w), np.nan))
    for k in range(min_batches, max_batches):
        mean, var = buf.mean()
        pv = preview(ref, rec, mean, var, normal, depth, tiles=active, **kw)
        m = tile_mask(active, w, h)
        last = (np.where(m[..., None], pv[0], last[0]), np.where(m, pv[1], last[1]), np.where(m, pv[2], last[2]))
        err = plane_tile_errors(pv[0], pv[1], floor, tiles=active)
        active = select_among(err, buf.tile_batches(), threshold, max_batches, active)
        lists.append(active.copy())
        if active.size == 0:
            break
        buf.add_tiles(batch_at(sample_offset + k * spp_per_batch), active)
        rounds += 1
        tile_batches += int(active.size)
    stats = (rounds, tile_batches, int((buf.tile_batches() == max_batches).sum()), tx * ty)
    return buf, stats, last, lists


def plain_adaptive_loop(batch_at, w, h, spp_per_batch, min_batches, max_batches, threshold, floor, sample_offset=0, buffer=None):
    """rpt_render_adaptive (at a sample offset) over the same callable: the buffer's tile_errors and adaptive_ref.select."""
    from tests.adaptive_ref import select
    buf = buffer if buffer is not None else RefBuffer(w, h)
    for k in range(min_batches):
        buf.add(batch_at(sample_offset + k * spp_per_batch))
    tx, ty = tile_grid(w, h)
    rounds, tile_batches = 0, min_batches * tx * ty
    for k in range(min_batches, max_batches):
        ids = select(buf.tile_errors(floor), buf.tile_batches(), threshold, max_batches)
        if ids.size == 0:
            break
        buf.add_tiles(batch_at(sample_offset + k * spp_per_batch), ids)
        rounds += 1
        tile_batches += int(ids.size)
    return buf, (rounds, tile_batches, int((buf.tile_batches() == max_batches).sum()), tx * ty)


# ---- the conditions of DESIGN.md section 4, "Adaptive sampling over a sequence": scenes.sliding_shadow(0) under its camera, at rest,
# 96 x 64 (6 tiles), four frames and a fifth behind a reset, seed 3.  The settings were chosen on the CPU (the oracle's renders) so that
# in frame 0 tiles stop at min_batches, between, and at max_batches: 2 3 2 8 6 8 there.
QUALITY_SCENE, QUALITY_W, QUALITY_H, QUALITY_FRAMES, QUALITY_SEED = "sliding_shadow", 96, 64, 4, 3
QUALITY_LOOP = dict(spp_per_batch=2, min_batches=2, max_batches=8, threshold=0.06, floor=0.05)


def frame_offset(f):
    return f * QUALITY_LOOP["max_batches"] * QUALITY_LOOP["spp_per_batch"]


def check_conditions(counts, plain_first, counts_after_reset, plain_after_reset):
    """counts: the (tiles_y, tiles_x) batches of frames 0 .. 3 of the new loop; plain_first: the plain adaptive loop's of frame 0;
    the last two: the frame behind a reset, by the new and by the plain loop at the same offset.  Directions, never thresholds."""
    lo, hi = QUALITY_LOOP["min_batches"], QUALITY_LOOP["max_batches"]
    first = np.asarray(counts[0]).reshape(-1)
    assert (first < hi).any() and (first > lo).any(), first                     # else the conditions say nothing
    assert np.array_equal(counts[0], plain_first)                                # (a)
    totals = [int(np.asarray(c).sum()) for c in counts]
    assert all(t <= totals[0] for t in totals[1:]) and sum(totals) < len(totals) * totals[0], totals   # (b)
    assert np.array_equal(counts_after_reset, plain_after_reset)                 # (c)
    return totals


def oracle_frame_inputs(osc, cam, max_bounces, w, h, seed, spp_per_batch, min_batches):
    """-> (batch_at(offset), planes_at(offset) -> (normal, depth)): the oracle's full-frame batches of spp_per_batch samples, and the
    feature planes of the first min_batches * spp_per_batch camera samples from `offset` on, as rpt_render_features defines them."""
    import functools

    from oracle import pyoracle

    @functools.lru_cache(maxsize=None)
    def batch_at(offset):
        b = osc.render(cam, w, h, spp_per_batch, max_bounces, seed=seed, sample_offset=offset, robust=1).reshape(h, w, 3)
        b.setflags(write=False)
        return b

    def planes_at(offset):
        n = min_batches * spp_per_batch
        feat, first = np.zeros((w * h, 5)), None
        for s in range(n):
            cs = pyoracle.camera_rays(cam, w, h, sample=offset + s, seed=seed)
            t, obj, nrm = osc.intersect(cs["o"], cs["d"], robust=1)
            hit = obj >= 0
            feat += np.concatenate([np.where(hit[:, None], nrm, 0.0), np.where(hit, t, 0.0)[:, None], hit[:, None].astype(np.float64)], axis=1)
            first = obj if first is None else first
        feat = feat / float(n)
        depth = np.stack([feat[:, 3], feat[:, 4], (first + 1).astype(np.float64)], axis=1).reshape(h, w, 3)
        return feat[:, 0:3].reshape(h, w, 3), depth
    return batch_at, planes_at
