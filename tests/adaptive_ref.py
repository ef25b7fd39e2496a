"""Adaptive sampling by tile (include/rpt_hip.h), restated in numpy: the buffer whose tiles hold different numbers of batches -- tile
add, per-tile image, variance and mean -- and the tile errors in the stated tree order with the selection.  Every operation below is
one IEEE fp64 operation on arrays, in the order the header states, so the kernels of rpt_amd/csrc/adaptive.hip are compared with it
bit for bit (tests/test_gpu_adaptive.py); tests/test_adaptive_host.py holds it to a slot-by-slot transcription of the definition.

Test infrastructure: not part of the product."""
import numpy as np

from rpt_amd import color_bytes

TILE = 32


def tile_grid(w, h):
    """-> (tiles_x, tiles_y)"""
    return (w + TILE - 1) // TILE, (h + TILE - 1) // TILE


def tile_pixels(tile, w, h):
    """-> (ys, xs) of the in-image pixels of tile id ty * tiles_x + tx, as slices."""
    tx_n, _ = tile_grid(w, h)
    ty, tx = divmod(int(tile), tx_n)
    return slice(TILE * ty, min(TILE * ty + TILE, h)), slice(TILE * tx, min(TILE * tx + TILE, w))


def pixel_counts(tile_counts, w, h):
    """(tiles_y, tiles_x) batch counts -> (h, w): n_p of every pixel."""
    return np.repeat(np.repeat(np.asarray(tile_counts), TILE, axis=0), TILE, axis=1)[:h, :w]


class RefBuffer:
    """The running sums of rpt_buffer: `total` (h, w, 3), `sumsq` (h, w), n_batches full-frame batches and `extra` (tiles_y,
    tiles_x) batches per tile."""

    def __init__(self, w, h, radius=0):
        self.w, self.h, self.radius = int(w), int(h), int(radius)
        self.total, self.sumsq = np.zeros((h, w, 3)), np.zeros((h, w))
        tx, ty = tile_grid(w, h)
        self.n_batches, self.extra = 0, np.zeros((ty, tx), dtype=np.uint32)

    @staticmethod
    def _add(total, sumsq, b):
        total += b                                                    # (each channel: sum = sum + b)
        sumsq += (b[..., 0] * b[..., 0] + b[..., 1] * b[..., 1]) + b[..., 2] * b[..., 2]

    def add(self, batch):
        """rpt_buffer_add_samples*: a full-frame batch."""
        self._add(self.total, self.sumsq, np.asarray(batch, dtype=np.float64).reshape(self.h, self.w, 3))
        self.n_batches += 1

    def add_tiles(self, batch, tiles):
        """rpt_buffer_add_samples_tiles_device: the same arithmetic on the in-image pixels of the listed tiles (distinct ids)."""
        batch = np.asarray(batch, dtype=np.float64).reshape(self.h, self.w, 3)
        assert len(set(int(t) for t in tiles)) == len(tiles)
        for t in tiles:
            ys, xs = tile_pixels(t, self.w, self.h)
            self._add(self.total[ys, xs], self.sumsq[ys, xs], batch[ys, xs])   # (views: in place)
            self.extra.reshape(-1)[int(t)] += 1

    def tile_batches(self):
        return (self.extra + np.uint32(self.n_batches)).astype(np.uint32)

    def counts(self):
        return pixel_counts(self.tile_batches(), self.w, self.h)

    def mean(self):
        """rpt_buffer_mean_device with n = double(n_p) -> (rgb (h, w, 3), var (h, w))."""
        n = self.counts().astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            m = self.total / n[..., None]
            ss = self.sumsq - n * ((m[..., 0] * m[..., 0] + m[..., 1] * m[..., 1]) + m[..., 2] * m[..., 2])
            return m, np.fmax(ss, 0.0) / (n - 1.0) / n

    def variance(self):
        """rpt_buffer_variance: its per-pixel expression with n = double(n_p), summed in pixel order, over the pixels."""
        n = self.counts().astype(np.float64)
        m = self.total / n[..., None]
        ss = self.sumsq - n * (m[..., 0] * m[..., 0] + m[..., 1] * m[..., 1] + m[..., 2] * m[..., 2])
        acc = 0.0
        for v in (np.fmax(ss, 0.0) / (n - 1.0)).reshape(-1).tolist():
            acc += v
        return acc / float(self.w * self.h)

    def filtered(self):
        """get_filtered_color (src/buffer.rs:75-93): the clipped window's sums, x outer and y inner, over the window's sample count."""
        r, h, w = self.radius, self.h, self.w
        pad = np.zeros((h + 2 * r, w + 2 * r, 3))                     # (a pixel outside the image adds +0.0: no change)
        pad[r:r + h, r:r + w] = self.total
        cnt = np.zeros((h + 2 * r, w + 2 * r), dtype=np.int64)
        cnt[r:r + h, r:r + w] = self.counts()
        acc, cacc = np.zeros((h, w, 3)), np.zeros((h, w), dtype=np.int64)
        for dx in range(2 * r + 1):
            for dy in range(2 * r + 1):
                acc = acc + pad[dy:dy + h, dx:dx + w]
                cacc = cacc + cnt[dy:dy + h, dx:dx + w]
        return acc / cacc.astype(np.float64)[..., None]

    def image(self):
        return color_bytes(self.filtered())

    def tile_errors(self, floor):
        return tile_errors(self.total, self.sumsq, self.tile_batches(), floor)


def tile_errors(total, sumsq, tile_counts, floor):
    """E_t of every tile -> (tiles_y, tiles_x).  Slot j = 32 ry + rx of tile (tx, ty) is pixel (32 tx + rx, 32 ty + ry); slots outside
    the image hold +0.0; the 1024 terms are reduced by halving strides."""
    h, w = sumsq.shape
    tx_n, ty_n = tile_grid(w, h)
    floor = float(floor)
    n = pixel_counts(tile_counts, w, h).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        m = total / n[..., None]
        ss = sumsq - n * ((m[..., 0] * m[..., 0] + m[..., 1] * m[..., 1]) + m[..., 2] * m[..., 2])
        v = np.fmax(ss, 0.0) / (n - 1.0) / n
        y = (m[..., 0] + m[..., 1]) + m[..., 2]
        a = v / (y * y + floor * floor)
    slots = np.zeros((ty_n * TILE, tx_n * TILE))
    slots[:h, :w] = a
    # (ty, ry, tx, rx) -> (ty, tx, 32 ry + rx)
    t = slots.reshape(ty_n, TILE, tx_n, TILE).transpose(0, 2, 1, 3).reshape(ty_n, tx_n, TILE * TILE).copy()
    s = TILE * TILE // 2
    with np.errstate(invalid="ignore"):
        while s >= 1:
            t[..., :s] = t[..., :s] + t[..., s:2 * s]
            s //= 2
    inside = np.minimum(TILE, w - TILE * np.arange(tx_n))[None, :] * np.minimum(TILE, h - TILE * np.arange(ty_n))[:, None]
    with np.errstate(invalid="ignore"):
        return t[..., 0] / inside.astype(np.float64)


def select(errors, tile_counts, threshold, max_batches):
    """The ids of the selected tiles, ascending: E_t > threshold threshold (false for NaN) and n_t < max_batches."""
    thr2 = float(threshold) * float(threshold)
    with np.errstate(invalid="ignore"):
        keep = (np.asarray(errors).reshape(-1) > thr2) & (np.asarray(tile_counts).reshape(-1) < int(max_batches))
    return np.flatnonzero(keep).astype(np.uint32)
