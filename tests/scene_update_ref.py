"""The records of a sphere under translate(c) * scale(r, r, r), restated in numpy one rounded operation at a time: what
rpt_amd/csrc/scene_update_core.h states for the device and what the flattener computes for the matrix diag(r, r, r | c).  fp64 scalars
for the matrices, then the fp32 roundings and nextafter.  Also the scene tree's refit (union, then the builder's padding) on the arrays
rpt_debug_scene_records hands out.  Shared by tests/test_scene_update_host.py and tests/test_gpu_scene_update.py."""
import numpy as np

F64, F32 = np.float64, np.float32
IDENTITY_RECORD = np.zeros(24)
IDENTITY_RECORD[[0, 5, 10, 12, 16, 20]] = 1.0

NODE = np.dtype([("lo0", "<f4", 3), ("e0", "<u4"), ("hi0", "<f4", 3), ("pad0", "<u4"), ("lo1", "<f4", 3), ("e1", "<u4"), ("hi1", "<f4", 3), ("pad1", "<u4")])
ENTRY = np.dtype([("lo", "<f4", 3), ("a", "<u4"), ("hi", "<f4", 3), ("b", "<u4")])
TABLE = np.dtype([("sph", "<u4"), ("object", "<u4"), ("rec64", "<u4"), ("reserved", "<u4"), ("radius", "<f8"), ("centre", "<f8", 3)])
CULL = np.dtype([("lo", "<f4", 3), ("unbounded", "<u4"), ("hi", "<f4", 3), ("slab_test", "<u4")])
NONE, INNER = 0xFFFFFFFF, 0xFFFFFFFE
# which: the arrays of rpt_debug_scene_records
SPH, SPH_SHADE, PBOX, TREE_NODES, RECS, SHADE, CULLS, CULL32, TREE_RAW, TREE_ENTRIES, TREE_ORDER, ITEM_BOXES, MOVABLE_TABLE = range(13)


def matrix(r, c):
    m = np.diag([r, r, r, 1.0]).astype(F64)
    m[:3, 3] = c
    return m


def _std_min(a, b):   # std::min(a, b): b if b < a else a
    return b if b < a else a


def _std_max(a, b):
    return b if a < b else a


def sphere_records(r, c):
    """dict of the records of part 1 for radius r and centre c: scan (12 f32), shade_n (f32), item_lo / item_hi, pbox_lo / pbox_hi (f32 x 3),
    inv (12 f64), nrm (f64), cull_lo / cull_hi (f32 x 3), unbounded."""
    with np.errstate(all="ignore"):
        r = F64(r)
        c = [F64(x) for x in c]
        zero, one = F64(0.0), F64(1.0)
        # invert4 on [M | I]: rows 0..2 divided by their pivot r, then f = c[k] / r times row 3 = (0 0 0 1 | 0 0 0 1) taken off if f != 0
        z, d = zero / r, one / r
        inv = []
        for k in range(3):
            f = c[k] / r
            for j in range(4):
                m = d if j == k else z
                if f != 0.0:
                    m = m - f * (one if j == 3 else zero)
                inv.append(m)
        # finish_xf: the determinant and the inverse transpose of diag(r, r, r) by the cofactor formulas
        det = r * (r * r - zero * zero) - zero * (zero * r - zero * zero) + zero * (zero * zero - r * zero)
        n = (r * r - zero * zero) / det
        out = {"inv": np.array(inv, dtype=F64), "nrm": n, "det": det}
        out["scan"] = np.array([F32(v) for v in inv], dtype=F32)
        out["shade_n"] = F32(n)
        # xf_box(.., sphere)
        lo, hi = [], []
        for i in range(3):
            h = zero
            for j in range(3):
                m = r if i == j else zero
                h = h + m * m
            h = np.sqrt(h)
            h = h + F64(1e-5) * (h + abs(c[i]))
            lo.append(F32(c[i] - h))
            hi.append(F32(c[i] + h))
        out["item_lo"], out["item_hi"] = np.array(lo, dtype=F32), np.array(hi, dtype=F32)
        # push_box
        plo, phi = [], []
        for a in range(3):
            pad = F32(1e-5) * (abs(lo[a]) + abs(hi[a]) + (hi[a] - lo[a])) + F32(1e-7)
            plo.append(lo[a] - pad)
            phi.append(hi[a] + pad)
        out["pbox_lo"], out["pbox_hi"] = np.array(plo, dtype=F32), np.array(phi, dtype=F32)
        # cull_box64 of a transformed sphere
        fwd = [[r if i == j else zero for j in range(3)] + [c[i]] for i in range(3)]
        wlo, whi = [F64(np.inf)] * 3, [F64(-np.inf)] * 3
        for corner in range(8):
            p = [one if corner & 1 else -one, one if corner & 2 else -one, one if corner & 4 else -one]
            for i in range(3):
                w = fwd[i][0] * p[0] + fwd[i][1] * p[1] + fwd[i][2] * p[2] + fwd[i][3]
                wlo[i] = _std_min(wlo[i], w)
                whi[i] = _std_max(whi[i], w)
        size, mag = zero, zero
        for i in range(3):
            size = _std_max(size, whi[i] - wlo[i])
            mag = _std_max(mag, _std_max(abs(wlo[i]), abs(whi[i])))
        pad = F64(1e-5) * size + F64(1e-5) * mag + F64(1e-30)
        clo = np.array([np.nextafter(F32(wlo[i] - pad), F32(-np.inf)) for i in range(3)], dtype=F32)
        chi = np.array([np.nextafter(F32(whi[i] + pad), F32(np.inf)) for i in range(3)], dtype=F32)
        finite = bool(np.all(np.isfinite(clo)) and np.all(np.isfinite(chi)))
        out["unbounded"] = 0 if finite else 1
        out["cull_lo"] = clo if finite else np.zeros(3, dtype=F32)
        out["cull_hi"] = chi if finite else np.zeros(3, dtype=F32)
    return out


def _cofactors3(m):
    k = [[None] * 3 for _ in range(3)]
    k[0][0] = m[1][1] * m[2][2] - m[1][2] * m[2][1]; k[0][1] = m[0][2] * m[2][1] - m[0][1] * m[2][2]; k[0][2] = m[0][1] * m[1][2] - m[0][2] * m[1][1]
    k[1][0] = m[1][2] * m[2][0] - m[1][0] * m[2][2]; k[1][1] = m[0][0] * m[2][2] - m[0][2] * m[2][0]; k[1][2] = m[0][2] * m[1][0] - m[0][0] * m[1][2]
    k[2][0] = m[1][0] * m[2][1] - m[1][1] * m[2][0]; k[2][1] = m[0][1] * m[2][0] - m[0][0] * m[2][1]; k[2][2] = m[0][0] * m[1][1] - m[0][1] * m[1][0]
    return (m[0][0] * k[0][0] + m[0][1] * k[1][0]) + m[0][2] * k[2][0], k


def sphere_motion_record(r, c, p):
    """The 24 doubles of rpt_temporal_motion_record(T(c) S(r), T(p) S(r)) in the header's order, or None where it refuses."""
    with np.errstate(all="ignore"):
        r = F64(r)
        c = [F64(x) for x in c]
        p = [F64(x) for x in p]
        zero = F64(0.0)
        if not np.isfinite(r) or not all(np.isfinite(x) for x in c + p):
            return None
        cur = [[r if i == j else zero for j in range(3)] for i in range(3)]
        det, k = _cofactors3(cur)
        if det == 0.0 or not np.isfinite(det):
            return None
        if all(c[i] == p[i] for i in range(3)):
            return IDENTITY_RECORD.copy()
        out = np.zeros(24)
        inv = [[k[i][j] / det for j in range(3)] for i in range(3)]
        u = [-((inv[i][0] * c[0] + inv[i][1] * c[1]) + inv[i][2] * c[2]) for i in range(3)]
        a = [[None] * 3 for _ in range(3)]
        for i in range(3):
            row = [r if i == j else zero for j in range(3)] + [p[i]]
            for j in range(3):
                a[i][j] = out[4 * i + j] = (row[0] * inv[0][j] + row[1] * inv[1][j]) + row[2] * inv[2][j]
            out[4 * i + 3] = ((row[0] * u[0] + row[1] * u[1]) + row[2] * u[2]) + row[3]
        det_a, k = _cofactors3(a)
        if det_a == 0.0 or not np.isfinite(det_a):
            return None
        for i in range(3):
            for j in range(3):
                out[12 + 3 * i + j] = k[j][i] / det_a
        return out


# ---- the scene tree's refit on the downloaded arrays
def pad_node_box(lo, hi):
    """BvhBuilder::build's padding of a node box, fp32: 1e-6 of the larger magnitude + 1e-30 per axis."""
    lo, hi = np.asarray(lo, dtype=F32), np.asarray(hi, dtype=F32)
    pad = F32(1e-6) * np.maximum(np.abs(lo), np.abs(hi)) + F32(1e-30)
    return (lo - pad).astype(F32), (hi + pad).astype(F32)


def check_order(entries, order):
    """The height lists as one sequence: a permutation of the nodes in which every inner child comes before its parent."""
    n = len(entries) // 2
    assert sorted(order.tolist()) == list(range(n))
    place = np.empty(n, dtype=np.int64)
    place[order] = np.arange(n)
    for node in range(n):
        for side in range(2):
            e = entries[2 * node + side]
            if e["a"] == INNER:
                assert place[int(e["b"])] < place[node], (node, side)


def refit(entries, order, items):
    """(raw, boxes): per entry the unpadded bounds (n_entries, 2, 3) and the padded box a node holds, from the fixed boxes, the movable
    spheres' item boxes (n, 2, 4) and the children's bounds, in `order`."""
    raw = np.zeros((len(entries), 2, 3), dtype=F32)
    for node in order.tolist():
        for side in range(2):
            e = entries[2 * node + side]
            if e["a"] == INNER:
                ch = raw[2 * int(e["b"]):2 * int(e["b"]) + 2]
                lo, hi = np.minimum(ch[0, 0], ch[1, 0]), np.maximum(ch[0, 1], ch[1, 1])
            else:
                lo, hi = e["lo"].copy(), e["hi"].copy()
                for m in (int(e["a"]), int(e["b"])):
                    if m != NONE:
                        lo, hi = np.minimum(lo, items[m, 0, :3]), np.maximum(hi, items[m, 1, :3])
            raw[2 * node + side, 0], raw[2 * node + side, 1] = lo, hi
    boxes = np.zeros_like(raw)
    for i in range(len(raw)):
        boxes[i, 0], boxes[i, 1] = pad_node_box(raw[i, 0], raw[i, 1])
    return raw, boxes


def node_boxes(nodes):
    """The (n_entries, 2, 3) boxes of downloaded nodes, entry 2 i + side."""
    out = np.zeros((2 * len(nodes), 2, 3), dtype=F32)
    out[0::2, 0], out[0::2, 1], out[1::2, 0], out[1::2, 1] = nodes["lo0"], nodes["hi0"], nodes["lo1"], nodes["hi1"]
    return out
