"""The photon shooting pass chain by chain: what to demand of a computation that makes decisions (CPU only: numpy + the oracle).

Photon i of a map draws from the streams (seed, i, 0x80000000 + (i >> 32)) and (seed, i, 0xC0000000 + (i >> 32)) in the library and in
the oracle alike, and both keep their records in shooting order, so the library's chain i can be held against the oracle's chain i:
`OracleScene.photon_chains` (orc_photon_chains) shoots single chains with orc_photon_map_build's streams and power and reports, per
photon, the record counts, the records, a signature of the chain's decisions -- per vertex: volume event and the side of y = 250,
surface hit and the object, or miss; what ended the chain (absorbed at 0.7, sample_f None, medium roulette, escape); the sign of wi.n
behind `cosine_term`; the two record counts after thinning -- and the rows the bound below is computed from.

The rule is the one of tests/ray_cloud.py and tests/photon_ref.py.  A chain decides things (which object, hit or escape, volume event
or surface), and on a ray that lies on such a boundary fp32 (or fp64) and the oracle's fp64 may decide differently and both be right.
So the oracle is asked about a cloud: the chain itself and 12 more in which every vertex's ray is displaced, the origin by
amp (1 + max|o|) xi and the direction by amp xi, xi uniform in [-1, 1]^3 from a generator keyed by (member, photon index);
amp = MODES[mode]["amp"] (2e-6 with the oracle's robust policy for the fp32 kernels, 1e-14 with the literal policy for the
reference-epsilon mode).  The chain's own streams are untouched.

  * A chain is DECIDED when its 13 signatures are equal.  The library's counts must then equal the reference's, and every record k --
    position, direction (beam-beam volume records: the beam's start), power; surface and volume arrays separately -- must lie in the
    per-component range of the 13 values, widened by the bound below.
  * An undecided chain gets 58 more members (71 in all, photon_ref.py's count).  The library's chain must have the counts of one
    signature among the 71 and lie in the widened range of the members that share it.  A chain that fits no signature fails.
  * No quantile, no chain left out.

The bound -- an error model of photon_shoot_kernel (photon.hip) and photon_shoot_f64_kernel (kernels_f64.hip) made of bounds the suite
already states, written down before the first run on a device.  u = 2^-24 (fp32) or 2^-53 (reference-epsilon mode).  Per vertex j of
the reference chain (vertex 0 is the emission), L_j the length of the segment that ends there:

  D_j   bound of the direction that leaves vertex j (the next record's direction is its negative, normalised: + 3 u)
          surface    the `wi` bound of tests/test_gpu_device_materials.py for the vertex's material: fp32 5e-5, Phong
                     + min(1.8e-7 / st, 6e-4), glass refracted + min(sqrt(dk), dk / (2 sqrt(k))), dk = 3e-7 eta^2; fp64 1e-12.  That
                     bound is for exact inputs; here wo carries D_(j-1), which a mirror and a Phong lobe hand on one to one and glass
                     times max(eta, 1): + g D_(j-1), g = 0 for a Lambertian surface (wi does not depend on wo).
          medium     4 u: normalize of three draws ("a few u")
          emission   the direction is sample_f's Lambertian form -- (st cos, ct, st sin) through v_cos_f32 / v_sin_f32 and
                     rotate_from_y -- so the 5e-5 (1e-12) of `wi` covers the instructions; two terms it does not cover:
                     (a) st = sqrt(1 - ct^2) with ct = 1 - u2 exact: one rounding of ct^2 (<= u) ahead of a cancelling subtraction, so
                         st is off by at most min(u / (2 st), sqrt(u)) (the Phong term's derivation with one rounding instead of three);
                     (b) the emitter's normal n is itself a result: test_gpu_device_samplers.py bounds it by 5e-5 m (1e-12), m =
                         1 / (16 z)^2 on the rim of a sphere (local z < 1/16), else 1.  R(n) v, the rotation that takes Y to n, moves
                         by |dn| when n moves along its meridian and by 2 |dn| / s when it moves around the pole, s = sqrt(n.x^2 +
                         n.z^2) (the axis Y x n turns by |dn| / s, and a turn of the axis by a moves the image by at most 2 a):
                         + 5e-5 m (1 + 2 / s); for s below 1e-12 both sides take the fallback at the pole and the term is 5e-5 m.
  P_j   bound of the position of vertex j:  P_0 = 2e-5 (1 + |v|) m  (test_gpu_device_samplers.py's `v`; fp64 1e-12 (1 + |v|)),
        P_j = P_(j-1) + L_j (b_t + D_(j-1)) + 2 u (max|o| + L_j):  b_t of ray_cloud.MODES times the segment length as the issue
        states it; L_j D_(j-1) because the hit point is o + t d and d carries the direction's bound (without it a Phong bounce's 6e-4
        would have to hide in b_t = 2e-4); 2 u |x| for o + t d formed and kept in the working precision.  A beam's start is the position
        of the vertex before.
  K_j   relative bound of the power that arrives at vertex j:  K_1 = 2 u (power x colour), K_(j+1) = K_j + k_j with
          surface    k_j = the `k` bound of test_gpu_device_materials.py: D_j |n|_1 / (wi.n) for the cosine (wi.n > 0 only: otherwise
                     cosine_term is the constant 1) + f's bound (fp32 1e-6, Phong + W(c)) + pdf's bound (2e-4, Phong + W(c)),
                     W(c) = shininess (4e-7 / c + 2^-22 |log2 c|); fp64 1e-12 each; + 3 u for the products.  Where wi.n <= D_j |n|_1
                     the cosine's relative error has no bound: the rest of that chain's powers are not bounded (its counts, positions
                     and directions still are); the sign of wi.n is part of the signature.
          medium     4 u
        A kept beam's x 1000: + u.
  Reference-epsilon mode: directions, powers and volume positions (beam starts too) are stored as floats: + 2^-24 |value|.  Surface
  positions are compared in fp64 (rpt_debug_photon_positions64) without it.

What the bound leaves to the cloud: that a displaced hit point has another normal (curved surfaces), and every decision."""
import functools

import numpy as np

from tests.ray_cloud import MODES

N_FIRST, N_MORE = 12, 58
U32 = 2.0 ** -24
ROW = 12
WI, PDF, F, V_LIGHT, NRM = {"fp32": 5e-5, "fp64": 1e-12}, {"fp32": 2e-4, "fp64": 1e-12}, {"fp32": 1e-6, "fp64": 1e-12}, \
    {"fp32": 2e-5, "fp64": 1e-12}, {"fp32": 5e-5, "fp64": 1e-12}


def _excl(c):
    out = np.zeros(len(c), dtype=np.int64)
    np.cumsum(c[:-1], out=out[1:])
    return out


def _segments(first, count):
    """Indices first[i] .. first[i] + count[i] - 1 of every i, concatenated."""
    count = count.astype(np.int64)
    total = int(count.sum())
    return np.repeat(first.astype(np.int64) - _excl(count), count) + np.arange(total, dtype=np.int64)


def row_bounds(rows, nrows, mode):
    """Per row of the chains (rows: (T, 12), nrows per chain): P (position of the vertex), D_in (direction that arrives), K_in (relative,
    power that arrives), P_prev (position of the vertex before: a beam's start)."""
    u = U32 if mode == "fp32" else 2.0 ** -53
    b_t = MODES[mode]["b_t"]
    T = rows.shape[0]
    P, D, K_out = np.zeros(T), np.zeros(T), np.zeros(T)
    D_in, K_in, P_prev = np.zeros(T), np.zeros(T), np.zeros(T)
    start = _excl(nrows)
    code, end, L, omax, kind, cw, n1, a1, a2, a3 = (rows[:, k] for k in (0, 2, 3, 4, 6, 7, 8, 9, 10, 11))
    with np.errstate(divide="ignore", invalid="ignore"):
        # emission rows
        e = start[nrows > 0]
        z, s, st = a1[e], a2[e], cw[e]
        m = np.where(z < 1.0 / 16.0, 1.0 / (16.0 * z) ** 2, 1.0) if mode == "fp32" else np.ones(len(e))
        P[e] = V_LIGHT[mode] * (1.0 + a3[e]) * m
        D[e] = WI[mode] + np.minimum(u / (2.0 * st), np.sqrt(u)) + NRM[mode] * m * np.where(s > 1e-12, 1.0 + 2.0 / s, 1.0)
        K_out[e] = 2.0 * u
        for d in range(1, int(nrows.max()) if len(nrows) else 0):
            j = start[nrows > d] + d
            p = j - 1
            P_prev[j] = P[p]
            P[j] = P[p] + L[j] * (b_t + D[p]) + 2.0 * u * (omax[j] + L[j])
            D_in[j], K_in[j] = D[p] + 3.0 * u, K_out[p]
            vol = code[j] == 1
            D[j[vol]] = 4.0 * u
            K_out[j[vol]] = K_in[j[vol]] + 4.0 * u
            sf = j[(code[j] == 2) & (end[j] == 0)]
            ps = sf - 1
            own = np.full(len(sf), WI[mode])
            w = np.zeros(len(sf))
            g = np.where(kind[sf] == 0, 0.0, 1.0)
            if mode == "fp32":
                ph = kind[sf] == 1
                own = own + np.where(ph, np.minimum(1.8e-7 / np.sqrt(np.maximum(1.0 - a1[sf] ** 2, 0.0)), 6e-4), 0.0)
                w = np.where(ph, np.where(a1[sf] > 0, a2[sf] * (4e-7 / a1[sf] + 2.0 ** -22 * np.abs(np.log2(a1[sf]))), np.inf), 0.0)
                gl = (kind[sf] == 3) & (a3[sf] == 1)
                dk = 3e-7 * a1[sf] ** 2
                own = own + np.where(gl, np.minimum(np.sqrt(dk), dk / (2.0 * np.sqrt(np.maximum(a2[sf], 0.0)))), 0.0)
            g = np.where(kind[sf] == 3, np.maximum(a1[sf], 1.0), g)
            D[sf] = own + g * D[ps]
            dc = D[sf] * n1[sf]
            cosine = np.where(cw[sf] > 0, np.where(cw[sf] > dc, dc / cw[sf], np.inf), 0.0)
            K_out[sf] = K_in[sf] + cosine + F[mode] + PDF[mode] + 2.0 * w + 3.0 * u
    return P, D_in, K_in, P_prev


def record_bounds(rows, nrows, mode, kind):
    """-> (surface, volume): per record of the chains, in order, (pos, dir, pow relative) bounds, each (n_records, 3)."""
    P, D_in, K_in, P_prev = row_bounds(rows, nrows, mode)
    u = U32 if mode == "fp32" else 2.0 ** -53
    s, v = rows[:, 5] == 1, rows[:, 5] == 2
    surf = np.stack([P[s], D_in[s], K_in[s]], axis=1)
    vol = np.stack([P[v], P_prev[v] if kind == 2 else D_in[v], K_in[v] + (u if kind == 2 else 0.0)], axis=1)
    return surf, vol


def _absolute(b, lo, hi, mode, which):
    """(n, 3) bounds -> (n, 9) absolute ones on the records whose cloud range is lo..hi."""
    big = np.maximum(np.abs(lo), np.abs(hi))
    out = np.empty_like(big)
    out[:, 0:3] = b[:, 0:1]
    out[:, 3:6] = b[:, 1:2]
    out[:, 6:9] = np.where(big[:, 6:9] > 0, b[:, 2:3] * big[:, 6:9], 0.0)      # (inf * 0: a zero power stays exact)
    if mode == "fp64":
        out[:, 3:9] += U32 * big[:, 3:9]
        if which == 1:
            out[:, 0:3] += U32 * big[:, 0:3]
    return out


def _ratio(x, lo, hi, bound):
    ex = np.maximum(np.maximum(lo - x, x - hi), 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(ex == 0, 0.0, ex / bound)
    return np.where(np.isnan(r), np.inf, r)


class Reference:
    """The clouds of photons first .. first + n - 1 (see the module docstring).  members[m]: the oracle's answer for cloud member m over
    all photons (m = 0: the chain itself, with rows); decided: (n,) bool; groups[i] for an undecided photon i (relative index):
    {signature: {"ns", "nv", "surface": [(ns, 9)...], "volume": [...], "bounds": (surface (ns, 3), volume (nv, 3))}}."""

    def __init__(self, osc, args, mode, kind, seed, second_pass=True):
        self.mode, self.kind, self.n, self.first = mode, kind, int(args["n"]), int(args["first"])
        cfg = MODES[mode]
        self._shoot = lambda m, **kw: osc.photon_chains(args["photon_count"], kind, args["watts"], seed=seed, robust=cfg["robust"],
                                                        amp=0.0 if m == 0 else cfg["amp"], cloud_seed=m, **kw)
        self.members = [self._shoot(m, first=self.first, n=self.n, verts=(m == 0)) for m in range(N_FIRST + 1)]
        sig0 = self.members[0]["sig"]
        self.decided = np.all([mb["sig"] == sig0 for mb in self.members], axis=0)
        self.bounds = record_bounds(self.members[0]["rows"], self.members[0]["nrows"], mode, kind)
        self.groups = {}
        if second_pass:
            self._second_pass()

    def _second_pass(self):
        und = np.flatnonzero(~self.decided)
        if und.size == 0:
            return
        self.groups = {int(i): {} for i in und}
        for m in range(N_FIRST + 1 + N_MORE):
            mb = self._shoot(m, indices=und.astype(np.uint64) + np.uint64(self.first), verts=True)
            bs, bv = record_bounds(mb["rows"], mb["nrows"], self.mode, self.kind)
            os_, ov_ = _excl(mb["ns"]), _excl(mb["nv"])
            for k, i in enumerate(und):
                ns, nv = int(mb["ns"][k]), int(mb["nv"][k])
                g = self.groups[int(i)].setdefault(int(mb["sig"][k]), {"ns": ns, "nv": nv, "surface": [], "volume": [],
                                                                        "bounds": (bs[os_[k]:os_[k] + ns], bv[ov_[k]:ov_[k] + nv])})
                g["surface"].append(mb["surface"][os_[k]:os_[k] + ns, :9])
                g["volume"].append(mb["volume"][ov_[k]:ov_[k] + nv, :9])

    def counts(self):
        return self.members[0]["ns"], self.members[0]["nv"]


@functools.lru_cache(maxsize=None)
def reference_for(family, mode, kind):
    """The Reference of a case of tests/photon_chain_cases.py: computed once, shared by every test that needs it, not to be changed."""
    from oracle.pyoracle import OracleScene
    from tests import photon_chain_cases as cases
    return Reference(OracleScene(cases.scene(family)), cases.shoot_args(family, kind), mode, kind, cases.SEED)


NAMES = ("surface position", "surface direction", "surface power", "volume position", "volume direction", "volume power")


def check(ref, cnt_s, cnt_v, surface, volume):
    """The rule.  cnt_s, cnt_v: the library's records per photon; surface, volume: its records, (., >= 9) in shooting order (position,
    direction or beam start, power).  -> (failures: list of str, worst: {quantity: (error / bound, photon index, record of the chain)},
    {"decided": share, "undecided": count})."""
    fails, worst = [], {k: (0.0, -1, -1) for k in NAMES}
    dev = (np.asarray(surface, np.float64)[:, :9], np.asarray(volume, np.float64)[:, :9])
    cnt = (np.asarray(cnt_s).astype(np.int64), np.asarray(cnt_v).astype(np.int64))
    if len(cnt[0]) != ref.n or len(cnt[1]) != ref.n:
        return [f"{len(cnt[0])} / {len(cnt[1])} counts for {ref.n} photons"], worst, {}
    for which in (0, 1):
        if cnt[which].sum() != len(dev[which]):
            fails.append(f"{'surface' if which == 0 else 'volume'}: the counts add up to {cnt[which].sum()}, the array holds {len(dev[which])} records")
    if fails:
        return fails, worst, {}
    off = (_excl(cnt[0]), _excl(cnt[1]))

    def note(which, r, photon, within):
        """r: (T, 9) ratios; photon, within: (T,) where they are."""
        for q in range(3):
            if r.shape[0] == 0:
                continue
            rq = r[:, 3 * q:3 * q + 3].max(axis=1)
            k = int(rq.argmax())
            name = NAMES[3 * which + q]
            if rq[k] > worst[name][0]:
                worst[name] = (float(rq[k]), int(photon[k]) + ref.first, int(within[k]))
            bad = np.flatnonzero(~(rq < 1.0))
            for b in bad[:4]:
                fails.append(f"photon {int(photon[b]) + ref.first} record {int(within[b])}: {name} {rq[b]:.3g} x its bound")
            if bad.size > 4:
                fails.append(f"... and {bad.size - 4} more {name} records")

    # ---- decided chains, all at once
    D = np.flatnonzero(ref.decided)
    key = ("ns", "nv")
    for which in (0, 1):
        c = ref.members[0][key[which]].astype(np.int64)
        wrong = D[cnt[which][D] != c[D]]
        for i in wrong[:6]:
            fails.append(f"photon {int(i) + ref.first} (decided): {cnt[which][i]} {'surface' if which == 0 else 'volume'} records, the reference has {c[i]}")
        if wrong.size > 6:
            fails.append(f"... and {wrong.size - 6} more decided chains with other counts")
        ok = D[cnt[which][D] == c[D]]
        name = "surface" if which == 0 else "volume"
        vals = np.stack([mb[name][_segments(_excl(mb[key[which]])[ok], c[ok]), :9] for mb in ref.members[:N_FIRST + 1]])
        lo, hi = vals.min(axis=0), vals.max(axis=0)
        base_idx = _segments(_excl(c)[ok], c[ok])
        bound = _absolute(ref.bounds[which][base_idx], lo, hi, ref.mode, which)
        x = dev[which][_segments(off[which][ok], c[ok])]
        photon = np.repeat(ok, c[ok])
        within = np.arange(len(photon)) - np.repeat(_excl(c[ok]), c[ok])
        note(which, _ratio(x, lo, hi, bound), photon, within)
    # ---- undecided chains, one by one: the counts of one signature, and inside the range of the members that share it
    for i, groups in ref.groups.items():
        mine = [dev[w][off[w][i]:off[w][i] + cnt[w][i]] for w in (0, 1)]
        best = None
        for g in groups.values():
            if (g["ns"], g["nv"]) != (int(cnt[0][i]), int(cnt[1][i])):
                continue
            rs = []
            for w, name in ((0, "surface"), (1, "volume")):
                vals = np.stack(g[name])
                lo, hi = vals.min(axis=0), vals.max(axis=0)
                rs.append(_ratio(mine[w], lo, hi, _absolute(g["bounds"][w], lo, hi, ref.mode, w)))
            top = max([float(r.max()) for r in rs if r.size] + [0.0])
            if best is None or top < best[0]:
                best = (top, rs)
        if best is None:
            have = sorted({(g["ns"], g["nv"]) for g in groups.values()})
            fails.append(f"photon {i + ref.first} (undecided): {int(cnt[0][i])} surface and {int(cnt[1][i])} volume records fit no signature of its cloud {have}")
            continue
        for w in (0, 1):
            r = best[1][w]
            note(w, r, np.full(r.shape[0], i), np.arange(r.shape[0]))
    return fails, worst, {"decided": float(ref.decided.mean()), "undecided": int((~ref.decided).sum())}


def report(title, worst, info):
    print(f"{title}: decided {info.get('decided', float('nan')):.4f} ({info.get('undecided', 0)} undecided); error / bound: " +
          ", ".join(f"{k} {v[0]:.3g} (photon {v[1]} record {v[2]})" for k, v in worst.items() if v[1] >= 0))


def as_device(ref_member, mode):
    """What a faultless library would hand back for the oracle's own chains: the records rounded to fp32 (fp64 mode: the surface
    positions kept) -> cnt_s, cnt_v, surface (n, 9) fp64, volume."""
    s = ref_member["surface"][:, :9].astype(np.float32).astype(np.float64)
    v = ref_member["volume"][:, :9].astype(np.float32).astype(np.float64)
    if mode == "fp64":
        s[:, 0:3] = ref_member["surface"][:, 0:3]
    return ref_member["ns"].copy(), ref_member["nv"].copy(), s, v
