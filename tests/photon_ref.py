"""The photon-map camera pass restated: numpy, fp64, brute force, one camera ray at a time (CPU only: numpy + the oracle's ray queries).

With hand-made photons a one-sample camera pass is a deterministic function of the camera ray: pixel p, sample s gets the ray of
`oracle.pyoracle.camera_rays`, its first hit comes from `OracleScene.intersect(robust=1)`, and the estimate is a closed formula over the
photons nearest to the hit point (surface) and over the photon spheres the ray passes through (beam x point):

  surface   (emission + sum_j clamp(w_j . n, 0, 1) f(n, wo, w_j) P_j) / (pi r^2) * exp(-sigma_t t)        (the last factor in a medium)
            j over the K photons nearest to x = o + t d (all of them when the map holds fewer), r^2 the largest of their squared
            distances, a photon left out when something lies between it and x: a hit of the ray photon -> x nearer than |x - p| (1 - 1e-3)
            that does not lie in x's own tangent plane (|(hit - x) . n| <= 1e-4 |x - p|) -- the policy of the fp32 kernels, which the
            oracle calls robust;
  beam      colour_medium * sum_i P_i phase (3 / pi) (1 - D_i / r_i^2)^2 / r_i^2 exp(-sigma_t s_i)
            i over the volume photons with s_i = (p_i - o) . d > 0, D_i = |o + s_i d - p_i|^2 < r_i^2 and, when the ray hits,
            |p_i - o| <= t; r_i the distance from p_i to its 10th nearest volume photon, itself included (the farthest one in a map
            of fewer than 10).

The nearest photons come from a full distance matrix, not from a tree.  `tests/test_photon_ref_host.py` pins this restatement to the
oracle's `photon_map_from_photons(...).render` (1e-12 relative: both are fp64).

The rule of comparison (`check`) is the one of `tests/ray_cloud.py`: the library is not asked to agree with one fp64 answer but with the
answers in a small neighbourhood of the query.  The cloud of a camera ray: the ray itself, and 12 more whose direction is moved by
AMP * off and whose query point (hit point) is moved by AMP (1 + max|x|) * off, off = the six axis offsets and six seeded ones in
[-1, 1]^3; AMP = 2e-6 is ray_cloud.py's fp32 amplitude.  Every cloud ray is answered from scratch (its own first hit, its own selection,
its own visibility and beam tests).  A cloud answer carries a signature of its decisions: hit object, the multiset of the selected
photons' payloads (two identical records are one payload), which of them are occluded, which volume photons contribute.  A pixel is
DECIDED when all 13 signatures are equal; the library's value must then lie inside the range of the 13 values widened by the fp32 bound
below.  An undecided pixel must lie in the widened range of the answers of one signature; as in ray_cloud.py such a pixel gets a second
pass at the same amplitude -- the 26 offsets {-1, 0, 1}^3 \\ {0} and 32 more seeded ones -- so that the answers of one signature span
the neighbourhood in every direction that does not change the decision (13 samples split over three signatures do not).  Non-finite
reference values (a map without surface photons: 0 / 0) must come back non-finite in the same way.  No quantile, no pixel left out.

The fp32 bound, per cloud answer and colour channel -- an error model of the device code (photon.hip: add_photon_term, gather_serve,
beam_estimate_photon_lanes, volume_estimate_sample_lanes), stated here before anything was measured; u = 2^-24:

  surface   B_s = exp(-sigma_t t) / (pi r^2) * sum_j P_j (f_j E_COS + c_j E_BSDF |f_j|)  +  |V_s| ((K + 16) u + E_EXP [in a medium])
            E_COS = 1e-6 absolute on the clamped cosine (the fp32 normal of a flat face, 3 roundings of the dot product); E_BSDF = 1e-6
            relative on f (the bound of test_gpu_device_materials.py's `_f_bound` for a Lambertian surface; only such materials are
            used here); K u for the sum of K non-negative terms by fma; 16 u for the distance (the roundings of p - x, three products,
            two sums: 4 u on r^2), rcp (1 ulp), 1 / pi and the three products that follow; E_EXP = 2e-6 on exp(-sigma_t t) (__expf
            and the rounding of its argument).  Where the query point lies is not part of the bound: that is the cloud's job.
  beam      B_b = sum_i A_i [2 tmp_i dt_i + dt_i^2 + tmp_i^2 (12 u + E_EXP)]  +  |V_b| (n_i + 8) u
            A_i = colour_medium P_i phase (3 / pi) exp(-sigma_t s_i) / r_i^2, tmp_i = 1 - D_i / r_i^2,
            dt_i = 6 u + (2 sqrt(D_i) |c_i| 10 u + (10 u |c_i|)^2) / r_i^2 with c_i = p_i - o: D_i is the squared length of the
            difference of two vectors of length ~|c_i|, each component carrying about 10 u |c_i| (4 sqrt(3) u from s_i d - c_i, 3 u from
            the unit direction); 6 u for r_i^2 (4 u from the radius kernel's distance, sqrt, the square, rcp); n_i contributing photons.
            The photon-per-lane form replaces exp(-sigma_t s) by exp(-sigma_t |c|) (1 + sigma_t (|c| - s)) and states "to fp32
            precision" (|c| - s <= r^2 / |c|): the model takes it at its word and has no term for it.

The other two kinds of map (`Restated(kind=0)` and `Restated(kind=2)`; kind 1 above is unchanged).  Both are restated literally from
the reference's loops, src/photon.rs:384-438 and :503-593, one camera ray at a time.

  point x point (kind 0, RPT_PHOTON_MAP), in a medium: the sampled distance d = -ln(xi) / sigma_t, xi the uniform of the sample's own
            stream right after the camera's draws (`camera_rays`' next_word; Medium::sample_d, the host test proves the stream and the
            draw).  When d < t, or nothing is hit:
              colour_medium * phase * sum_j P_j / ((4/3) pi r^3) / sigma_t * T(d) / (sigma_t T(d)),     T(s) = exp(-sigma_t s)
            j over the `gather_size_volume` volume photons nearest to x = o + d dir (all of them when the map holds fewer), r the
            largest of their distances; no visibility test.  Otherwise the surface estimate above times T(t) / T(d).  An empty
            volume map gives 0 / 0.
  beam x beam (kind 2, RPT_PHOTON_BEAM_BEAM): the volume list holds (end, start, power, radius).  Per beam, in the reference's
            order: it is looked at only when the ray hits the beam's own box (min/max of the two ends, widened per axis by
            radius * sqrt of the other two squared extents over their sum; t_far >= max(t_near, 0)) -- the only test that keeps
            a beam behind the eye out; with b = unit(end - start), l = start - o, u = unit(l x b), n = unit(b x u):
            tq = (n . l) / (n . d), left out when the ray hits and tq >= t; beam_t = b . (o + tq d - start), left out when
            beam_t < 0 or beam_t > |end - start|; dist = |o + tq d - (start + beam_t b)|, left out when dist >= radius; else
              sigma_t colour_medium P phase / sqrt(max(0, 1 - (d . b)^2)) T(tq) T(beam_t) (3 / pi) (1 - dist / radius)^2 / (2 radius)
            and the surface estimate times T(t) is added as for kind 1.  The radius is the record's (the reference's is the
            constant 3).  A comparison with NaN lets the beam through, as the reference's negated tests do.

The cloud of a kind-0 ray also moves the sampled distance: member c uses d + A_d s_c, s_c = clamp(off_x + off_y + off_z, -1, 1) and
A_d = FOG_K u max(1, -ln xi) / sigma_t, the bound that tests/test_gpu_device_samplers.py::test_medium_distance_matches_oracle states for
-__logf(xi) / sigma_t (FOG_K = 8.32); the query point x = o + d dir is moved by AMP (1 + max|x|) off like a hit point, and the branch is
taken with the moved d against the moved t.  Signatures gain: the branch and the multiset of the selected volume payloads (kind 0; in
the volume branch the hit object is not part of it), the set of contributing beams (kind 2).

The fp32 bounds of the two estimates, stated before any device value was looked at (photon.hip: gather_knn and the scale line of
photon_query_kernel<..., RPT_PHOTON_MAP>; visit_beam in volume_estimate_sample_lanes):

  point x point, volume branch   B_pp = |V| (Kv + 24) u
            Kv u for the sum of Kv non-negative powers; 8 u for r^3 = max_d2 sqrt(max_d2) (4 u on a squared distance as above, times
            3/2, sqrt, one product); 3 u for rcp((4/3) pi r^3) (the constant, the product, rcp); 2 u for rcp(sigma_t); 3 u for
            T(d) rcp(sigma_t T(d)) -- __expf's own error cancels, both factors hold the same tr_d --; 5 u for the phase constant and
            the four products of the scale line; 3 u for colour_medium, sum * colour and scale * (...).  Where x lies is the cloud's.
            Ties: photons whose squared distance from x lies within 8 u (relative) of the K-th's cannot be told apart from it in
            fp32 (the 4 u of each squared distance); when such a photon stays outside the selection the sum may hold any n of the
            band in place of the n it holds here: B_pp grows by scale * (the largest change of the band's sum of powers, per
            channel) and by 12 u |V| for r^3.  p-deep16 has such a band: 16 origin copies and two comb teeth 0.03 and 0.06 fp32
            ulp nearer to a query 4.5 away.
  point x point, surface branch  B_ps = B_s / T(d) + |V| (E_EXP max(1, sigma_t d) + 3 u)
            B_s the surface bound above (T(t) included); __expf(-sigma_t d): E_EXP while the argument is below 1, growing with the
            argument (its rounding and that of the product with log2 e are relative to it); rcp and two products.
  beam x beam   B_bb = sum_i A_i [2 tmp_i dtmp_i + dtmp_i^2 + tmp_i^2 R_i]  +  |V_b| (n_i + 8) u,      A_i = term_i / tmp_i^2
            L = |l|, h = |n . l| (the eye's distance from the beam's line), g = |qc - start|, qc = o + tq d:
            eps_n  = 8 u (1 + L / h)            direction error of u and n: l x b cancels down to a vector of length h
            dtq    = (L (eps_n + 3 u) + |tq| (eps_n + 3 u)) / |n . d| + 2 u |tq|        numerator, denominator, rcp and product
            dqc    = dtq + 2 u (max|o| + |tq|)                                          fma3(tq, rd, ro)
            dbt    = dqc + 8 u g                       beam_t: b carries 4 u (sqrt, rcp, product), the difference and the dot 4 u
            ddist  = dqc + dbt + 4 u |beam_t| + u max|start| + 2 u dist                 bc = fma3(beam_t, b, start), |qc - bc|
            dtmp_i = ddist / radius + 3 u                                               rcp(radius), product, 1 - ...
            R_i    = sigma_t (dtq + dbt) + E_EXP (max(1, sigma_t |tq|) + max(1, sigma_t |beam_t|)) + 8 u / (1 - (d . b)^2) + 16 u
            the two __expf as above; 1 - dd^2 cancels near parallel: dd carries 6 u absolute (b's 4 u, the dot), 1 - dd^2 twice
            that plus its own roundings, rsq halves the relative error: at most 8 u / (1 - dd^2); 16 u for rsq, rcp(2 radius),
            3 / pi, sigma_t, phase and the nine products of the weight line.
"""
import itertools

import numpy as np

from tests.ray_cloud import MODES

AMP = MODES["fp32"]["amp"]
U = 2.0 ** -24
E_COS, E_BSDF, E_EXP = 1e-6, 1e-6, 2e-6
N_SEEDED = 6
KNN_RADIUS = 10
TIE_POOL = 64           # how far beyond the K-th nearest a band of indistinguishable distances is followed
FOG_K = 2 * 4.16        # tests/test_gpu_device_samplers.py: |dmed sigma_t + ln xi| <= FOG_K u max(1, -ln xi)


def _offsets():
    rng = np.random.default_rng(11)
    return np.concatenate([np.zeros((1, 3)), np.eye(3), -np.eye(3), rng.uniform(-1.0, 1.0, (N_SEEDED, 3))])


OFFS = _offsets()
OFFS_MORE = np.concatenate([np.array([c for c in itertools.product((-1.0, 0.0, 1.0), repeat=3) if any(c)]),
                            np.random.default_rng(12).uniform(-1.0, 1.0, (32, 3))])


def word_uniform(word):
    """The oracle's uniform of one generator word: (2k + 1) 2^-24, k the word's top 23 bits (in (0, 1), exact in fp32)."""
    w = np.asarray(word).astype(np.uint64)
    return (((w >> np.uint64(9)) << np.uint64(1)) | np.uint64(1)).astype(np.float64) * 2.0 ** -24


def knn_radii(pos, k=KNN_RADIUS):
    """Distance from every position to its k-th nearest, itself included (the farthest one when there are fewer than k)."""
    pos = np.ascontiguousarray(pos, dtype=np.float64).reshape(-1, 3)
    n = len(pos)
    out = np.zeros(n)
    if n == 0:
        return out
    kk = min(k, n) - 1
    for i0 in range(0, n, 512):
        a = pos[i0:i0 + 512]
        d2 = (a[:, None, 0] - pos[None, :, 0]) ** 2 + (a[:, None, 1] - pos[None, :, 1]) ** 2 + (a[:, None, 2] - pos[None, :, 2]) ** 2
        out[i0:i0 + 512] = np.sqrt(np.partition(d2, kk, axis=1)[:, kk])
    return out


def _payload_weights(ph, seed, cols=9):
    """One random 64-bit weight per distinct (position, direction, power): identical records share theirs."""
    if len(ph) == 0:
        return np.zeros(0, dtype=np.uint64)
    _, inv = np.unique(ph[:, :cols], axis=0, return_inverse=True)
    inv = np.asarray(inv).reshape(-1)
    return np.random.default_rng(seed).integers(1, 2 ** 62, int(inv.max()) + 1, dtype=np.uint64)[inv]


def _nearest(P, X, k):
    """The k photons nearest to each of X -> indices (q, k) in the order (distance, index), squared distances (q, k)."""
    q, m = len(X), len(P)
    idx = np.zeros((q, k), dtype=np.int64)
    d2s = np.zeros((q, k))
    step = max(1, (1 << 22) // max(m, 1))
    for i0 in range(0, q, step):
        a = X[i0:i0 + step]
        d2 = (a[:, None, 0] - P[None, :, 0]) ** 2 + (a[:, None, 1] - P[None, :, 1]) ** 2 + (a[:, None, 2] - P[None, :, 2]) ** 2
        part = np.argpartition(d2, k - 1, axis=1)[:, :k] if k < m else np.broadcast_to(np.arange(m), (len(a), m)).copy()
        part.sort(axis=1)
        dp = np.take_along_axis(d2, part, axis=1)
        order = np.argsort(dp, axis=1, kind="stable")
        idx[i0:i0 + step] = np.take_along_axis(part, order, axis=1)
        d2s[i0:i0 + step] = np.take_along_axis(dp, order, axis=1)
    return idx, d2s


class Answers:
    """vals, bounds: (n, C, 3); sig: (n, C) uint64; column 0 is the camera ray itself.  decided: (n,) bool.  For the undecided pixels
    `again` (m,): vals2, bounds2, sig2 with the second pass appended, (m, C + 58 [, 3])."""

    def __init__(self, vals, bounds, sig, again=None, vals2=None, bounds2=None, sig2=None):
        self.vals, self.bounds, self.sig = vals, bounds, sig
        self.decided = (sig == sig[:, :1]).all(axis=1)
        self.again = np.zeros(0, dtype=np.int64) if again is None else again
        self.vals2, self.bounds2, self.sig2 = vals2, bounds2, sig2

    def cloud(self, i):
        """(vals, bounds, sig) of pixel i's whole cloud."""
        k = np.flatnonzero(self.again == i)
        if len(k):
            return self.vals2[k[0]], self.bounds2[k[0]], self.sig2[k[0]]
        return self.vals[i], self.bounds[i], self.sig[i]

    @property
    def value(self):
        return self.vals[:, 0]


class Restated:
    """The camera pass over the photon lists `surface` and `volume` ((n, 10): position, direction, power, -) in `scene`, gather size K.
    kind: the PhotonRenderKind of the map -- 1 beam x point (the default), 0 point x point with the volume gather size Kv, 2 beam x
    beam, whose volume list is (n, 10): end, start, power, radius."""

    def __init__(self, scene, camera, surface, volume, K, kind=1, Kv=3):
        from oracle.pyoracle import OracleScene
        from rpt_amd import Material, Medium, hex_color
        self.scene, self.camera, self.K, self.kind, self.Kv = scene, camera, int(K), int(kind), int(Kv)
        assert self.kind in (0, 1, 2)
        self.osc = OracleScene(scene)
        self.ps = np.ascontiguousarray(surface, dtype=np.float64).reshape(-1, 10)
        self.pv = np.ascontiguousarray(volume, dtype=np.float64).reshape(-1, 10)
        assert all(o.material_.kind == Material.LAMBERTIAN for o in scene.objects), "the bound models Lambertian surfaces"
        self.medium = scene.media[0] if scene.media else None
        self.sigma_t, self.phase, self.mcol = 0.0, 0.0, np.zeros(3)
        if self.medium is not None:
            assert self.medium.kind == Medium.HOMOGENEOUS_ISOTROPIC
            self.sigma_t = self.medium.absorption + self.medium.scattering
            self.phase = 1.0 / (4.0 * np.pi)
            self.mcol = np.asarray(hex_color(0xD2B48C), dtype=np.float64)
        self.radius = knn_radii(self.pv[:, :3]) if self.kind == 1 else self.pv[:, 9].copy()
        self.w_s, self.w_v = _payload_weights(self.ps, 5), _payload_weights(self.pv, 6, 10 if self.kind == 2 else 9)
        self.albedo = np.array([o.material_.color() for o in scene.objects], dtype=np.float64).reshape(-1, 3)
        self.emission = np.array([o.material_.emittance() * np.asarray(o.material_.color()) for o in scene.objects], dtype=np.float64).reshape(-1, 3)

    # ------------------------------------------------------------------ one batch of independent queries
    def _surface(self, x, n, wo, obj, t):
        """Surface estimate at the points x (normal n, direction to the eye wo, object obj, distance t along the camera ray)."""
        from oracle import pyoracle
        q, m = len(x), len(self.ps)
        k = min(self.K, m)
        T = np.exp(-self.sigma_t * t) if self.medium is not None else np.ones(q)
        em = self.emission[obj]
        if k == 0:
            with np.errstate(divide="ignore", invalid="ignore"):
                val = em * (1.0 / (np.pi * np.zeros(q)))[:, None] * T[:, None]
            return val, np.zeros((q, 3)), np.zeros(q, dtype=np.uint64)
        P, W, POW = self.ps[:, :3], self.ps[:, 3:6], self.ps[:, 6:9]
        sel, d2 = _nearest(P, x, k)
        r2 = d2.max(axis=1)
        pp = P[sel]                                                     # (q, k, 3)
        disp = x[:, None, :] - pp
        ln = np.sqrt((disp ** 2).sum(axis=2))
        safe = ln > 0.0
        dirv = np.where(safe[..., None], disp / np.where(safe, ln, 1.0)[..., None], np.array([0.0, 1.0, 0.0]))
        th, ob, _ = self.osc.intersect(pp.reshape(-1, 3), dirv.reshape(-1, 3), robust=1)
        th, ob = th.reshape(q, k), ob.reshape(q, k)
        hit = (ob >= 0) & safe
        hp = pp + np.where(hit, th, 0.0)[..., None] * dirv - x[:, None, :]
        own = np.abs((hp * n[:, None, :]).sum(axis=2)) <= 1e-4 * ln
        blocked = hit & ~own & (th < ln * (1.0 - 1e-3))
        wi = W[sel]
        c = np.clip((wi * n[:, None, :]).sum(axis=2), 0.0, 1.0)
        f = np.zeros((q, k, 3))
        for o_id in np.unique(obj):
            rows = np.flatnonzero(obj == o_id)
            nn = np.repeat(n[rows], k, axis=0)
            ww = np.repeat(wo[rows], k, axis=0)
            f[rows] = pyoracle.material_bsdf(self.scene.objects[o_id].material_, nn, ww, wi[rows].reshape(-1, 3)).reshape(len(rows), k, 3)
        vis = (~blocked)[..., None]
        terms = f * POW[sel] * c[..., None] * vis
        with np.errstate(divide="ignore", invalid="ignore"):
            scale = T / (np.pi * r2)
            val = (em + terms.sum(axis=1)) * (1.0 / (np.pi * r2))[:, None] * T[:, None]
            bound = scale[:, None] * (POW[sel] * (f * E_COS + c[..., None] * E_BSDF * np.abs(f)) * vis).sum(axis=1)
            bound = bound + np.abs(val) * ((k + 16) * U + (E_EXP if self.medium is not None else 0.0))
        sig = (self.w_s[sel] * np.where(blocked, np.uint64(3), np.uint64(1))).sum(axis=1, dtype=np.uint64)
        return val, np.where(np.isfinite(bound), bound, 0.0), sig

    def _beam(self, o, d, hit, t):
        """Beam x point estimate along the rays (o, d), cut at t where `hit`."""
        q, m = len(o), len(self.pv)
        val, bound, sig = np.zeros((q, 3)), np.zeros((q, 3)), np.zeros(q, dtype=np.uint64)
        if m == 0 or self.medium is None:
            return val, bound, sig
        step = min(max(1, (1 << 21) // m), 4 * len(OFFS))       # (a few neighbouring pixels' clouds: a narrow cone)
        for i0 in range(0, q, step):
            sl = slice(i0, i0 + step)
            oo, dd = o[sl], d[sl]
            # Rays from one origin lie in a cone; a sphere that does not reach into it (with 1e-4 (1 + |c|) to spare, a hundred times what a
            # cloud ray moves) contributes to none of them: it is left out of this batch, which changes no value, bound or signature.
            keep = np.ones(m, dtype=bool)
            if np.all(oo == oo[0]):
                axis = dd.mean(axis=0)
                axis /= np.sqrt((axis ** 2).sum())
                theta = np.arccos(np.clip((dd @ axis).min(), -1.0, 1.0))
                c = self.pv[:, :3] - oo[0]
                cl = np.sqrt((c ** 2).sum(axis=1))
                far = cl > 0.0
                reach = self.radius + 1e-4 * (1.0 + cl)
                ang = np.arccos(np.clip((c @ axis) / np.where(far, cl, 1.0), -1.0, 1.0))
                keep = ~far | (cl <= reach) | (ang <= theta + np.arcsin(np.minimum(1.0, reach / np.where(far, cl, 1.0))) + 1e-6)
            P, POW, r, w_v = self.pv[keep, :3], self.pv[keep, 6:9], self.radius[keep], self.w_v[keep]
            r2 = r * r
            pos = r2 > 0.0
            ir2 = np.where(pos, 1.0 / np.where(pos, r2, 1.0), 0.0)
            cx, cy, cz = (P[None, :, k] - oo[:, k, None] for k in range(3))        # c = p - o, (b, m) each
            c2 = cx * cx + cy * cy + cz * cz
            disk = cx * dd[:, 0, None] + cy * dd[:, 1, None] + cz * dd[:, 2, None]
            dist2 = ((oo[:, 0, None] + disk * dd[:, 0, None] - P[None, :, 0]) ** 2 + (oo[:, 1, None] + disk * dd[:, 1, None] - P[None, :, 1]) ** 2
                     + (oo[:, 2, None] + disk * dd[:, 2, None] - P[None, :, 2]) ** 2)
            ok = (disk > 0.0) & (dist2 < r2[None, :]) & ~(hit[sl, None] & (np.sqrt(c2) > t[sl, None]))
            tmp = 1.0 - dist2 * ir2[None, :]
            A = (3.0 / np.pi) * self.phase * ir2[None, :] * np.exp(-self.sigma_t * disk)
            w = np.where(ok, A * tmp * tmp, 0.0)
            val[sl] = (w[..., None] * POW[None]).sum(axis=1) * self.mcol
            clen = np.sqrt(c2)
            dt = 6.0 * U + (2.0 * np.sqrt(dist2) * clen * 10.0 * U + (10.0 * U * clen) ** 2) * ir2[None, :]
            wb = np.where(ok, A * (2.0 * tmp * dt + dt * dt + tmp * tmp * (12.0 * U + E_EXP)), 0.0)
            bound[sl] = (wb[..., None] * POW[None]).sum(axis=1) * self.mcol + np.abs(val[sl]) * ((ok.sum(axis=1) + 8) * U)[:, None]
            sig[sl] = (ok * w_v[None, :]).sum(axis=1, dtype=np.uint64)
        return val, bound, sig

    def _point_point(self, o, d, shift, dist, t, obj, nrm):
        """Point x point estimate (kind 0 in a medium), src/photon.rs:384-438: the volume gather at o + dist d when dist < t or
        nothing is hit, else the surface estimate times T(t) / T(dist)."""
        q, m = len(o), len(self.pv)
        hit = obj >= 0
        dist = np.asarray(dist, dtype=np.float64).reshape(q)
        moved = np.zeros(q, dtype=bool) if shift is None else (shift != 0).any(axis=1)
        tt = np.where(hit, t, np.inf)
        xs = o + np.where(hit, t, 0.0)[:, None] * d
        if shift is not None:
            xs = xs + (AMP * (1.0 + np.abs(xs).max(axis=1)))[:, None] * shift
            tt = np.where(hit & moved, np.sqrt(((xs - o) ** 2).sum(axis=1)), tt)
        vol = ~hit | (dist < tt)
        val, bound, sig = np.zeros((q, 3)), np.zeros((q, 3)), np.zeros(q, dtype=np.uint64)
        Td = np.exp(-self.sigma_t * dist)
        rows = np.flatnonzero(vol)
        if len(rows):
            x = o[rows] + dist[rows, None] * d[rows]
            if shift is not None:
                x = x + (AMP * (1.0 + np.abs(x).max(axis=1)))[:, None] * shift[rows]
            k = min(self.Kv, m)
            if k == 0:
                sum_p, r2, s = np.zeros((len(rows), 3)), np.zeros(len(rows)), np.zeros(len(rows), dtype=np.uint64)
                tie = np.zeros((len(rows), 3))
            else:
                more = min(m, k + TIE_POOL)
                sel, d2 = _nearest(self.pv[:, :3], x, more)
                POW = self.pv[:, 6:9][sel]                                  # (q, more, 3) in the order (distance, index)
                sum_p, r2, s = POW[:, :k].sum(axis=1), d2[:, k - 1], self.w_v[sel[:, :k]].sum(axis=1, dtype=np.uint64)
                # photons whose squared distance is within 8 u of the K-th's cannot be told apart from it in fp32 (4 u each): the
                # device's sum may hold any n_in of that band; per channel the largest and the smallest such sum
                inside = np.arange(more)[None, :] < k
                band = np.abs(d2 - r2[:, None]) <= 8.0 * U * r2[:, None]
                n_in = (band & inside).sum(axis=1)
                cur = np.where((band & inside)[..., None], POW, 0.0).sum(axis=1)
                hi_p = -np.sort(np.where(band[..., None], -POW, 0.0), axis=1)        # descending, zeros last
                lo_p = np.sort(np.where(band[..., None], POW, np.inf), axis=1)        # ascending, inf last
                take = (np.arange(more)[None, :] < n_in[:, None])[..., None]
                tie = np.maximum(np.where(take, hi_p, 0.0).sum(axis=1) - cur, cur - np.where(take, lo_p, 0.0).sum(axis=1))
                tie = np.where((band & ~inside).any(axis=1)[:, None], tie, 0.0)
            with np.errstate(divide="ignore", invalid="ignore"):
                scale = self.mcol * self.phase / ((4.0 / 3.0) * np.pi * r2 ** 1.5)[:, None] / self.sigma_t
                scale = scale * Td[rows, None] / (self.sigma_t * Td[rows])[:, None]
                v = sum_p * scale
                b = np.abs(v) * ((k + 24) * U) + scale * tie + np.where(tie.any(axis=1), 12.0 * U, 0.0)[:, None] * np.abs(v)
            val[rows], bound[rows] = v, np.where(np.isfinite(b), b, 0.0)
            sig[rows] = np.uint64(0xD1B54A32D192ED03) + s * np.uint64(7)
        rows = np.flatnonzero(~vol)
        if len(rows):
            wo = -d[rows] / np.sqrt((d[rows] ** 2).sum(axis=1))[:, None]
            v, b, s = self._surface(xs[rows], nrm[rows], wo, obj[rows], tt[rows])
            with np.errstate(divide="ignore", invalid="ignore"):
                v = v / Td[rows, None]
                b = b / Td[rows, None] + np.abs(v) * (E_EXP * np.maximum(1.0, self.sigma_t * dist[rows]) + 3.0 * U)[:, None]
            val[rows], bound[rows] = v, np.where(np.isfinite(b), b, 0.0)
            sig[rows] = (obj[rows].astype(np.int64) + 2).astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15) + s
        return val, bound, sig

    def _beam_beam(self, o, d, hit, t):
        """Beam x beam estimate along the rays (o, d), cut at t where `hit`: src/photon.rs:503-593 over the beams whose own box the ray
        hits (impl Bounded for PhotonBeam, :74-104), the radius from the record."""
        q, m = len(o), len(self.pv)
        val, bound, sig = np.zeros((q, 3)), np.zeros((q, 3)), np.zeros(q, dtype=np.uint64)
        if m == 0 or self.medium is None:
            return val, bound, sig
        E, S, POW, R = self.pv[:, 0:3], self.pv[:, 3:6], self.pv[:, 6:9], self.pv[:, 9]
        omax = np.abs(o).max(axis=1)
        smax = np.abs(S).max(axis=1)
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            bvec = E - S
            blen = np.sqrt((bvec ** 2).sum(axis=1))
            bdir = bvec / blen[:, None]
            c = (S - E) ** 2
            tot = c[:, 0] + c[:, 1] + c[:, 2]
            adj = np.sqrt(np.stack([c[:, 1] + c[:, 2], c[:, 0] + c[:, 2], c[:, 0] + c[:, 1]], axis=1) / tot[:, None]) * R[:, None]
            lo, hi = np.minimum(S, E) - adj, np.maximum(S, E) + adj

            def unit(v):
                return v / np.sqrt((v ** 2).sum(axis=2))[..., None]

            step = max(1, (1 << 18) // m)
            for i0 in range(0, q, step):
                sl = slice(i0, i0 + step)
                oo, dd = o[sl, None, :], d[sl, None, :]
                a1, a2 = (lo[None] - oo) / dd, (hi[None] - oo) / dd
                tn = np.fmax(np.fmax(np.fmin(a1, a2)[..., 0], np.fmin(a1, a2)[..., 1]), np.fmin(a1, a2)[..., 2])
                tf = np.fmin(np.fmin(np.fmax(a1, a2)[..., 0], np.fmax(a1, a2)[..., 1]), np.fmax(a1, a2)[..., 2])
                box = tf >= np.fmax(tn, 0.0)
                l = S[None] - oo
                bd = np.broadcast_to(bdir[None], l.shape)
                u = unit(np.cross(l, bd))
                n = unit(np.cross(bd, u))
                nl, nd = (n * l).sum(axis=2), (n * dd).sum(axis=2)
                tq = nl / nd
                qc = oo + tq[..., None] * dd
                dot_db = (dd * bd).sum(axis=2)
                inv_sin = 1.0 / np.sqrt(np.maximum(0.0, 1.0 - dot_db * dot_db))
                rel = qc - S[None]
                beam_t = (bd * rel).sum(axis=2)
                dq = qc - (S[None] + beam_t[..., None] * bd)
                dist = np.sqrt((dq ** 2).sum(axis=2))
                ok = box & ~(hit[sl, None] & (tq >= t[sl, None])) & ~((beam_t < 0.0) | (beam_t > blen[None])) & ~(dist >= R[None])
                tmp = 1.0 - dist / R[None]
                A = (self.sigma_t * self.phase * inv_sin * np.exp(-self.sigma_t * tq) * np.exp(-self.sigma_t * beam_t) * (3.0 / np.pi)
                     / (2.0 * R[None]))
                w = np.where(ok, A * tmp * tmp, 0.0)
                val[sl] = (w[..., None] * POW[None]).sum(axis=1) * self.mcol
                L, h, g = np.sqrt((l ** 2).sum(axis=2)), np.abs(nl), np.sqrt((rel ** 2).sum(axis=2))
                eps_n = 8.0 * U * (1.0 + L / h)
                dtq = (L * (eps_n + 3.0 * U) + np.abs(tq) * (eps_n + 3.0 * U)) / np.abs(nd) + 2.0 * U * np.abs(tq)
                dqc = dtq + 2.0 * U * (omax[sl, None] + np.abs(tq))
                dbt = dqc + 8.0 * U * g
                ddist = dqc + dbt + 4.0 * U * np.abs(beam_t) + U * smax[None] + 2.0 * U * dist
                dtmp = ddist / R[None] + 3.0 * U
                rr = (self.sigma_t * (dtq + dbt) + E_EXP * (np.maximum(1.0, self.sigma_t * np.abs(tq)) + np.maximum(1.0, self.sigma_t * np.abs(beam_t)))
                      + 8.0 * U / (1.0 - dot_db * dot_db) + 16.0 * U)
                wb = np.where(ok, np.abs(A) * (2.0 * np.abs(tmp) * dtmp + dtmp * dtmp + tmp * tmp * rr), 0.0)
                b = (wb[..., None] * POW[None]).sum(axis=1) * self.mcol + np.abs(val[sl]) * ((ok.sum(axis=1) + 8) * U)[:, None]
                bound[sl] = np.where(np.isfinite(b), b, 0.0)
                sig[sl] = (ok * self.w_v[None, :]).sum(axis=1, dtype=np.uint64)
        return val, bound, sig

    def evaluate(self, o, d, shift=None, dist=None):
        """photon_estimate_indirect for the rays (o, d), each on its own; shift: (q, 3) displacement of the hit point in units of
        AMP (1 + max|x|) (the cloud); dist (q,): the sampled medium distances of a kind-0 map, the cloud's move included
        -> value (q, 3), fp32 bound (q, 3), decision signature (q,)."""
        o = np.ascontiguousarray(o, dtype=np.float64).reshape(-1, 3)
        d = np.ascontiguousarray(d, dtype=np.float64).reshape(-1, 3)
        q = len(o)
        t, obj, nrm = self.osc.intersect(o, d, robust=1)
        hit = obj >= 0
        if self.kind == 0 and self.medium is not None:
            return self._point_point(o, d, shift, dist, t, obj, nrm)
        val, bound = np.zeros((q, 3)), np.zeros((q, 3))
        sig = (obj.astype(np.int64) + 2).astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15)
        rows = np.flatnonzero(hit)
        tt = np.where(hit, t, np.inf)
        if len(rows):
            x = o[rows] + t[rows, None] * d[rows]
            if shift is not None:
                x = x + (AMP * (1.0 + np.abs(x).max(axis=1)))[:, None] * shift[rows]
                moved = np.sqrt(((x - o[rows]) ** 2).sum(axis=1))
                tt[rows] = np.where((shift[rows] != 0).any(axis=1), moved, t[rows])
            wo = -d[rows] / np.sqrt((d[rows] ** 2).sum(axis=1))[:, None]
            v, b, s = self._surface(x, nrm[rows], wo, obj[rows], tt[rows])
            val[rows], bound[rows] = v, b
            sig[rows] += s
        if self.medium is None:
            miss = np.flatnonzero(~hit)
            if len(miss):
                val[miss] = self.osc.env_color(d[miss])
        else:
            v, b, s = self._beam(o, d, hit, tt) if self.kind == 1 else self._beam_beam(o, d, hit, tt)
            val, bound = val + v, bound + b
            sig += s * np.uint64(7)
        return val, bound, sig

    # ------------------------------------------------------------------ frames
    def rays(self, width, height, sample, seed=0):
        from oracle.pyoracle import camera_rays
        r = camera_rays(self.camera, width, height, sample=sample, seed=seed)
        return r["o"], r["d"]

    def distances(self, width, height, sample, seed=0):
        """Medium::sample_d of every pixel's sample `sample` -> the distance (n,), its cloud amplitude A_d (n,): the uniform is the
        stream's next draw after the camera's, (2k + 1) 2^-24 with k the word's top 23 bits."""
        from oracle.pyoracle import camera_rays
        mlog = -np.log(word_uniform(camera_rays(self.camera, width, height, sample=sample, seed=seed)["next_word"]))
        return mlog / self.sigma_t, FOG_K * U * np.maximum(1.0, mlog) / self.sigma_t

    def _cloud(self, o, d, offs, dist=None, amp_d=None):
        n, C = len(o), len(offs)
        oo = np.repeat(o, C, axis=0)
        dd = np.repeat(d, C, axis=0) + AMP * np.tile(offs, (n, 1))
        nz = np.tile((offs != 0).any(axis=1), n)
        dd[~nz] = np.repeat(d, C, axis=0)[~nz]                       # (the ray itself, bit for bit)
        dd[nz] /= np.sqrt((dd[nz] ** 2).sum(axis=1))[:, None]
        if dist is None:
            val, bound, sig = self.evaluate(oo, dd, np.tile(offs, (n, 1)))
        else:
            ds = np.repeat(dist, C) + np.repeat(amp_d, C) * np.tile(np.clip(offs.sum(axis=1), -1.0, 1.0), n)
            val, bound, sig = self.evaluate(oo, dd, np.tile(offs, (n, 1)), ds)
        return val.reshape(n, C, 3), bound.reshape(n, C, 3), sig.reshape(n, C)

    def sample(self, width, height, sample, seed=0):
        """Sample `sample` of every pixel -> Answers."""
        o, d = self.rays(width, height, sample, seed)
        dist, amp_d = self.distances(width, height, sample, seed) if self.kind == 0 and self.medium is not None else (None, None)
        val, bound, sig = self._cloud(o, d, OFFS, dist, amp_d)
        again = np.flatnonzero((sig != sig[:, :1]).any(axis=1))
        if len(again) == 0:
            return Answers(val, bound, sig)
        v2, b2, s2 = self._cloud(o[again], d[again], OFFS_MORE, None if dist is None else dist[again], None if dist is None else amp_d[again])
        return Answers(val, bound, sig, again, np.concatenate([val[again], v2], axis=1), np.concatenate([bound[again], b2], axis=1),
                       np.concatenate([sig[again], s2], axis=1))

    def mean(self, width, height, samples, seed=0, first=0):
        """The mean of `samples` samples per pixel -> value (n, 3), lo, hi (n, 3): the means of every sample's widened cloud range, and
        a further samples * u * |value| for the fp32 sum of the samples."""
        n = width * height
        v, lo, hi = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros((n, 3))
        for s in range(first, first + samples):
            a = self.sample(width, height, s, seed)
            v += a.value
            lo += (a.vals - a.bounds).min(axis=1)
            hi += (a.vals + a.bounds).max(axis=1)
        v, lo, hi = v / samples, lo / samples, hi / samples
        slack = samples * U * np.abs(v)
        return v, lo - slack, hi + slack


# ------------------------------------------------------------------ the rule
def _same_kind(got, ref):
    """Non-finite reference values: the same kind of value, channel by channel."""
    return bool(np.all(np.where(np.isnan(ref), np.isnan(got), np.where(np.isinf(ref), got == ref, np.isfinite(got)))))


def check(ans, got):
    """The rule, pixel by pixel -> failed (n,) bool, ratio (n,): the distance of `got` from the range of the cloud's (unwidened)
    values over the fp32 bound, the smallest over the signatures of the pixel (<= 1 passes; 0 / 0 = 0)."""
    got = np.asarray(got, dtype=np.float64).reshape(-1, 3)
    n = len(got)
    assert ans.vals.shape[0] == n
    failed, ratio = np.zeros(n, dtype=bool), np.zeros(n)
    for i in range(n):
        (vals, bnds, sig), g = ans.cloud(i), got[i]
        if not np.all(np.isfinite(vals)):
            ok = any(_same_kind(g, v) for v in vals)
            failed[i], ratio[i] = not ok, 0.0 if ok else np.inf
            continue
        if not np.all(np.isfinite(g)):
            failed[i], ratio[i] = True, np.inf
            continue
        best = np.inf
        for s in (sig[:1] if ans.decided[i] else np.unique(sig)):
            rows = sig == s
            lo, hi, b = vals[rows].min(axis=0), vals[rows].max(axis=0), bnds[rows].max(axis=0)
            excess = np.maximum(np.maximum(lo - g, g - hi), 0.0)
            with np.errstate(divide="ignore", invalid="ignore"):
                r = np.where(excess == 0.0, 0.0, excess / b)
            best = min(best, float(r.max()))
        ratio[i], failed[i] = best, not best <= 1.0
    return failed, ratio


def report(name, ans, got, show=6):
    """check + one printed line (and the first failing pixels) -> number of failures, largest error / bound."""
    failed, ratio = check(ans, got)
    fin = ratio[np.isfinite(ratio)]
    worst = float(fin.max()) if len(fin) else 0.0
    print(f"{name}: {len(ratio)} pixels, {int((~ans.decided).sum())} undecided, {int(failed.sum())} fail, largest error / bound "
          f"{worst:.3g}" + (" (and non-finite ones)" if len(fin) < len(ratio) else ""))
    for i in np.flatnonzero(failed)[:show]:
        print(f"  pixel {i} {'decided' if ans.decided[i] else 'undecided'}: library {np.asarray(got).reshape(-1, 3)[i].tolist()!r}")
        vals, bnds, sig = ans.cloud(i)
        print(f"    cloud of {len(sig)} with {len(np.unique(sig))} signatures: min {vals.min(axis=0).tolist()!r} max {vals.max(axis=0).tolist()!r} bound {bnds.max(axis=0).tolist()!r}")
    return int(failed.sum()), worst
