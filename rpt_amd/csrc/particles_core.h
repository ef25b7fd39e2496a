// particles_core.h — the arithmetic of rpt_particles_* and rpt_monomial_closest_point (src/ode/, MonomialSurface::closest_point*,
// examples/marbles.rs:76-88 of the reference) as include/rpt_hip.h states it: an order of fp64 operations, each rounded on its own.
// One text for the kernel (particles.hip) and for the host functions (rpt_particles.cpp), which run it serially: the pieces below are
// what a lane does for one particle, one partner or one candidate.  No operation here may be contracted into an fma.
#pragma once
#include <cmath>
#include <cstdint>

#ifdef __HIP__
#define RPTP_HD __host__ __device__ __forceinline__
#else
#define RPTP_HD inline
#endif
#ifdef __clang__
#pragma clang fp contract(off)
#endif

namespace rptp {
constexpr int kCoarseN = 100, kPreciseN = 10000;        // closest_point: candidates -n..n
constexpr uint32_t kMaxParticles = 256;
constexpr uint32_t kMaxLaunchSteps = 256;               // RK4 steps per kernel launch (100 ms at n = 256)
constexpr uint64_t kMaxSteps = 1ull << 20;              // ... and per call
constexpr double kNoWin = 1e18;                         // a candidate at this distance or beyond (or NaN) never wins
constexpr int kNoIndex = 0x7fffffff;

RPTP_HD double root(double x) {
#ifdef __HIP_DEVICE_COMPILE__
    return __dsqrt_rn(x);
#else
    return std::sqrt(x);
#endif
}
RPTP_HD double dot3(const double* a, const double* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
RPTP_HD double length3(const double* v) { return root(dot3(v, v)); }

// ---- closest_point: the candidate i of -n..n, and what follows the scan
RPTP_HD double cand_xf(int i, int n) { return double(i) / double(n); }
RPTP_HD double cand_yc(double height, double xf) { return height * ((xf * xf) * (xf * xf)); }
RPTP_HD double cand_d(double px, double py, double xf, double yc) {
    const double a = px - xf, b = py - yc;
    return a * a + b * b;
}
RPTP_HD double closest_px(const double* P) { return root(P[0] * P[0] + P[2] * P[2]); }
// xf: the winner's (-1.0 if nothing won)
RPTP_HD void closest_finish(double height, const double* P, double px, double xf, double* out) {
    const double ux = P[0] / px, uz = P[2] / px;
    const double X = xf * ux, Z = xf * uz;
    const double s = X * X + Z * Z;
    out[0] = X;
    out[1] = height * (s * s);
    out[2] = Z;
}
RPTP_HD void closest_point(double height, const double* P, int n, double* out) {
    if (length3(P) < 1e-12) {
        out[0] = P[0]; out[1] = P[1]; out[2] = P[2];
        return;
    }
    const double px = closest_px(P), py = P[1];
    double best = kNoWin, win = -1.0;
    for (int i = -n; i <= n; i++) {
        const double xf = cand_xf(i, n);
        const double d = cand_d(px, py, xf, cand_yc(height, xf));
        if (d < best) {
            best = d;
            win = xf;
        }
    }
    closest_finish(height, P, px, win, out);
}

// ---- MarblesSystem: one pair of particles, hi the one with the larger index (d = pos_hi - pos_lo is what BOTH of them see: for
// particle hi the partner is below it, for particle lo above).  True if the two touch; f: the pair's force.
RPTP_HD bool marbles_pair_force(const double* hi, const double* lo, double r, double* f) {
    double d[3];
    for (int k = 0; k < 3; k++) d[k] = hi[k] - lo[k];
    const double len = length3(d), two_r = 2.0 * r;
    if (!(len < two_r)) return false;
    const double c = (two_r - len) / r;
    for (int k = 0; k < 3; k++) {
        const double dir = d[k] / len;
        f[k] = ((-dir) * 5.0) * c;
    }
    return true;
}
// ... and what a touching partner q does to particle p's accumulator (below: q < p)
RPTP_HD void marbles_pair_apply(const double* f, const double* vp, bool below, double* acc) {
    for (int k = 0; k < 3; k++) {
        acc[k] = below ? acc[k] - f[k] : acc[k] + f[k];
        acc[k] = acc[k] - vp[k] * 0.5;
    }
}
RPTP_HD bool marbles_pair(const double* pp, const double* pq, const double* vp, double r, bool below, double* acc) {
    double f[3];
    if (!marbles_pair_force(below ? pp : pq, below ? pq : pp, r, f)) return false;
    marbles_pair_apply(f, vp, below, acc);
    return true;
}
// ... and what follows the pair terms: surface (C: closest_point of P), table, air.  cnt: surface band, surface push, table band, table push
RPTP_HD void marbles_rest(double r, const double* P, const double* V, const double* C, double* acc, uint32_t* cnt) {
    double v[3], nrm[3];
    for (int k = 0; k < 3; k++) v[k] = P[k] - C[k];
    const double L = length3(v);
    for (int k = 0; k < 3; k++) nrm[k] = v[k] / L;
    const double ratio = (r - L) / r;
    const double nv = dot3(V, nrm);
    if (-0.1 < ratio && ratio < 0.0) {
        const double nv3 = (nv * nv) * nv;
        for (int k = 0; k < 3; k++) acc[k] = acc[k] - (30.0 * nrm[k]) * nv3;
        cnt[0]++;
    } else if (ratio >= 0.0) {
        for (int k = 0; k < 3; k++) acc[k] = acc[k] + (100.0 * nrm[k]) * ratio;
        cnt[1]++;
    }
    const double tn[3] = {0.0, 1.0, 0.0};
    const double tr = ((r - 0.06) - P[1]) / r;
    const double tv = (V[0] * 0.0 + V[1] * 1.0) + V[2] * 0.0;
    if (length3(P) > 0.1) {
        if (-0.1 < tr && tr < 0.0) {
            for (int k = 0; k < 3; k++) acc[k] = acc[k] - (20.0 * tn[k]) * tv;
            cnt[2]++;
        } else if (tr >= 0.0) {
            for (int k = 0; k < 3; k++) acc[k] = acc[k] + (300000.0 * tn[k]) * tr;
            cnt[3]++;
        }
    }
    for (int k = 0; k < 3; k++) acc[k] = acc[k] - V[k] / 5.0;
}

// ---- SolidGravitySystem: one pair, and one partner
RPTP_HD void gravity_pair_force(const double* hi, const double* lo, double* f) {
    double d[3];
    for (int k = 0; k < 3; k++) d[k] = hi[k] - lo[k];
    const double len = length3(d);
    const double s = 1.0 / (len * len) - 0.0001 * (1.0 / (len * ((len * len) * (len * len))));
    for (int k = 0; k < 3; k++) f[k] = (d[k] / len) * s;
}
RPTP_HD void gravity_pair_apply(const double* f, bool below, double* acc) {
    for (int k = 0; k < 3; k++) acc[k] = below ? acc[k] - f[k] : acc[k] + f[k];
}
RPTP_HD void gravity_pair(const double* pp, const double* pq, bool below, double* acc) {
    double f[3];
    gravity_pair_force(below ? pp : pq, below ? pq : pp, f);
    gravity_pair_apply(f, below, acc);
}
// ---- SimpleCircleSystem
RPTP_HD void circle_derivative(const double* P, double* dpos, double* dvel) {
    dpos[0] = -P[1]; dpos[1] = P[0]; dpos[2] = 0.0;
    dvel[0] = dvel[1] = dvel[2] = 0.0;
}

// ---- RK4 over the six values of a particle: the stage state, the running sum ((k1 + k2 2) + k3 2) + k4, the new state
RPTP_HD double rk4_stage(double s, double k, double f) { return s + k * f; }
RPTP_HD double rk4_sum(double sum, double k, int stage /* 1..4 */) { return stage == 1 ? k : (stage == 4 ? sum + k : sum + k * 2.0); }
RPTP_HD double rk4_new(double s, double sum, double h) { return s + sum * (h / 6.0); }

// ---- the display position of marbles.rs:77-83; C: closest_point_precise of P
RPTP_HD void display_position(double r, const double* P, const double* C, double* out) {
    double v[3];
    for (int k = 0; k < 3; k++) {
        v[k] = P[k] - C[k];
        out[k] = P[k];
    }
    const double len = length3(v);
    if (len < r * 1.05)
        for (int k = 0; k < 3; k++) out[k] = C[k] + ((v[k] / len) * r) * 1.05;
    const double lo = r - 0.06;
    out[1] = (out[1] != out[1]) ? lo : ((lo != lo) ? out[1] : (out[1] >= lo ? out[1] : lo));   // f64::max
}

// ---- the host's serial run of the same text
// The time loop of rk4_integrate: n_full steps of `step` and one of *last; false if that is more than kMaxSteps steps.
inline bool step_sequence(double time, double step, uint64_t* n_full, double* last) {
    double t = time;
    uint64_t c = 0;
    while (t > step) {
        if (c + 1 >= kMaxSteps) return false;
        t = t - step;
        c++;
    }
    *n_full = c;
    *last = t;
    return true;
}
// The derivative of (pos, vel), n x 3 each, to (dpos, dvel).  cnt[6]: evaluations, pair contacts, surface band / push, table band / push.
inline void derivative(int kind, uint32_t n, double r, double height, const double* pos, const double* vel, double* dpos, double* dvel, uint64_t* cnt) {
    cnt[0]++;
    for (uint32_t p = 0; p < n; p++) {
        const double *P = pos + 3 * p, *V = vel + 3 * p;
        if (kind == 0) {
            circle_derivative(P, dpos + 3 * p, dvel + 3 * p);
            continue;
        }
        double acc[3] = {0.0, kind == 2 ? -1.0 : 0.0, 0.0};
        for (uint32_t q = 0; q < n; q++) {
            if (q == p) continue;
            if (kind == 1)
                gravity_pair(P, pos + 3 * q, q < p, acc);
            else if (marbles_pair(P, pos + 3 * q, V, r, q < p, acc) && q < p)
                cnt[1]++;
        }
        if (kind == 2) {
            double C[3];
            uint32_t c4[4] = {0, 0, 0, 0};
            closest_point(height, P, kCoarseN, C);
            marbles_rest(r, P, V, C, acc, c4);
            for (int k = 0; k < 4; k++) cnt[2 + k] += c4[k];
        }
        for (int k = 0; k < 3; k++) {
            dpos[3 * p + k] = V[k];
            dvel[3 * p + k] = acc[k];
        }
    }
}
}  // namespace rptp
