// scene_update_core.h — the records of a sphere whose transform is translate(c) * scale(r, r, r), as one defined order of operations:
// what the flattener of rpt_capi.cpp (make_xf / finish_xf / invert4, emit, xf_box, collect_scan_boxes' push_box, the fp64 flatten with
// cull_box64) and rpt_temporal_motion_record compute for the matrix
//
//      r 0 0 cx
//      0 r 0 cy        (every zero a +0.0, the bottom row 0 0 0 1)
//      0 0 r cz
//
// restated for that form, operation by operation, so that the kernel of scene_update.hip writes the bytes a fresh commit would upload.
// One text for the kernel and for the host (rpt_sphere_records_host, the CPU harness).  No operation here may be contracted into an fma,
// and nothing is simplified by the mathematics: N is r^2 / r^3, not 1 / r; a product with a zero of the matrix is kept wherever its
// sign or a NaN could reach the result (the compiler folds the ones that cannot).
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>

#ifdef __HIP__
#define RPTU_HD __host__ __device__ __forceinline__
#else
#define RPTU_HD inline
#endif
#ifdef __clang__
#pragma clang fp contract(off)
#endif

namespace rptu {

RPTU_HD double root(double x) {
#ifdef __HIP_DEVICE_COMPILE__
    return __dsqrt_rn(x);
#else
    return std::sqrt(x);
#endif
}
RPTU_HD uint32_t f32_bits(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    return u;
}
RPTU_HD float bits_f32(uint32_t u) {
    float f;
    memcpy(&f, &u, 4);
    return f;
}
// std::nextafter(x, -inf) and std::nextafter(x, +inf) of an fp32 value with integer operations: the same on the host and on the
// device for every input (a NaN stays the NaN it is; an infinity in the direction of travel stays; +-0 steps to the smallest subnormal).
RPTU_HD float next_down(float x) {
    const uint32_t u = f32_bits(x), mag = u & 0x7fffffffu;
    if (mag > 0x7f800000u) return x;               // NaN
    if (u == 0xff800000u) return x;                // -inf
    if (mag == 0u) return bits_f32(0x80000001u);   // +-0 -> -min subnormal
    return bits_f32((u & 0x80000000u) ? u + 1u : u - 1u);
}
RPTU_HD float next_up(float x) {
    const uint32_t u = f32_bits(x), mag = u & 0x7fffffffu;
    if (mag > 0x7f800000u) return x;
    if (u == 0x7f800000u) return x;                // +inf
    if (mag == 0u) return bits_f32(0x00000001u);
    return bits_f32((u & 0x80000000u) ? u - 1u : u + 1u);
}
RPTU_HD bool finite32(float x) { return (f32_bits(x) & 0x7f800000u) != 0x7f800000u; }
RPTU_HD bool finite64(double x) {
    uint64_t u;
    memcpy(&u, &x, 8);
    return (u & 0x7ff0000000000000ull) != 0x7ff0000000000000ull;
}
// std::min(a, b) / std::max(a, b) as the flattener's calls evaluate them (the first argument wins a tie and against a NaN second)
RPTU_HD double min_std(double a, double b) { return b < a ? b : a; }
RPTU_HD double max_std(double a, double b) { return a < b ? b : a; }
RPTU_HD float min_std(float a, float b) { return b < a ? b : a; }
RPTU_HD float max_std(float a, float b) { return a < b ? b : a; }

// ---- the derived matrices (make_xf -> finish_xf): rows of M^-1 (3 x 4), the diagonal of N = (linear)^-T and det(linear)
struct SphereXf {
    double inv[12];   // rows of M^-1
    double n;         // N[0][0] = N[1][1] = N[2][2] (the off-diagonals are +0.0: 0 / det with det > 0)
    double det;
};
RPTU_HD void sphere_xf(double r, const double* c, SphereXf* x) {
    // invert4 on [M | I]: the pivot of column k < 3 is row k (every other entry of the column is zero), the row is divided by r, and no
    // other row holds a non-zero in that column, so nothing is subtracted.  Column 3: the pivot is row 3 (1.0; the division by it
    // changes nothing), and row k < 3 loses f = c[k] / r times row 3 = (0 0 0 1 | 0 0 0 1), if f != 0.
    const double z = 0.0 / r;      // what every zero of a row becomes when the row is divided by its pivot
    const double d = 1.0 / r;      // the identity half's 1.0
    for (int k = 0; k < 3; k++) {
        const double f = c[k] / r;
        for (int j = 0; j < 4; j++) {
            double m = j == k ? d : z;
            if (f != 0.0) m = m - f * (j == 3 ? 1.0 : 0.0);
            x->inv[4 * k + j] = m;
        }
    }
    // finish_xf: the determinant and the inverse transpose of the linear part a = diag(r, r, r), by the cofactor formulas as written
    const double a[3][3] = {{r, 0.0, 0.0}, {0.0, r, 0.0}, {0.0, 0.0, r}};
    x->det = a[0][0] * (a[1][1] * a[2][2] - a[1][2] * a[2][1]) - a[0][1] * (a[1][0] * a[2][2] - a[1][2] * a[2][0]) +
             a[0][2] * (a[1][0] * a[2][1] - a[1][1] * a[2][0]);
    x->n = (a[1][1] * a[2][2] - a[1][2] * a[2][1]) / x->det;   // inv[0][0]; inv[1][1] and inv[2][2] are the same product of r with r
}

// ---- fp32 path: XfScan (12 floats: rows of M^-1) and the three normal-transform floats of XfShade (emit)
RPTU_HD void sphere_scan_rows(const SphereXf& x, float* rows /* 12 */) {
    for (int k = 0; k < 12; k++) rows[k] = float(x.inv[k]);
}
// xf_box(.., sphere): the world box of the unit sphere under M, as add_item and push_box receive it
RPTU_HD void sphere_item_box(double r, const double* c, float* lo, float* hi) {
    for (int i = 0; i < 3; i++) {
        double h = 0.0;
        for (int j = 0; j < 3; j++) {
            const double m = i == j ? r : 0.0;
            h += m * m;
        }
        h = root(h);
        h += 1e-5 * (h + std::fabs(c[i]));
        lo[i] = float(c[i] - h);
        hi[i] = float(c[i] + h);
    }
}
// push_box of collect_scan_boxes: the item box with the padding of SceneView::pbox, in fp32
RPTU_HD void pad_scan_box(const float* lo, const float* hi, float* plo, float* phi) {
    for (int a = 0; a < 3; a++) {
        const float pad = 1e-5f * (std::fabs(lo[a]) + std::fabs(hi[a]) + (hi[a] - lo[a])) + 1e-7f;
        plo[a] = lo[a] - pad;
        phi[a] = hi[a] + pad;
    }
}
// BvhBuilder::build: a node's box is the bounds of its items with this padding (the scene tree's refit applies it to the union again)
RPTU_HD void pad_node_box(const float* lo, const float* hi, float* plo, float* phi) {
    for (int a = 0; a < 3; a++) {
        const float pad = 1e-6f * max_std(std::fabs(lo[a]), std::fabs(hi[a])) + 1e-30f;
        plo[a] = lo[a] - pad;
        phi[a] = hi[a] + pad;
    }
}

// ---- reference-epsilon mode: cull_box64 of a transformed sphere.  False: a box fp32 cannot hold (the flattener's `unbounded`: lo, hi zero)
RPTU_HD bool sphere_cull_box(double r, const double* c, float* lo, float* hi) {
    const double fwd[3][4] = {{r, 0.0, 0.0, c[0]}, {0.0, r, 0.0, c[1]}, {0.0, 0.0, r, c[2]}};
    double wlo[3] = {HUGE_VAL, HUGE_VAL, HUGE_VAL}, whi[3] = {-HUGE_VAL, -HUGE_VAL, -HUGE_VAL};
    for (int corner = 0; corner < 8; corner++) {
        const double p[3] = {corner & 1 ? 1.0 : -1.0, corner & 2 ? 1.0 : -1.0, corner & 4 ? 1.0 : -1.0};
        for (int i = 0; i < 3; i++) {
            const double w = fwd[i][0] * p[0] + fwd[i][1] * p[1] + fwd[i][2] * p[2] + fwd[i][3];
            wlo[i] = min_std(wlo[i], w);
            whi[i] = max_std(whi[i], w);
        }
    }
    double size = 0.0, mag = 0.0;
    for (int i = 0; i < 3; i++) {
        size = max_std(size, whi[i] - wlo[i]);
        mag = max_std(mag, max_std(std::fabs(wlo[i]), std::fabs(whi[i])));
    }
    const double pad = 1e-5 * size + 1e-5 * mag + 1e-30;
    bool finite = true;
    for (int i = 0; i < 3; i++) {
        lo[i] = next_down(float(wlo[i] - pad));
        hi[i] = next_up(float(whi[i] + pad));
        finite = finite && finite32(lo[i]) && finite32(hi[i]);
    }
    if (!finite)
        for (int i = 0; i < 3; i++) lo[i] = hi[i] = 0.f;
    return finite;
}

// ---- rpt_temporal_motion_record(cur, prev) for cur = T(c) S(r), prev = T(p) S(r): the 24 doubles in the order include/rpt_hip.h states
// (the map A, u and the normal map).  Matrices that compare equal -- c[k] == p[k] for every k, so -0.0 and 0.0 are equal -- give the
// exact identity record.  False (and an all-zero record): rpt_temporal_motion_record would refuse the pair; for finite centres that
// depends on r alone, and rpt_scene_set_movable_spheres refuses such an r.
RPTU_HD double cofactors3(const double m[3][3], double k[3][3]) {
    k[0][0] = m[1][1] * m[2][2] - m[1][2] * m[2][1]; k[0][1] = m[0][2] * m[2][1] - m[0][1] * m[2][2]; k[0][2] = m[0][1] * m[1][2] - m[0][2] * m[1][1];
    k[1][0] = m[1][2] * m[2][0] - m[1][0] * m[2][2]; k[1][1] = m[0][0] * m[2][2] - m[0][2] * m[2][0]; k[1][2] = m[0][2] * m[1][0] - m[0][0] * m[1][2];
    k[2][0] = m[1][0] * m[2][1] - m[1][1] * m[2][0]; k[2][1] = m[0][1] * m[2][0] - m[0][0] * m[2][1]; k[2][2] = m[0][0] * m[1][1] - m[0][1] * m[1][0];
    return (m[0][0] * k[0][0] + m[0][1] * k[1][0]) + m[0][2] * k[2][0];
}
RPTU_HD bool sphere_motion_record(double r, const double* c, const double* p, double* out /* 24 */) {
    for (int i = 0; i < 24; i++) out[i] = 0.0;
    if (!finite64(r)) return false;
    for (int k = 0; k < 3; k++)
        if (!finite64(c[k]) || !finite64(p[k])) return false;
    const bool same = c[0] == p[0] && c[1] == p[1] && c[2] == p[2];
    const double cur[3][3] = {{r, 0.0, 0.0}, {0.0, r, 0.0}, {0.0, 0.0, r}};
    double k3[3][3], a[3][3];
    const double det = cofactors3(cur, k3);
    if (det == 0.0 || !finite64(det)) return false;
    if (same) {
        out[0] = out[5] = out[10] = out[12] = out[16] = out[20] = 1.0;
        return true;
    }
    double inv[3][3], u[3];
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) inv[i][j] = k3[i][j] / det;
        u[i] = -((inv[i][0] * c[0] + inv[i][1] * c[1]) + inv[i][2] * c[2]);
    }
    for (int i = 0; i < 3; i++) {
        const double prow[4] = {i == 0 ? r : 0.0, i == 1 ? r : 0.0, i == 2 ? r : 0.0, p[i]};
        for (int j = 0; j < 3; j++) a[i][j] = out[4 * i + j] = (prow[0] * inv[0][j] + prow[1] * inv[1][j]) + prow[2] * inv[2][j];
        out[4 * i + 3] = ((prow[0] * u[0] + prow[1] * u[1]) + prow[2] * u[2]) + prow[3];
    }
    const double det_a = cofactors3(a, k3);
    if (det_a == 0.0 || !finite64(det_a)) {
        for (int i = 0; i < 24; i++) out[i] = 0.0;
        return false;
    }
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) out[12 + 3 * i + j] = k3[j][i] / det_a;
    return true;
}

// ---- everything at once, as rpt_sphere_records_host hands it out
struct SphereRecords {
    float scan[12];        // XfScan: r0, r1, r2
    float shade_n;         // XfShade: r0.x = r1.y = r2.z (the other normal entries are +0.f; r0.w the object, r1.w = 1.f, r2.w = 0.f)
    float item_lo[3], item_hi[3];   // xf_box
    float pbox_lo[3], pbox_hi[3];   // SceneView::pbox (the .w of both rows is 0.f)
    double inv[12];        // ObjRec::inv
    double nrm;            // ObjShade::nrm[0] = [4] = [8] (the others +0.0)
    float cull_lo[3], cull_hi[3];
    uint32_t cull_unbounded;
};
RPTU_HD void sphere_records(double r, const double* c, SphereRecords* o) {
    SphereXf x;
    sphere_xf(r, c, &x);
    sphere_scan_rows(x, o->scan);
    o->shade_n = float(x.n);
    sphere_item_box(r, c, o->item_lo, o->item_hi);
    pad_scan_box(o->item_lo, o->item_hi, o->pbox_lo, o->pbox_hi);
    for (int k = 0; k < 12; k++) o->inv[k] = x.inv[k];
    o->nrm = x.n;
    o->cull_unbounded = sphere_cull_box(r, c, o->cull_lo, o->cull_hi) ? 0u : 1u;
}
}  // namespace rptu
