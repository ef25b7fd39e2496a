// device_core.h — gfx950 device functions of the path-tracing core (fp32).
// Reference line citations are relative to the rpt source tree (src/...).
#pragma once
#ifndef __HIPCC_RTC__   // (runtime compilation has both built in)
#include <hip/hip_runtime.h>
#include <type_traits>
#endif
#include "gpu_layout.h"

namespace rptg {

// The names of <type_traits> that the device code uses: the standard library's, or -- runtime compilation has no standard library --
// their few lines.
#ifndef __HIPCC_RTC__
namespace tt = std;
#else
namespace tt {
template <bool B> struct bool_constant { static constexpr bool value = B; };
typedef bool_constant<true> true_type;
typedef bool_constant<false> false_type;
template <class A, class B> inline constexpr bool is_same_v = false;
template <class A> inline constexpr bool is_same_v<A, A> = true;
template <bool C, class A, class B> struct conditional { typedef A type; };
template <class A, class B> struct conditional<false, A, B> { typedef B type; };
template <bool C, class A, class B> using conditional_t = typename conditional<C, A, B>::type;
}  // namespace tt
#endif

#define RPT_DEV __device__ __forceinline__

static constexpr float kPi = 3.14159265358979323846f;
static constexpr float kInvPi = 0.31830988618379067154f;
static constexpr float kInf = __builtin_huge_valf();

// ------------------------------------------------------------------ vec3
struct V {
    float x, y, z;
};
RPT_DEV V mk(float x, float y, float z) { return V{x, y, z}; }
RPT_DEV V operator+(V a, V b) { return V{a.x + b.x, a.y + b.y, a.z + b.z}; }
RPT_DEV V operator-(V a, V b) { return V{a.x - b.x, a.y - b.y, a.z - b.z}; }
RPT_DEV V operator-(V a) { return V{-a.x, -a.y, -a.z}; }
RPT_DEV V operator*(float s, V a) { return V{s * a.x, s * a.y, s * a.z}; }
RPT_DEV V operator*(V a, float s) { return V{s * a.x, s * a.y, s * a.z}; }
RPT_DEV V operator*(V a, V b) { return V{a.x * b.x, a.y * b.y, a.z * b.z}; }
RPT_DEV float dot(V a, V b) { return fmaf(a.x, b.x, fmaf(a.y, b.y, a.z * b.z)); }
RPT_DEV V cross(V a, V b) {
    return V{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}
RPT_DEV V fma3(float s, V a, V b) { return V{fmaf(s, a.x, b.x), fmaf(s, a.y, b.y), fmaf(s, a.z, b.z)}; }
RPT_DEV V fma3(V s, V a, V b) { return V{fmaf(s.x, a.x, b.x), fmaf(s.y, a.y, b.y), fmaf(s.z, a.z, b.z)}; }
RPT_DEV float rsq(float x) { return __builtin_amdgcn_rsqf(x); }
RPT_DEV float rcp(float x) { return __builtin_amdgcn_rcpf(x); }
// v_sqrt_f32 as it is (1 ulp, like rcp / rsq above).  sqrtf() is correctly rounded by default under hipcc: one v_sqrt_f32
// plus ~17 instructions of scaling and refinement around it, per call, in the sphere test and the direction samplers.
RPT_DEV float sqrt1(float x) { return __builtin_amdgcn_sqrtf(x); }
RPT_DEV V normalize(V a) { return rsq(dot(a, a)) * a; }
RPT_DEV V vmin(V a, V b) { return V{fminf(a.x, b.x), fminf(a.y, b.y), fminf(a.z, b.z)}; }
RPT_DEV float max3(float a, float b, float c) { return fmaxf(fmaxf(a, b), c); }
RPT_DEV float min3(float a, float b, float c) { return fminf(fminf(a, b), c); }
RPT_DEV V xyz(const F4& f) { return V{f.x, f.y, f.z}; }
RPT_DEV float dot3w(const F4& r, V p) { return fmaf(r.x, p.x, fmaf(r.y, p.y, fmaf(r.z, p.z, r.w))); }
RPT_DEV float dot3(const F4& r, V p) { return fmaf(r.x, p.x, fmaf(r.y, p.y, r.z * p.z)); }
RPT_DEV bool is_zero(V a) { return a.x == 0.f && a.y == 0.f && a.z == 0.f; }

// Wave-uniform read of a 16-byte-multiple scene record through the constant address space, so
// hipcc emits scalar loads (s_load_dwordx4/x8 into SGPRs).  A plain load through the generic
// pointer is emitted as a per-lane global_load (12 VGPRs per 48-byte record) because the kernel
// also stores to global memory and the compiler cannot prove the record is never clobbered.
// Only valid when `p` is the same in every lane.
template <class T>
RPT_DEV T uload(const T* p) {
    static_assert(sizeof(T) % 16 == 0, "scene records are 16-byte multiples");
    typedef uint32_t u4v __attribute__((ext_vector_type(4)));
    typedef const __attribute__((address_space(4))) u4v* CP;
    CP q = (CP)(uintptr_t)p;
    u4v raw[sizeof(T) / 16];
#pragma unroll
    for (unsigned i = 0; i < sizeof(T) / 16; i++) raw[i] = q[i];
    T out;
    __builtin_memcpy(&out, raw, sizeof(T));  // not a cast: the record's fields are floats, the loads are uint vectors
    return out;
}

// The scene view as it lies in the kernel-argument segment.  EVERY kernel of this library takes its arguments as one
// struct that begins with the SceneView (RenderArgs, QueryArgs, ShootArgs, intersect_kernel's first parameter: static
// asserts next to each), so kernarg + 0 is the view.  Reading a field through this pointer -- constant address space,
// behind an opaque copy of the pointer -- is a scalar load at the place of use; read as a plain kernel argument it is
// hoisted to the kernel's entry and held in a scalar register for the kernel's whole life.
// CONSEQUENCE: the `const SceneView&` parameter that scan_prims, closest_hit, finalize_hit, load_mat, env_color, ... still take
// is NOT what they read -- it only keeps the call sites readable.  A kernel whose first argument is not the view, or a caller
// that builds a modified copy of the view, would silently get the launch's own view: every kernel that calls these functions
// carries a static_assert (or, for intersect_kernel, a comment) that its argument struct begins with the SceneView.
typedef const __attribute__((address_space(4))) SceneView* KernargView;
RPT_DEV KernargView kernarg_scene() {
    KernargView kv = (KernargView)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(kv));
    return kv;
}
// A sub-struct of the kernel arguments by value (dword loads through the constant address space).
template <class T>
RPT_DEV T kernarg_load(const __attribute__((address_space(4))) T* p) {
    static_assert(sizeof(T) % 4 == 0, "kernel-argument structs are dword multiples");
    typedef const __attribute__((address_space(4))) uint32_t* Q;
    Q q = (Q)p;
    uint32_t raw[sizeof(T) / 4];
#pragma unroll
    for (unsigned i = 0; i < sizeof(T) / 4; i++) raw[i] = q[i];
    T out;
    __builtin_memcpy(&out, raw, sizeof(T));
    return out;
}
// The same for a kernel's whole argument struct T (it lies at kernarg + 0).
template <class T>
RPT_DEV const __attribute__((address_space(4))) T* kernarg_args() {
    typedef const __attribute__((address_space(4))) T* P;
    P p = (P)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p));
    return p;
}

// ------------------------------------------------------------------ RNG
// xoshiro128+ seeded through splitmix64 from (seed, pixel, sample); bit-identical to the
// oracle's Rng.  Replaces StdRng::from_entropy() per row (src/renderer.rs:163).
RPT_DEV uint64_t mix64(uint64_t x) {
    x ^= x >> 30;
    x *= 0xBF58476D1CE4E5B9ULL;
    x ^= x >> 27;
    x *= 0x94D049BB133111EBULL;
    x ^= x >> 31;
    return x;
}
// The leaner forms of the generator and its draws, one bit each so that a build can take them singly (-DRPT_RNG_FORMS=<mask>, default:
// all).  Each is an integer identity or an exact scaling by a power of two: draw values, their number and their order stay what
// they are, and the old form of every changed function stays next to it as *_ref (rpt_debug_draw_forms runs all the new forms, on
// or off in this build, and the old ones).
#define RPT_RNG_STEP 1u        // Rng::next: three xor3 (v_bitop3_b32) and one xor for six xors
#define RPT_RNG_ONE_MASK 2u    // triangle-light rejection: one operand masked, not both
#define RPT_RNG_RANGE 4u       // Rng::range: 2^-24 folded into the width
#define RPT_RNG_ROULETTE 8u    // uniform() < 0.8 compared on the raw word
#define RPT_RNG_ALL 15u
// Default: the step alone.  Measured on C3: the step pays 0.29 ms of 18.08; the one-mask test and the
// two draw forms lower the instruction count as predicted but each stayed inside three times the run-to-run range, so they are off.
#ifndef RPT_RNG_FORMS
#define RPT_RNG_FORMS RPT_RNG_STEP
#endif
RPT_DEV uint32_t xor3(uint32_t x, uint32_t y, uint32_t z) { return __builtin_amdgcn_bitop3_b32(x, y, z, 0x96); }
// uniform() < p on the draw's word: with u = (2k+1) 2^-24, k = word >> 9, u < p <=> 2k+1 < p 2^24 <=> k < ceil((p 2^24 - 1) / 2) =: K
// <=> word < K << 9 (the low nine bits do not matter, and K < 2^23).  p 2^24 and the halving are exact in fp64 for a float or a
// double p in (0, 1); the same K serves u read as a float and as a double, since u is the same number in both.
constexpr uint32_t roulette_k(double p) {
    const double h = (p * 0x1p24 - 1.0) / 2.0;
    const uint32_t k = uint32_t(h);
    return double(k) < h ? k + 1u : k;
}
constexpr uint32_t roulette_word(double p) { return roulette_k(p) << 9; }
constexpr bool roulette_exact(double p) {   // the last draw below p and the first one not below it, in the draw's own terms
    const uint32_t k = roulette_k(p);
    return k > 0u && k < (1u << 23) && double(2u * (k - 1u) + 1u) * 0x1p-24 < p && !(double(2u * k + 1u) * 0x1p-24 < p);
}
static constexpr uint32_t kRoulette08 = roulette_word(0.8f);
static_assert(float(0x00CCCCCDu) * 0x1p-24f == 0.8f, "0.8f = 13421773 * 2^-24");
static_assert(kRoulette08 == 0xCCCCCC00u && roulette_exact(0.8f), "uniform() < 0.8f <=> word < 0xCCCCCC00");
static_assert(roulette_word(0.8) == kRoulette08 && roulette_exact(0.8), "the fp64 path's 0.8 cuts the draws at the same word");
// FORMS: the forms this generator takes.  Every kernel runs Rng = RngT<RPT_RNG_FORMS> but the one flavour that names another mask
// because a form costs it a register (photon.hip, QueryRng), and the test hook, which runs them all.
template <uint32_t FORMS>
struct RngT {
    uint32_t s0, s1, s2, s3;
    // `a` = mix64(seed + GOLDEN), computed on the host.
    RPT_DEV void seed(uint64_t a, uint32_t pixel, uint32_t sample) {
        const uint64_t G = 0x9E3779B97F4A7C15ULL;
        uint64_t z = a ^ ((uint64_t(sample) << 32) | uint64_t(pixel));
        uint64_t r0 = mix64(z + G), r1 = mix64(z + 2 * G);
        s0 = uint32_t(r0);
        s1 = uint32_t(r0 >> 32);
        s2 = uint32_t(r1);
        s3 = uint32_t(r1 >> 32);
    }
    // The step as the reference writes it: eight two-input operations (the compiler never fuses the xors on its own).
    RPT_DEV uint32_t next_ref() {
        uint32_t r = s0 + s3;
        uint32_t t = s1 << 9;
        s2 ^= s0;
        s3 ^= s1;
        s1 ^= s2;
        s0 ^= s3;
        s2 ^= t;
        s3 = __builtin_rotateleft32(s3, 11);
        return r;
    }
    // The same function of the state with the intermediate values substituted: three v_bitop3_b32 (x ^ y ^ z) and one xor,
    // seven instructions for eight.
    RPT_DEV uint32_t next() {
        if constexpr ((FORMS & RPT_RNG_STEP) != 0) {
            const uint32_t a = s0, b = s1, c = s2, d = s3;
            const uint32_t r = a + d;
            const uint32_t t = b << 9;
            s1 = xor3(b, c, a);
            s0 = xor3(a, d, b);
            s2 = xor3(c, a, t);
            s3 = __builtin_rotateleft32(d ^ b, 11);
            return r;
        } else {
            return next_ref();
        }
    }
    // The odd 24-bit integer 2k+1 of a word, k = its top 23 bits, as a float (exact).
    RPT_DEV static float odd24(uint32_t word) { return float(((word >> 9) << 1) | 1u); }
    // (2k+1) * 2^-24 with k = top 23 bits: open interval (0,1), exact in fp32.
    RPT_DEV float uniform() { return odd24(next()) * 0x1p-24f; }
    RPT_DEV float uniform_ref() { return odd24(next_ref()) * 0x1p-24f; }
    RPT_DEV float range_ref(float a, float b) { return fmaf(b - a, uniform_ref(), a); }
    // a + (b - a) u with the 2^-24 of u moved into the width: both scalings are exact (no b - a the kernels use comes near the
    // denormals), the fma rounds the same real number, and the conversion's multiply is gone from every draw (constant or
    // wave-uniform widths: the scaled width is formed once).
    RPT_DEV float range(float a, float b) {
        if constexpr ((FORMS & RPT_RNG_RANGE) != 0) return fmaf((b - a) * 0x1p-24f, odd24(next()), a);
        else return fmaf(b - a, uniform(), a);
    }
    // uniform() < p on the word itself (see roulette_word).
    template <uint32_t T>
    RPT_DEV bool below(float p) {
        if constexpr ((FORMS & RPT_RNG_ROULETTE) != 0) return next() < T;
        else return uniform() < p;
    }
    RPT_DEV bool below_ref(float p) { return uniform_ref() < p; }
    RPT_DEV uint32_t index(uint32_t n) { return __umulhi(next(), n); }
    RPT_DEV void unit_disc(float& x, float& y) {  // rand_distr::UnitDisc (rejection)
        for (;;) {
            x = range(-1.f, 1.f);
            y = range(-1.f, 1.f);
            if (fmaf(x, x, y * y) <= 1.f) return;
        }
    }
};
using Rng = RngT<RPT_RNG_FORMS>;
// The accepted pair of a triangle sample, as the draws' top 23 bits (see sample_light_leaf): redraw while ku + kv >= 2^23, i.e. while
// the sum of the two words without their low nine bits carries out of 32 bits.  One mask is enough: the low nine bits of
// (a & ~511) + b are those of b alone and cannot carry into bit 9, so the carry out is that of (a & ~511) + (b & ~511).
template <uint32_t FORMS>
RPT_DEV void triangle_pair_ref(RngT<FORMS>& rng, uint32_t& ku, uint32_t& kv) {
    uint32_t wu = rng.next_ref() & ~511u, wv = rng.next_ref() & ~511u, sum;
    while (__builtin_add_overflow(wu, wv, &sum)) {
        wu = rng.next_ref() & ~511u;
        wv = rng.next_ref() & ~511u;
    }
    ku = wu >> 9;
    kv = wv >> 9;
}
template <uint32_t FORMS = RPT_RNG_FORMS>
RPT_DEV void triangle_pair(RngT<FORMS>& rng, uint32_t& ku, uint32_t& kv) {
    constexpr uint32_t kMaskV = (FORMS & RPT_RNG_ONE_MASK) ? ~0u : ~511u;
    uint32_t wu = rng.next() & ~511u, wv = rng.next() & kMaskV, sum;
    while (__builtin_add_overflow(wu, wv, &sum)) {
        wu = rng.next() & ~511u;
        wv = rng.next() & kMaskV;
    }
    ku = wu >> 9;
    kv = wv >> 9;
}

// ------------------------------------------------------------------ primitive tests
// Each returns the hit parameter or a negative value for "no hit in [tmin, tmax)".
// `t` is shared between world and local space because the local direction is not
// renormalised (Ray::apply_transform, src/shape.rs:65-72).

// Unit sphere, src/shape/sphere.rs:14-46.  Same roots as the reference's (-b -/+ sqrt(b^2-ac))/a,
// evaluated through the closest-approach vector so fp32 keeps the discriminant's digits.
RPT_DEV bool sphere_closer(V ol, V dl, float tmin, float tbest, float& t);
RPT_DEV float hit_sphere(V ol, V dl, float tmin) {
    float t;
    return sphere_closer(ol, dl, tmin, __builtin_inff(), t) ? t : -1.f;
}
// The scans' form of the three bounded primitives: "is there an accepted root closer than tbest", one chain of compares
// (a negative discriminant leaves NaN in t, which fails them).  hit_sphere / hit_cube / hit_aabb are these
// with tbest = inf, and the bodies are compiled without fp contraction (their fmas are written out): a scan and a tree
// walk that reach the same primitive then get the same bits for t wherever the body is inlined.
RPT_DEV bool sphere_closer(V ol, V dl, float tmin, float tbest, float& t) {
#pragma clang fp contract(off)
    float a = dot(dl, dl);
    float inv_a = rcp(a);
    float bb = dot(dl, ol) * inv_a;
    V l = fma3(-bb, dl, ol);
    float sq = sqrt1((1.f - dot(l, l)) * inv_a);
    float t0 = -bb - sq;
    t = (t0 < tmin) ? -bb + sq : t0;
    return t >= tmin && t < tbest;
}
RPT_DEV bool slabs_closer(float x1, float x2, float y1, float y2, float z1, float z2, float tmin, float tbest, float& t) {
#pragma clang fp contract(off)
    const float start = max3(fminf(x1, x2), fminf(y1, y2), fminf(z1, z2));
    const float end = min3(fmaxf(x1, x2), fmaxf(y1, y2), fmaxf(z1, z2));
    t = start < tmin ? end : start;
    return !(start > end) && !(end < tmin) && t < tbest;
}
RPT_DEV bool cube_closer(V ol, V dl, float tmin, float tbest, float& t) {
#pragma clang fp contract(off)
    float ix = rcp(dl.x), iy = rcp(dl.y), iz = rcp(dl.z);
    return slabs_closer((-0.5f - ol.x) * ix, (0.5f - ol.x) * ix, (-0.5f - ol.y) * iy, (0.5f - ol.y) * iy, (-0.5f - ol.z) * iz,
                        (0.5f - ol.z) * iz, tmin, tbest, t);
}
RPT_DEV bool aabb_closer(const F4& lo, const F4& hi, V o, V inv, float tmin, float tbest, float& t) {
#pragma clang fp contract(off)
    return slabs_closer((lo.x - o.x) * inv.x, (hi.x - o.x) * inv.x, (lo.y - o.y) * inv.y, (hi.y - o.y) * inv.y,
                        (lo.z - o.z) * inv.z, (hi.z - o.z) * inv.z, tmin, tbest, t);
}
// Unit cube [-1/2,1/2]^3, src/shape/cube.rs:22-74: t of the accepted root (the face is found afterwards, for the winner alone: box_face_normal).
RPT_DEV float hit_cube(V ol, V dl, float tmin) {
    float t;
    return cube_closer(ol, dl, tmin, __builtin_inff(), t) ? t : -1.f;
}
// Plane, src/shape/plane.rs:17-32 (world-space (n, value)).
RPT_DEV float hit_plane(const F4& nv, V o, V d, float tmin) {
    float c = dot3(nv, d);
    if (fabsf(c) < 1e-8f) return -1.f;
    float t = (nv.w - dot3(nv, o)) * rcp(c);
    return (t >= tmin) ? t : -1.f;
}
// The scans' form, as sphere_closer: "is there an accepted t closer than tbest" (hit_plane's value with the compare the scan
// puts behind it: the scan then selects tbest once instead of selecting -1 first and comparing that with 0).  The same accepts
// because tmin > 0 in every caller (ray_tmin): t >= tmin implies the t >= 0 that followed hit_plane.  tri_closer, rect_closer alike.
RPT_DEV bool plane_closer(const F4& nv, V o, V d, float tmin, float tbest, float& t) {
    float c = dot3(nv, d);
    t = (nv.w - dot3(nv, o)) * rcp(c);
    return !(fabsf(c) < 1e-8f) && t >= tmin && t < tbest;
}
// Triangle, src/shape/mesh.rs:50-83, with the plane normal and the barycentric functionals
// pre-solved on the host.  Accepts t in [tmin, tmax).
RPT_DEV bool tri_closer(const F4& pn, const F4& A, const F4& B, V o, V d, float tmin, float tmax, float& t) {
    float c = dot3(pn, d);
    t = (pn.w - dot3(pn, o)) * rcp(c);
    V p = fma3(t, d, o);
    float v = dot3w(A, p), w = dot3w(B, p);
    float u = 1.f - v - w;
    return fabsf(c) >= 1e-8f && t >= tmin && t < tmax && u >= 0.f && v >= 0.f && w >= 0.f;
}
RPT_DEV float hit_tri(const F4& pn, const F4& A, const F4& B, V o, V d, float tmin, float tmax) {
    float t;
    return tri_closer(pn, A, B, o, d, tmin, tmax, t) ? t : -1.f;
}
// Axis-aligned box in world space (a cube under positive scale + translation): the reference's
// local slab test (src/shape/cube.rs:22-74) evaluated in world coordinates, where it yields the
// same entry/exit parameters because t is shared between the two spaces.  `inv` = 1/d.
RPT_DEV float hit_aabb(const F4& lo, const F4& hi, V o, V inv, float tmin) {
    float t;
    return aabb_closer(lo, hi, o, inv, tmin, __builtin_inff(), t) ? t : -1.f;
}
// Axis-aligned rectangle = two coplanar triangles of src/shape/mesh.rs:50-83 (u,v,w >= 0 on one
// of them <=> the point lies in the closed rectangle).  oa/da/ia: origin, direction and 1/direction
// on the rectangle's axis; (ou,du), (ov,dv) on the two in-plane axes.
RPT_DEV bool rect_closer(const F4& a, float vmax, float oa, float ia, float ou, float du, float ov, float dv,
                         float tmin, float tmax, float& t) {
    t = (a.x - oa) * ia;
    float pu = fmaf(t, du, ou), pv = fmaf(t, dv, ov);
    return t >= tmin && t < tmax && pu >= a.y && pu <= a.z && pv >= a.w && pv <= vmax;
}
RPT_DEV float hit_rect(const F4& a, float vmax, float oa, float ia, float ou, float du, float ov, float dv,
                       float tmin, float tmax) {
    float t;
    return rect_closer(a, vmax, oa, ia, ou, du, ov, dv, tmin, tmax, t) ? t : -1.f;
}
// Box shell (ShellScan): the closest rectangle among the faces of one axis-aligned box = the slab entry if
// that face exists and lies at or beyond tmin, else the slab exit.  Same t = (plane - o) * inv as hit_rect.
// `acc(ok, t, code_of)`: what the caller keeps of an accepted face (code_of() selects its hit code: the shadow form never calls it;
// which faces exist is decided from the codes either way, because an open face must not hit).
template <class Acc>
RPT_DEV void shell_closer(const ShellScan& s, V o, V inv, float tmin, float tbest, Acc&& acc) {
    float x1 = (s.lo.x - o.x) * inv.x, x2 = (s.hi.x - o.x) * inv.x;
    float y1 = (s.lo.y - o.y) * inv.y, y2 = (s.hi.y - o.y) * inv.y;
    float z1 = (s.lo.z - o.z) * inv.z, z2 = (s.hi.z - o.z) * inv.z;
    bool sx = x1 > x2, sy = y1 > y2, sz = z1 > z2;
    float xl = sx ? x2 : x1, xh = sx ? x1 : x2;
    float yl = sy ? y2 : y1, yh = sy ? y1 : y2;
    float zl = sz ? z2 : z1, zh = sz ? z1 : z2;
    float start = max3(xl, yl, zl), end = min3(xh, yh, zh);
    // entering through the lo face of an axis unless the direction is negative there (swapped)
    uint32_t in_x = sx ? s.face[1] : s.face[0], out_x = sx ? s.face[0] : s.face[1];
    uint32_t in_y = sy ? s.face[3] : s.face[2], out_y = sy ? s.face[2] : s.face[3];
    uint32_t in_z = sz ? s.face[5] : s.face[4], out_z = sz ? s.face[4] : s.face[5];
    uint32_t c_in = (xl > yl && xl > zl) ? in_x : (yl > zl ? in_y : in_z);
    uint32_t c_out = (xh < yh && xh < zh) ? out_x : (yh < zh ? out_y : out_z);
    bool box = start <= end;
    bool use_in = box && start >= tmin && c_in != CODE_MISS;
    bool use_out = box && end >= tmin && c_out != CODE_MISS;
    float t = use_in ? start : end;
    acc((use_in || use_out) && t < tbest, t, [&] { return use_in ? c_in : c_out; });
}
RPT_DEV void to_local(const XfScan& x, V o, V d, V& ol, V& dl) {
    ol = mk(dot3w(x.r0, o), dot3w(x.r1, o), dot3w(x.r2, o));
    dl = mk(dot3(x.r0, d), dot3(x.r1, d), dot3(x.r2, d));
}
// to_local for a record whose rows hold exact zeros at r0.y, r1.x, r1.z and r2.y (a rotation about the vertical axis under any
// scale and translation: SceneView::sph_yrot / cub_yrot, set at commit): the same fma chains with the terms fma(0, p, acc) and
// 0 * p left out, 10 operations instead of 18.  Such a term returns acc exactly, so ol and dl keep their bits -- except that a
// result which is zero may change its sign (-0 + 0 = +0).  In dl that swaps the +inf / -inf of a slab pair, whose min / max are
// unchanged; tests/test_gpu_scan_specialise.py holds t and the hit code bit-equal to the generic form's.
RPT_DEV void to_local_y(const XfScan& x, V o, V d, V& ol, V& dl) {
    ol = mk(fmaf(x.r0.x, o.x, fmaf(x.r0.z, o.z, x.r0.w)), fmaf(x.r1.y, o.y, x.r1.w), fmaf(x.r2.x, o.x, fmaf(x.r2.z, o.z, x.r2.w)));
    dl = mk(fmaf(x.r0.x, d.x, x.r0.z * d.z), x.r1.y * d.y, fmaf(x.r2.x, d.x, x.r2.z * d.z));
}
// Two world-space boxes that are adjacent in the scan, tested in record order: aabb_closer twice, operation for operation.  `shared`:
// the axes (bit 0 = x, 1 = y, 2 = z) on which the second box's lo and hi are bit-equal to the first's (AabbScan::hi.w of the first,
// wave-uniform): its slab interval there IS the first box's -- identical operands, identical results -- and is not computed again.
// One uniform if per axis rather than a body per combination: every combination is served, and a three-way choice between whole
// bodies compiles to a chain of flag tests that costs ~60 scalar instructions per trip on C3.  The first box's entry / exit are
// pinned before the ifs: sunk below them they keep its intervals alive, and each shared one then costs two register copies.
template <class Acc>
RPT_DEV void aabb_pair_closer(const AabbScan& b0, const AabbScan& b1, uint32_t shared, V o, V inv, float tmin, float& tbest, uint32_t i,
                              Acc&& acc) {   // acc(ok, t, record): `ok` was formed against tbest, which acc lowers (scan_prims)
#pragma clang fp contract(off)
    const float x1 = (b0.lo.x - o.x) * inv.x, x2 = (b0.hi.x - o.x) * inv.x;
    const float y1 = (b0.lo.y - o.y) * inv.y, y2 = (b0.hi.y - o.y) * inv.y;
    const float z1 = (b0.lo.z - o.z) * inv.z, z2 = (b0.hi.z - o.z) * inv.z;
    float xl = fminf(x1, x2), xh = fmaxf(x1, x2), yl = fminf(y1, y2), yh = fmaxf(y1, y2), zl = fminf(z1, z2), zh = fmaxf(z1, z2);
    float start = max3(xl, yl, zl), end = min3(xh, yh, zh);   // slabs_closer from here on
    asm volatile("" : "+v"(start), "+v"(end));
    float t = start < tmin ? end : start;
    acc(!(start > end) && !(end < tmin) && t < tbest, t, i);
    if (!(shared & 1u)) { const float u1 = (b1.lo.x - o.x) * inv.x, u2 = (b1.hi.x - o.x) * inv.x; xl = fminf(u1, u2); xh = fmaxf(u1, u2); }
    if (!(shared & 2u)) { const float u1 = (b1.lo.y - o.y) * inv.y, u2 = (b1.hi.y - o.y) * inv.y; yl = fminf(u1, u2); yh = fmaxf(u1, u2); }
    if (!(shared & 4u)) { const float u1 = (b1.lo.z - o.z) * inv.z, u2 = (b1.hi.z - o.z) * inv.z; zl = fminf(u1, u2); zh = fmaxf(u1, u2); }
    start = max3(xl, yl, zl), end = min3(xh, yh, zh);
    t = start < tmin ? end : start;
    acc(!(start > end) && !(end < tmin) && t < tbest, t, i + 1u);
}
// MonomialSurface::intersect, src/shape/monomial_surface.rs:22-107, in the surface's local space (t is shared), step for step:
// the box test against [-1, 0, -1]..[1, h, 1] (min / max per axis, so h <= 0 works), maximize = dist(t_min) < 0, Newton from
// the box's midpoint (at most 10 steps, leaving as soon as dist > 0) for the end of the bracket -- or 10000 --, the sign check,
// exactly 60 bisection steps, then `r > tbest` (an equal time replaces the record) and the x^2 + z^2 > 1 rejection.  The fp32
// policy's one addition: a NaN or infinite root is a miss.  The quartic costs ~700 flops per ray, so a
// wave leaves before the solve when none of its lanes passes the box test; the lanes that do run the 60 steps together.
// Compiled without contraction (fmas written out), as sphere_closer: the scan and the tree walks get the same bits.
RPT_DEV bool mono_closer(V ol, V dl, const F4& hb, float tmin, float tbest, float& t) {
#pragma clang fp contract(off)
    const float ix = rcp(dl.x), iy = rcp(dl.y), iz = rcp(dl.z);
    const float x1 = (-1.f - ol.x) * ix, x2 = (1.f - ol.x) * ix;
    const float y1 = (hb.y - ol.y) * iy, y2 = (hb.z - ol.y) * iy;
    const float z1 = (-1.f - ol.z) * iz, z2 = (1.f - ol.z) * iz;
    const float b_min = max3(fminf(x1, x2), fminf(y1, y2), fminf(z1, z2));
    const float b_max = min3(fmaxf(x1, x2), fmaxf(y1, y2), fmaxf(z1, z2));
    const bool in_box = !(fmaxf(b_min, tmin) > fminf(b_max, tbest));
    if (__ballot(in_box) == 0ull) return false;   // (wave-uniform: nobody solves)
    if (!in_box) return false;
    const float h = hb.x;
    auto dist = [&](float s) {   // :27-32
        const float x = fmaf(s, dl.x, ol.x), y = fmaf(s, dl.y, ol.y), z = fmaf(s, dl.z, ol.z);
        const float r2 = fmaf(x, x, z * z);
        return fmaf(-h, r2 * r2, y);
    };
    // :33-48, in Horner form: deriv = d.y - h (A + s (B + s (C + s D))), deriv2 = -h (B + s (2 C + s 3 D))
    const float c0 = fmaf(ol.x, ol.x, ol.z * ol.z), c1 = 2.f * fmaf(ol.x, dl.x, ol.z * dl.z), c2 = fmaf(dl.x, dl.x, dl.z * dl.z);
    const float A = 2.f * c0 * c1, B = 2.f * fmaf(c1, c1, 2.f * c0 * c2), Cq = 6.f * c1 * c2, Dq = 4.f * c2 * c2;
    const float d_tmin = dist(tmin);
    const bool maximize = d_tmin < 0.f;   // :50
    float t_max = 10000.f;                // :70
    if (maximize) {                       // :51-68
        float cur = 0.5f * (b_min + b_max);
        for (int k = 0; k < 10; k++) {
            if (dist(cur) > 0.f) break;
            const float der = fmaf(-h, fmaf(cur, fmaf(cur, fmaf(cur, Dq, Cq), B), A), dl.y);
            const float der2 = -h * fmaf(cur, fmaf(cur, 3.f * Dq, 2.f * Cq), B);
            cur -= der / der2;
        }
        t_max = cur;
        if (t_max < tmin) return false;
    }
    if (maximize == (dist(t_max) < 0.f)) return false;   // :72-74
    float l = tmin, r = t_max;
    for (int k = 0; k < 60; k++) {        // :75-84
        const float m = (l + r) * 0.5f;
        if ((dist(m) >= 0.f) == maximize) r = m;
        else l = m;
    }
    if (r > tbest || !(fabsf(r) < __builtin_huge_valf())) return false;   // :85-87; NaN / inf: a miss (fp32 policy)
    const float px = fmaf(r, dl.x, ol.x), pz = fmaf(r, dl.z, ol.z);
    if (fmaf(px, px, pz * pz) > 1.f) return false;   // :88-92
    t = r;
    return true;
}

// ------------------------------------------------------------------ closest hit
// Renderer::get_closest_hit, src/renderer.rs:416-425: every object is tested, the closest
// accepted hit wins, ties keep the earlier object (strict `<`).  The analytic primitives are
// scanned with a wave-uniform index (scalar loads); BVH meshes are walked per lane.
// Per-lane BVH walk ("while-while"): descend inner nodes until every lane of the wave holds a
// leaf (or is done), then test the leaves' triangles together.  Stack = one LDS column per lane.
RPT_DEV void slab2(const float lo[3], const float hi[3], V o, V inv, float& tn, float& tf) {
    float x1 = (lo[0] - o.x) * inv.x, x2 = (hi[0] - o.x) * inv.x;
    float y1 = (lo[1] - o.y) * inv.y, y2 = (hi[1] - o.y) * inv.y;
    float z1 = (lo[2] - o.z) * inv.z, z2 = (hi[2] - o.z) * inv.z;
    tn = max3(fminf(x1, x2), fminf(y1, y2), fminf(z1, z2));
    tf = min3(fmaxf(x1, x2), fmaxf(y1, y2), fmaxf(z1, z2));
}
// Occluder test of a shadow walk: a hit closer than t_block on anything but the light's twin primitives
// (hit codes tw_lo..tw_hi) decides the shadow test -- the walk may stop without finding the closest hit.
struct AnyHit {
    float t_block;
    uint32_t tw_lo, tw_hi;
    RPT_DEV bool blocks(float t, uint32_t code) const { return t < t_block && !(code >= tw_lo && code <= tw_hi); }
};
template <bool COUNT, bool PRIMS, bool ANY = false, bool MONO = false>
RPT_DEV void bvh_traverse(const SceneView& sc, uint32_t root, V o, V d, float tmin, float& tbest, uint32_t& code,
                          uint32_t& inst, uint32_t* stk, uint32_t stride, uint32_t cap, uint32_t& c_nodes,
                          uint32_t& c_tris, AnyHit any = AnyHit{-kInf, 1u, 0u});

// One primitive of a BVH_PRIMS leaf (per lane: kinds may differ between lanes).  `stk`/`cap`:
// the part of the lane's stack column above the caller's entries, for the nested walk of an instance.
// MONO: the scene holds monomial surfaces (K_MONO leaf items; an instantiation of its own).
template <bool COUNT, bool MONO = false>
RPT_DEV void hit_prim(const SceneView& scene_, uint32_t pc, V o, V d, V inv, float tmin, float& tbest, uint32_t& code,
                      uint32_t& inst, uint32_t* stk, uint32_t stride, uint32_t cap, uint32_t& c_nodes,
                      uint32_t& c_tris) {
    const auto& sc = *kernarg_scene();   // (see kernarg_scene)
    const uint32_t kind = pc >> 28, i = pc & 0x0FFFFFFFu;
    float t = -1.f;
    if (MONO && kind == K_MONO) {
        const MonoScan m = sc.mono[i];
        V ol, dl;
        to_local(XfScan{m.r0, m.r1, m.r2}, o, d, ol, dl);
        if (mono_closer(ol, dl, m.h, tmin, tbest, t)) { tbest = t; code = pc; }
        return;
    }
    if (kind == K_INST) {
        const InstRec r = sc.inst[i];
        const V ol = mk(dot3w(r.r0, o), dot3w(r.r1, o), dot3w(r.r2, o));
        const V dl = mk(dot3(r.r0, d), dot3(r.r1, d), dot3(r.r2, d));   // not renormalised: t is shared
        uint32_t c2 = CODE_MISS, unused = 0;
        float tb = tbest;
        bvh_traverse<COUNT, false>(scene_, __float_as_uint(r.n1.w), ol, dl, tmin, tb, c2, unused, stk, stride, cap, c_nodes,
                                   c_tris);
        if (c2 != CODE_MISS) { tbest = tb; code = (K_INSTTRI << 28) | (c2 & 0x0FFFFFFFu); inst = i; }
        return;
    }
    if (kind == K_SPHERE) {
        const XfScan x = sc.sph[i];
        V ol, dl;
        to_local(x, o, d, ol, dl);
        t = hit_sphere(ol, dl, tmin);
    } else if (kind == K_CUBE) {
        const XfScan x = sc.cub[i];
        V ol, dl;
        to_local(x, o, d, ol, dl);
        t = hit_cube(ol, dl, tmin);
    } else if (kind == K_AABB) {
        const AabbScan b = sc.aabb[i];
        t = hit_aabb(b.lo, b.hi, o, inv, tmin);
    } else if (kind == K_RECT) {
        const RectScan r = sc.rect[i];
        if (i < sc.n_rect_x) t = hit_rect(r.a, r.b.x, o.x, inv.x, o.y, d.y, o.z, d.z, tmin, tbest);
        else if (i < sc.n_rect_x + sc.n_rect_y) t = hit_rect(r.a, r.b.x, o.y, inv.y, o.z, d.z, o.x, d.x, tmin, tbest);
        else t = hit_rect(r.a, r.b.x, o.z, inv.z, o.x, d.x, o.y, d.y, tmin, tbest);
    } else {  // K_TRI
        const TriScan tr = sc.tri[i];
        t = hit_tri(tr.pn, tr.A, tr.B, o, d, tmin, tbest);
    }
    if (t >= 0.f && t < tbest) { tbest = t; code = pc; }
}

template <bool COUNT, bool PRIMS, bool ANY, bool MONO>
RPT_DEV void bvh_traverse(const SceneView& scene_, uint32_t root, V o, V d, float tmin, float& tbest, uint32_t& code,
                          uint32_t& inst, uint32_t* stk, uint32_t stride, uint32_t cap, uint32_t& c_nodes,
                          uint32_t& c_tris, AnyHit any) {
    const auto& sc = *kernarg_scene();   // (see kernarg_scene)
    const BvhNode* nodes = sc.nodes;
    const V inv = mk(rcp(d.x), rcp(d.y), rcp(d.z));
    const uint32_t kDone = 0xFFFFFFFFu;  // a 32-item prim leaf at the last index never occurs
    uint32_t sp = 0;
    uint32_t cur = root;  // a root is always an inner node
    while (cur != kDone) {
        while (!(cur & BVH_LEAF)) {  // kDone has the leaf bit set, so finished lanes fall through
            const BvhNode nd = nodes[cur];
            if (COUNT) c_nodes++;
            float n0, f0, n1, f1;
            slab2(nd.lo0, nd.hi0, o, inv, n0, f0);
            slab2(nd.lo1, nd.hi1, o, inv, n1, f1);
            const bool h0 = fmaxf(n0, tmin) <= fminf(f0, tbest);
            const bool h1 = fmaxf(n1, tmin) <= fminf(f1, tbest);
            if (h0 && h1) {
                const bool first0 = n0 <= n1;
                if (sp < cap) { stk[sp * stride] = first0 ? nd.e1 : nd.e0; sp++; }
                else if (COUNT && sc.stack_overflows) atomicAdd(sc.stack_overflows, 1ull);   // (never, by the commit-time depth check)
                cur = first0 ? nd.e0 : nd.e1;
            } else if (h0 || h1) {
                cur = h0 ? nd.e0 : nd.e1;
            } else if (sp) {
                sp--;
                cur = stk[sp * stride];
            } else {
                cur = kDone;
            }
        }
        if (cur != kDone) {
            const uint32_t first = cur & BVH_INDEX_MASK;
            const uint32_t count = ((cur >> 26) & 31u) + 1u;
            if (PRIMS && (cur & BVH_PRIMS)) {
                for (uint32_t i = 0; i < count; i++) {
                    if (COUNT) c_tris++;
                    hit_prim<COUNT, MONO>(scene_, sc.pleaf[first + i], o, d, inv, tmin, tbest, code, inst, stk + sp * stride, stride,
                                    cap - sp, c_nodes, c_tris);
                }
            } else {
                for (uint32_t i = 0; i < count; i++) {
                    const TriScan tr = sc.btri[first + i];
                    if (COUNT) c_tris++;
                    float t = hit_tri(tr.pn, tr.A, tr.B, o, d, tmin, tbest);
                    if (t >= 0.f) { tbest = t; code = (K_BVHTRI << 28) | (first + i); }
                }
            }
            if (ANY && code != CODE_MISS && any.blocks(tbest, code)) sp = 0;  // an occluder is known: nothing left to find
            if (sp) {
                sp--;
                cur = stk[sp * stride];
            } else {
                cur = kDone;
            }
        }
    }
}

// Does the lane's interval [tmin, tbest) overlap the slab interval of the box?  The slab pairs are ordered as the scan orders them, so
// that a NaN ((plane - o) * inv with o in the plane and the direction parallel to it) is treated as there: with fminf / fmaxf, which
// drop it, like slabs_closer (box records); SHELL: with a compare and two selects like hit_shell, where a NaN leaves the pair's other
// value as the only bound.  The final comparison lets a NaN pass.
template <bool SHELL>
RPT_DEV bool interval_meets_box(const SceneView::ScanBox& b, V o, V inv, float tmin, float tbest) {
#pragma clang fp contract(off)
    const float x1 = (b.lo[0] - o.x) * inv.x, x2 = (b.hi[0] - o.x) * inv.x;
    const float y1 = (b.lo[1] - o.y) * inv.y, y2 = (b.hi[1] - o.y) * inv.y;
    const float z1 = (b.lo[2] - o.z) * inv.z, z2 = (b.hi[2] - o.z) * inv.z;
    float start, end;
    if (SHELL) {
        const bool sx = x1 > x2, sy = y1 > y2, sz = z1 > z2;
        start = max3(sx ? x2 : x1, sy ? y2 : y1, sz ? z2 : z1);
        end = min3(sx ? x1 : x2, sy ? y1 : y2, sz ? z1 : z2);
    } else {
        start = max3(fminf(x1, x2), fminf(y1, y2), fminf(z1, z2));
        end = min3(fmaxf(x1, x2), fmaxf(y1, y2), fmaxf(z1, z2));
    }
    return !(fmaxf(start, tmin) > fminf(end, tbest));
}
// The linear scan over the wave-uniform primitive records (everything that is not in a tree).
// MASKED: bit i of `mask` (wave-uniform) says whether bounded record i -- numbered in scan order: spheres, cubes,
// boxes, rectangles, triangles, as in SceneView::pbox -- can be hit at all; planes and the shell are always tested.
// MONO: ... and then the monomial surfaces; an instantiation of its own.  Not with MASKED: scan_mask_for_ball numbers only the
// records up to the triangles (only photon mapping masks its scans, and it refuses scenes with monomial surfaces).
// TAIL (the primary scans in a medium; option "scan_cull"): the records behind the shell in scan order -- boxes, rectangles, triangles --
// are left out when no lane's interval [tmin, tbest) reaches the box around them (SceneView::scan_tail; tbest as the records before
// them have left it).  A primary interval mostly ends at the sampled medium distance: on C3 the tail is the lampshade under the
// ceiling, which four trips in five do not reach.  One slab test and one ballot; the records that are tested are tested as ever, and a record
// that is left out could not have been accepted by any lane (rpt_capi.cpp, group_scans, has the rounding argument).  tail_skipped
// (counters builds): set when the tail was left out.
// SHADOW (the shadow query of an object light whose twin -- the scene object that IS the light -- is one index range of one scanned
// kind; option "shadow_scan"): the light test reads one bit of the closest hit, "it is a twin record", so this form keeps no hit code.
// The tbest chain is the closest-hit form's, compare for compare; beside it runs one lane predicate, "the best so far is a twin
// record": an accepted twin record sets it, every other accepted record clears it (clearing before the twin range changes nothing:
// it is still false there).  Which of the two a record does is wave-uniform -- the kind's loop is chosen once per kind, and only the
// twin kind's loop looks at the index -- and the predicate lives in a scalar register pair.  `twin`: see ShadowTwin.
// Why the bit is the closest-hit form's `code in [twin_lo, twin_hi]`: DESIGN.md section 4, round 7.
struct ShadowTwin {
    uint32_t kind, lo, span;   // twin records: kind `kind`, indices lo .. lo + span
    RPT_DEV bool has(uint32_t i) const { return i - lo <= span; }
};
// What a scan knows about the scene before it reads a record: how many records of each kind there are, whether there is a shell,
// which spheres and cubes are y-rotations, whether the tail cull is on -- all fixed when the scene is committed.  SHAPE says where these
// come from.  ScanShapeRt: from the launch's view, each read at its place of use, as ever.  ScanShapeK (builds with
// -DRPT_SCAN_SHAPE=n_sph,n_cub,n_pln,n_aabb,n_rect_x,n_rect_y,n_rect_z,n_tri,has_shell,scan_cull,sph_yrot,cub_yrot): constants, so that
// an empty kind's loop, its count's load and its branch are not compiled at all and a short loop has no loop control.  Record values
// -- transforms, boxes, the tail box -- are read from memory in both.
struct ScanShapeRt {
    KernargView sc;
    RPT_DEV uint32_t n_sph() const { return sc->n_sph; }
    RPT_DEV uint32_t n_cub() const { return sc->n_cub; }
    RPT_DEV uint32_t n_pln() const { return sc->n_pln; }
    RPT_DEV uint32_t n_aabb() const { return sc->n_aabb; }
    RPT_DEV uint32_t n_rect_x() const { return sc->n_rect_x; }
    RPT_DEV uint32_t n_rect_y() const { return sc->n_rect_y; }
    RPT_DEV uint32_t n_rect_z() const { return sc->n_rect_z; }
    RPT_DEV uint32_t n_tri() const { return sc->n_tri; }
    RPT_DEV uint32_t has_shell() const { return sc->has_shell; }
    RPT_DEV uint32_t scan_cull() const { return sc->scan_cull; }
    RPT_DEV uint64_t sph_yrot() const { return sc->sph_yrot; }
    RPT_DEV uint64_t cub_yrot() const { return sc->cub_yrot; }
};
#ifdef RPT_SCAN_SHAPE
struct ScanShapeK {
    KernargView sc;
    static constexpr uint64_t k[12] = {RPT_SCAN_SHAPE};
    RPT_DEV constexpr uint32_t n_sph() const { return uint32_t(k[0]); }
    RPT_DEV constexpr uint32_t n_cub() const { return uint32_t(k[1]); }
    RPT_DEV constexpr uint32_t n_pln() const { return uint32_t(k[2]); }
    RPT_DEV constexpr uint32_t n_aabb() const { return uint32_t(k[3]); }
    RPT_DEV constexpr uint32_t n_rect_x() const { return uint32_t(k[4]); }
    RPT_DEV constexpr uint32_t n_rect_y() const { return uint32_t(k[5]); }
    RPT_DEV constexpr uint32_t n_rect_z() const { return uint32_t(k[6]); }
    RPT_DEV constexpr uint32_t n_tri() const { return uint32_t(k[7]); }
    RPT_DEV constexpr uint32_t has_shell() const { return uint32_t(k[8]); }
    RPT_DEV constexpr uint32_t scan_cull() const { return uint32_t(k[9]); }
    RPT_DEV constexpr uint64_t sph_yrot() const { return k[10]; }
    RPT_DEV constexpr uint64_t cub_yrot() const { return k[11]; }
};
#else
typedef ScanShapeRt ScanShapeK;
#endif
// What the code AROUND the scans knows about the scene before it reads a record -- the second constant block of the scan JIT
// (DESIGN.md section 4, round 11): which lights there are and of what kind and shape, whether the small tables are staged in LDS, which
// material kinds occur, the medium's kind, whether there is an HDRI, the box pairs' common slabs.  All of it is fixed at commit.
// SceneStructRt: every question is answered from the record or the view at its place of use, as ever.  SceneStructK (builds with
// -DRPT_SCENE_STRUCT=groups,n_lights,light word x 4,twin_lo x 4,twin_hi x 4,material mask,medium_kind,hdri,pair bits): constants, one
// group of them per bit of `groups`, so that a build can take them singly; a group whose bit is clear answers as SceneStructRt does.
// Record VALUES -- colours, transforms, boxes, light triangles, a mesh light's count and first -- stay data in both.  No constant of the
// block is a floating-point operand: nothing the compiler could fold through an approximate instruction (rcp, rsq, sqrt).
// A light word: bits 0-1 kind, 2-3 shape, 4 its LightXf has a transform, 5 twin_object >= 0, 6 the twin is a code range (lo <= hi).
// (The group bits SS_*, kStructLights and kStructPairs: gpu_layout.h, shared with the host.)
struct LightRt {   // one light of the light loop, known from its record
    uint32_t i;
    RPT_DEV uint32_t kind(const Light& L) const { return L.kind; }
    RPT_DEV uint32_t shape(const Light& L) const { return L.shape; }
    RPT_DEV bool has_twin(const Light& L) const { return L.twin_object >= 0; }
    RPT_DEV bool has_range(const Light& L) const { return L.twin_lo <= L.twin_hi; }
    RPT_DEV uint32_t twin_lo(const Light& L) const { return L.twin_lo; }
    RPT_DEV uint32_t twin_hi(const Light& L) const { return L.twin_hi; }
    template <class X> RPT_DEV bool has_xf(const X& x) const { return x.has_transform(); }
};
struct SceneStructRt {
    static constexpr bool kLights = false;
    typedef LightRt LightAt;
    static RPT_DEV uint32_t light_count(uint32_t n_lights) { return n_lights; }
    static RPT_DEV bool mat_staged(uint32_t obj, uint32_t n_staged) { return obj < n_staged; }
    static RPT_DEV bool ltri_staged(uint32_t i, uint32_t n_staged) { return i < n_staged; }
    static RPT_DEV bool is_mat(uint32_t kind, uint32_t which) { return kind == which; }
    static RPT_DEV bool mat_has_colour(uint32_t kind) { return kind <= 1u; }
    static RPT_DEV bool fog_by_height(uint32_t medium_kind) { return medium_kind == 1u; }
    static RPT_DEV bool has_hdri(uint32_t hdri_w) { return hdri_w != 0u; }
    static RPT_DEV uint32_t pair_shared(uint32_t, uint32_t word) { return word; }
};
#ifdef RPT_SCENE_STRUCT
struct SceneStructK;
struct LightK {   // light i of the light loop, known from the block (the loop is unrolled: i is a constant in every copy of its body)
    uint32_t i;
    template <uint32_t AT> RPT_DEV constexpr uint32_t word() const;
    RPT_DEV constexpr uint32_t kind(const Light&) const { return word<2u>() & 3u; }
    RPT_DEV constexpr uint32_t shape(const Light&) const { return (word<2u>() >> 2) & 3u; }
    RPT_DEV constexpr bool has_twin(const Light&) const { return ((word<2u>() >> 5) & 1u) != 0u; }
    RPT_DEV constexpr bool has_range(const Light&) const { return ((word<2u>() >> 6) & 1u) != 0u; }
    RPT_DEV constexpr uint32_t twin_lo(const Light&) const { return word<6u>(); }
    RPT_DEV constexpr uint32_t twin_hi(const Light&) const { return word<10u>(); }
    template <class X> RPT_DEV constexpr bool has_xf(const X&) const { return ((word<2u>() >> 4) & 1u) != 0u; }
};
struct SceneStructK {
    static constexpr uint64_t k[18] = {RPT_SCENE_STRUCT};
    static constexpr uint32_t groups = uint32_t(k[0]), mats = uint32_t(k[14]);
    static constexpr bool kLights = (groups & SS_LIGHTS) != 0u;
    static_assert(!kLights || k[1] <= kStructLights, "the block describes at most kStructLights lights");
    typedef tt::conditional_t<kLights, LightK, LightRt> LightAt;
    static RPT_DEV constexpr uint32_t light_count(uint32_t n_lights) { return kLights ? uint32_t(k[1]) : n_lights; }
    static RPT_DEV constexpr bool mat_staged(uint32_t obj, uint32_t n_staged) { return (groups & SS_TABLES) ? true : obj < n_staged; }
    static RPT_DEV constexpr bool ltri_staged(uint32_t i, uint32_t n_staged) { return (groups & SS_TABLES) ? true : i < n_staged; }
    static RPT_DEV constexpr bool is_mat(uint32_t kind, uint32_t which) {
        if (!(groups & SS_MATS)) return kind == which;
        return !((mats >> which) & 1u) ? false : (mats == (1u << which) ? true : kind == which);
    }
    static RPT_DEV constexpr bool mat_has_colour(uint32_t kind) {
        if (!(groups & SS_MATS)) return kind <= 1u;
        return !(mats & ~3u) ? true : (!(mats & 3u) ? false : kind <= 1u);
    }
    static RPT_DEV constexpr bool fog_by_height(uint32_t medium_kind) { return (groups & SS_SMALL) ? k[15] == 1u : medium_kind == 1u; }
    // Only the ABSENCE of an HDRI is a constant (the lookup is not compiled).  With its presence a constant too, the lookup loses the branch
    // around it and the compiler contracts its bilinear sums (a * b + c * d: either product can go into the fma) the other way round: frames
    // one ulp off the AOT kernel's in a fifth of the pixels (profiles/r11/scan_jit_structure.txt).  A scene with an HDRI asks the view, as ever.
    static RPT_DEV constexpr bool has_hdri(uint32_t hdri_w) { return ((groups & SS_SMALL) && k[16] == 0u) ? false : hdri_w != 0u; }
    static RPT_DEV constexpr uint32_t pair_shared(uint32_t i, uint32_t word) { return (groups & SS_PAIRS) ? uint32_t(k[17] >> (3u * (i >> 1))) & 7u : word; }
};
template <uint32_t AT>
RPT_DEV constexpr uint32_t LightK::word() const {   // k[AT + i], by constant indices only
    return uint32_t(i == 0u ? SceneStructK::k[AT] : i == 1u ? SceneStructK::k[AT + 1u] : i == 2u ? SceneStructK::k[AT + 2u] : SceneStructK::k[AT + 3u]);
}
#else
typedef SceneStructRt SceneStructK;
#endif
// The common-slab bits of the box pair that begins at record i: the block's where the scan takes the JIT's constants, else `word`.
template <class SHAPE>
RPT_DEV uint32_t scan_pair_shared(uint32_t i, uint32_t word) {
#if defined(RPT_SCAN_SHAPE) && defined(RPT_SCENE_STRUCT)
    if constexpr (tt::is_same_v<SHAPE, ScanShapeK>) return SceneStructK::pair_shared(i, word);
#endif
    return word;
}
template <bool MASKED = false, bool MONO = false, bool TAIL = false, bool SHADOW = false, class SHAPE = ScanShapeRt>
RPT_DEV void scan_prims(const SceneView& scene, V o, V d, float tmin, float& tbest, uint32_t& code, uint64_t mask = ~0ull,
                        bool* tail_skipped = nullptr, ShadowTwin twin = ShadowTwin{0u, 1u, 0u}, bool* best_is_twin = nullptr) {
    static_assert(!(TAIL && MASKED), "one cull at a time");
    static_assert(!(SHADOW && (MASKED || TAIL)), "the shadow form is a plain scan");
    // The scene view is a kernel argument (every caller passes its kernarg struct): its fields are read HERE, through the
    // constant address space, behind an opaque copy of the pointer.  Read as plain kernel arguments they are all hoisted to
    // the kernel's entry and held in scalar registers for its whole life -- the render kernels have ~110 such values, the
    // compiler parks the overflow in VGPR lanes, and 14 % of their VALU instructions were v_readlane / v_writelane.
    const auto& sc = *kernarg_scene();
    (void)scene;
    const SHAPE sh{&sc};
    bool flag = false;   // (SHADOW) the best so far is a twin record
    // ... and inside the twin kind's loop: tbest as the last accepted TWIN record left it (NaN: none yet).  At the loop's end the best
    // so far is a twin record iff tbest still has that value: every later accepted record lowered it (t < tbest is strict).  A float
    // select under (lane mask & uniform bit) -- a select between a uniform and a divergent bool is compiled to four vector instructions.
    float t_twin = __builtin_nanf("");
    // An accepted record (`ok` holds t < tbest): the new tbest, and its code or -- SHADOW -- whether it is a twin record (`is_twin`: a
    // tt::false_type outside the twin kind's loop, a wave-uniform bool inside).
    auto acc = [&](bool ok, float t, uint32_t c, auto is_twin) {
        if (ok) tbest = t;
        asm volatile("" : "+v"(tbest));   // one tbest: without the pin the loops carry a second copy of it (a third select per record)
        if constexpr (!SHADOW) { if (ok) code = c; }
        else if constexpr (tt::is_same_v<decltype(is_twin), tt::false_type>) flag = flag && !ok;
        else if (ok && is_twin) t_twin = t;
    };
    // twin_at(tw, i): acc's last argument for record i of a kind whose loop was entered as the twin kind's (tw: true_type) or not.
    auto twin_at = [&](auto tw, uint32_t i) {
        if constexpr (decltype(tw)::value) return twin.has(i);
        else return tt::false_type{};
    };
    // A kind's loop: SHADOW compiles it twice, for the twin's kind (its records ask twin.has(i)) and for every other kind.
    auto kind_loop = [&](uint32_t kind, auto&& loop) {
        if constexpr (SHADOW) {
            if (twin.kind == kind) {   // (wave-uniform)
                loop(tt::true_type{});
                flag = t_twin == tbest;
                return;
            }
        }
        loop(tt::false_type{});
    };
    uint32_t bit = 0;  // wave-uniform record number
    auto on = [&](uint32_t i) { return !MASKED || ((mask >> ((bit + i) & 63u)) & 1ull) != 0ull; };
    // Unmasked scans: records the commit found to be rotations about the vertical axis take to_local_y (wave-uniform branches).
    const uint64_t sph_yrot = MASKED ? 0ull : sh.sph_yrot(), cub_yrot = MASKED ? 0ull : sh.cub_yrot();
    kind_loop(K_SPHERE, [&](auto tw) {
        for (uint32_t i = 0; i < sh.n_sph(); i++) {
            if (!on(i)) continue;
            const XfScan x = uload(&sc.sph[i]);
            V ol, dl;
            if (!MASKED && ((sph_yrot >> (i & 63u)) & 1ull)) to_local_y(x, o, d, ol, dl);
            else to_local(x, o, d, ol, dl);
            float t;
            acc(sphere_closer(ol, dl, tmin, tbest, t), t, (K_SPHERE << 28) | i, twin_at(tw, i));
        }
    });
    bit += sh.n_sph();
    kind_loop(K_CUBE, [&](auto tw) {   // two records per iteration: independent instruction streams for the scheduler (unmasked scans)
        uint32_t i = 0;
        if (!MASKED)
            for (; i + 1u < sh.n_cub(); i += 2u) {
                const XfScan x0 = uload(&sc.cub[i]), x1 = uload(&sc.cub[i + 1u]);
                V ol0, dl0, ol1, dl1;
                float t0, t1;
                if (((cub_yrot >> (i & 63u)) & 3ull) == 3ull) {
                    to_local_y(x0, o, d, ol0, dl0);
                    to_local_y(x1, o, d, ol1, dl1);
                } else {
                    to_local(x0, o, d, ol0, dl0);
                    to_local(x1, o, d, ol1, dl1);
                }
                acc(cube_closer(ol0, dl0, tmin, tbest, t0), t0, (K_CUBE << 28) | i, twin_at(tw, i));
                acc(cube_closer(ol1, dl1, tmin, tbest, t1), t1, (K_CUBE << 28) | (i + 1u), twin_at(tw, i + 1u));
            }
        for (; i < sh.n_cub(); i++) {
            if (!on(i)) continue;
            const XfScan x = uload(&sc.cub[i]);
            V ol, dl;
            if (!MASKED && ((cub_yrot >> (i & 63u)) & 1ull)) to_local_y(x, o, d, ol, dl);
            else to_local(x, o, d, ol, dl);
            float t;
            acc(cube_closer(ol, dl, tmin, tbest, t), t, (K_CUBE << 28) | i, twin_at(tw, i));
        }
    });
    bit += sh.n_cub();
    for (uint32_t i = 0; i < sh.n_pln(); i++) {   // (a plane is never a twin: no light shape is one)
        const F4 nv = uload(&sc.pln[i]).nv;
        float t;
        acc(plane_closer(nv, o, d, tmin, tbest, t), t, (K_PLANE << 28) | i, tt::false_type{});
    }
    const uint32_t n_rect = sh.n_rect_x() + sh.n_rect_y() + sh.n_rect_z();
    if (sh.n_aabb() + n_rect + sh.has_shell() != 0) {  // wave-uniform: these kinds share one reciprocal direction per ray
        const V inv = mk(rcp(d.x), rcp(d.y), rcp(d.z));
        if (sh.has_shell())   // (SHADOW: a light whose twin is a shell face takes the closest-hit form)
            shell_closer(uload(sc.shell), o, inv, tmin, tbest, [&](bool ok, float t, auto code_of) {
                if constexpr (SHADOW) acc(ok, t, 0u, tt::false_type{});
                else { if (ok) { tbest = t; code = code_of(); } }
            });
        if constexpr (TAIL) {
            if (sh.scan_cull()) {   // (wave-uniform)
                const SceneView::ScanBox tb = kernarg_load(&sc.scan_tail);
                if (__ballot(interval_meets_box<false>(tb, o, inv, tmin, tbest)) == 0ull) {
                    if (tail_skipped) *tail_skipped = true;
                    return;   // (no monomial surfaces behind the tail: TAIL is not instantiated with MONO)
                }
            }
        }
        kind_loop(K_AABB, [&](auto tw) {
            uint32_t i = 0;
            if (!MASKED)
                for (; i + 1u < sh.n_aabb(); i += 2u) {
                    const AabbScan b0 = uload(&sc.aabb[i]), b1 = uload(&sc.aabb[i + 1u]);
                    aabb_pair_closer(b0, b1, scan_pair_shared<SHAPE>(i, __float_as_uint(b0.hi.w)), o, inv, tmin, tbest, i,   // hi.w: the slabs they have in common
                                     [&](bool ok, float t, uint32_t k) { acc(ok, t, (K_AABB << 28) | k, twin_at(tw, k)); });
                }
            for (; i < sh.n_aabb(); i++) {
                if (!on(i)) continue;
                const AabbScan b = uload(&sc.aabb[i]);
                float t;
                acc(aabb_closer(b.lo, b.hi, o, inv, tmin, tbest, t), t, (K_AABB << 28) | i, twin_at(tw, i));
            }
        });
        bit += sh.n_aabb();
        kind_loop(K_RECT, [&](auto tw) {
            uint32_t i = 0;
            for (uint32_t e = sh.n_rect_x(); i < e; i++) {
                if (!on(i)) continue;
                const RectScan r = uload(&sc.rect[i]);
                float t;
                acc(rect_closer(r.a, r.b.x, o.x, inv.x, o.y, d.y, o.z, d.z, tmin, tbest, t), t, (K_RECT << 28) | i, twin_at(tw, i));
            }
            for (uint32_t e = sh.n_rect_x() + sh.n_rect_y(); i < e; i++) {
                if (!on(i)) continue;
                const RectScan r = uload(&sc.rect[i]);
                float t;
                acc(rect_closer(r.a, r.b.x, o.y, inv.y, o.z, d.z, o.x, d.x, tmin, tbest, t), t, (K_RECT << 28) | i, twin_at(tw, i));
            }
            for (uint32_t e = n_rect; i < e; i++) {
                if (!on(i)) continue;
                const RectScan r = uload(&sc.rect[i]);
                float t;
                acc(rect_closer(r.a, r.b.x, o.z, inv.z, o.x, d.x, o.y, d.y, tmin, tbest, t), t, (K_RECT << 28) | i, twin_at(tw, i));
            }
        });
        bit += n_rect;
    } else {
        bit += sh.n_aabb() + n_rect;
    }
    kind_loop(K_TRI, [&](auto tw) {
        for (uint32_t i = 0; i < sh.n_tri(); i++) {
            if (!on(i)) continue;
            const TriScan tr = uload(&sc.tri[i]);
            float t;
            acc(tri_closer(tr.pn, tr.A, tr.B, o, d, tmin, tbest, t), t, (K_TRI << 28) | i, twin_at(tw, i));
        }
    });
    if constexpr (MONO) {
        static_assert(!MASKED && !TAIL, "scan_mask_for_ball and the tail cull do not cover the monomial surfaces");
        for (uint32_t i = 0; i < sc.n_mono; i++) {   // (SHADOW: a light with a monomial-surface twin takes the closest-hit form)
            const MonoScan m = uload(&sc.mono[i]);
            V ol, dl;
            to_local(XfScan{m.r0, m.r1, m.r2}, o, d, ol, dl);
            float t;
            acc(mono_closer(ol, dl, m.h, tmin, tbest, t), t, (K_MONO << 28) | i, tt::false_type{});
        }
    }
    if constexpr (SHADOW) *best_is_twin = flag;
}
// Which scanned records can a query touch that stays inside the ball (c, r) of each live lane?  Wave-uniform mask
// for scan_prims<true> (the union over the lanes: one lane's ball reaching a box keeps that record for all of them).
// Scenes with more than 64 bounded scan records do not occur (from 64 on, the scene-level tree takes over).  The monomial surfaces'
// boxes follow the triangles' in pbox but are not counted here: scan_prims<true, true> does not exist (static_assert there).
// `touched` (optional): does any record's box reach THIS lane's ball?
RPT_DEV uint64_t scan_mask_for_ball(const SceneView& scene_, bool live, V c, float r, bool* touched = nullptr) {
    const auto& sc = *kernarg_scene();   // (see kernarg_scene)
    const uint32_t n = sc.n_sph + sc.n_cub + sc.n_aabb + sc.n_rect_x + sc.n_rect_y + sc.n_rect_z + sc.n_tri;
    if (touched) *touched = n != 0u;
    if (n > 64u) return ~0ull;
    bool mine = false;
    const float r2 = r * r;
    uint64_t mask = 0ull;
    auto reaches = [&](const AabbScan& b) {
        const float dx = fmaxf(fmaxf(b.lo.x - c.x, c.x - b.hi.x), 0.f);
        const float dy = fmaxf(fmaxf(b.lo.y - c.y, c.y - b.hi.y), 0.f);
        const float dz = fmaxf(fmaxf(b.lo.z - c.z, c.z - b.hi.z), 0.f);
        const bool t = live && fmaf(dx, dx, fmaf(dy, dy, dz * dz)) <= r2;
        mine = mine || t;
        return __any(t);
    };
    uint32_t i = 0;
    for (; i + 4u <= n; i += 4u) {   // four records' scalar loads in flight at a time
        const AabbScan b0 = uload(&sc.pbox[i]), b1 = uload(&sc.pbox[i + 1u]), b2 = uload(&sc.pbox[i + 2u]), b3 = uload(&sc.pbox[i + 3u]);
        if (reaches(b0)) mask |= 1ull << i;
        if (reaches(b1)) mask |= 2ull << i;
        if (reaches(b2)) mask |= 4ull << i;
        if (reaches(b3)) mask |= 8ull << i;
    }
    for (; i < n; i++)
        if (reaches(uload(&sc.pbox[i]))) mask |= 1ull << i;
    if (touched) *touched = mine;
    return mask;
}
// The primary query of a scan flavour in a medium: the scan with its tail cull.  The counters build also classifies the trip (`cnt`,
// rpt_scan_cull_counters): cnt[0..4] trips by the number of lanes whose interval reaches the box around all scanned records (0, 1-2,
// 3-4, 5-8, more), cnt[5..8] trips with such a lane in which none of them reaches the box of record group g (SceneView::scan_groups:
// the candidates of a finer cull, measured and not built: DESIGN.md section 4, round 6), cnt[9] trips that left out the tail.
template <bool COUNT, class SHAPE = ScanShapeRt>
RPT_DEV void scan_primary(const SceneView& scene, V o, V d, float tmin, float& tbest, uint32_t& code, unsigned long long* cnt) {
    if constexpr (COUNT) {
        const auto& sc = *kernarg_scene();
        const SceneView::ScanBox bound = kernarg_load(&sc.scan_bound);
        const bool first = cnt && uint32_t(__builtin_ctzll(__ballot(true))) == (threadIdx.x & 63u);
        if (!(bound.lo[0] > bound.hi[0])) {
            const V inv = mk(rcp(d.x), rcp(d.y), rcp(d.z));
            const bool need = interval_meets_box<true>(bound, o, inv, tmin, tbest);
            const uint32_t n_need = uint32_t(__popcll(__ballot(need)));
            if (first) atomicAdd(&cnt[n_need == 0u ? 0 : n_need <= 2u ? 1 : n_need <= 4u ? 2 : n_need <= 8u ? 3 : 4], 1ull);
            if (n_need != 0u)
                for (uint32_t g = 0; g < sc.n_scan_groups; g++) {
                    const SceneView::ScanGroup grp = kernarg_load(&sc.scan_groups[g]);
                    const bool reach = need && interval_meets_box<false>(grp.box, o, inv, tmin, tbest);
                    if (__ballot(reach) == 0ull && first) atomicAdd(&cnt[5u + g], 1ull);
                }
        }
        bool skipped = false;
        scan_prims<false, false, true, false, SHAPE>(scene, o, d, tmin, tbest, code, ~0ull, &skipped);
        if (skipped && first) atomicAdd(&cnt[9], 1ull);
    } else {
        scan_prims<false, false, true, false, SHAPE>(scene, o, d, tmin, tbest, code);
    }
}

// Would a walk of the per-mesh trees visit anything?  The two child boxes of every mesh root against the
// interval the scan left (scalar loads: the roots are wave-uniform).
RPT_DEV bool mesh_roots_hit(const SceneView& scene_, V o, V d, float tmin, float tbest) {
    const auto& sc = *kernarg_scene();   // (see kernarg_scene)
    const V inv = mk(rcp(d.x), rcp(d.y), rcp(d.z));
    bool need = false;
    for (uint32_t i = 0; i < sc.n_mesh; i++) {
        const MeshRef m = uload(&sc.meshes[i]);
        const BvhNode nd = uload(&sc.nodes[m.root]);
        float n0, f0, n1, f1;
        slab2(nd.lo0, nd.hi0, o, inv, n0, f0);
        slab2(nd.lo1, nd.hi1, o, inv, n1, f1);
        need = need || fmaxf(n0, tmin) <= fminf(f0, tbest) || fmaxf(n1, tmin) <= fminf(f1, tbest);
    }
    return need;
}
template <bool COUNT, bool ANY>
RPT_DEV void walk_meshes(const SceneView& scene_, V o, V d, float tmin, float& tbest, uint32_t& code, uint32_t& inst,
                         uint32_t* stk, uint32_t stride, uint32_t& c_nodes, uint32_t& c_tris, AnyHit any, uint32_t cap = 32u) {
    const auto& sc = *kernarg_scene();   // (see kernarg_scene)
    for (uint32_t i = 0; i < sc.n_mesh; i++) {
        const MeshRef m = uload(&sc.meshes[i]);
        if (ANY && code != CODE_MISS && any.blocks(tbest, code)) break;  // (per lane) already occluded
        bvh_traverse<COUNT, false, ANY>(scene_, m.root, o, d, tmin, tbest, code, inst, stk, stride, cap, c_nodes, c_tris, any);
    }
}
// The same walk as a resumable one (deferred walks of the render kernel): the lane's position -- current entry,
// stack height, mesh -- lives in `w` and its stack column in LDS, and the wave leaves the loop as soon as fewer
// than `min_active` lanes are still walking; the stragglers continue with the next batch of parked walks instead
// of holding 60 idle lanes.  w.cur == kWalkDone: nothing left to do.
static const uint32_t kWalkDone = 0xFFFFFFFFu;  // has the leaf bit set; a 32-item prim leaf at the last index never occurs
struct WalkState {
    uint32_t cur, sp, mesh;
};
RPT_DEV WalkState walk_begin(const SceneView&) { return WalkState{uload(&kernarg_scene()->meshes[0]).root, 0u, 0u}; }
// `cap`: rows of the stack column (a mesh tree is at most bvh_max_depth = 20 levels deep: it pushes at most 19 entries).
template <bool COUNT>
// `leaf_quarters`: the lanes reach their next leaf after very different numbers of steps (a few on average, a dozen for the
// slowest of 25), and a descent that waits for the last of them runs most of its steps for a handful of lanes.  So the
// descent pauses as soon as 4 x (lanes waiting at a leaf) >= leaf_quarters x (lanes still descending): the waiting lanes
// test their triangles, the others go on from where they are.  Every lane still performs its own steps in its own order.
RPT_DEV void walk_meshes_resumable(const SceneView& scene_, V o, V d, float tmin, float& tbest, uint32_t& code, uint32_t* stk,
                                   uint32_t stride, WalkState& w, uint32_t min_active, AnyHit any, uint32_t& c_nodes,
                                   uint32_t& c_tris, uint32_t cap = 32u, uint32_t leaf_quarters = 0u, uint32_t* c_wave = nullptr) {
    const auto& sc = *kernarg_scene();   // (see kernarg_scene)
    const BvhNode* nodes = sc.nodes;
    const V inv = mk(rcp(d.x), rcp(d.y), rcp(d.z));
    uint32_t cur = w.cur, sp = w.sp, mesh = w.mesh;
    while (uint32_t(__popcll(__ballot(cur != kWalkDone))) >= min_active) {
        for (;;) {  // the descent (kWalkDone has the leaf bit set: finished lanes take no part)
            const bool inner = !(cur & BVH_LEAF);
            const uint32_t n_inner = uint32_t(__popcll(__ballot(inner)));
            if (n_inner == 0u) break;
            if (leaf_quarters != 0u && 4u * uint32_t(__popcll(__ballot(!inner && cur != kWalkDone))) >= leaf_quarters * n_inner) break;
            if (COUNT && c_wave) c_wave[0]++;   // (wave-level: descent steps)
            if (!inner) continue;
            const BvhNode nd = nodes[cur];
            if (COUNT) c_nodes++;
            float n0, f0, n1, f1;
            slab2(nd.lo0, nd.hi0, o, inv, n0, f0);
            slab2(nd.lo1, nd.hi1, o, inv, n1, f1);
            const bool h0 = fmaxf(n0, tmin) <= fminf(f0, tbest);
            const bool h1 = fmaxf(n1, tmin) <= fminf(f1, tbest);
            if (h0 && h1) {
                const bool first0 = n0 <= n1;
                if (sp < cap) { stk[sp * stride] = first0 ? nd.e1 : nd.e0; sp++; }
                else if (COUNT && sc.stack_overflows) atomicAdd(sc.stack_overflows, 1ull);   // (never, by the commit-time depth check)
                cur = first0 ? nd.e0 : nd.e1;
            } else if (h0 || h1) {
                cur = h0 ? nd.e0 : nd.e1;
            } else if (sp) {
                sp--;
                cur = stk[sp * stride];
            } else {
                cur = kWalkDone;
            }
        }
        if (COUNT && c_wave) {   // (wave-level: triangle steps of this round = the largest leaf among the lanes at one)
            uint32_t mx = 0;
            for (uint32_t k = 1; k <= 4u; k++)
                if (__ballot((cur & BVH_LEAF) && cur != kWalkDone && ((cur >> 26) & 31u) + 1u >= k) != 0ull) mx = k;
            c_wave[1] += mx;
        }
        if ((cur & BVH_LEAF) && cur != kWalkDone) {   // (lanes that are still descending go on with the next round)
            const uint32_t first = cur & BVH_INDEX_MASK;
            const uint32_t count = ((cur >> 26) & 31u) + 1u;
            TriScan nxt = sc.btri[first];
            for (uint32_t i = 0; i < count; i++) {  // the next triangle is in flight while this one is tested
                const TriScan tr = nxt;
                if (i + 1u < count) nxt = sc.btri[first + i + 1u];
                if (COUNT) c_tris++;
                float t = hit_tri(tr.pn, tr.A, tr.B, o, d, tmin, tbest);
                if (t >= 0.f) { tbest = t; code = (K_BVHTRI << 28) | (first + i); }
            }
            if (code != CODE_MISS && any.blocks(tbest, code)) { sp = 0; mesh = sc.n_mesh; }  // an occluder is known
            if (sp) {
                sp--;
                cur = stk[sp * stride];
            } else {
                cur = kWalkDone;
            }
        }
        if (cur == kWalkDone && mesh + 1u < sc.n_mesh) {  // the next mesh's tree
            mesh++;
            cur = sc.meshes[mesh].root;
        }
    }
    w.cur = cur;
    w.sp = sp;
    w.mesh = mesh;
}

// BVH: 0 = no tree in the scene, 1 = per-mesh trees only, 2 = scene-level tree possible.
template <int BVH, bool COUNT, bool ANY = false, bool MONO = false, class SHAPE = ScanShapeRt>
RPT_DEV void closest_hit(const SceneView& scene_, V o, V d, float tmin, float& tbest, uint32_t& code, uint32_t& inst,
                         uint32_t* stk, uint32_t stride, uint32_t& c_nodes, uint32_t& c_tris,
                         AnyHit any = AnyHit{-kInf, 1u, 0u}) {
    const auto& sc = *kernarg_scene();   // (see kernarg_scene)
    if (BVH == 2 && sc.scene_bvh) {  // wave-uniform: planes (unbounded) are scanned, everything else is in the tree
        for (uint32_t i = 0; i < sc.n_pln; i++) {
            const F4 nv = uload(&sc.pln[i]).nv;
            float t = hit_plane(nv, o, d, tmin);
            if (t >= 0.f && t < tbest) { tbest = t; code = (K_PLANE << 28) | i; }
        }
        bvh_traverse<COUNT, true, ANY, MONO>(scene_, sc.top_root, o, d, tmin, tbest, code, inst, stk, stride, 32u, c_nodes, c_tris, any);
        if (sc.mesh_deferred) walk_meshes<COUNT, ANY>(scene_, o, d, tmin, tbest, code, inst, stk, stride, c_nodes, c_tris, any);   // (wave-uniform)
        return;
    }
    scan_prims<false, MONO, false, false, SHAPE>(scene_, o, d, tmin, tbest, code);
    if (BVH) walk_meshes<COUNT, ANY>(scene_, o, d, tmin, tbest, code, inst, stk, stride, c_nodes, c_tris, any);
}

// Everything of a query except the per-mesh trees: the linear scan, or -- BVH = 3: a scene tree whose meshes are walked
// separately (SceneView::mesh_deferred) -- the planes and the scene tree.
template <int BVH, bool COUNT, bool MONO = false>
RPT_DEV void scan_or_tree(const SceneView& scene_, V o, V d, float tmin, float& tbest, uint32_t& code, uint32_t& inst, uint32_t* stk,
                          uint32_t stride, uint32_t& c_nodes, uint32_t& c_tris) {
    if constexpr (BVH == 3) {
        const auto& sc = *kernarg_scene();
        for (uint32_t i = 0; i < sc.n_pln; i++) {
            const F4 nv = uload(&sc.pln[i]).nv;
            float t = hit_plane(nv, o, d, tmin);
            if (t >= 0.f && t < tbest) { tbest = t; code = (K_PLANE << 28) | i; }
        }
        bvh_traverse<COUNT, true, false, MONO>(scene_, sc.top_root, o, d, tmin, tbest, code, inst, stk, stride, 32u, c_nodes, c_tris);
    } else {
        scan_prims<false, MONO>(scene_, o, d, tmin, tbest, code);
    }
}

// Outward normal of the face of the axis-aligned box [lo, hi] that the surface point p lies on: the axis whose nearer face
// plane is closest to p.
// The face of a box [lo, hi] that bounds the accepted root t of its slab test (src/shape/cube.rs:37-55).  Away from the edges that is
// the face nearest to the hit point, six subtractions.  Within rounding of an edge the nearest face can be the hidden one, a normal
// that faces away from the ray: where the two nearest faces are closer than 1e-5 (1 + |p|) to each other the slab test is run again
// and decides as the reference does -- the slab entered last when the entry lies at or beyond tmin, else the slab left first; among
// equal times x before y before z.  (A lane in 10^4 takes that branch.)
RPT_DEV V slab_face_normal(V o, V d, V lo, V hi, float tmin);
RPT_DEV V box_face_normal(V o, V d, V lo, V hi, float t, float tmin) {
    const V p = fma3(t, d, o);
    const float pxl = fabsf(p.x - lo.x), pxh = fabsf(p.x - hi.x), pyl = fabsf(p.y - lo.y), pyh = fabsf(p.y - hi.y);
    const float pzl = fabsf(p.z - lo.z), pzh = fabsf(p.z - hi.z);
    const float ex = fminf(pxl, pxh), ey = fminf(pyl, pyh), ez = fminf(pzl, pzh);
    if (__builtin_amdgcn_fmed3f(ex, ey, ez) > 1e-5f * (1.f + max3(fabsf(p.x), fabsf(p.y), fabsf(p.z)))) {
        const bool ax0 = ex <= ey && ex <= ez, ax1 = !ax0 && ey <= ez;
        return mk(ax0 ? (pxh < pxl ? 1.f : -1.f) : 0.f, ax1 ? (pyh < pyl ? 1.f : -1.f) : 0.f, (!ax0 && !ax1) ? (pzh < pzl ? 1.f : -1.f) : 0.f);
    }
    return slab_face_normal(o, d, lo, hi, tmin);
}
RPT_DEV V slab_face_normal(V o, V d, V lo, V hi, float tmin) {
#pragma clang fp contract(off)
    const float ix = rcp(d.x), iy = rcp(d.y), iz = rcp(d.z);
    const float x1 = (lo.x - o.x) * ix, x2 = (hi.x - o.x) * ix, y1 = (lo.y - o.y) * iy, y2 = (hi.y - o.y) * iy;
    const float z1 = (lo.z - o.z) * iz, z2 = (hi.z - o.z) * iz;
    const bool sx = x1 > x2, sy = y1 > y2, sz = z1 > z2;
    const float xl = fminf(x1, x2), xh = fmaxf(x1, x2), yl = fminf(y1, y2), yh = fmaxf(y1, y2), zl = fminf(z1, z2), zh = fmaxf(z1, z2);
    const bool in = !(max3(xl, yl, zl) < tmin);   // slabs_closer's choice of the root
    const bool ax0 = in ? (xl > yl && xl > zl) : (xh < yh && xh < zh);
    const bool ax1 = !ax0 && (in ? yl > zl : yh < zh);
    const bool swapped = ax0 ? sx : (ax1 ? sy : sz);
    const float sg = (in == swapped) ? 1.f : -1.f;   // in through the lo face, out through the hi face, unless the direction is negative there
    return mk(ax0 ? sg : 0.f, ax1 ? sg : 0.f, (!ax0 && !ax1) ? sg : 0.f);
}
// Normal and object of the winning primitive (per lane).
template <bool MONO = false>
RPT_DEV void finalize_hit(const SceneView& scene_, V o, V d, float tmin, float t, uint32_t code, uint32_t inst, V& n,
                          uint32_t& obj) {
    const auto& sc = *kernarg_scene();   // (see kernarg_scene)
    uint32_t kind = code >> 28, idx = code & 0x0FFFFFFFu;
    if (MONO && kind == K_MONO) {   // src/shape/monomial_surface.rs:88-104 (flipped against the local ray), then src/shape.rs:131-134
        const MonoScan m = sc.mono[idx];
        const XfShade s = sc.mono_sh[idx];
        V ol, dl;
        to_local(XfScan{m.r0, m.r1, m.r2}, o, d, ol, dl);
        const V p = fma3(t, dl, ol);
        const float k = m.h.x * 4.f * fmaf(p.x, p.x, p.z * p.z);
        V nl = normalize(mk(k * p.x, -1.f, k * p.z));
        if (dot(nl, dl) > 0.f) nl = -nl;
        n = (s.r1.w != 0.f) ? normalize(mk(dot3(s.r0, nl), dot3(s.r1, nl), dot3(s.r2, nl))) : nl;
        obj = __float_as_uint(s.r0.w);
        return;
    }
    if (kind == K_INSTTRI) {  // src/shape/mesh.rs:78 in the instance's space, then src/shape.rs:131-134
        const InstRec r = sc.inst[inst];
        const TriShade s = sc.btri_sh[idx];
        V nl;
        if (s.n2.w != 0.f) {
            nl = xyz(s.n1);
        } else {
            const TriScan tr = sc.btri[idx];
            const V ol = mk(dot3w(r.r0, o), dot3w(r.r1, o), dot3w(r.r2, o));
            const V dl = mk(dot3(r.r0, d), dot3(r.r1, d), dot3(r.r2, d));
            V p = fma3(t, dl, ol);
            float v = dot3w(tr.A, p), w = dot3w(tr.B, p);
            float u = 1.f - v - w;
            nl = normalize(u * xyz(s.n1) + v * xyz(s.n2) + w * xyz(s.n3));
        }
        n = normalize(mk(dot3(r.n0, nl), dot3(r.n1, nl), dot3(r.n2, nl)));
        obj = __float_as_uint(r.n0.w);
        return;
    }
    if (kind == K_SPHERE) {  // src/shape/sphere.rs:40-41 then src/shape.rs:131-134
        const XfScan x = sc.sph[idx];
        const XfShade s = sc.sph_sh[idx];
        V ol, dl;
        to_local(x, o, d, ol, dl);
        V nl = normalize(fma3(t, dl, ol));
        n = (s.r1.w != 0.f) ? normalize(mk(dot3(s.r0, nl), dot3(s.r1, nl), dot3(s.r2, nl))) : nl;
        obj = __float_as_uint(s.r0.w);
    } else if (kind == K_CUBE) {
        const XfScan x = sc.cub[idx];
        const XfShade s = sc.cub_sh[idx];
        V ol, dl;
        to_local(x, o, d, ol, dl);
        const V nl = box_face_normal(ol, dl, mk(-0.5f, -0.5f, -0.5f), mk(0.5f, 0.5f, 0.5f), t, tmin);
        n = (s.r1.w != 0.f) ? normalize(mk(dot3(s.r0, nl), dot3(s.r1, nl), dot3(s.r2, nl))) : nl;
        obj = __float_as_uint(s.r0.w);
    } else if (kind == K_AABB) {
        const AabbScan b = sc.aabb[idx];
        n = box_face_normal(o, d, xyz(b.lo), xyz(b.hi), t, tmin);   // (as for the cube)
        obj = __float_as_uint(b.lo.w);
    } else if (kind == K_RECT) {
        const F4 s = sc.rect_sh[idx].n_obj;
        n = xyz(s);
        obj = __float_as_uint(s.w);
    } else if (kind == K_PLANE) {  // src/shape/plane.rs:27: -normalize(n) * signum(cos)
        const F4 nv = sc.pln[idx].nv;
        const F4 s = sc.pln_sh[idx].unit_n_obj;
        float c = dot3(nv, d);
        float sg = __builtin_signbit(c) ? 1.f : -1.f;
        n = sg * xyz(s);
        obj = __float_as_uint(s.w);
    } else {  // triangle: src/shape/mesh.rs:78, normals never face-forwarded
        const TriScan* ta = (kind == K_TRI) ? sc.tri : sc.btri;
        const TriShade* sa = (kind == K_TRI) ? sc.tri_sh : sc.btri_sh;
        const TriShade s = sa[idx];
        obj = __float_as_uint(s.n1.w);
        if (s.n2.w != 0.f) {  // flat: n1 == n2 == n3
            n = xyz(s.n1);
        } else {
            const TriScan tr = ta[idx];
            V p = fma3(t, d, o);
            float v = dot3w(tr.A, p), w = dot3w(tr.B, p);
            float u = 1.f - v - w;
            n = normalize(u * xyz(s.n1) + v * xyz(s.n2) + w * xyz(s.n3));
        }
    }
}

// ------------------------------------------------------------------ materials
struct Mat {
    V albedo;
    float emit;
    uint32_t kind;
    float shin, ior;
};
// Small per-scene tables that every lane indexes on its own -- the material of the object it hit, the triangle of the
// light it samples -- staged in LDS by the render kernel (a ds_read instead of a dependent global load in the middle of a
// stage).  A table that does not fit stays in global memory (count 0 here); kernels that stage nothing pass LdsTables{}.
struct LdsTables {
    const F4* mats = nullptr;    // [n_mats] Material records
    uint32_t n_mats = 0;
    const F4* ltris = nullptr;   // [n_ltris] LightTri records
    uint32_t n_ltris = 0;
};
// (kLdsMats = 32, kLdsLtris = 8: gpu_layout.h; 32 x 32 B + 8 x 96 B = 1.75 KB per block)
template <class ST = SceneStructRt>   // (ST: what is known about the scene beforehand, here and below -- SceneStructRt / SceneStructK)
RPT_DEV Mat load_mat(const SceneView& scene_, uint32_t obj, const LdsTables& tab = LdsTables{}) {
    const auto& sc = *kernarg_scene();   // (see kernarg_scene)
    Material m;
    if (ST::mat_staged(obj, tab.n_mats)) {   // wave-uniform in effect: either every object's material is staged or none
        m.albedo_emit = tab.mats[2u * obj];
        m.params = tab.mats[2u * obj + 1u];
    } else {
        m = sc.mats[obj];
    }
    return Mat{xyz(m.albedo_emit), m.albedo_emit.w, __float_as_uint(m.params.x), m.params.y, m.params.z};
}
template <class ST = SceneStructRt>
RPT_DEV V mat_color(const Mat& m) { return ST::mat_has_colour(m.kind) ? m.albedo : mk(0.f, 0.f, 0.f); }   // src/material.rs:107
template <class ST = SceneStructRt>
RPT_DEV float mat_emit(const Mat& m) { return ST::mat_has_colour(m.kind) ? m.emit : 0.f; }                // src/material.rs:100

// Rotation taking +Y onto `b` applied to v (nalgebra rotation_between(+Y, b)): axis k =
// normalize(Y x b), angle acos(b.y).  `pi_fallback_x`: Lambertian's (0,1,1e-8) retry
// (src/material.rs:186-194) is a half-turn about +X; Phong's quat_rotation falls back to identity.
// nalgebra rotates only when |Y x b| > f64::EPSILON = 2^-52 and falls back below that (sin(pi) = 1.2e-16 is below: a face
// turned with rotate_z(pi)); the square of the threshold, 2^-104, is a normal fp32 number, so no denormal reaches rsq either.
RPT_DEV V rotate_from_y(V b, V v, bool pi_fallback_x) {
    float s2 = fmaf(b.x, b.x, b.z * b.z);
    if (s2 > 0x1p-104f) {
        float is = rsq(s2);
        float s = s2 * is;           // sin(angle)
        float kx = b.z * is, kz = -b.x * is;  // k = (b.z, 0, -b.x)/s
        float kv = kx * v.x + kz * v.z;       // k . v
        // k x v = (-kz*v.y, kz*v.x - kx*v.z, kx*v.y)
        V kxv = mk(-kz * v.y, kz * v.x - kx * v.z, kx * v.y);
        float c = b.y;
        float omc = 1.f - c;
        return mk(fmaf(c, v.x, fmaf(s, kxv.x, omc * kv * kx)), fmaf(c, v.y, s * kxv.y),
                  fmaf(c, v.z, fmaf(s, kxv.z, omc * kv * kz)));
    }
    if (b.y < 0.f && pi_fallback_x) return mk(v.x, -v.y, -v.z);
    return v;
}
RPT_DEV V reflect_neg(V w, V n) { return fma3(2.f * dot(n, w), n, -w); }  // -glm::reflect_vec(w, n)

// Material::sample_f, src/material.rs:166-263.  Returns false for None (total internal reflection).
template <class ST = SceneStructRt>
RPT_DEV bool sample_f(const Mat& m, V n, V wo, Rng& rng, V& wi, float& pdf) {
    if (ST::is_mat(m.kind, M_LAMBERTIAN)) {
        float r1 = rng.uniform(), r2 = rng.uniform();
        float ct = sqrt1(r2);             // cos(acos(sqrt(r2)))
        float st = sqrt1(1.f - r2);
        pdf = ct * kInvPi;
        V dir = mk(st * __builtin_amdgcn_cosf(r1), ct, st * __builtin_amdgcn_sinf(r1));  // phi = 2 pi r1
        wi = normalize(rotate_from_y(n, dir, true));
        return true;
    } else if (ST::is_mat(m.kind, M_PHONG)) {
        float r1 = rng.uniform(), r2 = rng.uniform();
        float ct = __powf(r2, rcp(m.shin + 1.f));
        float st = sqrt1(fmaxf(1.f - ct * ct, 0.f));
        pdf = (m.shin + 1.f) * (0.5f * kInvPi) * __powf(ct, m.shin);
        V dir = mk(st * __builtin_amdgcn_cosf(r1), ct, st * __builtin_amdgcn_sinf(r1));
        V refl = reflect_neg(wo, n);
        wi = normalize(rotate_from_y(normalize(refl), dir, false));
        return true;
    } else if (ST::is_mat(m.kind, M_MIRROR)) {
        wi = reflect_neg(wo, normalize(n));
        pdf = 1.f;
        return true;
    } else {
        bool inside = dot(n, wo) < 0.f;
        V nn = inside ? -n : n;
        float ci = fminf(fmaxf(dot(wo, nn), 0.f), 1.f);
        float ni = inside ? m.ior : 1.f, nt = inside ? 1.f : m.ior;
        float r0 = (ni - nt) * rcp(ni + nt);
        r0 *= r0;
        float mm = 1.f - ci;
        float m2 = mm * mm;
        float sr = fminf(fmaxf(fmaf(1.f - r0, m2 * m2 * mm, r0), 0.f), 1.f);
        pdf = 1.f;
        if (rng.uniform() < sr) {
            wi = reflect_neg(wo, n);
            return true;
        }
        float eta = ni * rcp(nt);
        float k = 1.f - eta * eta * (1.f - ci * ci);
        if (k < 0.f) return false;  // sqrt -> NaN -> None
        float cost = sqrt1(k);
        wi = fma3(eta * ci - cost, nn, -eta * wo);
        return true;
    }
}
// Material::bsdf, src/material.rs:266-289.
template <class ST = SceneStructRt>
RPT_DEV V bsdf(const Mat& m, V n, V wo, V wi) {
    float nwi = dot(n, wi), nwo = dot(n, wo);
    if (__builtin_signbit(nwi) || __builtin_signbit(nwo)) return mk(0.f, 0.f, 0.f);
    if (ST::is_mat(m.kind, M_LAMBERTIAN)) return kInvPi * m.albedo;
    if (ST::is_mat(m.kind, M_PHONG)) {
        V r = -normalize(fma3(-2.f * dot(n, wi), n, wi));
        float c = fminf(fmaxf(dot(r, wo), 0.f), 1.f);
        // The shininess behind an opaque copy: its two terms below are invariant in the render kernels' light loop, and hoisted out
        // of it each of them holds a register across the shadow scan (the kernels sit at their 80-register limit: two more spills).
        float shin = m.shin;
        asm volatile("" : "+v"(shin));
        // powf(0, s) = 0 for s > 0, 1 for s == 0
        float pw = (c > 0.f) ? __powf(c, shin) : (shin == 0.f ? 1.f : 0.f);
        return ((shin + 2.f) * (0.5f * kInvPi) * pw) * m.albedo;
    }
    return mk(1.f, 1.f, 1.f);
}

// ------------------------------------------------------------------ lights
// Light::illuminate for Light::Object, src/light.rs:34-45, over the shape samplers
// (src/kdtree.rs:141-146 + src/shape/mesh.rs:85-99, sphere.rs:53-65, cube.rs:76-89,
//  Transformed::sample src/shape.rs:140-151).
// Shape::sample of the light's shape: point v, normal n, pdf p (per world area).
// The transform of the sampled leaf.  A plain Light::Object is wave-uniform: the whole record sits in SGPRs.
// A leaf picked out of a group differs per lane: its rows are loaded where they are used, so that the 48
// floats never live in VGPRs at once.
template <bool UNIFORM> struct LightXfRows;
// (UNIFORM: rows and the has-transform word are scalar loads AT THEIR USE, inside the wave-uniform branches that need them.  Loaded by
// value up front the record is three s_load_dwordx16 and 48 live scalar registers -- for a world-space mesh light, which reads the
// one word nrm[1].w -- and the kernels park the overflow in VGPR lanes.)
template <> struct LightXfRows<true> {
    const LightXf* p;
    RPT_DEV explicit LightXfRows(const LightXf* q) : p(q) {}
    RPT_DEV F4 fwd(int r) const { return uload(&p->fwd[r]); }
    RPT_DEV F4 inv(int r) const { return uload(&p->inv[r]); }
    RPT_DEV F4 nrm(int r) const { return uload(&p->nrm[r]); }
    RPT_DEV F4 lin(int r) const { return uload(&p->lin[r]); }
    RPT_DEV bool has_transform() const {
        typedef const __attribute__((address_space(4))) float* CF;
        return *(CF)(uintptr_t)&p->nrm[1].w != 0.f;
    }
};
template <> struct LightXfRows<false> {
    const LightXf* p;
    RPT_DEV explicit LightXfRows(const LightXf* q) : p(q) {}
    RPT_DEV F4 fwd(int r) const { return p->fwd[r]; }
    RPT_DEV F4 inv(int r) const { return p->inv[r]; }
    RPT_DEV F4 nrm(int r) const { return p->nrm[r]; }
    RPT_DEV F4 lin(int r) const { return p->lin[r]; }
    RPT_DEV bool has_transform() const { return p->nrm[1].w != 0.f; }
};
// One leaf shape of a Light::Object (Sphere/Cube/Mesh::sample under Transformed::sample, src/shape.rs:140-151).
template <bool UNIFORM, class ST = SceneStructRt, class LD = LightRt>   // (LD: what is known about this light beforehand -- LightRt / LightK)
RPT_DEV void sample_light_leaf(const SceneView& scene_, uint32_t shape, uint32_t first, uint32_t count, const LightXf* xp,
                               V pos, Rng& rng, V& v, V& n, float& p, const LdsTables& tab = LdsTables{}, LD ld = LD{}) {
    const auto& sc = *kernarg_scene();   // (see kernarg_scene)
    V vl, nl;
    const LightXfRows<UNIFORM> x(xp);
    const bool xf = ld.has_xf(x);
    const bool mesh = shape == LS_MESH;
    if (mesh) {
        uint32_t idx = rng.index(count);
        LightTri tr;
        if (ST::ltri_staged(first + idx, tab.n_ltris)) {
            const F4* q = tab.ltris + 6u * (first + idx);
            tr.v1 = q[0]; tr.v2 = q[1]; tr.v3 = q[2]; tr.n1 = q[3]; tr.n2 = q[4]; tr.n3 = q[5];
        } else {
            tr = sc.ltris[first + idx];
        }
        // `while u + v > 1 { redraw }` (src/shape/mesh.rs:89-93) on the draws' integers: with u = (2k+1) 2^-24 the sum is exact
        // in fp32 and u + v > 1 <=> ku + kv >= 2^23, so the rejected pairs are never converted (the wave runs the loop for its
        // unluckiest lane: ~7 rounds for 2 on average).  On the words themselves: (a & ~511) + (b & ~511) = 512 (ku + kv) carries
        // out of 32 bits exactly when ku + kv >= 2^23 -- and, and, add with carry, instead of shift, shift, add, compare.
        uint32_t ku, kv;
        triangle_pair(rng, ku, kv);
        const float u = float((ku << 1) | 1u) * 0x1p-24f, vv = float((kv << 1) | 1u) * 0x1p-24f;
        float w = 1.f - u - vv;
        vl = u * xyz(tr.v1) + vv * xyz(tr.v2) + w * xyz(tr.v3);  // already world space
        nl = normalize(u * xyz(tr.n1) + vv * xyz(tr.n2) + w * xyz(tr.n3));
        p = tr.v1.w * rcp(float(count));
    } else if (shape == LS_SPHERE) {
        V tl = pos;
        if (xf) {
            const F4 i0 = x.inv(0), i1 = x.inv(1), i2 = x.inv(2);
            tl = mk(dot3w(i0, pos), dot3w(i1, pos), dot3w(i2, pos));
        }
        float dx, dy;
        rng.unit_disc(dx, dy);
        float z = sqrt1(fmaxf(1.f - dx * dx - dy * dy, 0.f));
        V nn = normalize(tl);
        bool normal_x = fabsf(nn.x) >= 1.17549435e-38f && fabsf(nn.x) < kInf;
        V n1 = normal_x ? normalize(mk(nn.y, -nn.x, 0.f)) : normalize(mk(0.f, -nn.z, nn.y));
        V n2 = cross(n1, nn);
        vl = dx * n1 + dy * n2 + z * nn;
        nl = vl;
        p = z * kInvPi;
    } else {
        float a = rng.uniform() - 0.5f, b = rng.uniform() - 0.5f;
        uint32_t f = rng.index(6);
        switch (f) {
            case 0: vl = mk(a, b, 0.5f); nl = mk(0, 0, 1); break;
            case 1: vl = mk(a, b, -0.5f); nl = mk(0, 0, -1); break;
            case 2: vl = mk(a, 0.5f, b); nl = mk(0, 1, 0); break;
            case 3: vl = mk(a, -0.5f, b); nl = mk(0, -1, 0); break;
            case 4: vl = mk(0.5f, a, b); nl = mk(1, 0, 0); break;
            default: vl = mk(-0.5f, a, b); nl = mk(-1, 0, 0); break;
        }
        p = 1.f / 6.f;
    }
    if (xf) {
        const F4 n0 = x.nrm(0), n1 = x.nrm(1), n2 = x.nrm(2);
        n = normalize(mk(dot3(n0, nl), dot3(n1, nl), dot3(n2, nl)));
        const F4 l0 = x.lin(0), l1 = x.lin(1), l2 = x.lin(2);
        V ln = mk(dot3(l0, nl), dot3(l1, nl), dot3(l2, nl));
        float height = dot(ln, n);
        float base = n0.w * rcp(height);
        if (mesh) {
            v = vl;
        } else {
            const F4 f0 = x.fwd(0), f1 = x.fwd(1), f2 = x.fwd(2);
            v = mk(dot3w(f0, vl), dot3w(f1, vl), dot3w(f2, vl));
        }
        p = p * rcp(base);
    } else {
        v = vl;
        n = nl;
    }
}
// Shape::sample of a Light::Object.  A KdTree group (src/kdtree.rs:141-146) samples a uniformly chosen child and
// divides its pdf by the child count, nested groups repeat that: every lane descends to its own leaf.
template <bool GROUPS, class ST = SceneStructRt, class LD = LightRt>
RPT_DEV void sample_light_shape(const SceneView& scene_, const Light& L, V pos, Rng& rng, V& v, V& n, float& p,
                                const LdsTables& tab = LdsTables{}, LD ld = LD{}) {
    const auto& sc = *kernarg_scene();   // (see kernarg_scene)
    if (!GROUPS || L.shape != LS_GROUP) {  // wave-uniform
        sample_light_leaf<true, ST, LD>(scene_, ld.shape(L), L.first, L.count, &sc.lxf[L.xf], pos, rng, v, n, p, tab, ld);
        return;
    }
    uint32_t shape = LS_GROUP, first = L.first, count = L.count, xfi = 0;
    float pick = 1.f;
    while (shape == LS_GROUP) {
        const uint32_t idx = rng.index(count);
        pick *= rcp(float(count));
        const LightPart part = sc.lparts[first + idx];
        shape = part.shape; first = part.first; count = part.count; xfi = part.xf;
    }
    sample_light_leaf<false, ST>(scene_, shape, first, count, &sc.lxf[xfi], pos, rng, v, n, p, tab);
    p *= pick;
}
template <bool GROUPS, class ST = SceneStructRt, class LD = LightRt>
RPT_DEV void illuminate_object(const SceneView& sc, const Light& L, V pos, Rng& rng, V& intensity, V& wi,
                               float& dist, const LdsTables& tab = LdsTables{}, LD ld = LD{}) {
    V v, n;
    float p;
    sample_light_shape<GROUPS, ST, LD>(sc, L, pos, rng, v, n, p, tab, ld);
    V disp = v - pos;
    float len2 = dot(disp, disp);
    float ilen = rsq(len2);
    float cosine = fmaxf(-dot(disp, n), 0.f) * ilen;
    float surface_area = cosine * rcp(len2);
    intensity = (surface_area * rcp(p)) * xyz(L.color);
    wi = ilen * disp;
    dist = len2 * ilen;
}

// ------------------------------------------------------------------ environment
// Environment::get_color, src/environment.rs:72-77; Hdri::get_color / bilinear_sample :25-52.
template <class ST = SceneStructRt>
RPT_DEV V env_color(const SceneView& scene_, V dir) {
    const auto& sc = *kernarg_scene();   // (see kernarg_scene)
    if (!ST::has_hdri(sc.hdri_w)) return mk(sc.env[0], sc.env[1], sc.env[2]);
    const V d = normalize(dir);
    const float azimuth = atan2f(d.z, d.x) + kPi;
    const float polar = acosf(fminf(fmaxf(d.y, -1.f), 1.f));
    const float x = azimuth * (0.5f * kInvPi) * float(sc.hdri_w - 1u);
    const float y = polar * kInvPi * float(sc.hdri_h - 1u);
    const uint32_t x0 = min(uint32_t(x), sc.hdri_w - 1u), y0 = min(uint32_t(y), sc.hdri_h - 1u);
    const float ax = x - float(x0), ay = y - float(y0);
    const uint32_t x1 = min(x0 + 1u, sc.hdri_w - 1u), y1 = min(y0 + 1u, sc.hdri_h - 1u);  // weight 0 where clamped
    const V c00 = xyz(sc.hdri[y0 * sc.hdri_w + x0]), c01 = xyz(sc.hdri[y0 * sc.hdri_w + x1]);
    const V c10 = xyz(sc.hdri[y1 * sc.hdri_w + x0]), c11 = xyz(sc.hdri[y1 * sc.hdri_w + x1]);
    const V top = (1.f - ax) * c00 + ax * c01, bot = (1.f - ax) * c10 + ax * c11;
    return (1.f - ay) * top + ay * bot;
}

// ------------------------------------------------------------------ camera
// Pixel -> NDC of get_color, src/renderer.rs:174-176 (2 x + 1 and 2 (h - y) - 1 in u32, like the reference; inv_dim = 1 / max(w, h)).
RPT_DEV float pixel_xn(uint32_t x, uint32_t w, float inv_dim) { return (float(2u * x + 1u) - float(w)) * inv_dim; }
RPT_DEV float pixel_yn(uint32_t y, uint32_t h, float inv_dim) { return (float(2u * (h - y) - 1u) - float(h)) * inv_dim; }
// Camera::cast_ray, src/camera.rs:65-82 (cot(fov/2)*direction and `right` hoisted to the host).
template <class R>   // (R: Rng, or the generator of a flavour that takes other forms)
RPT_DEV void cast_ray(const CameraG& c, float x, float y, R& rng, V& o, V& d) {
    V right = mk(c.right[0], c.right[1], c.right[2]), up = mk(c.up[0], c.up[1], c.up[2]);
    o = mk(c.eye[0], c.eye[1], c.eye[2]);
    V nd = mk(c.ddir[0], c.ddir[1], c.ddir[2]) + x * right + y * up;
    if (c.aperture > 0.f) {
        V focal = fma3(c.focal_distance, normalize(nd), o);
        float dx, dy;
        rng.unit_disc(dx, dy);
        o = o + c.aperture * (dx * right + dy * up);
        nd = focal - o;
    }
    d = normalize(nd);
}

}  // namespace rptg
