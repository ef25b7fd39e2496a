// particles.hip — rpt_particles_*: the particle systems of the reference's src/ode/ (SimpleCircleSystem, SolidGravitySystem,
// MarblesSystem) integrated with RK4 on the device, and the display positions of examples/marbles.rs.  The arithmetic is the order of
// fp64 operations that include/rpt_hip.h states and particles_core.h spells out, every one rounded on its own (contraction off, IEEE
// division and square root, no atomics on the state): tests/particles_ref.py restates it in numpy and the state is compared bit for bit.
//
// One workgroup integrates one system; the time loop runs inside the kernel.  Lane p owns particle p: its state, the stage state, the
// stage derivative and the running RK4 sum are the lane's registers (six doubles each); what the OTHER lanes read -- the stage
// positions -- is in LDS, with the winning candidate of each particle's closest-point scan and the 201 candidates (xf, yc), which
// depend on the height alone and are staged once per launch.  One derivative evaluation is three phases between two barriers:
//   1. pair terms: lane p loops over its partners q in ascending order (every lane reads the same LDS address: a broadcast), which
//      is the order in which the reference's loop touches particle p's accumulator.  Up to kStagedMaxN particles the n (n - 1) / 2
//      pair forces -- the square root and the four divisions, which both members of a pair see alike -- are first computed by ALL
//      lanes, one pair each, into LDS, and lane p's loop only adds them up (after the barrier of phase 2): the same operations on
//      the same values in the same order, so the same bits as the loop that computes them itself, which larger systems run;
//   2. the closest-point argmin: LANES lanes per particle (a power of two <= 64, so a group lies in one wave), candidates dealt
//      round robin, a butterfly of cross-lane shuffles on the key (distance, index): the smaller distance wins, of equal distances
//      the smaller index, NaN and >= 1e18 never -- the sequential scan's winner;
//   3. surface, table and air terms, lane p again.
// No grid-wide synchronisation, no spin wait.  The six counters are summed per lane, added up in LDS at the end of a launch and
// written by six lanes with ordinary stores.  A launch is at most 256 steps (rpt_particles.cpp cuts the sequence).
//
// rpt_particles_batch_*: the same body (integrate_system) with a grid of n_systems workgroups, block b on system b of a device
// table, and the per-system LDS arrays dynamic, sized for the batch's largest n.
#include <hip/hip_runtime.h>

#include "../../include/rpt_hip.h"
#include "particles.h"
#include "particles_core.h"

#pragma clang fp contract(off)

namespace rptg {
namespace {
using namespace rptp;

constexpr int kCand = 2 * kCoarseN + 1;
constexpr uint32_t kStagedMaxN = 56, kPairSlots = kStagedMaxN * (kStagedMaxN - 1) / 2;   // 1540 pairs: 36 KiB of forces, 6 KiB of indices
__device__ __forceinline__ uint32_t pair_slot(uint32_t hi, uint32_t lo) { return hi * (hi - 1u) / 2u + lo; }

struct Key {
    double d;
    int i;
};
__device__ __forceinline__ Key key_min(Key a, Key b) { return (b.d < a.d || (b.d == a.d && b.i < a.i)) ? b : a; }
template <int WIDTH>
__device__ __forceinline__ Key key_reduce(Key k) {
#pragma unroll
    for (int off = WIDTH / 2; off >= 1; off >>= 1) {
        Key o;
        o.d = __shfl_xor(k.d, off, WIDTH);
        o.i = __shfl_xor(k.i, off, WIDTH);
        k = key_min(k, o);
    }
    return k;
}

// What one workgroup does for one system: the body of both kernels, so that a system of a batch cannot differ from a system
// alone.  `lds` is where the per-system arrays lie (static in the single kernel, carved out of dynamic LDS in the batched one);
// `staged` is uniform over the block and picks where the pair forces are computed, never their values.
struct SystemLds {
    double* pos;        // [3 n]: the stage positions
    double* win;        // [n]: the winning xf of each particle's scan
    double *xf, *yc;    // [kCand]
    unsigned* cnt;      // [6]
    double* f;          // staged: the force of pair (hi, lo) at pair_slot(hi, lo)
    uint32_t* pair;     // ... hi << 16 | lo, and bit 31: the two touch (MARBLES; written per evaluation)
};
template <int BLOCK, int LANES>
__device__ __forceinline__ void integrate_system(const ParticlesArgs& a, const bool staged, const SystemLds lds) {
    static_assert(BLOCK >= int(kMaxParticles) && BLOCK % 64 == 0 && LANES <= 64 && (LANES & (LANES - 1)) == 0, "a lane per particle; a group within a wave");
    double* const s_pos = lds.pos;
    double* const s_win = lds.win;
    double* const s_xf = lds.xf;
    double* const s_yc = lds.yc;
    unsigned* const s_cnt = lds.cnt;
    double* const s_f = lds.f;
    uint32_t* const s_pair = lds.pair;
    const uint32_t t = threadIdx.x, n = a.n;
    const uint32_t n_pairs = n * (n - 1u) / 2u;
    if (staged && t < n)
        for (uint32_t lo = 0; lo < t; lo++) s_pair[pair_slot(t, lo)] = t << 16 | lo;
    const bool mine = t < n;
    const int kind = a.kind;
    const double r = a.radius, height = a.height;
    if (t < 6) s_cnt[t] = 0;
    if (kind == RPT_PARTICLES_MARBLES)
        for (uint32_t c = t; c < uint32_t(kCand); c += BLOCK) {
            const double xf = cand_xf(int(c) - kCoarseN, kCoarseN);
            s_xf[c] = xf;
            s_yc[c] = cand_yc(height, xf);
        }
    __syncthreads();
    double S[6] = {0, 0, 0, 0, 0, 0}, X[6], K[6] = {0, 0, 0, 0, 0, 0}, A[6] = {0, 0, 0, 0, 0, 0};
    if (mine)
        for (int k = 0; k < 3; k++) {
            S[k] = a.pos[3 * t + k];
            S[3 + k] = a.vel[3 * t + k];
        }
    uint32_t cnt[5] = {0, 0, 0, 0, 0};   // pair contacts, surface band / push, table band / push
    for (uint32_t step = 0; step < a.n_steps; step++) {
        const double h = (a.tail && step + 1 == a.n_steps) ? a.h_tail : a.h;
        const double hh = h / 2.0;
        for (int stage = 1; stage <= 4; stage++) {
            const double f = stage == 4 ? h : hh;
            for (int k = 0; k < 6; k++) X[k] = stage == 1 ? S[k] : rk4_stage(S[k], K[k], f);
            // ---- K = f(X)
            if (kind == RPT_PARTICLES_CIRCLE) {
                circle_derivative(X, K, K + 3);
            } else {
                if (mine)
                    for (int k = 0; k < 3; k++) s_pos[3 * t + k] = X[k];
                __syncthreads();
                double acc[3] = {0.0, kind == RPT_PARTICLES_MARBLES ? -1.0 : 0.0, 0.0};
                if (staged) {
                    for (uint32_t i = t; i < n_pairs; i += BLOCK) {
                        const uint32_t w = s_pair[i] & 0x7fffffffu, hi = w >> 16, lo = w & 0xffffu;
                        double f[3] = {0.0, 0.0, 0.0};
                        bool touch = false;
                        if (kind == RPT_PARTICLES_GRAVITY)
                            gravity_pair_force(s_pos + 3 * hi, s_pos + 3 * lo, f);
                        else
                            touch = marbles_pair_force(s_pos + 3 * hi, s_pos + 3 * lo, r, f);
                        for (int k = 0; k < 3; k++) s_f[3 * i + k] = f[k];
                        s_pair[i] = w | (touch ? 0x80000000u : 0u);
                    }
                    if (kind == RPT_PARTICLES_GRAVITY) {
                        __syncthreads();
                        if (mine)
                            for (uint32_t q = 0; q < n; q++)
                                if (q != t) gravity_pair_apply(s_f + 3 * (q < t ? pair_slot(t, q) : pair_slot(q, t)), q < t, acc);
                    }
                } else if (mine) {
                    if (kind == RPT_PARTICLES_GRAVITY) {
                        for (uint32_t q = 0; q < n; q++)
                            if (q != t) gravity_pair(X, s_pos + 3 * q, q < t, acc);
                    } else {
                        for (uint32_t q = 0; q < n; q++)
                            if (q != t && marbles_pair(X, s_pos + 3 * q, X + 3, r, q < t, acc) && q < t) cnt[0]++;
                    }
                }
                if (kind == RPT_PARTICLES_MARBLES) {
                    constexpr uint32_t kGroups = BLOCK / LANES;
                    const uint32_t g = t / LANES, l = t % LANES;
                    for (uint32_t base = 0; base < n; base += kGroups) {   // (uniform over the block: every lane takes part in the shuffles)
                        const uint32_t p = base + g;
                        const bool have = p < n;
                        double P[3] = {0.0, 0.0, 0.0};
                        if (have)
                            for (int k = 0; k < 3; k++) P[k] = s_pos[3 * p + k];
                        const double px = closest_px(P), py = P[1];
                        Key best{kNoWin, kNoIndex};
                        for (int c = int(l); c < kCand; c += LANES) {
                            const double d = cand_d(px, py, s_xf[c], s_yc[c]);
                            if (d < best.d) best = Key{d, c};
                        }
                        best = key_reduce<LANES>(best);
                        if (have && l == 0) s_win[p] = best.i == kNoIndex ? -1.0 : s_xf[best.i];
                    }
                    __syncthreads();
                    if (staged && mine)
                        for (uint32_t q = 0; q < n; q++) {
                            if (q == t) continue;
                            const uint32_t slot = q < t ? pair_slot(t, q) : pair_slot(q, t);
                            if (s_pair[slot] >> 31) {
                                marbles_pair_apply(s_f + 3 * slot, X + 3, q < t, acc);
                                if (q < t) cnt[0]++;
                            }
                        }
                    if (mine) {
                        double C[3];
                        if (length3(X) < 1e-12) {
                            C[0] = X[0]; C[1] = X[1]; C[2] = X[2];
                        } else {
                            closest_finish(height, X, closest_px(X), s_win[t], C);
                        }
                        marbles_rest(r, X, X + 3, C, acc, cnt + 1);
                    }
                } else {
                    __syncthreads();   // nobody overwrites s_pos while a lane still reads it
                }
                for (int k = 0; k < 3; k++) {
                    K[k] = X[3 + k];
                    K[3 + k] = acc[k];
                }
            }
            for (int k = 0; k < 6; k++) A[k] = rk4_sum(A[k], K[k], stage);
        }
        for (int k = 0; k < 6; k++) S[k] = rk4_new(S[k], A[k], h);
    }
    if (mine)
        for (int k = 0; k < 3; k++) {
            a.pos[3 * t + k] = S[k];
            a.vel[3 * t + k] = S[3 + k];
        }
    // the counters: LDS atomics on integers (never on the state), then six plain stores
    if (mine)
        for (int k = 0; k < 5; k++)
            if (cnt[k]) atomicAdd(&s_cnt[1 + k], cnt[k]);
    if (t == 0) s_cnt[0] = 4u * a.n_steps;
    __syncthreads();
    if (t < 6) a.counters[t] = a.counters[t] + uint64_t(s_cnt[t]);
}

template <int BLOCK, int LANES>
__global__ __launch_bounds__(BLOCK) void particles_integrate_kernel(const ParticlesArgs a) {
    __shared__ double s_pos[3 * kMaxParticles];
    __shared__ double s_win[kMaxParticles];
    __shared__ double s_xf[kCand], s_yc[kCand];
    __shared__ unsigned s_cnt[6];
    __shared__ double s_f[3 * kPairSlots];        // n <= kStagedMaxN
    __shared__ uint32_t s_pair[kPairSlots];
    integrate_system<BLOCK, LANES>(a, a.n <= kStagedMaxN && a.kind != RPT_PARTICLES_CIRCLE, SystemLds{s_pos, s_win, s_xf, s_yc, s_cnt, s_f, s_pair});
}

// The batched form: block b integrates system b of the table.  The per-system arrays are dynamic LDS sized for the batch's largest
// n (particles_batch_lds), so blocks of small systems co-reside up to the CU's wave limit; pair forces are staged when that n is at
// most kStagedMaxN, for every system of the batch alike.  Blocks share nothing: no grid-wide synchronisation, no spin wait, no
// atomics on state, and system b's counters at counters[8 b ..] get the same plain stores.
template <int BLOCK, int LANES>
__global__ __launch_bounds__(BLOCK) void particles_batch_integrate_kernel(const ParticlesBatchArgs b) {
    extern __shared__ __attribute__((aligned(16))) unsigned char s_batch[];
    const uint32_t sys = blockIdx.x;
    if (sys >= b.n_systems) return;   // (uniform over the block)
    const ParticlesSystemRecord rec = b.table[sys];
    const ParticlesBatchLds l = particles_batch_lds(b.n_max);
    ParticlesArgs a;
    a.kind = rec.kind;
    a.n = rec.n;
    a.radius = rec.radius;
    a.height = rec.height;
    a.pos = b.pos + 3 * size_t(rec.first);
    a.vel = b.vel + 3 * size_t(rec.first);
    a.counters = b.counters + 8 * size_t(sys);
    a.n_steps = b.n_steps;
    a.tail = b.tail;
    a.h = b.h;
    a.h_tail = b.h_tail;
    integrate_system<BLOCK, LANES>(a, b.n_max <= kStagedMaxN && rec.kind != RPT_PARTICLES_CIRCLE,
                                   SystemLds{reinterpret_cast<double*>(s_batch + l.pos), reinterpret_cast<double*>(s_batch + l.win),
                                             reinterpret_cast<double*>(s_batch + l.xf), reinterpret_cast<double*>(s_batch + l.yc),
                                             reinterpret_cast<unsigned*>(s_batch + l.cnt), reinterpret_cast<double*>(s_batch + l.f),
                                             reinterpret_cast<uint32_t*>(s_batch + l.pair)});
}

// The display positions: closest_point_precise recomputes its 20,001 candidates, the whole workgroup on one particle at a time.
constexpr int kDisplayBlock = 256;
__device__ __forceinline__ void display_system(const ParticlesArgs& a, double* __restrict__ out) {
    constexpr int kWaves = kDisplayBlock / 64;
    __shared__ double s_d[kWaves];
    __shared__ int s_i[kWaves];
    __shared__ int s_win[kMaxParticles];
    const uint32_t t = threadIdx.x, n = a.n;
    for (uint32_t p = 0; p < n; p++) {
        const double P[3] = {a.pos[3 * p], a.pos[3 * p + 1], a.pos[3 * p + 2]};
        const double px = closest_px(P), py = P[1];
        Key best{kNoWin, kNoIndex};
        for (int c = int(t); c <= 2 * kPreciseN; c += kDisplayBlock) {
            const double xf = cand_xf(c - kPreciseN, kPreciseN);
            const double d = cand_d(px, py, xf, cand_yc(a.height, xf));
            if (d < best.d) best = Key{d, c};
        }
        best = key_reduce<64>(best);
        if ((t & 63u) == 0) {
            s_d[t >> 6] = best.d;
            s_i[t >> 6] = best.i;
        }
        __syncthreads();
        if (t == 0) {
            Key k{s_d[0], s_i[0]};
            for (int w = 1; w < kWaves; w++) k = key_min(k, Key{s_d[w], s_i[w]});
            s_win[p] = k.i;
        }
        __syncthreads();
    }
    if (t < n) {
        const double P[3] = {a.pos[3 * t], a.pos[3 * t + 1], a.pos[3 * t + 2]};
        double C[3], D[3];
        if (length3(P) < 1e-12) {
            C[0] = P[0]; C[1] = P[1]; C[2] = P[2];
        } else {
            const int w = s_win[t];
            closest_finish(a.height, P, closest_px(P), w == kNoIndex ? -1.0 : cand_xf(w - kPreciseN, kPreciseN), C);
        }
        display_position(a.radius, P, C, D);
        for (int k = 0; k < 3; k++) out[3 * t + k] = D[k];
    }
}
__global__ __launch_bounds__(kDisplayBlock) void particles_display_kernel(const ParticlesArgs a, double* __restrict__ out) { display_system(a, out); }
// ... and of a batch: block b shows system b of the table (every system MARBLES: the host checks)
__global__ __launch_bounds__(kDisplayBlock) void particles_batch_display_kernel(const ParticlesBatchArgs b, double* __restrict__ out) {
    const uint32_t sys = blockIdx.x;
    if (sys >= b.n_systems) return;
    const ParticlesSystemRecord rec = b.table[sys];
    ParticlesArgs a{};
    a.kind = rec.kind;
    a.n = rec.n;
    a.radius = rec.radius;
    a.height = rec.height;
    a.pos = b.pos + 3 * size_t(rec.first);
    display_system(a, out + 3 * size_t(rec.first));
}

template <int BLOCK>
hipError_t launch_block(const ParticlesArgs& a, uint32_t lanes, hipStream_t stream) {
    switch (lanes) {
    case 8: hipLaunchKernelGGL((particles_integrate_kernel<BLOCK, 8>), dim3(1), dim3(BLOCK), 0, stream, a); break;
    case 16: hipLaunchKernelGGL((particles_integrate_kernel<BLOCK, 16>), dim3(1), dim3(BLOCK), 0, stream, a); break;
    case 32: hipLaunchKernelGGL((particles_integrate_kernel<BLOCK, 32>), dim3(1), dim3(BLOCK), 0, stream, a); break;
    case 64: hipLaunchKernelGGL((particles_integrate_kernel<BLOCK, 64>), dim3(1), dim3(BLOCK), 0, stream, a); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// The batched instantiations, by (block, lanes): one table for the launch and for the occupancy query, so that R is asked of the
// kernel that runs.
using BatchKernel = void (*)(const ParticlesBatchArgs);
template <int BLOCK>
BatchKernel batch_kernel_of(uint32_t lanes) {
    switch (lanes) {
    case 8: return particles_batch_integrate_kernel<BLOCK, 8>;
    case 16: return particles_batch_integrate_kernel<BLOCK, 16>;
    case 32: return particles_batch_integrate_kernel<BLOCK, 32>;
    case 64: return particles_batch_integrate_kernel<BLOCK, 64>;
    default: return nullptr;
    }
}
BatchKernel batch_kernel(uint32_t block, uint32_t lanes) {
    switch (block) {
    case 256: return batch_kernel_of<256>(lanes);
    case 512: return batch_kernel_of<512>(lanes);
    case 1024: return batch_kernel_of<1024>(lanes);
    default: return nullptr;
    }
}
}  // namespace

hipError_t launch_particles_integrate(const ParticlesArgs& a, uint32_t block, uint32_t lanes, hipStream_t stream) {
    if (a.n < 1 || a.n > kMaxParticles || a.n_steps < 1 || a.n_steps > kMaxLaunchSteps || a.kind < 0 || a.kind > 2) return hipErrorInvalidValue;
    switch (block) {
    case 256: return launch_block<256>(a, lanes, stream);
    case 512: return launch_block<512>(a, lanes, stream);
    case 1024: return launch_block<1024>(a, lanes, stream);
    default: return hipErrorInvalidValue;
    }
}

hipError_t launch_particles_display(const ParticlesArgs& a, double* d_out, hipStream_t stream) {
    if (a.n < 1 || a.n > kMaxParticles) return hipErrorInvalidValue;
    hipLaunchKernelGGL(particles_display_kernel, dim3(1), dim3(kDisplayBlock), 0, stream, a, d_out);
    return hipGetLastError();
}

hipError_t launch_particles_batch_integrate(const ParticlesBatchArgs& a, uint32_t block, uint32_t lanes, hipStream_t stream) {
    const BatchKernel k = batch_kernel(block, lanes);
    if (!k || !a.table || !a.pos || !a.vel || !a.counters || a.n_systems < 1 || a.n_systems > kBatchMaxSystems || a.n_max < 1 || a.n_max > kMaxParticles ||
        a.n_steps < 1 || a.n_steps > kMaxLaunchSteps || a.lds_pad > kBatchMaxLds ||
        particles_batch_lds(a.n_max).bytes + a.lds_pad > kBatchMaxLds)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(k, dim3(a.n_systems), dim3(block), particles_batch_lds(a.n_max).bytes + a.lds_pad, stream, a);
    return hipGetLastError();
}

hipError_t launch_particles_batch_display(const ParticlesBatchArgs& a, double* d_out, hipStream_t stream) {
    if (!a.table || !a.pos || !d_out || a.n_systems < 1 || a.n_systems > kBatchMaxSystems) return hipErrorInvalidValue;
    hipLaunchKernelGGL(particles_batch_display_kernel, dim3(a.n_systems), dim3(kDisplayBlock), 0, stream, a, d_out);
    return hipGetLastError();
}

hipError_t particles_batch_resident_blocks(int device, uint32_t block, uint32_t lanes, uint32_t n_max, uint32_t lds_pad, uint32_t* resident) {
    const BatchKernel k = batch_kernel(block, lanes);
    if (!k || !resident || n_max < 1 || n_max > kMaxParticles || lds_pad > kBatchMaxLds || particles_batch_lds(n_max).bytes + lds_pad > kBatchMaxLds)
        return hipErrorInvalidValue;
    int per_cu = 0, cus = 0;
    hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, reinterpret_cast<const void*>(k), int(block), particles_batch_lds(n_max).bytes + lds_pad);
    if (e == hipSuccess) e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device);
    if (e != hipSuccess) return e;
    if (per_cu < 1 || cus < 1) return hipErrorInvalidValue;
    *resident = uint32_t(per_cu) * uint32_t(cus);
    return hipSuccess;
}

}  // namespace rptg
