// particles.h — what rpt_particles.cpp hands to particles.hip (the declarations are weak, as in kernels.h: a host build without the
// kernels links, and the entry points then report RPT_ERR_UNSUPPORTED).
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>

namespace rptg {
struct ParticlesArgs {
    int32_t kind;            // RPT_PARTICLES_*
    uint32_t n;              // 1..256
    double radius, height;
    double* pos;             // [n * 3], read at the start of a launch and written at its end
    double* vel;
    uint64_t* counters;      // [6]: the launch adds its own
    uint32_t n_steps;        // 1..256 RK4 steps: all of size h, but the last of size h_tail where `tail` is set
    uint32_t tail;
    double h, h_tail;
};
// block: 256, 512 or 1024 threads; lanes: 8, 16, 32 or 64 lanes per particle in the closest-point argmin (tuning, no effect on results)
__attribute__((weak)) hipError_t launch_particles_integrate(const ParticlesArgs& a, uint32_t block, uint32_t lanes, hipStream_t stream);
// MARBLES: the display positions of pos to d_out [n * 3]
__attribute__((weak)) hipError_t launch_particles_display(const ParticlesArgs& a, double* d_out, hipStream_t stream);

// ---- ensembles (rpt_particles_batch_*): block b of a launch integrates system b of the table
struct ParticlesSystemRecord {   // 32 bytes
    int32_t kind;
    uint32_t n;
    uint32_t first;          // the index of the system's first particle in the batch's concatenated pos / vel arrays
    uint32_t reserved;
    double radius, height;
};
struct ParticlesBatchArgs {
    const ParticlesSystemRecord* table;   // [n_systems], on the device
    uint32_t n_systems;      // the grid
    uint32_t n_max;          // the largest n of the table: what the dynamic LDS is sized for, and whether pair forces are staged
    double* pos;             // [sum(n) * 3]
    double* vel;
    uint64_t* counters;      // [n_systems * 8]: system b's six at 8 b
    uint32_t n_steps, tail;  // as ParticlesArgs: one step sequence for every system
    uint32_t lds_pad;        // bytes of dynamic LDS asked for on top of particles_batch_lds (measurements only: RPT_PARTICLES_TUNE's third number)
    double h, h_tail;
};
constexpr uint32_t kBatchStagedMaxN = 56;   // particles.hip's kStagedMaxN
constexpr uint32_t kBatchMaxSystems = 4096;
constexpr uint32_t kBatchMaxLds = 64u << 10;   // dynamic LDS of a launch, padding included (n_max = 56 needs 47 KiB)
constexpr uint32_t kBatchDefaultBlock = 256, kBatchDefaultLanes = 8;   // the sweep at n_systems = R ("Ensembles")
// A launch of a batch that needs `rounds` rounds of resident blocks lasts rounds x steps: it gets 256 / (rounds * kBatchLaunchScale)
// steps.  kBatchLaunchScale is what co-resident blocks cost each other in the longest launch, measured and rounded up to a power
// of two: 1,024 systems of 256 particles, four blocks on a CU, take 1.98 times the single handle's 256 steps (DESIGN.md section 4,
// "Ensembles").
constexpr uint32_t kBatchLaunchScale = 2;
// The dynamic LDS of a batch launch, every part a multiple of 16 bytes: stage positions and winners for n_max particles, the 201
// candidates (xf, yc), the six counter words, and up to 56 particles the pair forces and pair indices of n_max (n_max - 1) / 2 pairs.
struct ParticlesBatchLds {
    uint32_t pos, win, xf, yc, cnt, f, pair, bytes;   // byte offsets, and the total
};
inline constexpr uint32_t batch_lds_round16(uint32_t b) { return (b + 15u) & ~15u; }
inline constexpr ParticlesBatchLds particles_batch_lds(uint32_t n_max) {
    ParticlesBatchLds l{};
    const uint32_t pairs = n_max <= kBatchStagedMaxN ? n_max * (n_max - 1u) / 2u : 0u;
    l.pos = 0;
    l.win = l.pos + batch_lds_round16(24u * n_max);
    l.xf = l.win + batch_lds_round16(8u * n_max);
    l.yc = l.xf + batch_lds_round16(8u * 201u);
    l.cnt = l.yc + batch_lds_round16(8u * 201u);
    l.f = l.cnt + 32u;
    l.pair = l.f + batch_lds_round16(24u * pairs);
    l.bytes = l.pair + batch_lds_round16(4u * pairs);
    return l;
}
__attribute__((weak)) hipError_t launch_particles_batch_integrate(const ParticlesBatchArgs& a, uint32_t block, uint32_t lanes, hipStream_t stream);
// every system MARBLES: the display positions of pos to d_out [sum(n) * 3], one workgroup per system
__attribute__((weak)) hipError_t launch_particles_batch_display(const ParticlesBatchArgs& a, double* d_out, hipStream_t stream);
// R: how many blocks of the (block, lanes) instantiation with the dynamic LDS of n_max the device holds at once, CUs x blocks per CU
// from the occupancy query.  The one place the launch rule's R comes from (a CPU harness replaces it).
__attribute__((weak)) hipError_t particles_batch_resident_blocks(int device, uint32_t block, uint32_t lanes, uint32_t n_max, uint32_t lds_pad,
                                                                 uint32_t* resident);
}  // namespace rptg
