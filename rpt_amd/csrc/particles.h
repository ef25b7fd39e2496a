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
}  // namespace rptg
