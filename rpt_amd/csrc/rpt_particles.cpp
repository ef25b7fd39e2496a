// rpt_particles.cpp — the host half of rpt_particles_* and the pure host functions next to them (include/rpt_hip.h, "particle
// systems").  The arithmetic is particles_core.h's, the text the kernel compiles: rpt_particles_integrate_host is that text run
// serially.  A handle owns its state arrays and counters on one device and shares nothing with scenes or with other handles; its
// calls are ordered, whatever their streams, through one event, as the accumulators' are.  A batch (rpt_particles_batch) is the same
// for many systems at once: concatenated state arrays, a device table with one record per system, one event, and a launch length
// that shrinks with the number of rounds the device needs for the batch's blocks.
#include <hip/hip_runtime_api.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/rpt_hip.h"
#include "host_internal.h"
#include "particles.h"
#include "particles_core.h"

using rpti::fail;
using namespace rptg;

struct rpt_particles {
    int device = 0;
    rpt_particles_params prm{};
    rpti::DevMem d_pos, d_vel, d_cnt, d_disp;
    rpti::Event done;                 // recorded after the last launch of a call: the next call waits for it, whatever its stream
    bool used = false;
    uint64_t launches = 0;
    uint32_t block = 512, lanes = 16;   // tuning (the sweep at n = 25); RPT_PARTICLES_TUNE="block,lanes" overrides them for measurements
};

static int check_params(const rpt_particles_params* p) {
    if (!p) return fail(RPT_ERR_INVALID, "null particle parameters");
    if (p->kind < RPT_PARTICLES_CIRCLE || p->kind > RPT_PARTICLES_MARBLES) return fail(RPT_ERR_INVALID, "unknown particle system kind");
    if (p->n < 1 || p->n > rptp::kMaxParticles) return fail(RPT_ERR_INVALID, "the number of particles must be 1..256");
    if (!std::isfinite(p->radius) || !std::isfinite(p->height)) return fail(RPT_ERR_INVALID, "radius and height must be finite");
    if (p->kind == RPT_PARTICLES_MARBLES && !(p->radius > 0.0)) return fail(RPT_ERR_INVALID, "a marbles system needs radius > 0");
    return RPT_OK;
}
static int check_time(double time, double step, uint64_t* n_full, double* last) {
    if (!std::isfinite(time) || time < 0.0) return fail(RPT_ERR_INVALID, "time must be finite and >= 0");
    if (!std::isfinite(step) || !(step > 0.0)) return fail(RPT_ERR_INVALID, "step must be finite and > 0");
    if (!rptp::step_sequence(time, step, n_full, last)) return fail(RPT_ERR_INVALID, "more than 2^20 steps in one call");
    return RPT_OK;
}

extern "C" {
rpt_particles* rpt_particles_create(int device, const rpt_particles_params* prm) {
    if (check_params(prm) != RPT_OK) return nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) { fail(RPT_ERR_INVALID, "device index out of range"); return nullptr; }
    auto* h = new rpt_particles();
    h->device = device;
    h->prm = *prm;
    if (const char* tune = std::getenv("RPT_PARTICLES_TUNE")) {
        unsigned b = 0, l = 0;
        if (std::sscanf(tune, "%u,%u", &b, &l) == 2 && (b == 256 || b == 512 || b == 1024) && (l == 8 || l == 16 || l == 32 || l == 64)) {
            h->block = b;
            h->lanes = l;
        }
    }
    const size_t bytes = size_t(prm->n) * 3 * sizeof(double);
    const bool ok = hipSetDevice(device) == hipSuccess && h->d_pos.reserve(bytes) == hipSuccess && h->d_vel.reserve(bytes) == hipSuccess &&
                    h->d_disp.reserve(bytes) == hipSuccess && h->d_cnt.reserve(8 * sizeof(uint64_t)) == hipSuccess &&
                    hipMemset(h->d_pos.get(), 0, bytes) == hipSuccess && hipMemset(h->d_vel.get(), 0, bytes) == hipSuccess &&
                    hipMemset(h->d_cnt.get(), 0, 8 * sizeof(uint64_t)) == hipSuccess && h->done.create(hipEventDisableTiming) == hipSuccess;
    if (!ok) {
        fail(RPT_ERR_DEVICE, "rpt_particles_create: device allocation failed");
        rpt_particles_destroy(h);
        return nullptr;
    }
    return h;
}
void rpt_particles_destroy(rpt_particles* h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    delete h;
}
// The synchronous calls: wait for what the handle has queued, then use blocking copies.
static int settle(rpt_particles* h) {
    RPTI_HIP_TRY(hipSetDevice(h->device));
    if (h->used) RPTI_HIP_TRY(hipEventSynchronize(h->done.get()));
    return RPT_OK;
}
int rpt_particles_set_state(rpt_particles* h, const double* pos, const double* vel) {
    if (!pos) return fail(RPT_ERR_INVALID, "null positions");
    if (!h) return fail(RPT_ERR_INVALID, "null particle system");
    if (int rc = settle(h)) return rc;
    const size_t bytes = size_t(h->prm.n) * 3 * sizeof(double);
    RPTI_HIP_TRY(hipMemcpy(h->d_pos.get(), pos, bytes, hipMemcpyHostToDevice));
    if (vel)
        RPTI_HIP_TRY(hipMemcpy(h->d_vel.get(), vel, bytes, hipMemcpyHostToDevice));
    else
        RPTI_HIP_TRY(hipMemset(h->d_vel.get(), 0, bytes));
    return RPT_OK;
}
int rpt_particles_state(rpt_particles* h, double* pos, double* vel) {
    if (!pos && !vel) return fail(RPT_ERR_INVALID, "null outputs");
    if (!h) return fail(RPT_ERR_INVALID, "null particle system");
    if (int rc = settle(h)) return rc;
    const size_t bytes = size_t(h->prm.n) * 3 * sizeof(double);
    if (pos) RPTI_HIP_TRY(hipMemcpy(pos, h->d_pos.get(), bytes, hipMemcpyDeviceToHost));
    if (vel) RPTI_HIP_TRY(hipMemcpy(vel, h->d_vel.get(), bytes, hipMemcpyDeviceToHost));
    return RPT_OK;
}
int rpt_particles_state_device(rpt_particles* h, void** d_pos, void** d_vel) {
    if (!d_pos && !d_vel) return fail(RPT_ERR_INVALID, "null outputs");
    if (!h) return fail(RPT_ERR_INVALID, "null particle system");
    if (d_pos) *d_pos = h->d_pos.get();
    if (d_vel) *d_vel = h->d_vel.get();
    return RPT_OK;
}
int rpt_particles_integrate(rpt_particles* h, double time, double step, void* hip_stream) {
    uint64_t n_full = 0;
    double last = 0.0;
    if (int rc = check_time(time, step, &n_full, &last)) return rc;
    if (!h) return fail(RPT_ERR_INVALID, "null particle system");
    if (!launch_particles_integrate) return fail(RPT_ERR_UNSUPPORTED, "rpt_particles_integrate: built without the kernels");
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    RPTI_HIP_TRY(hipSetDevice(h->device));
    if (h->used) RPTI_HIP_TRY(hipStreamWaitEvent(st, h->done.get(), 0));
    h->used = true;
    ParticlesArgs a{};
    a.kind = h->prm.kind;
    a.n = h->prm.n;
    a.radius = h->prm.radius;
    a.height = h->prm.height;
    a.pos = h->d_pos.get<double>();
    a.vel = h->d_vel.get<double>();
    a.counters = h->d_cnt.get<uint64_t>();
    a.h = step;
    a.h_tail = last;
    // n_full steps of `step` and one of `last`, in launches of at most kMaxLaunchSteps steps; the state stays in the handle's arrays
    hipError_t e = hipSuccess;
    for (uint64_t left = n_full + 1; left > 0 && e == hipSuccess;) {
        const uint32_t m = uint32_t(left < rptp::kMaxLaunchSteps ? left : rptp::kMaxLaunchSteps);
        a.n_steps = m;
        a.tail = left == m ? 1u : 0u;
        e = launch_particles_integrate(a, h->block, h->lanes, st);
        if (e == hipSuccess) h->launches++;
        left -= m;
    }
    // (recorded after a failed launch too: the launches before it are queued, and the next call has to wait for them)
    const hipError_t er = hipEventRecord(h->done.get(), st);
    RPTI_HIP_TRY(e);
    RPTI_HIP_TRY(er);
    return RPT_OK;
}
int rpt_particles_display_positions(rpt_particles* h, double* out) {
    if (!out) return fail(RPT_ERR_INVALID, "null output");
    if (!h) return fail(RPT_ERR_INVALID, "null particle system");
    if (h->prm.kind != RPT_PARTICLES_MARBLES) return fail(RPT_ERR_UNSUPPORTED, "display positions are defined for a marbles system only");
    if (!launch_particles_display) return fail(RPT_ERR_UNSUPPORTED, "rpt_particles_display_positions: built without the kernels");
    if (int rc = settle(h)) return rc;
    ParticlesArgs a{};
    a.kind = h->prm.kind;
    a.n = h->prm.n;
    a.radius = h->prm.radius;
    a.height = h->prm.height;
    a.pos = h->d_pos.get<double>();
    a.vel = h->d_vel.get<double>();
    RPTI_HIP_TRY(launch_particles_display(a, h->d_disp.get<double>(), nullptr));
    h->launches++;
    RPTI_HIP_TRY(hipMemcpy(out, h->d_disp.get(), size_t(a.n) * 3 * sizeof(double), hipMemcpyDeviceToHost));
    return RPT_OK;
}
int rpt_particles_display_positions_device(rpt_particles* h, void** d_out, void* hip_stream) {
    if (!d_out) return fail(RPT_ERR_INVALID, "null output");
    if (!h) return fail(RPT_ERR_INVALID, "null particle system");
    if (h->prm.kind != RPT_PARTICLES_MARBLES) return fail(RPT_ERR_UNSUPPORTED, "display positions are defined for a marbles system only");
    if (!launch_particles_display) return fail(RPT_ERR_UNSUPPORTED, "rpt_particles_display_positions_device: built without the kernels");
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    RPTI_HIP_TRY(hipSetDevice(h->device));
    if (h->used) RPTI_HIP_TRY(hipStreamWaitEvent(st, h->done.get(), 0));
    h->used = true;
    ParticlesArgs a{};
    a.kind = h->prm.kind;
    a.n = h->prm.n;
    a.radius = h->prm.radius;
    a.height = h->prm.height;
    a.pos = h->d_pos.get<double>();
    a.vel = h->d_vel.get<double>();
    const hipError_t e = launch_particles_display(a, h->d_disp.get<double>(), st);
    if (e == hipSuccess) h->launches++;
    const hipError_t er = hipEventRecord(h->done.get(), st);   // (after a failed launch too, as rpt_particles_integrate)
    RPTI_HIP_TRY(e);
    RPTI_HIP_TRY(er);
    *d_out = h->d_disp.get();
    return RPT_OK;
}
int rpt_particles_counters(rpt_particles* h, uint64_t out[8]) {
    if (!out) return fail(RPT_ERR_INVALID, "null output");
    if (!h) return fail(RPT_ERR_INVALID, "null particle system");
    if (int rc = settle(h)) return rc;
    RPTI_HIP_TRY(hipMemcpy(out, h->d_cnt.get(), 8 * sizeof(uint64_t), hipMemcpyDeviceToHost));
    out[6] = h->launches;
    out[7] = 0;
    return RPT_OK;
}

}  // extern "C"

// ---- ensembles: many independent systems, one workgroup each, in one launch (include/rpt_hip.h, "particle ensembles")
struct rpt_particles_batch {
    int device = 0;
    std::vector<ParticlesSystemRecord> table;   // the host's copy of the device table
    uint32_t total = 0, n_max = 0;              // particles of all systems; the largest system
    bool all_marbles = true;
    rpti::DevMem d_pos, d_vel, d_disp, d_cnt, d_table, d_first;
    rpti::Event done;                           // as rpt_particles::done
    bool used = false;
    uint64_t launches = 0;
    uint32_t block = kBatchDefaultBlock, lanes = kBatchDefaultLanes;   // the sweep at n_systems = R; RPT_PARTICLES_TUNE overrides them
    uint32_t lds_pad = 0;                       // RPT_PARTICLES_TUNE="block,lanes,pad": extra dynamic LDS per block, to measure what sizing it to the batch buys
    uint32_t resident = 0;                      // R of the launch rule, for this instantiation and this dynamic LDS
};

static ParticlesBatchArgs batch_args(rpt_particles_batch* b) {
    ParticlesBatchArgs a{};
    a.table = b->d_table.get<ParticlesSystemRecord>();
    a.n_systems = uint32_t(b->table.size());
    a.n_max = b->n_max;
    a.pos = b->d_pos.get<double>();
    a.vel = b->d_vel.get<double>();
    a.counters = b->d_cnt.get<uint64_t>();
    a.lds_pad = b->lds_pad;
    return a;
}
// rounds = ceil(n_systems / R); a launch lasts rounds x steps, so it gets 256 / (rounds x kBatchLaunchScale) steps, at least one
static uint32_t batch_rounds(const rpt_particles_batch* b) { return uint32_t((b->table.size() + b->resident - 1) / b->resident); }
static uint32_t batch_launch_steps(const rpt_particles_batch* b) {
    const uint32_t l = rptp::kMaxLaunchSteps / (batch_rounds(b) * kBatchLaunchScale);
    return l < 1 ? 1 : l;
}
static int settle(rpt_particles_batch* b) {
    RPTI_HIP_TRY(hipSetDevice(b->device));
    if (b->used) RPTI_HIP_TRY(hipEventSynchronize(b->done.get()));
    return RPT_OK;
}

extern "C" {
rpt_particles_batch* rpt_particles_batch_create(int device, const rpt_particles_params* params, uint32_t n_systems) {
    if (!params) { fail(RPT_ERR_INVALID, "null particle parameters"); return nullptr; }
    if (n_systems < 1 || n_systems > kBatchMaxSystems) { fail(RPT_ERR_INVALID, "the number of systems must be 1..4096"); return nullptr; }
    for (uint32_t s = 0; s < n_systems; s++)
        if (check_params(params + s) != RPT_OK) {
            fail(RPT_ERR_INVALID, "system " + std::to_string(s) + ": " + rpt_last_error());
            return nullptr;
        }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) { fail(RPT_ERR_INVALID, "device index out of range"); return nullptr; }
    if (!launch_particles_batch_integrate || !particles_batch_resident_blocks) { fail(RPT_ERR_UNSUPPORTED, "rpt_particles_batch_create: built without the kernels"); return nullptr; }
    auto* b = new rpt_particles_batch();
    b->device = device;
    b->table.resize(n_systems);
    std::vector<uint32_t> first(n_systems);
    for (uint32_t s = 0; s < n_systems; s++) {
        b->table[s] = ParticlesSystemRecord{params[s].kind, params[s].n, b->total, 0u, params[s].radius, params[s].height};
        first[s] = b->total;
        b->total += params[s].n;
        if (params[s].n > b->n_max) b->n_max = params[s].n;
        if (params[s].kind != RPT_PARTICLES_MARBLES) b->all_marbles = false;
    }
    if (const char* tune = std::getenv("RPT_PARTICLES_TUNE")) {
        unsigned bl = 0, l = 0, pad = 0;
        if (std::sscanf(tune, "%u,%u,%u", &bl, &l, &pad) >= 2 && (bl == 256 || bl == 512 || bl == 1024) && (l == 8 || l == 16 || l == 32 || l == 64)) {
            b->block = bl;
            b->lanes = l;
            b->lds_pad = (pad + 15u) & ~15u;
            if (b->lds_pad > kBatchMaxLds || particles_batch_lds(b->n_max).bytes + b->lds_pad > kBatchMaxLds) b->lds_pad = 0;
        }
    }
    const size_t bytes = size_t(b->total) * 3 * sizeof(double), cnt_bytes = size_t(n_systems) * 8 * sizeof(uint64_t);
    const size_t table_bytes = size_t(n_systems) * sizeof(ParticlesSystemRecord), first_bytes = size_t(n_systems) * sizeof(uint32_t);
    const bool ok = hipSetDevice(device) == hipSuccess && b->d_pos.reserve(bytes) == hipSuccess && b->d_vel.reserve(bytes) == hipSuccess &&
                    b->d_disp.reserve(bytes) == hipSuccess && b->d_cnt.reserve(cnt_bytes) == hipSuccess && b->d_table.reserve(table_bytes) == hipSuccess &&
                    b->d_first.reserve(first_bytes) == hipSuccess && hipMemset(b->d_pos.get(), 0, bytes) == hipSuccess &&
                    hipMemset(b->d_vel.get(), 0, bytes) == hipSuccess && hipMemset(b->d_cnt.get(), 0, cnt_bytes) == hipSuccess &&
                    hipMemcpy(b->d_table.get(), b->table.data(), table_bytes, hipMemcpyHostToDevice) == hipSuccess &&
                    hipMemcpy(b->d_first.get(), first.data(), first_bytes, hipMemcpyHostToDevice) == hipSuccess &&
                    b->done.create(hipEventDisableTiming) == hipSuccess;
    if (!ok) {
        fail(RPT_ERR_DEVICE, "rpt_particles_batch_create: device allocation failed");
        rpt_particles_batch_destroy(b);
        return nullptr;
    }
    if (particles_batch_resident_blocks(device, b->block, b->lanes, b->n_max, b->lds_pad, &b->resident) != hipSuccess || b->resident < 1) {
        fail(RPT_ERR_DEVICE, "rpt_particles_batch_create: the occupancy query failed");
        rpt_particles_batch_destroy(b);
        return nullptr;
    }
    return b;
}
void rpt_particles_batch_destroy(rpt_particles_batch* b) {
    if (!b) return;
    (void)hipSetDevice(b->device);
    delete b;
}
int rpt_particles_batch_set_state(rpt_particles_batch* b, const double* pos, const double* vel) {
    if (!pos) return fail(RPT_ERR_INVALID, "null positions");
    if (!b) return fail(RPT_ERR_INVALID, "null particle ensemble");
    if (int rc = settle(b)) return rc;
    const size_t bytes = size_t(b->total) * 3 * sizeof(double);
    RPTI_HIP_TRY(hipMemcpy(b->d_pos.get(), pos, bytes, hipMemcpyHostToDevice));
    if (vel)
        RPTI_HIP_TRY(hipMemcpy(b->d_vel.get(), vel, bytes, hipMemcpyHostToDevice));
    else
        RPTI_HIP_TRY(hipMemset(b->d_vel.get(), 0, bytes));
    return RPT_OK;
}
int rpt_particles_batch_set_system_state(rpt_particles_batch* b, uint32_t system, const double* pos, const double* vel) {
    if (!pos) return fail(RPT_ERR_INVALID, "null positions");
    if (!b) return fail(RPT_ERR_INVALID, "null particle ensemble");
    if (system >= b->table.size()) return fail(RPT_ERR_INVALID, "system index out of range");
    if (int rc = settle(b)) return rc;
    const ParticlesSystemRecord& r = b->table[system];
    const size_t bytes = size_t(r.n) * 3 * sizeof(double), at = size_t(r.first) * 3;
    RPTI_HIP_TRY(hipMemcpy(b->d_pos.get<double>() + at, pos, bytes, hipMemcpyHostToDevice));
    if (vel)
        RPTI_HIP_TRY(hipMemcpy(b->d_vel.get<double>() + at, vel, bytes, hipMemcpyHostToDevice));
    else
        RPTI_HIP_TRY(hipMemset(b->d_vel.get<double>() + at, 0, bytes));
    return RPT_OK;
}
int rpt_particles_batch_state(rpt_particles_batch* b, double* pos, double* vel) {
    if (!pos && !vel) return fail(RPT_ERR_INVALID, "null outputs");
    if (!b) return fail(RPT_ERR_INVALID, "null particle ensemble");
    if (int rc = settle(b)) return rc;
    const size_t bytes = size_t(b->total) * 3 * sizeof(double);
    if (pos) RPTI_HIP_TRY(hipMemcpy(pos, b->d_pos.get(), bytes, hipMemcpyDeviceToHost));
    if (vel) RPTI_HIP_TRY(hipMemcpy(vel, b->d_vel.get(), bytes, hipMemcpyDeviceToHost));
    return RPT_OK;
}
int rpt_particles_batch_state_device(rpt_particles_batch* b, void** d_pos, void** d_vel, void** d_first) {
    if (!d_pos && !d_vel && !d_first) return fail(RPT_ERR_INVALID, "null outputs");
    if (!b) return fail(RPT_ERR_INVALID, "null particle ensemble");
    if (d_pos) *d_pos = b->d_pos.get();
    if (d_vel) *d_vel = b->d_vel.get();
    if (d_first) *d_first = b->d_first.get();
    return RPT_OK;
}
int rpt_particles_batch_integrate(rpt_particles_batch* b, double time, double step, void* hip_stream) {
    uint64_t n_full = 0;
    double last = 0.0;
    if (int rc = check_time(time, step, &n_full, &last)) return rc;
    if (!b) return fail(RPT_ERR_INVALID, "null particle ensemble");
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    RPTI_HIP_TRY(hipSetDevice(b->device));
    if (b->used) RPTI_HIP_TRY(hipStreamWaitEvent(st, b->done.get(), 0));
    b->used = true;
    ParticlesBatchArgs a = batch_args(b);
    a.h = step;
    a.h_tail = last;
    // the same step sequence as the single handle's, in launches of L steps: only the last launch carries the tail step
    const uint32_t L = batch_launch_steps(b);
    hipError_t e = hipSuccess;
    for (uint64_t left = n_full + 1; left > 0 && e == hipSuccess;) {
        const uint32_t m = uint32_t(left < L ? left : L);
        a.n_steps = m;
        a.tail = left == m ? 1u : 0u;
        e = launch_particles_batch_integrate(a, b->block, b->lanes, st);
        if (e == hipSuccess) b->launches++;
        left -= m;
    }
    const hipError_t er = hipEventRecord(b->done.get(), st);   // (after a failed launch too, as rpt_particles_integrate)
    RPTI_HIP_TRY(e);
    RPTI_HIP_TRY(er);
    return RPT_OK;
}
int rpt_particles_batch_display_positions(rpt_particles_batch* b, double* out) {
    if (!out) return fail(RPT_ERR_INVALID, "null output");
    if (!b) return fail(RPT_ERR_INVALID, "null particle ensemble");
    if (!b->all_marbles) return fail(RPT_ERR_UNSUPPORTED, "display positions are defined for marbles systems only");
    if (!launch_particles_batch_display) return fail(RPT_ERR_UNSUPPORTED, "rpt_particles_batch_display_positions: built without the kernels");
    if (int rc = settle(b)) return rc;
    RPTI_HIP_TRY(launch_particles_batch_display(batch_args(b), b->d_disp.get<double>(), nullptr));
    b->launches++;
    RPTI_HIP_TRY(hipMemcpy(out, b->d_disp.get(), size_t(b->total) * 3 * sizeof(double), hipMemcpyDeviceToHost));
    return RPT_OK;
}
int rpt_particles_batch_display_positions_device(rpt_particles_batch* b, void** d_out, void* hip_stream) {
    if (!d_out) return fail(RPT_ERR_INVALID, "null output");
    if (!b) return fail(RPT_ERR_INVALID, "null particle ensemble");
    if (!b->all_marbles) return fail(RPT_ERR_UNSUPPORTED, "display positions are defined for marbles systems only");
    if (!launch_particles_batch_display) return fail(RPT_ERR_UNSUPPORTED, "rpt_particles_batch_display_positions_device: built without the kernels");
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    RPTI_HIP_TRY(hipSetDevice(b->device));
    if (b->used) RPTI_HIP_TRY(hipStreamWaitEvent(st, b->done.get(), 0));
    b->used = true;
    const hipError_t e = launch_particles_batch_display(batch_args(b), b->d_disp.get<double>(), st);
    if (e == hipSuccess) b->launches++;
    const hipError_t er = hipEventRecord(b->done.get(), st);
    RPTI_HIP_TRY(e);
    RPTI_HIP_TRY(er);
    *d_out = b->d_disp.get();
    return RPT_OK;
}
int rpt_particles_batch_counters(rpt_particles_batch* b, uint64_t* out) {
    if (!out) return fail(RPT_ERR_INVALID, "null output");
    if (!b) return fail(RPT_ERR_INVALID, "null particle ensemble");
    if (int rc = settle(b)) return rc;
    RPTI_HIP_TRY(hipMemcpy(out, b->d_cnt.get(), b->table.size() * 8 * sizeof(uint64_t), hipMemcpyDeviceToHost));
    for (size_t s = 0; s < b->table.size(); s++) {
        out[8 * s + 6] = b->launches;
        out[8 * s + 7] = 0;
    }
    return RPT_OK;
}
int rpt_particles_batch_info(rpt_particles_batch* b, uint64_t out[8]) {
    if (!out) return fail(RPT_ERR_INVALID, "null output");
    if (!b) return fail(RPT_ERR_INVALID, "null particle ensemble");
    out[0] = b->resident;
    out[1] = batch_rounds(b);
    out[2] = batch_launch_steps(b);
    out[3] = particles_batch_lds(b->n_max).bytes + b->lds_pad;
    out[4] = b->n_max;
    out[5] = b->total;
    out[6] = b->block;
    out[7] = b->lanes;
    return RPT_OK;
}

// ---- pure host functions: no device is touched
int rpt_monomial_closest_point(double height, const double p[3], int precise, double out[3]) {
    if (!p || !out) return fail(RPT_ERR_INVALID, "null argument");
    if (!std::isfinite(height)) return fail(RPT_ERR_INVALID, "height must be finite");
    const double P[3] = {p[0], p[1], p[2]};
    rptp::closest_point(height, P, precise ? rptp::kPreciseN : rptp::kCoarseN, out);
    return RPT_OK;
}
int rpt_particles_derivative_host(const rpt_particles_params* prm, const double* pos, const double* vel, double* dpos, double* dvel, uint64_t counters[8]) {
    if (int rc = check_params(prm)) return rc;
    if (!pos || !vel || !dpos || !dvel) return fail(RPT_ERR_INVALID, "null state");
    uint64_t cnt[6] = {0, 0, 0, 0, 0, 0};
    const size_t m = size_t(prm->n) * 3;
    std::vector<double> p(pos, pos + m), v(vel, vel + m);   // (the outputs may be the inputs)
    rptp::derivative(prm->kind, prm->n, prm->radius, prm->height, p.data(), v.data(), dpos, dvel, cnt);
    if (counters) {
        for (int k = 0; k < 6; k++) counters[k] = cnt[k];
        counters[6] = counters[7] = 0;
    }
    return RPT_OK;
}
int rpt_particles_integrate_host(const rpt_particles_params* prm, double* pos, double* vel, double time, double step, uint64_t counters[8]) {
    if (int rc = check_params(prm)) return rc;
    uint64_t n_full = 0;
    double last = 0.0;
    if (int rc = check_time(time, step, &n_full, &last)) return rc;
    if (!pos || !vel) return fail(RPT_ERR_INVALID, "null state");
    const size_t m = size_t(prm->n) * 3;
    std::vector<double> x(2 * m), k(2 * m), sum(2 * m);
    uint64_t cnt[6] = {0, 0, 0, 0, 0, 0};
    for (uint64_t s = 0; s <= n_full; s++) {
        const double h = s == n_full ? last : step;
        const double hh = h / 2.0;
        for (int stage = 1; stage <= 4; stage++) {
            const double f = stage == 4 ? h : hh;
            for (size_t i = 0; i < m; i++) {
                x[i] = stage == 1 ? pos[i] : rptp::rk4_stage(pos[i], k[i], f);
                x[m + i] = stage == 1 ? vel[i] : rptp::rk4_stage(vel[i], k[m + i], f);
            }
            rptp::derivative(prm->kind, prm->n, prm->radius, prm->height, x.data(), x.data() + m, k.data(), k.data() + m, cnt);
            for (size_t i = 0; i < 2 * m; i++) sum[i] = rptp::rk4_sum(sum[i], k[i], stage);
        }
        for (size_t i = 0; i < m; i++) {
            pos[i] = rptp::rk4_new(pos[i], sum[i], h);
            vel[i] = rptp::rk4_new(vel[i], sum[m + i], h);
        }
    }
    if (counters) {
        for (int i = 0; i < 6; i++) counters[i] = cnt[i];
        counters[6] = counters[7] = 0;
    }
    return RPT_OK;
}
int rpt_particles_display_positions_host(const rpt_particles_params* prm, const double* pos, double* out) {
    if (int rc = check_params(prm)) return rc;
    if (!pos || !out) return fail(RPT_ERR_INVALID, "null argument");
    if (prm->kind != RPT_PARTICLES_MARBLES) return fail(RPT_ERR_UNSUPPORTED, "display positions are defined for a marbles system only");
    for (uint32_t p = 0; p < prm->n; p++) {
        const double P[3] = {pos[3 * p], pos[3 * p + 1], pos[3 * p + 2]};
        double C[3];
        rptp::closest_point(prm->height, P, rptp::kPreciseN, C);
        rptp::display_position(prm->radius, P, C, out + 3 * p);
    }
    return RPT_OK;
}
}  // extern "C"
