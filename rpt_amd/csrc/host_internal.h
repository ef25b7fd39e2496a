// host_internal.h — what the host sources share with rpt_comm.cpp and the host test harnesses: the owners of device memory and
// events, the error store and the scan JIT's declarations.  (rpt_scene and the functions that take one: scene_host.h.)
#pragma once
#include <hip/hip_runtime_api.h>

#include <functional>
#include <string>
#include <utility>
#include <vector>

#include "../../include/rpt_hip.h"
#include "kernels.h"

namespace rpti {
// One hipMalloc block and its byte capacity, freed when the owner is reset, reassigned or destroyed.  hipFree runs on the
// device that is current then: whoever destroys an owner of another device's memory sets that device first.
class DevMem {
  public:
    DevMem() = default;
    DevMem(DevMem&& o) noexcept : p_(std::exchange(o.p_, nullptr)), cap_(std::exchange(o.cap_, 0)) {}
    DevMem& operator=(DevMem&& o) noexcept {
        if (this != &o) {
            reset();
            p_ = std::exchange(o.p_, nullptr);
            cap_ = std::exchange(o.cap_, 0);
        }
        return *this;
    }
    ~DevMem() { reset(); }
    // Grow-only.  The old block is freed before the new one is allocated (peak memory stays one block), so a failure
    // leaves an empty owner, never a capacity without memory behind it.
    hipError_t reserve(size_t bytes) {
        if (bytes <= cap_) return hipSuccess;
        hipError_t e = p_ ? hipFree(p_) : hipSuccess;
        p_ = nullptr;
        cap_ = 0;
        if (e == hipSuccess) e = hipMalloc(&p_, bytes);
        if (e != hipSuccess) { p_ = nullptr; return e; }
        cap_ = bytes;
        return hipSuccess;
    }
    void reset() {
        if (p_) (void)hipFree(p_);
        p_ = nullptr;
        cap_ = 0;
    }
    template <class T = void>
    T* get() const { return static_cast<T*>(p_); }
    size_t capacity() const { return cap_; }
    explicit operator bool() const { return p_ != nullptr; }

  private:
    void* p_ = nullptr;
    size_t cap_ = 0;
};
// One hipEvent_t, destroyed with its owner (on the device that is current then, as for DevMem).
class Event {
  public:
    Event() = default;
    Event(Event&& o) noexcept : e_(std::exchange(o.e_, nullptr)) {}
    Event& operator=(Event&& o) noexcept {
        if (this != &o) {
            reset();
            e_ = std::exchange(o.e_, nullptr);
        }
        return *this;
    }
    ~Event() { reset(); }
    hipError_t create(unsigned flags = hipEventDefault) {
        reset();
        hipError_t e = hipEventCreateWithFlags(&e_, flags);
        if (e != hipSuccess) e_ = nullptr;
        return e;
    }
    void reset() {
        if (e_) (void)hipEventDestroy(e_);
        e_ = nullptr;
    }
    hipEvent_t get() const { return e_; }

  private:
    hipEvent_t e_ = nullptr;
};
// Milliseconds between two recorded events (0 if the runtime cannot tell).
inline float elapsed_ms(const Event& a, const Event& b) {
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, a.get(), b.get());
    return ms;
}

int fail(int code, const std::string& msg);
// What the scans of a committed scene know before they read a record (device_core.h, ScanShapeK), and which of the two scan kernels
// runs them.  Two scenes with the same shape share one specialised code object; record values are not part of it.
struct ScanShape {
    uint32_t n_sph, n_cub, n_pln, n_aabb, n_rect_x, n_rect_y, n_rect_z, n_tri, has_shell, scan_cull, medium;
    uint64_t sph_yrot, cub_yrot;
};
bool scan_shape_of(const rptg::SceneView& v, ScanShape* out, std::string* why);   // false: a flavour outside the scope (tree, group light, monomial surface)
std::string scan_shape_string(const ScanShape& h);
std::string scan_jit_program(const ScanShape& h);        // the program text: the shape block and #include "kernels.hip"
std::string scan_jit_kernel_name(const ScanShape& h);    // the name expression of the one instantiation it emits
const std::vector<std::string>& scan_jit_options();
bool scan_jit_sources(const std::string& dir, std::vector<std::pair<std::string, std::string>>* out, std::string* why);
std::string scan_jit_key(const std::string& program, const std::vector<std::pair<std::string, std::string>>& sources,
                         const std::vector<std::string>& options, int rtc_major, int rtc_minor);
bool scan_jit_compile(const ScanShape& shape, const std::vector<std::pair<std::string, std::string>>& sources, std::vector<char>* code,
                      std::string* lowered, double* ms, std::string* why);
bool scan_jit_resources(const std::vector<char>& code, int* vgprs, int* scratch);
// What the code around the scans knows beforehand (device_core.h, SceneStructK): the second constant block of the program.  `groups`: the
// SS_* bits of the groups of constants in effect; the fields of a group that is not are zero, so that scenes which differ only there
// share a code object.  Filled at commit from the records as they are uploaded; record values are not part of it.
struct SceneStruct {
    uint32_t groups, n_lights;
    uint32_t light[4], twin_lo[4], twin_hi[4];   // light word (bits 0-1 kind, 2-3 shape, 4 has a transform, 5 has a twin, 6 the twin is a code range)
    uint32_t mats;                                // bit k: some object's material is of kind k
    uint32_t medium_kind, hdri;
    uint64_t pairs;                               // three common-slab bits per pair of boxes, pair 0 lowest
};
uint32_t scan_struct_default_groups();   // the groups a commit takes: the default, or RPT_SCAN_STRUCT_GROUPS (a mask; measurements)
SceneStruct scan_struct_of(uint32_t groups, const std::vector<rptg::Light>& lights, const std::vector<rptg::LightXf>& lxf, size_t n_ltris,
                           const std::vector<rptg::Material>& mats, const std::vector<rptg::AabbScan>& aabb, uint32_t medium_kind, bool hdri);
std::string scan_struct_string(const SceneStruct& t);   // "groups=<names>;lights=...;mats=...;medium_kind=..;hdri=..;pairs=..": what rpt_scan_jit_structure reports
std::string scan_jit_program(const ScanShape& h, const SceneStruct& t);   // the shape block, the structure block, #include "kernels.hip" and the instantiation's name
bool scan_jit_compile(const ScanShape& shape, const SceneStruct* structure, const std::vector<std::pair<std::string, std::string>>& sources,
                      std::vector<char>* code, std::string* lowered, double* ms, std::string* why);
bool scan_jit_cache_read(const std::string& path, std::vector<char>* code, std::string* lowered, std::string* why);
bool scan_jit_cache_write(const std::string& dir, const std::string& path, const std::vector<char>& code, const std::string& lowered);
// A scene's state of it (rpt_scan_jit_info).
struct ScanJit {
    int state = 1, cache = 0;   // RPT_SCAN_JIT_IDLE, RPT_SCAN_JIT_CACHE_NONE
    bool probed = false;
    ScanShape shape{};
    SceneStruct structure{};   // set by the commit
    std::string shape_text, reason, key, compiler;
    std::vector<std::pair<std::string, std::string>> sources;
    double compile_ms = 0;
    int vgprs = 0, scratch = 0, aot_vgprs = 0;
    size_t lds = 0;
    hipFunction_t fn = nullptr;
    uint64_t launches = 0;
};
uint64_t seed_mix(uint64_t seed);
}  // namespace rpti

#define RPTI_HIP_TRY(expr)                                                                          \
    do {                                                                                            \
        hipError_t e__ = (expr);                                                                    \
        if (e__ != hipSuccess)                                                                      \
            return rpti::fail(RPT_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e__));  \
    } while (0)
