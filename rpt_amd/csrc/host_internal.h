// host_internal.h — internals of rpt_capi.cpp shared with the photon-mapping translation unit.
#pragma once
#include <hip/hip_runtime_api.h>

#include <functional>
#include <string>
#include <utility>
#include <vector>

#include "../../include/rpt_hip.h"
#include "kernels.h"

namespace rpt64 { struct Args; struct Camera; }

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
bool scan_jit_cache_read(const std::string& path, std::vector<char>* code, std::string* lowered, std::string* why);
bool scan_jit_cache_write(const std::string& dir, const std::string& path, const std::vector<char>& code, const std::string& lowered);
// A scene's state of it (rpt_scan_jit_info).
struct ScanJit {
    int state = 1, cache = 0;   // RPT_SCAN_JIT_IDLE, RPT_SCAN_JIT_CACHE_NONE
    bool probed = false;
    ScanShape shape{};
    std::string shape_text, reason, key, compiler;
    std::vector<std::pair<std::string, std::string>> sources;
    double compile_ms = 0;
    int vgprs = 0, scratch = 0, aot_vgprs = 0;
    size_t lds = 0;
    hipFunction_t fn = nullptr;
    uint64_t launches = 0;
};
uint64_t seed_mix(uint64_t seed);
struct SceneDev {
    bool committed;
    int device, n_cus;
    rptg::SceneView view;
    int first_object_light;  // index into scene.lights of the first Light::Object, or -1
    bool epsilon64;          // committed in the reference-epsilon mode (epsilon_policy = 1)
    bool has_monomial;       // some object is (or holds) a MonomialSurface: photon mapping refuses such scenes
};
SceneDev scene_dev(rpt_scene* s);
void fill_camera64(const rpt_camera* cam, rpt64::Camera& q);   // the reference-epsilon mode's camera record (renders and rpt_debug_camera_sample_f64)
int light_kind(rpt_scene* s, uint32_t light);   // kind of scene.lights[light] (0 point, 1 ambient, 2 directional, 3 object), -1: no such light
void*& photon_slot(rpt_scene* s);  // owned by photon.hip (PhotonMapDev*), released through photon_release
void photon_release(void* p);      // defined in photon.hip
// Fills camera, tiles, slab, queue, chunking exactly as for the path tracer; `st` is the stream the launch will run
// on (it selects the launch set: slab + work counter).
// min_chunk: lower bound of the automatic samples-per-work-item choice (an explicit "chunk_spp" option wins).
// fixed_chunk != 0: the caller's kernel has its own work decomposition with exactly that many samples per chunk
// (the photon camera pass: 64); option and automatic rule are ignored, so the slab [n_chunks][n_owned] this
// function sizes is the one that kernel and resolve_kernel index.
int prepare_render(rpt_scene* s, hipStream_t st, const rpt_camera* cam, const rpt_render_params* prm, uint32_t iterations, uint64_t seed,
                   uint32_t sample_offset, rptg::RenderArgs& a, uint32_t min_chunk = 0, uint32_t fixed_chunk = 0,
                   uint32_t slab_item_bytes = 16,   // 32: the reference-epsilon mode's partial sums are fp64
                   bool launch_set = true);   // false: the caller brings its own scratch (the feature pass): no launch set is taken, a.slab and a.queue stay null
// Zeroes the queue / sharded frame, calls `launch(args, n_blocks, stream)` with a persistent grid of
// blocks_per_cu blocks per CU, then resolves the slab into d_out.
int run_persistent(rpt_scene* s, const rpt_render_params* prm, const rptg::RenderArgs& a, double* d_out, hipStream_t st,
                   int blocks_per_cu, const std::function<hipError_t(const rptg::RenderArgs&, int, hipStream_t)>& launch,
                   bool indexed_start = false, bool wave_items = false,   // wave_items: n_items counts one item per wave, not per lane
                   const std::function<hipError_t(double, double*, hipStream_t)>& resolve = nullptr,   // (scale, d_out, stream): instead of resolve_kernel
                   bool clear_sharded = true);   // false: a sharded frame keeps what is in d_out (a resolve that adds to the earlier slices of the same frame)
int serialize_with_other_streams(rpt_scene* s, hipStream_t st);  // for launches with per-scene scratch outside the launch set
int fetch_counters(rpt_scene* s, const rptg::RenderArgs& a);  // after the stream has been synchronised
// Arguments the fp64 kernels share (rpt_capi.cpp): scene; camera, frame and `a`'s tiles / chunking / work counter / slab when given.
void fill_args64(rpt_scene* s, const rpt_camera* cam, const rpt_render_params* prm, const rptg::RenderArgs* a, rpt64::Args& q);
double* scratch_out(rpt_scene* s, size_t bytes);  // cached device frame for the host-buffer entry points
int64_t option_photon_skip(rpt_scene* s);  // option "photon_skip" of the scene: diagnostic bit mask for the camera pass
int64_t option_max_blocks(rpt_scene* s);          // option "max_blocks": cap on the blocks of a persistent launch (0: none)
int64_t option_f64_photon_slice(rpt_scene* s);    // option "f64_photon_slice": samples per slice of the reference-epsilon photon camera pass (0: automatic)
int64_t option_photon_parts(rpt_scene* s);        // option "photon_parts": strips per 8x8 pixel block of the camera pass (1, 2, 4, 8)
int64_t option_photon_coop_gather(rpt_scene* s);  // option "photon_coop_gather": wave-level surface gather on (default) / off
int64_t option_photon_split(rpt_scene* s);        // option "photon_split": volume and surface estimate of the beam kinds in two launches (default off: measured slower)
int64_t option_photon_block_lists(rpt_scene* s);  // option "photon_block_lists": per-block candidate lists on (default) / off
}  // namespace rpti

#define RPTI_HIP_TRY(expr)                                                                          \
    do {                                                                                            \
        hipError_t e__ = (expr);                                                                    \
        if (e__ != hipSuccess)                                                                      \
            return rpti::fail(RPT_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e__));  \
    } while (0)
