// kernels.h — host-callable launchers of the HIP kernels (implemented in kernels.hip).
#pragma once
#ifndef __HIPCC_RTC__
#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <stdint.h>
#endif
#include "gpu_layout.h"

namespace rptg {

struct RenderArgs {
    SceneView sc;
    CameraG cam;
    uint32_t width, height;
    float inv_dim;            // 1 / max(width, height)
    uint32_t max_bounces;
    uint32_t iterations;      // paths per pixel in this call
    uint32_t sample_offset;
    uint32_t chunk_spp;       // samples per work item
    uint32_t n_chunks;        // ceil(iterations / chunk_spp)
    uint64_t seed_mixed;      // mix64(seed + GOLDEN)
    const uint32_t* tiles;    // owned 32x32 tiles (tile id = ty * tiles_x + tx)
    uint32_t n_tiles, tiles_x;
    uint32_t n_owned;         // n_tiles * 1024 pixel slots
    uint32_t n_items;         // n_owned * n_chunks
    float* slab;              // [n_chunks][n_owned] float4 partial sums
    float* slab2;             // a second term per (chunk, pixel) that resolve_kernel adds (the split photon camera pass), or null
    unsigned long long* queue;  // 64-bit work counter (zeroed before the launch)
    unsigned long long* counters;  // 8 x u64 or nullptr
    uint32_t lds_stack;       // 1: BVH stack in dynamic LDS
    uint32_t defer_lanes;     // per-mesh-tree kernels: parked tree walks per wave that trigger a walk (1..64)
    uint32_t defer_stop;      // ... and the number of still-walking lanes below which the wave leaves the walk
    uint32_t walk_leaf_quarters;  // ... and the descent of a walk pauses for the leaves when 4 x (lanes at a leaf) >= this x (lanes descending); 0: never
    uint32_t detach;              // per-mesh-tree kernels in a medium: 1 = shadow queries that need a tree walk leave their path (wave queue
                                  // in LDS); 2 = every tree walk leaves its path (ring + parked path contexts in stream_scratch)
    uint32_t pull_batch;          // lanes that must wait for a new work item before the wave runs the item bookkeeping (it also runs when no lane has anything else to do)
    uint32_t detach_trigger;      // detach = 1: a walk session is due as soon as the queue holds this many (1..32)
    uint32_t stream_backlog;      // detach = 2: ... as soon as the ring holds this many queries
    uint32_t stream_contexts;     // detach = 2: parked paths per lane (1..6)
    uint32_t n_twin_lights;       // object lights that can be visible (each may write one shadow query per lane and trip)
    uint32_t* stream_scratch;     // detach = 2: stream_scratch_bytes_per_block() per block of the grid
};

// The device functions read the scene view at kernarg + 0 (kernarg_scene in device_core.h): every kernel that calls them
// takes ONE argument struct that begins with the SceneView.
static_assert(__builtin_offsetof(RenderArgs, sc) == 0, "RenderArgs must begin with the SceneView");

#ifndef __HIPCC_RTC__   // (runtime compilation takes the argument struct alone)

struct KernelInfo {
    int vgprs, sgprs, lds, max_blocks_per_cu;
};

// Persistent megakernel: grid = n_blocks x 256 threads.
hipError_t launch_render(const RenderArgs& a, int n_blocks, hipStream_t stream);
hipError_t render_occupancy(bool medium, int bvh, int* blocks_per_cu, int detach = 0);  // bvh: bvh_mode(); detach: RenderArgs::detach
size_t stream_scratch_bytes_per_block();
// Registers, scratch bytes per lane and dynamic LDS of the AOT scan kernel render_kernel<medium, 0, false>: what a specialised twin
// (rpt_capi.cpp, scan JIT) is launched with and must not exceed.  (Weak: the host-only test builds have no kernels.)
__attribute__((weak)) hipError_t scan_render_info(bool medium, int* vgprs, int* scratch, size_t* lds);
int bvh_mode(const SceneView& sc);  // 0 no tree, 1 per-mesh trees, 2 scene-level tree
// out[pixel] = sum_chunks slab / iterations * scale for owned pixels (others untouched).
hipError_t launch_buffer_add(uint32_t n_pixels, const double* d_batch, double* d_sum, double* d_sumsq, hipStream_t st);
hipError_t launch_buffer_image(uint32_t w, uint32_t h, uint32_t radius, uint32_t n_batches, const double* d_sum, uint8_t* d_out,
                               hipStream_t st);
hipError_t launch_buffer_variance(uint32_t n_pixels, uint32_t n_batches, const double* d_sum, const double* d_sumsq, double* d_out,
                                  hipStream_t st);
hipError_t launch_resolve(const RenderArgs& a, double scale, double* d_out, hipStream_t stream);
// Frame exchange: owned tiles <-> packed blocks of 32 x 32 x 3 f64 (tile list on the device).
hipError_t launch_frame_pack(const double* d_frame, double* d_packed, const uint32_t* d_tiles, uint32_t n_tiles, uint32_t tiles_x,
                             uint32_t width, uint32_t height, hipStream_t st);
hipError_t launch_frame_unpack(const double* d_packed, double* d_frame, const uint32_t* d_tiles, uint32_t n_tiles, uint32_t tiles_x,
                               uint32_t width, uint32_t height, hipStream_t st);
// (Weak: the host-only test harnesses link rpt_capi.cpp against stubs of the launchers they know; this one is reached from
// rpt_intersect_segments alone, which reports RPT_ERR_UNSUPPORTED where no kernel library is linked.)
__attribute__((weak)) hipError_t launch_intersect_segments(const SceneView& sc, uint64_t n, const float* d_o, const float* d_d, const float* d_tmax,
                                                           float* d_t, uint32_t* d_code, hipStream_t stream);
hipError_t launch_intersect(const SceneView& sc, uint64_t n, const float* d_o, const float* d_d, float* d_t,
                            int32_t* d_obj, float* d_n, bool bvh, hipStream_t stream);
// rpt_render_features*: the first-hit feature pass.  One lane per (pixel slot, chunk) item of RenderArgs' decomposition (no work
// counter: a plain grid); the lane sums its chunk's samples in fp64 and writes one record, feature_resolve_kernel adds a pixel's
// records in chunk order, divides by the sample count and writes the requested planes.  (r.slab, r.queue and r.counters are unused.)
struct FeatureArgs {
    RenderArgs r;
    double* slab;             // [8][n_items]: channel k of item i at [k * n_items + i] -- albedo rgb, normal xyz, depth, coverage
    uint32_t* ids;            // [n_owned]: object index + 1 of the call's sample 0 (written by the items of chunk 0), 0: a miss
};
static_assert(offsetof(FeatureArgs, r) == 0, "FeatureArgs must begin with the SceneView");
// The resolve of both modes (the reference-epsilon mode's feature kernel writes the same records).
struct FeatureResolveArgs {
    const uint32_t* tiles;
    uint32_t tiles_x, n_owned, n_chunks, n_items;
    uint32_t width, height, iterations, pad_;
    const double* slab;
    const uint32_t* ids;
    double *albedo, *normal, *depth;   // [width * height * 3] each, or null: not requested
};
// (Weak: reached from rpt_render_features* alone, which report RPT_ERR_UNSUPPORTED where no kernel library is linked.)
__attribute__((weak)) hipError_t launch_features(const FeatureArgs& a, hipStream_t stream);
__attribute__((weak)) hipError_t launch_feature_resolve(const FeatureResolveArgs& a, hipStream_t stream);
// rpt_denoise* (denoise.hip): the a-trous filter of include/rpt_hip.h.  Plain grids, one lane per pixel.  The prepare kernel writes one
// record of 8 doubles per pixel (c rgb = rgb / den, v, n xyz, z) and the id beside it; a pass reads records and ids and writes the
// next records, or -- the last one, `out` set -- the remodulated frame and, if asked, the filtered variance.
struct DenoisePrepareArgs {
    uint32_t n_pixels, flags;                            // RPT_DENOISE_* (DEMODULATE needs albedo)
    const double *rgb, *var, *albedo, *normal, *depth;   // var, albedo, normal, depth: or null
    double* rec;                                         // [n_pixels][8]
    double* ids;                                         // [n_pixels]
};
struct DenoisePassArgs {
    uint32_t width, height, step, flags;
    uint32_t terms, pad_;                                // bit 0 colour, 1 normal, 2 depth
    double sigma_color2, a_n, a_z;                       // sigma_color * sigma_color, 1 / sigma_normal, 1 / (sigma_depth * double(step))
    const double* rec_in;
    const double* ids;
    const double* albedo;                                // den of the pixel itself (flag DEMODULATE), else unused
    double* rec_out;                                     // every pass but the last
    double *out, *out_var;                               // the last pass (out_var: or null)
};
// (Weak: reached from rpt_denoise* and rpt_buffer_mean_device / rpt_buffer_denoised_image alone, which report RPT_ERR_UNSUPPORTED
// where no kernel library is linked.)
__attribute__((weak)) hipError_t launch_denoise_prepare(const DenoisePrepareArgs& a, hipStream_t stream);
__attribute__((weak)) hipError_t launch_denoise_pass(const DenoisePassArgs& a, bool staged /* tile + halo in LDS */, hipStream_t stream);
static constexpr uint32_t kDenoiseMaxStagedStep = 2;   // the largest step whose tile + halo the staged form holds (option "denoise_stage")
__attribute__((weak)) hipError_t launch_buffer_mean(uint32_t n_pixels, uint32_t n_batches, const double* d_sum, const double* d_sumsq,
                                                    double* d_rgb, double* d_var /* or null */, hipStream_t st);
__attribute__((weak)) hipError_t launch_color_bytes(uint64_t n_values, const double* d_rgb, uint8_t* d_out, hipStream_t st);
// rpt_upsample* (upsample.hip): the guided upsampling of include/rpt_hip.h, one kernel, one lane per full-resolution pixel, the taps
// gathered from the low-resolution planes.  width x height is the LOW resolution; the outputs are scale times as large on each axis.
struct UpsampleArgs {
    uint32_t width, height, scale, radius;
    uint32_t flags, terms;                               // RPT_UPSAMPLE_*; bit 0 normal, 1 depth
    double a_n, a_z;                                     // 1 / sigma_normal, 1 / (sigma_depth * double(scale))
    const double *lo_rgb, *lo_var, *lo_albedo, *lo_normal, *lo_depth;   // all but lo_rgb: or null
    const double *hi_albedo, *hi_normal, *hi_depth;      // or null
    double *out_rgb, *out_var;                           // out_var: or null
};
// (Weak: reached from rpt_upsample* and rpt_buffer_upsampled_image alone, which report RPT_ERR_UNSUPPORTED where no kernel library is
// linked.)
__attribute__((weak)) hipError_t launch_upsample(const UpsampleArgs& a, hipStream_t stream);
// rpt_temporal_* (temporal.hip): the accumulation of include/rpt_hip.h, one kernel, one lane per pixel.  The history is one record of
// kTemporalRecDoubles doubles per pixel (c rgb, v, len, n xyz, z, id); a call reads the old records of its four taps and writes the new
// ones elsewhere.  The two camera records are rpt_temporal_camera_record's 13 doubles.
static constexpr uint32_t kTemporalRecDoubles = 10;
struct TemporalCam {
    double eye[3], dir[3], right[3], up[3], d;
};
struct TemporalArgs {
    uint32_t width, height, max_history, flags;          // RPT_TEMPORAL_MATCH_ID | RPT_TEMPORAL_CLIP
    uint32_t have_history, pad_;                         // 0: hist_in holds no frame (the first call, or the first after a reset)
    double depth_tol, normal_tol;                        // 0: the test is off
    TemporalCam cur, prev;                               // prev: the record stored with hist_in
    const double *rgb, *var, *normal, *depth;            // var, normal: or null
    const double* hist_in;                               // [n_pixels][kTemporalRecDoubles]
    double* hist_out;
    double *out_rgb, *out_var, *out_len;                 // out_var, out_len: or null
    const double* motion;                                // [n_motion][kTemporalMotionDoubles] motion records, or null: no table is set
    uint32_t n_motion, pad2_;                            // (with a table the launcher takes the kernel's second instantiation)
    // RPT_TEMPORAL_CLIP (flags): rpt_temporal_set_clip's settings; without the flag they are 0 and never read
    uint32_t clip_radius, clip_history;                  // 1..kTemporalClipMaxRadius; 0..4096, 0: a clipped pixel keeps its length
    double clip_gamma;
};
static constexpr uint32_t kTemporalClipMaxRadius = 3;    // the largest window radius whose halo the kernel's tile holds
static constexpr uint32_t kTemporalMotionDoubles = 24;   // RPT_TEMPORAL_MOTION_DOUBLES: A 3 x 4, G 3 x 3, three zeros
// (Weak: reached from rpt_temporal_accumulate* / rpt_temporal_frame_image alone, which report RPT_ERR_UNSUPPORTED where no kernel
// library is linked.)
__attribute__((weak)) hipError_t launch_temporal_accumulate(const TemporalArgs& a, hipStream_t stream);
// rpt_temporal_preview_device: steps 1 - 5 of the same kernel over the in-image pixels of the listed 32 x 32 tiles (d_tiles null: over
// the frame); hist_out is not written.  A list with no entries launches nothing; one longer than the frame's tiles is
// hipErrorInvalidValue.  (Weak, like the launcher above.)
__attribute__((weak)) hipError_t launch_temporal_preview(const TemporalArgs& a, const uint32_t* d_tiles, uint32_t n_tiles, hipStream_t stream);
// rpt_temporal_set_motion's table on its way to the device: `bytes` from host memory to d_table, enqueued on `stream` (the host
// array may be reused as soon as the call returns).  (Weak, like the launcher above.)
__attribute__((weak)) hipError_t launch_temporal_motion_upload(void* d_table, const double* records, size_t bytes, hipStream_t stream);
// Adaptive sampling by tile (adaptive.hip).  A buffer whose tiles have different batch counts: a pixel of tile t holds
// n_batches + extra[t] batches (extra null: no tile batch was ever added).
struct TileBufferView {
    uint32_t width, height, tiles_x, tiles_y;
    uint32_t n_batches, pad_;
    const uint32_t* extra;   // [tiles_x * tiles_y] or null
};
// (Weak: reached from rpt_buffer_add_samples_tiles_device, rpt_buffer_tile_errors_device, rpt_buffer_refine_tiles and the read-outs of a
// buffer with extra batches alone, which report RPT_ERR_UNSUPPORTED where no kernel library is linked.)
// buffer_add_kernel on the in-image pixels of the listed tiles (ids distinct; an id out of range is skipped), extra[id] += 1.
__attribute__((weak)) hipError_t launch_buffer_add_tiles(const TileBufferView& b, const double* d_batch, double* d_sum, double* d_sumsq,
                                                         uint32_t* d_extra, const uint32_t* d_tiles, uint32_t n_tiles, hipStream_t st);
__attribute__((weak)) hipError_t launch_buffer_image_tiles(const TileBufferView& b, uint32_t radius, const double* d_sum, uint8_t* d_out,
                                                           hipStream_t st);
__attribute__((weak)) hipError_t launch_buffer_variance_tiles(const TileBufferView& b, const double* d_sum, const double* d_sumsq, double* d_out,
                                                              hipStream_t st);
__attribute__((weak)) hipError_t launch_buffer_mean_tiles(const TileBufferView& b, const double* d_sum, const double* d_sumsq, double* d_rgb,
                                                          double* d_var /* or null */, hipStream_t st);
// err[t] for every tile (one block each); then the ids with err > threshold2 and fewer than max_batches batches, ascending, and their
// number (one block).
__attribute__((weak)) hipError_t launch_tile_errors(const TileBufferView& b, double floor, const double* d_sum, const double* d_sumsq,
                                                    double* d_err, hipStream_t st);
__attribute__((weak)) hipError_t launch_tile_select(const TileBufferView& b, double threshold2, uint32_t max_batches, const double* d_err,
                                                    uint32_t* d_tiles_out, uint32_t* d_n_out, hipStream_t st);
// rpt_temporal_tile_errors_device: err[t] of the listed tiles (d_tiles null: of every tile) with the pixel's terms from the planes
// rgb and var; an id out of range is skipped.  Then launch_tile_select among a list (d_tiles_in null: among every tile), the
// selected ids in the list's order; d_tiles_out may be d_tiles_in.  (Weak, like the two above.)
__attribute__((weak)) hipError_t launch_plane_tile_errors(uint32_t width, uint32_t height, double floor, const double* d_rgb, const double* d_var,
                                                          const uint32_t* d_tiles, uint32_t n_tiles, double* d_err, hipStream_t st);
__attribute__((weak)) hipError_t launch_tile_select_list(const TileBufferView& b, double threshold2, uint32_t max_batches, const double* d_err,
                                                         const uint32_t* d_tiles_in, uint32_t n_in, uint32_t* d_tiles_out, uint32_t* d_n_out,
                                                         hipStream_t st);
hipError_t launch_debug_rng(uint64_t seed_mixed, uint32_t pixel, uint32_t sample, uint32_t n, uint32_t* d_out,
                            hipStream_t stream);
hipError_t launch_debug_sample_f(const Material& m, uint64_t n, const float* d_n, const float* d_wo,
                                 uint64_t seed_mixed, float* d_wi, float* d_pdf, int32_t* d_some, hipStream_t s);
hipError_t launch_debug_bsdf(const Material& m, uint64_t n, const float* d_n, const float* d_wo, const float* d_wi,
                             float* d_out, hipStream_t s);
// rpt_debug_camera_rays / rpt_debug_camera_sample: the camera sample of a render, inv_dim as the host forms it, and the stream's next
// word.  (Weak, like the hooks below.)
__attribute__((weak)) hipError_t launch_debug_camera_sample(const CameraG& cam, uint32_t w, uint32_t h, float inv_dim, uint64_t seed_mixed,
                                                            uint32_t sample, float* d_o, float* d_d, uint32_t* d_next_word /* or null */,
                                                            hipStream_t s);
// rpt_debug_light_sample / rpt_debug_env_color / rpt_debug_medium_distance: one call of the device function per lane on the committed
// scene (device arrays).  (Weak, like launch_intersect_segments: the host-only harnesses do not know them.)
struct LightSampleArgs {
    uint32_t light;           // index into SceneView::lights (an L_OBJECT)
    uint32_t pad_;
    uint64_t n;
    uint64_t seed_mixed;
    const float* pos;         // [3 n]
    float *v, *nrm, *pdf;     // sample_light_shape: [3 n], [3 n], [n]
    float *intensity, *wi, *dist;   // illuminate_object: [3 n], [3 n], [n]
    uint32_t* next_word;      // [n]: the stream's next word after illuminate_object
};
__attribute__((weak)) hipError_t launch_debug_light_sample(const SceneView& sc, const LightSampleArgs& q, hipStream_t s);
__attribute__((weak)) hipError_t launch_debug_env_color(const SceneView& sc, uint64_t n, const float* d_dirs, float* d_rgb, hipStream_t s);
__attribute__((weak)) hipError_t launch_debug_medium_distance(const SceneView& sc, uint64_t n, uint64_t seed_mixed, float* d_dmed,
                                                              float* d_limit, hipStream_t s);
// rpt_debug_shadow_test: the scan flavours' shadow query and light decision (scan_light_visible), one segment per lane; device arrays.
struct ShadowTestArgs {
    uint32_t light;           // index into SceneView::lights (an L_OBJECT with a twin)
    uint32_t pad_;
    uint64_t n;
    const float *o, *d;       // [3 n] origin and direction of the segment
    const float* dist;        // [n] distance of the light's sample along d
    int32_t* flag;            // [n] the decision: the light is visible
    float* t;                 // [n] the closest hit's t (dist (1 + 1e-3) where the scan found none)
};
__attribute__((weak)) hipError_t launch_debug_shadow_test(const SceneView& sc, const ShadowTestArgs& q, hipStream_t s);
// rpt_debug_distance_pair: the medium distance of draw k as the render kernels form it and by the guarded __logf, k = k0 .. k0 + n - 1.
__attribute__((weak)) hipError_t launch_debug_distance_pair(float sigma_t, uint32_t k0, uint32_t n, float* d_new, float* d_guarded, hipStream_t s);
// rpt_debug_draw_forms: the draw forms behind RPT_RNG_FORMS and their *_ref twins, kDrawFormWords words per lane and side, word w of
// lane i at [w * n + i] (layout: debug_draw_forms_kernel).
static constexpr uint32_t kDrawFormWords = 274;
__attribute__((weak)) hipError_t launch_debug_draw_forms(uint64_t seed_mixed, uint32_t n, const float inv[3], uint32_t* d_new, uint32_t* d_ref,
                                                         hipStream_t s);
// rpt_debug_bounce: stage_bounce<MEDIUM, false> of the render kernels, one case per lane on stream (seed, lane, 0).
struct BounceArgs {
    Material m;
    uint32_t max_bounces, depth;
    uint32_t in_medium;       // the scene has a medium: the MEDIUM instantiation (roulette at surfaces, pdf * 0.8)
    uint32_t medium_event;    // the vertex is a medium point (in_medium only)
    float albedo_med;         // scattering / extinction
    float mcol[3];            // Medium::color at the vertex
    uint64_t n;
    uint64_t seed_mixed;
    const float *nrm, *rd;    // [3 n] surface normal, direction of the arriving ray (not normalised by the hook)
    int32_t* flag;            // [n] stage_bounce's return value
    float *wi, *k;            // [3 n] next direction and path weight (zero where the stage wrote none)
    uint32_t* next_word;      // [n] the stream's next word after the stage
};
__attribute__((weak)) hipError_t launch_debug_bounce(const BounceArgs& q, hipStream_t s);

}  // namespace rptg
namespace rpt64 { struct Args; struct ShootArgs64; struct SurfArgs64; struct FeatureArgs64; }
namespace rptg {
// Reference-epsilon mode (kernels_f64.hip): persistent grid over (pixel, chunk) items with an fp64 slab, then its resolve.
hipError_t launch_render_f64(const rpt64::Args& a, int n_blocks, hipStream_t stream);
hipError_t launch_resolve_f64(const rpt64::Args& a, double scale, double* d_out, hipStream_t stream);
hipError_t render_f64_occupancy(bool medium, int* blocks_per_cu);
// Photon mapping in that mode: the shooting pass (count pass when a.surf and a.vol are null) and the camera pass's surface estimate.
hipError_t launch_photon_shoot_f64(const rpt64::ShootArgs64& a, int n_blocks, hipStream_t stream);
hipError_t launch_photon_surface_f64(const rpt64::SurfArgs64& a, int n_blocks, hipStream_t stream);
hipError_t launch_resolve_photon_f64(const rpt64::Args& a, const void* slab32, uint32_t n_chunks32, double scale_over_total, bool accumulate,
                                     double* d_out, hipStream_t stream);
// The feature pass of that mode (records as FeatureArgs'; launch_feature_resolve resolves them).  (Weak, like launch_features.)
__attribute__((weak)) hipError_t launch_features_f64(const rpt64::FeatureArgs64& a, hipStream_t stream);
#endif  // __HIPCC_RTC__

}  // namespace rptg
