// scene_host.h — the host scene behind the C ABI as rpt_capi.cpp, photon.hip and the host half of kernels_f64.hip share it: the
// options, the host scene store, rpt_scene and rpt_buffer, and the render machinery rpt_capi.cpp defines for the other two.
// Not for kernels.h / kernels.hip: the scan JIT compiles those.
#pragma once
#include <array>
#include <functional>
#include <memory>
#include <string>
#include <unordered_map>
#include <vector>

#include "host_internal.h"
#include "f64_layout.h"

// Options.  Every scene carries its own set, copied from the process defaults when it is created
// (rpt_scene_create) and changed with rpt_scene_set_option; rpt_set_option changes the defaults, i.e. the scenes
// created afterwards.  Nothing a render or commit reads is process-global, so scenes with different options can
// be driven from different host threads.
struct rpt_options {
    int64_t counters = 0;
    int64_t chunk_spp = 0;          // 0 = auto: ceil(iterations / 16) clamped to [2, 32]
    int64_t blocks_per_cu = 0;      // 0 = occupancy query
    int64_t max_blocks = 0;         // cap on the blocks of every persistent launch (renders, photon camera pass, fp64 shooting and surface passes); 0 = no cap.
                                    // A small grid gives every lane / wave many work items: what the schedule tests run (the frame bits do not depend on it)
    int64_t timing = 0;
    int64_t room_shell = 1;         // fold rectangles that are the faces of one box into a single slab test
    int64_t scan_specialise = 1;    // mark y-rotated sphere / cube records and box pairs with common slabs for the unmasked scans (read by rpt_scene_commit)
    int64_t scan_cull = 1;          // primary scans in a medium leave out their tail -- boxes, rectangles, triangles -- when no lane's search interval reaches
                                    // the box around it (read by rpt_scene_commit; 0: the plain scans)
    int64_t scan_jit = 1;           // the scan flavours' render kernel compiled for the scene's record counts (hiprtc): 0 never, 2 always; 1: a cached code
                                    // object is used, and one is compiled at the first launch of at least 2^27 camera samples (rpt_scan_jit_info)
    int64_t shadow_scan = 1;        // shadow queries of the scan flavours keep one bit, "the closest hit is a record of the light's twin", instead of the hit
                                    // code, for every light whose twin is one range of scanned records (read by rpt_scene_commit; 0: the closest-hit scan)
    int64_t photon_skip = 0;
    int64_t photon_block_lists = 1;
    int64_t photon_keep_counts = 0; // 1: the shooting pass's per-photon record counts outlive it (rpt_debug_photon_chain_counts; a test hook)
    int64_t photon_coop_gather = 1; // surface gather of a pixel's samples by the wave together (0: one search per lane)
    int64_t photon_split = 0;       // camera pass of the beam kinds in a medium: volume estimate and surface estimate as two launches (no scratch in
                                    // either, but 112 ms instead of 95 on C4: in one kernel the LDS-bound and the VALU-bound estimate overlap)
    int64_t photon_parts = 4;       // work items per (8x8 pixel block, sample chunk) of the photon camera pass: the block's rows in strips
    int64_t instancing = 1;         // meshes shared by several shapes are stored once and instanced
    int64_t bvh_leaf_max = 4;       // triangles per leaf of a mesh tree (read by rpt_scene_commit)
    int64_t bvh_max_depth = 20;     // a mesh tree deeper than this is rebuilt balanced (read by rpt_scene_commit)
    int64_t bvh_sweep_below = 4096; // ranges of at most this many triangles are split by an exact SAH sweep instead of 16 bins (read by rpt_scene_commit; 0 = bins only)
    int64_t defer_stop = 16;        // still-walking lanes below which a wave leaves the walk (the rest resume later)
    int64_t walk_leaf_quarters = 6; // deferred walks: test the leaves when 4 x (lanes at a leaf) >= this x (lanes still descending); 0 = when all are there
    int64_t defer_lanes = 32;       // parked tree walks per wave that trigger a walk (per-mesh-tree kernels)
    int64_t detach_shadows = 1;     // per-mesh-tree kernels in a medium: 1 = shadow queries that need a tree walk leave their path (0: they park
                                    // the lane), 2 = every tree walk leaves its path ("streamed walks": ring + parked paths in memory)
    int64_t stream_backlog = 48;    // detach_shadows = 2: queries in a wave's ring that trigger a walk session
    int64_t stream_contexts = 1;    // detach_shadows = 2: paths a lane can have waiting in memory (1..6; C5: 272 / 279 / 290 ms for 1 / 2 / 4 at
                                    // 2048x2048x128 -- every parked path is a round trip to the fabric --, 234 with detach_shadows = 1)
    int64_t detach_lanes = 44;      // ... parked primary + queued shadow queries per wave that trigger a walk session
    int64_t pull_batch = 2;         // lanes waiting for a new work item before a wave runs its item bookkeeping (1..64)
    int64_t detach_trigger = 28;    // ... or this many queued shadow queries alone (the queue holds 32)
    int64_t scene_bvh_min = 64;     // bounded primitives + BVH meshes from which the scene-level BVH is built
    int64_t scene_tree_meshes = 0;  // 1: meshes with trees of their own are leaves of the scene tree (every query walks to completion);
                                    // 0: they stay outside it and their walks are parked as in scenes without a scene tree (read by rpt_scene_commit)
    int64_t refit_per_height = 0;   // rpt_scene_move_spheres*: the scene tree's refit as one launch per height (1) instead of one workgroup that walks the
                                    // heights with a barrier between two (0, the measured default: DESIGN.md section 4, "Moving spheres"); same boxes
    int64_t f64_cull = 1;           // reference-epsilon mode: 1 = a lane evaluates only the objects whose fp32 box its ray can reach (same bits), 0 = every object;
                                    // 2 = as 1, and the counters build keeps the search limits as well (its counters then describe the schedule, not the reference's work)
    int64_t f64_mesh_tree_min = 64; // reference-epsilon mode: triangles from which a mesh gets a candidate tree (read by rpt_scene_commit; 0 = never, 1 = every mesh;
                                    // f64_cull = 0 disables the trees as well).  Same bits as the scan of all its triangles
    int64_t f64_photon_slice = 0;   // reference-epsilon photon camera pass: samples per slice (0: as many whole chunks of 256 as fit 32 GB of per-sample selections)
    int64_t f64_surf_batch = 8;     // reference-epsilon mode, scenes with a medium: lanes of a wave that wait at a surface event before the wave runs the surface code (1..64)
    int64_t denoise_stage = -1;     // read by rpt_denoiser_create: passes of step <= this stage their tile + halo in LDS (0: none, -1: the measured default, kDenoiseStageDefault)
    int64_t epsilon_policy = 0;     // 1: the reference-epsilon mode (read by rpt_scene_commit): fp64, generic shapes, t_min = 1e-12, |hit - dist| < 1e-12
};
// ---------------------------------------------------------------------------- host scene
struct HShape {
    rpt_shape_desc d;            // tris / children pointers rewritten to own storage
    std::shared_ptr<const std::vector<double>> mesh;  // interned per scene: shapes sharing a mesh share this
    const std::vector<double>& T() const {
        static const std::vector<double> none;
        return mesh ? *mesh : none;
    }
    std::vector<HShape> children;  // RPT_SHAPE_GROUP
};
struct HObject {
    HShape shape;
    rpt_material mat;
};
struct HLight {
    int kind;
    double color[3], vec[3];
    HObject obj;
};
struct HMedium {
    int kind;
    double absorption, scattering;
};
inline bool holds_monomial(const HShape& h) {   // a MonomialSurface, alone or in a KdTree group
    if (h.d.kind == RPT_SHAPE_MONOMIAL) return true;
    for (const HShape& c : h.children)
        if (holds_monomial(c)) return true;
    return false;
}
// ---------------------------------------------------------------------------- rpt_scene
struct rpt_scene {
    std::vector<HObject> objects;
    std::vector<HLight> lights;
    std::vector<HMedium> media;
    double env[3] = {0, 0, 0};
    uint32_t hdri_w = 0, hdri_h = 0;
    std::vector<float> hdri;  // w*h*4
    std::vector<double> hdri64;  // w*h*3: the texels as they were given (the reference-epsilon mode reads these)
    bool committed = false;
    rpt_options opt;  // this scene's options (rpt_scene_set_option; starts as a copy of the process defaults)
    int device = 0;
    int n_cus = 256;
    rptg::SceneView view{};
    // What one launch owns until its resolve has run: the slab of partial sums and the work counter.  Two sets, so
    // that a caller who alternates between two streams (consecutive frames of an iterative render) gets launches
    // that overlap -- the next frame's blocks fill the CUs that the last paths of this frame no longer keep busy,
    // ~0.35 ms per launch -- while launches on one stream keep using one set.
    struct LaunchSet {
        rpti::DevMem d_slab;
        rpti::DevMem d_queue;
        rpti::DevMem d_stream;   // streamed walks (detach = 2): rings and parked paths of the grid's waves
        rpti::Event done;        // recorded after the resolve of the last launch that used the set
        rpti::Event launched;    // recorded right before its render kernel
        hipStream_t stream = nullptr;
        bool used = false;
    };
    // Everything a commit and the renders after it put on the device: release_device replaces it with an empty one.
    struct Device {
        rpti::DevMem arena;      // the flattened scene (view's arrays)
        rpti::DevMem arena64;    // reference-epsilon mode: view64's arrays
        // per-render cached buffers
        // The owned-tile lists, one per (width, height, shard rank, shard count) a render asked for.  A list is uploaded once, into
        // memory of its own, and never rewritten: the render and resolve kernels of a launch queued on a non-blocking stream read it
        // long after the call has returned, and the next call may ask for another frame.  (prepare_render; a scene that goes
        // through more than kTileLists frames frees the list it has not used for longest -- hipFree waits for the device.)
        struct TileList {
            rpti::DevMem ids;
            uint32_t w = 0, h = 0, rank = 0, count = 0, n_tiles = 0;
            uint64_t used = 0;   // tile_clock of the call that switched to it last
        };
        static constexpr size_t kTileLists = 16;
        std::vector<TileList> tile_lists;
        const uint32_t* d_tiles = nullptr;   // the current one (tk_* below), in tile_lists
        LaunchSet sets[2];
        rpti::DevMem d_counters;
        rpti::DevMem d_out;
        // the feature pass (rpt_render_features*): its records and ids, the planes of the host entry point, and the event recorded after
        // its resolve -- one pass of a scene at a time, whatever the stream; the launch sets above are not involved
        rpti::DevMem d_feat_slab, d_feat_out;
        rpti::Event feat_done;
        bool feat_used = false;
        // "timing": an event triple (before render, after render, after resolve) per launch, in a ring; nothing waits
        // for them until rpt_get_timing / rpt_get_timing_mean is called
        std::vector<rpti::Event> evs;
        // Movable spheres (rpt_scene_set_movable_spheres; rpt_scene_update.cpp): the tables of scene_update.h on the device, and the
        // event recorded after the kernels of the last move -- every later pass of the scene on another stream waits for it
        // (wait_for_move), as the move itself waits for the passes queued before it.
        struct Movable {
            bool set = false;
            uint32_t n = 0;
            std::vector<uint32_t> objects;          // as listed
            rpti::DevMem d_table, d_item_box, d_groups, d_entries, d_raw, d_order, d_centres, d_offsets, d_motion;
            uint32_t n_groups = 0, n_tree = 0, n_heights = 0;
            std::vector<uint32_t> height_first;     // n_heights + 1 values
            rpti::Event done;
            bool used = false;                      // `done` has been recorded
            hipStream_t stream = nullptr;           // ... on this stream
            uint64_t moves = 0;
        } mov;
        // Where the spheres of an earlier list were when that list was replaced (by object): the next list starts from these
        // centres, not from the committed matrices, whether it names the sphere again or leaves it where it was moved to.
        std::unordered_map<uint32_t, std::array<double, 3>> moved_centres;
    } dev;
    int cur_set = 0;
    uint64_t last_counters[64] = {0};  // [0..7] counters, [8..63] diagnostic trip stamps
    uint64_t last_cull[12] = {0};      // rpt_scan_cull_counters (device counters [64..75])
    static constexpr size_t kTimedLaunches = 1024;
    size_t ev_count = 0;  // timed launches since the last rpt_get_timing_mean
    int last_blocks = 0;
    uint64_t prims_per_ray = 0;
    uint32_t n_twin_lights = 0;  // Light::Objects with a twin among the scene's objects (the ones that can be visible)
    std::vector<rptg::Light> light_records;  // the committed light list as the device has it (rpt_shadow_scan_info)
    bool twins_scanned = false;  // every Light::Object that can be visible has its twin among the scanned records, as one range of hit codes
    uint64_t stats[16] = {0};
    rpti::ScanJit jit;   // the specialised render kernel of this scene, if any (option "scan_jit")
    void* photon = nullptr;  // PhotonMapDev*, owned by photon.hip
    bool photon_stale = false;   // spheres have moved since the map was built (rpt_scene_move_spheres*): the camera pass refuses it
    // The commit's record of its scene tree on the host, for a refit (rpt_scene_set_movable_spheres): per entry of pleaf the item's own
    // box (lo, hi), per child entry of a scene-tree node (2 x local node + side) the bounds of the items below it before padding.
    std::vector<float> pleaf_box, tree_raw;
    // reference-epsilon mode (option "epsilon_policy" = 1 at commit): the fp64 scene of kernels_f64.hip in dev.arena64
    rpt64::Scene view64{};
    double medium_color64[3] = {0, 0, 0}, medium_color_hi64[3] = {0, 0, 0};
    const rpt64::MeshNode* mnodes64 = nullptr;   // the candidate trees of its large meshes (f64_layout.h, Args::mnodes, mleaf, mroot), in dev.arena64
    const uint32_t* mleaf64 = nullptr;
    const uint32_t* mroot64 = nullptr;
    uint64_t mesh_tree_info64[8] = {0};          // rpt_f64_mesh_tree_info
    uint64_t last_counters64[64] = {0};   // [0..11] rpt_debug_epsilon_counters, [16 + 2k], [17 + 2k] section k of kernels_f64.hip (executions, lanes)
    // mesh data interned by content (hash -> candidates), so Arc<Mesh>-style sharing survives the C ABI
    std::unordered_map<uint64_t, std::vector<std::shared_ptr<const std::vector<double>>>> mesh_pool;
    // tile cache key: the list dev.d_tiles points to
    uint32_t tk_w = 0, tk_h = 0, tk_rank = 0, tk_count = 0, n_tiles = 0, tiles_x = 0;
    uint64_t tile_clock = 0;
};
// ---------------------------------------------------------------------------- Buffer on the device
struct rpt_buffer {
    int device = 0;
    uint32_t width = 0, height = 0, radius = 0, n_batches = 0;
    rpti::DevMem d_sum, d_sumsq, d_stage;  // stage: one batch / per-pixel variances
    rpti::DevMem d_img;
    rpti::DevMem d_up;                     // rpt_buffer_upsampled_image: mean, variance, filtered mean, the full-resolution frame and its bytes
    // Adaptive sampling by tile (adaptive.hip): allocated at the first tile batch / the first refinement.
    rpti::DevMem d_extra;                  // extra batches per 32 x 32 tile (u32); a pixel holds n_batches + extra[its tile]
    rpti::DevMem d_tile_err, d_active;     // rpt_buffer_refine_tiles' errors when the caller keeps none, its count; rpt_render_adaptive's list
    uint32_t tiles_x() const { return (width + 31) / 32; }
    uint32_t tiles_y() const { return (height + 31) / 32; }
    uint32_t n_tiles() const { return tiles_x() * tiles_y(); }
    rptg::TileBufferView view() const { return rptg::TileBufferView{width, height, tiles_x(), tiles_y(), n_batches, 0, d_extra.get<uint32_t>()}; }
};

// ---------------------------------------------------------------------------- what rpt_capi.cpp defines for photon.hip and kernels_f64.hip
namespace rpti {
inline int first_object_light(const rpt_scene* s) {   // index into scene.lights of the first Light::Object, or -1
    for (size_t i = 0; i < s->lights.size(); i++)
        if (s->lights[i].kind == int(rptg::L_OBJECT)) return int(i);
    return -1;
}
inline bool has_monomial(const rpt_scene* s) {   // some object is (or holds) a MonomialSurface: photon mapping refuses such scenes
    for (const auto& o : s->objects)
        if (holds_monomial(o.shape)) return true;
    return false;
}
// kind of scene.lights[light] (0 point, 1 ambient, 2 directional, 3 object), -1: no such light
inline int light_kind(const rpt_scene* s, uint32_t light) { return light < s->lights.size() ? int(s->lights[light].kind) : -1; }
// Arguments the fp64 kernels share: scene; camera, frame and `a`'s tiles / chunking / work counter / slab when given.
void fill_args64(rpt_scene* s, const rpt_camera* cam, const rpt_render_params* prm, const rptg::RenderArgs* a, rpt64::Args& q);
void fill_camera64(const rpt_camera* cam, rpt64::Camera& q);   // the reference-epsilon mode's camera record (renders and rpt_debug_camera_sample_f64)
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
// One persistent launch and its resolve (run_persistent).
struct PersistentLaunch {
    int blocks_per_cu = 1;                                                           // the grid: this many blocks per CU, at most
    std::function<hipError_t(const rptg::RenderArgs&, int, hipStream_t)> launch;     // (args, n_blocks, stream)
    std::function<hipError_t(double, double*, hipStream_t)> resolve;                 // (scale, d_out, stream); null: resolve_kernel
    bool indexed_start = false;   // every wave takes the batch with its own index first: the work counter starts behind those
    bool wave_items = false;      // n_items counts one item per wave, not per lane
    bool clear_sharded = true;    // false: a sharded frame keeps what is in d_out (a resolve that adds to the earlier slices of the same frame)
};
// Zeroes the queue / sharded frame, calls `launch` with a persistent grid, then resolves the slab into d_out.
int run_persistent(rpt_scene* s, const rpt_render_params* prm, const rptg::RenderArgs& a, double* d_out, hipStream_t st, const PersistentLaunch& pl);
int serialize_with_other_streams(rpt_scene* s, hipStream_t st);  // for launches with per-scene scratch outside the launch set
// A pass that reads the scene's records on `st` follows the last move of its spheres (rpt_scene_move_spheres_device), whatever
// stream that ran on.  Nothing to do for a scene that has not moved.
inline int wait_for_move(rpt_scene* s, hipStream_t st) {
    const auto& m = s->dev.mov;
    if (m.used && m.stream != st) RPTI_HIP_TRY(hipStreamWaitEvent(st, m.done.get(), 0));
    return RPT_OK;
}
int fetch_counters(rpt_scene* s, const rptg::RenderArgs& a);  // the fp32 kernels' counters, after the stream has been synchronised
double* scratch_out(rpt_scene* s, size_t bytes);  // cached device frame for the host-buffer entry points
// photon.hip
void photon_release(void* p);   // rpt_scene::photon (PhotonMapDev*)
}  // namespace rpti
