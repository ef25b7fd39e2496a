/* rpt_hip.h — C ABI of the MI355X-native path-tracing core (drop-in for rpt's hot path).
 *
 * The reference (neevparikh/rpt, Rust, #![forbid(unsafe_code)], src/lib.rs:3) has no FFI
 * seam.  The seam this library replaces is the private method
 *     Renderer::sample(&self, iterations: u32, buffer: &mut Buffer)     src/renderer.rs:158-171
 * i.e. (immutable Scene, Camera, width, height, exposure_value, max_bounces, iterations)
 *      -> width*height linear-RGB f64 means, row-major, y = 0 at the top,
 * which `render()` (src/renderer.rs:137-141) and `iterative_render()` (:144-156) call and
 * feed to `Buffer::add_samples` (src/buffer.rs:32-40).  The entry points below are what a
 * Rust `extern "C"` block (shown in INTEGRATION.md), or the C++ mirror in include/rpt.hpp,
 * binds: plain pointers and sizes, opaque handles owned by the caller, caller-allocated
 * output buffers, no caller pointer retained past a call (mesh data is copied at `add`).
 *
 * Every function returns 0 on success and a negative code on error (never aborts);
 * rpt_last_error() returns the thread-local message of the last failure.
 */
#ifndef RPT_HIP_H
#define RPT_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RPT_OK 0
#define RPT_ERR_INVALID (-1)   /* bad argument / would panic in the reference          */
#define RPT_ERR_STATE (-2)     /* call order (e.g. add after commit, render before)    */
#define RPT_ERR_DEVICE (-3)    /* HIP runtime failure (message carries hipGetErrorString) */
#define RPT_ERR_UNSUPPORTED (-4)

/* Opaque scene handle: mirrors `Scene` (src/scene.rs:12-24). */
typedef struct rpt_scene rpt_scene;

/* Shape kinds: the closed set of `impl Shape` on the hot path
 * (src/shape/sphere.rs, cube.rs, plane.rs, mesh.rs, monomial_surface.rs; `Mesh = KdTree<Triangle>`). */
enum { RPT_SHAPE_SPHERE = 0, RPT_SHAPE_CUBE = 1, RPT_SHAPE_PLANE = 2, RPT_SHAPE_MESH = 3,
       RPT_SHAPE_GROUP = 4, /* KdTree<Box<dyn Bounded>> of other shapes (src/kdtree.rs:103-146,
                              examples/fractal_spheres.rs:45); children must be Bounded (no planes) */
       RPT_SHAPE_MONOMIAL = 5 /* MonomialSurface { height, exp } (src/shape/monomial_surface.rs, monomial_surface(height, exp)
                                 src/shape.rs:292-295): y = height (x^2 + z^2)^2 for x^2 + z^2 <= 1, two-sided.  height is carried
                                 in plane_normal[0], exp in plane_normal[1]; as in the reference, intersection hard-codes the
                                 exponent 4 and ignores exp.  Bounded (a KdTree child may be one).  Not supported as a
                                 Light::Object (MonomialSurface::sample) nor in scenes that are photon-mapped: RPT_ERR_UNSUPPORTED. */ };

/* One `Box<dyn Shape>`: a unit primitive or mesh, optionally wrapped in `Transformed<T>`
 * (src/shape.rs:102-152).  `transform` is the composed homogeneous matrix M, row-major;
 * chained builder calls left-multiply (src/shape.rs:237-284).  The library derives
 * M^-1, the linear part, M^-T and det exactly as `Transformed::new` does (:112-125). */
typedef struct rpt_shape_desc {
    int32_t kind;            /* RPT_SHAPE_*                                              */
    int32_t has_transform;   /* 0: bare shape, 1: Transformed<shape>                     */
    double transform[16];    /* row-major 4x4, used iff has_transform                    */
    double plane_normal[3];  /* Plane { normal, value } (src/shape/plane.rs:7-13); RPT_SHAPE_MONOMIAL: height, exp, - */
    double plane_value;
    const double* tris;      /* n_tris * 18 doubles: v1 v2 v3 n1 n2 n3 (src/shape/mesh.rs:9-23) */
    uint64_t n_tris;
    const struct rpt_shape_desc* children; /* RPT_SHAPE_GROUP: the kd-tree's objects, each a     */
    uint64_t n_children;                   /* full shape (own transform, may itself be a group)  */
} rpt_shape_desc;

/* `enum Material` (src/material.rs:8-23). */
enum { RPT_MAT_LAMBERTIAN = 0, RPT_MAT_PHONG = 1, RPT_MAT_MIRROR = 2, RPT_MAT_TRANSMISSIVE = 3 };
typedef struct rpt_material {
    int32_t kind;
    int32_t _pad;
    double albedo[3];
    double emittance;  /* Lambertian / Phong */
    double shininess;  /* Phong */
    double ior;        /* Transmissive */
} rpt_material;

/* `Medium` constructors (src/medium.rs:80-122): the fields are private in the reference,
 * so these two are the closed set a user can create. */
enum { RPT_MEDIUM_HOMOGENEOUS_ISOTROPIC = 0, RPT_MEDIUM_COLORED_GLOWING_FOG = 1 };

/* `Camera` (src/camera.rs:9-27). */
typedef struct rpt_camera {
    double eye[3], direction[3], up[3];
    double fov, aperture, focal_distance;
} rpt_camera;

/* The `Renderer` fields the sampling path reads (src/renderer.rs:23-56) plus tile sharding. */
typedef struct rpt_render_params {
    uint32_t width, height;
    double exposure_value;
    uint32_t max_bounces;
    /* Multi-GPU tile sharding (no counterpart in the reference, which forks rayon tasks per
     * row, src/renderer.rs:159-162): 32x32 pixel tiles, tile (tx,ty) is rendered iff
     * (tx + ty) % shard_count == shard_rank; other pixels are written as 0 so a sum-reduce
     * over ranks assembles the frame bit-exactly.  shard_count = 0 or 1: whole frame. */
    uint32_t shard_rank, shard_count;
} rpt_render_params;

int rpt_device_count(void);
/* Tile ownership used by the renderer (pure host function): writes the ids (ty * tiles_x + tx,
 * tiles_x = ceil(width/32)) of the 32x32 tiles owned by shard_rank, in render order, and returns
 * their number (or a negative error).  tiles_out may be NULL to query the count. */
int64_t rpt_shard_tiles(uint32_t width, uint32_t height, uint32_t shard_rank, uint32_t shard_count,
                        uint32_t* tiles_out, uint64_t capacity);
const char* rpt_last_error(void);

rpt_scene* rpt_scene_create(void);                 /* Scene::new()            src/scene.rs:26-31 */
void rpt_scene_destroy(rpt_scene*);
/* SceneAdd<Object>  src/scene.rs:40-44; returns the object index (>= 0) or an error. */
int rpt_scene_add_object(rpt_scene*, const rpt_shape_desc*, const rpt_material*);
/* SceneAdd<Light>   src/scene.rs:46-50, one entry point per `enum Light` arm (src/light.rs:7-19). */
int rpt_scene_add_light_point(rpt_scene*, const double color[3], const double location[3]);
int rpt_scene_add_light_ambient(rpt_scene*, const double color[3]);
int rpt_scene_add_light_directional(rpt_scene*, const double color[3], const double direction[3]);
/* Light::Object.  A plane is rejected (Plane::sample is unimplemented!(), src/shape/plane.rs:34). */
int rpt_scene_add_light_object(rpt_scene*, const rpt_shape_desc*, const rpt_material*);
/* SceneAdd<Medium>  src/scene.rs:77-81.  Only media[0] is used (src/renderer.rs:190). */
int rpt_scene_add_medium(rpt_scene*, int32_t kind, double absorption, double scattering);
/* Environment::Color (src/environment.rs:56-77). */
int rpt_scene_set_environment_color(rpt_scene*, const double rgb[3]);
/* Environment::Hdri(Hdri::new(width, height, buf)) (src/environment.rs:3-52): equirectangular image of
 * width*height linear-RGB triples, row-major, looked up bilinearly by direction. */
int rpt_scene_set_environment_hdri(rpt_scene*, uint32_t width, uint32_t height, const double* rgb);
/* Flatten to the device layout and upload; the scene is immutable afterwards
 * (the reference shares `&Scene` immutably across rayon workers, src/renderer.rs:25). */
int rpt_scene_commit(rpt_scene*, int device);

/* Renderer::sample (src/renderer.rs:158-171) for `iterations` paths per pixel.
 * out_rgb: width*height*3 doubles, row-major, y = 0 top; each pixel =
 * mean(trace_ray) * 2^exposure_value, exactly what get_color returns (:173-184).
 * seed / sample_offset key the counter-based RNG stream per (pixel, sample_offset + s):
 * an additive deviation (the reference seeds from entropy, :163). */
int rpt_render_sample(rpt_scene*, const rpt_camera*, const rpt_render_params*, uint32_t iterations,
                      uint64_t seed, uint32_t sample_offset, double* out_rgb);
/* Same, asynchronous: d_out_rgb is a DEVICE pointer (width*height*3 doubles) on the scene's
 * device and hip_stream a hipStream_t (NULL = default stream).  Nothing is copied to the host.  Calls on one
 * stream run in order; calls that alternate between two streams overlap (the scene keeps the per-launch scratch
 * twice), which hides the tail of each launch behind the start of the next; a third stream waits for the scratch
 * it takes over (photon-mapped renders of one scene never overlap: their photon scratch exists once).  Calls on
 * the same scene must still come from one host thread at a time. */
int rpt_render_sample_device(rpt_scene*, const rpt_camera*, const rpt_render_params*, uint32_t iterations,
                             uint64_t seed, uint32_t sample_offset, void* d_out_rgb, void* hip_stream);
/* Tile-list renders (an addition): exactly the listed 32 x 32 tiles, with the kernels a full render of the same scene uses, in
 * both modes.  A tile id is ty * tiles_x + tx with tiles_x = ceil(width / 32), as in rpt_shard_tiles.  Every in-image pixel of a
 * listed tile receives the bits rpt_render_sample* with the same arguments writes there (a pixel's value is a function of scene,
 * camera, params, iterations, seed, sample_offset and the chunking alone, whatever tiles are rendered with it); every other element
 * of the output is left untouched, not zeroed.  n_tiles == 0 is RPT_OK and launches nothing; shard_count > 1 is RPT_ERR_INVALID (a
 * list is the sharding); photon-mapped renders have no such entry point.
 * _device: d_tiles is a DEVICE array of n_tiles ids, trusted to be in range and distinct (rpt_buffer_refine_tiles writes such
 * lists), read by the launch: it must stay unchanged until the call's work on hip_stream is done.  Stream ordering and the two
 * launch sets as for rpt_render_sample_device.
 * Host variant: synchronous; the ids are checked (out of range or listed twice: RPT_ERR_INVALID, before any device call); out_rgb
 * is read first, so the caller's values outside the listed tiles survive. */
int rpt_render_sample_tiles_device(rpt_scene*, const rpt_camera*, const rpt_render_params*, uint32_t iterations,
                                   uint64_t seed, uint32_t sample_offset,
                                   const void* d_tiles, uint32_t n_tiles, void* d_out_rgb, void* hip_stream);
int rpt_render_sample_tiles(rpt_scene*, const rpt_camera*, const rpt_render_params*, uint32_t iterations,
                            uint64_t seed, uint32_t sample_offset,
                            const uint32_t* tiles, uint32_t n_tiles, double* out_rgb);

/* First-hit feature planes of the camera samples a render of the same arguments traces (an addition: the reference renders
 * radiance only).  Sample s in [0, iterations) of pixel (x, y) is the render's camera sample on stream (seed, y*width + x,
 * sample_offset + s) -- rpt_debug_camera_sample / _f64 -- and its closest hit over the whole ray -- rpt_intersect_batch / _f64: t,
 * object, normal; a medium is ignored.  On a hit a = Material::color of the object (the albedo of Lambertian and Phong, 0 for the
 * others), n = the normal as returned (not re-oriented), z = t, c = 1; on a miss a = Environment::get_color(direction) --
 * rpt_debug_env_color / _f64 --, n = 0, z = 0, c = 0.  Every plane is width*height*3 doubles, row-major, y = 0 top, the frame's own
 * format (rpt_buffer_add_samples_device, rpt_frame_pack_device and rpt_gather_frame_device carry it unchanged):
 *   albedo: mean of a;   normal: mean of n (not renormalised);
 *   depth:  (mean of z over all samples, mean of c, id): id = object index + 1 of sample 0 of this call, 0 for a miss, as a double
 *           (the index rpt_intersect_batch* returns); channel 0 / channel 1 = mean hit distance.
 * Summation order: samples are cut into chunks as rpt_scene_render_chunking reports; each channel is an fp64 sum over a chunk in
 * sample order from +0.0 (fp32 mode: every term converted from float first), the chunk sums are added in chunk order from +0.0 and
 * the total is divided by double(iterations).  No atomics: the planes are a function of (scene, camera, params, iterations, seed,
 * sample_offset, chunk_spp) alone.  In the reference-epsilon mode a monomial surface's hit may carry t = NaN, which propagates.
 * Any plane may be NULL (not computed); all three NULL is RPT_ERR_INVALID.  exposure_value and max_bounces are ignored.  Sharding as
 * for rpt_render_sample: only the owned tiles are computed, every other pixel of a requested plane is 0, and the shards' planes add
 * up to the unsharded ones bit for bit.  Same scenes, in both modes, as rpt_render_sample. */
int rpt_render_features(rpt_scene*, const rpt_camera*, const rpt_render_params*, uint32_t iterations,
                        uint64_t seed, uint32_t sample_offset, double* out_albedo, double* out_normal, double* out_depth);
/* Same, asynchronous: DEVICE pointers on the scene's device, hip_stream a hipStream_t (NULL = default stream).  The pass has its
 * own scratch on the scene, apart from the renders': a feature pass and a render on different streams are independent; two feature
 * passes of one scene never overlap (the second waits for the first, whatever its stream). */
int rpt_render_features_device(rpt_scene*, const rpt_camera*, const rpt_render_params*, uint32_t iterations,
                               uint64_t seed, uint32_t sample_offset, void* d_albedo, void* d_normal, void* d_depth,
                               void* hip_stream);

/* Renderer::get_closest_hit (src/renderer.rs:416-425) over n rays (host pointers, fp32).
 * t = +inf, object = -1 on a miss.  normal may be NULL. */
int rpt_intersect_batch(rpt_scene*, uint64_t n, const float* origins, const float* dirs, float* t,
                        int32_t* object, float* normal);
/* The primary query of the scan kernels over n segments: the closest accepted hit with t in [t_min(origin), t_max[i]), through
 * the culled scan when the scene was committed with "scan_cull" = 1 (and is eligible for it) and through the plain scan
 * otherwise.  Consecutive groups of 64 segments form a wave, as 64 paths do in a render.  t = t_max[i] and code = 0xFFFFFFFF on a
 * miss; code = kind << 28 | record otherwise.  For scenes whose records are all scanned (no tree), else RPT_ERR_UNSUPPORTED. */
int rpt_intersect_segments(rpt_scene*, uint64_t n, const float* origins, const float* dirs, const float* t_max, float* t,
                           uint32_t* code);
/* The same query in the reference-epsilon mode (a scene committed with epsilon_policy = 1, else RPT_ERR_STATE): the fp64
 * closest hit of that mode's kernels, t_min = 1e-12, over n rays given in fp64.  t = +inf, object = -1 on a miss; a hit may
 * carry t = NaN where the reference's own test produces one (MonomialSurface).  normal may be NULL. */
int rpt_intersect_batch_f64(rpt_scene*, uint64_t n, const double* origins, const double* dirs, double* t,
                            int32_t* object, double* normal);

/* Flattened-layout statistics of a committed scene: [0] spheres, [1] general (rotated) cubes,
 * [2] planes, [3] linearly scanned triangles, [4] axis-aligned boxes, [5] axis-aligned
 * rectangles (pairs of wall triangles), [6] BVH triangles, [7] BVH nodes, [8] bytes of scan
 * records every closest-hit query walks, [9] bytes of scene data resident in HBM, [10] 1 if one scene-level
 * tree replaces the scan (2: ... and the meshes with trees of their own stay outside it, their walks parked), [11] primitives in it, [12] mesh instances, [13] meshes stored once and instanced,
 * [14] wall rectangles folded into a box shell, [15] levels of the deepest walk (scene tree + mesh tree). */
int rpt_scene_stats(rpt_scene*, uint64_t out[16]);
/* Counters of the last rpt_render_sample* call on this scene (device-side, exact):
 * [0] camera samples, [1] closest-hit queries (rays), [2] path vertices, [3] kernel loop trips
 * (wave-iterations summed over waves), [4] primitive tests, [5] BVH nodes visited,
 * [6] BVH triangle tests, [7] tree walks that found their stack full (must be 0: scenes whose trees could overflow it
 * are refused at commit).  Filled only when the library is built with RPT_COUNTERS or
 * rpt_set_option("counters", 1) was called before the render; otherwise zeros (also for a scene with a
 * group as a Light::Object: that kernel flavour has no counters build). */
int rpt_get_counters(rpt_scene*, uint64_t out[8]);
/* Diagnostic (counters on): for section k of the megakernel's loop body (kernels.hip, SECT(k)),
 * out[2k] = wave-level executions and out[2k+1] = lanes active in them during the last path-traced
 * render: the lane utilisation of each divergent piece of code. */
int rpt_debug_section_counters(rpt_scene*, uint64_t out[56]);
/* Diagnostic (counters on; a render of a scene with a medium whose records are all scanned): the primary scans of the last render
 * by wave trip.  out[0..4]: trips in which 0, 1-2, 3-4, 5-8, more than 8 lanes have a search interval that reaches the box around
 * all scanned records; out[5..8]: trips with such a lane in which none of them reaches the box of candidate record group 0..3
 * (rpt_scan_cull_groups); out[9]: trips whose scan left out its tail (option "scan_cull"); out[10..11]: 0.  out[12]: the scene has
 * a bound and groups (no planes, at most 64 scanned records), out[13]: the number of groups, out[14]: the records in no group
 * because their box is most of the bound (mask), out[15]: the scene's primary scans are culled. */
int rpt_scan_cull_counters(rpt_scene*, uint64_t out[16]);
/* The boxes of a committed scene's primary scans: out_boxes[0..5] = lo, hi of the box around all scanned records, [6..29] lo, hi of
 * the candidate groups (6 floats each, 4 groups), [30..35] lo, hi of the box around the scan's tail -- boxes, rectangles,
 * triangles --, which "scan_cull" tests; out_masks[0..3] the groups' records (the scan's numbering: spheres, cubes, boxes,
 * rectangles, triangles), out_masks[4] the records in no group; *n_groups their number; *enabled = the scans are culled. */
int rpt_scan_cull_groups(rpt_scene*, float out_boxes[36], uint64_t out_masks[5], uint32_t* n_groups, uint32_t* enabled);
/* HIP-event timing of the last render on this scene (needs rpt_set_option("timing", 1)):
 * milliseconds of the megakernel and of the resolve kernel on the stream they ran on, and the
 * persistent grid size.  Synchronises on the last recorded event. */
int rpt_get_timing(rpt_scene*, double* render_ms, double* resolve_ms, int32_t* grid_blocks);
/* The same over every timed render since the previous call of this function (at most the latest 1024): mean
 * milliseconds per launch.  Renders do not wait for their events, so a loop of rpt_render_sample_device calls
 * stays asynchronous and is measured afterwards.  Starts a new measurement. */
int rpt_get_timing_mean(rpt_scene*, double* render_ms, double* resolve_ms, int32_t* launches);
/* The work decomposition rpt_render_sample* will use for `iterations` samples per pixel (pure host function of
 * `iterations` and the "chunk_spp" option): samples per work item and work items (= partial-sum slab entries of
 * 16 bytes) per pixel. */
int rpt_render_chunking(uint32_t iterations, uint32_t* chunk_spp, uint32_t* n_chunks);
/* The same for one scene: reads that scene's "chunk_spp" option (rpt_scene_set_option), i.e. exactly what its
 * renders use; rpt_render_chunking reads the process defaults. */
int rpt_scene_render_chunking(rpt_scene*, uint32_t iterations, uint32_t* chunk_spp, uint32_t* n_chunks);
/* Options.  Every scene has its own set: a copy of the process defaults taken by rpt_scene_create, changed with
 * rpt_scene_set_option (before rpt_scene_commit for the options the commit reads, at any time for the others; nothing
 * a commit or render reads is process-global, so scenes with different options may be driven from different host
 * threads).  rpt_set_option changes the defaults, i.e. the scenes created afterwards (and what rpt_render_chunking
 * reports).  Names (all optional): "counters" 0/1, "chunk_spp" (samples per work item, 0 = auto),
 * "blocks_per_cu" (persistent grid size), "max_blocks" (cap on the blocks of every persistent launch -- renders, photon camera
 * pass, the reference-epsilon shooting and surface passes --, 0 = none, the default: a small grid gives every lane or wave many work
 * items, which is what the schedule tests need; no effect on the image), "timing" 0/1, "scene_bvh_min" (read by rpt_scene_commit:
 * number of bounded primitives + BVH meshes from which one scene-level BVH replaces the linear
 * object scan, default 64), "instancing" 0/1 (read by rpt_scene_commit: store a mesh that several
 * shapes share once and instance it, default 1), "room_shell" 0/1 (read by rpt_scene_commit: answer the
 * rectangles that are the faces of one axis-aligned box with a single slab test, default 1),
 * "scan_specialise" 0/1 (read by rpt_scene_commit: mark the sphere / cube records that are rotated about the vertical axis only
 * and the adjacent box records with common slabs, so that the linear scans leave out the zero terms and the repeated slab
 * arithmetic, default 1; the hits are bit-identical either way),
 * "scan_cull" 0/1 (read by rpt_scene_commit, default 1: in a medium a primary scan tests the box around the records behind the
 * shell in scan order -- boxes, rectangles, triangles -- once per lane and leaves those records out when no lane of the wave has a
 * search interval that reaches it; the frames are bit-identical either way),
 * "scan_jit" 0/1/2 (default 1: the scan kernels compiled for the scene's record counts, see rpt_scan_jit_info; read at every render),
 * "shadow_scan" 0/1 (read by rpt_scene_commit, default 1: the shadow query of a linear scan keeps one bit, "the closest hit is a
 * record of the light's twin object", in place of the hit code, for every object light whose twin is one range of records of one
 * scanned kind; group lights, twins that are faces of the room shell or monomial surfaces, and 0 keep the closest-hit scan; the
 * frames are bit-identical either way),
 * "photon_block_lists" 0/1 (camera pass of the beam x point kind: collect the photon spheres of each strip of an
 * 8x8 pixel block once per work item and test them with one photon per lane, default 1; 0 walks the tree per
 * sample), "photon_parts" (work items per 8x8 pixel block and sample chunk of the photon camera pass: the block's
 * rows in 1, 2, 4 or 8 strips, default 4; changes the fp32 order of a pixel's beam sum, nothing else),
 * "photon_keep_counts" 0/1 (default 0; 1: the per-photon record counts of a shooting pass are kept with the map for
 * rpt_debug_photon_chain_counts -- a test hook; without it the shooting pass allocates and launches exactly what it did),
 * "photon_coop_gather" 0/1 (surface estimate of the photon camera pass: the wave collects the candidates of a
 * pixel's samples together and every lane picks its K nearest from that list, default 1; 0 searches per lane),
 * "photon_skip" (diagnostic bit mask that switches parts of the photon camera pass off), "defer_lanes" / "defer_stop" (scenes whose meshes
 * have their own trees: a wave starts its parked tree walks when this many lanes wait, default 32, and leaves
 * them when fewer than this many are still walking, default 16; the image does not depend on either),
 * "detach_shadows" 0/1/2 (scenes whose meshes have their own trees, in a medium: 1, the default: a shadow query that needs a tree walk
 * leaves its path and is answered from a queue of its wave, "detach_lanes" (default 44) waiting + queued queries or "detach_trigger"
 * (default 28) queued ones start a walk session; 0: shadow queries park like primary ones; 2: primary queries leave as well, their
 * paths wait in memory, "stream_backlog" (default 48) queued queries start a session and a lane may have "stream_contexts" (1..6,
 * default 1) paths waiting -- slower, kept for measurement; the image depends on none of the thresholds),
 * "scene_tree_meshes" 0/1 (read by rpt_scene_commit: in a scene that has a scene-level tree, 1 makes the meshes with trees of their own
 * leaves of it; default 0: their walks are parked beside it), "bvh_sweep_below" (read by rpt_scene_commit: ranges of at most this many
 * triangles are split by an exact SAH sweep instead of 16 bins, default 4096, 0 = bins only),
 * "photon_split" 0/1 (camera pass of the beam kinds in a medium: volume and surface estimate as two launches, default 0 -- slower),
 * "pull_batch" (path tracer: a wave hands out new work items when this many of its lanes wait for one, or when none of its lanes
 * has anything else to do; 1..64, default 2; no effect on the image),
 * "walk_leaf_quarters" (same scenes: the descent of such a walk pauses for the triangle tests as soon as 4 x the lanes
 * waiting at a leaf >= this x the lanes still descending, default 6, 0 = when every lane is at a leaf; no effect on the image),
 * "bvh_leaf_max" (read by rpt_scene_commit: triangles per leaf of a mesh tree, default 4 -- C5: 49.8 / 43.1 / 41.1 /
 * 41.1 / 41.7 ms for 1 / 2 / 4 / 6 / 8), "bvh_max_depth" (read by rpt_scene_commit: a mesh tree that the SAH builder makes deeper than this is rebuilt
 * with object-median splits, default and maximum 20 -- the traversal stack holds 21 entries per mesh tree, 32 for scene tree + mesh tree;
 * a scene that still does not fit is refused with RPT_ERR_UNSUPPORTED),
 * "denoise_stage" (a process option, read by rpt_denoiser_create: -1, 0, 1 or 2, see the denoiser below);
 * returns RPT_ERR_INVALID for unknown names. */
int rpt_set_option(const char* name, int64_t value);
int rpt_scene_set_option(rpt_scene*, const char* name, int64_t value);

/* ---- Buffer on the device (src/buffer.rs:5-97): the samples of each pixel are kept as running
 * sums, so image() = box filter (Filter::Box(radius), :76-97) + color_bytes (src/color.rs:18-24)
 * and variance() (:60-74) run where the frame is and only width*height*3 bytes come back. */
typedef struct rpt_buffer rpt_buffer;
rpt_buffer* rpt_buffer_create(int device, uint32_t width, uint32_t height, uint32_t filter_radius); /* Buffer::new */
void rpt_buffer_destroy(rpt_buffer*);
int rpt_buffer_add_samples(rpt_buffer*, const double* rgb /* host, width*height*3 */);           /* Buffer::add_samples */
int rpt_buffer_add_samples_device(rpt_buffer*, const void* d_rgb, void* hip_stream);
int rpt_buffer_image(rpt_buffer*, uint8_t* out_rgb8 /* host, width*height*3 */);                 /* Buffer::image */
int rpt_buffer_variance(rpt_buffer*, double* out);                                               /* Buffer::variance */
int rpt_buffer_batches(rpt_buffer*, uint32_t* n);
/* Renderer::sample(&self, iterations, &mut Buffer) itself (src/renderer.rs:158-171): render one
 * batch and push its means into the buffer without leaving the device. */
int rpt_render_into_buffer(rpt_scene*, const rpt_camera*, const rpt_render_params*, uint32_t iterations,
                           uint64_t seed, uint32_t sample_offset, rpt_buffer*);

/* ---- denoiser on the device (an addition: the reference's only spatial filter is Filter::Box) ----
 * An edge-avoiding a-trous wavelet filter of the SVGF family, spatial part only, guided by the first-hit feature planes
 * (rpt_render_features*) and by the per-pixel variance of a frame's mean (rpt_buffer_mean_device).  Temporal accumulation and
 * reprojection are rpt_temporal_* below.  Sharded frames are not filtered shard by shard: a shard's planes and frame are assembled first
 * (rpt_gather_frame_device carries them) and rank 0 filters.
 *
 * The filter is defined as an order of fp64 operations, each rounded on its own (no fused multiply-add, IEEE division, no atomics),
 * so the result is a function of the arguments alone, whatever the tiling, the option "denoise_stage" or the stream.  Every array
 * is fp64, row-major, y = 0 at the top: rgb[h][w][3]; var[h][w], the variance of the pixel's mean, or NULL; albedo, normal, depth
 * in the format rpt_render_features writes, each or NULL.  passes P in 1..8; flags RPT_DENOISE_*; a term is on iff its sigma > 0.
 * A term or flag whose plane is NULL is RPT_ERR_INVALID: sigma_color > 0 needs var, sigma_normal > 0 normal, sigma_depth > 0 depth,
 * RPT_DENOISE_DEMODULATE albedo, RPT_DENOISE_MATCH_ID depth.
 *   Per pixel p:  den_k = (DEMODULATE and albedo_k > 0.0) ? albedo_k : 1.0 (false for NaN);  c_k = rgb_k / den_k;
 *     v = var ? var[p] : 0.0;  n = normal (0 when NULL);  z = depth[..][0], id = depth[..][2] (0 when NULL).
 *   Pass i = 0 .. P-1, step s = 2^i:
 *     colour term only:  vhat_p = (sum (g_dy g_dx) v_q) / (sum g_dy g_dx) over the 3 x 3 neighbours (distance 1) inside the image,
 *       g = (1/4, 1/2, 1/4), dy outer, dx inner, both sums from +0.0;  k_p = 1.0 / ((sigma_color sigma_color) (vhat_p + 1e-12)).
 *     a_n = 1.0 / sigma_normal;  a_z = 1.0 / (sigma_depth double(s)).
 *     For dy = -2..2 (outer), dx = -2..2 (inner), q = p + s (dx, dy); taps outside the image are skipped.
 *       x = +0.0, then the enabled terms in the order colour, normal, depth:
 *         colour: e_k = (c_q,k - c_p,k) den_p,k;  x = x + ((e0 e0 + e1 e1) + e2 e2) k_p
 *         normal: e_k = (n_q,k - n_p,k) a_n;      x = x + ((e0 e0 + e1 e1) + e2 e2)
 *         depth:  e = (z_q - z_p) a_z;            x = x + e e
 *       The tap is skipped unless x < 4.0 and, with MATCH_ID, id_q == id_p (NaN fails both tests).
 *       t = 1.0 - x 0.25;  t2 = t t;  w = (t2 t2) (h_dy h_dx), h = (1/16, 1/4, 3/8, 1/4, 1/16): a compactly supported stand-in for
 *       exp(-x) without a transcendental.   W += w;  C_k += w c_q,k;  V += (w w) v_q, all from +0.0.
 *     End of the pass: if W > 0.0, c' = C_k / W and v' = V / (W W); otherwise the pixel keeps c and v (what a NaN colour with the
 *     colour term on, a NaN variance, depth or id with their term or flag on does to the pixel itself).
 *   Output: out_k = c_k den_k, and optionally the filtered v.
 * A denoiser owns the ping-pong records of one frame size on one device.  rpt_denoiser_create reads the process option
 * "denoise_stage" (rpt_set_option): -1 the measured default (2), 0 every pass gathers its taps from global memory, n = 1 or 2 the passes
 * of step <= n stage their tile and its halo in LDS first (larger n: RPT_ERR_INVALID) -- the same bits either way.
 * Every argument check precedes every device call.  d_out (and d_out_var) must not be one of the inputs.  Two calls on one denoiser
 * are ordered, whatever their streams; denoisers are independent of each other and of renders. */
#define RPT_DENOISE_DEMODULATE 1u
#define RPT_DENOISE_MATCH_ID 2u
typedef struct rpt_denoise_params {
    uint32_t passes, flags;
    double sigma_color, sigma_normal, sigma_depth;
} rpt_denoise_params;
typedef struct rpt_denoiser rpt_denoiser;
rpt_denoiser* rpt_denoiser_create(int device, uint32_t width, uint32_t height);
void rpt_denoiser_destroy(rpt_denoiser*);
/* DEVICE pointers on the denoiser's device, hip_stream a hipStream_t (NULL = default stream); d_out: width*height*3 doubles,
 * d_out_var: width*height doubles or NULL. */
int rpt_denoise_device(rpt_denoiser*, const rpt_denoise_params*, const void* d_rgb, const void* d_var, const void* d_albedo,
                       const void* d_normal, const void* d_depth, void* d_out, void* d_out_var, void* hip_stream);
/* The same with host pointers, synchronous. */
int rpt_denoise(rpt_denoiser*, const rpt_denoise_params*, const double* rgb, const double* var, const double* albedo,
                const double* normal, const double* depth, double* out, double* out_var);
/* Per pixel of a buffer with n batches: d_rgb = sum / n in push order (width*height*3 doubles), d_var (width*height doubles, or
 * NULL) = the variance of that mean, max(sumsq - n ((mr mr + mg mg) + mb mb), 0) / (n - 1) / n: the per-pixel expression of
 * rpt_buffer_variance divided by n, each operation rounded on its own.  RPT_ERR_STATE with fewer than 2 batches.  Enqueued on
 * hip_stream; batches added on other streams must have been waited for by the caller. */
int rpt_buffer_mean_device(rpt_buffer*, void* d_rgb, void* d_var, void* hip_stream);
/* mean -> filter -> color_bytes (src/color.rs:18-24), no box filter; synchronous, only width*height*3 bytes come back.  The planes
 * are DEVICE pointers (each or NULL, as the parameters allow).  Buffer and denoiser of different devices or sizes: RPT_ERR_INVALID. */
int rpt_buffer_denoised_image(rpt_buffer*, rpt_denoiser*, const rpt_denoise_params*, const void* d_albedo, const void* d_normal,
                              const void* d_depth, uint8_t* out_rgb8);

/* ---- guided upsampling on the device (an addition: the reference renders every pixel it shows) ----
 * A joint-bilateral upsampling: a frame rendered at (w, h) and the variance of its mean are taken to (W, H) = (s w, s h), steered by
 * the first-hit feature planes of BOTH sizes (rpt_render_features* of the same camera: the reference's pixel-to-ray map,
 * src/renderer.rs:173-181, is scale-consistent, so pixel (i, j) of the small render integrates exactly over the full-size pixels
 * s i .. s i + s - 1, s j .. s j + s - 1).  Texture and geometry edges come from the full-size planes; only the lighting is interpolated.
 *
 * Defined, like the denoiser, as an order of fp64 operations, each rounded on its own (no fused multiply-add, IEEE division, no
 * atomics): the result is a function of the arguments alone, whatever the tiling or the stream.  Every array is fp64, row-major,
 * y = 0 at the top.  Low resolution (w x h): lo_rgb[h][w][3]; lo_var[h][w] or NULL; lo_albedo, lo_normal, lo_depth in the format
 * rpt_render_features writes, each or NULL.  Full resolution: hi_albedo, hi_normal, hi_depth, each or NULL.  Outputs: out_rgb[H][W][3],
 * out_var[H][W] or NULL.  scale s in {2, 3, 4}; radius r in {1, 2} (2 r taps per axis); flags RPT_UPSAMPLE_*; a term is on iff its sigma
 * > 0.  A term or flag whose plane is NULL on either side is RPT_ERR_INVALID: sigma_normal > 0 needs both normal planes,
 * sigma_depth > 0 and RPT_UPSAMPLE_MATCH_ID both depth planes, RPT_UPSAMPLE_DEMODULATE both albedo planes.
 *   Full-resolution pixel p = (X, Y):
 *     den_p,k = (DEMODULATE and hi_albedo_p,k > 0.0) ? hi_albedo_p,k : 1.0 (false for NaN); for a low-resolution pixel q, den_q,k is
 *       the same rule on lo_albedo;  c_q,k = lo_rgb_q,k / den_q,k;  v_q = lo_var ? lo_var[q] : 0.0.
 *     Position, in integers: tx = 2 X + 1 - s (signed);  i0 = floor(tx / (2 s)) (floor division, may be -1);
 *       fx = double(tx - 2 s i0) / double(2 s);  the same for ty, j0, fy: the pixel's centre in low-resolution pixel-centre coordinates.
 *     a_n = 1.0 / sigma_normal;  a_z = 1.0 / (sigma_depth double(s)).
 *     For dy = 1-r .. r (outer), dx = 1-r .. r (inner), q = (i0 + dx, j0 + dy); taps outside the low-resolution image are skipped.
 *       g_dx = 1.0 - |fx - double(dx)| / double(r), likewise g_dy; the tap is skipped unless g_dx > 0.0 and g_dy > 0.0 (r = 1: the
 *       bilinear 2 x 2).
 *       x = +0.0, then the enabled terms in the order normal, depth:
 *         normal: e_k = (lo_normal_q,k - hi_normal_p,k) a_n;   x = x + ((e0 e0 + e1 e1) + e2 e2)
 *         depth:  e = (lo_depth_q[0] - hi_depth_p[0]) a_z;     x = x + e e
 *       The tap is skipped unless x < 4.0 and, with MATCH_ID, lo_depth_q[2] == hi_depth_p[2] (NaN fails every test).
 *       t = 1.0 - x 0.25;  t2 = t t;  wgt = (t2 t2) (g_dy g_dx): the denoiser's stand-in for exp(-x).
 *       Wsum += wgt;  C_k += wgt c_q,k;  V += (wgt wgt) v_q, all from +0.0.
 *     If Wsum > 0.0: c_k = C_k / Wsum and v = V / (Wsum Wsum); otherwise the pixel falls back to its own footprint q = (X / s, Y / s)
 *     (integer division): c = c_q, v = v_q.
 *     out_rgb_k = c_k den_p,k;  out_var = v.
 * Checks, in this order and all before any device call, each RPT_ERR_INVALID: null parameters; scale; radius; unknown flag; a sigma
 * that is not finite and >= 0; a zero size; s w or s h not below 2^32, or W H not below 2^31; null lo_rgb or out_rgb; the planes of
 * sigma_normal, sigma_depth, DEMODULATE, MATCH_ID (in that order, the low-resolution one first); an output that is one of the inputs
 * or the other output; (rpt_upsample) the device index. */
#define RPT_UPSAMPLE_DEMODULATE 1u
#define RPT_UPSAMPLE_MATCH_ID 2u
typedef struct rpt_upsample_params {
    uint32_t scale;    /* s in {2, 3, 4} */
    uint32_t radius;   /* r in {1, 2}: taps per axis = 2 r */
    uint32_t flags;    /* RPT_UPSAMPLE_* */
    uint32_t _pad;
    double sigma_normal, sigma_depth;   /* a term is on iff its sigma > 0 */
} rpt_upsample_params;
/* Stateless and asynchronous, on the current device (as rpt_frame_pack_device): DEVICE pointers, hip_stream a hipStream_t (NULL =
 * default stream); one out-of-place pass, no scratch.  The outputs must not alias the inputs. */
int rpt_upsample_device(const rpt_upsample_params*, uint32_t lo_width, uint32_t lo_height, const void* d_lo_rgb, const void* d_lo_var,
                        const void* d_lo_albedo, const void* d_lo_normal, const void* d_lo_depth, const void* d_hi_albedo,
                        const void* d_hi_normal, const void* d_hi_depth, void* d_out_rgb, void* d_out_var, void* hip_stream);
/* The same with host pointers on device `device`, synchronous. */
int rpt_upsample(int device, const rpt_upsample_params*, uint32_t lo_width, uint32_t lo_height, const double* lo_rgb, const double* lo_var,
                 const double* lo_albedo, const double* lo_normal, const double* lo_depth, const double* hi_albedo,
                 const double* hi_normal, const double* hi_depth, double* out_rgb, double* out_var);
/* color_bytes (src/color.rs:18-24) of a DEVICE plane of width*height*3 doubles on the current device, enqueued on hip_stream and
 * waited for: only the width*height*3 bytes come back, to host memory.  What ends a pipeline composed from device entry points.
 * RPT_ERR_INVALID: a null pointer, a zero size, width*height not below 2^31. */
int rpt_image_bytes_device(const void* d_rgb, uint32_t width, uint32_t height, uint8_t* out_rgb8_host, void* hip_stream);
/* mean -> (with a denoiser of the buffer's size: the a-trous filter at the low resolution, on the low-resolution planes) -> upsample ->
 * color_bytes; synchronous, only (s w)(s h)*3 bytes come back.  `lo` holds the low-resolution batches; the planes are DEVICE
 * pointers (each or NULL, as the parameters allow).  Checks in this order: null buffer or output; the upsampling's (above); with a
 * denoiser the denoiser's, then devices and sizes; RPT_ERR_STATE with fewer than 2 batches.  Without a denoiser the denoise parameters
 * are ignored. */
int rpt_buffer_upsampled_image(rpt_buffer* lo, rpt_denoiser* lo_denoiser_or_null, const rpt_denoise_params*, const rpt_upsample_params*,
                               const void* d_lo_albedo, const void* d_lo_normal, const void* d_lo_depth, const void* d_hi_albedo,
                               const void* d_hi_normal, const void* d_hi_depth, uint8_t* out_rgb8);

/* ---- temporal accumulation with reprojection (an addition with no counterpart in the reference, whose frame sequences --
 * examples/simple_video.rs, marbles.rs -- render every frame from nothing) ----
 * For a camera that moves over a scene whose objects keep their indices: a frame's pixel is blended with what the previous
 * frames saw at the same surface point.  The point comes from the depth plane and the camera, its place in the previous frame from the
 * camera stored with the history and, for objects that move, from a motion record per object (below); id, depth and normal tests
 * reject history of another surface.  Without a motion table an object that has moved far degrades to no reuse, but one that still
 * overlaps its previous footprint has the same id and nearly the same depth: its pixels pass the tests and are blended with history
 * of a DIFFERENT surface point (on the moving, spinning sphere of tests/test_temporal_motion_host.py 167 of 285 pixels do, with a
 * median error of 0.17 of a colour painted in object space; with the table 284 of 285 and 0.0016).  No demodulation (materials are one
 * colour per object and ids are matched).  With a thin lens (aperture > 0) depths are measured from lens samples but reprojected from `eye`: an approximation
 * that the depth test absorbs.
 *
 * Defined, like the denoiser, as an order of fp64 operations, each rounded on its own: no contraction, IEEE division, sqrt the
 * correctly rounded square root, no atomics; tan is evaluated on the host only.  Arrays are row-major, y = 0 at the top; rgb, var,
 * normal and depth in the formats rpt_buffer_mean_device and rpt_render_features* write.
 *
 * The camera record: rpt_temporal_camera_record (pure host function, no device is touched) writes eye[3], direction[3], right[3],
 * up[3], d with right = normalize(cross(direction, up)) and d = 1 / tan(fov / 2) (src/camera.rs:67-68); RPT_ERR_INVALID for a field
 * that is not finite, fov outside (0, pi) or a zero cross product.  The accumulation takes records, never a camera.
 *
 * Per pixel p = (x, y) of a W x H frame; dim = double(max(W, H)); R the call's camera record, R' the one stored with the history;
 * v_in = var ? var[p] : 0.0.
 *   1. Pixel centre (src/renderer.rs:174-176 without jitter):
 *        xn = (double(2x+1) - double(W)) / dim;   yn = (double(2(H-y)-1) - double(H)) / dim
 *        v_k = (d direction_k + xn right_k) + yn up_k;   l = sqrt((v0 v0 + v1 v1) + v2 v2)
 *   2. cov = depth[p][1]; hit = cov > 0.0 (false for NaN); zc = depth[p][0] / cov; id = depth[p][2]; n = normal[p] (0 when NULL).
 *   3. History is looked up only if the accumulator holds a frame and hit:
 *        s = zc / l;  P_k = eye_k + s v_k;  q_k = P_k - eye'_k;  zq = (q0 dir'0 + q1 dir'1) + q2 dir'2;  require zq > 0.0
 *        u = (((q0 r'0 + q1 r'1) + q2 r'2) d') / zq, and w likewise with up'
 *        fx = ((u dim + double(W)) - 1.0) 0.5;   fy = ((double(H) - 1.0) - w dim) 0.5
 *        require fx > -1.0 && fx < double(W), and the same for fy against H (NaN fails)
 *        ix = floor(fx), ax = fx - ix; iy, ay likewise;  qq = (q0 q0 + q1 q1) + q2 q2
 *   4. Taps j = 0, 1 (outer), i = 0, 1 (inner) at (ix+i, iy+j); taps outside the image are skipped.
 *        b = (i ? ax : 1.0 - ax) (j ? ay : 1.0 - ay).  The tap's history record h is skipped unless h.len > 0.0; with MATCH_ID unless
 *        h.id == id; with depth_tol > 0, r = h.z h.z, unless fabs(r - qq) <= depth_tol qq; with normal_tol > 0, e_k = h.n_k - n_k,
 *        unless ((e0 e0 + e1 e1) + e2 e2) <= normal_tol normal_tol.  NaN fails every test.
 *        B += b;  C_k += b h.c_k;  V += (b b) h.v;  L += b h.len, all from +0.0.
 *   5. If B > 0.0:  hc_k = C_k / B;  hv = V / (B B);  hl = L / B;  len = min(hl + 1.0, double(max_history));  a = 1.0 / len
 *        out_k = hc_k + (rgb_k - hc_k) a;   om = 1.0 - a;   out_v = (om om) hv + (a a) v_in
 *      (the variance of a blend of independent terms, in the units rpt_denoise_device expects).
 *      Otherwise out = rgb, out_v = v_in, len = 1.0.
 *   6. The new history record: c = out, v = out_v, n, z = zc, id, len.  If the pixel is not a hit, or any of out_k, out_v is not
 *      finite (t - t != 0.0), len = 0.0 is stored (the len written to d_out_len is unchanged): a NaN or a firefly at inf never outlives
 *      its frame, and a miss carries no history.
 *
 * max_history 1..4096 (1: no reuse); the tolerances finite and >= 0 (0: the test is off); depth_tol is relative, on SQUARED distances;
 * normal_tol on the distance of the normal planes.  d_normal is NULL iff normal_tol == 0.  Defaults: 16, MATCH_ID, 0.1, 0.5.
 * An accumulator owns the history of one frame size on one device: two arrays of 80-byte records (c[3], v, len, n[3], z, id) that swap
 * per call -- a call reads its neighbours' old records while it writes new ones -- and the camera record of the last call.  Every
 * argument check precedes every device call, the parameters' and the planes' before the handle's.  Outputs must not alias inputs or
 * each other.  The calls of one accumulator are ordered, whatever their streams; accumulators share nothing with each other, with
 * scenes or with denoisers.
 *
 * Moving objects.  A motion record is RPT_TEMPORAL_MOTION_DOUBLES = 24 doubles (192 bytes, 16-byte aligned on the device):
 *   r[0..11]   A, a 3 x 4 row-major affine map that takes a world point on the object in the current frame to the world point the
 *              same material point had in the previous frame;
 *   r[12..20]  G, a 3 x 3 row-major map for normals, current to previous;
 *   r[21..23]  zero, never read.
 * rpt_temporal_motion_record (pure host function, no device is touched) writes the record of an object whose composed
 * object-to-world matrices (the format of rpt_shape_desc.transform) are `cur` in the current and `prev` in the previous frame:
 * A = the top three rows of prev . cur^-1, G = (linear part of A)^-T, by cofactors, every fp64 operation rounded on its own.  With
 * c_ij = cur[4i+j], t_i = cur[4i+3], p_ij = prev[4i+j], s_i = prev[4i+3] (i, j = 0..2):
 *   k_00 = c11 c22 - c12 c21;  k_01 = c02 c21 - c01 c22;  k_02 = c01 c12 - c02 c11
 *   k_10 = c12 c20 - c10 c22;  k_11 = c00 c22 - c02 c20;  k_12 = c02 c10 - c00 c12
 *   k_20 = c10 c21 - c11 c20;  k_21 = c01 c20 - c00 c21;  k_22 = c00 c11 - c01 c10
 *   det = (c00 k_00 + c01 k_10) + c02 k_20;   I_ij = k_ij / det;   u_i = -((I_i0 t0 + I_i1 t1) + I_i2 t2)
 *   A_ij = (p_i0 I_0j + p_i1 I_1j) + p_i2 I_2j;   A_i3 = ((p_i0 u0 + p_i1 u1) + p_i2 u2) + s_i
 *   k', det' = the same nine cofactors and determinant of the linear part of A;   G_ij = k'_ji / det'
 * If the 16 doubles of `cur` compare equal to those of `prev` the result is exactly the identity record (1.0 and 0.0): a static
 * object costs no rounding.  RPT_ERR_INVALID for a value that is not finite, a bottom row other than 0 0 0 1 (either matrix), or a
 * det or det' that is 0 or not finite (in this order, and all but det' before the comparison of the matrices).  G is exact for rigid motions; where an object changes size between frames |G n| != |n| and
 * the normal test is correspondingly tighter or looser (such callers can set normal_tol = 0).
 *
 * With a table of m records set for the call (rpt_temporal_set_motion*), step 3 forms P_k = eye_k + s v_k (rounded once: the value
 * q_k contains without a table).  If id >= 1.0 && id <= double(m) (false for NaN), with o = uint32(id) - 1 (truncating) and
 * r = table + 24 o:
 *        P'_k = ((r[4k] P_0 + r[4k+1] P_1) + r[4k+2] P_2) + r[4k+3]
 *        n'_k = (r[12+3k] n_0 + r[13+3k] n_1) + r[14+3k] n_2
 * otherwise P' = P and n' = n: objects past the table, misses and foreign ids keep their places.  Then q_k = P'_k - eye'_k, the rest of
 * step 3 and qq as above; the normal test of step 4 uses e_k = h.n_k - n'_k; step 6 still stores the untransformed n, zc and id.
 * Without a table nothing differs.
 *
 * rpt_temporal_set_motion takes a HOST array of n_objects records and copies it: the caller may free or overwrite the array as soon
 * as the call returns.  Each of the 21 used doubles per record must be finite, else RPT_ERR_INVALID, before any device call.
 * records == NULL with n_objects == 0 clears the table; NULL with n_objects > 0 is RPT_ERR_INVALID.  rpt_temporal_set_motion_device
 * takes a caller-owned DEVICE table whose contents are trusted and which must stay unchanged until the consuming call's work is done.
 * The table is one-shot: the next rpt_temporal_accumulate_device, rpt_temporal_accumulate or rpt_temporal_frame_image that passes
 * its checks consumes it (the first frame after create or reset included, which looks nothing up); a refused call leaves it in
 * place, rpt_temporal_reset drops it, a second set before consumption replaces the first: a stale table is wrong for every later
 * frame, so it never persists.  The host variant's upload is ordered like every call of the accumulator: on the consuming call's
 * stream, behind the predecessor's event, so a set issued while an earlier call is still queued does not change what that call
 * reads.
 *
 * History clipping (flag RPT_TEMPORAL_CLIP).  The reprojection follows geometry: it cannot see that the LIGHTING of an unchanged
 * surface point has changed (the shadow of a moving object on a static floor, a light that moves), and blends the old lighting in for
 * up to max_history frames.  With the flag, the reprojected history colour is clamped to mean +- gamma . sigma of the CURRENT frame's
 * (2r + 1)^2 window around the pixel itself (not around the reprojected place), and a clipped pixel gives up most of its history
 * length.  Three settings live on the accumulator (rpt_temporal_set_clip): radius r 1..3, gamma finite and >= 0, clip_history 0..4096
 * (0: a clipped pixel keeps its length); anything else is RPT_ERR_INVALID, a NULL handle after that.  Defaults (1, 0.5, 1).  Host state
 * only, no device is touched; the settings persist across calls and across rpt_temporal_reset (a setting, not data, unlike the
 * one-shot motion table); they are read when a call with the flag passes its checks and ignored without the flag.
 * A new step between 4 and 5, only with the flag and B > 0.0, in the arithmetic of the other steps; fmax(a, b) here is a if
 * a >= b or b is NaN, else b, and fmin(a, b) is a if a <= b or b is NaN, else b (the operand that is not NaN; of two that compare
 * equal, the first):
 *        hc_k = C_k / B;  hl = L / B  (as step 5 forms them)
 *        Window dy = -r..r (outer), dx = -r..r (inner), p' = (x + dx, y + dy); pixels outside the image are skipped.  A pixel counts
 *        iff all three rgb[p']_k are finite (t - t == 0.0) and, with MATCH_ID, depth[p'][2] == id (false for NaN: a NaN id counts nothing).
 *        n += 1.0;  S_k += c_k;  Q_k += c_k c_k  with c = rgb[p'], all from +0.0.
 *        If n > 0.0:  m_k = S_k / n;  s_k = fmax(Q_k / n - m_k m_k, 0.0);  sd_k = sqrt(s_k)
 *                     lo_k = m_k - gamma sd_k;  hi_k = m_k + gamma sd_k;  hc'_k = fmin(fmax(hc_k, lo_k), hi_k)
 *                     clipped = some hc'_k != hc_k;  if clipped && clip_history > 0: hl = fmin(hl, double(clip_history))
 *        otherwise hc' = hc.
 * Step 5 continues with hc' and this hl.  hv is unchanged: the variance of a clipped pixel's history is NOT corrected (it describes
 * the history before the clamp).  There are no new outputs: a clipped pixel shows in d_out_len.  The motion path (P', n') is
 * untouched.  gamma = 0.5 over a 3 x 3 window also pulls history towards the local mean, which is a spatial blur. */
#define RPT_TEMPORAL_MATCH_ID 1u
#define RPT_TEMPORAL_CLIP 2u
#define RPT_TEMPORAL_MOTION_DOUBLES 24u
typedef struct rpt_temporal_params {
    uint32_t max_history;   /* 1..4096; 1 = no reuse */
    uint32_t flags;         /* RPT_TEMPORAL_MATCH_ID | RPT_TEMPORAL_CLIP */
    double depth_tol;       /* on SQUARED distances, relative; 0 = test off */
    double normal_tol;      /* on the distance of the normal planes; 0 = off */
} rpt_temporal_params;
int rpt_temporal_camera_record(const rpt_camera*, double out[13]);
typedef struct rpt_temporal rpt_temporal;
rpt_temporal* rpt_temporal_create(int device, uint32_t width, uint32_t height);
void rpt_temporal_destroy(rpt_temporal*);
int rpt_temporal_reset(rpt_temporal*);                 /* forget the history */
int rpt_temporal_frames(rpt_temporal*, uint32_t* n);   /* frames since create / reset */
int rpt_temporal_motion_record(const double cur[16], const double prev[16], double out[24]);
int rpt_temporal_set_motion(rpt_temporal*, const double* records, uint32_t n_objects);          /* host array, copied; one-shot */
int rpt_temporal_set_motion_device(rpt_temporal*, const void* d_records, uint32_t n_objects);   /* caller-owned device table; one-shot */
int rpt_temporal_set_clip(rpt_temporal*, uint32_t radius, double gamma, uint32_t clip_history);      /* RPT_TEMPORAL_CLIP's settings; persistent */
/* DEVICE pointers on the accumulator's device, hip_stream a hipStream_t (NULL = default stream).  d_out_rgb: width*height*3 doubles;
 * d_out_var, d_out_len: width*height doubles each, or NULL. */
int rpt_temporal_accumulate_device(rpt_temporal*, const rpt_temporal_params*, const rpt_camera*, const void* d_rgb, const void* d_var,
                                   const void* d_normal, const void* d_depth, void* d_out_rgb, void* d_out_var, void* d_out_len,
                                   void* hip_stream);
/* The same with host pointers, synchronous. */
int rpt_temporal_accumulate(rpt_temporal*, const rpt_temporal_params*, const rpt_camera*, const double* rgb, const double* var,
                            const double* normal, const double* depth, double* out_rgb, double* out_var, double* out_len);
/* The sequence counterpart of rpt_buffer_denoised_image: mean and variance of the buffer -> accumulate -> (with a denoiser: the a-trous
 * filter with the accumulated variance) -> color_bytes; synchronous, only width*height*3 bytes come back.  The planes are DEVICE
 * pointers; d_depth always, d_normal where normal_tol > 0 or the filter needs it (the accumulation reads it only with normal_tol > 0),
 * d_albedo as the filter needs it.  Without a denoiser the denoise parameters are ignored.  Buffer, denoiser and accumulator of different
 * devices or sizes: RPT_ERR_INVALID; fewer than 2 batches: RPT_ERR_STATE. */
int rpt_temporal_frame_image(rpt_temporal*, const rpt_temporal_params*, const rpt_camera*, rpt_buffer*, rpt_denoiser*,
                             const rpt_denoise_params*, const void* d_albedo, const void* d_normal, const void* d_depth,
                             uint8_t* out_rgb8);

/* ---- adaptive sampling by tile (an addition; the reference's Buffer::add_sample(x, y, ..), src/buffer.rs:25-29, at the
 * granularity of the render kernels' 32 x 32 tiles) ----
 * A buffer keeps, besides its full-frame batches, a count of EXTRA batches per tile (allocated and zeroed at the first tile batch):
 * a pixel p holds n_p = n_batches + extra[tile(p)] batches.  rpt_buffer_add_samples_tiles_device does rpt_buffer_add_samples_device's
 * arithmetic on the in-image pixels of the listed tiles only (DEVICE list of distinct ids in range; an id out of range is skipped)
 * and adds 1 to their counters.  rpt_buffer_batches keeps reporting the full-frame batches; rpt_buffer_tile_batches downloads
 * n_batches + extra per tile (tiles_x * tiles_y values, row-major; a smaller capacity is RPT_ERR_INVALID).
 * A buffer that never received a tile batch runs the kernels and gives the bits it always did.  One with extra batches:
 *   rpt_buffer_image: the window's sums, added in the same x-outer / y-inner order, divided by the SUM of the window's n_p
 *     (`count += samples[index].len()`, buffer.rs:75-93), then color_bytes;
 *   rpt_buffer_variance: its per-pixel expression with n = double(n_p), summed on the host in pixel order;
 *   rpt_buffer_mean_device (and with it rpt_buffer_denoised_image): both outputs with n = double(n_p); the check stays
 *     n_batches >= 2, the full-frame batches. */
int rpt_buffer_add_samples_tiles_device(rpt_buffer*, const void* d_rgb, const void* d_tiles, uint32_t n_tiles, void* hip_stream);
int rpt_buffer_tile_batches(rpt_buffer*, uint32_t* out /* tiles_x * tiles_y */, uint64_t capacity);
/* Tile errors and selection.  An order of fp64 operations, each rounded on its own (no fused multiply-add, IEEE division, no atomics,
 * no sqrt).  For tile t = (tx, ty), slot j = 32 ry + rx is pixel (32 tx + rx, 32 ty + ry).  A slot outside the image contributes
 * a_j = +0.0; otherwise, with m_k = sum_k / n and v exactly as rpt_buffer_mean_device computes them, n = double(n_p):
 *     y = (m_0 + m_1) + m_2;   a_j = v / (y y + floor floor).
 * The 1024 terms are reduced by halving strides: for s = 512, 256, .., 1: a_j = a_j + a_{j+s} for j < s.
 *     E_t = a_0 / double(in-image pixels of the tile):
 * the mean over the tile of the squared relative standard error of a pixel's mean, `floor` keeping dark pixels from dominating.
 * A tile is SELECTED iff E_t > threshold threshold (the square formed once on the host) and n_t < max_batches; a NaN error selects
 * nothing (such a tile would never converge).  rpt_buffer_refine_tiles writes the errors (to d_err, tiles_x * tiles_y doubles, if
 * given), then the selected ids in ascending order to d_tiles_out (DEVICE, capacity: every tile) and, after one synchronisation of
 * hip_stream, their number to *n_out (host): 4 bytes, the only read-back.  Both need 2 full-frame batches (RPT_ERR_STATE);
 * min_batches < 2, max_batches < min_batches, floor <= 0 (or not finite), a negative or NaN threshold: RPT_ERR_INVALID, like every
 * argument check before any device call. */
typedef struct rpt_adaptive_params {
    uint32_t spp_per_batch, min_batches, max_batches, _pad;   /* min_batches >= 2, max_batches >= min_batches */
    double threshold;   /* relative standard error of a tile's mean at which it stops; >= 0, +inf allowed */
    double floor;       /* > 0: added to the squared brightness, so that dark pixels do not dominate */
} rpt_adaptive_params;
int rpt_buffer_tile_errors_device(rpt_buffer*, double floor, void* d_err /* tiles_x*tiles_y doubles */, void* hip_stream);
int rpt_buffer_refine_tiles(rpt_buffer*, const rpt_adaptive_params*, void* d_tiles_out /* capacity: every tile */,
                            uint32_t* n_out /* host */, void* d_err /* or NULL */, void* hip_stream);
/* The loop, on the default stream, synchronous.  The buffer must be empty (RPT_ERR_STATE) and match the frame and the scene's device
 * (as for rpt_render_into_buffer); shard_count > 1 is RPT_ERR_INVALID.  Batches k = 0 .. min_batches - 1 are full-frame
 * rpt_render_into_buffer calls of spp_per_batch samples at sample_offset = k spp_per_batch.  Round k >= min_batches: refine; stop when
 * no tile is selected; otherwise a tile-list render of spp_per_batch samples at sample_offset = k spp_per_batch into the buffer's
 * stage, added to the listed tiles.  (A tile's error does not change while it is not sampled: the active set only shrinks and every
 * active tile holds k batches.)  A pixel of a tile that ended with n_t batches holds exactly the sums n_t full-frame batches would have
 * put there.  stats (or NULL): [0] rounds that rendered a tile list, [1] tile-batches rendered (min_batches tiles + the lists'
 * lengths), [2] tiles that ended at max_batches, [3] tiles. */
int rpt_render_adaptive(rpt_scene*, const rpt_camera*, const rpt_render_params*, const rpt_adaptive_params*,
                        uint64_t seed, rpt_buffer*, uint64_t stats[4] /* rounds, tile-batches rendered, tiles at max_batches, tiles */);

/* ---- adaptive sampling over a sequence: the loop above aimed at the error of the ACCUMULATED frame (an addition) ----
 * In a sequence the picture that is shown is the accumulation's: its variance is (1 - a)^2 hv + a^2 v_in, and with a long history
 * the frame's own variance counts for little of it.  Three calls let the adaptive loop see that: a preview of the accumulation, the
 * tile errors of planes, and the loop that uses both.  Tiles are the buffer's 32 x 32 tiles, ids ty * tiles_x + tx.
 *
 * rpt_temporal_preview_device: for the in-image pixels of the listed tiles, steps 1 - 5 of rpt_temporal_accumulate_device exactly as
 * defined above, the motion path and (with RPT_TEMPORAL_CLIP) the clipping step included -- the same kernel body, the same fp64
 * operations in the same order; the clipping window still reads rgb and depth of pixels in tiles that are not listed.  Step 6 does
 * not happen: no history record is written, the records do not swap, the stored camera record and rpt_temporal_frames are unchanged,
 * and a pending one-shot motion table is read but NOT consumed (the next accumulating call still consumes it; a host table is
 * uploaded once, by the first call that reads it, on that call's stream behind the predecessor's event, as promised above).  On an
 * accumulator that holds no frame: out = rgb, out_v = v_in, len = 1.0.  d_tiles is a DEVICE list of n_tiles distinct uint32 ids; an id
 * out of range is skipped; NULL with n_tiles == 0 means every tile; a list with n_tiles == 0 writes nothing.  Pixels outside the listed
 * tiles are not written in any output.  The argument checks, their order and the NULL rules are rpt_temporal_accumulate_device's; in
 * addition d_tiles == NULL with n_tiles > 0 is RPT_ERR_INVALID (after the planes' checks, before the handle's), and so is a list
 * longer than tiles_x * tiles_y (after the handle's).  A preview is ordered like every other call of the accumulator, through the
 * same event: it waits for its predecessor and its successor waits for it, whatever their streams.
 *
 * rpt_temporal_tile_errors_device: E_t of the tile errors above for each listed tile (NULL with 0: every tile), with the pixel's terms
 * taken from planes: y = (rgb_0 + rgb_1) + rgb_2;  a_j = var[p] / (y y + floor floor);  slots outside the image hold +0.0; the 1024
 * terms reduced by halving strides 512 .. 1; the result divided by double(in-image pixels).  Only the listed tiles' entries of d_err
 * (tiles_x * tiles_y doubles) are written; an id out of range is skipped.  The frame size is the accumulator's, of which nothing else
 * is read: the call is NOT ordered with the accumulator's other calls (order it on its stream).  floor finite and > 0, then the
 * pointers, then the list (as for the preview): RPT_ERR_INVALID.  On the planes rpt_buffer_mean_device wrote, the result is
 * rpt_buffer_tile_errors_device's of that buffer, bit for bit.
 *
 * rpt_render_adaptive_temporal: rpt_render_adaptive with the tile errors taken from the preview, on the default stream, synchronous.
 * Checks, all before any device call and in this order: rpt_render_adaptive's (NULL arguments, the adaptive parameters with
 * min_batches >= 2; then sample_offset + max_batches spp_per_batch must fit 32 bits; not sharded, the buffer's size and device); the
 * temporal parameters' and planes' (d_depth always, d_normal read only with normal_tol > 0), the NULL accumulator; buffer and
 * accumulator of one device and one size (RPT_ERR_INVALID); an empty buffer (RPT_ERR_STATE).
 * Batches k < min_batches are full-frame rpt_render_into_buffer calls at sample_offset + k spp_per_batch.  The active list starts as
 * every tile.  Round k >= min_batches: (1) rpt_buffer_mean_device; (2) the preview of those two planes over the active list;
 * (3) the tile errors of the preview's out / out_v over the active list; (4) the selection among the active list: a listed tile is
 * selected iff E_t > threshold threshold (false for NaN) and n_t < max_batches, the ids stay ascending, and their number comes back
 * through the round's one 4-byte read-back; (5) stop if nothing is selected; (6) otherwise a tile-list render of spp_per_batch samples
 * at sample_offset + k spp_per_batch, added to the listed tiles, which are the next round's active list.
 * A tile that left the active list is not evaluated again.  Without RPT_TEMPORAL_CLIP a pixel's preview depends on its own tile's
 * samples alone, so the accumulation that follows the loop returns in every tile exactly the out / out_v / len of that tile's last
 * preview (a tile that ended at max_batches got its last batch after its last preview: there the accumulation equals a preview
 * taken after the loop).  With clipping, a neighbour's later samples can move the window of a finished tile's edge pixels: its final error may
 * differ slightly from the one it stopped at.
 * The loop does NOT accumulate: history, frame count and pending motion table are as before the call; the caller finishes the frame
 * with rpt_temporal_frame_image or rpt_temporal_accumulate_device.  On an accumulator without a frame and with sample_offset 0 the
 * buffer and the stats are bit-identical to rpt_render_adaptive's.  stats as for rpt_render_adaptive. */
int rpt_temporal_preview_device(rpt_temporal*, const rpt_temporal_params*, const rpt_camera*, const void* d_rgb, const void* d_var,
                                const void* d_normal, const void* d_depth, const void* d_tiles, uint32_t n_tiles, void* d_out_rgb,
                                void* d_out_var, void* d_out_len, void* hip_stream);
int rpt_temporal_tile_errors_device(rpt_temporal*, const void* d_rgb, const void* d_var, double floor, const void* d_tiles, uint32_t n_tiles,
                                    void* d_err /* tiles_x*tiles_y doubles */, void* hip_stream);
int rpt_render_adaptive_temporal(rpt_scene*, const rpt_camera*, const rpt_render_params*, const rpt_adaptive_params*, uint64_t seed,
                                 uint32_t sample_offset, rpt_buffer*, rpt_temporal*, const rpt_temporal_params*, const void* d_normal,
                                 const void* d_depth, uint64_t stats[4]);

/* ---- particle systems (src/ode/particle_system.rs, particle_state.rs; MonomialSurface::closest_point*, src/shape/
 * monomial_surface.rs:126-178; the display positions of examples/marbles.rs:76-88) ----
 * The second of the two sequences the temporal code exists for, examples/marbles.rs, advances 25 marbles by rk4_integrate(state,
 * 1/16, 1/10000) per frame.  A handle holds one system's state (pos, vel: n x 3 doubles each) on a device and integrates it there.
 * The arithmetic is DEFINED here as an order of fp64 operations, each rounded on its own: no contraction, IEEE division, the
 * correctly rounded square root.  tests/particles_ref.py restates it in numpy and the device's state is compared bit for bit.  Juxtaposition
 * is a product; every bracket is a rounded operation; vector operations are componentwise.
 *
 *   length(v) = sqrt((v0 v0 + v1 v1) + v2 v2);  dot(a, b) = (a0 b0 + a1 b1) + a2 b2;  normalize(v)_k = v_k / length(v) (a division per
 *   component);  x.powi(4) = (x x)(x x), powi(3) = (x x) x, powi(2) = x x, powi(1) = x;  len.powi(-2) = 1.0 / (len len);
 *   len.powi(-5) = 1.0 / (len ((len len)(len len)));  max(a, b) = a if a >= b or b is NaN, else b (f64::max: the operand that is not NaN).
 *
 * closest_point(height, P) with n = 100, closest_point_precise with n = 10000:
 *   1. If length(P) < 1e-12: the result is P.
 *   2. px = sqrt(P0 P0 + P2 P2) (NOT the reference's f64::hypot: within an ulp of it where nothing over- or underflows, and numpy can
 *      restate it);  py = P1.
 *   3. For i = -n..n ascending:  xf = double(i) / double(n);  yc = height ((xf xf)(xf xf));  d = (px - xf)(px - xf) + (py - yc)(py - yc).
 *      The winner is the first candidate with d < best, scanning upward from best = 1e18 (strict: of equal distances the lowest i wins;
 *      a NaN distance or one >= 1e18 never wins).  If nothing wins, xf = -1.0.
 *   4. ux = P0 / px;  uz = P2 / px;  X = xf ux;  Z = xf uz;  s = X X + Z Z;  the result is (X, height (s s), Z).
 *      On the axis (px = 0, P1 != 0) that is NaN by IEEE rules, as in the reference.  Nothing is special-cased.
 *
 * RPT_PARTICLES_MARBLES, MarblesSystem{radius r}: the derivative of (pos, vel) is (vel, acc), with, for particle p, acc_p from (0, -1, 0):
 *   pair terms, over the partners q != p in ASCENDING order (the order in which the reference's loop, i ascending and j < i, touches
 *   particle p's accumulator):
 *     q < p:  d = pos_p - pos_q;  q > p:  d = pos_q - pos_p.   len = length(d);  dir_k = d_k / len.
 *     If len < 2.0 r:  c = (2.0 r - len) / r;  f_k = ((-dir_k) 5.0) c;  q < p: acc_p -= f;  q > p: acc_p += f;  then acc_p -= vel_p 0.5.
 *     (Coincident marbles: NaN, as IEEE says.)
 *   surface:  C = closest_point(height, pos_p);  v = pos_p - C;  L = length(v);  nrm_k = v_k / L;  ratio = (r - L) / r;  nv = dot(vel_p, nrm).
 *     If -0.1 < ratio && ratio < 0.0 ("band"):  acc_p -= (30.0 nrm_k)((nv nv) nv).  Else if ratio >= 0.0 ("push"):  acc_p += (100.0 nrm_k) ratio.
 *     NaN takes neither branch.
 *   table:  n = (0, 1, 0);  ratio = ((r - 0.06) - pos_p.y) / r;  nv = ((vel0 0.0 + vel1 1.0) + vel2 0.0).  Only if length(pos_p) > 0.1:
 *     band:  acc_p -= (20.0 n_k) nv;  push:  acc_p += (300000.0 n_k) ratio  -- on all three components, literally as written.
 *   air:  acc_p -= vel_p / 5.0.
 *   `height` is a parameter (the reference: 2.0); the exponent is the reference's hard-wired 4.
 * RPT_PARTICLES_GRAVITY, SolidGravitySystem: acc_p from (0, 0, 0); partners in the same order and with the same d, len and dir;
 *   s = 1.0 / (len len) - 0.0001 (1.0 / (len ((len len)(len len))));  f_k = dir_k s;  q < p: acc_p -= f;  q > p: acc_p += f.  (vel, acc).
 * RPT_PARTICLES_CIRCLE, SimpleCircleSystem: the derivative is ((-pos.y, pos.x, 0.0), (0, 0, 0)).
 *
 * rk4_integrate(state, time, step).  One step of size h, on all six values of every particle alike:
 *   k1 = f(S);  k2 = f(S + k1 (h / 2.0));  k3 = f(S + k2 (h / 2.0));  k4 = f(S + k3 h);  S = S + (((k1 + k2 2.0) + k3 2.0) + k4)(h / 6.0).
 * The time loop is  t = time; while (t > step) { one(step); t = t - step; } one(t);  -- in fp64 (1/16, 1/10000) is 624 steps of `step` and one
 * of 9.999999999924044e-05.  The host runs this loop for the step sequence and the device executes exactly that sequence, in launches
 * of at most 256 steps chained on the caller's stream (a shared machine never sees a long kernel: 256 steps of 256 particles take 0.1 s).
 *
 * Display positions (MARBLES only):  C = closest_point_precise(pos);  v = pos - C;  if length(v) < r 1.05:  pos = C + (normalize(v) r) 1.05;
 * then pos.y = max(pos.y, r - 0.06).
 *
 * Arguments, all checked before any device call and the parameters before the handle: n is 1..256; radius and height are finite, radius > 0
 * for MARBLES; time is finite and >= 0, step finite and > 0; a step sequence of more than 2^20 steps is RPT_ERR_INVALID;
 * rpt_particles_display_positions on a system that is not MARBLES is RPT_ERR_UNSUPPORTED.  State values that are not finite are
 * accepted: NaN propagates as defined.  The calls of one handle are ordered whatever their streams; handles share nothing with scenes
 * or with each other.  rpt_particles_integrate is asynchronous; the calls that move data to or from the host are synchronous.
 * Counters: 0 derivative evaluations, 1 pair contacts (len < 2r, once per pair and evaluation), 2 surface band, 3 surface push, 4 table
 * band, 5 table push, 6 kernel launches, 7 zero.  0..5 are part of the definition; the host functions report them with 6 = 7 = 0. */
#define RPT_PARTICLES_CIRCLE 0
#define RPT_PARTICLES_GRAVITY 1
#define RPT_PARTICLES_MARBLES 2
typedef struct rpt_particles_params {
    int32_t kind;    /* RPT_PARTICLES_* */
    uint32_t n;      /* 1..256 particles */
    double radius;   /* MARBLES: > 0; otherwise unused */
    double height;   /* MARBLES: the glass, y = height (x^2 + z^2)^2; otherwise unused */
} rpt_particles_params;
typedef struct rpt_particles rpt_particles;
rpt_particles* rpt_particles_create(int device, const rpt_particles_params*);   /* the state starts as zeros */
void rpt_particles_destroy(rpt_particles*);
int rpt_particles_set_state(rpt_particles*, const double* pos, const double* vel /* NULL = zeros */);   /* host, n*3 each, copied */
int rpt_particles_state(rpt_particles*, double* pos, double* vel);                                      /* synchronous; either may be NULL */
int rpt_particles_state_device(rpt_particles*, void** d_pos, void** d_vel);                             /* the handle's own arrays */
int rpt_particles_integrate(rpt_particles*, double time, double step, void* hip_stream);                /* asynchronous */
int rpt_particles_display_positions(rpt_particles*, double* out /* host n*3 */);                        /* MARBLES only, synchronous */
/* The same positions left on the device: asynchronous on hip_stream and ordered like rpt_particles_integrate (behind the handle's
 * earlier calls, ahead of its later ones, whatever their streams).  *d_out is the handle's own array of n*3 doubles, valid until the
 * handle is destroyed and rewritten by the next display call of either kind. */
int rpt_particles_display_positions_device(rpt_particles*, void** d_out, void* hip_stream);             /* MARBLES only, asynchronous */
int rpt_particles_counters(rpt_particles*, uint64_t out[8]);
/* Pure host functions, no device is touched: the same text run serially. */
int rpt_monomial_closest_point(double height, const double p[3], int precise, double out[3]);
int rpt_particles_derivative_host(const rpt_particles_params*, const double* pos, const double* vel, double* dpos, double* dvel,
                                  uint64_t counters[8] /* or NULL */);
int rpt_particles_integrate_host(const rpt_particles_params*, double* pos, double* vel, double time, double step, uint64_t counters[8]);
int rpt_particles_display_positions_host(const rpt_particles_params*, const double* pos, double* out);

/* ---- particle ensembles: many independent systems in one launch ----
 * A batch holds n_systems systems (1..4096, a stated limit as 256 is for n) of any kinds, sizes and parameters on one device: their
 * states concatenated in system order (pos, vel: sum(n) x 3 doubles each; system s starts at particle first[s] = n_0 + .. + n_(s-1))
 * and eight counters per system.  rpt_particles_batch_integrate advances every system by the same (time, step).  The result of system
 * s -- state, display positions, counters 0..5 at out[8 s ..] -- is DEFINED as that of rpt_particles_integrate_host (and
 * rpt_particles_display_positions_host) on that system alone, by the text above: the systems do not interact, and the device compares
 * bit for bit, whatever else is in the batch.
 *
 * On the device one workgroup integrates one system, block s of a launch system s, with local memory sized for the batch's largest n,
 * so that blocks of small systems share a compute unit.  R = compute units x blocks per compute unit (the occupancy query for the
 * kernel and the local memory actually launched) blocks run at once; a batch of more runs in rounds = ceil(n_systems / R) rounds, and a
 * launch lasts rounds x steps.  The host runs the time loop above for the step sequence and the device executes exactly that sequence in
 * launches of L = max(1, floor(256 / (rounds x 2))) steps; only the last launch carries the remainder step.  (The factor 2 is what blocks
 * that share a compute unit were measured to cost each other in the longest launch -- 1.98, four blocks of 256 particles on a compute
 * unit -- rounded up to a power of two: DESIGN.md section 4, "Ensembles".)  Counter 6 of every system is the number of kernel launches of the batch's calls so far, 7 is zero.
 * rpt_particles_batch_info: out[0] = R, 1 = rounds, 2 = L, 3 = bytes of dynamic local memory per block, 4 = the largest n, 5 = sum(n),
 * 6 = threads per block, 7 = lanes per particle in the closest-point scan (6 and 7: tuning, no effect on results).
 *
 * Arguments, all checked before any device call and the parameters before the handle: params is not NULL; n_systems is 1..4096; then
 * every system's parameters as rpt_particles_create checks them, in system order -- the first bad one is named in rpt_last_error
 * ("system 17: ..."); time and step as rpt_particles_integrate checks them; rpt_particles_batch_set_system_state's system is
 * < n_systems; rpt_particles_batch_display_positions on a batch in which any system is not MARBLES is RPT_ERR_UNSUPPORTED.  The calls of
 * one batch are ordered whatever their streams; batches share nothing with handles, scenes or each other.
 * rpt_particles_batch_integrate is asynchronous; the calls that move data to or from the host are synchronous. */
typedef struct rpt_particles_batch rpt_particles_batch;
rpt_particles_batch* rpt_particles_batch_create(int device, const rpt_particles_params* params /* [n_systems] */, uint32_t n_systems);
void rpt_particles_batch_destroy(rpt_particles_batch*);
int rpt_particles_batch_set_state(rpt_particles_batch*, const double* pos, const double* vel /* NULL = zeros */);   /* concatenated, sum(n) x 3 */
int rpt_particles_batch_set_system_state(rpt_particles_batch*, uint32_t system, const double* pos, const double* vel /* NULL = zeros */);
int rpt_particles_batch_state(rpt_particles_batch*, double* pos, double* vel);                    /* synchronous; either may be NULL */
int rpt_particles_batch_state_device(rpt_particles_batch*, void** d_pos, void** d_vel, void** d_first /* uint32 first[n_systems] */);
int rpt_particles_batch_integrate(rpt_particles_batch*, double time, double step, void* hip_stream);   /* asynchronous, one step sequence for all */
int rpt_particles_batch_display_positions(rpt_particles_batch*, double* out /* host sum(n) x 3 */);    /* every system MARBLES, synchronous */
int rpt_particles_batch_display_positions_device(rpt_particles_batch*, void** d_out /* sum(n) x 3, the batch's own */, void* hip_stream);   /* as rpt_particles_display_positions_device */
int rpt_particles_batch_counters(rpt_particles_batch*, uint64_t* out /* n_systems x 8 */);
int rpt_particles_batch_info(rpt_particles_batch*, uint64_t out[8]);

/* ---- moving spheres: a committed scene updated on the device (an addition; the reference rebuilds its Scene for every frame) ----
 * rpt_scene_commit makes a scene immutable with one exception: spheres whose transform is translate(c) * scale(r, r, r) can be moved to
 * new centres that lie in device memory, in both render modes, in scenes that are scanned and in scenes with a scene tree.  The radius
 * stays.  Out of scope: every other transform, cubes, meshes, monomial surfaces, lights, members of groups, a tree rebuild.
 *
 * The records of a moved sphere are DEFINED as the ones a fresh commit of the scene with the matrix (r 0 0 cx | 0 r 0 cy | 0 0 r cz | 0 0 0 1),
 * every zero +0.0, would upload, bit for bit: XfScan, XfShade and the pbox entry of the fp32 path; ObjRec::inv, ObjShade::nrm and the
 * CullBox of the reference-epsilon mode (and the cull32 box of its group of 32 records); the motion record is
 * rpt_temporal_motion_record(cur, prev) of the two matrices, so a sphere moved onto its own place (c == prev, component by component:
 * -0.0 equals 0.0) gets the exact identity record.  rpt_amd/csrc/scene_update_core.h states the operations; rpt_sphere_records_host
 * runs them once on the host (any output may be NULL; motion needs prev_centre, and is RPT_ERR_INVALID where
 * rpt_temporal_motion_record would refuse the pair): scan = XfScan (12 floats), shade = XfShade (12 floats, the object id r0.w left 0),
 * item_box = the sphere's own world box as the scene tree's build received it (lo, hi), pbox = the pbox entry (8 floats), inv =
 * ObjRec::inv, nrm = ObjShade::nrm, cull = the 32 bytes of its CullBox.
 *
 * rpt_scene_set_movable_spheres(scene, objects, n): after the commit; a second call replaces the list: it waits for a queued move,
 * and every sphere the earlier list has moved stays where it is -- a sphere that is listed again moves on from there (that centre is
 * the previous centre of its next motion record), one that is dropped keeps its moved records, and a refit bounds it where it is.
 * `objects` are indices of scene objects in rpt_scene_add_object order.  Refusals, in this order: a null scene, or a null list with
 * n > 0 (RPT_ERR_INVALID); a scene that is not committed (RPT_ERR_STATE); then for every entry in list order: an index that is not an
 * object's, or one listed before (RPT_ERR_INVALID); a group (RPT_ERR_UNSUPPORTED); any other shape that is not a sphere
 * (RPT_ERR_INVALID); the twin of a Light::Object (RPT_ERR_UNSUPPORTED: the light's sampler would stay behind); no transform, a non-zero
 * off-diagonal in the linear part, a diagonal that is not one value r, an r that is not finite and > 0, a bottom row other than
 * 0 0 0 1, a centre that is not finite, an r whose motion record has a zero or non-finite determinant (RPT_ERR_INVALID each);
 * then a library built without the kernels (RPT_ERR_UNSUPPORTED); last, for a scene with a scene tree: a leaf of the tree that holds
 * more than two listed spheres (RPT_ERR_UNSUPPORTED: the builder makes leaves of two items, and larger ones only where it finds no
 * split, as for spheres that coincide; list fewer of them or commit with a larger "scene_bvh_min"), and a tree that is not the one the
 * commit recorded -- a child that does not follow its parent, a leaf that is no primitive list, more than 32 heights, record counts
 * that are not the scene's (RPT_ERR_STATE: none of these can happen to a scene this library committed).  rpt_last_error names the object.
 * From this call on the scene reports no scan bound and no scan groups (rpt_scan_cull_counters, rpt_scan_cull_groups: lo[0] > hi[0],
 * n_groups = 0): diagnostics of the counters build that a moved sphere would make stale.  The scan JIT's scene shape stays valid (the
 * y-rotation bits of this matrix form do not depend on r or c).
 *
 * rpt_scene_move_spheres_device(scene, d_centres, d_offsets, d_motion, stream): asynchronous, ordered like a render of the scene --
 * behind every pass of the scene queued before it, on `stream`, ahead of every pass issued later, whatever their streams (renders,
 * feature passes, photon passes and every hook that takes the scene: each waits for the last move before its first launch).  The centre
 * of listed sphere k becomes d_centres[k] (n x 3 doubles), or d_centres[k] + d_offsets[k], one rounded add per component.  With
 * d_motion (n_objects x 24 doubles, which the caller has filled with identity records) the rows of the listed objects are written:
 * the motion from the centre of the previous call (or of the commit) to the new one.  Centres that are not finite give records that
 * are not: nothing on the device checks them.  A photon map built before the call is stale: rpt_photon_render_sample* is RPT_ERR_STATE
 * until rpt_photon_map_build or rpt_photon_map_from_records has run again.  Refusals: null scene (RPT_ERR_INVALID); not committed, no
 * list set (RPT_ERR_STATE); with n > 0: null d_centres (RPT_ERR_INVALID), built without the kernels (RPT_ERR_UNSUPPORTED).
 * rpt_scene_move_spheres is the host-array variant: it uploads, moves on the null stream, synchronises and downloads `motion`
 * (n_objects x 24, identity for the objects that are not listed).
 *
 * Scene tree (fp32 records, more than "scene_bvh_min" bounded records): the topology stays, the boxes are refitted bottom-up -- an
 * entry's bounds are the union of the own boxes of the items below it, and its box is those bounds under the padding the commit's
 * builder applies (1e-6 of the larger magnitude + 1e-30 per axis), so a move onto the committed centres reproduces the committed
 * boxes.  A refitted tree finds the hits a fresh commit finds; it is not the tree a fresh commit would build, and its quality decays
 * as the spheres travel ("Moving spheres"): a caller who sees that commits again.  Option "refit_per_height" = 1
 * runs the refit as one launch per height instead of one workgroup (same boxes).
 *
 * rpt_scene_movable_info: out[0] = a list is set, 1 = its length, 2 = scene-tree nodes refitted per move, 3 = their heights, 4 = cull32
 * groups recomputed per move, 5 = moves so far, 6 = bytes of the tables on the device, 7 = 1 in the reference-epsilon mode.
 * rpt_debug_scene_records downloads one array an update touches (synchronous; it waits for the device): *bytes is its size, `out` may be
 * NULL to ask for that alone.  The reference-epsilon arrays of a scene committed without the mode are RPT_ERR_STATE. */
enum { RPT_SCENE_RECORDS_SPH = 0, RPT_SCENE_RECORDS_SPH_SHADE = 1, RPT_SCENE_RECORDS_PBOX = 2,
       RPT_SCENE_RECORDS_TREE_NODES = 3,     /* the scene tree's two-box nodes, 64 bytes each (none: 0 bytes) */
       RPT_SCENE_RECORDS_RECS = 4, RPT_SCENE_RECORDS_SHADE = 5, RPT_SCENE_RECORDS_CULL = 6, RPT_SCENE_RECORDS_CULL32 = 7,
       RPT_SCENE_RECORDS_TREE_RAW = 8,       /* per node 16 floats: the unpadded bounds of its two entries (lo, -, hi, -) x 2; a list must be set */
       RPT_SCENE_RECORDS_TREE_ENTRIES = 9,   /* per entry 32 bytes: fixed lo, a, fixed hi, b (a = 0xFFFFFFFE: the union of node b's entries; else the fixed
                                                box united with movable spheres a and b, 0xFFFFFFFF = none) */
       RPT_SCENE_RECORDS_TREE_ORDER = 10,    /* the scene tree's local node numbers by height, children before parents */
       RPT_SCENE_RECORDS_ITEM_BOXES = 11,    /* per listed sphere 8 floats: its own box (lo, -, hi, -) */
       RPT_SCENE_RECORDS_TABLE = 12 };       /* per listed sphere 48 bytes: sphere record, object, fp64 record, 0 (uint32 each); radius; centre[3] */
int rpt_sphere_records_host(double radius, const double centre[3], const double prev_centre[3] /* or NULL */, float scan[12], float shade[12],
                            float item_box[6], float pbox[8], double inv[12], double nrm[9], void* cull /* 32 bytes */, double motion[24]);
int rpt_scene_set_movable_spheres(rpt_scene*, const uint32_t* objects, uint32_t n);
int rpt_scene_move_spheres_device(rpt_scene*, const void* d_centres /* n x 3 doubles */, const void* d_offsets /* n x 3 doubles or NULL */,
                                  void* d_motion /* n_objects x 24 doubles or NULL */, void* hip_stream);
int rpt_scene_move_spheres(rpt_scene*, const double* centres, const double* offsets_or_null, double* motion_or_null);
int rpt_scene_movable_info(rpt_scene*, uint64_t out[8]);
int rpt_debug_scene_records(rpt_scene*, uint32_t which, void* out, uint64_t capacity_bytes, uint64_t* bytes);

/* ---- photon mapping (next tier: src/photon.rs; config C4 = photon_point_query_beam_render) ----
 * `enum PhotonRenderKind` (src/photon.rs:631-639): point-point (photon_map_render), beam-point
 * (photon_point_query_beam_render, config C4) and beam-beam (photon_beam_query_beam_render). */
enum { RPT_PHOTON_MAP = 0, RPT_PHOTON_POINT_BEAM = 1, RPT_PHOTON_BEAM_BEAM = 2 };
/* Renderer::photon_render, first half (src/photon.rs:655-704): shoot `photon_count` photons of
 * power watts/photon_count from the first Light::Object (shoot_photon / trace_photon, :724-946),
 * build the surface and volume point maps and the per-photon gather radii (:204-247).  The map is
 * stored in the scene handle and replaced by the next build.  Photon i draws from the RNG stream
 * (seed, i, 0x80000000 + (i >> 32)). */
int rpt_photon_map_build(rpt_scene*, uint64_t photon_count, int32_t kind, double watts, uint64_t seed);
/* The same map built by several GPUs (one process each): the "Shooting photons" loop
 * (src/photon.rs:656-690) is sharded by photon index, the map is needed whole on every GPU.
 *   1. rpt_photon_shoot: shoot photons [rank*N/count, (rank+1)*N/count) of the N-photon map and keep
 *      their records on the device; n_out = {surface, volume} record counts of this shard.
 *   2. rpt_photon_records: device pointer + count of those records (RPT_PHOTON_RECORD_BYTES each,
 *      shooting order); the caller all-gathers them in rank order (RCCL), which reproduces the
 *      single-GPU arrays exactly because the blocks are contiguous.
 *   3. rpt_photon_map_from_records: build the maps of rpt_photon_map_build from device arrays
 *      (the gathered ones; they are read, not kept).  Invalidates the pointers of step 2.
 * The records may be any photons.  The volume map of kinds RPT_PHOTON_MAP and RPT_PHOTON_POINT_BEAM is searched with a stack of 64
 * pending nodes per lane: a map whose k-nearest tree has more than 64 inner nodes on a path (thousands of coincident photons next
 * to far outliers; a shot map has about 15) is refused with RPT_ERR_UNSUPPORTED, the depth in the message -- by both builds.
 * A record is twelve floats.  Surface records, and volume records of kinds RPT_PHOTON_MAP and RPT_PHOTON_POINT_BEAM:
 *   position xyz, 0;  direction xyz, 0;  power rgb, 0     (the build of kind 1 computes each volume photon's gather radius itself).
 * Volume records of kind RPT_PHOTON_BEAM_BEAM are beams:
 *   end xyz, radius;  start xyz, 0;  power rgb, 0
 * The beam's radius is read from the record: the camera pass uses it for the beam's own box and for the kernel's support (the shooting
 * pass writes the reference's constant 3 there, src/photon.rs:250-305).  Degenerate beams behave as in the reference: one of length 0
 * has no box and adds nothing; one whose line passes exactly through the eye makes every pixel NaN whose ray hits its box. */
#define RPT_PHOTON_RECORD_BYTES 48
int rpt_photon_shoot(rpt_scene*, uint64_t photon_count, int32_t kind, double watts, uint64_t seed,
                     uint32_t shard_rank, uint32_t shard_count, uint64_t n_out[2]);
int rpt_photon_records(rpt_scene*, int32_t which /* 0 surface, 1 volume */, void** d_records, uint64_t* n);
int rpt_photon_map_from_records(rpt_scene*, uint64_t photon_count, int32_t kind, const void* d_surface,
                                uint64_t n_surface, const void* d_volume, uint64_t n_volume);
/* [0] surface photons, [1] volume photons, [2] photons shot, [3] shooting us, [4] map build us, [5] blocks of the shooting
 * pass's grid, [6] blocks of the last reference-epsilon surface pass over this map (0: none yet). */
int rpt_photon_map_stats(rpt_scene*, uint64_t out[8]);
/* Test hook: which = 0 surface / 1 volume; out = n * 10 floats in shooting order:
 * position, direction (toward the previous vertex), power, gather radius (volume photons). */
int rpt_photon_map_download(rpt_scene*, int32_t which, float* out, uint64_t capacity_photons);
/* Renderer::photon_render, second half = get_color_with_photon_map over the frame
 * (src/photon.rs:706-716, 950-985; estimate_indirect :316-628) with `num_samples` camera
 * samples per pixel; same output convention, seed keying and sharding as rpt_render_sample. */
int rpt_photon_render_sample(rpt_scene*, const rpt_camera*, const rpt_render_params*, uint64_t gather_size,
                             uint64_t gather_size_volume, uint32_t num_samples, uint64_t seed,
                             uint32_t sample_offset, double* out_rgb);
int rpt_photon_render_sample_device(rpt_scene*, const rpt_camera*, const rpt_render_params*, uint64_t gather_size,
                                    uint64_t gather_size_volume, uint32_t num_samples, uint64_t seed,
                                    uint32_t sample_offset, void* d_out_rgb, void* hip_stream);

/* ---- frame exchange between the GPUs of one node (the loop being sharded is src/renderer.rs:158-171) ----
 * One process per GPU renders the 32x32 tiles it owns (rpt_render_params.shard_rank / shard_count) into a full-size
 * device frame; rank 0 assembles the image.  The exchange is a gather of the OWNED tiles over RCCL (xGMI), not a reduce
 * of whole frames: rank r packs its tiles (rpt_shard_tiles order; 32 x 32 pixels x 3 f64 each, pixels of a clipped tile
 * that lie outside the image are zero) and sends them to rank 0, which receives every rank's block in one ncclGroup and
 * scatters it into its frame.  The payload stays f64 -- the frame's own type -- so the assembled frame is bit-identical
 * to the one a single GPU renders (C5: 12.6 MB per rank instead of a 100 MB zero-padded frame per rank).
 * RCCL is loaded at run time (dlopen of librccl.so.1, the copy already in the process if there is one): the library
 * has no link-time dependency on it and single-GPU users never touch it. */
typedef struct rpt_comm rpt_comm;
#define RPT_COMM_ID_BYTES 128
/* ncclGetUniqueId: rank 0 calls it and hands the 128 bytes to the other ranks by any means (the launcher's store). */
int rpt_comm_unique_id(void* id_out);
/* ncclCommInitRank on `device` (collective over the n_ranks processes). */
int rpt_comm_create(const void* id, int rank, int n_ranks, int device, rpt_comm** out);
void rpt_comm_destroy(rpt_comm*);
int rpt_comm_rank(const rpt_comm*, int* rank, int* n_ranks);
/* Collective.  d_shard: this rank's frame (width*height*3 f64 on its device, as written by rpt_render_sample_device
 * with shard_rank = the communicator's rank); d_frame: on rank 0 the assembled frame (may be d_shard itself: the
 * received tiles are then written in place), ignored on the other ranks.  Everything is enqueued on hip_stream.
 * flags: RPT_GATHER_LOOPBACK makes rank 0 send its own tiles to itself through RCCL as well (self-test of the
 * transport with one rank; needs d_frame != d_shard to be observable). */
#define RPT_GATHER_LOOPBACK 1u
int rpt_gather_frame_device(rpt_comm*, uint32_t width, uint32_t height, const void* d_shard, void* d_frame,
                            uint32_t flags, void* hip_stream);
/* The photon maps' exchange step: the shooting loop (src/photon.rs:656-690) is sharded by photon index (rpt_photon_shoot) and
 * every rank builds the whole map, so the shot records (rpt_photon_records: RPT_PHOTON_RECORD_BYTES each) are all-gathered in
 * rank order -- contiguous blocks in rank order ARE the single-GPU arrays.  Collective.  d_local / n_local: this rank's records
 * (device); d_out: room for `capacity` records (device); n_per_rank (optional, n_ranks values) and n_total are filled on the host;
 * the call synchronises hip_stream once (the second all-gather is sized by the counts of the first).  If `capacity` is too
 * small the call fails with RPT_ERR_INVALID after filling n_total -- on every rank alike -- and can be repeated with room.
 * d_out = NULL with capacity = 0 exchanges the counts only (RPT_OK): how a caller learns the size to bring (a photon stores
 * one record per scattering event, so no multiple of the photon count bounds it). */
int rpt_allgather_records_device(rpt_comm*, const void* d_local, uint64_t n_local, void* d_out, uint64_t capacity,
                                 uint64_t* n_per_rank, uint64_t* n_total, void* hip_stream);
/* The packed layout (pure host function): tile_offsets[r] = first tile of rank r's block in the gathered buffer,
 * r = 0..n_ranks (tile_offsets[n_ranks] = tiles of the whole frame); a tile is 32*32*3 f64. */
int rpt_frame_pack_layout(uint32_t width, uint32_t height, uint32_t n_ranks, uint64_t* tile_offsets);
/* Pack / unpack on one device without any transport (what the exchange does on either side; test hooks):
 * d_packed holds rpt_shard_tiles(rank).count * 3072 f64. */
int rpt_frame_pack_device(uint32_t width, uint32_t height, uint32_t rank, uint32_t n_ranks, const void* d_frame,
                          void* d_packed, void* hip_stream);
int rpt_frame_unpack_device(uint32_t width, uint32_t height, uint32_t rank, uint32_t n_ranks, const void* d_packed,
                            void* d_frame, void* hip_stream);

/* ---- reference-epsilon mode: rpt_scene_set_option(scene, "epsilon_policy", 1) before rpt_scene_commit ----
 * The fp32 path replaces the reference's 1e-12 epsilons (src/renderer.rs:17, 348, 396, 420), which fp32 cannot resolve, by
 * scaled tolerances and a geometric twin test; its images are brighter than rpt's by the energy rpt loses to
 * self-intersections and near-miss shadow rejections.  A scene committed with epsilon_policy = 1
 * is rendered by a second, fp64 kernel whose arithmetic follows the reference literally instead: every object the generic
 * shape under its own Transformed matrices, in scene order, t_min = 1e-12, light visible iff |hit - dist| < 1e-12, f64
 * colours, no fused multiply-adds (only the objects a ray's padded fp32 box test keeps are evaluated -- the result is that of
 * the full scan bit for bit; option "f64_cull" = 0 runs the full scan).  Same entry points (rpt_render_sample*,
 * rpt_render_into_buffer), same RNG streams, same sharding; 4-5 times slower than the fp32 path (C3: 2.9 Gsamples/s).
 * Supported: spheres, cubes, planes, meshes (scanned triangle by triangle, or through a candidate tree: rpt_f64_mesh_tree_info), monomial surfaces, KdTree groups of them as objects and as
 * Light::Objects (nested at most three deep), all materials, lights and media, Environment::Color and Environment::Hdri.
 * Photon mapping (rpt_photon_map_build, rpt_photon_render_sample*): the shooting pass and the surface estimate's visibility rays run in
 * fp64 with the reference's tests (t_min = 1e-12; a gathered photon counts unless len > hit.time, src/photon.rs:357-361); the maps, the
 * k-nearest selection and the volume estimates are those of the fp32 records.
 * Refused with RPT_ERR_UNSUPPORTED: groups nested deeper; rpt_photon_shoot / rpt_photon_map_from_records (the 48-byte records do not
 * carry the photons' fp64 positions: every rank builds the whole map with rpt_photon_map_build).
 * Options of the mode: "f64_cull" (1; 0 = full scan, 2 = the counters build keeps the search limits), "f64_surf_batch"
 * (8: lanes of a wave that wait at a surface event in a medium before the wave runs the surface code).
 * "f64_photon_slice" (0 = automatic: as many whole chunks of 256 samples as keep the per-sample selections, (gather_size + 2) dwords
 * each, within 32 GB): samples per slice of the photon camera pass.  "photon_skip" bits 4096 / 16384: no visibility rays / visibility rays without
 * the search limit at the query point (diagnostics).
 * rpt_debug_epsilon_counters (option "counters" = 1): [0] closest-hit queries, [1] accepted hits, [2] accepted hits with
 * t < 1e-9 (1 + |origin|) -- a ray hitting the surface it starts on --, [3] shadow tests, [4] passed, [5] failed although
 * |hit - dist| < 1e-6 dist -- the light's own surface missed by rounding --, [6] camera samples, [7] path vertices; the
 * schedule: [8] objects evaluated in fp64 (all lanes), [9] wave-level evaluation rounds, [10] wave-level loop trips, [11] lanes
 * holding a path summed over the trips. */
int rpt_debug_epsilon_counters(rpt_scene*, uint64_t out[12]);
/* The candidate trees of the mode's large meshes.  Scene option "f64_mesh_tree_min" (64; read by rpt_scene_commit): every distinct
 * mesh of at least that many triangles gets a binary tree over its triangles, in the mesh's own space (0 = never, 1 = every mesh;
 * "f64_cull" = 0 disables the trees as well; a mesh that several shapes share has one tree; a mesh with needle triangles, whose
 * barycentric test is ill-conditioned, keeps the scan).  A tree only chooses which triangles a ray is tested against: the test is
 * the scan's, in fp64, and the result is that of the scan over all of them in given order -- the smallest accepted time, the
 * smallest index among the triangles that reach it -- bit for bit.  Node boxes: the fp64 box of the vertices, padded by 1e-5 of its
 * extent and of its coordinates, rounded outwards to fp32.  Depth limit and builder options as for the fp32 path's mesh trees
 * ("bvh_max_depth", "bvh_leaf_max", "bvh_sweep_below"); RPT_ERR_UNSUPPORTED from rpt_scene_commit only if a balanced tree is still too deep.
 * The render and rpt_intersect_batch_f64 walk the trees; scenes with a monomial surface or a group light, and the photon passes of
 * the mode, scan every triangle as before.
 * out: [0] meshes with a tree, [1] triangles under trees, [2] nodes, [3] levels below the root of the deepest tree, [4] bytes on the
 * device, [5] 1: the render and the batch query walk the trees, 0: they scan (no tree, or a flavour without the walk), [6] the same
 * for the photon passes (0), [7] the threshold the scene was committed with.  RPT_ERR_STATE: not committed, or an fp32 scene. */
int rpt_f64_mesh_tree_info(rpt_scene*, uint64_t out[8]);

/* ---- device self-test hooks (each runs the device function in a one-block kernel) ---- */
int rpt_debug_rng_u32(uint64_t seed, uint32_t pixel, uint32_t sample, uint32_t n, uint32_t* out);
int rpt_debug_material_sample_f(const rpt_material*, uint64_t n, const float* normals, const float* wos,
                                uint64_t seed, float* wi, float* pdf, int32_t* some);
int rpt_debug_material_bsdf(const rpt_material*, uint64_t n, const float* normals, const float* wos,
                            const float* wis, float* out_rgb);
/* sort_scan.h, the photon-map build's own device-wide primitives (host arrays in and out): the stable radix sort of 64-bit keys --
 * keys_out = the keys in ascending order, order_out[i] = input position of the i-th (equal keys keep their input order) -- and the
 * exclusive prefix sums of two u32 arrays with their 64-bit totals. */
int rpt_debug_radix_sort(uint64_t n, const uint64_t* keys, uint64_t* keys_out, uint32_t* order_out);
int rpt_debug_exclusive_scan2(uint64_t n, const uint32_t* a, const uint32_t* b, uint32_t* out_a, uint32_t* out_b, uint64_t totals[2]);
/* Reference-epsilon mode: the surface photons' positions as the shooting pass holds them (fp64, 3 per photon, shooting order -- the
 * order of rpt_photon_map_download(which = 0)); capacity in photons. */
int rpt_debug_photon_positions64(rpt_scene*, double* out, uint64_t capacity);
/* Scenes with the option "photon_keep_counts" = 1: the record counts of every photon of the last shooting pass (rpt_photon_shoot: of
 * this rank's photons; rpt_photon_map_build: of all), in shooting order; which = 0 surface, 1 volume; capacity in photons.  Their
 * exclusive prefix sums index each photon's first record in the shooting-order arrays.  RPT_ERR_STATE when nothing was kept. */
int rpt_debug_photon_chain_counts(rpt_scene*, int32_t which, uint32_t* out, uint64_t capacity);
/* ... and what the last camera pass (its last slice) handed from the k-nearest selection to the fp64 surface estimate:
 * dims = {owned pixel slots, gather_size + 2, samples}; out[slot][row][sample], rows: photon indices (sorted order), their number,
 * the squared distance of the farthest (float bits).  out may be null (dims only). */
int rpt_debug_photon_selections(rpt_scene*, uint32_t* out, uint64_t capacity_words, uint64_t dims[3]);
int rpt_debug_camera_rays(const rpt_camera*, const rpt_render_params*, uint64_t seed, uint32_t sample,
                          float* origins, float* dirs); /* one ray per pixel, width*height*3 each */
/* The camera sample of a render for every pixel of a width x height frame and one sample index: the render kernels' pixel -> NDC
 * mapping, their two jitter draws and cast_ray on stream (seed, pixel, sample) -> one ray per pixel (width*height*3 each) and
 * next_word[pixel], the stream's next word after cast_ray (fp32: may be null).  rpt_debug_camera_rays is the same without the word.
 * The _f64 twin runs the reference-epsilon mode's functions.  Neither reads a scene. */
int rpt_debug_camera_sample(const rpt_camera*, const rpt_render_params*, uint64_t seed, uint32_t sample,
                            float* origins, float* dirs, uint32_t* next_word);
int rpt_debug_camera_sample_f64(const rpt_camera*, const rpt_render_params*, uint64_t seed, uint32_t sample,
                                double* origins, double* dirs, uint32_t* next_word);
/* What a path vertex calls besides the above, one call per lane on the committed scene (host arrays in and out).
 * Shape::sample and Light::illuminate of Light::Object `light` (index into the scene's lights, RPT_ERR_INVALID for another kind)
 * at n positions: lane i seeds its stream with (seed, i, 0), runs the render kernels' sample_light_shape on one copy (v, nrm, pdf)
 * and their illuminate_object on another (intensity, wi, dist) -- the kernel instantiation (group lights or not) and the staging of the
 * light-triangle table in LDS are the render kernels' --, and next_word[i] is the stream's next word after illuminate_object.
 * The _f64 twin runs the reference-epsilon mode's functions; each refuses a scene of the other mode with RPT_ERR_STATE. */
int rpt_debug_light_sample(rpt_scene*, uint32_t light, uint64_t n, const float* positions, uint64_t seed, float* v, float* nrm,
                           float* pdf, float* intensity, float* wi, float* dist, uint32_t* next_word);
int rpt_debug_light_sample_f64(rpt_scene*, uint32_t light, uint64_t n, const double* positions, uint64_t seed, double* v, double* nrm,
                               double* pdf, double* intensity, double* wi, double* dist, uint32_t* next_word);
/* Environment::get_color of n directions (any length), each mode's env_color. */
int rpt_debug_env_color(rpt_scene*, uint64_t n, const float* dirs, float* rgb);
int rpt_debug_env_color_f64(rpt_scene*, uint64_t n, const double* dirs, double* rgb);
/* The distance sample of a vertex in the scene's medium (fp32 mode; RPT_ERR_INVALID without a medium): lane i on stream
 * (seed, i, 0) -> the sampled distance and the search limit the closest-hit query gets (+inf: the whole ray). */
int rpt_debug_medium_distance(rpt_scene*, uint64_t n, uint64_t seed, float* dmed, float* t_limit);
/* The shadow query and the light decision of the scan kernels (fp32 mode, scenes without a tree: RPT_ERR_UNSUPPORTED otherwise) for
 * Light::Object `light`, one segment per lane, 64 consecutive ones to a wave: from origins[i] along dirs[i] (used as given; the
 * render kernels pass the unit vector towards the light's sample) with the sample at dist[i].  out_flag[i]: the kernels would add
 * the light's term -- the closest hit in [t_min(origin), dist (1 + 1e-3)) is a record of the light's twin object at
 * t >= dist (1 - 1e-3); out_t[i]: that hit's parameter (dist (1 + 1e-3) where there is none).  The query takes the form the commit
 * chose for the light (option "shadow_scan"; rpt_shadow_scan_info), as in a render. */
int rpt_debug_shadow_test(rpt_scene*, uint32_t light, uint64_t n, const float* origins, const float* dirs, const float* dist,
                          int32_t* out_flag, float* out_t);
/* How the committed scene tests Light::Object `light`: out[0], out[1] = first and last hit code of its twin object's records
 * (out[0] > out[1]: they are no single range), out[2] = 1 if the scan kernels use the scan's shadow form for it (option
 * "shadow_scan" = 1, the scene is scanned, and the range is of one scanned kind -- not faces of the room shell), out[3] = the twin
 * object's index (0xFFFFFFFF: the light has none and is never visible). */
int rpt_shadow_scan_info(rpt_scene*, uint32_t light, uint32_t out[4]);
/* The scan kernels compiled for a scene's record counts (option "scan_jit": 0 never; 2 at the scene's first render; 1, the default: a
 * code object found in the cache is used, and one is compiled -- synchronously, a few seconds -- at the first launch of at least 2^27
 * camera samples).  Scenes rendered by the linear-scan kernels without group lights, monomial surfaces or counters are in scope; their
 * shape is the number of records of each scanned kind, the shell, the y-rotation masks, the tail cull and the medium -- not the
 * records' values.  The compiler is libhiprtc, opened at run time (RPT_HIPRTC_LIB: its path; else /opt/rocm/lib/libhiprtc.so, else libhiprtc.so); code objects are kept in the process and
 * under $RPT_JIT_CACHE (default ~/.cache/rpt_amd/jit; unwritable: memory only).  Frames are the AOT kernel's, bit for bit, and whatever
 * fails leaves the scene on the AOT kernel.  out[0]: state (RPT_SCAN_JIT_*), out[1]: where the code object came from
 * (RPT_SCAN_JIT_CACHE_*), out[2]: compile time in microseconds (0 on a hit), out[3], out[4]: its VGPRs and scratch bytes per lane,
 * out[5]: launches of the specialised kernel on this scene, out[6]: compiles in this process, out[7]: the AOT kernel's VGPRs.
 * text (optional): "<shape>\n<reason>" (an active scene: the compiler's version and path), truncated to text_capacity. */
#define RPT_SCAN_JIT_OFF 0           /* option scan_jit = 0 */
#define RPT_SCAN_JIT_IDLE 1          /* nothing compiled or loaded (yet): no render so far, or option 1 below its threshold without a cached object */
#define RPT_SCAN_JIT_ACTIVE 2        /* renders run the specialised kernel */
#define RPT_SCAN_JIT_FALLBACK 3      /* tried and failed: the reason says why */
#define RPT_SCAN_JIT_OUT_OF_SCOPE 4  /* a kernel flavour that is not specialised; nothing is attempted */
#define RPT_SCAN_JIT_CACHE_NONE 0
#define RPT_SCAN_JIT_CACHE_MEMORY 1  /* hit: compiled or loaded earlier in this process */
#define RPT_SCAN_JIT_CACHE_DISK 2    /* hit: read from the cache directory */
#define RPT_SCAN_JIT_CACHE_MISS 3    /* compiled for this scene */
int rpt_scan_jit_info(rpt_scene*, int64_t out[8], char* text, uint64_t text_capacity);
/* The second block of constants such a kernel is compiled with: what the code around the scans knows when the scene is committed.
 * text: "groups=<lights+tables+mats+small+pairs | none>;lights=<n>:<kind[/shape[/xf][/twin][/lo-hi]]>|...;mats=0x<mask of material
 * kinds>;medium_kind=<k>;hdri=<0|1>;pairs=0x<three common-slab bits per pair of boxes>", truncated to text_capacity; a group that is
 * not in effect for this scene (more than 4 lights, a table too large for LDS, more than 21 box pairs) says "view": its questions
 * are answered from the scene's records at run time.  Scenes of one shape and one structure share a code object; record values --
 * colours, transforms, boxes, light triangles -- are part of neither.  Empty for a scene outside the JIT's scope. */
int rpt_scan_jit_structure(rpt_scene*, char* text, uint64_t text_capacity);
/* Drops the process's code objects (not the cache directory's): the next scene of each shape looks on disk again.  Scenes that
 * already run a specialised kernel keep it.  Returns the number dropped. */
int rpt_scan_jit_forget(void);
/* The medium distance -ln(xi) / sigma_t of the draws xi = (2 k + 1) 2^-24, k = k0 .. k0 + n - 1 (k0 + n <= 2^23; needs no scene):
 * out_new as the render kernels compute it (the bare v_log_f32 and the two-word product with ln 2), out_guarded through __logf with
 * its denormal and infinity guards, which no such draw needs.  The two are the same bits for every k. */
int rpt_debug_distance_pair(float sigma_t, uint32_t k0, uint32_t n, float* out_new, float* out_guarded);
/* The draws whose form the kernels changed for speed (the generator's step with three-input xors, a width that carries the draw's
 * 2^-24, the roulette test on the raw word, the one-mask rejection test of the triangle sampler), next to the forms they replace
 * (needs no scene; n <= 2^20).  Lane i runs each form on its own copy of stream (seed, i, 0); word w of lane i is out[w * n + i],
 * 274 words per lane: [0, 64) the first 64 results of range(-1, 1) (float bits); [64, 128), [128, 192), [192, 256) of
 * range(-inv, inv) for inv = 1/64, 1/1024, 1/3000; [256, 258) bit j of the pair = the roulette decision (draw < 0.8) of draw j;
 * [258, 274) the top 23 bits of the first eight accepted pairs of the triangle sampler.  out_new and out_ref are the same bits. */
int rpt_debug_draw_forms(uint64_t seed, uint32_t n, uint32_t* out_new, uint32_t* out_ref);

/* The bounce of a path vertex, one case per lane on stream (seed, i, 0) (fp32 mode; needs no scene): the render kernels' own stage
 * (roulette or max_bounces, phase or BSDF sample, path weight) at a surface of material `m` with normal normals[i], reached along
 * rds[i] (not normalised by the hook), or -- medium_event != 0, which needs in_medium != 0 -- at a point of a medium with
 * scattering / extinction = albedo_med and colour medium_color[3].  in_medium chooses the kernels' instantiation for scenes with a
 * medium (roulette at surfaces too).  flag[i]: the path goes on with a non-zero weight; wi, k: its next direction and weight (zero
 * where the stage wrote none); next_word[i]: the stream's next word after the stage. */
int rpt_debug_bounce(const rpt_material* m, uint32_t max_bounces, uint32_t depth, int32_t in_medium, int32_t medium_event,
                     float albedo_med, const float* medium_color, uint64_t n, const float* normals, const float* rds, uint64_t seed,
                     int32_t* flag, float* wi, float* k, uint32_t* next_word);
/* The reference-epsilon mode's Material::sample_f on stream (seed, i, 0), then its Material::bsdf at the sampled direction (wi, pdf and f zero for
 * None); next_word[i]: the stream's next word after sample_f.  rpt_debug_material_bsdf_f64: its bsdf at given directions.  Neither
 * reads a scene. */
int rpt_debug_material_f64(const rpt_material* m, uint64_t n, const double* normals, const double* wos, uint64_t seed, int32_t* some,
                           double* wi, double* pdf, double* f, uint32_t* next_word);
int rpt_debug_material_bsdf_f64(const rpt_material* m, uint64_t n, const double* normals, const double* wos, const double* wis,
                                double* f);
#ifdef __cplusplus
}
#endif
#endif /* RPT_HIP_H */
