/*
 * rustray_hip.h — C ABI of the MI355X trace-loop replacement for rustray.
 *
 * This is the drop-in boundary for ONE path of the reference: the per-pixel /
 * per-sample trace loop that `RendererManager::start` spawns
 * (reference src/renderer.rs:105-172, worker body :267-315) and that calls
 * `Raytracing::render(x, y) -> PixelData` (reference src/raytracing.rs:275-427).
 * One `rr_render*` call replaces that whole cell-queue + thread-pool frame and
 * fills the four buffers `Run::apply_pixels` fills today
 * (reference src/run.rs:519-541: image RGBA8, normals, depth, objects).
 *
 * The reference has no FFI; its `Scene` is made of Rust trait objects
 * (src/scene.rs:69-83, src/shape/mod.rs:14-46).  The boundary therefore takes
 * a *flat scene*: plain arrays that a small host-side shim fills by walking
 * `Scene` (see INTEGRATION.md for the Rust shim).  Every struct below is POD,
 * little-endian, naturally aligned; all matrices are column-major 4x4 f32 as
 * nalgebra stores them.
 *
 * Ownership: the caller owns every input and output buffer.  The library
 * copies what it needs during rr_scene_create and owns only its handle and
 * device memory.  Nothing here calls back into the host.  No function aborts
 * or throws across the ABI: every entry point returns RR_OK (0) or a negative
 * rr_status, and rr_last_error() returns a thread-local message.
 */
#ifndef RUSTRAY_HIP_H
#define RUSTRAY_HIP_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Version of this header's struct layouts and entry points.  rr_scene_create refuses a flat scene that names another
 * version, and rr_abi_version() reports what the loaded library was built with, so a caller compiled against an older
 * header (round 1: a shorter rr_frame_stats, rr_scene_set_profiling) fails at the first call instead of being written
 * past its structs.  2: rr_frame_stats grew (level-1 timing, binning, multi-GPU exchange), rr_tuning, rr_abi_version.
 * 3: rr_frame_stats carries the level-1 share of the shade and shadow kernels too (one roofline per kernel build in bench.py).
 * rr_scene_update_lights, rr_scene_update_item_flags and rr_scene_add_textures came later without a change of any struct, so the
 * version stayed 3: a version-3 library may lack these three symbols (look them up, e.g. with dlsym, before relying on them).
 * rr_scene_add_meshes and rr_scene_set_items came later still, in the same way: a version-3 library may lack these two as well.
 * So did rr_trace_shadow_rays and rr_shade_rays (with rr_shadow_hit and rr_radiance, structs of their own), and after them the
 * device-buffer forms of the three ray queries: rr_trace_rays_device, rr_trace_shadow_rays_device and rr_shade_rays_device.
 * rr_surface_rays and rr_surface_rays_device (with rr_surface_hit, a struct of its own) came after those, in the same way.
 * rr_render_pixels and rr_render_pixels_device came after those, again without a change of any struct: a version-3 library may lack the two.
 * rr_render_pixel_parts and rr_render_pixel_parts_device came after those in the same way: a version-3 library may lack these two as well.
 * rr_refine_list_capacity, rr_refine_list_device, rr_render_adaptive and rr_render_adaptive_device came after those, again without a change
 * of any struct: a version-3 library may lack these four as well.
 * rr_refine_sublist_device, rr_render_adaptive_levels and rr_render_adaptive_levels_device came after those in the same way: a version-3
 * library may lack these three as well.
 * rr_render_pixel_prefix, rr_render_pixel_prefix_device, rr_render_adaptive_prefix and rr_render_adaptive_prefix_device came after those in
 * the same way: a version-3 library may lack these four as well.
 * rr_denoise_default_params, rr_denoise_records and rr_denoise_records_device (with rr_denoise_params, a struct of its own) came after
 * those, again without a change of any existing struct: a version-3 library may lack these three as well.
 * rr_accumulate_default_params, rr_accumulate_records and rr_accumulate_records_device (with rr_accumulate_params, a struct of its own)
 * came after those in the same way: a version-3 library may lack these three as well.
 * rr_motion_records and rr_motion_records_device came after those, without a struct of their own: a version-3 library may lack these two
 * as well.
 * rr_surface_pixels and rr_surface_pixels_device came after those in the same way: a version-3 library may lack these two as well.
 * rr_albedo_pixels and rr_albedo_pixels_device came after those in the same way: a version-3 library may lack these two as well.
 * rr_render_pixel_split, rr_render_pixel_split_device, rr_denoise_split_records and rr_denoise_split_records_device came after those in the
 * same way: a version-3 library may lack these four as well.
 * rr_accumulate_split_records and rr_accumulate_split_records_device came after those in the same way: a version-3 library may lack
 * these two as well.
 * rr_history_clamp_default_params, rr_accumulate_clamped_records and rr_accumulate_clamped_records_device (with rr_history_clamp_params, a
 * struct of its own) came after those, again without a change of any existing struct: a version-3 library may lack these three as well.
 * rr_accumulate_clamped_split_records and rr_accumulate_clamped_split_records_device came after those, without a struct of their own: a
 * version-3 library may lack these two as well.
 * rr_upsample_default_params, rr_upsample_records and rr_upsample_records_device (with rr_upsample_params, a struct of its own) came
 * after those, again without a change of any existing struct: a version-3 library may lack these three as well.
 * rr_upsample_albedo_records and rr_upsample_albedo_records_device came after those, without a struct of their own: a version-3 library
 * may lack these two as well. */
#define RR_ABI_VERSION 3u

typedef enum rr_status {
    RR_OK = 0,
    RR_ERR_INVALID_ARGUMENT = -1,  /* NULL pointer, bad index, bad size */
    RR_ERR_UNSUPPORTED = -2,       /* e.g. max_recursion above RR_MAX_RECURSION */
    RR_ERR_NO_DEVICE = -3,         /* no HIP device / HIP runtime failure at init */
    RR_ERR_DEVICE = -4,            /* a HIP call failed during the frame */
    RR_ERR_OUT_OF_MEMORY = -5,
    RR_ERR_CANCELLED = -6          /* *cancel became non-zero during the frame */
} rr_status;

/* Largest RaytracingConfig::max_recursion the device path accepts (reference default: 6, src/raytracing.rs:124).  A path node at
 * recursion depth d carries d in five bits of its shadow-ray records and its index (root 1, children 2k and 2k + 1) in 32: depth
 * max_recursion + 1 <= 31. */
#define RR_MAX_RECURSION 30u

/* Largest RaytracingConfig::samples accepted.  The reference computes the sub-sample cell size as
 * `(samples + 2).next_power_of_two() / 2` in u16 arithmetic (src/raytracing.rs:297), which overflows from 32767 samples on:
 * RR_MAX_SAMPLES_WITH_TABLE = 32766 is the reference's own limit, accepted whenever the caller passes its sub-sample table
 * (`sample_xy`, the recommended way: INTEGRATION.md).  The BUILT-IN table (sample_xy = NULL, rr_sample_table) is limited to
 * RR_MAX_SAMPLES = 16382, the last count of the cell size below that (cell_size 8192: 8192^2 = 67 M cells, 268 MB of host memory
 * while they are shuffled; the next cell size needs 1 GB). */
#define RR_MAX_SAMPLES_WITH_TABLE 32766u
#define RR_MAX_SAMPLES 16382u

/* Largest number of scene items (the reference has none: `items: Vec<..>`, src/scene.rs:69-83).  The top level of the acceleration
 * structure holds one item per leaf and shares a fixed traversal stack (39 entries per ray, in LDS) with the per-mesh trees: up to
 * 4 096 items it takes 12 levels of it, beyond that ceil(log2 n_items), which leaves 36 - ceil(log2 n_items) levels -- at least 16:
 * 524 288 triangles in any ONE mesh at worst, 134 M with up to 4 096 items -- to a mesh's own tree.  rr_scene_create answers
 * RR_ERR_UNSUPPORTED beyond either bound.  Scenes of 17 .. 512 items additionally get the packet form of the top level (coherent
 * packets test the items' boxes with one item per lane instead of walking the tree per ray); outside that range every ray walks
 * the tree -- same frame, bit for bit, at more node steps per ray.
 * Memory per INSTANCE of a mesh: a 208-B item record plus 32 B per triangle of the mesh (the world normals of its flat-shaded hits,
 * both signs, evaluated once per instanced triangle instead of per hit); the mesh itself -- vertices, attributes, tree: about 230 B
 * per triangle -- is shared by its instances.  The sum over all items of their meshes' triangle counts is limited to 2^31 (64 GB of
 * such normals): RR_ERR_UNSUPPORTED beyond. */
#define RR_MAX_ITEMS 1048576u

/* TextureType order of reference src/shape/mod.rs:633-643. */
enum {
    RR_TEX_BASE = 0,
    RR_TEX_AMBIENT_EMISSIVE = 1,
    RR_TEX_SPECULAR = 2,
    RR_TEX_NORMAL = 3,
    RR_TEX_ALPHA = 4,
    RR_TEX_ROUGHNESS = 5,
    RR_TEX_AMBIENT_OCCLUSION = 6,
    RR_TEX_REFLECTIVITY = 7,
    RR_TEX_COUNT = 8
};

/* One decoded image (image::DynamicImage after `.to_rgba()`,
 * reference src/shape/mod.rs:531, :586-589).  Row-major, top row first. */
typedef struct rr_texture {
    uint32_t width;
    uint32_t height;
    const uint8_t* rgba8; /* width*height*4 bytes */
} rr_texture;

/* All fields of `Material` that the trace loop reads
 * (reference src/shape/mod.rs:95-134; defaults :138-180). */
typedef struct rr_material {
    float ambient_color[3];
    float base_color[3];
    float specular_color[3];
    float alpha;
    float shininess;
    float reflectivity;
    float refraction_index;
    float normal_map_strength;
    float shadow_softness;
    float roughness;
    int32_t texture[RR_TEX_COUNT]; /* index into rr_flat_scene.textures, or -1 */
    uint8_t texture_filtering_nearest;
    uint8_t cast_shadow;
    uint8_t receive_shadow;
    uint8_t monte_carlo;
    uint8_t smooth_shading;
    uint8_t reflection_only;
    uint8_t backface_cullig; /* sic: the reference's field name */
    uint8_t _pad;
} rr_material;

/* Triangle mesh data of `Mesh` (reference src/shape/mesh.rs:10-21).  Meshes
 * are shared: several items may name the same mesh (instancing). */
typedef struct rr_mesh {
    const float* positions;         /* n_vertices * 3 */
    const uint32_t* indices;        /* n_triangles * 3 */
    const float* uvs;               /* n_uvs * 2, may be NULL */
    const uint32_t* uv_indices;     /* n_uv_faces * 3, may be NULL */
    const float* normals;           /* n_normals * 3, may be NULL */
    const uint32_t* normal_indices; /* n_normal_faces * 3, may be NULL */
    uint32_t n_vertices;
    uint32_t n_triangles;
    uint32_t n_uvs;
    uint32_t n_uv_faces;
    uint32_t n_normals;
    uint32_t n_normal_faces;
} rr_mesh;

enum { RR_ITEM_SPHERE = 0, RR_ITEM_MESH = 1 };

/* One scene item: `ShapeBasics` (reference src/shape/mod.rs:661-680) plus
 * the shape payload.  Item ORDER is semantically significant
 * (reference src/raytracing.rs:440-487) and must be Scene.items order. */
typedef struct rr_item {
    uint32_t kind;          /* RR_ITEM_SPHERE | RR_ITEM_MESH */
    uint32_t id;            /* ShapeBasics::id, reported as object_id */
    int32_t material;       /* `get_material()`: full material, textures included */
    int32_t material_cache; /* `get_material_cache_without_textures()`
                               (reference src/shape/mod.rs:769-772): must have every
                               texture slot = -1 */
    int32_t mesh;           /* index into meshes (kind == mesh), else -1 */
    float radius;           /* Ball radius (kind == sphere) */
    float trans[16];        /* ShapeBasics::trans, column-major */
    float trans_inv[16];    /* ShapeBasics::tran_inverse, column-major */
    float bbox_min[3];      /* ShapeBasics::b_box in LOCAL space */
    float bbox_max[3];
    uint8_t visible;
    uint8_t flip_normals;
    uint8_t _pad[2];
} rr_item;

enum { RR_LIGHT_DIRECTIONAL = 0, RR_LIGHT_POINT = 1, RR_LIGHT_SPOT = 2 };

/* `Light` (reference src/scene.rs:40-51). */
typedef struct rr_light {
    float pos[3];
    float dir[3];
    float color[3];
    float intensity;
    float max_angle; /* radians */
    uint32_t light_type;
    uint8_t enabled;
    uint8_t _pad[3];
} rr_light;

typedef struct rr_flat_scene {
    uint32_t abi_version; /* RR_ABI_VERSION */
    uint32_t n_items;
    uint32_t n_meshes;
    uint32_t n_materials;
    uint32_t n_textures;
    uint32_t n_lights;
    const rr_item* items;
    const rr_mesh* meshes;
    const rr_material* materials;
    const rr_texture* textures;
    const rr_light* lights;
} rr_flat_scene;

/* What the trace loop reads of `Camera` (reference src/camera.rs:19-40,
 * used at src/raytracing.rs:282-283, :340, :349, :355-356, :369-393). */
typedef struct rr_camera {
    uint32_t width;
    uint32_t height;
    float projection_inverse[16];
    float view_inverse[16];
} rr_camera;

/* `RaytracingConfig` by value (reference src/raytracing.rs:92-106) plus the
 * seed of the counter-based RNG that replaces the reference's un-seeded
 * `rand::thread_rng()` in `jitter` (src/raytracing.rs:616-618).  Pass the
 * EFFECTIVE config: JSON `config` blocks override the CLI in the reference
 * (src/scene.rs:180-198). */
typedef struct rr_config {
    uint64_t seed;
    float focal_length;
    float aperture_size;
    float fog_density;
    float fog_color[3];
    uint16_t samples;
    uint16_t max_recursion;
    uint8_t monte_carlo;
    uint8_t gamma_correction;
    uint8_t _pad[2];
} rr_config;

/* Output of one frame = what `Run::apply_pixels` stores per PixelData
 * (reference src/run.rs:519-541, PixelData src/raytracing.rs:57-70).
 * rgba8 is required; the aux pointers may be NULL.  All are row-major with
 * `width` pixels per row, y = 0 at the top. */
typedef struct rr_frame {
    uint8_t* rgba8;      /* w*h*4, alpha forced to 255 (src/run.rs:527) */
    float* normal;       /* w*h*3 */
    float* depth;        /* w*h */
    uint32_t* object_id; /* w*h */
} rr_frame;

/* A subset of the frame for one rank of a multi-GPU render.  The frame is cut
 * into tiles of tile_w x tile_h pixels, numbered row-major; this rank owns the
 * tiles with (tile_index % n_ranks == rank).  The rank's pixels are written
 * COMPACTLY, in tile order then row-major inside the tile (clipped at the
 * frame border), into buffers of rr_region_pixel_count() pixels.
 * n_ranks = 1, rank = 0 selects the whole frame (still in tile order). */
typedef struct rr_region {
    uint32_t tile_w;
    uint32_t tile_h;
    uint32_t n_ranks;
    uint32_t rank;
} rr_region;

/* Result of rr_pick (reference Raytracing::pick, src/raytracing.rs:237-273). */
typedef struct rr_pick_result {
    uint32_t hit;       /* 0 = None */
    uint32_t object_id; /* ShapeBasics::id */
    uint32_t item_index;
    float distance;
} rr_pick_result;

/* Per-frame work counters: one "ray" = one Raytracing::trace
 * call (reference src/raytracing.rs:429).
 * The ms_* fields of the kernels are sums of per-launch durations.  Where level 1 runs in stages (rr_scene_overlap_stages)
 * its shade and shadow launches run side by side on two streams: their durations overlap in time, each is the
 * launch's time while it shared the device, and their sum may exceed ms_total (first to last event of the frame on the
 * caller's stream).  Where such a level is one slice of the ray arena, its closest hits are traced stage by stage as well, on a
 * third stream beside the other two: launches_trace_closest_level1 then counts one launch per stage (not one per batch), and
 * ms_trace_closest_level1 -- with it ms_trace_closest -- is a sum of durations that overlap the shade and shadow launches' in
 * the same way.  The shadow launches of the level's last two stages run beside each other and beside the first launches of level 2
 * (whose shade and shadow launches join them where their shadow queue fits into the buffer at rest): those durations overlap too. */
typedef struct rr_frame_stats {
    uint64_t primary_rays;
    uint64_t secondary_rays; /* reflection + refraction */
    uint64_t shadow_rays;
    uint64_t shaded_hits;
    double ms_total;        /* device time of the whole frame */
    double ms_trace_closest;
    double ms_trace_shadow;
    double ms_shade;
    uint64_t launches_trace_closest;
    uint64_t launches_trace_shadow;
    uint64_t launches_shade;
    uint64_t batches;       /* device batches of primary samples the frame was cut into */
    uint64_t sliced_levels; /* depth levels whose children did not fit behind them in the ray arena at once */
    uint64_t binned_rays;   /* secondary rays that were re-ordered by (origin cell, direction octant) before being traced */
    double ms_binning;      /* device time of that re-ordering (kernel_timing); after rr_render_adaptive, rr_render_adaptive_levels and rr_render_adaptive_prefix, also of the launches that make their lists */
    double ms_trace_closest_level1;          /* the part of ms_trace_closest spent on depth level 1 (the primary rays); in stages: see above */
    uint64_t launches_trace_closest_level1;
    /* rr_render_multi only (on scenes[0]; zero after any other frame): how the per-device buffers reached scenes[0]'s device */
    uint32_t multi_devices;       /* handles that took part */
    uint32_t multi_peer_links;    /* handles whose buffers went device-to-device (peer access enabled both ways, or the same device) */
    uint32_t multi_staged_links;  /* handles whose buffers were staged through pinned host memory (no peer access between the devices) */
    uint32_t _pad;
    double ms_multi_exchange;     /* host wall time from the last device finishing its tiles to the frame being in `out` */
    /* the share of ms_shade / ms_trace_shadow spent in the level-1 BUILDS of those kernels (k_shade<true>; k_trace_shadow<true>: level 1 of a scene
     * whose shadow rays have fixed slots -- 17 .. 512 items, up to 32 enabled lights -- else 0: level 1 then runs the deeper levels' build), as
     * ms_trace_closest_level1 (ABI 3) */
    double ms_shade_level1;
    uint64_t launches_shade_level1;
    double ms_trace_shadow_level1;
    uint64_t launches_trace_shadow_level1;
} rr_frame_stats;

/* Execution knobs of the device path.  None of them changes a single output bit (fixed-point accumulation makes
 * the frame independent of batching, chunking and grouping); they exist for memory-constrained hosts, for tests
 * that force the slicing paths, and for profiling.  All zero = automatic.  The library reads NO environment
 * variables. */
typedef struct rr_tuning {
    uint32_t struct_size;        /* sizeof(rr_tuning) */
    uint32_t sample_group;       /* primary samples of one pixel per 64-ray packet: 0 = largest that divides `samples`, else 1, 2, 4 ... 64 */
    uint64_t queue_budget_bytes; /* ray-arena memory: 0 = a quarter of the free HBM, at most 64 GB */
    uint64_t shade_chunk_rays;   /* rays shaded per launch: 0 = 64 Mi (minimum 65536) */
    uint32_t kernel_timing;      /* non-zero: per-launch HIP events fill the ms_* fields of rr_frame_stats */
    uint32_t multi_force_staged; /* rr_render_multi, read from scenes[0]: non-zero stages every device's buffers through pinned host memory even
                                    where peer access exists (the path taken between devices WITHOUT peer access; lets one GPU exercise it) */
    uint64_t bin_min_rays;       /* deeper depth levels of at least this many rays are re-ordered by (origin cell, direction
                                    octant) before they are traced: 0 = never (measured: spawn order is already coherent) */
} rr_tuning;

typedef struct rr_scene rr_scene; /* opaque */

/* RR_ABI_VERSION of the loaded library (never fails). */
uint32_t rr_abi_version(void);

/* Number of HIP devices visible; 0 if none (never fails). */
int rr_device_count(void);

/* Thread-local description of the last failure on this thread ("" if none). */
const char* rr_last_error(void);

/* Validate and upload a flat scene to `device`; build the acceleration
 * structures (replaces Scene::update's BVH build, reference
 * src/scene.rs:1674-1688, and parry's per-TriMesh Qbvh, src/shape/mesh.rs:171). */
int rr_scene_create(const rr_flat_scene* scene, int device, rr_scene** out);
void rr_scene_destroy(rr_scene* scene);

/* Replace item transforms in place (animation / GUI edits between frames:
 * reference ShapeBasics::apply_mat, src/shape/mod.rs:748-753; Scene::apply_frame
 * src/scene.rs:1695-1713).  trans / trans_inv hold n_items * 16 floats.
 * All or nothing, as rr_scene_update_materials: an update that fails (a non-finite matrix anywhere: RR_ERR_INVALID_ARGUMENT;
 * a device or host failure part-way) leaves the scene rendering exactly what it rendered before the call.  Should putting
 * the old scene back fail as well, the scene is marked broken: every frame call (rr_render and its progressive forms,
 * rr_render_region_device, rr_render_multi, rr_pick, rr_trace_rays, rr_trace_shadow_rays, rr_shade_rays, rr_render_pixels) returns RR_ERR_DEVICE and says so in rr_last_error,
 * until an update of the same kind succeeds. */
int rr_scene_update_transforms(rr_scene* scene, const float* trans, const float* trans_inv);

/* Replace every material in place (GUI edits between frames: reference Material::apply_diff, src/shape/mod.rs:182-242,
 * driven from src/run.rs:1132-1133).  `materials` holds the same n_materials records, in the same order, as the
 * flat scene the handle was created from (full materials and material caches alike); texture slots may name any
 * texture uploaded at creation.  Meshes, acceleration structures and texture images are not touched.  A failed update
 * leaves the scene as it was (see rr_scene_update_transforms). */
int rr_scene_update_materials(rr_scene* scene, const rr_material* materials, uint32_t n_materials);

/* The edits below, like the two above, leave the handle rendering bit for bit what a handle freshly created from the edited flat
 * scene renders (every frame call, rr_pick, rr_trace_rays, rr_trace_shadow_rays, rr_shade_rays, rr_render_pixels, the counters of rr_frame_stats).  Each takes the scene's lock, waits for
 * frames still in flight on the device (rr_render_region_device) before it overwrites what they read, and returns
 * RR_ERR_INVALID_ARGUMENT when called from on_pass of the same scene.  Every handle that takes part in a multi-GPU frame must
 * receive the same edits. */

/* Replace the whole light list (the GUI's light "+", edits and "delete": reference src/run.rs:1294-1409).  n_lights may differ
 * from the count at creation and may be 0 (lights may then be NULL); a light type beyond RR_LIGHT_SPOT is refused, as by
 * rr_scene_create.  Order is semantic: a light's index is the RNG stream of its shadow jitter, disabled lights keep their slot, and
 * deleting a light shifts the streams of the lights after it (as Vec::remove does in the reference).  All or nothing, as
 * rr_scene_update_transforms; a scene broken by a failed roll-back refuses frames until a light update succeeds. */
int rr_scene_update_lights(rr_scene* scene, const rr_light* lights, uint32_t n_lights);

/* Set ShapeBasics::visible and flip_normals of every item (the GUI's "Visible" and "flip normals" checkboxes, reference
 * src/run.rs:1464-1489): n_items must equal the scene's item count, both arrays are required, a value is 0 or non-zero.  Hidden
 * items keep their place in the acceleration structure (they cost traversal, not hits); nothing is rebuilt.  Later material updates
 * keep these values.  All or nothing; a scene broken by a failed roll-back refuses frames until an item flag update succeeds. */
int rr_scene_update_item_flags(rr_scene* scene, const uint8_t* visible, const uint8_t* flip_normals, uint32_t n_items);

/* Append images to the scene's texture list (a material's texture "+", reference src/run.rs:936-947); *first_index receives the
 * index of the first new one.  Textures are checked as by rr_scene_create.  The existing images keep their indices; the new ones
 * take the indices (and layout) a scene created with the longer list gives them, and are used once a following
 * rr_scene_update_materials names them.  Adding 0 textures changes nothing.  A failure leaves the scene as it was.  Texture memory
 * never shrinks: images no material names any more stay resident until the scene is destroyed. */
int rr_scene_add_textures(rr_scene* scene, const rr_texture* textures, uint32_t n_textures, uint32_t* first_index);

/* Append meshes to the scene's mesh list (the GUI's "add ground plane", reference src/scene.rs:1564-1578, brings a mesh the scene
 * does not hold yet); *first_index receives the index of the first new one.  Meshes are checked as by rr_scene_create and their trees
 * built for the scene's current share of the traversal stack.  The resident meshes keep their indices and their place; the new
 * ones take the indices (and layout) a scene created with the longer list gives them.  Nothing is rendered from them until a
 * following rr_scene_set_items names them.  Adding 0 meshes changes nothing.  A failure leaves the scene as it was.  Meshes are
 * never removed: a mesh no item names stays resident, on the device and as the scene's host copy of its arrays, until the scene
 * is destroyed. */
int rr_scene_add_meshes(rr_scene* scene, const rr_mesh* meshes, uint32_t n_meshes, uint32_t* first_index);

/* Replace the whole item list AND the whole material list, together (items name materials by index): the GUI's object "delete",
 * "add ground plane" and "add environment sphere" (reference src/scene.rs:1602-1620, :1564-1578).  Any item count from 0 to
 * RR_MAX_ITEMS, in any order; an item may name any resident mesh (rr_scene_create, rr_scene_add_meshes), a material any resident
 * texture (rr_scene_create, rr_scene_add_textures); every check and limit of rr_scene_create applies.  Afterwards
 * rr_scene_update_materials / _transforms / _item_flags expect the new counts.  Resident meshes, their trees and the texture images
 * stay as they are, and items whose transform, mesh and flags did not change keep what was derived for them, so the cost follows
 * the edit and not the scene -- with one exception: the per-mesh trees share the traversal stack with the top level, whose share
 * depends on the item count below 14 and above 4096 items; an edit that changes the share rebuilds every mesh's tree (from the
 * scene's host copies), and returns RR_ERR_UNSUPPORTED when a mesh no longer fits.  A failure leaves the scene as it was: the new
 * state is built beside the old one and replaces it last.  A scene that a failed update of another kind left broken (see
 * rr_scene_update_transforms) refuses this call as it refuses frames. */
int rr_scene_set_items(rr_scene* scene, const rr_item* items, uint32_t n_items, const rr_material* materials, uint32_t n_materials);

/* Compatibility switches: behaviours of EARLIER reference binaries that the source at HEAD no longer has.  Default 0 = HEAD.
 * RR_COMPAT_OCCLUDER_ALPHA_SHADOWS: a shadow is attenuated by the OCCLUDER's material.alpha, where HEAD takes the
 * receiver's (`shadow_source_alpha = material.alpha`, src/raytracing.rs:898).  That is what the binary behind the 2022-05
 * README renderings did (tests/test_ref_shots.py: with it the product matches those renderings over the whole frame);
 * it exists so that the shipped kernels can be checked against the only outputs the reference holds. */
#define RR_COMPAT_OCCLUDER_ALPHA_SHADOWS 1u
int rr_scene_set_compat(rr_scene* scene, uint32_t flags);

/* Execution knobs (see rr_tuning). */
int rr_scene_set_tuning(rr_scene* scene, const rr_tuning* tuning);
int rr_scene_get_tuning(const rr_scene* scene, rr_tuning* tuning);

/* The reference's per-pixel sub-sample table (src/raytracing.rs:290-313):
 * cell_size^2 cells shuffled with StdRng::seed_from_u64(0), truncated to
 * `samples`.  Writes samples*2 uint16 (x_i, y_i) and *cell_size. */
int rr_sample_table(uint16_t samples, uint16_t* xy_out, uint32_t* cell_size_out);

/* Render one whole frame into HOST buffers (synchronous).
 * sample_xy: samples*2 uint16 from the host's own rand, or NULL for the
 * built-in table.  cancel: optional flag polled between device launches. */
int rr_render(rr_scene* scene, const rr_camera* camera, const rr_config* config,
              const uint16_t* sample_xy, const rr_frame* out, const volatile int* cancel);

/* The same frame on SEVERAL GPUs from one host process, as the reference host is one process (src/renderer.rs:105-172).
 * scenes[i] is a handle created with rr_scene_create(scene, device_i, ...) from the SAME flat scene; handle i renders
 * the 32x8-pixel tiles with (tile_index % n_scenes == i) on its device (one host thread per device inside the call),
 * the compact per-device buffers are copied peer-to-peer into scenes[0]'s device, de-interleaved there and copied to
 * `out` (host buffers, as rr_render).  The frame is bit-identical to rr_render's for any n_scenes.  Two handles may sit
 * on the same device (a rehearsal on one GPU).  Peer access between scenes[0]'s device and every other device is
 * checked (hipDeviceCanAccessPeer) and enabled both ways on first use; a pair without it is staged through pinned host
 * memory instead, and rr_scene_last_stats(scenes[0]) says which way each handle's buffers went.  Every device works on
 * a non-blocking stream of its own.  Handles are locked in address order: concurrent calls that share handles, in any
 * order, serialise instead of deadlocking. */
int rr_render_multi(rr_scene* const* scenes, uint32_t n_scenes, const rr_camera* camera, const rr_config* config,
                    const uint16_t* sample_xy, const rr_frame* out, const volatile int* cancel);

/* Diagnostic: the order in which rr_render_multi locks `scenes` (address order), as indices into the caller's array.
 * Looks at the pointer values only, never through them (tests/test_abi.py checks the order without a GPU). */
int rr_multi_lock_order(rr_scene* const* scenes, uint32_t n_scenes, uint32_t* order_out);

/* Progressive form of rr_render.  Stands in for the progressive fill the reference shows while a frame renders:
 * Run::apply_pixels drains the PixelData channel every GUI tick (src/run.rs:506-545) and RendererManager::stop
 * (src/renderer.rs:174-198) ends the frame early.  The frame is rendered in at least `min_passes` device batches of
 * whole sample slices (every pixel, a subset of the samples); after each batch but the last, the host buffers of
 * `out` hold the frame resolved over the samples finished so far (colour, normal and depth are means; object_id is
 * only final after the last batch) and `on_pass(user, samples_done, samples_total)` is called on the calling
 * thread.  A non-zero return stops the frame: the call returns RR_ERR_CANCELLED and `out` keeps the last preview.
 * The finished frame is bit-identical to rr_render's.
 * Inside on_pass the frame still holds the scene: rr_scene_last_stats on that scene is allowed and reports the passes finished so far
 * (the work counters; timings come with the finished frame); every other call on that scene returns RR_ERR_INVALID_ARGUMENT (re-entry),
 * and the scene must not be destroyed there.  Calls on other scenes are not restricted. */
typedef int (*rr_pass_fn)(void* user, uint64_t primary_samples_done, uint64_t primary_samples_total);
int rr_render_progressive(rr_scene* scene, const rr_camera* camera, const rr_config* config,
                          const uint16_t* sample_xy, const rr_frame* out, uint32_t min_passes,
                          rr_pass_fn on_pass, void* user, const volatile int* cancel);

/* The frame filled in TILE BY TILE instead: every pixel is final when it appears, as in the reference's GUI (shuffled 2x2-pixel cells, each
 * rendered with all of its samples: src/renderer.rs:125-172).  Pass k of n_passes (0 = 16; at most the number of tiles) renders the 32x8-pixel
 * tiles with (tile_index % n_passes == k), an interleaved subset of the frame, and after each pass but the last the host buffers of `out` hold the
 * frame so far (pixels not rendered yet are zero) and `on_pass(user, samples_done, samples_total)` is called on the calling thread; a non-zero
 * return stops the frame (RR_ERR_CANCELLED, `out` keeps what was finished).  A frame cancelled before its first pass leaves every buffer of
 * `out` zero.  The finished frame is bit-identical to rr_render's; rr_scene_last_stats reports the sums over the passes (inside on_pass:
 * over the passes so far).  What on_pass may call is as for rr_render_progressive. */
int rr_render_progressive_tiles(rr_scene* scene, const rr_camera* camera, const rr_config* config,
                                const uint16_t* sample_xy, const rr_frame* out, uint32_t n_passes,
                                rr_pass_fn on_pass, void* user, const volatile int* cancel);

/* Number of pixels `region` owns in a width x height frame. */
uint64_t rr_region_pixel_count(uint32_t width, uint32_t height, const rr_region* region);

/* Render `region` of the frame into DEVICE buffers (HIP device pointers on the
 * scene's device) holding rr_region_pixel_count() pixels, compact, in region
 * order.  Work is enqueued on `hip_stream` (a hipStream_t, NULL = the default
 * stream); the call returns once everything is enqueued or, when the frame
 * needs more than one batch of samples, after the last batch has been
 * enqueued (earlier batches are awaited).  The caller synchronises the stream. */
int rr_render_region_device(rr_scene* scene, const rr_camera* camera, const rr_config* config,
                            const uint16_t* sample_xy, const rr_region* region,
                            const rr_frame* out_device, void* hip_stream,
                            const volatile int* cancel);

/* Scatter a compact region buffer back to full-frame layout, on device.
 * Used by rank 0 after the gather; src holds the concatenated per-rank
 * compact buffers in rank order. elem_bytes = bytes per pixel (4, 12, 4, 4). */
int rr_deinterleave_device(uint32_t width, uint32_t height, uint32_t tile_w, uint32_t tile_h,
                           uint32_t n_ranks, uint32_t elem_bytes, const void* src_device,
                           void* dst_device, int device, void* hip_stream);

/* The same for the gathered PACKS of a multi-rank frame, all buffers in one launch and without a concatenation pass: rank r's pack
 * (a byte buffer) starts at packs + r * pack_stride and holds, for output buffer k (0 rgba8, 1 normal, 2 depth, 3 object id), that
 * rank's compact pixels at section_offset[k] (elem_bytes[k] bytes per pixel; 0 = the buffer is absent, dst[k] ignored).  dst[k]: the
 * frame-order buffer.  This is what rank 0 runs on the target of its one gather per frame (rustray_amd/renderer.py: TiledFrame). */
int rr_deinterleave_packed_device(uint32_t width, uint32_t height, uint32_t tile_w, uint32_t tile_h, uint32_t n_ranks,
                                  const void* packs_device, uint64_t pack_stride, const uint64_t* section_offset,
                                  const uint32_t* elem_bytes, void* const* dst_device, int device, void* hip_stream);

/* Single-ray query at the pixel centre (reference src/raytracing.rs:237-273). */
int rr_pick(rr_scene* scene, const rr_camera* camera, int x, int y, rr_pick_result* out);

/* Closest-hit queries for a batch of caller-supplied rays: Raytracing::trace(ray, false, false, depth)
 * (reference src/raytracing.rs:429-490) for each of them, the generalisation of rr_pick (which is one such query for
 * a pixel-centre ray).  origins / directions: n * 3 floats (host); directions are used as given (trace does not
 * normalise).  `depth` is the recursion depth the candidate filter sees: reflection-only items are candidates for
 * depth > 1 only (:454).  out[i].item_index = 0xffffffff when nothing is hit.
 * Memory: this call and rr_trace_shadow_rays are rr_trace_rays_device / rr_trace_shadow_rays_device (below) behind a staging copy.
 * For the duration of the call they hold the caller's arrays and the answers on the device (12 + 12 + 20 B per ray, 4 more with
 * limits); the packed records and raw hits are the handle's, as for the device forms: 56 B per ray (48 for a shadow query) of the
 * largest such query so far, kept until rr_scene_destroy. */
typedef struct rr_ray_hit {
    uint32_t hit;        /* 0 = None */
    uint32_t item_index;
    uint32_t object_id;  /* ShapeBasics::id of the item */
    uint32_t face_id;    /* as Shape::intersect reports it: triangle index, + n_triangles for back faces; 0 for spheres */
    float distance;      /* toi */
} rr_ray_hit;
int rr_trace_rays(rr_scene* scene, const float* origins, const float* directions, uint32_t n, uint32_t depth, rr_ray_hit* out);

/* Shadow queries for a batch of caller-supplied rays: the other form of Raytracing::trace, trace(ray, true, true, depth)
 * (reference src/raytracing.rs:429-490), followed by the light loop's `in_light = toi > len` (:883-892) -- what a frame asks for
 * every shadow ray, answered by the walk the frames use.  For ray i let r = trace(ray_i, true, true, depth): the first ITEM in
 * (bbox distance, item index) order that is hit at all (shadow casters only, balls never solid), with that item's nearest hit.
 *   max_distance == NULL (a directional light):  occluded = r.is_some()
 *   max_distance[i] = len (a point or spot light at that distance):  occluded = r.is_some() && !(r.toi > len); a NaN toi (a ball
 *   whose arithmetic overflows, a non-finite ray) therefore counts as occluded, as in the reference.
 * When occluded, item_index / object_id / face_id / distance are those of r.  When not, the record is {0, 0xffffffff, 0, 0, 0}:
 * the item of a ray that is lit BECAUSE its first item lies beyond the distance is not reported.
 * origins / directions: n * 3 floats (host), directions used as given; max_distance: n floats or NULL, each >= 0 (NaN or a
 * negative value: RR_ERR_INVALID_ARGUMENT, rr_last_error names the first offending index; +inf means "no limit" for that ray);
 * `depth`: what the candidate filter sees, 1 .. 255, as for rr_trace_rays.  n == 0 returns RR_OK and touches nothing;
 * n > 0x7fffff00: RR_ERR_UNSUPPORTED.  The attenuation of a shadow (receiver alpha, alpha maps) needs a receiver and stays
 * inside the frame. */
typedef struct rr_shadow_hit {
    uint32_t occluded;   /* 1 = the reference's `!in_light` for this ray and distance */
    uint32_t item_index; /* the deciding item; 0xffffffff when not occluded */
    uint32_t object_id;  /* its ShapeBasics::id; 0 when not occluded */
    uint32_t face_id;    /* as Shape::intersect reports it (triangle index, + n_triangles for back faces; 0 for spheres) */
    float distance;      /* toi of the deciding item's nearest hit (may be NaN: an overflowing ball); 0 when not occluded */
} rr_shadow_hit;         /* 20 bytes */
int rr_trace_shadow_rays(rr_scene* scene, const float* origins, const float* directions, const float* max_distance,
                         uint32_t n, uint32_t depth, rr_shadow_hit* out);

/* Radiance queries for caller-supplied rays: Raytracing::get_color_depth_normal_id(scene, ray, 1) (reference
 * src/raytracing.rs:720-998), the function `render` calls per sample -- for any camera the host can write down: a panorama, an
 * orthographic view, light probes, lightmap texels, its own lens model.  The call is a frame without the pinhole / DOF camera.
 *   Grouping: ray j * rays_per_result + k is sample k of result j; out[j] is the mean over result j's rays.  The direction is
 *   normalised on entry, as the reference does (:723); recursion, lights, shadows, fog, textures and the candidate filter of
 *   depth 1 are exactly a frame's.
 *   Config: seed, monte_carlo, max_recursion (at most RR_MAX_RECURSION, else RR_ERR_UNSUPPORTED), fog_density and fog_color are
 *   used.  samples (replaced by rays_per_result), focal_length and aperture_size (the caller made the rays) and gamma_correction
 *   (the output is linear) are ignored.
 *   RNG: the generator behind `jitter` is keyed (seed, pixel, sample, path node, stream); here pixel = stream_ids ? stream_ids[j] : j
 *   and sample = k.  Rays of frame pixel y * width + x given with that id draw what the frame draws for that pixel.
 *   Outputs: what a frame resolves for a pixel whose samples are these rays, BEFORE its min(., 1): color[c] = (float)(fixed-point
 *   sum * 2^-24) / (float)rays_per_result, NaN or +-inf where a ray's term was (as the reference's f32 sum); depth, normal and
 *   object_id exactly a frame's.  A ray that misses contributes colour 0, depth 0, normal 0, id 0.
 *   Limits: rays_per_result 1 .. RR_MAX_SAMPLES_WITH_TABLE (0: RR_ERR_INVALID_ARGUMENT, more: RR_ERR_UNSUPPORTED); n_results == 0
 *   returns RR_OK and touches nothing; n_results > 0x7fffff00: RR_ERR_UNSUPPORTED.  The total ray count may exceed 2^32: the
 *   call works in batches sized by rr_tuning::queue_budget_bytes.  Device memory: 64 B per result for the call's accumulators
 *   (RR_ERR_OUT_OF_MEMORY when they do not fit; the handle stays usable).
 *   Non-finite rays are accepted and answered as a frame answers them.  cancel: polled between device launches; a cancelled call
 *   returns RR_ERR_CANCELLED and the contents of `out` are then unspecified.
 * A frame call: it takes the scene's lock, returns RR_ERR_INVALID_ARGUMENT from on_pass of the same scene and RR_ERR_DEVICE on a
 * broken scene, and rr_scene_last_stats afterwards reports its counters (primary_rays = the number of rays).
 * origins / directions: n_results * rays_per_result * 3 floats (host); stream_ids: n_results ids, or NULL (result j uses j).
 * The device-buffer, stream-ordered form is rr_shade_rays_device below. */
typedef struct rr_radiance {
    float color[3];     /* mean over the result's rays of get_color_depth_normal_id(..).0: LINEAR, no min(., 1), no gamma */
    float depth;        /* mean of .1 */
    float normal[3];    /* the mean of .2, normalised (NaN when every ray missed: 0/0, as a frame's pixel) */
    uint32_t object_id; /* .3 as a frame reports it for a pixel whose samples are these rays */
} rr_radiance;          /* 32 bytes */
int rr_shade_rays(rr_scene* scene, const rr_config* config, const float* origins, const float* directions,
                  uint32_t n_results, uint32_t rays_per_result, const uint32_t* stream_ids,
                  rr_radiance* out, const volatile int* cancel);

/* The three ray queries on DEVICE buffers, in stream order: for rays that were produced on the GPU (a torch op, an earlier query's
 * hits, a lens model run as a kernel) and answers that are consumed there.  Every buffer is memory the scene's device can address
 * -- device memory of that device, of another device this library has enabled peer access to, pinned or managed memory -- in the
 * layout of the host form: n * 3 floats, n floats, n records of 20 / 20 / 32 bytes; every pointer 4-byte aligned, out_dev of
 * rr_shade_rays_device 16-byte aligned.  Each pointer is classified (hipPointerGetAttributes) before anything is enqueued: pageable
 * host memory, or another device's memory without peer access, is RR_ERR_INVALID_ARGUMENT with the argument's name in rr_last_error,
 * never a launch.
 *   Results: once `hip_stream` is synchronised, out_dev holds byte for byte what the host form writes into `out` for the same inputs
 *   on the same handle state (NaN bit patterns, the not-hit and not-occluded records and the reference's face ids included).
 *   Limits and argument checks are the host forms': n == 0 returns RR_OK and touches nothing, n > 0x7fffff00 is RR_ERR_UNSUPPORTED,
 *   depth 1 .. 255, rays_per_result, max_recursion; a NaN or negative max_distance_dev[i] is RR_ERR_INVALID_ARGUMENT naming the
 *   first such i, and nothing is written to out_dev.
 *   Stream: work is enqueued on `hip_stream` (a hipStream_t, NULL = the default stream).  The inputs are read in stream order -- the
 *   caller need not synchronise after producing them on that stream -- and the call returns once its last launch is enqueued; the
 *   caller synchronises before it reads out_dev on the host.  The call WAITS inside for what it must learn from the device before it
 *   can enqueue the walk: once, for 16 bytes -- the largest finite |origin| per axis, for which the top level must be padded (found
 *   on the device, in float; rr_shade_rays scans its host origins on the host), and the first bad max_distance.  rr_shade_rays_device
 *   waits in addition where rr_shade_rays does: for its frame constants and for the size of every depth level.
 *   Scene state: a frame call like the host forms -- the scene's lock, RR_ERR_INVALID_ARGUMENT from on_pass of the same scene,
 *   RR_ERR_DEVICE on a broken scene.  The handle's query buffers are shared, so a call on another stream than the handle's last
 *   call first waits for that stream, as rr_render_region_device does.  A scene edit or rr_scene_destroy waits for queries in
 *   flight; rr_scene_last_stats after rr_shade_rays_device behaves as after rr_render_region_device (it waits for the stream).
 *   Memory: nothing is allocated per call.  What the launches read after the call has returned belongs to the handle, grows on
 *   demand and is freed by rr_scene_destroy: 56 B per ray of the largest closest-hit or shadow query so far, host or device form
 *   (the packed records and the walk's raw hits), 4 B per result of the largest rr_shade_rays_device without stream ids, plus what
 *   rr_shade_rays keeps (64 B per result, the ray arena).  A growth that fails is RR_ERR_OUT_OF_MEMORY and leaves the handle usable.
 *   The host forms are these calls behind a staging copy: the caller's arrays in buffers of the call, the null stream, and the
 *   copy of the answers into `out`.
 *   cancel (rr_shade_rays_device): as rr_shade_rays; a call that is cancelled or fails part-way leaves the stream idle. */
int rr_trace_rays_device(rr_scene* scene, const float* origins_dev, const float* directions_dev, uint32_t n, uint32_t depth,
                         rr_ray_hit* out_dev, void* hip_stream);
int rr_trace_shadow_rays_device(rr_scene* scene, const float* origins_dev, const float* directions_dev, const float* max_distance_dev /* or NULL */,
                                uint32_t n, uint32_t depth, rr_shadow_hit* out_dev, void* hip_stream);
int rr_shade_rays_device(rr_scene* scene, const rr_config* config, const float* origins_dev, const float* directions_dev,
                         uint32_t n_results, uint32_t rays_per_result, const uint32_t* stream_ids_dev /* or NULL */,
                         rr_radiance* out_dev, void* hip_stream, const volatile int* cancel);

/* Surface queries for a batch of caller-supplied rays: what lies between rr_trace_rays (which item and face, how far) and
 * rr_shade_rays (the finished colour) -- the hit point, the normals, the uv and the material as the reference evaluates it there.
 * For a baker, a G-buffer, the albedo and normal guides of a denoiser, a host that applies its own BRDF.
 * Ray i is Raytracing::trace(ray_i, false, false, depth) (reference src/raytracing.rs:429-490) followed by the surface part of
 * get_color_depth_normal_id for that hit (:747-811, :928-933, :985-991): lights, recursion, fog and the generator are left out, so
 * the query is deterministic and takes no config.  Directions are used as given, as in rr_trace_rays (neither trace nor the hit
 * point normalises).  A miss is {0, 0xffffffff, 0, 0} followed by 112 zero bytes.
 * origins / directions: n * 3 floats (host); `depth`: what the candidate filter sees, 1 .. 255 (1 = a frame's primary ray).  Limits
 * and argument checks are rr_trace_rays': n == 0 returns RR_OK and touches nothing, n > 0x7fffff00 is RR_ERR_UNSUPPORTED.
 * Non-finite rays are accepted and answered as a frame answers them.  A frame call: the scene's lock, RR_ERR_INVALID_ARGUMENT from
 * on_pass of the same scene, RR_ERR_DEVICE on a broken scene; nothing of a frame's state (accumulators, counters, rr_scene_last_stats)
 * is touched.
 * rr_surface_rays_device: the same on DEVICE buffers in stream order, under every rule of rr_trace_rays_device above -- pointers
 * classified before any launch, origins_dev / directions_dev 4-byte aligned, out_dev 16-byte aligned (RR_ERR_INVALID_ARGUMENT naming
 * the argument, never a launch), one wait inside for the 16 bytes of the origins' reach, the handle's query buffers (56 B per ray
 * of the largest query so far) shared with the other queries.  Once `hip_stream` is synchronised out_dev holds byte for byte what
 * the host form writes.  The host form is the device form behind a staging copy (12 + 12 + 128 B per ray for the call). */
typedef struct rr_surface_hit {       /* 128 bytes, eight 16-byte rows */
    uint32_t hit;                     /* 0 = None; this row is exactly rr_ray_hit's four words for the ray */
    uint32_t item_index;
    uint32_t object_id;
    uint32_t face_id;
    float position[3];                /* origin + direction * toi, in f32 (:747) */
    float distance;                   /* toi */
    float normal[3];                  /* Shape::intersect's world normal = what a frame sums into its normal buffer: smooth interpolation,
                                         back face and flip_normals applied */
    int32_t material;                 /* the item's `material` index */
    float shading_normal[3];          /* after normal mapping (:757-784), BEFORE the roughness jitter; = normal without a normal map */
    uint32_t has_uv;                  /* material.has_any_texture() (:751) */
    float base_color[4];              /* get_item_color(Base), rgba (:677-712) */
    float ambient_color[3];           /* get_item_color(Ambient).xyz */
    float alpha;                      /* material.alpha * base_color.w, * the alpha texel's .x with an alpha map (:806-811) */
    float specular_color[3];          /* get_item_color(Specular).xyz */
    float reflectivity;               /* material.reflectivity, or the reflectivity map's .x (:928-933) */
    float uv[2];                      /* get_uv as the frame uses it; (0, 0) when !has_uv */
    float roughness;                  /* material.roughness, or (1/PI/2) * texel.x with a roughness map (:790-795), whatever monte_carlo says */
    float ambient_occlusion;          /* the AO texel's .x; 1 without an AO map (:985-991) */
} rr_surface_hit;
int rr_surface_rays(rr_scene* scene, const float* origins, const float* directions, uint32_t n, uint32_t depth, rr_surface_hit* out);
int rr_surface_rays_device(rr_scene* scene, const float* origins_dev, const float* directions_dev, uint32_t n, uint32_t depth,
                           rr_surface_hit* out_dev, void* hip_stream);

/* Pixels of the frame's own camera, as linear floats: Raytracing::render(x, y) -> PixelData (reference src/raytracing.rs:275-427) for a
 * list of pixels of the caller's choice or for every pixel of the frame, BEFORE the clamp, the gamma curve and the truncation to bytes
 * that rr_render applies.  For tone mapping, a denoiser, EXR output, averages over frames of several seeds, compositing; for a crop
 * window, the part of the screen an edit touched, more samples where a host found noise, the reference's own shuffled 2x2 cells.
 * The call is a frame: the camera, the sub-sample table (sample_xy or the built-in one), depth of field, the sample groups, the level
 * walk and the generator are rr_render's, and a pixel's record does not depend on which other pixels the call holds.
 *   Pixel list: pixel_xy[i] = x | y << 16 with x < width and y < height; out[i] (and rgba8_out + 4 * i) is that pixel.  Duplicates are
 *   allowed and give equal records; any order is allowed.  List order is slot order: a 64-ray packet of primary rays holds 64 / G
 *   consecutive entries (G = the frame's sample group, 1 .. 64), so screen neighbours should be list neighbours -- 8x8 blocks, as the
 *   library orders a whole frame -- or the packets lose their coherence.  A list whose length is no multiple of 64 / G runs with G = 1.
 *   NULL list: every pixel of the frame; n_pixels must be width * height (else RR_ERR_INVALID_ARGUMENT); pixel (x, y) goes to
 *   out[y * width + x], and the call is traced in the library's own 8x8-block slot order, as rr_render is.
 *   out[i]: rr_radiance exactly as rr_shade_rays defines it -- color = (float)(fixed-point sum * 2^-24) / (float)samples, LINEAR, NaN or
 *   +-inf where a sample's term was; depth; the normalised mean normal (NaN when every sample missed); object_id.  depth, normal and
 *   object_id are what rr_render writes for the pixel (the three sums are always accumulated here).
 *   rgba8_out (or NULL): 4 bytes per pixel, the bytes rr_render writes for it: min(., 1), the gamma curve when config->gamma_correction
 *   is set, truncation, alpha 255.  An output of its own because the device's powf cannot be reproduced on the host; without gamma it
 *   equals (uint8_t)(fminf(color, 1) * 255) in f32.
 *   Config: every field is used as a frame uses it (samples, focal_length / aperture_size, fog, seed, monte_carlo, max_recursion);
 *   gamma_correction affects rgba8_out only.
 *   Limits and checks: rr_render's for scene, camera, config and table; out == NULL is RR_ERR_INVALID_ARGUMENT; n_pixels == 0 returns
 *   RR_OK and touches nothing; n_pixels > 2^30 is RR_ERR_UNSUPPORTED before anything is allocated; an entry outside the frame is
 *   RR_ERR_INVALID_ARGUMENT, rr_last_error names the first such index, and nothing is written to out.  Device memory: 64 B per pixel
 *   of accumulators and 12 B per list entry, kept by the handle; the host form adds 36 (40 with a list) B per pixel for the call.
 *   A frame call: the scene's lock, RR_ERR_INVALID_ARGUMENT from on_pass of the same scene, RR_ERR_DEVICE on a broken scene;
 *   rr_scene_last_stats and rr_scene_overlap_stages report it like a frame (primary_rays = n_pixels * samples).  cancel: as
 *   rr_shade_rays.  The frames before and after are not affected: the list's slot table is the call's own.
 * rr_render_pixels_device: the same on DEVICE buffers in stream order, under every rule of rr_shade_rays_device above -- pointers
 * classified before any launch (RR_ERR_INVALID_ARGUMENT naming the argument), out_dev 16-byte aligned, pixel_xy_dev and rgba8_out_dev
 * 4-byte aligned; camera, config and sample_xy are host memory.  The call waits inside where a frame waits (its constants, the size of
 * every depth level) and, with a list, once for 4 bytes: the first index outside the frame.  The list is copied into a buffer of the
 * handle first, so nothing the launches read after the return is the caller's.  A scene edit or rr_scene_destroy waits for calls in
 * flight.  Once `hip_stream` is synchronised the buffers hold byte for byte what the host form writes; the host form is this call
 * behind a staging copy (without a list there is nothing to stage in). */
int rr_render_pixels(rr_scene* scene, const rr_camera* camera, const rr_config* config, const uint16_t* sample_xy,
                     const uint32_t* pixel_xy /* or NULL */, uint32_t n_pixels,
                     rr_radiance* out, uint8_t* rgba8_out /* or NULL */, const volatile int* cancel);
int rr_render_pixels_device(rr_scene* scene, const rr_camera* camera, const rr_config* config, const uint16_t* sample_xy,
                            const uint32_t* pixel_xy_dev /* or NULL */, uint32_t n_pixels,
                            rr_radiance* out_dev, uint8_t* rgba8_out_dev /* or NULL */, void* hip_stream, const volatile int* cancel);

/* A pixel's samples as K interleaved means next to its full record: what a host needs to FIND noise (the half-buffer error estimate
 * |A - B| / 2 at K = 2), to reject fireflies (median of means), or to see every single sample of a pixel (K = samples <= 64).  The rays
 * are exactly those of rr_render_pixels for the same arguments; only where their terms are summed differs.
 *   Subsets: with S = config->samples and K = n_parts, part h of a pixel is the samples {s : s mod K == h} of the frame's S samples.
 *   s is the frame's sample index: the row of the sub-sample table, the `sample` key of the generator, the index the object-id rule
 *   looks at.  Nothing about a sample changes because it is in a part.
 *   parts_out[i * K + h]: an rr_radiance over the part's S / K samples -- color[c] = (float)(fixed-point sum of the part's terms * 2^-24)
 *   / (float)(S / K), NaN or +-inf where a term of THAT part was; depth and normal resolved the same way over the part's samples (the
 *   normal normalised, NaN when every sample of the part missed); object_id is the pixel's id, out[i].object_id, in every part.
 *   out[i]: byte for byte the record rr_render_pixels writes for that pixel under the same handle state, camera, config and table.  It
 *   is formed from the sum of the parts' integer sums and the OR of their flags; integer adds commute, so this is exact.  Required, as
 *   parts_out is (NULL: RR_ERR_INVALID_ARGUMENT).
 *   n_parts: a power of two from 2 to 64 that divides samples; anything else is RR_ERR_INVALID_ARGUMENT and rr_last_error says which
 *   rule failed.  n_pixels * n_parts > 2^30 is RR_ERR_UNSUPPORTED before anything is allocated.
 *   Everything else is rr_render_pixels': the list form and the NULL list for the whole frame (n_pixels == width * height; pixel (x, y)
 *   at out[y * width + x] and parts_out[(y * width + x) * K + h]); duplicates and any order; an entry outside the frame refused naming
 *   its index with nothing written; n_pixels == 0 returns RR_OK and touches nothing; a frame call (the scene's lock, refused from
 *   on_pass, RR_ERR_DEVICE on a broken scene); rr_scene_last_stats gives primary_rays = n_pixels * samples and all four work counters
 *   equal those of rr_render_pixels for the same pixels; cancel; the frames before and after are not affected.
 *   Device memory: 64 * K B per pixel of accumulators and 12 * K B per list entry (a whole frame counts as a list here), kept by the
 *   handle; the host form adds 32 + 32 * K (with a list 36 + 32 * K) B per pixel, kept by the handle as well.
 *   Sample groups: the call runs as n_pixels * K accumulator slots of S / K samples each, the K slots of an entry side by side.  A
 *   64-ray packet holds 64 / G consecutive slots, so G is the largest power of two that divides S / K (at most 64) for which
 *   n_pixels * K is a multiple of 64 / G; where there is none the call runs with G = 1.  K = S leaves one sample per slot: G = 1.  A
 *   list padded to a multiple of 64 entries keeps its group for every K.
 * rr_render_pixel_parts_device: the same on DEVICE buffers in stream order, under every rule of rr_render_pixels_device: pointers
 * classified before any launch, out_dev and parts_out_dev 16-byte aligned, pixel_xy_dev 4-byte aligned, the list copied into a buffer
 * of the handle, the call waits where a frame waits and once for the 4 bytes of the list check.  Once `hip_stream` is synchronised
 * the buffers hold byte for byte what the host form writes; the host form is this call behind a staging copy.
 * There is no byte output: bytes are rr_render_pixels' business. */
int rr_render_pixel_parts(rr_scene* scene, const rr_camera* camera, const rr_config* config, const uint16_t* sample_xy,
                          const uint32_t* pixel_xy /* or NULL */, uint32_t n_pixels, uint32_t n_parts,
                          rr_radiance* out /* n_pixels */, rr_radiance* parts_out /* n_pixels * n_parts */, const volatile int* cancel);
int rr_render_pixel_parts_device(rr_scene* scene, const rr_camera* camera, const rr_config* config, const uint16_t* sample_xy,
                                 const uint32_t* pixel_xy_dev /* or NULL */, uint32_t n_pixels, uint32_t n_parts,
                                 rr_radiance* out_dev /* n_pixels */, rr_radiance* parts_out_dev /* n_pixels * n_parts */, void* hip_stream,
                                 const volatile int* cancel);

/* Adaptive sampling on the device: find the noisy pixels of a frame and spend more samples on them, without a trip through the host.
 * The estimate is the half-buffer one: with A and B the LINEAR colours of the two halves of a pixel (rr_render_pixel_parts at K = 2),
 *   error = max over r, g, b of |min(A, 1) - min(B, 1)| / 2, and 0 where any of the six floats is NaN or infinite
 * (more samples cannot cure a non-finite term); every step is exact in binary32, so a host that computes it itself gets the same bits.
 *
 * rr_refine_list_device: the pixels of a width x height frame whose error exceeds `threshold`, as a list rr_render_pixels_device takes.
 *   parts_dev: width * height * 2 records, the whole-frame layout of rr_render_pixel_parts at K = 2 (part h of pixel (x, y) at
 *   (y * width + x) * 2 + h), 16-byte aligned.  error_out_dev (or NULL): width * height floats, the error at y * width + x.
 *   list_out_dev: rr_refine_list_capacity(width, height) entries x | y << 16 (width * height rounded up to a multiple of 64).  The list
 *   is ordered as the library orders a whole frame -- 8x8 blocks row-major, row-major inside a block -- so that screen neighbours are
 *   list neighbours, and is padded with copies of its last entry to a multiple of 64 entries (the call that renders it keeps its sample
 *   group; duplicates give equal records).  *count_out (HOST) = the entries before the pad; an empty list has no pad.  Entries behind
 *   the padded length are not written.  A pixel is taken when error > threshold: a negative threshold takes every pixel.
 *   The call follows the rules of the device ray queries: every pointer is classified before any launch (RR_ERR_INVALID_ARGUMENT naming
 *   the argument), error_out_dev and list_out_dev 4-byte aligned, work enqueued on `hip_stream` in stream order (the parts may have been
 *   produced on that stream without a synchronisation), the scene's lock, RR_ERR_INVALID_ARGUMENT from on_pass of the same scene.  It
 *   WAITS inside once, for the 4 bytes of the count.  Nothing of a frame's state or statistics is touched.
 *   Refusals: width or height 0 or above 65535, a NaN threshold, a NULL parts_dev, list_out_dev or count_out: RR_ERR_INVALID_ARGUMENT;
 *   width * height * 2 > 2^30: RR_ERR_UNSUPPORTED before anything is allocated.
 *   Memory: 12 B per 8x8 block of the largest frame so far, kept by the handle until rr_scene_destroy.
 *
 * rr_render_adaptive: a frame at two sample counts.  Under ONE hold of the scene's lock (no edit can land between the estimate and the
 * refinement), on one stream: the whole frame in two parts at base_samples, the list above, the padded list through the body of
 * rr_render_pixels at max_samples, and the refined records scattered over the base frame.
 *   out[y * width + x]: byte for byte the record rr_render_pixels writes for that pixel at the sample count samples_out names there,
 *   base_samples or max_samples, under the table given for that count (sample_xy_base, sample_xy_max; NULL = the built-in one).
 *   rgba8_out (or NULL): the bytes rr_render_pixels writes for that pixel at that count.  samples_out (or NULL): the count per pixel.
 *   error_out (or NULL): the error of the BASE frame's halves, as above.  *n_refined_out (or NULL, HOST): the pixels refined, the list's
 *   count before the pad.
 *   Config: samples is ignored; every other field is used as a frame uses it; gamma_correction affects rgba8_out only.
 *   Checks: base_samples even and at least 2 (the two halves must be equal), both counts under rr_render's rule for their table, a
 *   NaN threshold and out == NULL: RR_ERR_INVALID_ARGUMENT; width * height * 2 > 2^30: RR_ERR_UNSUPPORTED before anything is allocated.
 *   A frame call: the scene's lock, RR_ERR_INVALID_ARGUMENT from on_pass of the same scene, RR_ERR_DEVICE on a broken scene; cancel as
 *   rr_render_pixels (RR_ERR_CANCELLED, `out` unspecified, the stream left idle); the frames before and after are not affected.
 *   rr_scene_last_stats reports the SUMS over the two passes, as rr_render_progressive_tiles sums its passes: primary_rays = width *
 *   height * base_samples + padded count * max_samples; with rr_tuning::kernel_timing, ms_binning holds the device time of the three
 *   launches that make the list (an order-preserving compaction is a re-ordering too).  The call waits inside where its two passes
 *   wait, and once for the 4 bytes of the count; with count 0 the fine pass and the scatter are skipped.
 *   Device memory kept by the handle: per pixel 64 B of part records, 4 B of list, and rr_render_pixel_parts' own at K = 2 (128 B of
 *   accumulators, 24 B of slot table); per entry of the largest padded list 32 B of fine records and rr_render_pixels' own (64 + 12 B);
 *   12 B per 8x8 block.  The host form adds 32 B per pixel, and 4, 2 and 4 B for the outputs it is asked for.
 * rr_render_adaptive_device: the same on DEVICE buffers in stream order, under every rule of rr_render_pixels_device: pointers classified
 * before any launch, out_dev 16-byte aligned, rgba8_out_dev and error_out_dev 4-byte aligned, samples_out_dev 2-byte aligned.  Once
 * `hip_stream` is synchronised the buffers hold byte for byte what the host form writes; the host form is this call behind a staging copy. */
uint64_t rr_refine_list_capacity(uint32_t width, uint32_t height);
int rr_refine_list_device(rr_scene* scene, uint32_t width, uint32_t height, const rr_radiance* parts_dev /* width * height * 2 */,
                          float threshold, float* error_out_dev /* width * height, or NULL */,
                          uint32_t* list_out_dev /* rr_refine_list_capacity entries */, uint32_t* count_out /* HOST */, void* hip_stream);
int rr_render_adaptive(rr_scene* scene, const rr_camera* camera, const rr_config* config,
                       uint16_t base_samples, uint16_t max_samples, float threshold,
                       const uint16_t* sample_xy_base /* or NULL */, const uint16_t* sample_xy_max /* or NULL */,
                       rr_radiance* out /* width * height */, uint8_t* rgba8_out /* or NULL */, uint16_t* samples_out /* or NULL */,
                       float* error_out /* or NULL */, uint32_t* n_refined_out /* or NULL, HOST */, const volatile int* cancel);
int rr_render_adaptive_device(rr_scene* scene, const rr_camera* camera, const rr_config* config,
                              uint16_t base_samples, uint16_t max_samples, float threshold,
                              const uint16_t* sample_xy_base /* or NULL */, const uint16_t* sample_xy_max /* or NULL */,
                              rr_radiance* out_dev /* width * height */, uint8_t* rgba8_out_dev /* or NULL */, uint16_t* samples_out_dev /* or NULL */,
                              float* error_out_dev /* or NULL */, uint32_t* n_refined_out /* or NULL, HOST */, void* hip_stream,
                              const volatile int* cancel);

/* Refinement level by level.  rr_render_adaptive knows two sample counts; most pixels that fail the threshold at the lower one pass it
 * long before the upper one.  Here a pixel climbs a ladder of counts and stops at the first whose halves agree.
 *
 * rr_refine_sublist_device: the list of a list.  Entry i of list_dev is x | y << 16 and its two halves lie at parts_dev[2 i] and
 * parts_dev[2 i + 1], the layout rr_render_pixel_parts writes for a list at K = 2.
 *   error_out_dev (or NULL): `count` floats, the error of entry i at i (the estimate above, the same bits as on the host).
 *   list_out_dev: the entries with error > threshold in the order they had (a sub-sequence of a block-ordered list is block-ordered),
 *   padded with copies of its last entry to a multiple of 64; room for `count` rounded up to a multiple of 64 entries.  *count_out
 *   (HOST) = the entries before the pad.  An empty result has no pad and writes nothing to the list; words behind the padded length
 *   are not written.
 *   Only the first `count` entries and their halves are looked at: the caller's own pad is never taken.  Duplicates are entries like
 *   any other.  The coordinates are not interpreted: there is no frame size.
 *   The call follows rr_refine_list_device: every pointer classified before any launch (RR_ERR_INVALID_ARGUMENT naming the argument),
 *   parts_dev 16-byte aligned, the others 4-byte aligned, work enqueued on `hip_stream` in stream order, the scene's lock,
 *   RR_ERR_INVALID_ARGUMENT from on_pass of the same scene, ONE wait inside for the 4 bytes of the count, nothing of a frame's state
 *   or statistics touched.
 *   Refusals: a NULL scene or count_out, a NaN threshold, and with count > 0 a NULL list_dev, parts_dev or list_out_dev, a misaligned
 *   pointer, or list_out_dev (padded) overlapping list_dev: RR_ERR_INVALID_ARGUMENT; count > 2^29: RR_ERR_UNSUPPORTED.  count == 0:
 *   RR_OK with *count_out = 0; nothing is launched and no other pointer is looked at.
 *   Memory: 12 B per 64 entries of the longest list so far, kept by the handle until rr_scene_destroy (the buffer rr_refine_list_device grows).
 *
 * rr_render_adaptive_levels: a frame at n_levels sample counts, 2 <= n_levels <= RR_MAX_ADAPTIVE_LEVELS.  Under ONE hold of the scene's
 * lock, on one stream: the whole frame in two parts at level_samples[0] and its list, as rr_render_adaptive; then for l = 1, 2, ...
 * while the list is not empty, the padded list in two parts at level_samples[l], its records scattered over the frame, and the
 * sublist above as the next level's list.  Every pixel ends below the threshold or at the top count.
 *   sample_xy_levels: NULL, or n_levels pointers, each the table of its level or NULL for the built-in one.
 *   out[y * width + x]: byte for byte the record rr_render_pixels writes for that pixel at the count samples_out names there, under the
 *   table of that level.  rgba8_out (or NULL): its bytes at that count.  samples_out (or NULL): the count of the last level that
 *   rendered the pixel.
 *   error_out (or NULL): the error of the pixel's halves AT THAT COUNT, the residual error.  This differs by design from
 *   rr_render_adaptive, whose error_out is the base frame's: there a refined pixel keeps the error that had it refined.
 *   level_pixels_out (or NULL, HOST, n_levels words): the pixels rendered at each level before the pad; [0] = width * height; levels
 *   never reached are 0.
 *   Config: samples is ignored; every other field is used as a frame uses it; gamma_correction affects rgba8_out only.
 *   Checks: n_levels out of range, a count that is odd or below 2 (the two halves must be equal), a count not above the one before
 *   it (the message names the level and the rule), a NaN threshold, out == NULL: RR_ERR_INVALID_ARGUMENT; every count under rr_render's
 *   rule for its table; width * height * 2 > 2^30: RR_ERR_UNSUPPORTED before anything is allocated.
 *   A frame call: the scene's lock, RR_ERR_INVALID_ARGUMENT from on_pass of the same scene, RR_ERR_DEVICE on a broken scene; cancel is
 *   polled inside the passes and between levels (RR_ERR_CANCELLED, `out` unspecified, the stream left idle); the frames before and
 *   after are not affected.
 *   rr_scene_last_stats reports the SUMS over all passes: primary_rays = the sum over the levels reached of padded list length x the
 *   level's count (level 0: width * height); with rr_tuning::kernel_timing, ms_binning holds the device time of every list's launches.
 *   The call waits inside where its passes wait, and once per level but the last for the 4 bytes of a count.
 *   Device memory kept by the handle: what rr_render_adaptive keeps (per pixel 64 B of part records, rounded up to 64 pixels, 4 B of
 *   list and rr_render_pixel_parts' own at K = 2; 12 B per 8x8 block), per entry of the largest padded list 32 B of records, 4 B of
 *   the second list and rr_render_pixel_parts' own at K = 2 (128 B of accumulators, 24 B of slot table).  The host form adds 32 B per
 *   pixel, and 4, 2 and 4 B for the outputs it is asked for.
 * rr_render_adaptive_levels_device: the same on DEVICE buffers in stream order, under every rule of rr_render_adaptive_device.  Once
 * `hip_stream` is synchronised the buffers hold byte for byte what the host form writes; the host form is this call behind a staging copy. */
#define RR_MAX_ADAPTIVE_LEVELS 8u
int rr_refine_sublist_device(rr_scene* scene, const uint32_t* list_dev, uint32_t count, const rr_radiance* parts_dev /* count * 2 */,
                             float threshold, float* error_out_dev /* count, or NULL */,
                             uint32_t* list_out_dev /* count rounded up to 64 entries */, uint32_t* count_out /* HOST */, void* hip_stream);
int rr_render_adaptive_levels(rr_scene* scene, const rr_camera* camera, const rr_config* config,
                              const uint16_t* level_samples, uint32_t n_levels, float threshold,
                              const uint16_t* const* sample_xy_levels /* NULL, or n_levels pointers each a table or NULL */,
                              rr_radiance* out /* width * height */, uint8_t* rgba8_out /* or NULL */, uint16_t* samples_out /* or NULL */,
                              float* error_out /* or NULL */, uint32_t* level_pixels_out /* n_levels, HOST, or NULL */,
                              const volatile int* cancel);
int rr_render_adaptive_levels_device(rr_scene* scene, const rr_camera* camera, const rr_config* config,
                                     const uint16_t* level_samples, uint32_t n_levels, float threshold,
                                     const uint16_t* const* sample_xy_levels /* NULL, or n_levels pointers each a table or NULL */,
                                     rr_radiance* out_dev /* width * height */, uint8_t* rgba8_out_dev /* or NULL */,
                                     uint16_t* samples_out_dev /* or NULL */, float* error_out_dev /* or NULL */,
                                     uint32_t* level_pixels_out /* n_levels, HOST, or NULL */, void* hip_stream, const volatile int* cancel);

/* Refinement that keeps its samples.  A level of rr_render_adaptive_levels is a frame of its own: its table and its cell size are those
 * of its count, so a pixel that climbs 16 -> 32 -> 64 -> 128 is traced from scratch four times.  Here every level is a PREFIX of one
 * frame of config->samples samples, and a pixel that climbs is only given the samples it does not have yet.
 *
 * rr_render_pixel_prefix: rr_render_pixels over samples 0 .. samples_used - 1 of the frame of config->samples samples.  Everything is
 * that frame's: its table (sample_xy, or the built-in one for config->samples), its cell size, its depth-of-field offsets, its
 * generator keys; only the sums are divided by samples_used.  This is the estimator a progressive preview shows after samples_used
 * slices, at a count of the caller's choice and as records.
 *   out[i]: the record over those samples; object_id is the id of sample samples_used - 1, the last one taken.
 *   halves_out (or NULL): n_pixels * 2 records in the layout of rr_render_pixel_parts at K = 2; half h is the samples
 *   {s < samples_used : s mod 2 == h}, resolved over samples_used / 2.  With it samples_used must be even: the two halves of a pixel
 *   must be equal (RR_ERR_INVALID_ARGUMENT), and n_pixels * 2 > 2^30 is RR_ERR_UNSUPPORTED.
 *   rgba8_out (or NULL): the frame's bytes of `out`, as rr_render_pixels writes them.
 *   samples_used == config->samples: out and rgba8_out are byte for byte what rr_render_pixels writes, halves_out byte for byte what
 *   rr_render_pixel_parts writes at K = 2.  samples_used == 0 or above config->samples: RR_ERR_INVALID_ARGUMENT.
 *   Every other check, limit, list rule, lock rule, cancel behaviour and memory note is rr_render_pixels' (without halves_out) or
 *   rr_render_pixel_parts' at K = 2 (with it).  rr_scene_last_stats reports primary_rays = n_pixels * samples_used.
 *   Sample groups: the plan groups the samples_used / K samples of a slot, not the frame's; a count that no group divides runs with
 *   G = 1.  The bits do not depend on G.
 * rr_render_pixel_prefix_device: the same on DEVICE buffers in stream order, under every rule of rr_render_pixels_device; out_dev and
 * halves_out_dev 16-byte aligned, pixel_xy_dev and rgba8_out_dev 4-byte aligned.
 *
 * rr_render_adaptive_prefix: a frame at the n_levels prefixes prefix_samples[0] < ... < prefix_samples[n_levels - 1] == config->samples
 * of ONE frame (sample_xy: ONE table of config->samples entries, or NULL), 2 <= n_levels <= RR_MAX_ADAPTIVE_LEVELS.  Under one hold of
 * the scene's lock, on one stream: the whole frame in two halves over samples [0, P0) and its list, made with the estimate and in the
 * order of rr_refine_list_device; then for l = 1, 2, ... while the list is not empty: ONLY samples [P(l-1), Pl) of the listed pixels,
 * added to the fixed-point sums those pixels already have (integer adds: the sums are those of a pixel traced from sample 0 in one
 * go), the records at Pl written over the frame, and the sublist for the next level.  The sums stay on the device between levels.
 *   out[y * width + x]: byte for byte what rr_render_pixel_prefix writes for that pixel at the samples_used that samples_out names
 *   there.  rgba8_out (or NULL): its bytes at that count.  samples_out (or NULL): the last prefix the pixel reached.  error_out (or
 *   NULL): the residual error of its halves at that count, as rr_render_adaptive_levels reports it.  level_pixels_out (or NULL, HOST,
 *   n_levels words): as rr_render_adaptive_levels.
 *   Config: samples IS used here: it is the frame every prefix is taken from, and the last prefix.
 *   Checks: n_levels out of range, a prefix that is odd or below 2, a prefix not above the one before it, a last prefix other than
 *   config->samples (the message names the level and the rule), a NaN threshold, out == NULL: RR_ERR_INVALID_ARGUMENT; config->samples
 *   under rr_render's rule for its table; width * height * 2 > 2^30: RR_ERR_UNSUPPORTED before anything is allocated.
 *   A frame call, cancel, and the frames before and after: as rr_render_adaptive_levels.
 *   rr_scene_last_stats reports the sums over all passes: primary_rays = width * height * P0 + the sum over the levels reached of
 *   padded list length x (Pl - P(l-1)); with rr_tuning::kernel_timing, ms_binning holds the device time of the launches that make
 *   the lists and move the sums.  The call waits inside where its passes wait and once per level but the last for the 4 bytes of a
 *   count; a level's pass does not wait for a list check, the list being the library's own.
 *   Device memory kept by the handle: rr_render_pixel_parts' own at K = 2 for the frame (128 B of accumulators and 24 B of slot table
 *   per pixel), and per entry of the first padded list two sets of accumulators (128 B each), two lists (4 B each), 24 B of slot table;
 *   12 B per 64 pixels.  The host form adds 32 B per pixel, and 4, 2 and 4 B for the outputs it is asked for.
 * rr_render_adaptive_prefix_device: the same on DEVICE buffers in stream order, under every rule of rr_render_adaptive_levels_device. */
int rr_render_pixel_prefix(rr_scene* scene, const rr_camera* camera, const rr_config* config, const uint16_t* sample_xy,
                           const uint32_t* pixel_xy /* or NULL */, uint32_t n_pixels, uint32_t samples_used,
                           rr_radiance* out /* n_pixels */, rr_radiance* halves_out /* n_pixels * 2, or NULL */,
                           uint8_t* rgba8_out /* or NULL */, const volatile int* cancel);
int rr_render_pixel_prefix_device(rr_scene* scene, const rr_camera* camera, const rr_config* config, const uint16_t* sample_xy,
                                  const uint32_t* pixel_xy_dev /* or NULL */, uint32_t n_pixels, uint32_t samples_used,
                                  rr_radiance* out_dev /* n_pixels */, rr_radiance* halves_out_dev /* n_pixels * 2, or NULL */,
                                  uint8_t* rgba8_out_dev /* or NULL */, void* hip_stream, const volatile int* cancel);
int rr_render_adaptive_prefix(rr_scene* scene, const rr_camera* camera, const rr_config* config, const uint16_t* sample_xy /* ONE table, or NULL */,
                              const uint16_t* prefix_samples, uint32_t n_levels, float threshold,
                              rr_radiance* out /* width * height */, uint8_t* rgba8_out /* or NULL */, uint16_t* samples_out /* or NULL */,
                              float* error_out /* or NULL */, uint32_t* level_pixels_out /* n_levels, HOST, or NULL */,
                              const volatile int* cancel);
int rr_render_adaptive_prefix_device(rr_scene* scene, const rr_camera* camera, const rr_config* config, const uint16_t* sample_xy /* ONE table, or NULL */,
                                     const uint16_t* prefix_samples, uint32_t n_levels, float threshold,
                                     rr_radiance* out_dev /* width * height */, uint8_t* rgba8_out_dev /* or NULL */,
                                     uint16_t* samples_out_dev /* or NULL */, float* error_out_dev /* or NULL */,
                                     uint32_t* level_pixels_out /* n_levels, HOST, or NULL */, void* hip_stream, const volatile int* cancel);

/* A denoiser for the records the calls above produce: an edge-avoiding a-trous wavelet filter (5x5 B3 spline, step 1, 2, 4, ... per pass)
 * over a whole frame of rr_radiance records, on the device.  It is guided by the records' own object id, normal and depth; when the two
 * halves of every pixel are given (rr_render_pixel_parts at K = 2, rr_render_pixel_prefix with halves_out) also by the luminance variance
 * estimated from them, which costs no ray; with an albedo (rr_surface_pixels_device for the frame's camera: albedo_out) it runs on
 * albedo-demodulated colour.  Without halves the filter is geometry-only: it does not cross an id, normal or depth edge, but blurs
 * texture and shading inside a surface.
 * As for the half-buffer error above, EVERY STEP IS EXACT IN BINARY32 IN THE ORDER STATED HERE: no transcendentals (the weights are
 * rational functions), no contraction, division and sqrt correctly rounded.  A host that follows this text gets the same bits
 * (rustray_amd/denoise.py: atrous_denoise does, in numpy).
 *   dot(a, b) = (a.x*b.x + a.y*b.y) + a.z*b.z;  lum(c) = (0.2126f*r + 0.7152f*g) + 0.0722f*b;  EPS = 2^-20.
 *   Prepare, per pixel p.  fin_p: the three colour floats of records[p] are finite.  valid_p: depth and the three normal floats are.
 *   With albedo, channel k of a colour is demodulated as c_k / a_k when 2^-10 < a_k <= FLT_MAX, otherwise left as it is; the same rule
 *   is applied to both halves, and undone by * a_k at the end.  Variance, with halves: where fin_p holds and all six half colours (as
 *   given) are finite, d = (lum(A) - lum(B)) * 0.5f on the demodulated halves and v_p = d*d, otherwise v_p = 0; then a 3x3 prefilter
 *   over the taps q inside the frame with fin_q, row-major (dy outer), weights g = {1/2, 1/4}[|dx|] * {1/2, 1/4}[|dy|], both sums
 *   starting at 0: var_p = (sum g*v_q) / (sum g).  Without halves, and where !fin_p, var_p = 0.
 *   Pass i, step s = 2^i, for every p with fin_p.  Three sums start at 0; dy = -2..2 (outer), dx = -2..2 (inner), q = p + s*(dx, dy).
 *   A tap is skipped when q lies outside the frame, !fin_q, id_q != id_p, or valid_q != valid_p.  Otherwise, in this order:
 *     1. w = K[|dx|] * K[|dy|], K = {3/8, 1/4, 1/16}.
 *     2. If valid_p: cs = dot(n_p, n_q); cs = cs > 0 ? cs : 0; normal_power_log2 times cs = cs*cs; w = w * cs; and unless dx = dy = 0:
 *        t = |z_p - z_q| / ((sigma_depth * |z_p|) * (float)(s * max(|dx|, |dy|)) + EPS), w = w / (1.0f + t*t).
 *     3. With halves: t = |lum(c_p) - lum(c_q)| / (sigma_luminance * sqrtf(var_p) + EPS), w = w / (1.0f + t*t); c and var are the
 *        pass's input.
 *     4. sum_c[k] += w * c_q[k]; sum_v += (w*w) * var_q; sum_w += w.
 *   Then, if 0 < sum_w <= FLT_MAX: c'_p = sum_c / sum_w and var'_p = sum_v / (sum_w * sum_w).  Otherwise (sum_w is 0, inf or NaN: a
 *   weightless pixel) c'_p = c_p and var'_p = var_p: the pixel keeps the colour and variance of the pass's input for this pass.  A
 *   pixel with !fin_p keeps its colour bits and var 0 through every pass and is never a tap.
 *   Normals are expected to be of unit length or non-finite, as the records of this library are.  Any finite normal is accepted: a
 *   zero normal, or a short one at a high power (length 0.5 at normal_power_log2 7: 0.25^128 underflows), makes the centre tap's own cs
 *   and with it sum_w 0, a huge one makes a dot product overflow and sum_w inf or NaN; such a pixel is weightless in that pass, keeps
 *   its colour by the rule above and remains a tap of its neighbours with that finite colour.
 *   Finite working colours stay finite through the passes: a pass forms a weighted mean with weights of one sign, which cannot
 *   overflow.  What a finite input can still produce that is not finite:
 *     - a +inf variance, where a squared luminance difference (colours above 2^64 or so) overflows;
 *     - an inf colour at the finish, where the remodulation c * a_k by an albedo above 1 overflows;
 *     - an inf working colour at the start, where the demodulation c_k / a_k of a colour above 2^117 by an albedo below 1 overflows:
 *       fin is judged on the input, so that inf is a tap of its id region and makes infs and NaNs there; where both halves overflow
 *       as well, the seed (lum(A) - lum(B)) is inf - inf = NaN and still a tap of the prefilter, a NaN variance for the 3x3 pixels
 *       around it.  All of it follows from the text above and is the same on every implementation, but keep c_k / a_k finite;
 *     - a NaN variance: (w*w) * var_q is 0 * inf where a weight's square underflows at a tap whose variance is +inf, and
 *       sum_v / (sum_w * sum_w) is 0 / 0 where sum_w * sum_w underflows (normals of length 0.5 at normal_power_log2 6).  A pixel whose
 *       variance is NaN has NaN weights with halves, is weightless and keeps its colour: the colours stay finite.
 *   NaNs that the arithmetic generates, as opposed to the NaNs of the input that pass through with their bits, have unspecified sign
 *   and payload: only "is a NaN" is the same on every implementation.
 *   Finish.  The colour is remodulated.  out[p].color is the result, for !fin_p the input's bits; out[p].depth, normal and object_id
 *   are the input's bits.  rgba8_out (or NULL): the bytes rr_render_pixels writes for the record out[p], with params->gamma_correction
 *   as rr_config's.  variance_out (or NULL): the last var.
 * rr_denoise_params: struct_size = sizeof(rr_denoise_params); iterations 1 .. RR_MAX_DENOISE_ITERATIONS (pass i uses step 2^i);
 * normal_power_log2 0 .. 7; sigma_depth and sigma_luminance finite and above 0 (sigma_luminance is used only with halves).
 * rr_denoise_default_params writes 5 iterations, power 5, sigma_depth 0.05, sigma_luminance 4, no gamma; it never touches a device.
 * rr_denoise_records_device: records_dev width * height records (pixel (x, y) at y * width + x), halves_dev width * height * 2 records
 * in the K = 2 layout or NULL, albedo_dev width * height * 3 floats or NULL, out_dev width * height records.  The scene handle serves
 * for its device, its lock and the buffers it keeps, as for rr_refine_list_device: every pointer is classified before any launch
 * (RR_ERR_INVALID_ARGUMENT naming the argument); records_dev, halves_dev and out_dev 16-byte aligned, the others 4-byte aligned; work is
 * enqueued on `hip_stream` in stream order (the inputs may have been produced on that stream without a synchronisation); the scene's
 * lock; RR_ERR_INVALID_ARGUMENT from on_pass of the same scene.  Nothing of a frame's state or statistics is touched, and the call does
 * not wait inside; a scene edit or rr_scene_destroy waits for a call in flight.
 *   out_dev == records_dev (in place) is allowed.  Every other overlap between an output and an input, or between two outputs, is
 *   RR_ERR_INVALID_ARGUMENT.
 *   Refusals: a NULL scene, params, records or out; width or height 0 or above 65535; a struct_size other than
 *   sizeof(rr_denoise_params); iterations or power out of range; a sigma that is NaN, infinite or <= 0: RR_ERR_INVALID_ARGUMENT.
 *   width * height * 2 > 2^30: RR_ERR_UNSUPPORTED before anything is allocated.
 *   Memory kept by the handle until rr_scene_destroy: 56 B per pixel of the largest frame so far (two working colours of 16 B, the
 *   packed guide of 16 + 8 B).  A growth that fails is RR_ERR_OUT_OF_MEMORY and leaves the handle usable.
 * rr_denoise_records: the same on HOST pointers, the device form on the null stream behind a staging copy (32 + 32 B per pixel, and
 * 64, 12, 4 and 4 B for halves, albedo, rgba8_out and variance_out where given, in the pool of staging buffers the handle keeps for this
 * call, rr_accumulate_records, rr_accumulate_split_records (the most positions: sixteen) and rr_motion_records together: per argument
 * position the largest any of them has needed); it returns
 * with `out` written. */
#define RR_MAX_DENOISE_ITERATIONS 6u
typedef struct rr_denoise_params {
    uint32_t struct_size;        /* sizeof(rr_denoise_params) */
    uint32_t iterations;         /* 1 .. RR_MAX_DENOISE_ITERATIONS; pass i uses step 2^i */
    uint32_t normal_power_log2;  /* 0 .. 7: the normal weight is max(0, n_p . n_q) squared this many times */
    float    sigma_depth;        /* > 0, finite */
    float    sigma_luminance;    /* > 0, finite; used only with halves */
    uint32_t gamma_correction;   /* rgba8_out only, as rr_config's */
} rr_denoise_params;
int rr_denoise_default_params(rr_denoise_params* out);
int rr_denoise_records_device(rr_scene* scene, uint32_t width, uint32_t height, const rr_denoise_params* params,
                              const rr_radiance* records_dev /* width * height */, const rr_radiance* halves_dev /* width * height * 2, or NULL */,
                              const float* albedo_dev /* width * height * 3, or NULL */,
                              rr_radiance* out_dev /* width * height */, uint8_t* rgba8_out_dev /* or NULL */, float* variance_out_dev /* width * height, or NULL */,
                              void* hip_stream);
int rr_denoise_records(rr_scene* scene, uint32_t width, uint32_t height, const rr_denoise_params* params,
                       const rr_radiance* records /* width * height */, const rr_radiance* halves /* width * height * 2, or NULL */,
                       const float* albedo /* width * height * 3, or NULL */,
                       rr_radiance* out /* width * height */, uint8_t* rgba8_out /* or NULL */, float* variance_out /* width * height, or NULL */);

/* Temporal accumulation, the step a real-time denoiser takes before its spatial filter: the previous call's result is reprojected into
 * the current frame and the current records are blended into it, on the device.  Frame after frame of a few samples then converge
 * where nothing moved, and a pixel whose surface was not visible before starts anew.  With halves, each half accumulates its own
 * half-history with the same taps and weights: the two stay independent estimators, their difference remains the variance guide of
 * the accumulated mean, and rr_denoise_records takes out / halves_out as they are.
 * EVERY STEP IS EXACT IN BINARY32 IN THE ORDER STATED HERE, as for rr_denoise_records: no transcendentals, no contraction, division and
 * sqrt correctly rounded (rustray_amd/temporal.py: accumulate_records follows this text in numpy and gives the same bits).
 *   W, H = camera->width, height; n = W * H; pixel (x, y) is p = y * W + x.  dot(a, b) = (a.x*b.x + a.y*b.y) + a.z*b.z;
 *   row(M, r, v) = ((M[r]*v.x + M[4+r]*v.y) + M[8+r]*v.z) + M[12+r]*v.w for a column-major matrix; EPS = 2^-20.
 *   Per pixel p, with fin_p and valid_p of records[p] as rr_denoise_records defines them:
 *   1. No history: if history is NULL (the first frame), !fin_p or !valid_p (a miss has a NaN normal; a constant background has no noise
 *      to average), or where a later step says so: out[p], halves_out[2p] and halves_out[2p + 1] are the bits of records[p], halves[2p]
 *      and halves[2p + 1]; length_out[p] = 1 if fin_p, else 0.
 *   2. World point.  cx = (((float)x + 0.5f) / (float)W) * 2.0f - 1.0f, cy = 1.0f - (((float)y + 0.5f) / (float)H) * 2.0f.
 *      pp_r = row(projection_inverse, r, (cx, cy, -1, 1)), o_r = row(view_inverse, r, (pp, 1)), d_r = row(view_inverse, r, (pp, 0)), r = 0..2;
 *      len = sqrtf(dot(d, d)); world_r = o_r + (d_r / len) * depth_p; with motion, prev_r = world_r + motion[3p + r], else prev = world.
 *      (The ray of a frame without depth of field through the pixel's centre; its bits need not be the frame kernels'.)
 *   3. Reprojection.  clip_r = row(prev_world_to_clip, r, (prev, 1)) for r = 0, 1, 3.  No history unless clip.w > EPS.
 *      fx = ((clip.x / clip.w) * 0.5f + 0.5f) * (float)W - 0.5f;  fy = (0.5f - (clip.y / clip.w) * 0.5f) * (float)H - 0.5f.
 *      No history if fx or fy is not finite, or unless -1 < fx < W and -1 < fy < H (no tap would lie inside the frame).
 *      e = prev - prev_eye, dist = sqrtf(dot(e, e)), z_exp = dist - dist / clip.w: the depth the previous frame recorded for that point.
 *      A record's depth is measured from its ray's origin, which lies on the plane one unit ahead of the eye, not from the eye; of the
 *      distance to the eye the part before that plane is dist / clip.w, clip.w of a perspective projection (last row 0 0 -1 0 times the
 *      view) being the distance ahead of the eye.  prev_world_to_clip must be of that kind.
 *   4. Taps.  rx = rintf(fx), ry = rintf(fy) (ties to even).  If |fx - rx| <= snap and |fy - ry| <= snap: the one tap (rx, ry) with weight
 *      1, so that a static camera neither blurs nor drifts.  Otherwise x0 = floorf(fx), y0 = floorf(fy), tx = fx - x0, ty = fy - y0 and
 *      the four taps k = 0..3 in this order: (x0 + (k & 1), y0 + (k >> 1)) with weight (k & 1 ? tx : 1.0f - tx) * (k >> 1 ? ty : 1.0f - ty).
 *   5. A tap q is taken when it lies inside the frame; history[q].object_id == object_id_p; the three floats of history[q].normal are
 *      finite and dot(n_p, n_q) >= normal_min; the three floats of history[q].color and history[q].depth are finite and
 *      |z_exp - depth_q| <= sigma_depth * z_exp + EPS; history_length[q] > 0; and, with halves, the six colour floats of
 *      history_halves[2q] and [2q + 1] are finite.
 *   6. Blend.  Starting from 0, in tap order over the taken taps: sum_w += w; sum_l += w * history_length[q]; per channel and layer
 *      sum_c += w * c_q.  No history unless sum_w >= 2^-6.  Otherwise h = sum_c / sum_w per channel and layer, len = sum_l / sum_w,
 *      N = len + 1.0f; if not N < max_history then N = max_history; a = 1.0f / N;  out.color = h + a * (cur - h) per channel, each half
 *      with its own half-history; a current half whose colour is not finite keeps its bits.  length_out[p] = N.  Depth, normal and
 *      object_id of every output record are the bits of the current record of that layer.
 *   rgba8_out (or NULL): the bytes rr_render_pixels writes for the record out[p], with params->gamma_correction as rr_config's.
 * rr_accumulate_params: struct_size = sizeof(rr_accumulate_params); prev_world_to_clip: the previous frame's projection x view,
 * column-major (the host has both matrices; rr_camera holds only inverses) and prev_eye, its eye; max_history 1 .. 65536 caps the
 * length, so the blend factor never falls below 1 / max_history; normal_min in [-1, 1]; sigma_depth finite and above 0; snap in [0, 0.5).
 * rr_accumulate_default_params writes max_history 32, normal_min 0.9, sigma_depth 0.05, snap 1/64, no gamma, the identity matrix and
 * an eye of 0; it never touches a device.
 * rr_accumulate_records_device: records_dev n records, halves_dev 2n records in the K = 2 layout of rr_render_pixel_parts or NULL;
 * history_dev n records, the previous call's out; history_halves_dev 2n records, the previous call's halves_out; history_length_dev n
 * floats, the previous call's length_out (0: the pixel has no history); motion_dev 3n floats or NULL (nothing moved): the world-space
 * displacement per pixel, the surface point pixel p shows now lay at world_p + motion_p in the previous frame.  history_dev == NULL
 * together with history_length_dev == NULL (and history_halves_dev == NULL) is the first frame; one of the two without the other is
 * RR_ERR_INVALID_ARGUMENT.  With history, history_halves_dev is required exactly when halves_dev is given; halves_out_dev is required
 * exactly when halves_dev is given; out_dev and length_out_dev are required.
 *   The call follows rr_denoise_records_device: every pointer is classified before any launch (RR_ERR_INVALID_ARGUMENT naming the
 *   argument); the record pointers 16-byte aligned, the others 4-byte aligned; one launch (and one for the bytes) enqueued on `hip_stream`
 *   in stream order, not waited for; the scene's lock; RR_ERR_INVALID_ARGUMENT from on_pass of the same scene; nothing of a frame's state
 *   or statistics is touched; a scene edit or rr_scene_destroy waits for a call in flight.  The call keeps no device memory.
 *   out_dev == records_dev and halves_out_dev == halves_dev (in place on the current frame) are allowed: those are read at p only.  Every
 *   other overlap between an output and an input, or between two outputs, is RR_ERR_INVALID_ARGUMENT: history is gathered, so it can
 *   never be written by the call.  Callers ping-pong two sets of buffers.
 *   Refusals: a NULL scene, camera, params, records, out or length_out; width or height 0 or above 65535; a struct_size other than
 *   sizeof(rr_accumulate_params); max_history, normal_min, sigma_depth or snap out of range or NaN; the pairing rules above:
 *   RR_ERR_INVALID_ARGUMENT.  width * height * 2 > 2^30: RR_ERR_UNSUPPORTED before anything is allocated.
 * rr_accumulate_records: the same on HOST pointers, the device form on the null stream behind staging copies in the pool the handle keeps
 * until rr_scene_destroy, shared with rr_denoise_records (per pixel 32 B each for records, history and out, 64 B each for halves, history_halves and halves_out, 4 B each for
 * history_length, length_out and rgba8_out, 12 B for motion, each only where the call has it); it returns with the outputs written. */
typedef struct rr_accumulate_params {
    uint32_t struct_size;            /* sizeof(rr_accumulate_params) */
    float    prev_world_to_clip[16]; /* the previous frame's projection x view, column-major */
    float    prev_eye[3];
    float    max_history;            /* 1 .. 65536 */
    float    normal_min;             /* -1 .. 1 */
    float    sigma_depth;            /* > 0, finite */
    float    snap;                   /* 0 <= snap < 0.5, in pixels */
    uint32_t gamma_correction;       /* rgba8_out only, as rr_config's */
} rr_accumulate_params;
int rr_accumulate_default_params(rr_accumulate_params* out);
int rr_accumulate_records_device(rr_scene* scene, const rr_camera* camera, const rr_accumulate_params* params,
                                 const rr_radiance* records_dev /* n */, const rr_radiance* halves_dev /* 2n, or NULL */,
                                 const rr_radiance* history_dev /* n, or NULL */, const rr_radiance* history_halves_dev /* 2n, or NULL */,
                                 const float* history_length_dev /* n, or NULL */, const float* motion_dev /* 3n, or NULL */,
                                 rr_radiance* out_dev /* n */, rr_radiance* halves_out_dev /* 2n, or NULL */, float* length_out_dev /* n */,
                                 uint8_t* rgba8_out_dev /* or NULL */, void* hip_stream);
int rr_accumulate_records(rr_scene* scene, const rr_camera* camera, const rr_accumulate_params* params,
                          const rr_radiance* records /* n */, const rr_radiance* halves /* 2n, or NULL */,
                          const rr_radiance* history /* n, or NULL */, const rr_radiance* history_halves /* 2n, or NULL */,
                          const float* history_length /* n, or NULL */, const float* motion /* 3n, or NULL */,
                          rr_radiance* out /* n */, rr_radiance* halves_out /* 2n, or NULL */, float* length_out /* n */,
                          uint8_t* rgba8_out /* or NULL */);

/* Temporal accumulation of a split frame: rr_accumulate_records with the diffuse layers of rr_render_pixel_split blended by the same taps,
 * weights and length, in one launch.  The blend is linear, so the accumulated `color - diffuse` is the accumulated rest, and
 * rr_denoise_split_records takes out / halves_out / diffuse_out / diffuse_halves_out as they are.
 * The diffuse arrays have the layouts rr_render_pixel_split writes and rr_denoise_split_records reads: diffuse[3p + c], and for half h
 * of pixel p diffuse_halves[3(2p + h) + c].  rr_accumulate_params and rr_accumulate_default_params are rr_accumulate_records'.
 * EVERY STEP IS EXACT IN BINARY32 IN THE ORDER STATED HERE (rustray_amd/temporal.py: accumulate_split_records follows this text in numpy
 * and gives the same bits).  Steps 1 .. 6 are rr_accumulate_records'; this call adds to them:
 *   Taps.  The taken taps, their weights w, sum_w, sum_l, the no-history decision, N and a are exactly rr_accumulate_records' for the same
 *      records, halves, history, history_halves, history_length, motion and params.  No diffuse value takes part in any of those
 *      decisions.  Hence out, halves_out, length_out and rgba8_out are, bit for bit, what rr_accumulate_records writes for those arguments.
 *   Layers.  For each layer L of diffuse, diffuse half 0 and diffuse half 1 (the halves only when halves are given) there are three more
 *      sums: per channel sum_d += w * d_q with d_q the floats of the history of L at tap q, in tap order over the taken taps, starting
 *      from 0; hd = sum_d / sum_w.  A tap's diffuse floats are read after everything else of the tap, and only when it is taken.
 *   Output.  Where the pixel kept its history (length_out[p] = N of step 6), L at p is hd + a * (cur - hd) per channel, cur the current
 *      floats of L at p, if the three cur and the three hd are finite.  In every other case -- no history, the first frame, !fin_p,
 *      !valid_p, a current triple that is not finite, a history mean that is not finite -- the output holds the bits of the current L
 *      at p.
 *   Non-finite input.  After a non-finite diffuse float (current, or in a taken tap's history) that layer of the pixel restarts from its
 *      current value while length_out goes on counting for the colour: the layer's effective length is then shorter than length_out
 *      says.  rr_render_pixel_split never produces that: a colour channel that is not finite holds the same value in diffuse, and a
 *      pixel or tap whose colour is not finite has no history.
 *   NaNs.  With cur and hd finite and 0 < a <= 1 the blend can overflow to +-inf but cannot generate a NaN: the diffuse outputs are
 *      specified bit for bit, without the NaN clause of the records.
 * rr_accumulate_split_records_device: the arguments of rr_accumulate_records_device, and diffuse_dev 3n floats; diffuse_halves_dev 6n
 * floats; history_diffuse_dev 3n floats, the previous call's diffuse_out; history_diffuse_halves_dev 6n floats, the previous call's
 * diffuse_halves_out; diffuse_out_dev 3n and diffuse_halves_out_dev 6n floats.  diffuse_dev and diffuse_out_dev are required;
 * diffuse_halves_dev and diffuse_halves_out_dev exactly when halves_dev is given; history_diffuse_dev exactly when history_dev is;
 * history_diffuse_halves_dev exactly when history_halves_dev is; otherwise the pairing rules of rr_accumulate_records_device.
 *   The call follows rr_accumulate_records_device: every pointer is classified before any launch (RR_ERR_INVALID_ARGUMENT naming the
 *   argument; pageable memory is refused); the record pointers 16-byte aligned, the float pointers 4-byte aligned; one launch (and one for
 *   the bytes) enqueued on `hip_stream` in stream order, not waited for; the scene's lock; RR_ERR_INVALID_ARGUMENT from on_pass of the
 *   same scene; nothing of a frame's state or statistics is touched.  The call keeps no device memory.
 *   out_dev == records_dev, halves_out_dev == halves_dev, diffuse_out_dev == diffuse_dev and diffuse_halves_out_dev ==
 *   diffuse_halves_dev (in place on the current frame) are allowed: those are read at p only.  Every other overlap between an output and
 *   an input, or between two outputs, is RR_ERR_INVALID_ARGUMENT naming both.
 *   Refusals: those of rr_accumulate_records_device; a NULL diffuse or diffuse_out; the pairing rules above: RR_ERR_INVALID_ARGUMENT.
 *   width * height * 2 > 2^30: RR_ERR_UNSUPPORTED before anything is allocated.
 * rr_accumulate_split_records: the same on HOST pointers, the device form on the null stream behind staging copies in the handle's pool
 * (rr_accumulate_records' sizes, and per pixel 12 B each for diffuse, history_diffuse and diffuse_out, 24 B each for diffuse_halves,
 * history_diffuse_halves and diffuse_halves_out, each only where the call has it); it returns with the outputs written. */
int rr_accumulate_split_records_device(rr_scene* scene, const rr_camera* camera, const rr_accumulate_params* params,
                                       const rr_radiance* records_dev /* n */, const rr_radiance* halves_dev /* 2n, or NULL */,
                                       const float* diffuse_dev /* 3n */, const float* diffuse_halves_dev /* 6n; NULL exactly when halves_dev is */,
                                       const rr_radiance* history_dev /* n, or NULL */, const rr_radiance* history_halves_dev /* 2n, or NULL */,
                                       const float* history_diffuse_dev /* 3n, or NULL */, const float* history_diffuse_halves_dev /* 6n, or NULL */,
                                       const float* history_length_dev /* n, or NULL */, const float* motion_dev /* 3n, or NULL */,
                                       rr_radiance* out_dev /* n */, rr_radiance* halves_out_dev /* 2n, or NULL */,
                                       float* diffuse_out_dev /* 3n */, float* diffuse_halves_out_dev /* 6n, or NULL */,
                                       float* length_out_dev /* n */, uint8_t* rgba8_out_dev /* or NULL */, void* hip_stream);
int rr_accumulate_split_records(rr_scene* scene, const rr_camera* camera, const rr_accumulate_params* params,
                                const rr_radiance* records /* n */, const rr_radiance* halves /* 2n, or NULL */,
                                const float* diffuse /* 3n */, const float* diffuse_halves /* 6n; NULL exactly when halves is */,
                                const rr_radiance* history /* n, or NULL */, const rr_radiance* history_halves /* 2n, or NULL */,
                                const float* history_diffuse /* 3n, or NULL */, const float* history_diffuse_halves /* 6n, or NULL */,
                                const float* history_length /* n, or NULL */, const float* motion /* 3n, or NULL */,
                                rr_radiance* out /* n */, rr_radiance* halves_out /* 2n, or NULL */,
                                float* diffuse_out /* 3n */, float* diffuse_halves_out /* 6n, or NULL */,
                                float* length_out /* n */, uint8_t* rgba8_out /* or NULL */);

/* Temporal accumulation with the history held to the current frame's colours (neighbourhood variance clipping): rr_accumulate_records,
 * and before the blend each history mean is clamped to the box mean +- sigma_scale * sd of the current frame's colours in a 3x3 or 5x5
 * window around the pixel; where the record's history had to be moved, the length is shortened.  rr_accumulate_records decides from id,
 * normal and depth alone, so an edit that moves no geometry -- rr_scene_update_lights, rr_scene_update_materials,
 * rr_scene_add_textures, rr_scene_update_item_flags, a moved item's shadow or mirror image on a surface that stood still -- leaves the
 * stale colour in the blend for up to max_history frames; this call lets it go within a few.  The price is a bias towards the current
 * frame's noise in a static view (DESIGN.md has the measured figures).  rr_accumulate_params is rr_accumulate_records'.
 * EVERY STEP IS EXACT IN BINARY32 IN THE ORDER STATED HERE (rustray_amd/temporal.py: accumulate_clamped_records follows this text in numpy
 * and gives the same bits).  Steps 1 .. 6 are rr_accumulate_records' up to and including N and a; a pixel that reaches the end of step 6
 * with its means h (of the records), ha, hb (of the halves, when given), N and a goes on:
 *   7. Window.  r = radius.  The pixels q = (x + dx, y + dy) are visited with dy = -r .. r outside and dx = -r .. r inside, ascending.  q
 *      is taken when it lies inside the frame and the three colour floats of records[q] are finite; id, normal and depth are not looked
 *      at (p itself is always taken: fin_p holds).  Starting from 0: m += 1 (an integer); per channel s1 += c and s2 += c * c, the
 *      product rounded first.  Then per channel mean = s1 / (float)m; v = s2 / (float)m - mean * mean; sd = sqrtf(v > 0 ? v : 0) (a NaN
 *      gives 0); e = sigma_scale * sd; lo = mean - e; hi = mean + e.  There is one box per pixel, from the full records: the halves are
 *      clamped to the same box.
 *      A channel in which s2 / (float)m, mean * mean or e is not finite HAS NO BOX: lo = -inf, hi = +inf, and nothing is moved in it.
 *      That settles every overflow: an s2 that overflowed (one colour above about 1.85e19), whether mean * mean is still finite
 *      (v = inf) or overflowed as well (v = inf - inf, a NaN, which without this rule would give sd = 0 and a box that is the point
 *      `mean`, dragging the history of every pixel of the window to it); an s1 that overflowed (an infinite mean); an e that did.
 *   8. Clamp.  Per layer (h, ha, hb) and channel: h' = h < lo ? lo : (h > hi ? hi : h).  A NaN mean stays.
 *   9. Length.  Only the record layer decides.  If no channel of h was moved, N and a are step 6's.  Otherwise per channel
 *      u_c = fabsf(h_c - h'_c) / (e_c + EPS) where the channel was moved and 0 where not; t = max(max(u_0, u_1), u_2), each max(a, b)
 *      being a > b ? a : b; keep = 1.0f / (1.0f + t); N = (N - 1.0f) * keep + 1.0f; a = 1.0f / N.  (e_c of a moved channel is finite
 *      and >= 0, so u_c is >= 0 or +inf, keep lies in [0, 1] and the new N in [1, N]: no NaN arises.)
 *   10. Blend.  As step 6, with h', ha', hb' and the new a: out.color = h' + a * (cur - h') per channel, each half with its own clamped
 *      half-history; a current half whose colour is not finite keeps its bits.  length_out[p] = N.
 *   What follows from that and the tests hold: every no-history path (the first frame, !fin_p, !valid_p, step 3, sum_w < 2^-6) writes
 *   rr_accumulate_records' bits.  A pixel in which no channel of any layer leaves its box writes rr_accumulate_records' bits in every
 *   output.  A pixel in which only a half leaves the box differs from rr_accumulate_records' answer in that half alone.  Depth, normal
 *   and object_id of every output record are the bits of the current record of that layer.  sigma_scale 0 pulls every history mean
 *   onto the window's mean.
 * rr_history_clamp_params: struct_size = sizeof(rr_history_clamp_params); radius 1 (3x3) or 2 (5x5); sigma_scale finite, 0 .. 65536.
 * rr_history_clamp_default_params writes radius 1 and sigma_scale 0.5 (chosen by measurement: DESIGN.md section 8, item 24); it never
 * touches a device.
 * rr_accumulate_clamped_records_device: the arguments of rr_accumulate_records_device behind `clamp`, with its pairing rules.
 *   The call follows rr_accumulate_records_device: every pointer is classified before any launch (RR_ERR_INVALID_ARGUMENT naming the
 *   argument; pageable memory is refused); the record pointers 16-byte aligned, the others 4-byte aligned; ONE launch (and one for the
 *   bytes) enqueued on `hip_stream` in stream order, not waited for; the scene's lock; RR_ERR_INVALID_ARGUMENT from on_pass of the same
 *   scene; nothing of a frame's state or statistics is touched.  The call keeps no device memory.
 *   out_dev MAY NOT OVERLAP records_dev AT ALL, not even in place: the window reads the records of other pixels, which another
 *   workgroup may already have overwritten.  RR_ERR_INVALID_ARGUMENT, and rr_last_error names both and says why.  halves_out_dev ==
 *   halves_dev stays allowed: halves are read at p only.  Every other overlap between an output and an input, or between two outputs, is
 *   RR_ERR_INVALID_ARGUMENT naming both.
 *   Refusals: those of rr_accumulate_records_device; a NULL clamp; a clamp->struct_size other than sizeof(rr_history_clamp_params); a
 *   radius other than 1 or 2; a sigma_scale that is NaN, infinite, negative or above 65536: RR_ERR_INVALID_ARGUMENT naming the field and
 *   the function.  width * height * 2 > 2^30: RR_ERR_UNSUPPORTED before anything is allocated.
 * rr_accumulate_clamped_records: the same on HOST pointers (out may not overlap records there either), the device form on the null
 * stream behind staging copies in the handle's pool, ten arrays of rr_accumulate_records' sizes; it returns with the outputs written. */
typedef struct rr_history_clamp_params {
    uint32_t struct_size;   /* sizeof(rr_history_clamp_params) */
    uint32_t radius;        /* 1 or 2: a 3x3 or a 5x5 window of the CURRENT frame */
    float    sigma_scale;   /* k: finite, 0 .. 65536 */
} rr_history_clamp_params;
int rr_history_clamp_default_params(rr_history_clamp_params* out);
int rr_accumulate_clamped_records_device(rr_scene* scene, const rr_camera* camera, const rr_accumulate_params* params,
                                         const rr_history_clamp_params* clamp,
                                         const rr_radiance* records_dev /* n */, const rr_radiance* halves_dev /* 2n, or NULL */,
                                         const rr_radiance* history_dev /* n, or NULL */, const rr_radiance* history_halves_dev /* 2n, or NULL */,
                                         const float* history_length_dev /* n, or NULL */, const float* motion_dev /* 3n, or NULL */,
                                         rr_radiance* out_dev /* n; not records_dev */, rr_radiance* halves_out_dev /* 2n, or NULL */,
                                         float* length_out_dev /* n */, uint8_t* rgba8_out_dev /* or NULL */, void* hip_stream);
int rr_accumulate_clamped_records(rr_scene* scene, const rr_camera* camera, const rr_accumulate_params* params,
                                  const rr_history_clamp_params* clamp,
                                  const rr_radiance* records /* n */, const rr_radiance* halves /* 2n, or NULL */,
                                  const rr_radiance* history /* n, or NULL */, const rr_radiance* history_halves /* 2n, or NULL */,
                                  const float* history_length /* n, or NULL */, const float* motion /* 3n, or NULL */,
                                  rr_radiance* out /* n; not records */, rr_radiance* halves_out /* 2n, or NULL */, float* length_out /* n */,
                                  uint8_t* rgba8_out /* or NULL */);

/* Temporal accumulation of a split frame with the history held to the current frame: rr_accumulate_split_records with the clamp of
 * rr_accumulate_clamped_records on the colour layers and a clamp of its own on the diffuse layers, in one launch -- the split pipeline
 * for a scene whose lights, materials, textures or flags are edited while it is shown.  rr_accumulate_params, rr_history_clamp_params,
 * its ranges and rr_history_clamp_default_params are those of the two calls; the diffuse arrays have rr_accumulate_split_records' layouts.
 * EVERY STEP IS EXACT IN BINARY32 IN THE ORDER STATED HERE (rustray_amd/temporal.py: accumulate_clamped_split_records follows this text
 * in numpy and gives the same bits):
 *   Colour side.  Steps 1 .. 10 of rr_accumulate_clamped_records for the same records, halves, history, history_halves, history_length,
 *      motion, params and clamp.  No diffuse value takes part in any decision about taps, sum_w, the colour box, N or a.  Hence out,
 *      halves_out, length_out and rgba8_out are, bit for bit, what rr_accumulate_clamped_records writes for those arguments.
 *   Diffuse means.  As rr_accumulate_split_records: for each layer L of diffuse, diffuse half 0 and diffuse half 1 (the halves only when
 *      halves are given) per channel sum_d += w * d_q in tap order over the taken taps, starting from 0; hd = sum_d / sum_w.  A tap's
 *      diffuse floats are read after everything else of the tap, and only when it is taken.
 *   Diffuse box.  One per pixel that kept its history, from the current `diffuse` array (the full layer, not the halves), in the window
 *      order of step 7: dy = -r .. r outside, dx = -r .. r inside, ascending.  q is taken when it lies inside the frame and the three
 *      floats of diffuse at q are finite, whatever its colour holds.  The sums m, s1, s2, then mean, v, sd, e = sigma_scale * sd,
 *      lo = mean - e and hi = mean + e are step 7's, and so is its rule that a channel in which s2 / (float)m, mean * mean or e is not
 *      finite has no box (lo = -inf, hi = +inf).  Unlike the colour window, p itself may fail the test; if nothing is taken, m = 0,
 *      s1 / 0.0f = 0.0f / 0.0f is a NaN, so is mean * mean, and by that rule no channel has a box.  Both diffuse halves are clamped to this
 *      one box.
 *   Diffuse clamp and blend.  Where the pixel kept its history and, for layer L, the three current floats cur of L at p and the three hd
 *      are finite: hd' = hd < lo ? lo : (hd > hi ? hi : hd) per channel, and L at p is hd' + a * (cur - hd') with the FINAL a of the
 *      colour side, after step 9.  In every other case -- no history, the first frame, !fin_p, !valid_p, a current triple that is not
 *      finite, a history mean that is not finite -- the output holds the bits of the current L at p, as rr_accumulate_split_records says
 *      (an infinite hd is NOT pulled onto a finite bound).  A moved diffuse layer does not shorten the length: only the record layer
 *      decides it, in step 9.
 *   What follows from that and the tests hold: every no-history path writes rr_accumulate_split_records' bits in all outputs.  A pixel
 *      whose record layer was not moved (so N and a are step 6's) and in which a diffuse layer L stays inside the diffuse box has L's bits
 *      from rr_accumulate_split_records.  A pixel in which no layer of either kind leaves its box equals rr_accumulate_split_records in
 *      every output.  With cur and hd' finite and 0 < a <= 1 the diffuse blend cannot generate a NaN: the diffuse outputs are specified bit
 *      for bit.
 * rr_accumulate_clamped_split_records_device: the arguments of rr_accumulate_split_records_device in its order, `clamp` behind `params`;
 * the pairing rules of rr_accumulate_split_records_device.
 *   The call follows that one: every pointer is classified before any launch (RR_ERR_INVALID_ARGUMENT naming the argument; pageable
 *   memory is refused); the record pointers 16-byte aligned, the float pointers 4-byte aligned; ONE launch (and one for the bytes)
 *   enqueued on `hip_stream` in stream order, not waited for; the scene's lock; RR_ERR_INVALID_ARGUMENT from on_pass of the same scene;
 *   nothing of a frame's state or statistics is touched.  The call keeps no device memory.
 *   out_dev MAY NOT OVERLAP records_dev AND diffuse_out_dev MAY NOT OVERLAP diffuse_dev AT ALL, not even in place: the windows read the
 *   records and the diffuse of other pixels, which another workgroup may already have overwritten.  RR_ERR_INVALID_ARGUMENT, and
 *   rr_last_error names both and says why.  halves_out_dev == halves_dev and diffuse_halves_out_dev == diffuse_halves_dev stay allowed:
 *   those are read at p only.  Every other overlap between an output and an input, or between two outputs, is RR_ERR_INVALID_ARGUMENT
 *   naming both.
 *   Refusals: those of rr_accumulate_split_records_device and those of rr_accumulate_clamped_records_device for `clamp`, each naming the
 *   argument or field and the function.  width * height * 2 > 2^30: RR_ERR_UNSUPPORTED before anything is allocated.
 * rr_accumulate_clamped_split_records: the same on HOST pointers (the two overlaps are refused there too), the device form on the null
 * stream behind staging copies in the handle's pool, sixteen arrays of rr_accumulate_split_records' sizes; it returns with the outputs
 * written. */
int rr_accumulate_clamped_split_records_device(rr_scene* scene, const rr_camera* camera, const rr_accumulate_params* params,
                                               const rr_history_clamp_params* clamp,
                                               const rr_radiance* records_dev /* n */, const rr_radiance* halves_dev /* 2n, or NULL */,
                                               const float* diffuse_dev /* 3n */, const float* diffuse_halves_dev /* 6n; NULL exactly when halves_dev is */,
                                               const rr_radiance* history_dev /* n, or NULL */, const rr_radiance* history_halves_dev /* 2n, or NULL */,
                                               const float* history_diffuse_dev /* 3n, or NULL */, const float* history_diffuse_halves_dev /* 6n, or NULL */,
                                               const float* history_length_dev /* n, or NULL */, const float* motion_dev /* 3n, or NULL */,
                                               rr_radiance* out_dev /* n; not records_dev */, rr_radiance* halves_out_dev /* 2n, or NULL */,
                                               float* diffuse_out_dev /* 3n; not diffuse_dev */, float* diffuse_halves_out_dev /* 6n, or NULL */,
                                               float* length_out_dev /* n */, uint8_t* rgba8_out_dev /* or NULL */, void* hip_stream);
int rr_accumulate_clamped_split_records(rr_scene* scene, const rr_camera* camera, const rr_accumulate_params* params,
                                        const rr_history_clamp_params* clamp,
                                        const rr_radiance* records /* n */, const rr_radiance* halves /* 2n, or NULL */,
                                        const float* diffuse /* 3n */, const float* diffuse_halves /* 6n; NULL exactly when halves is */,
                                        const rr_radiance* history /* n, or NULL */, const rr_radiance* history_halves /* 2n, or NULL */,
                                        const float* history_diffuse /* 3n, or NULL */, const float* history_diffuse_halves /* 6n, or NULL */,
                                        const float* history_length /* n, or NULL */, const float* motion /* 3n, or NULL */,
                                        rr_radiance* out /* n; not records */, rr_radiance* halves_out /* 2n, or NULL */,
                                        float* diffuse_out /* 3n; not diffuse */, float* diffuse_halves_out /* 6n, or NULL */,
                                        float* length_out /* n */, uint8_t* rgba8_out /* or NULL */);

/* The motion of moved items per pixel: what rr_accumulate_records takes as motion when items moved between the frame the history was
 * rendered from and the current one (rr_scene_update_transforms, rr_scene_set_items), computed on the device from the records it holds.
 * A call names n_moved items by index; for each, prev_trans + 16 k is the item's `trans` in the frame of the history, column-major.
 * inv_i is the item's trans_inv as the handle holds it now -- the one the current frame was traced with, from rr_scene_create, the
 * last rr_scene_update_transforms or rr_scene_set_items -- and id_i its object_id (ShapeBasics::id).
 * EVERY STEP IS EXACT IN BINARY32 IN THE ORDER STATED HERE, as for rr_accumulate_records, whose row and dot these are
 * (rustray_amd/temporal.py: motion_records follows this text in numpy and gives the same bits).
 *   Per pixel p of the camera->width x camera->height frame:
 *   1. world_p: step 2 of rr_accumulate_records, for every pixel whatever its record holds (a NaN it generates has no specified sign or
 *      payload).  world_out[3p ..] (or NULL) gets it.
 *   2. motion_p = (0, 0, 0) unless valid_p holds (depth and the three floats of the normal are finite, as rr_denoise_records defines it)
 *      and records[p].object_id equals some id_i.  A miss has a NaN normal, so an item of id 0 does not drag the background.
 *   3. Otherwise local_r = row(inv_i, r, (world_p, 1)), prev_r = row(prev_trans_i, r, (local, 1)), m_r = prev_r - world_p[r], r = 0..2;
 *      if any m_r is not finite all three are 0.  motion_out[3p + r] = m_r.
 *   The object id is the key, because a record holds no item index.  Two LISTED items with the same id: RR_ERR_INVALID_ARGUMENT naming
 *   both entries.  THE CALLER'S CONTRACT: an unlisted item that shares a listed item's id moves with it (the reference hands out unique ids).
 * rr_motion_records_device: records_dev n records (n = width * height), motion_out_dev 3n floats, world_out_dev 3n floats or NULL.  The
 *   rules are rr_accumulate_records_device's: every device pointer is classified before any launch (RR_ERR_INVALID_ARGUMENT naming the
 *   argument); records_dev 16-byte aligned, the outputs 4-byte aligned; no overlap between an output and the input or between the two
 *   outputs; the work (one copy of the table and one launch; with n_moved == 0 and no world_out one fill) is enqueued on `hip_stream` in
 *   stream order and not waited for, and the records may come from that stream unsynchronised; the scene's lock;
 *   RR_ERR_INVALID_ARGUMENT from on_pass of the same scene; RR_ERR_DEVICE on a scene that a failed update left broken; nothing of a
 *   frame's state or statistics is touched; a scene edit or rr_scene_destroy waits for a call in flight.
 *   item_index and prev_trans are HOST arrays, read before the call returns.  The table made from them (112 B per entry, sorted by id)
 *   goes into a buffer of the handle, sized for the largest list so far and kept until rr_scene_destroy, through one of four pinned
 *   copies of the same size, used in turn; a failed growth is RR_ERR_OUT_OF_MEMORY and leaves the handle usable.  That buffer is
 *   shared: a call on a different stream from the handle's last call first waits for that stream, as the query buffers do; a call on
 *   the same stream waits only until the table copy of the fourth call before it has run.
 *   Refusals: a NULL scene, camera, records or motion output; width or height 0 or above 65535; n_moved > the scene's item count; with
 *   n_moved > 0 a NULL item_index or prev_trans; an item_index[k] >= the item count; a prev_trans that is not finite (naming the entry);
 *   two listed items of one id: RR_ERR_INVALID_ARGUMENT, nothing launched.  width * height * 2 > 2^30: RR_ERR_UNSUPPORTED.
 * rr_motion_records: the same on HOST pointers, the device form on the null stream behind staging copies in the pool the handle keeps
 * until rr_scene_destroy, shared with rr_denoise_records (32 B per pixel for the records, 12 B for motion_out and 12 B for world_out where given); it returns with the
 * outputs written. */
int rr_motion_records_device(rr_scene* scene, const rr_camera* camera, const uint32_t* item_index /* HOST, n_moved */,
                             const float* prev_trans /* HOST, n_moved * 16 */, uint32_t n_moved, const rr_radiance* records_dev /* n */,
                             float* motion_out_dev /* 3n */, float* world_out_dev /* 3n, or NULL */, void* hip_stream);
int rr_motion_records(rr_scene* scene, const rr_camera* camera, const uint32_t* item_index, const float* prev_trans, uint32_t n_moved,
                      const rr_radiance* records /* n */, float* motion_out /* 3n */, float* world_out /* 3n, or NULL */);

/* The camera's surface per pixel: rr_surface_rays for the pinhole ray through the centre of each pixel, made on the device from the
 * camera -- the G-buffer of the frame, and the albedo rr_denoise_records takes.  As rr_render_pixels is the frame's camera per pixel for
 * radiance, this is the frame's camera per pixel for the surface.  There is no rr_config: no depth of field, no sub-sample table, no
 * generator; the call is deterministic, as rr_surface_rays is.
 * THE RAY OF A PIXEL.  The ray of pixel (x, y) of the camera->width x camera->height frame (w, h as floats) passes through the pixel's
 *   centre, the screen point rr_render_pixels gives it: cx = ((x + 0.5f) / w) * 2 - 1, cy = 1 - ((y + 0.5f) / h) * 2.  With
 *   row(m, r, v) = ((m[r]*v.x + m[4+r]*v.y) + m[8+r]*v.z) + m[12+r]*v.w over a column-major matrix:
 *     pp_r = row(projection_inverse, r, (cx, cy, -1, 1)),  origin_r = row(view_inverse, r, (pp, 1)),  u_r = row(view_inverse, r, (pp, 0)),
 *     direction_r = u_r / sqrtf((u.x*u.x + u.y*u.y) + u.z*u.z),  r = 0 .. 2.
 *   EVERY STEP IS EXACT IN BINARY32 IN THE ORDER STATED HERE, without contraction: these are bit for bit the o and d of step 2 of
 *   rr_accumulate_records (one function serves both), and rustray_amd/pixel_rays.py: pixel_rays follows this text in numpy and gives the
 *   same bits.
 *   out[i] (or NULL): byte for byte the record rr_surface_rays writes for that ray at depth 1 under the same handle state; for a miss
 *   {0, 0xffffffff, 0, 0} and 112 zero bytes.  position is origin + direction * distance, which makes it bit for bit the world point
 *   step 2 of rr_accumulate_records forms from a record whose depth is `distance`.
 *   albedo_out[3i .. 3i + 2] (or NULL): the bits of out[i].base_color[0 .. 2]; three zeros for a miss (the denoiser leaves a channel
 *   whose albedo is 0 alone).  This is the array rr_denoise_records(_device) takes as `albedo`.  It is the albedo of the FIRST hit of
 *   the pixel's centre: not seen through a mirror or glass, not averaged over the frame's sub-samples.
 *   At least one of the two outputs is required: both NULL is RR_ERR_INVALID_ARGUMENT.
 *   The list form and the NULL list are rr_render_pixels': pixel_xy NULL needs n_pixels == width * height, and pixel (x, y) goes to index
 *   y * width + x; else entry i = x | y << 16 answers index i, duplicates and any order allowed, and an entry outside the frame is
 *   RR_ERR_INVALID_ARGUMENT naming its index, with nothing written.  n_pixels == 0 returns RR_OK and touches nothing;
 *   n_pixels > 0x7fffff00: RR_ERR_UNSUPPORTED.  The camera checks are rr_render_pixels' (width or height 0 or above 65535, a matrix that
 *   is not finite: RR_ERR_INVALID_ARGUMENT).  The checks come in this order: a NULL scene or camera; both outputs NULL; the camera; the
 *   pixel limit; n_pixels == 0 (RR_OK); n_pixels against the frame without a list; (device form) alignment, then overlap; the scene; the
 *   pointers; the list.
 *   It is a frame call in the sense of rr_surface_rays: the scene's lock; RR_ERR_INVALID_ARGUMENT from on_pass of the same scene;
 *   RR_ERR_DEVICE on a scene that a failed update left broken; nothing of a frame's accumulators, counters or rr_scene_last_stats is
 *   touched, and the frames before and after are bit-identical.
 * rr_surface_pixels_device: pixel_xy_dev n_pixels entries or NULL, out_dev n_pixels records or NULL, albedo_out_dev 3 * n_pixels floats
 *   or NULL, all memory the scene's device can address: every pointer is classified before any launch, as rr_trace_rays_device does it
 *   (RR_ERR_INVALID_ARGUMENT naming the argument).  out_dev 16-byte aligned, albedo_out_dev and pixel_xy_dev 4-byte aligned; any overlap
 *   of the two outputs with each other or with the list is refused.  The work is enqueued on `hip_stream` in stream order, and the list
 *   may come from that stream unsynchronised.  The rays' origins are a function of the camera alone, so the reach the top level must be
 *   padded for is known on the host before the first launch (each origin component is affine in (cx, cy): its largest magnitude lies at
 *   one of the four corner pixels, evaluated in double with the margin 1.001 and the binary32 rounding added).  THE WHOLE-FRAME FORM
 *   THEREFORE WAITS FOR NOTHING: it enqueues and returns.  (Two exceptions, both one-time: a camera farther from the scene than any
 *   call before rebuilds the top level, which waits for the device; a frame larger than any query before grows the working memory.)
 *   The list form waits once for 4 bytes, the first index outside the frame, as rr_render_pixels_device does.  A call that ends early
 *   leaves the stream idle.  Working memory: the handle's query buffers, shared with the ray queries and kept until rr_scene_destroy
 *   (56 B per pixel of the largest query so far, 4 B more for the whole-frame form); a call on a different stream from the handle's last
 *   call first waits for that stream.  A scene edit or rr_scene_destroy waits for a call in flight.
 * rr_surface_pixels: the same on HOST pointers, the device form on the null stream behind staging copies in buffers of the call (4 B of
 *   list, 128 B and 12 B of answers per pixel, each only where the call has it), freed on return; the list is checked before anything
 *   is uploaded, and the call returns with the outputs written. */
int rr_surface_pixels(rr_scene* scene, const rr_camera* camera, const uint32_t* pixel_xy /* n_pixels, or NULL */, uint32_t n_pixels,
                      rr_surface_hit* out /* n_pixels, or NULL */, float* albedo_out /* n_pixels * 3, or NULL */);
int rr_surface_pixels_device(rr_scene* scene, const rr_camera* camera, const uint32_t* pixel_xy_dev /* n_pixels, or NULL */, uint32_t n_pixels,
                             rr_surface_hit* out_dev /* n_pixels, or NULL */, float* albedo_out_dev /* n_pixels * 3, or NULL */, void* hip_stream);

/* The frame's albedo per pixel: the mean, over the S = config->samples primary rays rr_render_pixels traces for the pixel, of the base
 * colour at each ray's first hit -- the albedo the pixel's colour was actually modulated by.  rr_surface_pixels gives the one colour
 * under the pixel's centre; a pixel on a texture edge, a silhouette or out of focus holds a mix, and rr_denoise_records divides by the
 * wrong value there.  This is the array to pass as its `albedo` instead.
 * RAYS.  Ray (p, s) is the primary ray rr_render_pixels derives for list entry (or pixel) p and frame sample s: the same slot tables, the
 *   same sub-sample table (sample_xy, or the built-in one when NULL) with the cell size of config->samples, the same depth-of-field
 *   branch (focal_length and aperture_size both above 1).  Of the config, samples, focal_length and aperture_size are used; the whole
 *   config is checked as every frame call checks it, then seed, monte_carlo, max_recursion, the fog and gamma_correction are ignored.
 *   Nothing is drawn from the generator: the call is deterministic.
 * TERM.  a(p, s) = base_color[0 .. 2] of the rr_surface_hit rr_surface_rays writes for that (normalised) ray at depth 1 under the same
 *   handle state -- the same evaluation in full, so the bits are the record's; (0, 0, 0) for a miss, as a miss adds 0 to the pixel's colour.
 * SUM.  Exactly rr_radiance.color's: every term is clamped to +-32768, scaled by 2^24 and rounded to nearest-even by itself, the terms are
 *   added as integers, and albedo_out[3p + c] = (float)(sum * 2^-24) / (float)S.  A NaN term adds 0 and makes the channel NaN, a +inf
 *   (-inf) term makes it +inf (-inf), both in one pixel and channel make it NaN -- as a frame's colour.  Integer adds commute: the
 *   result does not depend on batching, sample groups, chunks or rr_tuning.  rustray_amd/albedo.py: mean_albedo follows this text in numpy.
 * LIST AND WHOLE FRAME are rr_render_pixels': pixel_xy NULL needs n_pixels == width * height and pixel (x, y) goes to index y * width + x;
 *   else entry i = x | y << 16 answers index i, duplicates and any order allowed, a length that is no multiple of 64 / G runs with G = 1,
 *   and an entry outside the frame is RR_ERR_INVALID_ARGUMENT naming its index, with nothing written.  n_pixels == 0 returns RR_OK and
 *   touches nothing; n_pixels > 2^30 is RR_ERR_UNSUPPORTED before anything is allocated; albedo_out == NULL is RR_ERR_INVALID_ARGUMENT.
 *   The checks come in this order: scene, camera, config and table as rr_render checks them; albedo_out; the pixel limit; n_pixels == 0
 *   (RR_OK); n_pixels against the frame without a list; (device form) alignment, then overlap; (host form) the list; the scene; the
 *   pointers; (device form) the list.
 * A FRAME CALL in the sense of rr_render_pixels: the scene's lock; RR_ERR_INVALID_ARGUMENT from on_pass of the same scene; RR_ERR_DEVICE
 *   on a scene that a failed update left broken; rr_scene_last_stats afterwards reports primary_rays = n_pixels * samples and zero
 *   secondary_rays, shadow_rays and shaded_hits.  cancel: as rr_shade_rays.  The frames before and after are bit-identical: the list's
 *   slot table is the call's own, and the accumulators are cleared by every frame.
 * rr_albedo_pixels_device: pixel_xy_dev n_pixels entries or NULL and albedo_out_dev 3 * n_pixels floats, memory the scene's device can
 *   address, under every rule of rr_render_pixels_device: pointers classified before any launch (RR_ERR_INVALID_ARGUMENT naming the
 *   argument), both 4-byte aligned, an overlap of the two refused; camera, config and sample_xy are host memory.  The work is enqueued on
 *   `hip_stream` in stream order and the list may come from that stream unsynchronised: it is copied into the handle's buffer first, so
 *   nothing the launches read after the return is the caller's.  The call waits where a frame waits for its constants and, with a list,
 *   once for 4 bytes: the first index outside the frame.  It never waits for the size of a level, because nothing spawns.  A call that
 *   ends early leaves the stream idle.  Device memory, kept by the handle until rr_scene_destroy and shared with the frames: 28 B per
 *   pixel of accumulators (the colour planes and the flags), 16 B of hit records per primary ray of a batch, 12 B per list entry; no ray
 *   arena and no shadow queue is sized for the call.
 * rr_albedo_pixels: the same on HOST pointers, the device form on the null stream behind staging copies in buffers of the call (4 B of
 *   list and 12 B of answer per pixel), freed on return; the list is checked before anything is uploaded, and the call returns with the
 *   output written. */
int rr_albedo_pixels(rr_scene* scene, const rr_camera* camera, const rr_config* config, const uint16_t* sample_xy /* or NULL */,
                     const uint32_t* pixel_xy /* or NULL */, uint32_t n_pixels,
                     float* albedo_out /* n_pixels * 3 */, const volatile int* cancel);
int rr_albedo_pixels_device(rr_scene* scene, const rr_camera* camera, const rr_config* config, const uint16_t* sample_xy /* or NULL */,
                            const uint32_t* pixel_xy_dev /* or NULL */, uint32_t n_pixels,
                            float* albedo_out_dev /* n_pixels * 3 */, void* hip_stream, const volatile int* cancel);

/* A frame's records and, as a sum of its own, the DIRECT DIFFUSE light of its primary hits: the part of a pixel's colour that the base
 * colour of the surface under it modulates.  What is left, out.color - diffuse, is "rest": ambient and fog, highlights, and everything
 * behind mirrors and glass.  rr_denoise_split_records takes the pair; the diffuse pass is also what a compositor relights.
 * RECORDS.  out and halves_out are, bit for bit, what rr_render_pixel_parts writes at n_parts = 2 for the same arguments (out and parts_out);
 *   with halves_out == NULL, out is what rr_render_pixels writes.  The list and whole-frame rules are rr_render_pixels'.
 * TERM.  For every hit of depth 1 (a primary ray's own hit) and every enabled light, with the names of the shading step,
 *   d[c] = ((light.color[c] * (base_color[c] * dot_light)) * intensity) * w_light, in exactly this order of binary32 operations: the light's
 *   term of the frame with the specular product left out.  It is multiplied by the shadow factor the light's shadow ray gets for the whole
 *   term (1 for a receiver that takes no shadows, and no term where the whole term is exactly 0).  A miss adds 0; hits of depth 2 and
 *   deeper add nothing.
 * SUM.  Exactly rr_radiance.color's: every term clamped to +-32768, scaled by 2^24 and rounded to nearest-even by itself, added as an
 *   integer; diffuse_out[3p + c] = (float)(sum * 2^-24) / (float)S, and diffuse_halves_out[3 (2p + h) + c] the same over the half's S / 2
 *   samples (half h = the samples s with s mod 2 == h).  Integer adds commute: the result does not depend on batching, chunks or rr_tuning.
 *   A channel whose record colour is not finite (NaN, +-inf) holds the record's value in diffuse_out too; no second set of flags is kept.
 * ARGUMENTS.  out and diffuse_out are required; halves_out and diffuse_halves_out are given together or not at all, and with them
 *   config->samples must be even (RR_ERR_INVALID_ARGUMENT, the message of rr_render_pixel_parts).  n_pixels == 0 returns RR_OK and touches
 *   nothing; n_pixels (x 2 with halves) above 2^30 is RR_ERR_UNSUPPORTED.
 * A FRAME CALL in the sense of rr_render_pixels: the scene's lock; RR_ERR_INVALID_ARGUMENT from on_pass of the same scene; cancel as
 *   rr_render_pixel_parts; rr_scene_last_stats reports the counters rr_render_pixel_parts reports for the same frame; the frames before
 *   and after are bit-identical.  Level 1 of the call runs its shade and shadow launches one after the other on the call's stream.
 * rr_render_pixel_split_device: buffers the scene's device can address, in stream order, under every rule of rr_render_pixels_device:
 *   pointers classified before any launch, out_dev and halves_out_dev 16-byte aligned, the others 4-byte aligned, overlaps refused; the
 *   list may come from the stream unsynchronised.  A call that ends early leaves the stream idle.  Device memory kept by the handle until
 *   rr_scene_destroy, beyond rr_render_pixel_parts' own: 24 B per accumulator slot and 16 B per ray of the shadow queue.
 * rr_render_pixel_split: the same on HOST pointers, the device form on the null stream behind staging copies in buffers of the call, freed on
 *   return; the list is checked before anything is uploaded, and the call returns with the outputs written. */
int rr_render_pixel_split(rr_scene* scene, const rr_camera* camera, const rr_config* config, const uint16_t* sample_xy /* or NULL */,
                          const uint32_t* pixel_xy /* or NULL */, uint32_t n_pixels,
                          rr_radiance* out /* n_pixels */, rr_radiance* halves_out /* n_pixels * 2, or NULL */,
                          float* diffuse_out /* n_pixels * 3 */, float* diffuse_halves_out /* n_pixels * 2 * 3; NULL exactly when halves_out is */,
                          const volatile int* cancel);
int rr_render_pixel_split_device(rr_scene* scene, const rr_camera* camera, const rr_config* config, const uint16_t* sample_xy /* or NULL */,
                                 const uint32_t* pixel_xy_dev /* or NULL */, uint32_t n_pixels,
                                 rr_radiance* out_dev /* n_pixels */, rr_radiance* halves_out_dev /* n_pixels * 2, or NULL */,
                                 float* diffuse_out_dev /* n_pixels * 3 */,
                                 float* diffuse_halves_out_dev /* n_pixels * 2 * 3; NULL exactly when halves_out_dev is */,
                                 void* hip_stream, const volatile int* cancel);

/* rr_denoise_records with the albedo applied to the direct diffuse part of the colour alone.  Two record sets share depth, normal and id
 * with `records`: REST, whose colour is records.color - diffuse (one binary32 subtraction per channel), and DIRECT, whose colour is diffuse;
 * halves and diffuse_halves (given together or not at all) are split the same way.  out.color = F(rest, rest halves, no albedo).color +
 * F(direct, direct halves, albedo).color, one binary32 add per channel, with F the filter of rr_denoise_records under `params`, every
 * step exact in binary32 as stated there; a pixel whose record colour is not finite keeps the record's colour.  Depth, normal and id
 * are the record's bits.  rgba8_out (or NULL) gets the bytes of out as rr_denoise_records writes them; no variance is offered.
 * rustray_amd/denoise.py: atrous_denoise_split follows this text in numpy, and the result equals it bit for bit.
 * Arguments, refusals, alignment, the in-place rule (out == records) and the stream order are rr_denoise_records(_device)'s; diffuse is
 * width * height * 3 floats and required, diffuse_halves width * height * 2 * 3 floats, both 4-byte aligned in the device form, neither
 * overlapping an output.  Device memory kept by the handle until rr_scene_destroy, beyond rr_denoise_records' own: 64 B per pixel, and
 * 128 B more with halves. */
int rr_denoise_split_records_device(rr_scene* scene, uint32_t width, uint32_t height, const rr_denoise_params* params,
                                    const rr_radiance* records_dev, const rr_radiance* halves_dev /* or NULL */,
                                    const float* diffuse_dev, const float* diffuse_halves_dev /* NULL exactly when halves_dev is */,
                                    const float* albedo_dev /* or NULL */, rr_radiance* out_dev, uint8_t* rgba8_out_dev /* or NULL */,
                                    void* hip_stream);
int rr_denoise_split_records(rr_scene* scene, uint32_t width, uint32_t height, const rr_denoise_params* params,
                             const rr_radiance* records, const rr_radiance* halves /* or NULL */,
                             const float* diffuse, const float* diffuse_halves /* NULL exactly when halves is */,
                             const float* albedo /* or NULL */, rr_radiance* out, uint8_t* rgba8_out /* or NULL */);

/* A frame traced at a LOW resolution raised to the full one: a joint-bilateral upsampler guided by the G-buffer of the camera at both
 * sizes.  Every call above works at the resolution that was traced; this one lets a caller trace low_width x low_height pixels (a quarter
 * of the primary rays at half the size each way) and show width x height.  The two guides are rr_surface_pixels(_device) of two cameras
 * with the same matrices and the two sizes, which cost no shading; low and halves_low are rr_render_pixel_parts at n_parts = 2 on the
 * small camera.  out (and halves_out) is a valid input of rr_denoise_records, rr_accumulate_records and rr_motion_records at width x height.
 * EVERY STEP IS EXACT IN BINARY32 IN THE ORDER STATED HERE, as for rr_denoise_records: no transcendentals, no contraction, division
 * correctly rounded; rustray_amd/upsample.py: upsample_records follows this text in numpy and gives the same bits.
 *   W x H = width x height, w x h = low_width x low_height, 1 <= w <= W <= 65535 and 1 <= h <= H <= 65535; the ratios need not be whole.
 *   low[q] (w * h records, pixel (x, y) at y * w + x) is the traced colour; halves_low (or NULL) w * h * 2 records in the K = 2 layout;
 *   guide_low[q] (w * h) and guide[p] (W * H) are rr_surface_hit records, of which only rows 0, 1, 2 and 4 are read: hit, object_id,
 *   distance, normal, base_color[0 .. 2].
 *   fin_q: the three colour floats of low[q] are finite.  valid of a guide: hit != 0, and distance and the three normal floats are finite.
 *   Position of full pixel (x, y) in the low frame: u = (((float)x + 0.5f) * (float)w) / (float)W - 0.5f, x0 = (int)floorf(u),
 *   fx = u - (float)x0; the same for v, y0, fy with h and H.  The four taps are q = (x0 + dx, y0 + dy), dy outer, dx inner, each in
 *   {0, 1}; b = (dx ? fx : 1.0f - fx) * (dy ? fy : 1.0f - fy).  r = max((float)W / (float)w, (float)H / (float)h), once per call.
 *   Guided sum.  A tap is skipped when q is outside the low frame; !fin_q; (guide_low[q].hit != 0) != (guide[p].hit != 0); both hit and
 *   the object_ids differ; or valid_q != valid_p.  Otherwise wt = b, and if valid_p: cs = (n_p.x*n_q.x + n_p.y*n_q.y) + n_p.z*n_q.z;
 *   cs = cs > 0 ? cs : 0; normal_power_log2 times cs = cs*cs; wt = wt * cs; t = |z_p - z_q| / ((sigma_depth * |z_p|) * r + EPS),
 *   wt = wt / (1.0f + t*t); EPS = 2^-20.  With use_albedo and both sides hit, channel k of the tap's colour (and of its two half colours)
 *   is demodulated by guide_low[q].base_color[k] as rr_denoise_records demodulates: c_k / a_k when 2^-10 < a_k <= FLT_MAX, else as it is.
 *   sum_c[k] += wt * c_k, sum_w += wt, the halves' sums likewise with the same wt; all sums start at 0.
 *   Result.  If 0 < sum_w <= FLT_MAX: colour = sum_c / sum_w, with use_albedo and guide[p].hit remodulated by guide[p].base_color[k]
 *   (* a_k under the same condition); weight = sum_w.  Otherwise the FALLBACK: the same four taps again, a tap skipped only when q is
 *   outside the frame or !fin_q, weight b, no albedo; colour = sum_c / sum_b when 0 < sum_b <= FLT_MAX, else three zeros; weight = 0.
 *   The halves follow the colour in both cases.  A half colour that is not finite at a taken tap propagates into the half's sum; as for
 *   rr_denoise_records, a NaN the arithmetic generates there (0 * inf, a sum of two NaNs) has unspecified sign and payload.
 *   Guide fields of out[p], and of both halves_out records: for a hit, distance, normal and object_id of guide[p] -- a frame's record
 *   holds an item's id as it is, so these are the id bits of a pixel all of whose rays hit that item; for a miss the bits
 *   rr_render_pixels writes for a pixel all of whose rays missed: depth +0, every normal float the NaN 0xffc00000, object_id 0.
 *   rgba8_out (or NULL): the bytes rr_render_pixels writes for the record out[p], with params->gamma_correction as rr_config's.
 *   weight_out (or NULL): the weight above, W * H floats; 0 marks the pixels the guide found no tap for (a hole: a surface the low
 *   frame did not see), which a caller may trace at full resolution.
 * rr_upsample_params: struct_size = sizeof(rr_upsample_params); normal_power_log2 0 .. 7; sigma_depth finite and above 0.
 * rr_upsample_default_params writes power 5, sigma_depth 0.05, use_albedo 1, no gamma; it never touches a device.
 * rr_upsample_records_device follows rr_denoise_records_device: the scene handle serves for its device, its lock and its staging pool;
 * every pointer is classified before any launch (RR_ERR_INVALID_ARGUMENT naming the argument); work is enqueued on `hip_stream` in stream
 * order (the inputs may have been produced on that stream without a synchronisation) and the call does not wait inside;
 * RR_ERR_INVALID_ARGUMENT from on_pass of the same scene; nothing of a frame's state or statistics is touched; a scene edit or
 * rr_scene_destroy waits for a call in flight.  The call is one launch and keeps no device memory.
 *   Refusals, in this order: a NULL scene, params, low, guide_low, guide or out; width or height 0 or above 65535, low_width or
 *   low_height 0 or above the frame's; a struct_size other than sizeof(rr_upsample_params), a power out of range, a sigma_depth that is
 *   NaN, infinite or <= 0; halves_out without halves_low or the reverse; (device form) low, halves_low, guide_low, guide, out or
 *   halves_out not 16-byte aligned, rgba8_out or weight_out not 4-byte aligned; any overlap between an output and an input or between
 *   two outputs (nothing is in place): all RR_ERR_INVALID_ARGUMENT.  Then width * height * 2 > 2^30: RR_ERR_UNSUPPORTED.
 * rr_upsample_records: the same on HOST pointers, the device form on the null stream behind a staging copy in the pool of staging
 * buffers the record calls share (32, 64 and 128 B per low pixel, 128 + 32 and 64, 4 and 4 B per pixel, each only where given); it
 * returns with the outputs written.
 * rr_upsample_albedo_records(_device): rr_upsample_records(_device) with ALBEDO PLANES OF THE CALLER'S OWN, two more inputs after guide:
 * albedo_low (w * h * 3 floats, or NULL) and albedo (W * H * 3 floats, or NULL), pixel q at [3q .. 3q + 2], the layout rr_albedo_pixels
 * writes and rr_denoise_records reads.  A low frame's colour is a mean over its pixel's sub-samples, while guide_low[q].base_color is the
 * albedo under the pixel's centre: on a textured surface the quotient of the two is wrong, and rr_albedo_pixels on the low camera -- the
 * mean over exactly the rays that made the colour -- is the albedo to divide by.
 *   Wherever the text above reads guide_low[q].base_color[k], the call reads albedo_low[3q + k] when albedo_low is given; wherever it
 *   reads guide[p].base_color[k], the call reads albedo[3p + k] when albedo is given.  Nothing else changes: taps, skip rule, weights,
 *   fallback, halves, the guide fields of out, weight_out, rgba8_out.  With use_albedo == 0 the planes are not read.  The value of a
 *   plane at a pixel whose guide is not a hit reaches no result (it may be anything, a NaN included).
 *   So with both planes NULL the call IS rr_upsample_records, bit for bit; with planes it is rr_upsample_records on copies of the guides
 *   whose base_color[0 .. 2] were overwritten by the planes, bit for bit.  rr_upsample_records(_device) are this call with two NULLs.
 *   Refusals: those of rr_upsample_records in the same order -- the planes are optional, so no NULL is added; (device form) albedo_low
 *   or albedo not 4-byte aligned (a plane need NOT be 16-byte aligned), refused where rgba8_out and weight_out are; a plane that
 *   overlaps out, halves_out, rgba8_out or weight_out (the planes are inputs of 12 B per pixel: they may overlap each other and any other
 *   input).  The host form stages them with the rest (12 B per low pixel and per pixel more). */
typedef struct rr_upsample_params {
    uint32_t struct_size;        /* sizeof(rr_upsample_params) */
    uint32_t normal_power_log2;  /* 0 .. 7: the normal weight is max(0, n_p . n_q) squared this many times */
    float    sigma_depth;        /* > 0, finite */
    uint32_t use_albedo;         /* non-zero: the sum runs on albedo-demodulated colour */
    uint32_t gamma_correction;   /* rgba8_out only, as rr_config's */
} rr_upsample_params;
int rr_upsample_default_params(rr_upsample_params* out);
int rr_upsample_records_device(rr_scene* scene, uint32_t low_width, uint32_t low_height, uint32_t width, uint32_t height, const rr_upsample_params* params,
                               const rr_radiance* low_dev /* low_width * low_height */, const rr_radiance* halves_low_dev /* twice as many, or NULL */,
                               const rr_surface_hit* guide_low_dev /* low_width * low_height */, const rr_surface_hit* guide_dev /* width * height */,
                               rr_radiance* out_dev /* width * height */, rr_radiance* halves_out_dev /* width * height * 2; NULL exactly when halves_low_dev is */,
                               uint8_t* rgba8_out_dev /* or NULL */, float* weight_out_dev /* width * height, or NULL */, void* hip_stream);
int rr_upsample_records(rr_scene* scene, uint32_t low_width, uint32_t low_height, uint32_t width, uint32_t height, const rr_upsample_params* params,
                        const rr_radiance* low /* low_width * low_height */, const rr_radiance* halves_low /* twice as many, or NULL */,
                        const rr_surface_hit* guide_low /* low_width * low_height */, const rr_surface_hit* guide /* width * height */,
                        rr_radiance* out /* width * height */, rr_radiance* halves_out /* width * height * 2; NULL exactly when halves_low is */,
                        uint8_t* rgba8_out /* or NULL */, float* weight_out /* width * height, or NULL */);
int rr_upsample_albedo_records_device(rr_scene* scene, uint32_t low_width, uint32_t low_height, uint32_t width, uint32_t height, const rr_upsample_params* params,
                                      const rr_radiance* low_dev /* low_width * low_height */, const rr_radiance* halves_low_dev /* twice as many, or NULL */,
                                      const rr_surface_hit* guide_low_dev /* low_width * low_height */, const rr_surface_hit* guide_dev /* width * height */,
                                      const float* albedo_low_dev /* low_width * low_height * 3, or NULL */, const float* albedo_dev /* width * height * 3, or NULL */,
                                      rr_radiance* out_dev /* width * height */, rr_radiance* halves_out_dev /* width * height * 2; NULL exactly when halves_low_dev is */,
                                      uint8_t* rgba8_out_dev /* or NULL */, float* weight_out_dev /* width * height, or NULL */, void* hip_stream);
int rr_upsample_albedo_records(rr_scene* scene, uint32_t low_width, uint32_t low_height, uint32_t width, uint32_t height, const rr_upsample_params* params,
                               const rr_radiance* low /* low_width * low_height */, const rr_radiance* halves_low /* twice as many, or NULL */,
                               const rr_surface_hit* guide_low /* low_width * low_height */, const rr_surface_hit* guide /* width * height */,
                               const float* albedo_low /* low_width * low_height * 3, or NULL */, const float* albedo /* width * height * 3, or NULL */,
                               rr_radiance* out /* width * height */, rr_radiance* halves_out /* width * height * 2; NULL exactly when halves_low is */,
                               uint8_t* rgba8_out /* or NULL */, float* weight_out /* width * height, or NULL */);

/* Post-processing of a finished frame (reference run_post_processing, src/post_processing.rs:123-181, called from
 * Run::post_processing, src/run.rs:588-600): outline on object-id edges (:98-121), then cavity = curvature of the
 * normal buffer (:77-96), clamp, truncate to u8.  Consumes exactly the buffers rr_render produces.
 * rr_post_process: host buffers; rr_post_process_device: device buffers on `device`, enqueued on `hip_stream`.
 * rgba_in and rgba_out may not alias (the reference writes a new image). */
int rr_post_process(uint32_t width, uint32_t height, int cavity, int outline, const uint8_t* rgba_in,
                    const float* normal, const uint32_t* object_id, uint8_t* rgba_out, int device);
int rr_post_process_device(uint32_t width, uint32_t height, int cavity, int outline, const uint8_t* rgba_in,
                           const float* normal, const uint32_t* object_id, uint8_t* rgba_out, int device,
                           void* hip_stream);

/* Counters and device timings of the most recent frame on this scene. */
int rr_scene_last_stats(const rr_scene* scene, rr_frame_stats* out);

/* *out = the number of level-1 stages of the most recent frame on this scene whose shade and shadow launches went to two
 * streams (summed over the frame's batches); 0 = the frame took the serial schedule.  The frame's bits are the same either way. */
int rr_scene_overlap_stages(const rr_scene* scene, uint32_t* out);

#ifdef __cplusplus
}
#endif
#endif /* RUSTRAY_HIP_H */
