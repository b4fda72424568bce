// host_shim.cpp — C entry points over include/rustray_host.hpp so that the C++ host layer (Camera, RaytracingConfig,
// Raytracing, RendererManager) can be driven from the Python tests through ctypes.  Test plumbing, not part of the ABI.
#include "../../include/rustray_host.hpp"

#include <chrono>
#include <thread>

using namespace rustray;

static Camera make_camera(float fov, const float* eye, const float* up, const float* dir, float cnear, float cfar) {
    Camera c;
    c.fov = fov;
    c.eye_pos = Vec3{eye[0], eye[1], eye[2]}; c.up = Vec3{up[0], up[1], up[2]}; c.dir = Vec3{dir[0], dir[1], dir[2]};
    c.clipping_near = cnear; c.clipping_far = cfar;
    return c;
}

extern "C" int rh_camera(float fov, const float* eye, const float* up, const float* dir, float cnear, float cfar, uint32_t w, uint32_t h,
                         float* proj_inv16, float* view_inv16, int* is_default, const float* point, int* point_in_frustum) {
    Camera c = make_camera(fov, eye, up, dir, cnear, cfar);
    c.init(w, h);
    const rr_camera rc = c.c_struct();
    for (int i = 0; i < 16; i++) { proj_inv16[i] = rc.projection_inverse[i]; view_inv16[i] = rc.view_inverse[i]; }
    *is_default = c.is_default_cam() ? 1 : 0;
    if (point && point_in_frustum) *point_in_frustum = c.is_point_in_frustum(Vec3{point[0], point[1], point[2]}) ? 1 : 0;
    return 0;
}

extern "C" int rh_camera_world_to_clip(float fov, const float* eye, const float* up, const float* dir, float cnear, float cfar, uint32_t w, uint32_t h,
                                       float* world_to_clip16, float* eye3) {
    Camera c = make_camera(fov, eye, up, dir, cnear, cfar);
    c.init(w, h);
    c.world_to_clip(world_to_clip16, eye3);
    return 0;
}

static RaytracingConfig from_c(const rr_config* c) {
    RaytracingConfig r;
    r.monte_carlo = c->monte_carlo != 0; r.samples = c->samples; r.focal_length = c->focal_length; r.aperture_size = c->aperture_size;
    r.fog_density = c->fog_density; r.fog_color = Vec3{c->fog_color[0], c->fog_color[1], c->fog_color[2]};
    r.max_recursion = c->max_recursion; r.gamma_correction = c->gamma_correction != 0; r.seed = c->seed;
    return r;
}

// base.apply(n) -> out
extern "C" void rh_config_apply(const rr_config* base, const rr_config* n, rr_config* out) {
    RaytracingConfig b = from_c(base);
    b.apply(from_c(n));
    *out = b.c_struct();
}

// One frame through RendererManager::start / is_done / stop.  stats: [passes, rendered pixels, is_done, drained pixels,
// elapsed ms, was running right after start].  stop_after_passes > 0 calls stop() once that many passes were seen.
extern "C" int rh_render(const rr_flat_scene* fs, int device, float fov, const float* eye, const float* up, const float* dir, float cnear, float cfar,
                         const rr_config* cfg, uint32_t w, uint32_t h, uint32_t min_passes, int stop_after_passes,
                         uint8_t* rgba, float* normal, float* depth, uint32_t* ids, uint64_t* stats, int pick_x, int pick_y, float* pick_out) {
    auto scene = std::make_shared<DeviceScene>(*fs, device);
    if (!scene->ok()) return -1;
    auto rt = std::make_shared<Raytracing>(scene);
    rt->camera = make_camera(fov, eye, up, dir, cnear, cfar);
    rt->config.apply(from_c(cfg));
    rt->config.seed = cfg->seed;
    RendererManager mgr((int32_t)w, (int32_t)h, rt);
    mgr.min_passes = min_passes;
    mgr.start();
    stats[5] = mgr.is_running() ? 1 : 0;
    uint64_t drained = 0;
    while (mgr.is_running()) {
        drained += mgr.drain([](const PixelData&) {});
        if (stop_after_passes > 0 && mgr.passes() >= (uint32_t)stop_after_passes) mgr.stop();
        std::this_thread::sleep_for(std::chrono::microseconds(200));
    }
    mgr.wait();
    std::vector<uint8_t> im; std::vector<float> nr, dp; std::vector<uint32_t> id;
    uint64_t last = 0;
    last = mgr.drain([&](const PixelData& p) { (void)p; });
    drained += last;
    mgr.frame(&im, &nr, &dp, &id);
    std::memcpy(rgba, im.data(), im.size());
    std::memcpy(normal, nr.data(), nr.size() * 4);
    std::memcpy(depth, dp.data(), dp.size() * 4);
    std::memcpy(ids, id.data(), id.size() * 4);
    stats[0] = mgr.passes(); stats[1] = mgr.get_rendered_pixels(); stats[2] = mgr.is_done() ? 1 : 0; stats[3] = drained;
    stats[4] = mgr.check_and_get_elapsed_time();
    if (stop_after_passes == -1) { // the caller wants the post-processed image (cavity + outline)
        const std::vector<uint8_t> pp = mgr.post_processing(true, true, device);
        std::memcpy(rgba, pp.data(), pp.size());
    }
    if (pick_out) {
        auto p = rt->pick(pick_x, pick_y);
        pick_out[0] = p ? 1.0f : 0.0f; pick_out[1] = p ? (float)p->first : 0.0f; pick_out[2] = p ? p->second : 0.0f;
    }
    return mgr.failed() ? -2 : 0;
}

// Animation::frame_transforms for a two-keyframe animation of ONE named object among `n_items` items
// (names "item0", "item1", ...; the animated one is `animated`): tests the keyframe selection, the interpolation and
// the transformation order against the Python mirror.
extern "C" int rh_animation_frame(uint32_t fps, uint64_t t1_ms, const float* tr0, const float* rot0, const float* sc0,
                                  const float* tr1, const float* rot1, const float* sc1, uint32_t n_items, uint32_t animated,
                                  uint64_t frame, float* trans, float* trans_inv, uint64_t* frames_amount, int* exists) {
    Animation an;
    an.enabled = true; an.fps = fps;
    const std::string name = "item" + std::to_string(animated);
    Keyframe k0; k0.time = 0;
    k0.objects.push_back(Frame{name, Vec3{tr0[0], tr0[1], tr0[2]}, Vec3{rot0[0], rot0[1], rot0[2]}, Vec3{sc0[0], sc0[1], sc0[2]}});
    Keyframe k1; k1.time = t1_ms;
    k1.objects.push_back(Frame{name, Vec3{tr1[0], tr1[1], tr1[2]}, Vec3{rot1[0], rot1[1], rot1[2]}, Vec3{sc1[0], sc1[1], sc1[2]}});
    an.keyframes = {k0, k1};
    std::vector<std::string> names;
    for (uint32_t i = 0; i < n_items; i++) names.push_back("item" + std::to_string(i));
    *frames_amount = an.get_frames_amount_to_render();
    *exists = an.frame_exists(frame) ? 1 : 0;
    return an.frame_transforms(names, frame, trans, trans_inv) ? 1 : 0;
}

// A resident scene behind Raytracing for the edit tests: rh_scene_create, the edits through Raytracing / DeviceScene, one frame
// through RendererManager (rh_scene_render), rh_scene_destroy.
struct RhScene { std::shared_ptr<DeviceScene> scene; std::shared_ptr<Raytracing> rt; };

extern "C" void* rh_scene_create(const rr_flat_scene* fs, int device) {
    auto* h = new RhScene;
    h->scene = std::make_shared<DeviceScene>(*fs, device);
    if (!h->scene->ok()) { delete h; return nullptr; }
    h->rt = std::make_shared<Raytracing>(h->scene);
    return h;
}

extern "C" void rh_scene_destroy(void* h) { delete (RhScene*)h; }

extern "C" int rh_update_lights(void* h, const rr_light* lights, uint32_t n) {
    return ((RhScene*)h)->rt->update_lights(std::vector<rr_light>(lights, lights + n)) ? 0 : -1;
}

extern "C" int rh_update_item_flags(void* h, const uint8_t* visible, const uint8_t* flip_normals, uint32_t n) {
    return ((RhScene*)h)->rt->update_item_flags(std::vector<uint8_t>(visible, visible + n), std::vector<uint8_t>(flip_normals, flip_normals + n)) ? 0 : -1;
}

extern "C" int rh_add_textures(void* h, const rr_texture* textures, uint32_t n, uint32_t* first_index) {
    return ((RhScene*)h)->scene->add_textures(std::vector<rr_texture>(textures, textures + n), first_index);
}

extern "C" int rh_add_meshes(void* h, const rr_mesh* meshes, uint32_t n, uint32_t* first_index) {
    return ((RhScene*)h)->scene->add_meshes(std::vector<rr_mesh>(meshes, meshes + n), first_index);
}

extern "C" int rh_set_items(void* h, const rr_item* items, uint32_t n_items, const rr_material* materials, uint32_t n_materials) {
    return ((RhScene*)h)->scene->set_items(std::vector<rr_item>(items, items + n_items), std::vector<rr_material>(materials, materials + n_materials));
}

// Raytracing::trace_shadow for n rays, one call each: out[4 i ..] = (occluded, item index, face id, toi bits); max_distance NULL = the default (no limit)
extern "C" int rh_trace_shadow(void* h, const float* origins, const float* dirs, const float* max_distance, uint32_t n, uint32_t depth, uint32_t* out) {
    const Raytracing& rt = *((RhScene*)h)->rt;
    for (uint32_t i = 0; i < n; i++) {
        const Vec3 o{origins[3 * i], origins[3 * i + 1], origins[3 * i + 2]}, d{dirs[3 * i], dirs[3 * i + 1], dirs[3 * i + 2]};
        const auto r = max_distance ? rt.trace_shadow(o, d, depth, max_distance[i]) : rt.trace_shadow(o, d, depth);
        out[4 * i] = r ? 1u : 0u; out[4 * i + 1] = r ? r->item_index : 0xffffffffu; out[4 * i + 2] = r ? r->face_id : 0u; out[4 * i + 3] = 0u;
        if (r) std::memcpy(&out[4 * i + 3], &r->toi, 4);
    }
    return 0;
}

// Raytracing::shade_rays over n_rays rays with the given config: out = n_rays / rays_per_result records of 8 words (rr_radiance)
extern "C" int rh_shade_rays(void* h, const rr_config* cfg, const float* origins, const float* dirs, uint32_t n_rays, uint32_t rays_per_result,
                             const uint32_t* stream_ids, rr_radiance* out) {
    Raytracing& rt = *((RhScene*)h)->rt;
    rt.config = RaytracingConfig();
    rt.config.apply(from_c(cfg));
    rt.config.seed = cfg->seed;
    std::vector<Raytracing::Ray> rays(n_rays);
    for (uint32_t i = 0; i < n_rays; i++)
        rays[i] = Raytracing::Ray{Vec3{origins[3 * i], origins[3 * i + 1], origins[3 * i + 2]}, Vec3{dirs[3 * i], dirs[3 * i + 1], dirs[3 * i + 2]}};
    const std::vector<rr_radiance> r = rt.shade_rays(rays.data(), rays.size(), rays_per_result, stream_ids);
    if (r.empty()) return -1;
    std::memcpy(out, r.data(), r.size() * sizeof(rr_radiance));
    return 0;
}

// Raytracing::trace_device / trace_shadow_device / shade_device: the device-buffer ray queries, enqueued on `stream` (a hipStream_t)
extern "C" int rh_trace_device(void* h, const float* origins_dev, const float* dirs_dev, uint32_t n, uint32_t depth, rr_ray_hit* out_dev, void* stream) {
    return ((RhScene*)h)->rt->trace_device(origins_dev, dirs_dev, n, depth, out_dev, stream);
}

extern "C" int rh_trace_shadow_device(void* h, const float* origins_dev, const float* dirs_dev, const float* max_distance_dev, uint32_t n, uint32_t depth,
                                      rr_shadow_hit* out_dev, void* stream) {
    return ((RhScene*)h)->rt->trace_shadow_device(origins_dev, dirs_dev, max_distance_dev, n, depth, out_dev, stream);
}

extern "C" int rh_shade_device(void* h, const rr_config* cfg, const float* origins_dev, const float* dirs_dev, uint32_t n_results, uint32_t rays_per_result,
                               const uint32_t* stream_ids_dev, rr_radiance* out_dev, void* stream) {
    Raytracing& rt = *((RhScene*)h)->rt;
    rt.config = RaytracingConfig();
    rt.config.apply(from_c(cfg));
    rt.config.seed = cfg->seed;
    return rt.shade_device(origins_dev, dirs_dev, n_results, rays_per_result, stream_ids_dev, out_dev, stream);
}

// Raytracing::render_pixels with the given camera (of a w x h frame) and config: xy NULL = the whole frame (n = w * h); out = n records of 8
// words (rr_radiance), rgba8 (or NULL) = n x 4 bytes.  rh_render_pixel: Raytracing::render(x, y), out6 = (r, g, b, object id, x, y), nd4 =
// (normal, depth).  rh_render_pixels_device: Raytracing::render_pixels_device on device buffers.
static Raytracing& rh_with(void* h, float fov, const float* eye, const float* up, const float* dir, float cnear, float cfar, const rr_config* cfg,
                           uint32_t w, uint32_t hgt) {
    Raytracing& rt = *((RhScene*)h)->rt;
    rt.camera = make_camera(fov, eye, up, dir, cnear, cfar);
    rt.camera.init(w, hgt);
    rt.config = RaytracingConfig();
    rt.config.apply(from_c(cfg));
    rt.config.seed = cfg->seed;
    return rt;
}
extern "C" int rh_render_pixels(void* h, float fov, const float* eye, const float* up, const float* dir, float cnear, float cfar, const rr_config* cfg,
                                uint32_t w, uint32_t hgt, const uint32_t* xy, uint32_t n, rr_radiance* out, uint8_t* rgba8) {
    const Raytracing& rt = rh_with(h, fov, eye, up, dir, cnear, cfar, cfg, w, hgt);
    std::vector<uint8_t> bytes;
    const std::vector<rr_radiance> r = rt.render_pixels(xy, n, rgba8 ? &bytes : nullptr);
    if (r.empty()) return -1;
    std::memcpy(out, r.data(), r.size() * sizeof(rr_radiance));
    if (rgba8) std::memcpy(rgba8, bytes.data(), bytes.size());
    return (int)r.size();
}
extern "C" int rh_render_pixel(void* h, float fov, const float* eye, const float* up, const float* dir, float cnear, float cfar, const rr_config* cfg,
                               uint32_t w, uint32_t hgt, int x, int y, int32_t* out6, float* nd4) {
    const Raytracing& rt = rh_with(h, fov, eye, up, dir, cnear, cfar, cfg, w, hgt);
    const PixelData p = rt.render(x, y);
    out6[0] = p.r; out6[1] = p.g; out6[2] = p.b; out6[3] = (int32_t)p.object_id; out6[4] = p.x; out6[5] = p.y;
    nd4[0] = p.normal.x; nd4[1] = p.normal.y; nd4[2] = p.normal.z; nd4[3] = p.depth;
    return p.x < 0 ? -1 : 0;
}
extern "C" int rh_render_pixels_device(void* h, float fov, const float* eye, const float* up, const float* dir, float cnear, float cfar, const rr_config* cfg,
                                       uint32_t w, uint32_t hgt, const uint32_t* xy_dev, uint32_t n, rr_radiance* out_dev, uint8_t* rgba8_dev, void* stream,
                                       const int* cancel) {
    return rh_with(h, fov, eye, up, dir, cnear, cfar, cfg, w, hgt).render_pixels_device(xy_dev, n, out_dev, rgba8_dev, stream, cancel);
}
// Raytracing::render_pixel_parts: as rh_render_pixels, with parts = n * n_parts records; returns n, or -1 when the call was refused.
// rh_render_pixel_parts_device: Raytracing::render_pixel_parts_device on device buffers, the rr_status as it is.
extern "C" int rh_render_pixel_parts(void* h, float fov, const float* eye, const float* up, const float* dir, float cnear, float cfar, const rr_config* cfg,
                                     uint32_t w, uint32_t hgt, const uint32_t* xy, uint32_t n, uint32_t n_parts, rr_radiance* out, rr_radiance* parts) {
    const Raytracing& rt = rh_with(h, fov, eye, up, dir, cnear, cfar, cfg, w, hgt);
    std::vector<rr_radiance> p;
    const std::vector<rr_radiance> r = rt.render_pixel_parts(xy, n, n_parts, &p);
    if (r.empty() || p.size() != r.size() * n_parts) return -1;
    std::memcpy(out, r.data(), r.size() * sizeof(rr_radiance));
    std::memcpy(parts, p.data(), p.size() * sizeof(rr_radiance));
    return (int)r.size();
}
extern "C" int rh_render_pixel_parts_device(void* h, float fov, const float* eye, const float* up, const float* dir, float cnear, float cfar, const rr_config* cfg,
                                            uint32_t w, uint32_t hgt, const uint32_t* xy_dev, uint32_t n, uint32_t n_parts, rr_radiance* out_dev,
                                            rr_radiance* parts_dev, void* stream, const int* cancel) {
    return rh_with(h, fov, eye, up, dir, cnear, cfar, cfg, w, hgt).render_pixel_parts_device(xy_dev, n, n_parts, out_dev, parts_dev, stream, cancel);
}
// Raytracing::render_adaptive: out = w * h records, samples = w * h uint16, error = w * h floats, rgba8 = w * h x 4 bytes (each of the three
// or NULL); returns the number of refined pixels, or -1 when the call was refused.  rh_render_adaptive_device: Raytracing::render_adaptive_device
// on device buffers, the rr_status as it is.
extern "C" int rh_render_adaptive(void* h, float fov, const float* eye, const float* up, const float* dir, float cnear, float cfar, const rr_config* cfg,
                                  uint32_t w, uint32_t hgt, uint16_t base_samples, uint16_t max_samples, float threshold, rr_radiance* out, uint16_t* samples,
                                  float* error, uint8_t* rgba8) {
    const Raytracing& rt = rh_with(h, fov, eye, up, dir, cnear, cfar, cfg, w, hgt);
    std::vector<uint16_t> sm; std::vector<float> er; std::vector<uint8_t> bytes;
    uint32_t n_refined = 0;
    const std::vector<rr_radiance> r = rt.render_adaptive(base_samples, max_samples, threshold, samples ? &sm : nullptr, error ? &er : nullptr, rgba8 ? &bytes : nullptr, &n_refined);
    if (r.empty()) return -1;
    std::memcpy(out, r.data(), r.size() * sizeof(rr_radiance));
    if (samples) std::memcpy(samples, sm.data(), sm.size() * 2);
    if (error) std::memcpy(error, er.data(), er.size() * 4);
    if (rgba8) std::memcpy(rgba8, bytes.data(), bytes.size());
    return (int)n_refined;
}
extern "C" int rh_render_adaptive_device(void* h, float fov, const float* eye, const float* up, const float* dir, float cnear, float cfar, const rr_config* cfg,
                                         uint32_t w, uint32_t hgt, uint16_t base_samples, uint16_t max_samples, float threshold, rr_radiance* out_dev, uint8_t* rgba8_dev,
                                         uint16_t* samples_dev, float* error_dev, uint32_t* n_refined, void* stream, const int* cancel) {
    return rh_with(h, fov, eye, up, dir, cnear, cfar, cfg, w, hgt).render_adaptive_device(base_samples, max_samples, threshold, out_dev, rgba8_dev, samples_dev, error_dev,
                                                                                          n_refined, stream, cancel);
}
// Raytracing::render_adaptive_levels: as rh_render_adaptive, with n_levels counts and level_pixels = n_levels words (or NULL); returns 0, or -1
// when the call was refused.  rh_render_adaptive_levels_device: Raytracing::render_adaptive_levels_device on device buffers, the rr_status as it is.
extern "C" int rh_render_adaptive_levels(void* h, float fov, const float* eye, const float* up, const float* dir, float cnear, float cfar, const rr_config* cfg,
                                         uint32_t w, uint32_t hgt, const uint16_t* levels, uint32_t n_levels, float threshold, rr_radiance* out, uint16_t* samples,
                                         float* error, uint8_t* rgba8, uint32_t* level_pixels) {
    const Raytracing& rt = rh_with(h, fov, eye, up, dir, cnear, cfar, cfg, w, hgt);
    std::vector<uint16_t> sm; std::vector<float> er; std::vector<uint8_t> bytes; std::vector<uint32_t> lp;
    const std::vector<rr_radiance> r = rt.render_adaptive_levels(std::vector<uint16_t>(levels, levels + n_levels), threshold, samples ? &sm : nullptr, error ? &er : nullptr,
                                                                 rgba8 ? &bytes : nullptr, &lp);
    if (r.empty()) return -1;
    std::memcpy(out, r.data(), r.size() * sizeof(rr_radiance));
    if (samples) std::memcpy(samples, sm.data(), sm.size() * 2);
    if (error) std::memcpy(error, er.data(), er.size() * 4);
    if (rgba8) std::memcpy(rgba8, bytes.data(), bytes.size());
    if (level_pixels) std::memcpy(level_pixels, lp.data(), lp.size() * 4);
    return 0;
}
extern "C" int rh_render_adaptive_levels_device(void* h, float fov, const float* eye, const float* up, const float* dir, float cnear, float cfar, const rr_config* cfg,
                                                uint32_t w, uint32_t hgt, const uint16_t* levels, uint32_t n_levels, float threshold, rr_radiance* out_dev,
                                                uint8_t* rgba8_dev, uint16_t* samples_dev, float* error_dev, uint32_t* level_pixels, void* stream, const int* cancel) {
    return rh_with(h, fov, eye, up, dir, cnear, cfar, cfg, w, hgt).render_adaptive_levels_device(levels, n_levels, threshold, out_dev, rgba8_dev, samples_dev, error_dev,
                                                                                                 level_pixels, stream, cancel);
}
// Raytracing::render_pixel_prefix: as rh_render_pixels, with halves = n * 2 records (or NULL); returns n, or -1 when the call was refused.
// rh_render_adaptive_prefix and its device form: as rh_render_adaptive_levels, on the prefixes of the frame of cfg->samples samples.
extern "C" int rh_render_pixel_prefix(void* h, float fov, const float* eye, const float* up, const float* dir, float cnear, float cfar, const rr_config* cfg,
                                      uint32_t w, uint32_t hgt, const uint32_t* xy, uint32_t n, uint32_t samples_used, rr_radiance* out, rr_radiance* halves, uint8_t* rgba8) {
    const Raytracing& rt = rh_with(h, fov, eye, up, dir, cnear, cfar, cfg, w, hgt);
    std::vector<rr_radiance> p; std::vector<uint8_t> bytes;
    const std::vector<rr_radiance> r = rt.render_pixel_prefix(xy, n, samples_used, halves ? &p : nullptr, rgba8 ? &bytes : nullptr);
    if (r.empty()) return -1;
    std::memcpy(out, r.data(), r.size() * sizeof(rr_radiance));
    if (halves) std::memcpy(halves, p.data(), p.size() * sizeof(rr_radiance));
    if (rgba8) std::memcpy(rgba8, bytes.data(), bytes.size());
    return (int)r.size();
}
extern "C" int rh_render_adaptive_prefix(void* h, float fov, const float* eye, const float* up, const float* dir, float cnear, float cfar, const rr_config* cfg,
                                         uint32_t w, uint32_t hgt, const uint16_t* prefixes, uint32_t n_levels, float threshold, rr_radiance* out, uint16_t* samples,
                                         float* error, uint8_t* rgba8, uint32_t* level_pixels) {
    const Raytracing& rt = rh_with(h, fov, eye, up, dir, cnear, cfar, cfg, w, hgt);
    std::vector<uint16_t> sm; std::vector<float> er; std::vector<uint8_t> bytes; std::vector<uint32_t> lp;
    const std::vector<rr_radiance> r = rt.render_adaptive_prefix(std::vector<uint16_t>(prefixes, prefixes + n_levels), threshold, samples ? &sm : nullptr, error ? &er : nullptr,
                                                                 rgba8 ? &bytes : nullptr, &lp);
    if (r.empty()) return -1;
    std::memcpy(out, r.data(), r.size() * sizeof(rr_radiance));
    if (samples) std::memcpy(samples, sm.data(), sm.size() * 2);
    if (error) std::memcpy(error, er.data(), er.size() * 4);
    if (rgba8) std::memcpy(rgba8, bytes.data(), bytes.size());
    if (level_pixels) std::memcpy(level_pixels, lp.data(), lp.size() * 4);
    return 0;
}
extern "C" int rh_render_adaptive_prefix_device(void* h, float fov, const float* eye, const float* up, const float* dir, float cnear, float cfar, const rr_config* cfg,
                                                uint32_t w, uint32_t hgt, const uint16_t* prefixes, uint32_t n_levels, float threshold, rr_radiance* out_dev,
                                                uint8_t* rgba8_dev, uint16_t* samples_dev, float* error_dev, uint32_t* level_pixels, void* stream, const int* cancel) {
    return rh_with(h, fov, eye, up, dir, cnear, cfar, cfg, w, hgt).render_adaptive_prefix_device(prefixes, n_levels, threshold, out_dev, rgba8_dev, samples_dev, error_dev,
                                                                                                 level_pixels, stream, cancel);
}
// Raytracing::denoise: records = w * h, halves = w * h * 2 or NULL, albedo = w * h * 3 or NULL, params or NULL for the defaults; out = w * h
// records, variance = w * h floats or NULL, rgba8 = w * h x 4 bytes or NULL; returns 0, or -1 when the call was refused.
// rh_render_denoised: Raytracing::render_denoised; noisy = w * h records or NULL.
extern "C" int rh_denoise(void* h, float fov, const float* eye, const float* up, const float* dir, float cnear, float cfar, const rr_config* cfg,
                          uint32_t w, uint32_t hgt, const rr_radiance* records, const rr_radiance* halves, const float* albedo, const rr_denoise_params* params,
                          rr_radiance* out, float* variance, uint8_t* rgba8) {
    const Raytracing& rt = rh_with(h, fov, eye, up, dir, cnear, cfar, cfg, w, hgt);
    std::vector<float> var; std::vector<uint8_t> bytes;
    const std::vector<rr_radiance> r = rt.denoise(records, halves, albedo, params, variance ? &var : nullptr, rgba8 ? &bytes : nullptr);
    if (r.empty()) return -1;
    std::memcpy(out, r.data(), r.size() * sizeof(rr_radiance));
    if (variance) std::memcpy(variance, var.data(), var.size() * 4);
    if (rgba8) std::memcpy(rgba8, bytes.data(), bytes.size());
    return 0;
}
extern "C" int rh_render_denoised(void* h, float fov, const float* eye, const float* up, const float* dir, float cnear, float cfar, const rr_config* cfg,
                                  uint32_t w, uint32_t hgt, const rr_denoise_params* params, rr_radiance* out, uint8_t* rgba8, rr_radiance* noisy) {
    const Raytracing& rt = rh_with(h, fov, eye, up, dir, cnear, cfar, cfg, w, hgt);
    std::vector<uint8_t> bytes; std::vector<rr_radiance> raw;
    const std::vector<rr_radiance> r = rt.render_denoised(params, rgba8 ? &bytes : nullptr, noisy ? &raw : nullptr);
    if (r.empty()) return -1;
    std::memcpy(out, r.data(), r.size() * sizeof(rr_radiance));
    if (rgba8) std::memcpy(rgba8, bytes.data(), bytes.size());
    if (noisy) std::memcpy(noisy, raw.data(), raw.size() * sizeof(rr_radiance));
    return 0;
}
// Raytracing::upsample: low = lw * lh records, halves_low = twice as many or NULL, guide_low = lw * lh and guide = w * h surface records,
// params or NULL for the defaults; out = w * h records, halves_out = w * h * 2 or NULL (exactly when halves_low is), weight = w * h floats
// or NULL, rgba8 = w * h x 4 bytes or NULL; returns 0, or -1 when the call was refused.
// rh_render_upsampled: Raytracing::render_upsampled; out = w * h records, weight and rgba8 as above.
extern "C" int rh_upsample(void* h, float fov, const float* eye, const float* up, const float* dir, float cnear, float cfar, const rr_config* cfg,
                           uint32_t w, uint32_t hgt, uint32_t lw, uint32_t lh, const rr_radiance* low, const rr_radiance* halves_low, const rr_surface_hit* guide_low,
                           const rr_surface_hit* guide, const rr_upsample_params* params, rr_radiance* out, rr_radiance* halves_out, float* weight, uint8_t* rgba8) {
    const Raytracing& rt = rh_with(h, fov, eye, up, dir, cnear, cfar, cfg, w, hgt);
    std::vector<rr_radiance> hv; std::vector<float> wt; std::vector<uint8_t> bytes;
    const std::vector<rr_radiance> r = rt.upsample(lw, lh, low, halves_low, guide_low, guide, params, halves_out ? &hv : nullptr, weight ? &wt : nullptr, rgba8 ? &bytes : nullptr);
    if (r.empty()) return -1;
    std::memcpy(out, r.data(), r.size() * sizeof(rr_radiance));
    if (halves_out) std::memcpy(halves_out, hv.data(), hv.size() * sizeof(rr_radiance));
    if (weight) std::memcpy(weight, wt.data(), wt.size() * 4);
    if (rgba8) std::memcpy(rgba8, bytes.data(), bytes.size());
    return 0;
}
// rh_upsample_albedo: Raytracing::upsample with its albedo planes: albedo_low = lw * lh * 3 floats or NULL, albedo = w * h * 3 floats or NULL
extern "C" int rh_upsample_albedo(void* h, float fov, const float* eye, const float* up, const float* dir, float cnear, float cfar, const rr_config* cfg,
                                  uint32_t w, uint32_t hgt, uint32_t lw, uint32_t lh, const rr_radiance* low, const rr_radiance* halves_low, const rr_surface_hit* guide_low,
                                  const rr_surface_hit* guide, const float* albedo_low, const float* albedo, const rr_upsample_params* params, rr_radiance* out,
                                  rr_radiance* halves_out, float* weight, uint8_t* rgba8) {
    const Raytracing& rt = rh_with(h, fov, eye, up, dir, cnear, cfar, cfg, w, hgt);
    std::vector<rr_radiance> hv; std::vector<float> wt; std::vector<uint8_t> bytes;
    const std::vector<rr_radiance> r = rt.upsample(lw, lh, low, halves_low, guide_low, guide, params, halves_out ? &hv : nullptr, weight ? &wt : nullptr, rgba8 ? &bytes : nullptr,
                                                   albedo_low, albedo);
    if (r.empty()) return -1;
    std::memcpy(out, r.data(), r.size() * sizeof(rr_radiance));
    if (halves_out) std::memcpy(halves_out, hv.data(), hv.size() * sizeof(rr_radiance));
    if (weight) std::memcpy(weight, wt.data(), wt.size() * 4);
    if (rgba8) std::memcpy(rgba8, bytes.data(), bytes.size());
    return 0;
}
// rh_render_upsampled_albedo: Raytracing::render_upsampled with its albedo options: mean != 0 is AlbedoGuide::MEAN, full_albedo_samples 0 = none,
// low_denoise_params or NULL
extern "C" int rh_render_upsampled_albedo(void* h, float fov, const float* eye, const float* up, const float* dir, float cnear, float cfar, const rr_config* cfg,
                                          uint32_t w, uint32_t hgt, uint32_t scale, const rr_upsample_params* params, const rr_denoise_params* denoise_params, int mean,
                                          uint32_t full_albedo_samples, const rr_denoise_params* low_denoise_params, rr_radiance* out, float* weight, uint8_t* rgba8) {
    const Raytracing& rt = rh_with(h, fov, eye, up, dir, cnear, cfar, cfg, w, hgt);
    std::vector<float> wt; std::vector<uint8_t> bytes;
    const std::vector<rr_radiance> r = rt.render_upsampled(scale, params, denoise_params, rgba8 ? &bytes : nullptr, weight ? &wt : nullptr,
                                                           mean ? Raytracing::AlbedoGuide::MEAN : Raytracing::AlbedoGuide::CENTRE, full_albedo_samples, low_denoise_params);
    if (r.empty()) return -1;
    std::memcpy(out, r.data(), r.size() * sizeof(rr_radiance));
    if (weight) std::memcpy(weight, wt.data(), wt.size() * 4);
    if (rgba8) std::memcpy(rgba8, bytes.data(), bytes.size());
    return 0;
}
extern "C" int rh_render_upsampled(void* h, float fov, const float* eye, const float* up, const float* dir, float cnear, float cfar, const rr_config* cfg,
                                   uint32_t w, uint32_t hgt, uint32_t scale, const rr_upsample_params* params, const rr_denoise_params* denoise_params, rr_radiance* out,
                                   float* weight, uint8_t* rgba8) {
    const Raytracing& rt = rh_with(h, fov, eye, up, dir, cnear, cfar, cfg, w, hgt);
    std::vector<float> wt; std::vector<uint8_t> bytes;
    const std::vector<rr_radiance> r = rt.render_upsampled(scale, params, denoise_params, rgba8 ? &bytes : nullptr, weight ? &wt : nullptr);
    if (r.empty()) return -1;
    std::memcpy(out, r.data(), r.size() * sizeof(rr_radiance));
    if (weight) std::memcpy(weight, wt.data(), wt.size() * 4);
    if (rgba8) std::memcpy(rgba8, bytes.data(), bytes.size());
    return 0;
}
// rh_render_denoised_albedo: Raytracing::render_denoised with its albedo argument; albedo_out = w * h * 3 floats of Raytracing::albedo or NULL
extern "C" int rh_render_denoised_albedo(void* h, float fov, const float* eye, const float* up, const float* dir, float cnear, float cfar, const rr_config* cfg,
                                         uint32_t w, uint32_t hgt, const rr_denoise_params* params, int with_albedo, rr_radiance* out, rr_radiance* noisy, float* albedo_out) {
    const Raytracing& rt = rh_with(h, fov, eye, up, dir, cnear, cfar, cfg, w, hgt);
    std::vector<rr_radiance> raw;
    const std::vector<rr_radiance> r = rt.render_denoised(params, nullptr, noisy ? &raw : nullptr, with_albedo != 0);
    if (r.empty()) return -1;
    std::memcpy(out, r.data(), r.size() * sizeof(rr_radiance));
    if (noisy) std::memcpy(noisy, raw.data(), raw.size() * sizeof(rr_radiance));
    if (albedo_out) {
        const std::vector<float> a = rt.albedo();
        if (a.empty()) return -1;
        std::memcpy(albedo_out, a.data(), a.size() * 4);
    }
    return 0;
}
// Raytracing::surface_pixels: xy = n entries or NULL (the whole frame, n = w * h); out = n records, albedo_out = n * 3 floats or NULL;
// returns 0, or -1 when the call was refused.  rh_surface_pixels_device: Raytracing::surface_pixels_device; returns its rr_status.
extern "C" int rh_surface_pixels(void* h, float fov, const float* eye, const float* up, const float* dir, float cnear, float cfar, const rr_config* cfg,
                                 uint32_t w, uint32_t hgt, const uint32_t* xy, uint32_t n, rr_surface_hit* out, float* albedo_out) {
    const Raytracing& rt = rh_with(h, fov, eye, up, dir, cnear, cfar, cfg, w, hgt);
    std::vector<float> a;
    const std::vector<rr_surface_hit> r = rt.surface_pixels(xy, n, albedo_out ? &a : nullptr);
    if (r.empty()) return -1;
    std::memcpy(out, r.data(), r.size() * sizeof(rr_surface_hit));
    if (albedo_out) std::memcpy(albedo_out, a.data(), a.size() * 4);
    return 0;
}
extern "C" int rh_surface_pixels_device(void* h, float fov, const float* eye, const float* up, const float* dir, float cnear, float cfar, const rr_config* cfg,
                                        uint32_t w, uint32_t hgt, const uint32_t* xy_dev, uint32_t n, rr_surface_hit* out_dev, float* albedo_out_dev, void* stream) {
    return rh_with(h, fov, eye, up, dir, cnear, cfar, cfg, w, hgt).surface_pixels_device(xy_dev, n, out_dev, albedo_out_dev, stream);
}
// rh_render_denoised_mean_albedo: Raytracing::render_denoised(AlbedoGuide::MEAN); out = w * h records, noisy = the same or NULL,
// albedo_out = w * h * 3 floats of Raytracing::mean_albedo or NULL; returns 0, or -1 when a call was refused.
extern "C" int rh_render_denoised_mean_albedo(void* h, float fov, const float* eye, const float* up, const float* dir, float cnear, float cfar, const rr_config* cfg,
                                              uint32_t w, uint32_t hgt, const rr_denoise_params* params, rr_radiance* out, rr_radiance* noisy, float* albedo_out) {
    const Raytracing& rt = rh_with(h, fov, eye, up, dir, cnear, cfar, cfg, w, hgt);
    std::vector<rr_radiance> raw;
    const std::vector<rr_radiance> r = rt.render_denoised(Raytracing::AlbedoGuide::MEAN, params, nullptr, noisy ? &raw : nullptr);
    if (r.empty()) return -1;
    std::memcpy(out, r.data(), r.size() * sizeof(rr_radiance));
    if (noisy) std::memcpy(noisy, raw.data(), raw.size() * sizeof(rr_radiance));
    if (albedo_out) {
        const std::vector<float> a = rt.mean_albedo();
        if (a.empty()) return -1;
        std::memcpy(albedo_out, a.data(), a.size() * 4);
    }
    return 0;
}
// rh_render_pixel_split: Raytracing::render_pixel_split; xy = n entries or NULL (the whole frame, n = w * h); out = n records, diffuse = n * 3
// floats, halves = n * 2 records and diffuse_halves = n * 2 * 3 floats or both NULL; returns the number of records, or -1 when refused.
extern "C" int rh_render_pixel_split(void* h, float fov, const float* eye, const float* up, const float* dir, float cnear, float cfar, const rr_config* cfg,
                                     uint32_t w, uint32_t hgt, const uint32_t* xy, uint32_t n, rr_radiance* out, rr_radiance* halves, float* diffuse,
                                     float* diffuse_halves) {
    const Raytracing& rt = rh_with(h, fov, eye, up, dir, cnear, cfar, cfg, w, hgt);
    std::vector<rr_radiance> hv;
    std::vector<float> d, dh;
    const std::vector<rr_radiance> r = rt.render_pixel_split(xy, n, halves ? &hv : nullptr, &d, diffuse_halves ? &dh : nullptr);
    if (r.empty()) return -1;
    std::memcpy(out, r.data(), r.size() * sizeof(rr_radiance));
    std::memcpy(diffuse, d.data(), d.size() * 4);
    if (halves) std::memcpy(halves, hv.data(), hv.size() * sizeof(rr_radiance));
    if (diffuse_halves) std::memcpy(diffuse_halves, dh.data(), dh.size() * 4);
    return (int)r.size();
}
// rh_render_denoised_diffuse: Raytracing::render_denoised(AlbedoGuide::DIFFUSE); out = w * h records, noisy = the same or NULL; returns 0, or
// -1 when a call was refused.
extern "C" int rh_render_denoised_diffuse(void* h, float fov, const float* eye, const float* up, const float* dir, float cnear, float cfar, const rr_config* cfg,
                                          uint32_t w, uint32_t hgt, const rr_denoise_params* params, rr_radiance* out, rr_radiance* noisy) {
    const Raytracing& rt = rh_with(h, fov, eye, up, dir, cnear, cfar, cfg, w, hgt);
    std::vector<rr_radiance> raw;
    const std::vector<rr_radiance> r = rt.render_denoised(Raytracing::AlbedoGuide::DIFFUSE, params, nullptr, noisy ? &raw : nullptr);
    if (r.empty()) return -1;
    std::memcpy(out, r.data(), r.size() * sizeof(rr_radiance));
    if (noisy) std::memcpy(noisy, raw.data(), raw.size() * sizeof(rr_radiance));
    return 0;
}
// The history the four rh_accumulate* calls hand to Raytracing::accumulate*, from raw pointers of n pixels: empty without `history`
// (the first frame), a layer empty where its pointer is NULL.  The calls that are not split pass NULL for the two diffuse layers.
static Raytracing::SplitHistory rh_history(size_t n, const rr_radiance* history, const rr_radiance* history_halves, const float* history_diffuse,
                                           const float* history_diffuse_halves, const float* history_length) {
    Raytracing::SplitHistory hist;
    if (history) {
        hist.records.assign(history, history + n);
        if (history_halves) hist.halves.assign(history_halves, history_halves + 2 * n);
        if (history_diffuse) hist.diffuse.assign(history_diffuse, history_diffuse + 3 * n);
        if (history_diffuse_halves) hist.diffuse_halves.assign(history_diffuse_halves, history_diffuse_halves + 6 * n);
        if (history_length) hist.length.assign(history_length, history_length + n);
    }
    return hist;
}
// What such a call returned, copied out: 0, or -1 for an empty result (refused).  `layers`: the result as a SplitHistory, whose diffuse
// layers go to diffuse_out and diffuse_halves_out, or NULL for the calls that are not split.
static int rh_history_out(size_t n, const Raytracing::History& r, const Raytracing::SplitHistory* layers, const std::vector<uint8_t>& bytes, rr_radiance* out,
                          rr_radiance* halves_out, float* diffuse_out, float* diffuse_halves_out, float* length_out, uint8_t* rgba8) {
    if (r.empty()) return -1;
    std::memcpy(out, r.records.data(), n * sizeof(rr_radiance));
    if (halves_out && !r.halves.empty()) std::memcpy(halves_out, r.halves.data(), 2 * n * sizeof(rr_radiance));
    if (layers) std::memcpy(diffuse_out, layers->diffuse.data(), 3 * n * 4);
    if (layers && diffuse_halves_out && !layers->diffuse_halves.empty()) std::memcpy(diffuse_halves_out, layers->diffuse_halves.data(), 6 * n * 4);
    std::memcpy(length_out, r.length.data(), n * 4);
    if (rgba8) std::memcpy(rgba8, bytes.data(), bytes.size());
    return 0;
}
// Raytracing::accumulate: records = w * h, halves = w * h * 2 or NULL, history / history_halves / history_length = the previous call's
// out / halves_out / length_out or all NULL (the first frame), params or NULL for the defaults, motion = w * h * 3 floats or NULL; out,
// halves_out (with halves), length_out, rgba8 or NULL; returns 0, or -1 when the call was refused.
// rh_accumulate_records_device: Raytracing::accumulate_device on device pointers and a stream; returns its rr_status.
extern "C" int rh_accumulate_records(void* h, float fov, const float* eye, const float* up, const float* dir, float cnear, float cfar, const rr_config* cfg,
                                     uint32_t w, uint32_t hgt, const rr_radiance* records, const rr_radiance* halves, const rr_radiance* history,
                                     const rr_radiance* history_halves, const float* history_length, const rr_accumulate_params* params, const float* motion,
                                     rr_radiance* out, rr_radiance* halves_out, float* length_out, uint8_t* rgba8) {
    const Raytracing& rt = rh_with(h, fov, eye, up, dir, cnear, cfar, cfg, w, hgt);
    const size_t n = (size_t)w * hgt;
    const Raytracing::SplitHistory hist = rh_history(n, history, history_halves, nullptr, nullptr, history_length);
    std::vector<uint8_t> bytes;
    const Raytracing::History r = rt.accumulate(records, halves, history ? &hist : nullptr, params, motion, rgba8 ? &bytes : nullptr);
    return rh_history_out(n, r, nullptr, bytes, out, halves_out, nullptr, nullptr, length_out, rgba8);
}
extern "C" int rh_accumulate_records_device(void* h, float fov, const float* eye, const float* up, const float* dir, float cnear, float cfar, const rr_config* cfg,
                                            uint32_t w, uint32_t hgt, const rr_accumulate_params* params, const rr_radiance* records_dev, const rr_radiance* halves_dev,
                                            const rr_radiance* history_dev, const rr_radiance* history_halves_dev, const float* history_length_dev,
                                            const float* motion_dev, rr_radiance* out_dev, rr_radiance* halves_out_dev, float* length_out_dev, uint8_t* rgba8_dev,
                                            void* stream) {
    return rh_with(h, fov, eye, up, dir, cnear, cfar, cfg, w, hgt).accumulate_device(*params, records_dev, halves_dev, history_dev, history_halves_dev, history_length_dev,
                                                                                     motion_dev, out_dev, halves_out_dev, length_out_dev, rgba8_dev, stream);
}
// Raytracing::accumulate_split (on_device == 0: host pointers, through a SplitHistory; returns 0, or -1 when the call was refused) and
// Raytracing::accumulate_split_device (on_device != 0: device pointers and `stream`; returns its rr_status): the arguments of
// rr_accumulate_split_records in its order, params or NULL for the defaults (the host form only).
extern "C" int rh_accumulate_split(void* h, float fov, const float* eye, const float* up, const float* dir, float cnear, float cfar, const rr_config* cfg,
                                   uint32_t w, uint32_t hgt, const rr_accumulate_params* params, const rr_radiance* records, const rr_radiance* halves,
                                   const float* diffuse, const float* diffuse_halves, const rr_radiance* history, const rr_radiance* history_halves,
                                   const float* history_diffuse, const float* history_diffuse_halves, const float* history_length, const float* motion,
                                   rr_radiance* out, rr_radiance* halves_out, float* diffuse_out, float* diffuse_halves_out, float* length_out, uint8_t* rgba8,
                                   int on_device, void* stream) {
    const Raytracing& rt = rh_with(h, fov, eye, up, dir, cnear, cfar, cfg, w, hgt);
    if (on_device)
        return rt.accumulate_split_device(*params, records, halves, diffuse, diffuse_halves, history, history_halves, history_diffuse, history_diffuse_halves,
                                          history_length, motion, out, halves_out, diffuse_out, diffuse_halves_out, length_out, rgba8, stream);
    const size_t n = (size_t)w * hgt;
    const Raytracing::SplitHistory hist = rh_history(n, history, history_halves, history_diffuse, history_diffuse_halves, history_length);
    std::vector<uint8_t> bytes;
    const Raytracing::SplitHistory r = rt.accumulate_split(records, halves, diffuse, diffuse_halves, history ? &hist : nullptr, params, motion, rgba8 ? &bytes : nullptr);
    return rh_history_out(n, r, &r, bytes, out, halves_out, diffuse_out, diffuse_halves_out, length_out, rgba8);
}
// Raytracing::accumulate_clamped (on_device == 0: host pointers, through a History; returns 0, or -1 when the call was refused) and
// Raytracing::accumulate_clamped_device (on_device != 0: device pointers and `stream`; returns its rr_status): radius and sigma_scale, then
// the arguments of rr_accumulate_clamped_records behind `clamp`, params or NULL for the defaults (the host form only); radius 0: the
// library's default clamp.
extern "C" int rh_accumulate_clamped(void* h, float fov, const float* eye, const float* up, const float* dir, float cnear, float cfar, const rr_config* cfg,
                                     uint32_t w, uint32_t hgt, const rr_accumulate_params* params, uint32_t radius, float sigma_scale, const rr_radiance* records,
                                     const rr_radiance* halves, const rr_radiance* history, const rr_radiance* history_halves, const float* history_length,
                                     const float* motion, rr_radiance* out, rr_radiance* halves_out, float* length_out, uint8_t* rgba8, int on_device, void* stream) {
    const Raytracing& rt = rh_with(h, fov, eye, up, dir, cnear, cfar, cfg, w, hgt);
    const Raytracing::HistoryClamp clamp = radius ? Raytracing::HistoryClamp(radius, sigma_scale) : Raytracing::HistoryClamp();
    if (on_device)
        return rt.accumulate_clamped_device(*params, clamp, records, halves, history, history_halves, history_length, motion, out, halves_out, length_out, rgba8, stream);
    const size_t n = (size_t)w * hgt;
    const Raytracing::SplitHistory hist = rh_history(n, history, history_halves, nullptr, nullptr, history_length);
    std::vector<uint8_t> bytes;
    const Raytracing::History r = rt.accumulate_clamped(clamp, records, halves, history ? &hist : nullptr, params, motion, rgba8 ? &bytes : nullptr);
    return rh_history_out(n, r, nullptr, bytes, out, halves_out, nullptr, nullptr, length_out, rgba8);
}
// Raytracing::accumulate_clamped_split (on_device == 0: host pointers, through a SplitHistory; returns 0, or -1 when the call was refused)
// and Raytracing::accumulate_clamped_split_device (on_device != 0: device pointers and `stream`; returns its rr_status): radius and
// sigma_scale as rh_accumulate_clamped takes them, then the arguments of rh_accumulate_split.
extern "C" int rh_accumulate_clamped_split(void* h, float fov, const float* eye, const float* up, const float* dir, float cnear, float cfar, const rr_config* cfg,
                                           uint32_t w, uint32_t hgt, const rr_accumulate_params* params, uint32_t radius, float sigma_scale,
                                           const rr_radiance* records, const rr_radiance* halves, const float* diffuse, const float* diffuse_halves,
                                           const rr_radiance* history, const rr_radiance* history_halves, const float* history_diffuse,
                                           const float* history_diffuse_halves, const float* history_length, const float* motion, rr_radiance* out,
                                           rr_radiance* halves_out, float* diffuse_out, float* diffuse_halves_out, float* length_out, uint8_t* rgba8, int on_device,
                                           void* stream) {
    const Raytracing& rt = rh_with(h, fov, eye, up, dir, cnear, cfar, cfg, w, hgt);
    const Raytracing::HistoryClamp clamp = radius ? Raytracing::HistoryClamp(radius, sigma_scale) : Raytracing::HistoryClamp();
    if (on_device)
        return rt.accumulate_clamped_split_device(*params, clamp, records, halves, diffuse, diffuse_halves, history, history_halves, history_diffuse,
                                                  history_diffuse_halves, history_length, motion, out, halves_out, diffuse_out, diffuse_halves_out, length_out, rgba8,
                                                  stream);
    const size_t n = (size_t)w * hgt;
    const Raytracing::SplitHistory hist = rh_history(n, history, history_halves, history_diffuse, history_diffuse_halves, history_length);
    std::vector<uint8_t> bytes;
    const Raytracing::SplitHistory r = rt.accumulate_clamped_split(clamp, records, halves, diffuse, diffuse_halves, history ? &hist : nullptr, params, motion,
                                                                   rgba8 ? &bytes : nullptr);
    return rh_history_out(n, r, &r, bytes, out, halves_out, diffuse_out, diffuse_halves_out, length_out, rgba8);
}
// Raytracing::motion: records = w * h, item_index = n_moved indices, prev_trans = n_moved * 16 floats (column-major); motion_out = w * h * 3
// floats, world_out the same or NULL; returns 0, or -1 when the call was refused.
// rh_motion_records_device: Raytracing::motion_device on device pointers and a stream; returns its rr_status.
extern "C" int rh_motion_records(void* h, float fov, const float* eye, const float* up, const float* dir, float cnear, float cfar, const rr_config* cfg,
                                 uint32_t w, uint32_t hgt, const uint32_t* item_index, const float* prev_trans, uint32_t n_moved, const rr_radiance* records,
                                 float* motion_out, float* world_out) {
    const Raytracing& rt = rh_with(h, fov, eye, up, dir, cnear, cfar, cfg, w, hgt);
    const Raytracing::Motion r = rt.motion(records, item_index, prev_trans, n_moved, world_out != nullptr);
    if (r.empty()) return -1;
    std::memcpy(motion_out, r.motion.data(), r.motion.size() * 4);
    if (world_out) std::memcpy(world_out, r.world.data(), r.world.size() * 4);
    return 0;
}
extern "C" int rh_motion_records_device(void* h, float fov, const float* eye, const float* up, const float* dir, float cnear, float cfar, const rr_config* cfg,
                                        uint32_t w, uint32_t hgt, const uint32_t* item_index, const float* prev_trans, uint32_t n_moved,
                                        const rr_radiance* records_dev, float* motion_out_dev, float* world_out_dev, void* stream) {
    return rh_with(h, fov, eye, up, dir, cnear, cfar, cfg, w, hgt).motion_device(item_index, prev_trans, n_moved, records_dev, motion_out_dev, world_out_dev, stream);
}
// Raytracing::render_pixels called from on_pass of a progressive frame of the same scene: calls_refused[0] = the calls made there,
// [1] = how many of them were refused; returns the frame's rr_status
extern "C" int rh_render_pixels_from_on_pass(void* h, float fov, const float* eye, const float* up, const float* dir, float cnear, float cfar, const rr_config* cfg,
                                             uint32_t w, uint32_t hgt, uint32_t* calls_refused) {
    const Raytracing& rt = rh_with(h, fov, eye, up, dir, cnear, cfar, cfg, w, hgt);
    struct Ctx { const Raytracing* rt; uint32_t calls, refused; } ctx{&rt, 0u, 0u};
    const rr_camera cam = rt.camera.c_struct();
    const rr_config c = rt.config.c_struct();
    std::vector<uint8_t> rgba(4 * (size_t)w * hgt);
    const rr_frame fr{rgba.data(), nullptr, nullptr, nullptr};
    const int rc = rr_render_progressive(rt.scene->handle(), &cam, &c, nullptr, &fr, 2, [](void* user, uint64_t, uint64_t) -> int {
        Ctx* x = (Ctx*)user;
        const uint32_t xy = 0;
        x->calls++;
        if (x->rt->render_pixels(&xy, 1).empty() && x->rt->render(0, 0).x < 0) x->refused++;
        return 0;
    }, &ctx, nullptr);
    calls_refused[0] = ctx.calls; calls_refused[1] = ctx.refused;
    return rc;
}

// Raytracing::surface over n rays: out = n records of 128 bytes (rr_surface_hit); Raytracing::surface_device: the same on device buffers
extern "C" int rh_surface_rays(void* h, const float* origins, const float* dirs, uint32_t n, uint32_t depth, rr_surface_hit* out) {
    const Raytracing& rt = *((RhScene*)h)->rt;
    std::vector<Raytracing::Ray> rays(n);
    for (uint32_t i = 0; i < n; i++)
        rays[i] = Raytracing::Ray{Vec3{origins[3 * i], origins[3 * i + 1], origins[3 * i + 2]}, Vec3{dirs[3 * i], dirs[3 * i + 1], dirs[3 * i + 2]}};
    const std::vector<rr_surface_hit> r = rt.surface(rays.data(), rays.size(), depth);
    if (r.empty()) return -1;
    std::memcpy(out, r.data(), r.size() * sizeof(rr_surface_hit));
    return 0;
}

extern "C" int rh_surface_rays_device(void* h, const float* origins_dev, const float* dirs_dev, uint32_t n, uint32_t depth, rr_surface_hit* out_dev, void* stream) {
    return ((RhScene*)h)->rt->surface_device(origins_dev, dirs_dev, n, depth, out_dev, stream);
}

// one whole frame (min_passes passes) into the caller's buffers
extern "C" int rh_scene_render(void* hv, float fov, const float* eye, const float* up, const float* dir, float cnear, float cfar,
                               const rr_config* cfg, uint32_t w, uint32_t h, uint32_t min_passes,
                               uint8_t* rgba, float* normal, float* depth, uint32_t* ids) {
    RhScene* s = (RhScene*)hv;
    s->rt->camera = make_camera(fov, eye, up, dir, cnear, cfar);
    s->rt->config = RaytracingConfig();
    s->rt->config.apply(from_c(cfg));
    s->rt->config.seed = cfg->seed;
    RendererManager mgr((int32_t)w, (int32_t)h, s->rt);
    mgr.min_passes = min_passes;
    mgr.start();
    mgr.wait();
    std::vector<uint8_t> im; std::vector<float> nr, dp; std::vector<uint32_t> id;
    mgr.frame(&im, &nr, &dp, &id);
    std::memcpy(rgba, im.data(), im.size());
    std::memcpy(normal, nr.data(), nr.size() * 4);
    std::memcpy(depth, dp.data(), dp.size() * 4);
    std::memcpy(ids, id.data(), id.size() * 4);
    return mgr.failed() || !mgr.is_done() ? -2 : 0;
}
