// rustray_host.hpp — C++17 host layer over the C ABI of rustray_hip.h.
//
// The reference's host code around the trace loop is compiled Rust; no Rust toolchain exists in this pipeline, so
// this header restates, in C++, the part of that host code which drives the path: `Camera` (reference
// src/camera.rs:18-140), `RaytracingConfig` / `PixelData` / `Raytracing` (src/raytracing.rs:57-273) and
// `RendererManager` (src/renderer.rs:38-251) with the same names, argument meaning and call surface.  What changes
// behind that surface: `RendererManager::start` does not spawn num_cpus-2 workers over a queue of 2x2-pixel cells
// (src/renderer.rs:105-172) but ONE thread that issues a frame-level call into librustray_hip.so
// (rr_render_progressive); finished pixels arrive per pass (every pixel, more samples) instead of cell by cell.
//
// Header-only; link against librustray_hip.so.  Nothing here touches the GPU directly.
#pragma once

#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <functional>
#include <limits>
#include <memory>
#include <mutex>
#include <optional>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "rustray_hip.h"

namespace rustray {

// helper::approx_equal (reference src/helper.rs:11-20): six truncated decimals, in f32
inline bool approx_equal(float a, float b) {
    const float f = 1000000.0f;
    return std::trunc(a * f) == std::trunc(b * f);
}

struct Vec3 {
    float x = 0.0f, y = 0.0f, z = 0.0f;
};

// reference src/raytracing.rs:57-72
struct PixelData {
    uint8_t r = 0, g = 0, b = 0;
    Vec3 normal;
    float depth = 0.0f;
    uint32_t object_id = 0;
    int32_t x = 0, y = 0;
};

// reference src/raytracing.rs:92-185
struct RaytracingConfig {
    bool monte_carlo = false;
    uint16_t samples = 1; // this includes anti aliasing
    float focal_length = 1.0f;
    float aperture_size = 1.0f; // 1 means off
    float fog_density = 0.0f;
    Vec3 fog_color{0.4f, 0.4f, 0.4f};
    uint16_t max_recursion = 6;
    bool gamma_correction = false;
    uint64_t seed = 0; // not in the reference: its jitter draws from an un-seeded thread_rng

    // RaytracingConfig::apply: only fields that differ from the defaults are taken over (src/raytracing.rs:129-185)
    void apply(const RaytracingConfig& n) {
        const RaytracingConfig d;
        if (d.monte_carlo != n.monte_carlo) monte_carlo = n.monte_carlo;
        if (d.samples != n.samples) samples = n.samples;
        if (!approx_equal(d.focal_length, n.focal_length)) focal_length = n.focal_length;
        if (!approx_equal(d.aperture_size, n.aperture_size)) aperture_size = n.aperture_size;
        if (!approx_equal(d.fog_density, n.fog_density)) fog_density = n.fog_density;
        if (!approx_equal(d.fog_color.x, n.fog_color.x) || !approx_equal(d.fog_color.y, n.fog_color.y) || !approx_equal(d.fog_color.z, n.fog_color.z))
            fog_color = n.fog_color;
        if (d.max_recursion != n.max_recursion) max_recursion = n.max_recursion;
        if (d.gamma_correction != n.gamma_correction) gamma_correction = n.gamma_correction;
    }

    rr_config c_struct() const {
        rr_config c;
        std::memset(&c, 0, sizeof c);
        c.seed = seed;
        c.focal_length = focal_length; c.aperture_size = aperture_size; c.fog_density = fog_density;
        c.fog_color[0] = fog_color.x; c.fog_color[1] = fog_color.y; c.fog_color[2] = fog_color.z;
        c.samples = samples; c.max_recursion = max_recursion;
        c.monte_carlo = monte_carlo ? 1 : 0; c.gamma_correction = gamma_correction ? 1 : 0;
        return c;
    }
};

// reference src/camera.rs:10-15
constexpr float DEFAULT_FOV = 90.0f;
constexpr float DEFAULT_CLIPPING_NEAR = 0.001f;
constexpr float DEFAULT_CLIPPING_FAR = 1000.0f;

// reference src/camera.rs:18-140.  The trace loop consumes width, height and the two inverse matrices only
// (src/raytracing.rs:282-283, :349, :355, :369-393).  Matrices are column-major like nalgebra's; they are evaluated in
// double and rounded to f32 once, exactly as rustray_amd/camera.py does, so both host mirrors hand the library the
// same bits (the camera is harness code, outside the parity contract of the trace loop).
class Camera {
public:
    uint32_t width = 0, height = 0;
    float aspect_ratio = 0.0f;
    float fov = (float)(90.0 * 3.14159265358979323846 / 180.0);
    Vec3 eye_pos{0.0f, 0.0f, 0.0f}, up{0.0f, 1.0f, 0.0f}, dir{0.0f, 0.0f, -1.0f};
    float clipping_near = DEFAULT_CLIPPING_NEAR, clipping_far = DEFAULT_CLIPPING_FAR;
    double projection[16], view[16], projection_inverse[16], view_inverse[16]; // column-major

    Camera() {
        fov = (float)((double)DEFAULT_FOV * 3.14159265358979323846 / 180.0);
        identity(projection); identity(view); identity(projection_inverse); identity(view_inverse);
    }

    void init(uint32_t w, uint32_t h) { // src/camera.rs:69-77
        width = w; height = h;
        aspect_ratio = (float)w / (float)h;
        init_matrices();
    }

    void init_matrices() { // src/camera.rs:79-90: Perspective3::new, Isometry3::look_at_rh and their inverses
        const double a = aspect_ratio, fovy = fov, zn = clipping_near, zf = clipping_far;
        const double t = std::tan(fovy / 2.0);
        zero(projection);
        at(projection, 0, 0) = 1.0 / (a * t);
        at(projection, 1, 1) = 1.0 / t;
        at(projection, 2, 2) = (zf + zn) / (zn - zf);
        at(projection, 2, 3) = 2.0 * zf * zn / (zn - zf);
        at(projection, 3, 2) = -1.0;
        zero(projection_inverse);
        at(projection_inverse, 0, 0) = 1.0 / at(projection, 0, 0);
        at(projection_inverse, 1, 1) = 1.0 / at(projection, 1, 1);
        at(projection_inverse, 2, 3) = -1.0;
        at(projection_inverse, 3, 2) = 1.0 / at(projection, 2, 3);
        at(projection_inverse, 3, 3) = at(projection, 2, 2) / at(projection, 2, 3);
        const double e[3] = {eye_pos.x, eye_pos.y, eye_pos.z};
        const double tg[3] = {e[0] + (double)dir.x, e[1] + (double)dir.y, e[2] + (double)dir.z};
        double z[3] = {e[0] - tg[0], e[1] - tg[1], e[2] - tg[2]};
        normalize(z);
        const double u[3] = {up.x, up.y, up.z};
        double x[3]; cross(u, z, x); normalize(x);
        double y[3]; cross(z, x, y);
        identity(view);
        for (int k = 0; k < 3; k++) { at(view, 0, k) = x[k]; at(view, 1, k) = y[k]; at(view, 2, k) = z[k]; }
        at(view, 0, 3) = -dot(x, e); at(view, 1, 3) = -dot(y, e); at(view, 2, 3) = -dot(z, e);
        identity(view_inverse);
        for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) at(view_inverse, r, c) = at(view, c, r);
        for (int r = 0; r < 3; r++) at(view_inverse, r, 3) = e[r];
    }

    bool is_default_cam() const { // src/camera.rs:92-123
        return approx_equal(eye_pos.x, 0.0f) && approx_equal(eye_pos.y, 0.0f) && approx_equal(eye_pos.z, 0.0f) &&
               approx_equal(dir.x, 0.0f) && approx_equal(dir.y, 0.0f) && approx_equal(dir.z, -1.0f) &&
               approx_equal(up.x, 0.0f) && approx_equal(up.y, 1.0f) && approx_equal(up.z, 0.0f) &&
               approx_equal(fov, (float)((double)DEFAULT_FOV * 3.14159265358979323846 / 180.0)) &&
               approx_equal(clipping_near, DEFAULT_CLIPPING_NEAR) && approx_equal(clipping_far, DEFAULT_CLIPPING_FAR);
    }

    void set_cam_position(Vec3 eye, Vec3 d) { eye_pos = eye; dir = d; init_matrices(); } // src/camera.rs:125-131

    bool is_point_in_frustum(Vec3 p) const { // src/camera.rs:133-140
        double pv[16];
        for (int r = 0; r < 4; r++) for (int c = 0; c < 4; c++) {
            double s = 0.0;
            for (int k = 0; k < 4; k++) s += cat(projection, r, k) * cat(view, k, c);
            pv[c * 4 + r] = s;
        }
        const double h[4] = {p.x, p.y, p.z, 1.0};
        double o[4];
        for (int r = 0; r < 4; r++) { o[r] = 0.0; for (int k = 0; k < 4; k++) o[r] += pv[k * 4 + r] * h[k]; }
        return std::fabs(o[0]) <= o[3] && std::fabs(o[1]) <= o[3] && std::fabs(o[2]) <= o[3];
    }

    rr_camera c_struct() const {
        rr_camera c;
        c.width = width; c.height = height;
        for (int i = 0; i < 16; i++) { c.projection_inverse[i] = (float)projection_inverse[i]; c.view_inverse[i] = (float)view_inverse[i]; }
        return c;
    }
    // projection x view, column-major, and the eye: what the NEXT frame's rr_accumulate_params takes as prev_world_to_clip and prev_eye
    // (Raytracing::accumulate).  The product is formed in double and rounded once.
    void world_to_clip(float* m16, float* eye3) const {
        for (int c = 0; c < 4; c++)
            for (int r = 0; r < 4; r++) {
                double s = 0.0;
                for (int k = 0; k < 4; k++) s += projection[k * 4 + r] * view[c * 4 + k];
                m16[c * 4 + r] = (float)s;
            }
        for (int r = 0; r < 3; r++) eye3[r] = (float)view_inverse[12 + r];
    }

private:
    static double& at(double* m, int r, int c) { return m[c * 4 + r]; }
    static double cat(const double* m, int r, int c) { return m[c * 4 + r]; }
    static void zero(double* m) { for (int i = 0; i < 16; i++) m[i] = 0.0; }
    static void identity(double* m) { zero(m); m[0] = m[5] = m[10] = m[15] = 1.0; }
    static double dot(const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
    static void cross(const double* a, const double* b, double* o) {
        o[0] = a[1] * b[2] - a[2] * b[1]; o[1] = a[2] * b[0] - a[0] * b[2]; o[2] = a[0] * b[1] - a[1] * b[0];
    }
    static void normalize(double* v) { const double n = std::sqrt(dot(v, v)); v[0] /= n; v[1] /= n; v[2] /= n; }
};


// A flat scene under construction: owns the arrays an rr_flat_scene points to.  Stands in for what the Rust shim of
// INTEGRATION.md produces from `Scene` (items in Scene.items order, one texture-less material-cache entry per item).
struct Material { // defaults of Material::new, reference src/shape/mod.rs:138-180
    Vec3 ambient_color{0.0f, 0.0f, 0.0f}, base_color{1.0f, 1.0f, 1.0f}, specular_color{0.8f, 0.8f, 0.8f};
    float alpha = 1.0f, shininess = 150.0f, reflectivity = 0.0f, refraction_index = 1.0f, normal_map_strength = 1.0f;
    float shadow_softness = 0.01f, roughness = 0.0f;
    int32_t texture[RR_TEX_COUNT] = {-1, -1, -1, -1, -1, -1, -1, -1};
    bool texture_filtering_nearest = false, cast_shadow = true, receive_shadow = true, monte_carlo = true;
    bool smooth_shading = true, reflection_only = false, backface_cullig = true;

    rr_material c_struct(bool with_textures) const {
        rr_material m;
        std::memset(&m, 0, sizeof m);
        const Vec3* src[3] = {&ambient_color, &base_color, &specular_color};
        float* dst[3] = {m.ambient_color, m.base_color, m.specular_color};
        for (int k = 0; k < 3; k++) { dst[k][0] = src[k]->x; dst[k][1] = src[k]->y; dst[k][2] = src[k]->z; }
        m.alpha = alpha; m.shininess = shininess; m.reflectivity = reflectivity; m.refraction_index = refraction_index;
        m.normal_map_strength = normal_map_strength; m.shadow_softness = shadow_softness; m.roughness = roughness;
        for (int k = 0; k < RR_TEX_COUNT; k++) m.texture[k] = with_textures ? texture[k] : -1;
        m.texture_filtering_nearest = texture_filtering_nearest; m.cast_shadow = cast_shadow; m.receive_shadow = receive_shadow;
        m.monte_carlo = monte_carlo; m.smooth_shading = smooth_shading; m.reflection_only = reflection_only; m.backface_cullig = backface_cullig;
        return m;
    }
};

class FlatScene {
public:
    // a sphere of `radius` centred at `c` (Sphere::new + translation, reference src/shape/sphere.rs, src/shape/mod.rs:708-729)
    uint32_t add_sphere(Vec3 c, float radius, const Material& mat, uint32_t id) {
        rr_item it;
        std::memset(&it, 0, sizeof it);
        it.kind = RR_ITEM_SPHERE; it.id = id; it.mesh = -1; it.radius = radius;
        identity(it.trans); identity(it.trans_inv);
        it.trans[12] = c.x; it.trans[13] = c.y; it.trans[14] = c.z;
        it.trans_inv[12] = -c.x; it.trans_inv[13] = -c.y; it.trans_inv[14] = -c.z;
        for (int k = 0; k < 3; k++) { it.bbox_min[k] = -radius; it.bbox_max[k] = radius; }
        it.visible = 1;
        return push_item(it, mat);
    }
    // a triangle mesh in world space (identity transform); positions: 3 floats per vertex, indices: 3 per triangle
    uint32_t add_mesh(const std::vector<float>& positions, const std::vector<uint32_t>& indices, const Material& mat, uint32_t id) {
        mesh_pos_.push_back(positions); mesh_idx_.push_back(indices);
        rr_item it;
        std::memset(&it, 0, sizeof it);
        it.kind = RR_ITEM_MESH; it.id = id; it.mesh = (int32_t)mesh_pos_.size() - 1;
        identity(it.trans); identity(it.trans_inv);
        for (int k = 0; k < 3; k++) { it.bbox_min[k] = 3.0e38f; it.bbox_max[k] = -3.0e38f; }
        for (size_t v = 0; v + 2 < positions.size(); v += 3)
            for (int k = 0; k < 3; k++) { it.bbox_min[k] = std::fmin(it.bbox_min[k], positions[v + k]); it.bbox_max[k] = std::fmax(it.bbox_max[k], positions[v + k]); }
        it.visible = 1;
        return push_item(it, mat);
    }
    void add_point_light(Vec3 pos, float intensity, Vec3 color = Vec3{1.0f, 1.0f, 1.0f}) {
        rr_light l;
        std::memset(&l, 0, sizeof l);
        l.pos[0] = pos.x; l.pos[1] = pos.y; l.pos[2] = pos.z;
        l.color[0] = color.x; l.color[1] = color.y; l.color[2] = color.z;
        l.intensity = intensity; l.light_type = RR_LIGHT_POINT; l.enabled = 1;
        lights_.push_back(l);
    }
    // valid while this object lives and is not modified
    rr_flat_scene c_struct() {
        meshes_.clear();
        for (size_t i = 0; i < mesh_pos_.size(); i++) {
            rr_mesh m;
            std::memset(&m, 0, sizeof m);
            m.positions = mesh_pos_[i].data(); m.indices = mesh_idx_[i].data();
            m.n_vertices = (uint32_t)(mesh_pos_[i].size() / 3); m.n_triangles = (uint32_t)(mesh_idx_[i].size() / 3);
            meshes_.push_back(m);
        }
        rr_flat_scene fs;
        std::memset(&fs, 0, sizeof fs);
        fs.abi_version = RR_ABI_VERSION;
        fs.n_items = (uint32_t)items_.size(); fs.items = items_.data();
        fs.n_meshes = (uint32_t)meshes_.size(); fs.meshes = meshes_.data();
        fs.n_materials = (uint32_t)materials_.size(); fs.materials = materials_.data();
        fs.n_lights = (uint32_t)lights_.size(); fs.lights = lights_.data();
        return fs;
    }

private:
    static void identity(float* m) { for (int i = 0; i < 16; i++) m[i] = (i % 5 == 0) ? 1.0f : 0.0f; }
    uint32_t push_item(rr_item& it, const Material& mat) {
        materials_.push_back(mat.c_struct(true));  // get_material()
        materials_.push_back(mat.c_struct(false)); // get_material_cache_without_textures(), src/shape/mod.rs:769-772
        it.material = (int32_t)materials_.size() - 2; it.material_cache = (int32_t)materials_.size() - 1;
        items_.push_back(it);
        return (uint32_t)items_.size() - 1;
    }
    std::vector<rr_item> items_;
    std::vector<rr_material> materials_;
    std::vector<rr_light> lights_;
    std::vector<rr_mesh> meshes_;
    std::vector<std::vector<float>> mesh_pos_;
    std::vector<std::vector<uint32_t>> mesh_idx_;
};

// ---------------------------------------------------------------------------------------------------------
// Keyframe animation: reference src/animation.rs:9-205 and Scene::apply_frame (src/scene.rs:1695-1713).  Only item
// transforms change between frames, so a frame step on the device is rr_scene_update_transforms.
// ---------------------------------------------------------------------------------------------------------
struct Frame { // src/animation.rs:9-30; unset components are None in the reference
    std::string object_name;
    std::optional<Vec3> translation, rotation /* radians */, scale;
};
struct Keyframe { // src/animation.rs:35-52
    uint64_t time = 0; // milliseconds
    std::vector<Frame> objects;
};

class Animation {
public:
    bool enabled = false;
    uint32_t fps = 25;
    std::vector<Keyframe> keyframes;

    bool has_initial_keyframe() const { return !keyframes.empty() && keyframes[0].time == 0; }               // :79-88
    uint64_t get_frames_amount_to_render() const {                                                            // :90-98
        const uint64_t last = keyframes.empty() ? 0 : keyframes.back().time;
        return (uint64_t)std::floor((float)fps * ((float)last / 1000.0f));
    }
    bool has_animation() const {                                                                              // :100-103
        return enabled && get_frames_amount_to_render() > 0 && has_initial_keyframe() && keyframes.size() >= 2;
    }
    bool frame_exists(uint64_t frame) const { return has_animation() && frame < get_frames_amount_to_render(); } // scene.rs:1690-1693

    // :105-130: the keyframes around `frame` and the interpolation factor (NaN at the last keyframe: 1/0 * 0, as in Rust)
    void get_keyframes_for_frame(uint64_t frame, const Keyframe** first, const Keyframe** last, double* factor) const {
        const uint64_t timestamp = (uint64_t)std::floor((1000.0f / (float)fps) * (float)frame);
        *first = *last = &keyframes[0];
        for (size_t i = 0; i < keyframes.size(); i++)
            if (keyframes[i].time <= timestamp) { *first = &keyframes[i]; *last = (i + 1 >= keyframes.size()) ? &keyframes[i] : &keyframes[i + 1]; }
        const double pos = (double)(timestamp - (*first)->time), diff = (double)((*last)->time - (*first)->time);
        *factor = 1.0 / diff * pos;
    }

    // :132-205: interpolated T * Rz * Ry * Rx * S of one object for `frame` (column-major), false if it has no keyframes
    bool get_trans_for_frame(uint64_t frame, const std::string& object_name, float out[16]) const {
        const Keyframe *kf, *kl; double factor;
        get_keyframes_for_frame(frame, &kf, &kl, &factor);
        const Frame *a = nullptr, *b = nullptr;
        for (const Frame& f : kf->objects) if (f.object_name == object_name) { a = &f; break; }
        for (const Frame& f : kl->objects) if (f.object_name == object_name) { b = &f; break; }
        if (!a || !b) return false;
        const float f = (float)factor;
        auto lerp = [f](const std::optional<Vec3>& p, const std::optional<Vec3>& q, Vec3 d) {
            if (!p || !q) return d;
            return Vec3{p->x + f * (q->x - p->x), p->y + f * (q->y - p->y), p->z + f * (q->z - p->z)}; // helper::interpolate
        };
        const Vec3 t = lerp(a->translation, b->translation, Vec3{0.0f, 0.0f, 0.0f});
        const Vec3 sc = lerp(a->scale, b->scale, Vec3{1.0f, 1.0f, 1.0f});
        const Vec3 r = lerp(a->rotation, b->rotation, Vec3{0.0f, 0.0f, 0.0f});
        get_transformation(t, sc, r, out);
        return true;
    }

    // ShapeBasics::get_transformation on the identity (src/shape/mod.rs:708-729): T * Rz * Ry * Rx * S, f32, column-major
    static void get_transformation(Vec3 t, Vec3 s, Vec3 r, float out[16]) {
        float m[16]; ident(m);
        float f[16];
        ident(f); f[12] = t.x; f[13] = t.y; f[14] = t.z; mul(m, f);
        rot(2, r.z, f); mul(m, f);
        rot(1, r.y, f); mul(m, f);
        rot(0, r.x, f); mul(m, f);
        ident(f); f[0] = s.x; f[5] = s.y; f[10] = s.z; mul(m, f);
        std::memcpy(out, m, sizeof m);
    }

    // ShapeBasics::calc_inverse (src/shape/mod.rs:763-767) of an affine matrix; evaluated in double, rounded to f32
    static void inverse_affine(const float m[16], float out[16]) {
        const double a = m[0], b = m[4], c = m[8], d = m[1], e = m[5], f = m[9], g = m[2], h = m[6], i = m[10];
        const double det = a * (e * i - f * h) - b * (d * i - f * g) + c * (d * h - e * g);
        const double r[9] = {(e * i - f * h) / det, (c * h - b * i) / det, (b * f - c * e) / det,
                             (f * g - d * i) / det, (a * i - c * g) / det, (c * d - a * f) / det,
                             (d * h - e * g) / det, (b * g - a * h) / det, (a * e - b * d) / det}; // row-major inverse of the 3x3
        const double tx = m[12], ty = m[13], tz = m[14];
        for (int k = 0; k < 16; k++) out[k] = 0.0f;
        for (int rr = 0; rr < 3; rr++) {
            for (int cc = 0; cc < 3; cc++) out[cc * 4 + rr] = (float)r[rr * 3 + cc];
            out[12 + rr] = (float)(-(r[rr * 3] * tx + r[rr * 3 + 1] * ty + r[rr * 3 + 2] * tz));
        }
        out[15] = 1.0f;
    }

    // Scene::apply_frame on the arrays rr_scene_update_transforms takes: `trans` / `trans_inv` hold n_items * 16 floats
    // (start from the items' own matrices); items named in the keyframes get their matrix REPLACED (apply_mat).
    // Returns false when the reference would not touch the scene.
    bool frame_transforms(const std::vector<std::string>& item_names, uint64_t frame, float* trans, float* trans_inv) const {
        if (!has_animation() || frame > get_frames_amount_to_render()) return false;
        for (size_t i = 0; i < item_names.size(); i++) {
            float m[16];
            if (get_trans_for_frame(frame, item_names[i], m)) std::memcpy(trans + 16 * i, m, sizeof m);
            inverse_affine(trans + 16 * i, trans_inv + 16 * i);
        }
        return true;
    }

private:
    static void ident(float* m) { for (int k = 0; k < 16; k++) m[k] = (k % 5 == 0) ? 1.0f : 0.0f; }
    static void rot(int axis, float a, float* m) {
        ident(m);
        const float c = (float)std::cos((double)a), s = (float)std::sin((double)a);
        if (axis == 0) { m[5] = c; m[9] = -s; m[6] = s; m[10] = c; }
        else if (axis == 1) { m[0] = c; m[8] = s; m[2] = -s; m[10] = c; }
        else { m[0] = c; m[4] = -s; m[1] = s; m[5] = c; }
    }
    static void mul(float* m, const float* f) { // m = m * f, f32 accumulation in nalgebra's column-axpy order
        float o[16];
        for (int c = 0; c < 4; c++)
            for (int r = 0; r < 4; r++) {
                float acc = m[r] * f[c * 4];
                for (int k = 1; k < 4; k++) acc = acc + m[k * 4 + r] * f[c * 4 + k];
                o[c * 4 + r] = acc;
            }
        std::memcpy(m, o, sizeof o);
    }
};

// A scene resident on one GPU (rr_scene), owned.
class DeviceScene {
public:
    DeviceScene(const rr_flat_scene& flat, int device = 0) {
        if (rr_scene_create(&flat, device, &h_) != RR_OK) { error_ = rr_last_error(); h_ = nullptr; }
    }
    ~DeviceScene() { if (h_) rr_scene_destroy(h_); }
    DeviceScene(const DeviceScene&) = delete;
    DeviceScene& operator=(const DeviceScene&) = delete;
    rr_scene* handle() const { return h_; }
    bool ok() const { return h_ != nullptr; }
    const std::string& error() const { return error_; }

    // Edits in place between frames (include/rustray_hip.h); each returns the rr_status and keeps rr_last_error() in error() on failure.
    // The whole light list, in Scene::lights order (a light's index is the RNG stream of its shadow jitter).
    int update_lights(const std::vector<rr_light>& lights) { return check(rr_scene_update_lights(h_, lights.data(), (uint32_t)lights.size())); }
    // ShapeBasics::visible / flip_normals of every item, in Scene::items order.
    int update_item_flags(const std::vector<uint8_t>& visible, const std::vector<uint8_t>& flip_normals) {
        if (visible.size() != flip_normals.size()) { error_ = "update_item_flags: visible and flip_normals differ in length"; return RR_ERR_INVALID_ARGUMENT; }
        return check(rr_scene_update_item_flags(h_, visible.data(), flip_normals.data(), (uint32_t)visible.size()));
    }
    // Appends images to the texture list; *first_index: the index of the first (name it in a following material update).
    int add_textures(const std::vector<rr_texture>& textures, uint32_t* first_index) {
        return check(rr_scene_add_textures(h_, textures.data(), (uint32_t)textures.size(), first_index));
    }
    // Appends meshes to the mesh list; *first_index: the index of the first (name it in a following set_items).
    int add_meshes(const std::vector<rr_mesh>& meshes, uint32_t* first_index) {
        return check(rr_scene_add_meshes(h_, meshes.data(), (uint32_t)meshes.size(), first_index));
    }
    // The whole item list and the whole material list the items name, together (the GUI's object "delete", "add ground plane",
    // "add environment sphere"); an item's `mesh` is an index into the resident meshes.
    int set_items(const std::vector<rr_item>& items, const std::vector<rr_material>& materials) {
        return check(rr_scene_set_items(h_, items.data(), (uint32_t)items.size(), materials.data(), (uint32_t)materials.size()));
    }

private:
    int check(int rc) { if (rc != RR_OK) error_ = rr_last_error(); return rc; }
    rr_scene* h_ = nullptr;
    std::string error_;
};

// reference src/raytracing.rs:205-427: scene + config.  A frame is one device call (RendererManager); the per-pixel `render(x, y)` is
// here too, for one pixel and for lists of pixels (render, render_pixels: rr_render_pixels)
class Raytracing {
public:
    std::shared_ptr<DeviceScene> scene;
    Camera camera; // Scene::cam in the reference (src/scene.rs:69-83)
    RaytracingConfig config;

    explicit Raytracing(std::shared_ptr<DeviceScene> s) : scene(std::move(s)) {}

    float gamma_encode(float linear) const { return std::pow(linear, 1.0f / 2.2f); } // src/raytracing.rs:231-235

    // Raytracing::pick (src/raytracing.rs:237-273): Some((id, distance)) of the item under the pixel, or None
    std::optional<std::pair<uint32_t, float>> pick(int x, int y) const {
        rr_pick_result r;
        const rr_camera c = camera.c_struct();
        if (rr_pick(scene->handle(), &c, x, y, &r) != RR_OK || !r.hit) return std::nullopt;
        return std::make_pair(r.object_id, r.distance);
    }

    // Raytracing::trace(ray, true, true, depth) with `in_light = toi > len` (src/raytracing.rs:429-490, :883-892): the occluder of one
    // shadow ray as (item index, face id, toi), or None when the ray is lit.  max_distance: the distance to a point or spot light;
    // infinity (the default) = a directional light, no limit.
    struct ShadowHit { uint32_t item_index, face_id; float toi; };
    std::optional<ShadowHit> trace_shadow(const Vec3& origin, const Vec3& dir, uint32_t depth,
                                          float max_distance = std::numeric_limits<float>::infinity()) const {
        const float o[3] = {origin.x, origin.y, origin.z}, d[3] = {dir.x, dir.y, dir.z};
        rr_shadow_hit r;
        if (rr_trace_shadow_rays(scene->handle(), o, d, &max_distance, 1, depth, &r) != RR_OK || !r.occluded) return std::nullopt;
        return ShadowHit{r.item_index, r.face_id, r.distance};
    }

    // Raytracing::get_color_depth_normal_id(scene, ray, 1) (src/raytracing.rs:720-998) for a span of rays of the host's own, with this
    // handle's config (seed, monte_carlo, max_recursion, fog): (colour, depth, normal, object id) per ray when rays_per_result is 1,
    // or the mean over every rays_per_result consecutive rays.  The colour is LINEAR (no min(., 1), no gamma).  An empty vector =
    // refused or failed (rr_last_error() says why).  stream_ids: the RNG pixel id per result, or nullptr = the result's index.
    struct Ray { Vec3 origin, dir; };
    std::vector<rr_radiance> shade_rays(const Ray* rays, size_t n_rays, uint32_t rays_per_result = 1, const uint32_t* stream_ids = nullptr) const {
        std::vector<rr_radiance> out;
        if (rays_per_result == 0 || n_rays == 0 || n_rays % rays_per_result != 0 || n_rays / rays_per_result > 0x7fffff00u) return out;
        std::vector<float> o(3 * n_rays), d(3 * n_rays);
        for (size_t i = 0; i < n_rays; i++) {
            o[3 * i] = rays[i].origin.x; o[3 * i + 1] = rays[i].origin.y; o[3 * i + 2] = rays[i].origin.z;
            d[3 * i] = rays[i].dir.x; d[3 * i + 1] = rays[i].dir.y; d[3 * i + 2] = rays[i].dir.z;
        }
        const rr_config c = config.c_struct();
        out.resize(n_rays / rays_per_result);
        if (rr_shade_rays(scene->handle(), &c, o.data(), d.data(), (uint32_t)out.size(), rays_per_result, stream_ids, out.data(), nullptr) != RR_OK) out.clear();
        return out;
    }

    // Raytracing::render(x, y) -> PixelData (src/raytracing.rs:275-427): one pixel of this handle's camera with this handle's config (the
    // built-in sub-sample table, depth of field, all samples) -- the bytes, normal, depth and id a frame holds for that pixel.  A pixel
    // outside the frame, or a failed call, gives a default PixelData with x = y = -1 (rr_last_error() says why).  One device call per
    // pixel: for more than a few, use render_pixels.
    PixelData render(int x, int y) const {
        PixelData p;
        p.x = -1; p.y = -1;
        if (x < 0 || y < 0 || x > 65535 || y > 65535) return p;
        const uint32_t xy = (uint32_t)x | ((uint32_t)y << 16);
        std::vector<uint8_t> bytes;
        const std::vector<rr_radiance> r = render_pixels(&xy, 1, &bytes);
        if (r.size() != 1) return p;
        p.r = bytes[0]; p.g = bytes[1]; p.b = bytes[2];
        p.normal = Vec3{r[0].normal[0], r[0].normal[1], r[0].normal[2]};
        p.depth = r[0].depth; p.object_id = r[0].object_id;
        p.x = x; p.y = y;
        return p;
    }
    // What `render` holds BEFORE its clamp, as linear floats, for n pixels xy[i] = x | y << 16 in any order (list neighbours should be
    // screen neighbours: 8x8 blocks), or for every pixel of the frame in row-major order when xy is nullptr (n is then ignored).
    // rgba8 (optional): the frame's own 4 bytes per pixel.  An empty vector = refused or failed (rr_last_error() says why).
    std::vector<rr_radiance> render_pixels(const uint32_t* xy, size_t n, std::vector<uint8_t>* rgba8 = nullptr) const {
        std::vector<rr_radiance> out;
        const rr_camera cam = camera.c_struct();
        const rr_config c = config.c_struct();
        if (!xy) n = (size_t)cam.width * cam.height;
        if (n == 0 || n > ((size_t)1 << 30)) return out;
        out.resize(n);
        if (rgba8) rgba8->assign(4 * n, 0);
        if (rr_render_pixels(scene->handle(), &cam, &c, nullptr, xy, (uint32_t)n, out.data(), rgba8 ? rgba8->data() : nullptr, nullptr) != RR_OK) {
            out.clear();
            if (rgba8) rgba8->clear();
        }
        return out;
    }
    // the same on DEVICE buffers, in stream order (rr_render_pixels_device): as shade_device below; xy_dev nullptr = the whole frame
    // (n_pixels = width * height), rgba8_out_dev optional
    int render_pixels_device(const uint32_t* xy_dev, uint32_t n_pixels, rr_radiance* out_dev, uint8_t* rgba8_out_dev, void* hip_stream,
                             const volatile int* cancel = nullptr) const {
        const rr_camera cam = camera.c_struct();
        const rr_config c = config.c_struct();
        return rr_render_pixels_device(scene->handle(), &cam, &c, nullptr, xy_dev, n_pixels, out_dev, rgba8_out_dev, hip_stream, cancel);
    }

    // render_pixels, and per pixel the means over its n_parts interleaved sample subsets (rr_render_pixel_parts): part h of a pixel is
    // the samples s of config.samples with s % n_parts == h.  n_parts: a power of two from 2 to 64 that divides config.samples.  Returns
    // the full records (byte for byte render_pixels') and fills parts[i * n_parts + h].  Both empty = refused or failed (rr_last_error()
    // says why).  At n_parts = 2, |A - B| / 2 of a pixel's two part colours estimates the error of its mean.
    std::vector<rr_radiance> render_pixel_parts(const uint32_t* xy, size_t n, uint32_t n_parts, std::vector<rr_radiance>* parts) const {
        std::vector<rr_radiance> out;
        if (parts) parts->clear();
        const rr_camera cam = camera.c_struct();
        const rr_config c = config.c_struct();
        if (!xy) n = (size_t)cam.width * cam.height;
        if (!parts || n == 0 || n_parts == 0 || n_parts > 64 || n * n_parts > ((size_t)1 << 30)) return out;
        out.resize(n);
        parts->resize(n * n_parts);
        if (rr_render_pixel_parts(scene->handle(), &cam, &c, nullptr, xy, (uint32_t)n, n_parts, out.data(), parts->data(), nullptr) != RR_OK) {
            out.clear();
            parts->clear();
        }
        return out;
    }
    // the same on DEVICE buffers, in stream order (rr_render_pixel_parts_device): xy_dev nullptr = the whole frame (n_pixels = width * height)
    int render_pixel_parts_device(const uint32_t* xy_dev, uint32_t n_pixels, uint32_t n_parts, rr_radiance* out_dev, rr_radiance* parts_out_dev,
                                  void* hip_stream, const volatile int* cancel = nullptr) const {
        const rr_camera cam = camera.c_struct();
        const rr_config c = config.c_struct();
        return rr_render_pixel_parts_device(scene->handle(), &cam, &c, nullptr, xy_dev, n_pixels, n_parts, out_dev, parts_out_dev, hip_stream, cancel);
    }

    // render_pixel_parts at n_parts = 2 and, as a sum of its own, the frame's direct diffuse light of the primary hits (rr_render_pixel_split):
    // returns the full records and fills halves[i * 2 + h], diffuse[i * 3 + c] and diffuse_halves[(i * 2 + h) * 3 + c].  halves and
    // diffuse_halves are both given or both nullptr (then the records are render_pixels' and config.samples may be odd).  All empty =
    // refused or failed (rr_last_error() says why).  color - diffuse is everything the base colour does not modulate.
    std::vector<rr_radiance> render_pixel_split(const uint32_t* xy, size_t n, std::vector<rr_radiance>* halves, std::vector<float>* diffuse,
                                                std::vector<float>* diffuse_halves) const {
        std::vector<rr_radiance> out;
        if (halves) halves->clear();
        if (diffuse) diffuse->clear();
        if (diffuse_halves) diffuse_halves->clear();
        const rr_camera cam = camera.c_struct();
        const rr_config c = config.c_struct();
        if (!xy) n = (size_t)cam.width * cam.height;
        if (!diffuse || (halves == nullptr) != (diffuse_halves == nullptr) || n == 0 || n * 2 > ((size_t)1 << 30)) return out;
        out.resize(n);
        diffuse->assign(3 * n, 0.0f);
        if (halves) { halves->resize(2 * n); diffuse_halves->assign(6 * n, 0.0f); }
        if (rr_render_pixel_split(scene->handle(), &cam, &c, nullptr, xy, (uint32_t)n, out.data(), halves ? halves->data() : nullptr, diffuse->data(),
                                  halves ? diffuse_halves->data() : nullptr, nullptr) != RR_OK) {
            out.clear();
            diffuse->clear();
            if (halves) { halves->clear(); diffuse_halves->clear(); }
        }
        return out;
    }
    // the same on DEVICE buffers, in stream order (rr_render_pixel_split_device): xy_dev nullptr = the whole frame (n_pixels = width * height)
    int render_pixel_split_device(const uint32_t* xy_dev, uint32_t n_pixels, rr_radiance* out_dev, rr_radiance* halves_out_dev, float* diffuse_out_dev,
                                  float* diffuse_halves_out_dev, void* hip_stream, const volatile int* cancel = nullptr) const {
        const rr_camera cam = camera.c_struct();
        const rr_config c = config.c_struct();
        return rr_render_pixel_split_device(scene->handle(), &cam, &c, nullptr, xy_dev, n_pixels, out_dev, halves_out_dev, diffuse_out_dev, diffuse_halves_out_dev,
                                            hip_stream, cancel);
    }

    // A frame at two sample counts (rr_render_adaptive): every pixel at base_samples (even, at least 2), and at max_samples where the
    // half-buffer error of the base frame -- max over channels of |min(A, 1) - min(B, 1)| / 2 of the pixel's two halves -- exceeds
    // `threshold`; estimate, list, fine pass and scatter run on the device under one hold of the scene's lock.  config.samples is ignored.
    // Returns the records in row-major order, each byte for byte render_pixels' at the count `samples` names there; samples, error, rgba8
    // and n_refined are optional.  An empty vector = refused or failed (rr_last_error() says why).
    std::vector<rr_radiance> render_adaptive(uint16_t base_samples, uint16_t max_samples, float threshold, std::vector<uint16_t>* samples = nullptr,
                                             std::vector<float>* error = nullptr, std::vector<uint8_t>* rgba8 = nullptr, uint32_t* n_refined = nullptr) const {
        return fused_call(samples, error, rgba8, nullptr, 0, [&](const rr_camera* cam, const rr_config* c, rr_radiance* o, uint8_t* b, uint16_t* sm, float* e, uint32_t*) {
            return rr_render_adaptive(scene->handle(), cam, c, base_samples, max_samples, threshold, nullptr, nullptr, o, b, sm, e, n_refined, nullptr);
        });
    }
    // the same on DEVICE buffers, in stream order (rr_render_adaptive_device): out_dev holds width * height records; the other buffers are optional
    int render_adaptive_device(uint16_t base_samples, uint16_t max_samples, float threshold, rr_radiance* out_dev, uint8_t* rgba8_out_dev, uint16_t* samples_out_dev,
                               float* error_out_dev, uint32_t* n_refined, void* hip_stream, const volatile int* cancel = nullptr) const {
        const rr_camera cam = camera.c_struct();
        const rr_config c = config.c_struct();
        return rr_render_adaptive_device(scene->handle(), &cam, &c, base_samples, max_samples, threshold, nullptr, nullptr, out_dev, rgba8_out_dev, samples_out_dev,
                                         error_out_dev, n_refined, hip_stream, cancel);
    }

    // A frame at a ladder of sample counts (rr_render_adaptive_levels): every pixel at levels[0], and level after level the pixels whose
    // half-buffer error still exceeds `threshold` at the next count (2 to RR_MAX_ADAPTIVE_LEVELS counts, even and strictly increasing),
    // on the device under one hold of the scene's lock.  config.samples is ignored.  Returns the records in row-major order, each byte
    // for byte render_pixels' at the count `samples` names there; `error` is the RESIDUAL error, of the pixel's halves at that count;
    // level_pixels gets the pixels rendered at each level.  samples, error, rgba8 and level_pixels are optional.  An empty vector =
    // refused or failed (rr_last_error() says why).
    std::vector<rr_radiance> render_adaptive_levels(const std::vector<uint16_t>& levels, float threshold, std::vector<uint16_t>* samples = nullptr,
                                                    std::vector<float>* error = nullptr, std::vector<uint8_t>* rgba8 = nullptr,
                                                    std::vector<uint32_t>* level_pixels = nullptr) const {
        return fused_call(samples, error, rgba8, level_pixels, levels.size(), [&](const rr_camera* cam, const rr_config* c, rr_radiance* o, uint8_t* b, uint16_t* sm, float* e, uint32_t* lp) {
            return rr_render_adaptive_levels(scene->handle(), cam, c, levels.data(), (uint32_t)levels.size(), threshold, nullptr, o, b, sm, e, lp, nullptr);
        });
    }
    // the same on DEVICE buffers, in stream order (rr_render_adaptive_levels_device): out_dev holds width * height records, level_pixels (HOST, or
    // NULL) n_levels words; the other buffers are optional
    int render_adaptive_levels_device(const uint16_t* levels, uint32_t n_levels, float threshold, rr_radiance* out_dev, uint8_t* rgba8_out_dev, uint16_t* samples_out_dev,
                                      float* error_out_dev, uint32_t* level_pixels, void* hip_stream, const volatile int* cancel = nullptr) const {
        const rr_camera cam = camera.c_struct();
        const rr_config c = config.c_struct();
        return rr_render_adaptive_levels_device(scene->handle(), &cam, &c, levels, n_levels, threshold, nullptr, out_dev, rgba8_out_dev, samples_out_dev, error_out_dev,
                                                level_pixels, hip_stream, cancel);
    }

    // render_pixels over the first samples_used samples of the frame of config.samples samples (rr_render_pixel_prefix): that frame's table,
    // cell size and generator keys, the sums divided by samples_used.  halves (or nullptr; samples_used must then be even) gets the two
    // interleaved halves of those samples, halves[i * 2 + h]; rgba8 (or nullptr) the frame's bytes.  An empty vector = refused or failed.
    std::vector<rr_radiance> render_pixel_prefix(const uint32_t* xy, size_t n, uint32_t samples_used, std::vector<rr_radiance>* halves = nullptr,
                                                 std::vector<uint8_t>* rgba8 = nullptr) const {
        std::vector<rr_radiance> out;
        if (halves) halves->clear();
        if (rgba8) rgba8->clear();
        const rr_camera cam = camera.c_struct();
        const rr_config c = config.c_struct();
        if (!xy) n = (size_t)cam.width * cam.height;
        if (n == 0 || n > ((size_t)1 << 29)) return out;
        out.resize(n);
        if (halves) halves->resize(2 * n);
        if (rgba8) rgba8->assign(4 * n, 0);
        if (rr_render_pixel_prefix(scene->handle(), &cam, &c, nullptr, xy, (uint32_t)n, samples_used, out.data(), halves ? halves->data() : nullptr,
                                   rgba8 ? rgba8->data() : nullptr, nullptr) != RR_OK) {
            out.clear();
            if (halves) halves->clear();
            if (rgba8) rgba8->clear();
        }
        return out;
    }
    // the same on DEVICE buffers, in stream order (rr_render_pixel_prefix_device): xy_dev nullptr = the whole frame (n_pixels = width * height)
    int render_pixel_prefix_device(const uint32_t* xy_dev, uint32_t n_pixels, uint32_t samples_used, rr_radiance* out_dev, rr_radiance* halves_out_dev,
                                   uint8_t* rgba8_out_dev, void* hip_stream, const volatile int* cancel = nullptr) const {
        const rr_camera cam = camera.c_struct();
        const rr_config c = config.c_struct();
        return rr_render_pixel_prefix_device(scene->handle(), &cam, &c, nullptr, xy_dev, n_pixels, samples_used, out_dev, halves_out_dev, rgba8_out_dev, hip_stream, cancel);
    }

    // A frame at a ladder of PREFIXES of one frame of config.samples samples (rr_render_adaptive_prefix): every pixel over its first
    // prefixes[0] samples, and level after level only the samples up to the next prefix for the pixels whose half-buffer error still
    // exceeds `threshold`, added to the sums those pixels keep on the device.  2 to RR_MAX_ADAPTIVE_LEVELS prefixes, even and strictly
    // increasing, the last one config.samples.  Returns the records in row-major order, each byte for byte render_pixel_prefix's at the
    // count `samples` names there; the optional outputs are those of render_adaptive_levels.  An empty vector = refused or failed.
    std::vector<rr_radiance> render_adaptive_prefix(const std::vector<uint16_t>& prefixes, float threshold, std::vector<uint16_t>* samples = nullptr,
                                                    std::vector<float>* error = nullptr, std::vector<uint8_t>* rgba8 = nullptr,
                                                    std::vector<uint32_t>* level_pixels = nullptr) const {
        return fused_call(samples, error, rgba8, level_pixels, prefixes.size(), [&](const rr_camera* cam, const rr_config* c, rr_radiance* o, uint8_t* b, uint16_t* sm, float* e, uint32_t* lp) {
            return rr_render_adaptive_prefix(scene->handle(), cam, c, nullptr, prefixes.data(), (uint32_t)prefixes.size(), threshold, o, b, sm, e, lp, nullptr);
        });
    }
    // the same on DEVICE buffers, in stream order (rr_render_adaptive_prefix_device): the buffers of render_adaptive_levels_device
    int render_adaptive_prefix_device(const uint16_t* prefixes, uint32_t n_levels, float threshold, rr_radiance* out_dev, uint8_t* rgba8_out_dev, uint16_t* samples_out_dev,
                                      float* error_out_dev, uint32_t* level_pixels, void* hip_stream, const volatile int* cancel = nullptr) const {
        const rr_camera cam = camera.c_struct();
        const rr_config c = config.c_struct();
        return rr_render_adaptive_prefix_device(scene->handle(), &cam, &c, nullptr, prefixes, n_levels, threshold, out_dev, rgba8_out_dev, samples_out_dev, error_out_dev,
                                                level_pixels, hip_stream, cancel);
    }

    // The a-trous filter over a frame of this camera's size (rr_denoise_records): `records` width * height records in row-major order,
    // `halves` twice as many in the layout of render_pixel_parts at n_parts = 2 or nullptr (geometry only), `albedo` width * height * 3
    // floats or nullptr; `params` nullptr = rr_denoise_default_params.  Returns the filtered records (depth, normal and id are the
    // input's bits); variance (or nullptr) gets the last variance, rgba8 (or nullptr) the frame's bytes of the filtered records.  An
    // empty vector = refused or failed (rr_last_error() says why).
    std::vector<rr_radiance> denoise(const rr_radiance* records, const rr_radiance* halves, const float* albedo, const rr_denoise_params* params = nullptr,
                                     std::vector<float>* variance = nullptr, std::vector<uint8_t>* rgba8 = nullptr) const {
        std::vector<rr_radiance> out;
        const size_t n = (size_t)camera.width * camera.height;
        rr_denoise_params prm;
        if (params) prm = *params;
        else if (rr_denoise_default_params(&prm) != RR_OK) return out;
        if (!records || n == 0 || n > ((size_t)1 << 29)) return out;
        out.resize(n);
        if (variance) variance->assign(n, 0.0f);
        if (rgba8) rgba8->assign(4 * n, 0);
        if (rr_denoise_records(scene->handle(), camera.width, camera.height, &prm, records, halves, albedo, out.data(), rgba8 ? rgba8->data() : nullptr,
                               variance ? variance->data() : nullptr) != RR_OK) {
            out.clear();
            if (variance) variance->clear();
            if (rgba8) rgba8->clear();
        }
        return out;
    }
    // The whole frame in two halves (render_pixel_parts at n_parts = 2; config.samples even) followed by the filter guided by their
    // variance.  noisy (or nullptr) gets the records before the filter.  An empty vector = refused or failed.
    // with_albedo: one rr_surface_pixels call between the two makes this camera's albedo() and the filter runs on albedo-demodulated colour.
    std::vector<rr_radiance> render_denoised(const rr_denoise_params* params = nullptr, std::vector<uint8_t>* rgba8 = nullptr,
                                             std::vector<rr_radiance>* noisy = nullptr, bool with_albedo = false) const {
        std::vector<rr_radiance> halves;
        const std::vector<rr_radiance> records = render_pixel_parts(nullptr, 0, 2, &halves);
        if (records.empty()) return records;
        if (noisy) *noisy = records;
        std::vector<float> guide;
        if (with_albedo) {
            guide = albedo();
            if (guide.empty()) return std::vector<rr_radiance>();
        }
        return denoise(records.data(), halves.data(), with_albedo ? guide.data() : nullptr, params, nullptr, rgba8);
    }
    // The same with the albedo guide named: NONE and CENTRE are with_albedo = false and true above, bit for bit; MEAN takes mean_albedo(),
    // one rr_albedo_pixels call with this frame's config in place of the rr_surface_pixels call.  DIFFUSE: the frame comes from
    // render_pixel_split, the albedo is mean_albedo(), and rr_denoise_split_records demodulates the direct diffuse part of the colour alone.
    enum class AlbedoGuide { NONE, CENTRE, MEAN, DIFFUSE };
    std::vector<rr_radiance> render_denoised(AlbedoGuide guide_kind, const rr_denoise_params* params = nullptr, std::vector<uint8_t>* rgba8 = nullptr,
                                             std::vector<rr_radiance>* noisy = nullptr) const {
        if (guide_kind == AlbedoGuide::DIFFUSE) {
            std::vector<rr_radiance> halves, out;
            std::vector<float> diffuse, diffuse_halves;
            const std::vector<rr_radiance> records = render_pixel_split(nullptr, 0, &halves, &diffuse, &diffuse_halves);
            if (records.empty()) return records;
            if (noisy) *noisy = records;
            const std::vector<float> guide = mean_albedo();
            rr_denoise_params prm;
            if (params) prm = *params;
            else if (rr_denoise_default_params(&prm) != RR_OK) return out;
            if (guide.empty()) return out;
            out.resize(records.size());
            if (rgba8) rgba8->assign(4 * records.size(), 0);
            if (rr_denoise_split_records(scene->handle(), camera.width, camera.height, &prm, records.data(), halves.data(), diffuse.data(), diffuse_halves.data(),
                                         guide.data(), out.data(), rgba8 ? rgba8->data() : nullptr) != RR_OK) {
                out.clear();
                if (rgba8) rgba8->clear();
            }
            return out;
        }
        if (guide_kind != AlbedoGuide::MEAN) return render_denoised(params, rgba8, noisy, guide_kind == AlbedoGuide::CENTRE);
        std::vector<rr_radiance> halves;
        const std::vector<rr_radiance> records = render_pixel_parts(nullptr, 0, 2, &halves);
        if (records.empty()) return records;
        if (noisy) *noisy = records;
        const std::vector<float> guide = mean_albedo();
        if (guide.empty()) return std::vector<rr_radiance>();
        return denoise(records.data(), halves.data(), guide.data(), params, nullptr, rgba8);
    }

    // The albedo of the whole frame as the frame of config.samples samples sees it (rr_albedo_pixels): width * height * 3 floats in
    // row-major order, per pixel the mean over the frame's primary rays of the base colour at each ray's first hit -- at an edge pixel the
    // mix its colour was modulated by, where albedo() holds the colour under the pixel's centre.  empty = refused or failed.
    std::vector<float> mean_albedo() const {
        std::vector<float> out;
        const size_t n = (size_t)camera.width * camera.height;
        if (n == 0 || n > ((size_t)1 << 30)) return out;
        const rr_camera cam = camera.c_struct();
        const rr_config c = config.c_struct();
        out.assign(3 * n, 0.0f);
        if (rr_albedo_pixels(scene->handle(), &cam, &c, nullptr, nullptr, (uint32_t)n, out.data(), nullptr) != RR_OK) out.clear();
        return out;
    }
    // the same on DEVICE buffers, in stream order (rr_albedo_pixels_device): xy_dev nullptr = the whole frame (n_pixels = width * height)
    int mean_albedo_device(const uint32_t* xy_dev, uint32_t n_pixels, float* albedo_out_dev, void* hip_stream, const volatile int* cancel = nullptr) const {
        const rr_camera cam = camera.c_struct();
        const rr_config c = config.c_struct();
        return rr_albedo_pixels_device(scene->handle(), &cam, &c, nullptr, xy_dev, n_pixels, albedo_out_dev, hip_stream, cancel);
    }

    // The G-buffer of this camera (rr_surface_pixels): the rr_surface_hit record of the pinhole ray through the centre of each pixel --
    // xy[i] = x | y << 16, n_pixels entries, or xy nullptr for the whole frame in row-major order -- byte for byte what surface() gives
    // for that ray at depth 1.  albedo_out (or nullptr) gets 3 floats per pixel, the records' base_color and 0 for a miss: what
    // denoise() takes as `albedo`.  An empty vector = refused or failed (rr_last_error() says why).
    std::vector<rr_surface_hit> surface_pixels(const uint32_t* xy = nullptr, size_t n_pixels = 0, std::vector<float>* albedo_out = nullptr) const {
        std::vector<rr_surface_hit> out;
        const size_t n = xy ? n_pixels : (size_t)camera.width * camera.height;
        if (n == 0 || n > 0x7fffff00u) return out;
        const rr_camera cam = camera.c_struct();
        out.resize(n);
        if (albedo_out) albedo_out->assign(3 * n, 0.0f);
        if (rr_surface_pixels(scene->handle(), &cam, xy, (uint32_t)n, out.data(), albedo_out ? albedo_out->data() : nullptr) != RR_OK) {
            out.clear();
            if (albedo_out) albedo_out->clear();
        }
        return out;
    }
    // the albedo of the whole frame alone: width * height * 3 floats in row-major order; empty = refused or failed
    std::vector<float> albedo() const {
        std::vector<float> out;
        const size_t n = (size_t)camera.width * camera.height;
        if (n == 0 || n > 0x7fffff00u) return out;
        const rr_camera cam = camera.c_struct();
        out.assign(3 * n, 0.0f);
        if (rr_surface_pixels(scene->handle(), &cam, nullptr, (uint32_t)n, nullptr, out.data()) != RR_OK) out.clear();
        return out;
    }
    // the same on DEVICE buffers, in stream order (rr_surface_pixels_device): xy_dev nullptr = the whole frame (n_pixels = width * height),
    // which is enqueued and not waited for; out_dev or albedo_out_dev may be nullptr, not both
    int surface_pixels_device(const uint32_t* xy_dev, uint32_t n_pixels, rr_surface_hit* out_dev, float* albedo_out_dev, void* hip_stream) const {
        const rr_camera cam = camera.c_struct();
        return rr_surface_pixels_device(scene->handle(), &cam, xy_dev, n_pixels, out_dev, albedo_out_dev, hip_stream);
    }

    // The joint-bilateral upsampler to a frame of this camera's size (rr_upsample_records): `low` low_width * low_height records of a frame
    // traced at that size in row-major order, `halves_low` twice as many in the layout of render_pixel_parts at n_parts = 2 or nullptr,
    // `guide_low` and `guide` the surface_pixels() of the small camera and of this one; `params` nullptr = rr_upsample_default_params.
    // Returns width * height records whose depth, normal and id are the full guide's; halves_out (required exactly when halves_low is
    // given) gets twice as many, weight (or nullptr) the guided sum's weight per pixel (0: the bilinear fallback answered), rgba8 (or
    // nullptr) the frame's bytes of the records.  An empty vector = refused or failed (rr_last_error() says why).
    // albedo_low (low_width * low_height * 3 floats) and albedo (width * height * 3), each or nullptr: albedo planes in place of the guides'
    // base colours (rr_upsample_albedo_records), e.g. mean_albedo() of the two cameras; with both nullptr the call is rr_upsample_records.
    std::vector<rr_radiance> upsample(uint32_t low_width, uint32_t low_height, const rr_radiance* low, const rr_radiance* halves_low, const rr_surface_hit* guide_low,
                                      const rr_surface_hit* guide, const rr_upsample_params* params = nullptr, std::vector<rr_radiance>* halves_out = nullptr,
                                      std::vector<float>* weight = nullptr, std::vector<uint8_t>* rgba8 = nullptr, const float* albedo_low = nullptr,
                                      const float* albedo = nullptr) const {
        std::vector<rr_radiance> out;
        const size_t n = (size_t)camera.width * camera.height;
        rr_upsample_params prm;
        if (params) prm = *params;
        else if (rr_upsample_default_params(&prm) != RR_OK) return out;
        if (n == 0 || n > ((size_t)1 << 29)) return out;
        out.resize(n);
        if (halves_out) halves_out->assign(2 * n, rr_radiance{});
        if (weight) weight->assign(n, 0.0f);
        if (rgba8) rgba8->assign(4 * n, 0);
        rr_radiance* const ho = halves_out ? halves_out->data() : nullptr;
        uint8_t* const bytes = rgba8 ? rgba8->data() : nullptr;
        float* const wt = weight ? weight->data() : nullptr;
        const int rc = albedo_low || albedo
            ? rr_upsample_albedo_records(scene->handle(), low_width, low_height, camera.width, camera.height, &prm, low, halves_low, guide_low, guide, albedo_low, albedo,
                                         out.data(), ho, bytes, wt)
            : rr_upsample_records(scene->handle(), low_width, low_height, camera.width, camera.height, &prm, low, halves_low, guide_low, guide, out.data(), ho, bytes, wt);
        if (rc != RR_OK) {
            out.clear();
            if (halves_out) halves_out->clear();
            if (weight) weight->clear();
            if (rgba8) rgba8->clear();
        }
        return out;
    }
    // the same on DEVICE buffers, in stream order (rr_upsample_records_device): one launch, not waited for; nothing may overlap
    int upsample_device(uint32_t low_width, uint32_t low_height, const rr_upsample_params* params, const rr_radiance* low_dev, const rr_radiance* halves_low_dev,
                        const rr_surface_hit* guide_low_dev, const rr_surface_hit* guide_dev, rr_radiance* out_dev, rr_radiance* halves_out_dev, uint8_t* rgba8_out_dev,
                        float* weight_out_dev, void* hip_stream, const float* albedo_low_dev = nullptr, const float* albedo_dev = nullptr) const {
        rr_upsample_params prm;
        if (params) prm = *params;
        else if (const int rc = rr_upsample_default_params(&prm)) return rc;
        if (albedo_low_dev || albedo_dev)   // (rr_upsample_albedo_records_device: the planes are 4-byte aligned)
            return rr_upsample_albedo_records_device(scene->handle(), low_width, low_height, camera.width, camera.height, &prm, low_dev, halves_low_dev, guide_low_dev,
                                                     guide_dev, albedo_low_dev, albedo_dev, out_dev, halves_out_dev, rgba8_out_dev, weight_out_dev, hip_stream);
        return rr_upsample_records_device(scene->handle(), low_width, low_height, camera.width, camera.height, &prm, low_dev, halves_low_dev, guide_low_dev, guide_dev,
                                          out_dev, halves_out_dev, rgba8_out_dev, weight_out_dev, hip_stream);
    }
    // The frame traced at ceil(width / scale) x ceil(height / scale) with this camera's matrices (config.samples even) and raised to full
    // size: rr_render_pixel_parts at n_parts = 2 on the small camera, rr_surface_pixels on both, upsample() with halves and, with
    // denoise_params, denoise() with the full guide's albedo.  weight (or nullptr) gets upsample()'s.  An empty vector = refused or failed.
    // albedo_kind: CENTRE, the guides' pixel-centre albedo; MEAN, the low frame is demodulated by rr_albedo_pixels on the small camera with
    // this config, the mean over the rays that made the colour (anything else is refused).  full_albedo_samples: 0, or k >= 1:
    // rr_albedo_pixels on this camera at k samples remodulates and, with denoise_params, guides the full-size filter.  low_denoise_params:
    // rr_denoise_records at the low size on the low records and halves before the upsampler, with the low albedo in use; the filtered
    // records are raised without halves and the full-size filter runs without them.
    std::vector<rr_radiance> render_upsampled(uint32_t scale = 2, const rr_upsample_params* params = nullptr, const rr_denoise_params* denoise_params = nullptr,
                                              std::vector<uint8_t>* rgba8 = nullptr, std::vector<float>* weight = nullptr, AlbedoGuide albedo_kind = AlbedoGuide::CENTRE,
                                              uint32_t full_albedo_samples = 0, const rr_denoise_params* low_denoise_params = nullptr) const {
        const std::vector<rr_radiance> none;
        if (scale == 0 || camera.width == 0 || camera.height == 0) return none;
        if (albedo_kind != AlbedoGuide::CENTRE && albedo_kind != AlbedoGuide::MEAN) return none;
        const rr_camera cam = camera.c_struct();
        rr_camera low_cam = cam;
        low_cam.width = (cam.width + scale - 1) / scale;
        low_cam.height = (cam.height + scale - 1) / scale;
        const rr_config c = config.c_struct();
        const size_t nl = (size_t)low_cam.width * low_cam.height, n = (size_t)cam.width * cam.height;
        if (n > 0x7fffff00u) return none;
        std::vector<rr_radiance> low(nl), halves_low(2 * nl), halves;
        std::vector<rr_surface_hit> guide_low(nl), guide(n);
        if (rr_render_pixel_parts(scene->handle(), &low_cam, &c, nullptr, nullptr, (uint32_t)nl, 2, low.data(), halves_low.data(), nullptr) != RR_OK) return none;
        if (rr_surface_pixels(scene->handle(), &low_cam, nullptr, (uint32_t)nl, guide_low.data(), nullptr) != RR_OK) return none;
        if (rr_surface_pixels(scene->handle(), &cam, nullptr, (uint32_t)n, guide.data(), nullptr) != RR_OK) return none;
        std::vector<float> plane_low, plane;
        if (albedo_kind == AlbedoGuide::MEAN) {
            plane_low.assign(3 * nl, 0.0f);
            if (rr_albedo_pixels(scene->handle(), &low_cam, &c, nullptr, nullptr, (uint32_t)nl, plane_low.data(), nullptr) != RR_OK) return none;
        }
        if (full_albedo_samples) {
            rr_config ck = c;
            ck.samples = full_albedo_samples;
            plane.assign(3 * n, 0.0f);
            if (rr_albedo_pixels(scene->handle(), &cam, &ck, nullptr, nullptr, (uint32_t)n, plane.data(), nullptr) != RR_OK) return none;
        }
        const auto centre_albedo = [](const std::vector<rr_surface_hit>& g) {
            std::vector<float> a(3 * g.size());
            for (size_t i = 0; i < g.size(); i++)
                for (int k = 0; k < 3; k++) a[3 * i + k] = g[i].base_color[k];
            return a;
        };
        if (low_denoise_params) {
            const std::vector<float> a = plane_low.empty() ? centre_albedo(guide_low) : plane_low;
            std::vector<rr_radiance> filtered(nl);
            if (rr_denoise_records(scene->handle(), low_cam.width, low_cam.height, low_denoise_params, low.data(), halves_low.data(), a.data(), filtered.data(), nullptr,
                                   nullptr) != RR_OK) return none;
            low.swap(filtered);
        }
        const bool with_halves = !low_denoise_params;
        const std::vector<rr_radiance> up = upsample(low_cam.width, low_cam.height, low.data(), with_halves ? halves_low.data() : nullptr, guide_low.data(), guide.data(), params,
                                                     with_halves ? &halves : nullptr, weight, denoise_params ? nullptr : rgba8,
                                                     plane_low.empty() ? nullptr : plane_low.data(), plane.empty() ? nullptr : plane.data());
        if (up.empty() || !denoise_params) return up;
        const std::vector<float> guide_albedo = plane.empty() ? centre_albedo(guide) : plane;
        return denoise(up.data(), with_halves ? halves.data() : nullptr, guide_albedo.data(), denoise_params, nullptr, rgba8);
    }

    // What accumulate() returns and takes back as the history of the next call: the accumulated records, halves and lengths.
    struct History {
        std::vector<rr_radiance> records, halves; // width * height, and twice as many in the K = 2 layout (empty: no halves)
        std::vector<float> length;                // width * height (0: the pixel has no history)
        bool empty() const { return records.empty(); }
    };
    // Temporal accumulation over a frame of this camera (rr_accumulate_records): `records` width * height records in row-major order,
    // `halves` twice as many or nullptr; `history` what the previous call returned (nullptr or empty: the first frame; with halves it
    // must hold halves as well); `params` carries the PREVIOUS frame's view (prev_world_to_clip, prev_eye: Camera::world_to_clip() and
    // eye_pos of the camera that frame was rendered with) and nullptr = rr_accumulate_default_params; `motion` width * height * 3 floats
    // or nullptr.  rgba8 (or nullptr) gets the frame's bytes of the accumulated records.  An empty History = refused or failed
    // (rr_last_error() says why).
    History accumulate(const rr_radiance* records, const rr_radiance* halves, const History* history, const rr_accumulate_params* params = nullptr,
                       const float* motion = nullptr, std::vector<uint8_t>* rgba8 = nullptr) const {
        return colour_part(accumulate_call(false, nullptr, records, halves, nullptr, nullptr, history, nullptr, params, motion, rgba8));
    }
    // the same on DEVICE buffers, in stream order (rr_accumulate_records_device): not waited for
    int accumulate_device(const rr_accumulate_params& params, const rr_radiance* records_dev, const rr_radiance* halves_dev, const rr_radiance* history_dev,
                          const rr_radiance* history_halves_dev, const float* history_length_dev, const float* motion_dev, rr_radiance* out_dev,
                          rr_radiance* halves_out_dev, float* length_out_dev, uint8_t* rgba8_out_dev, void* hip_stream) const {
        const rr_camera cam = camera.c_struct();
        return rr_accumulate_records_device(scene->handle(), &cam, &params, records_dev, halves_dev, history_dev, history_halves_dev, history_length_dev, motion_dev,
                                            out_dev, halves_out_dev, length_out_dev, rgba8_out_dev, hip_stream);
    }

    // The clamp of accumulate_clamped(): rr_history_clamp_params with the library's defaults filled in.
    struct HistoryClamp : rr_history_clamp_params {
        HistoryClamp() { rr_history_clamp_default_params(this); }
        HistoryClamp(uint32_t radius_, float sigma_scale_) {
            rr_history_clamp_default_params(this);
            radius = radius_;
            sigma_scale = sigma_scale_;
        }
    };
    // accumulate() with the history held to the current frame's colours around each pixel (rr_accumulate_clamped_records): for the frames
    // after an edit that moves no geometry -- lights, materials, textures, item flags -- and under moving shadows, where accumulate()
    // would blend the stale colour in for up to max_history frames.  The arguments are accumulate()'s behind `clamp`.
    History accumulate_clamped(const HistoryClamp& clamp, const rr_radiance* records, const rr_radiance* halves, const History* history,
                               const rr_accumulate_params* params = nullptr, const float* motion = nullptr, std::vector<uint8_t>* rgba8 = nullptr) const {
        return colour_part(accumulate_call(false, &clamp, records, halves, nullptr, nullptr, history, nullptr, params, motion, rgba8));
    }
    // the same on DEVICE buffers, in stream order (rr_accumulate_clamped_records_device): not waited for; out_dev may not be records_dev
    int accumulate_clamped_device(const rr_accumulate_params& params, const HistoryClamp& clamp, const rr_radiance* records_dev, const rr_radiance* halves_dev,
                                  const rr_radiance* history_dev, const rr_radiance* history_halves_dev, const float* history_length_dev, const float* motion_dev,
                                  rr_radiance* out_dev, rr_radiance* halves_out_dev, float* length_out_dev, uint8_t* rgba8_out_dev, void* hip_stream) const {
        const rr_camera cam = camera.c_struct();
        return rr_accumulate_clamped_records_device(scene->handle(), &cam, &params, &clamp, records_dev, halves_dev, history_dev, history_halves_dev,
                                                    history_length_dev, motion_dev, out_dev, halves_out_dev, length_out_dev, rgba8_out_dev, hip_stream);
    }

    // What accumulate_split() returns and takes back: History plus the accumulated diffuse layers of rr_render_pixel_split.
    struct SplitHistory : History {
        std::vector<float> diffuse, diffuse_halves; // width * height * 3, and twice as many (empty: no halves)
    };

  private:
    // THE host form behind accumulate(), accumulate_clamped(), accumulate_split() and accumulate_clamped_split(): the variant by `split`
    // (the calls with the diffuse layers, which also refuse a frame without `diffuse`) and `clamp` (nullptr: the calls without one).  It
    // sizes the result, passes a history only when there is one (its halves only when it holds halves; `layers` is the same history seen
    // as a SplitHistory, nullptr in the calls that are not split), and empties the result and rgba8 when the library refuses or fails.
    SplitHistory accumulate_call(bool split, const HistoryClamp* clamp, const rr_radiance* records, const rr_radiance* halves, const float* diffuse,
                                 const float* diffuse_halves, const History* history, const SplitHistory* layers, const rr_accumulate_params* params,
                                 const float* motion, std::vector<uint8_t>* rgba8) const {
        SplitHistory out;
        const size_t n = (size_t)camera.width * camera.height;
        rr_accumulate_params prm;
        if (params) prm = *params;
        else if (rr_accumulate_default_params(&prm) != RR_OK) return out;
        if (!records || (split && !diffuse) || n == 0 || n > ((size_t)1 << 29)) return out;
        const bool first = !history || history->empty();
        const bool hist_halves = !first && !history->halves.empty();
        const rr_camera cam = camera.c_struct();
        out.records.resize(n);
        out.length.assign(n, 0.0f);
        if (halves) out.halves.resize(2 * n);
        if (split) out.diffuse.resize(3 * n);
        if (split && halves) out.diffuse_halves.resize(6 * n);
        if (rgba8) rgba8->assign(4 * n, 0);
        // the buffers by the names of the C arguments, in their order: the history, then the outputs
        const rr_radiance* h = first ? nullptr : history->records.data();
        const rr_radiance* h_halves = hist_halves ? history->halves.data() : nullptr;
        const float* h_diffuse = first || !layers || layers->diffuse.empty() ? nullptr : layers->diffuse.data();
        const float* h_diffuse_halves = hist_halves && layers && !layers->diffuse_halves.empty() ? layers->diffuse_halves.data() : nullptr;
        const float* h_length = first ? nullptr : history->length.data();
        rr_radiance* o = out.records.data();
        rr_radiance* o_halves = halves ? out.halves.data() : nullptr;
        float* o_diffuse = out.diffuse.data();
        float* o_diffuse_halves = halves ? out.diffuse_halves.data() : nullptr;
        float* o_length = out.length.data();
        uint8_t* bytes = rgba8 ? rgba8->data() : nullptr;
        rr_scene* s = scene->handle();
        int rc;
        if (!split && !clamp) rc = rr_accumulate_records(s, &cam, &prm, records, halves, h, h_halves, h_length, motion, o, o_halves, o_length, bytes);
        else if (!split) rc = rr_accumulate_clamped_records(s, &cam, &prm, clamp, records, halves, h, h_halves, h_length, motion, o, o_halves, o_length, bytes);
        else if (!clamp)
            rc = rr_accumulate_split_records(s, &cam, &prm, records, halves, diffuse, diffuse_halves, h, h_halves, h_diffuse, h_diffuse_halves, h_length, motion, o,
                                             o_halves, o_diffuse, o_diffuse_halves, o_length, bytes);
        else
            rc = rr_accumulate_clamped_split_records(s, &cam, &prm, clamp, records, halves, diffuse, diffuse_halves, h, h_halves, h_diffuse, h_diffuse_halves, h_length,
                                                     motion, o, o_halves, o_diffuse, o_diffuse_halves, o_length, bytes);
        if (rc != RR_OK) {
            out = SplitHistory();
            if (rgba8) rgba8->clear();
        }
        return out;
    }
    // the History a call that is not split returns: the vectors moved out of the helper's result, not copied
    static History colour_part(SplitHistory&& all) { return History(std::move(static_cast<History&>(all))); }

  public:
    // Temporal accumulation of a split frame (rr_accumulate_split_records): accumulate() with `diffuse` width * height * 3 floats and
    // `diffuse_halves` twice as many (exactly when `halves` is given) blended by the same taps, weights and length.  The result feeds
    // denoise_split as it is.  An empty SplitHistory = refused or failed (rr_last_error() says why).
    SplitHistory accumulate_split(const rr_radiance* records, const rr_radiance* halves, const float* diffuse, const float* diffuse_halves,
                                  const SplitHistory* history, const rr_accumulate_params* params = nullptr, const float* motion = nullptr,
                                  std::vector<uint8_t>* rgba8 = nullptr) const {
        return accumulate_call(true, nullptr, records, halves, diffuse, diffuse_halves, history, history, params, motion, rgba8);
    }
    // the same on DEVICE buffers, in stream order (rr_accumulate_split_records_device): not waited for
    int accumulate_split_device(const rr_accumulate_params& params, const rr_radiance* records_dev, const rr_radiance* halves_dev, const float* diffuse_dev,
                                const float* diffuse_halves_dev, const rr_radiance* history_dev, const rr_radiance* history_halves_dev,
                                const float* history_diffuse_dev, const float* history_diffuse_halves_dev, const float* history_length_dev, const float* motion_dev,
                                rr_radiance* out_dev, rr_radiance* halves_out_dev, float* diffuse_out_dev, float* diffuse_halves_out_dev, float* length_out_dev,
                                uint8_t* rgba8_out_dev, void* hip_stream) const {
        const rr_camera cam = camera.c_struct();
        return rr_accumulate_split_records_device(scene->handle(), &cam, &params, records_dev, halves_dev, diffuse_dev, diffuse_halves_dev, history_dev,
                                                  history_halves_dev, history_diffuse_dev, history_diffuse_halves_dev, history_length_dev, motion_dev, out_dev,
                                                  halves_out_dev, diffuse_out_dev, diffuse_halves_out_dev, length_out_dev, rgba8_out_dev, hip_stream);
    }
    // accumulate_split() with the history held to the current frame (rr_accumulate_clamped_split_records): the colour layers as
    // accumulate_clamped() holds them, the diffuse layers to the box of the current `diffuse` around each pixel.  The arguments are
    // accumulate_split()'s behind `clamp`; the result feeds denoise_split as it is.
    SplitHistory accumulate_clamped_split(const HistoryClamp& clamp, const rr_radiance* records, const rr_radiance* halves, const float* diffuse,
                                          const float* diffuse_halves, const SplitHistory* history, const rr_accumulate_params* params = nullptr,
                                          const float* motion = nullptr, std::vector<uint8_t>* rgba8 = nullptr) const {
        return accumulate_call(true, &clamp, records, halves, diffuse, diffuse_halves, history, history, params, motion, rgba8);
    }
    // the same on DEVICE buffers, in stream order (rr_accumulate_clamped_split_records_device): not waited for; out_dev may not be records_dev
    // and diffuse_out_dev not diffuse_dev
    int accumulate_clamped_split_device(const rr_accumulate_params& params, const HistoryClamp& clamp, const rr_radiance* records_dev, const rr_radiance* halves_dev,
                                        const float* diffuse_dev, const float* diffuse_halves_dev, const rr_radiance* history_dev,
                                        const rr_radiance* history_halves_dev, const float* history_diffuse_dev, const float* history_diffuse_halves_dev,
                                        const float* history_length_dev, const float* motion_dev, rr_radiance* out_dev, rr_radiance* halves_out_dev,
                                        float* diffuse_out_dev, float* diffuse_halves_out_dev, float* length_out_dev, uint8_t* rgba8_out_dev,
                                        void* hip_stream) const {
        const rr_camera cam = camera.c_struct();
        return rr_accumulate_clamped_split_records_device(scene->handle(), &cam, &params, &clamp, records_dev, halves_dev, diffuse_dev, diffuse_halves_dev,
                                                          history_dev, history_halves_dev, history_diffuse_dev, history_diffuse_halves_dev, history_length_dev,
                                                          motion_dev, out_dev, halves_out_dev, diffuse_out_dev, diffuse_halves_out_dev, length_out_dev,
                                                          rgba8_out_dev, hip_stream);
    }

    // What motion() returns: width * height * 3 floats of motion, and of world points where asked for.
    struct Motion {
        std::vector<float> motion, world;
        bool empty() const { return motion.empty(); }
    };
    // The motion of moved items per pixel of a frame of this camera (rr_motion_records), what accumulate() takes as `motion` when items
    // moved since the history was rendered: `records` width * height records of the current frame; item_index[k] names a moved item and
    // prev_trans + 16 k is its `trans` in the frame of the history, column-major (what rr_scene_update_transforms was given then).
    // An empty Motion = refused or failed (rr_last_error() says why).
    Motion motion(const rr_radiance* records, const uint32_t* item_index, const float* prev_trans, uint32_t n_moved, bool want_world = false) const {
        Motion out;
        const size_t n = (size_t)camera.width * camera.height;
        if (!records || n == 0 || n > ((size_t)1 << 29)) return out;
        const rr_camera cam = camera.c_struct();
        out.motion.assign(3 * n, 0.0f);
        if (want_world) out.world.assign(3 * n, 0.0f);
        if (rr_motion_records(scene->handle(), &cam, item_index, prev_trans, n_moved, records, out.motion.data(), want_world ? out.world.data() : nullptr) != RR_OK)
            out = Motion();
        return out;
    }
    // the same on DEVICE buffers, in stream order (rr_motion_records_device): not waited for; item_index and prev_trans are host arrays
    int motion_device(const uint32_t* item_index, const float* prev_trans, uint32_t n_moved, const rr_radiance* records_dev, float* motion_out_dev,
                      float* world_out_dev, void* hip_stream) const {
        const rr_camera cam = camera.c_struct();
        return rr_motion_records_device(scene->handle(), &cam, item_index, prev_trans, n_moved, records_dev, motion_out_dev, world_out_dev, hip_stream);
    }

    // The surface of the closest hits of a span of rays of the host's own (rr_surface_rays): Raytracing::trace(ray, false, false, depth)
    // and, at the hit, what get_color_depth_normal_id evaluates before its light loop (src/raytracing.rs:747-811, :928-933, :985-991) --
    // hit point, normals, uv, the three colours, alpha, reflectivity, roughness, ambient occlusion.  No config is used.  depth 1 = a
    // frame's primary ray.  One record per ray (hit == 0: nothing hit); an empty vector = refused or failed (rr_last_error() says why).
    std::vector<rr_surface_hit> surface(const Ray* rays, size_t n_rays, uint32_t depth = 1) const {
        std::vector<rr_surface_hit> out;
        if (n_rays == 0 || n_rays > 0x7fffff00u) return out;
        std::vector<float> o(3 * n_rays), d(3 * n_rays);
        for (size_t i = 0; i < n_rays; i++) {
            o[3 * i] = rays[i].origin.x; o[3 * i + 1] = rays[i].origin.y; o[3 * i + 2] = rays[i].origin.z;
            d[3 * i] = rays[i].dir.x; d[3 * i + 1] = rays[i].dir.y; d[3 * i + 2] = rays[i].dir.z;
        }
        out.resize(n_rays);
        if (rr_surface_rays(scene->handle(), o.data(), d.data(), (uint32_t)n_rays, depth, out.data()) != RR_OK) out.clear();
        return out;
    }
    // the same on DEVICE buffers, in stream order (rr_surface_rays_device): as trace_device below, with 128-byte records, 16-byte aligned
    int surface_device(const float* origins_dev, const float* dirs_dev, uint32_t n, uint32_t depth, rr_surface_hit* out_dev, void* hip_stream) const {
        return rr_surface_rays_device(scene->handle(), origins_dev, dirs_dev, n, depth, out_dev, hip_stream);
    }

    // The three ray queries on DEVICE buffers, in stream order (rr_trace_rays_device, rr_trace_shadow_rays_device, rr_shade_rays_device):
    // the pointers name memory the scene's device can address, in the layouts of the C ABI (3 floats per origin and direction, 20-byte
    // hit records, 32-byte radiance records); `hip_stream` is a hipStream_t (nullptr = the default stream).  The work is enqueued and
    // the call returns: synchronise the stream before reading the results on the host.  Each returns the rr_status (rr_last_error()
    // says why it is not RR_OK).  shade_device uses this handle's config, as shade_rays does.
    int trace_device(const float* origins_dev, const float* dirs_dev, uint32_t n, uint32_t depth, rr_ray_hit* out_dev, void* hip_stream) const {
        return rr_trace_rays_device(scene->handle(), origins_dev, dirs_dev, n, depth, out_dev, hip_stream);
    }
    int trace_shadow_device(const float* origins_dev, const float* dirs_dev, const float* max_distance_dev, uint32_t n, uint32_t depth,
                            rr_shadow_hit* out_dev, void* hip_stream) const {
        return rr_trace_shadow_rays_device(scene->handle(), origins_dev, dirs_dev, max_distance_dev, n, depth, out_dev, hip_stream);
    }
    int shade_device(const float* origins_dev, const float* dirs_dev, uint32_t n_results, uint32_t rays_per_result, const uint32_t* stream_ids_dev,
                     rr_radiance* out_dev, void* hip_stream, const volatile int* cancel = nullptr) const {
        const rr_config c = config.c_struct();
        return rr_shade_rays_device(scene->handle(), &c, origins_dev, dirs_dev, n_results, rays_per_result, stream_ids_dev, out_dev, hip_stream, cancel);
    }

    // The GUI's light and item edits (reference src/run.rs:1294-1409, :1464-1489), applied to the resident scene before the next
    // RendererManager::restart: `lights` is the edited Scene::lights, the flags are ShapeBasics::visible / flip_normals per item.
    // false = refused or failed (scene->error() says why); the scene then renders what it rendered before.
    bool update_lights(const std::vector<rr_light>& lights) { return scene->update_lights(lights) == RR_OK; }
    bool update_item_flags(const std::vector<uint8_t>& visible, const std::vector<uint8_t>& flip_normals) {
        return scene->update_item_flags(visible, flip_normals) == RR_OK;
    }

private:
    // The host form of a fused call (render_adaptive, render_adaptive_levels, render_adaptive_prefix): the frame's vectors sized and zeroed,
    // call(cam, config, out, rgba8, samples, error, level words) made, and every vector cleared if it fails.  level_pixels (or nullptr)
    // gets the first n_levels of the level words.
    template <class Call>
    std::vector<rr_radiance> fused_call(std::vector<uint16_t>* samples, std::vector<float>* error, std::vector<uint8_t>* rgba8, std::vector<uint32_t>* level_pixels,
                                        size_t n_levels, Call call) const {
        std::vector<rr_radiance> out;
        const rr_camera cam = camera.c_struct();
        const rr_config c = config.c_struct();
        const size_t n = (size_t)cam.width * cam.height;
        if (n == 0 || n > ((size_t)1 << 29)) return out;
        out.resize(n);
        if (samples) samples->assign(n, 0);
        if (error) error->assign(n, 0.0f);
        if (rgba8) rgba8->assign(4 * n, 0);
        std::vector<uint32_t> lp(n_levels > RR_MAX_ADAPTIVE_LEVELS ? n_levels : RR_MAX_ADAPTIVE_LEVELS, 0u);
        if (call(&cam, &c, out.data(), rgba8 ? rgba8->data() : nullptr, samples ? samples->data() : nullptr, error ? error->data() : nullptr, lp.data()) != RR_OK) {
            out.clear();
            if (samples) samples->clear();
            if (error) error->clear();
            if (rgba8) rgba8->clear();
            lp.clear();
        } else lp.resize(n_levels);
        if (level_pixels) *level_pixels = lp;
        return out;
    }
};

// reference src/renderer.rs:38-251
class RendererManager {
public:
    uint32_t thread_amount = 1; // one frame-level device call replaces the num_cpus - 2 workers (src/renderer.rs:67-71)
    uint32_t min_passes = 8;    // previews per frame (rr_render_progressive)

    RendererManager(int32_t width, int32_t height, std::shared_ptr<Raytracing> raytracing)
        : width_(width), height_(height), raytracing_(std::move(raytracing)) {}
    ~RendererManager() { stop(); join(); }

    void update_resolution(int32_t width, int32_t height) { width_ = width; height_ = height; } // :99-103

    // :105-172.  Returns at once; the frame renders on a worker thread.
    void start() {
        join();
        start_time_ = std::chrono::steady_clock::now();
        done_ms_ = 0;
        pixels_rendered_ = 0;
        cancel_ = 0;
        failed_ = false;
        running_ = true;
        const size_t n = (size_t)width_ * (size_t)height_;
        {
            std::lock_guard<std::mutex> lk(frame_mu_);
            image_.assign(n * 4, 0); normals_.assign(n * 3, 0.0f); depth_.assign(n, 0.0f); objects_.assign(n, 0u);
            fresh_ = false;
        }
        back_rgba_.assign(n * 4, 0); back_normal_.assign(n * 3, 0.0f); back_depth_.assign(n, 0.0f); back_ids_.assign(n, 0u);
        raytracing_->camera.init((uint32_t)width_, (uint32_t)height_);
        thread_ = std::thread([this]() { this->run(); });
    }

    // :174-198: ends the frame early; the buffers keep the last finished pass
    void stop() {
        if (!running_.exchange(false)) return;
        cancel_ = 1;
        join();
    }

    void restart(int32_t width, int32_t height) { stop(); update_resolution(width, height); start(); } // :201-208

    bool has_cells_left() const { return running_ && !is_done(); }                     // :210-213
    uint64_t get_rendered_pixels() const { return pixels_rendered_; }                  // :215-218
    bool is_running() const { return running_; }                                      // :220-226
    bool is_done() const { return pixels_rendered_ == (uint64_t)width_ * (uint64_t)height_; } // :228-231

    uint64_t check_and_get_elapsed_time() { // :233-246
        if (done_ms_ > 0) return done_ms_;
        const uint64_t ms = (uint64_t)std::chrono::duration_cast<std::chrono::milliseconds>(std::chrono::steady_clock::now() - start_time_).count();
        if (is_done()) done_ms_ = ms;
        return ms;
    }

    // Stands in for get_message_receiver (:248-251) + Run::apply_pixels (src/run.rs:506-545): calls `f` for every pixel
    // of the newest finished pass, once per pass.  Returns the number of pixels delivered.
    size_t drain(const std::function<void(const PixelData&)>& f) {
        std::lock_guard<std::mutex> lk(frame_mu_);
        if (!fresh_) return 0;
        fresh_ = false;
        const size_t n = (size_t)width_ * (size_t)height_;
        for (size_t i = 0; i < n; i++) {
            PixelData p;
            p.r = image_[4 * i]; p.g = image_[4 * i + 1]; p.b = image_[4 * i + 2];
            p.normal = Vec3{normals_[3 * i], normals_[3 * i + 1], normals_[3 * i + 2]};
            p.depth = depth_[i]; p.object_id = objects_[i];
            p.x = (int32_t)(i % (size_t)width_); p.y = (int32_t)(i / (size_t)width_);
            f(p);
        }
        return n;
    }

    // the four buffers Run::apply_pixels fills (src/run.rs:519-541); copies, safe while a frame renders
    void frame(std::vector<uint8_t>* rgba, std::vector<float>* normal = nullptr, std::vector<float>* depth = nullptr,
               std::vector<uint32_t>* object_id = nullptr) {
        std::lock_guard<std::mutex> lk(frame_mu_);
        if (rgba) *rgba = image_;
        if (normal) *normal = normals_;
        if (depth) *depth = depth_;
        if (object_id) *object_id = objects_;
    }

    // Run::post_processing (src/run.rs:588-600) -> run_post_processing (src/post_processing.rs:123-181) on the finished
    // frame: outline on object-id edges, then cavity shading from the normal buffer.  Returns the new image.
    std::vector<uint8_t> post_processing(bool cavity, bool outline, int device = 0) {
        std::vector<uint8_t> in; std::vector<float> nr; std::vector<uint32_t> ids;
        frame(&in, &nr, nullptr, &ids);
        std::vector<uint8_t> out(in.size());
        if (rr_post_process((uint32_t)width_, (uint32_t)height_, cavity ? 1 : 0, outline ? 1 : 0, in.data(), nr.data(), ids.data(), out.data(), device) != RR_OK) {
            std::lock_guard<std::mutex> lk(frame_mu_);
            error_ = rr_last_error();
            return in;
        }
        return out;
    }

    void wait() { join(); } // not in the reference: block until the frame is done or stopped
    bool failed() const { return failed_; }
    std::string last_error() { std::lock_guard<std::mutex> lk(frame_mu_); return error_; }
    uint32_t passes() const { return passes_; }

private:
    void join() { if (thread_.joinable()) thread_.join(); }

    static int on_pass(void* user, uint64_t done, uint64_t total) {
        RendererManager* m = (RendererManager*)user;
        m->publish();
        // the reference counts finished pixels; a pass finishes a share of every pixel's samples
        m->pixels_rendered_ = (uint64_t)m->width_ * (uint64_t)m->height_ * done / total;
        m->passes_++;
        return m->running_ ? 0 : 1;
    }

    void publish() {
        std::lock_guard<std::mutex> lk(frame_mu_);
        image_ = back_rgba_; normals_ = back_normal_; depth_ = back_depth_; objects_ = back_ids_;
        fresh_ = true;
    }

    void run() {
        passes_ = 0;
        const rr_camera cam = raytracing_->camera.c_struct();
        const rr_config cfg = raytracing_->config.c_struct();
        rr_frame out{back_rgba_.data(), back_normal_.data(), back_depth_.data(), back_ids_.data()};
        const int rc = rr_render_progressive(raytracing_->scene->handle(), &cam, &cfg, nullptr, &out, min_passes, &RendererManager::on_pass, this, &cancel_);
        if (rc == RR_OK) {
            publish();
            pixels_rendered_ = (uint64_t)width_ * (uint64_t)height_;
        } else if (rc != RR_ERR_CANCELLED) {
            std::lock_guard<std::mutex> lk(frame_mu_);
            error_ = rr_last_error();
            failed_ = true;
        }
        running_ = false;
    }

    int32_t width_, height_;
    std::shared_ptr<Raytracing> raytracing_;
    std::thread thread_;
    std::atomic<bool> running_{false}, failed_{false};
    std::atomic<uint64_t> pixels_rendered_{0};
    std::atomic<uint32_t> passes_{0};
    volatile int cancel_ = 0;
    std::chrono::steady_clock::time_point start_time_ = std::chrono::steady_clock::now();
    uint64_t done_ms_ = 0;
    std::mutex frame_mu_;
    std::vector<uint8_t> image_, back_rgba_;
    std::vector<float> normals_, depth_, back_normal_, back_depth_;
    std::vector<uint32_t> objects_, back_ids_;
    bool fresh_ = false;
    std::string error_;
};

} // namespace rustray
