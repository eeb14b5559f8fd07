// rusty_marcher.hpp -- C++ host-side mirror of the reference's module surface
// (engine/src/{geometry,shapes,sphere,polygon,lights,obj,scene,framebuffer,renderer}.rs)
// over the C ABI of include/rusty_marcher_amd.h.  Header-only; link with
// librusty_marcher_amd.so.  Same names, argument order and failure behaviour as the
// Rust code: where the reference panics this throws rusty_marcher::Panic.
//
// The reference's toolchain (rustc/cargo) is absent from the build image, so this is the
// compiled-language host layer; the Rust shim a maintainer adds is in INTEGRATION.md.
#ifndef RUSTY_MARCHER_HPP
#define RUSTY_MARCHER_HPP

#include <chrono>
#include <cstdint>
#include <cstdio>
#include <fstream>
#include <memory>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "rusty_marcher_amd.h"

namespace rusty_marcher {

struct Panic : std::runtime_error {
    rm_status status;
    Panic(rm_status st, const std::string &what) : std::runtime_error(what), status(st) {}
};

inline void check(rm_status st, const rm_ctx *ctx = nullptr) {
    if (st != RM_OK) throw Panic(st, rm_last_error(ctx));
}

// ---- geometry.rs ----------------------------------------------------------------
namespace geometry {
struct Vec3f {
    double x = 0., y = 0., z = 0.;
    static Vec3f zero() { return {0., 0., 0.}; }
    static Vec3f ones() { return {1., 1., 1.}; }
    Vec3f operator+(Vec3f o) const { return {x + o.x, y + o.y, z + o.z}; }
    Vec3f operator-(Vec3f o) const { return {x - o.x, y - o.y, z - o.z}; }
    Vec3f scaled(double s) const { return {x * s, y * s, z * s}; }
    rm_vec3 c() const { return rm_vec3{x, y, z}; }
};
}  // namespace geometry
using geometry::Vec3f;

// ---- shapes.rs --------------------------------------------------------------------
namespace shapes {
struct Reflectance {
    double diffusion, specular, specular_exponent, reflection, refractive_index;
    Vec3f diffuse_color;
    bool is_glass_like;
    static Reflectance create_default() {             // shapes.rs:49-61
        rm_reflectance r;
        rm_reflectance_default(&r);
        return from_c(r);
    }
    static Reflectance from_c(const rm_reflectance &r) {
        return {r.diffusion, r.specular, r.specular_exponent, r.reflection, r.refractive_index,
                Vec3f{r.diffuse_color.x, r.diffuse_color.y, r.diffuse_color.z}, r.is_glass_like != 0};
    }
    rm_reflectance c() const {
        return rm_reflectance{diffusion, diffuse_color.c(), specular, specular_exponent, is_glass_like ? 1 : 0, 0,
                              reflection, refractive_index};
    }
};

// `trait Shape` (shapes.rs:40-47): what a shape must be able to do here is add itself to
// the flat scene, in list order.
struct Shape {
    virtual ~Shape() = default;
    virtual void describe(rm_scene *scene, uint32_t index) const = 0;
};
}  // namespace shapes
using shapes::Reflectance;

// ---- sphere.rs ----------------------------------------------------------------------
namespace sphere {
struct Sphere : shapes::Shape {
    Vec3f center;
    double radius;
    Reflectance reflectance;
    Sphere(Vec3f c, double r, Reflectance m) : center(c), radius(r), reflectance(m) {}
    void describe(rm_scene *scene, uint32_t) const override {
        const rm_reflectance r = reflectance.c();
        check(rm_scene_add_sphere(scene, center.c(), radius, &r));
    }
};
inline std::unique_ptr<Sphere> create(Vec3f center, double radius, Reflectance r) {   // sphere.rs:13-24
    return std::unique_ptr<Sphere>(new Sphere(center, radius, r));
}
}  // namespace sphere

// ---- polygon.rs ---------------------------------------------------------------------
namespace polygon {
struct ConvexPolygon : shapes::Shape {
    std::vector<Vec3f> vertices;
    Reflectance reflectance;
    std::vector<Vec3f> offsets;
    static std::unique_ptr<ConvexPolygon> create(std::vector<Vec3f> v, Reflectance r) {   // polygon.rs:16-42
        if (v.size() <= 2) throw Panic(RM_ERR_INVALID_ARG, "assertion failed: vertices.len() > 2");
        std::unique_ptr<ConvexPolygon> p(new ConvexPolygon());
        p->vertices = std::move(v);
        p->reflectance = r;
        return p;
    }
    void offset(Vec3f off) { offsets.push_back(off); }                                   // polygon.rs:44-49
    void describe(rm_scene *scene, uint32_t index) const override {
        std::vector<rm_vec3> v;
        for (const auto &p : vertices) v.push_back(p.c());
        const rm_reflectance r = reflectance.c();
        check(rm_scene_add_polygon(scene, v.data(), (uint32_t)v.size(), &r));
        for (const auto &o : offsets) check(rm_scene_offset_shape(scene, index, o.c()));
    }

  private:
    ConvexPolygon() : reflectance(Reflectance::create_default()) {}
};
}  // namespace polygon

// ---- lights.rs ------------------------------------------------------------------------
namespace lights {
struct Light {
    Vec3f position, color;
    double intensity;
};
inline Light create_light(Vec3f position, Vec3f color, double intensity) {   // lights.rs:10-16
    return Light{position, color, intensity};                               // L-inf normalised inside the library
}
}  // namespace lights

// ---- obj.rs ---------------------------------------------------------------------------
namespace obj {
struct Obj : shapes::Shape {
    std::vector<double> tri_xyz;   // 9 per triangle, f32 positions widened (obj.rs:103-105)
    std::vector<Vec3f> offsets;
    void offset(Vec3f off) { offsets.push_back(off); }                                    // obj.rs:24-29
    void describe(rm_scene *scene, uint32_t index) const override {
        check(rm_scene_add_mesh(scene, tri_xyz.data(), (uint32_t)(tri_xyz.size() / 9), rm_vec3{0., 0., 0.}));
        for (const auto &o : offsets) check(rm_scene_offset_shape(scene, index, o.c()));
    }
};

// obj.rs:44-151: `Some(Vec<Obj>)`; `ok == false` when the file cannot be read (obj.rs:53-56).
inline std::vector<std::unique_ptr<Obj>> load(const std::string &path, bool *ok = nullptr) {
    std::vector<std::unique_ptr<Obj>> out;
    rm_scene *s = nullptr;
    check(rm_scene_new(&s));
    uint32_t n = 0;
    const rm_status st = rm_scene_load_obj(s, path.c_str(), rm_vec3{0., 0., 0.}, &n);
    if (st == RM_ERR_IO && std::string(rm_last_error(nullptr)).rfind("Could not load obj", 0) == 0) {
        std::printf("Could not load obj from %s\n", path.c_str());
        rm_scene_free(s);
        if (ok) *ok = false;
        return out;
    }
    if (st != RM_OK) { rm_scene_free(s); check(st); }
    rm_scene_desc d;
    check(rm_scene_get_desc(s, &d));
    for (uint32_t i = 0; i < d.n_shapes; i++) {
        std::unique_ptr<Obj> o(new Obj());
        for (uint32_t t = 0; t < d.shapes[i].count; t++)
            for (const rm_vec3 &v : d.triangles[d.shapes[i].first + t].vertices) {
                o->tri_xyz.push_back(v.x); o->tri_xyz.push_back(v.y); o->tri_xyz.push_back(v.z);
            }
        out.push_back(std::move(o));
    }
    rm_scene_free(s);
    if (ok) *ok = true;
    return out;
}
}  // namespace obj

// ---- scene.rs -------------------------------------------------------------------------
namespace scene {
struct Scene {
    std::vector<lights::Light> lights;
    std::vector<std::unique_ptr<shapes::Shape>> shapes;   // Vec<Box<dyn Shape + Sync>>
    Vec3f camera;

    static Scene make() { return Scene(); }                                               // Scene::new, scene.rs:16-23
    void offset_camera(Vec3f off) { camera = camera + off; }                              // scene.rs:25-27

    static Scene create_default() {                                                       // scene.rs:28-211
        Scene s;
        check(rm_scene_create_default(&s.prebuilt_));
        s.adopt();
        return s;
    }
    static Scene open_obj(const std::string &path) {                                      // main.rs:261-327
        Scene s;
        check(rm_scene_open_obj(path.c_str(), &s.prebuilt_));
        s.adopt();
        return s;
    }

    Scene() = default;
    Scene(Scene &&o) noexcept { *this = std::move(o); }
    Scene &operator=(Scene &&o) noexcept {
        lights = std::move(o.lights); shapes = std::move(o.shapes); camera = o.camera;
        std::swap(prebuilt_, o.prebuilt_);
        return *this;
    }
    ~Scene() { rm_scene_free(prebuilt_); }

    // Flat form for upload; the caller frees it unless it is the library-built scene.
    rm_scene *flatten(bool *owned) const {
        if (prebuilt_ && shapes.empty()) {                  // library-built, shapes untouched
            check(rm_scene_set_camera(prebuilt_, camera.c()));
            *owned = false;
            return prebuilt_;
        }
        rm_scene *s = nullptr;
        check(rm_scene_new(&s));
        uint32_t i = 0;
        for (const auto &sh : shapes) sh->describe(s, i++);
        for (const auto &l : lights) check(rm_scene_add_light(s, l.position.c(), l.color.c(), l.intensity));
        check(rm_scene_set_camera(s, camera.c()));
        *owned = true;
        return s;
    }

  private:
    rm_scene *prebuilt_ = nullptr;
    void adopt() {
        rm_scene_desc d;
        check(rm_scene_get_desc(prebuilt_, &d));
        camera = Vec3f{d.camera.x, d.camera.y, d.camera.z};
        for (uint32_t i = 0; i < d.n_lights; i++)
            lights.push_back({Vec3f{d.lights[i].position.x, d.lights[i].position.y, d.lights[i].position.z},
                              Vec3f{d.lights[i].color.x, d.lights[i].color.y, d.lights[i].color.z}, d.lights[i].intensity});
    }
};
}  // namespace scene

// ---- framebuffer.rs ---------------------------------------------------------------------
namespace framebuffer {
// framebuffer.rs:6-10: `buffer: Vec<Vec<geometry::Vec3f>>` -- one heap allocation per scan line.
// Vec3f is three doubles, x y z in that order (the `#[repr(C)]` the shim asks of geometry.rs:4-8).
static_assert(sizeof(Vec3f) == 3 * sizeof(double), "Vec3f must be three packed doubles");
struct FrameBuffer {
    size_t width, height;
    std::vector<std::vector<Vec3f>> buffer;   // [height] rows of [width] pixels
    // what rm_render_rows / rm_fetch_rows take: one pointer per scan line
    // (width, height and buffer are public, as in the reference: a frame whose fields disagree is refused here -- the
    // library writes width * 3 doubles into each of height rows)
    std::vector<double *> row_pointers() {
        if (buffer.size() < height) throw std::runtime_error("FrameBuffer: fewer rows than its height");
        std::vector<double *> rows(height);
        for (size_t y = 0; y < height; y++) {
            if (buffer[y].size() != width) throw std::runtime_error("FrameBuffer: a row that is not `width` pixels long");
            rows[y] = reinterpret_cast<double *>(buffer[y].data());
        }
        return rows;
    }
    static uint8_t quantize(double f) {                                   // framebuffer.rs:80-82
        const double c = f > 0. ? (f < 1. ? f : 1.) : 0.;                 // f.max(0.).min(1.): NaN -> 0
        return (uint8_t)(255. * c);
    }
    std::vector<uint8_t> to_vec() const {                                 // framebuffer.rs:40-55
        std::vector<uint8_t> out(width * height * 3);
        size_t k = 0;
        for (size_t i = 0; i < height; i++)
            for (size_t j = 0; j < width; j++) {
                out[k++] = quantize(buffer[i][j].x); out[k++] = quantize(buffer[i][j].y); out[k++] = quantize(buffer[i][j].z);
            }
        return out;
    }
    void normalize() {                                                    // framebuffer.rs:58-77
        double mx = 0., my = 0., mz = 0.;
        auto fmax = [](double a, double b) { return b > a ? b : a; };     // f64::max: NaN loses
        for (const auto &row : buffer)
            for (const Vec3f &p : row) { mx = fmax(mx, p.x); my = fmax(my, p.y); mz = fmax(mz, p.z); }
        const double max_val = fmax(fmax(mx, my), mz);
        if (max_val > 0.) {
            const double s = 1. / max_val;
            for (auto &row : buffer)
                for (Vec3f &p : row) p = p.scaled(s);
        }
    }
    void write_ppm(const std::string &filename) const {                   // framebuffer.rs:26-38
        std::ofstream f(filename, std::ios::binary);
        f << "P6\n" << width << " " << height << "\n255\n";
        const std::vector<uint8_t> rgb = to_vec();
        f.write(reinterpret_cast<const char *>(rgb.data()), (std::streamsize)rgb.size());
    }
};
inline FrameBuffer create_frame_buffer(size_t width, size_t height) {     // framebuffer.rs:12-22
    return FrameBuffer{width, height, std::vector<std::vector<Vec3f>>(height, std::vector<Vec3f>(width, Vec3f::zero()))};
}
}  // namespace framebuffer

// ---- renderer.rs --------------------------------------------------------------------------
namespace renderer {
struct Renderer {
    double fov, half_fov, height, width, ratio;
    uint32_t max_depth = 3;        // renderer.rs:262, exposed
    uint32_t flags = RM_FLAG_NONE;
    rm_timing last_timing{};
    uint32_t last_refined = 0;     // render_antialiased: pixels it refined
    uint32_t last_samples = 0;     // render_progressive: samples a pixel in its frame
    rm_converge_report last_report{};   // render_converging: the last tick's report

    ~Renderer() { rm_destroy(ctx_); }
    Renderer(const Renderer &) = delete;
    Renderer(Renderer &&o) noexcept : fov(o.fov), half_fov(o.half_fov), height(o.height), width(o.width), ratio(o.ratio),
                                      max_depth(o.max_depth), flags(o.flags), ctx_(o.ctx_) { o.ctx_ = nullptr; }
    Renderer(double fov_, double height_, double width_) {
        rm_params p;
        rm_create_renderer(fov_, height_, width_, &p);
        fov = p.fov; half_fov = p.half_fov; height = p.height; width = p.width; ratio = p.ratio;
    }

    // renderer.rs:36-126: synchronous, fills `frame` -- rows of rows, like the reference's -- and
    // returns the status string
    std::string render(framebuffer::FrameBuffer &frame, const scene::Scene &sc) {
        const auto t0 = std::chrono::steady_clock::now();
        const rm_params p = prepare(frame.width, frame.height, sc);
        std::vector<double *> rows = frame.row_pointers();
        check(rm_render_rows(ctx_, &p, rows.data(), &last_timing), ctx_);
        return status(t0, frame.width, frame.height);
    }
    // The same call with a device-resident FrameBuffer: the f64 frame stays on the device, what
    // comes back is `fb.to_vec()` -- the bytes the window blits (main.rs:337-346) -- into `rgb8`
    // (width * height * 3; rows below the last whole patch row keep their contents).
    std::string render_display(size_t width, size_t height, const scene::Scene &sc, std::vector<uint8_t> &rgb8) {
        const auto t0 = std::chrono::steady_clock::now();
        const rm_params p = prepare(width, height, sc);
        rgb8.resize(width * height * 3);
        check(rm_render_display(ctx_, &p, rgb8.data(), &last_timing), ctx_);
        return status(t0, width, height);
    }
    // f64 rows of the device-resident frame on demand (save_to_file: normalize + write_ppm)
    void fetch(framebuffer::FrameBuffer &frame) {
        std::vector<double *> rows = frame.row_pointers();
        // (refused with RM_ERR_INVALID_ARG when the frame on the device is of another size: a window resized since)
        check(rm_fetch_rows(context(), rows.data(), (uint32_t)frame.width, (uint32_t)frame.height, 0, 0), ctx_);
    }
    // What render(frame, sc) shows at pixel (x = column, y = row) of a width x height frame: the closest hit of the ray
    // renderer.rs:80 casts there (rm_pick) -- hit.shape indexes sc.shapes; hit.hit == 0 where the ray leaves the scene.
    rm_hit pick(size_t width_px, size_t height_px, const scene::Scene &sc, uint32_t x, uint32_t y) {
        const rm_params p = prepare(width_px, height_px, sc, false);
        rm_hit hit;
        check(rm_pick(ctx_, &p, x, y, &hit), ctx_);
        return hit;
    }
    // Can a see b in sc (rm_visible_segments)?  Nothing may lie on the segment between `skin` and its length less `skin`: the
    // guard against the surfaces the two points lie on (the render's own is 1e-3).
    bool visible(const scene::Scene &sc, Vec3f a, Vec3f b, double skin = 0.) {
        upload(sc);
        const rm_vec3 from = a.c(), to = b.c();
        uint8_t seen = 0;
        check(rm_visible_segments(ctx_, &from, &to, 1, skin, &seen), ctx_);
        return seen != 0;
    }
    // Which of sc.lights reach the surface point `point` with normal `normal` -- a pick's (rm_lights_visible).  clipped false:
    // the decision direct_lighting takes (renderer.rs:166-174), a shape behind the light shadows; true: the ray ends at the light.
    std::vector<bool> lit_by(const scene::Scene &sc, Vec3f point, Vec3f normal, bool clipped = false) {
        upload(sc);
        const rm_vec3 p = point.c(), n = normal.c();
        std::vector<uint8_t> lit(sc.lights.size());
        check(rm_lights_visible(ctx_, &p, &n, 1, (uint32_t)lit.size(), clipped ? RM_LIGHTS_CLIPPED : RM_LIGHTS_AS_RENDERED, lit.data()), ctx_);
        return std::vector<bool>(lit.begin(), lit.end());
    }
    // What comes back along rays of the caller's own in sc (rm_radiance_rays): cast_ray (renderer.rs:254-309) with this
    // Renderer's max_depth and the render's background, one colour per ray.  Directions are unit vectors; a ray that leaves
    // the scene returns zero, as a primary ray of the render does.
    std::vector<Vec3f> radiance(const scene::Scene &sc, const std::vector<Vec3f> &origins, const std::vector<Vec3f> &directions) {
        if (origins.size() != directions.size()) throw std::invalid_argument("radiance: origins and directions differ in length");
        upload(sc);
        std::vector<rm_vec3> o(origins.size()), d(origins.size()), rgb(origins.size());
        for (size_t i = 0; i < origins.size(); i++) { o[i] = origins[i].c(); d[i] = directions[i].c(); }
        const rm_shading shading{rm_vec3{0.1, 0.1, 0.1}, max_depth, 0u};                  // renderer.rs:40-44
        check(rm_radiance_rays(ctx_, o.data(), d.data(), (uint32_t)o.size(), &shading, rgb.data()), ctx_);
        std::vector<Vec3f> out(rgb.size());
        for (size_t i = 0; i < rgb.size(); i++) out[i] = Vec3f{rgb[i].x, rgb[i].y, rgb[i].z};
        return out;
    }
    // The radiance at real-valued positions (sx = column, sy = row; xy holds the pairs back to back) of the width x height
    // frame render() would draw (rm_radiance_samples): sub-pixel samples; integer positions are the render's own pixels.
    std::vector<Vec3f> radiance_samples(size_t width_px, size_t height_px, const scene::Scene &sc, const std::vector<double> &xy) {
        const rm_params p = prepare(width_px, height_px, sc, false);
        std::vector<rm_vec3> rgb(xy.size() / 2);
        check(rm_radiance_samples(ctx_, &p, xy.data(), (uint32_t)rgb.size(), rgb.data()), ctx_);
        std::vector<Vec3f> out(rgb.size());
        for (size_t i = 0; i < rgb.size(); i++) out[i] = Vec3f{rgb[i].x, rgb[i].y, rgb[i].z};
        return out;
    }
    // render() with adaptive anti-aliasing (rm_render_antialiased): rendered once, then every pixel that differs from a
    // neighbour by more than `threshold` in a channel is replaced by the mean of n x n radiance samples (n in 1..8), found,
    // shaded and resolved on the device.  Fills the whole patch rows of `frame`; the pixels refined are left in last_refined.
    std::string render_antialiased(framebuffer::FrameBuffer &frame, const scene::Scene &sc, uint32_t n, double threshold) {
        const auto t0 = std::chrono::steady_clock::now();
        const rm_params p = prepare(frame.width, frame.height, sc);
        const rm_refine refine{n, 0u, threshold};
        const size_t rows = frame.height - frame.height % 32;
        std::vector<double> flat(rows * frame.width * 3);
        check(rm_render_antialiased(ctx_, &p, &refine, flat.data(), &last_refined, &last_timing), ctx_);
        for (size_t y = 0; y < rows; y++)
            for (size_t x = 0; x < frame.width; x++) {
                const double *c = &flat[(y * frame.width + x) * 3];
                frame.buffer[y][x] = Vec3f{c[0], c[1], c[2]};
            }
        return status(t0, frame.width, frame.height);
    }
    // render() through a thin lens (rm_render_lens): n_samples rays a pixel (1..64), each from a point of its own of a lens of
    // radius `aperture` towards the point its sample ray reaches at the distance `focus` along the view direction.  The sample
    // table is the library's (rm_lens_table); sampled, shaded and averaged on the device.  Fills the whole patch rows of `frame`.
    std::string render_lens(framebuffer::FrameBuffer &frame, const scene::Scene &sc, double aperture, double focus, uint32_t n_samples) {
        const auto t0 = std::chrono::steady_clock::now();
        const rm_params p = prepare(frame.width, frame.height, sc);
        const rm_lens lens{aperture, focus, n_samples, 0u};
        std::vector<double> table(4 * 64);                                                  // (room for the most rows there can be)
        check(rm_lens_table(n_samples, table.data()));
        const size_t rows = frame.height - frame.height % 32;
        std::vector<double> flat(rows * frame.width * 3 + 1);                              // (+ 1: never a NULL frame)
        check(rm_render_lens(ctx_, &p, &lens, table.data(), flat.data(), &last_timing), ctx_);
        for (size_t y = 0; y < rows; y++)
            for (size_t x = 0; x < frame.width; x++) {
                const double *c = &flat[(y * frame.width + x) * 3];
                frame.buffer[y][x] = Vec3f{c[0], c[1], c[2]};
            }
        return status(t0, frame.width, frame.height);
    }
    // A tick of a standing view (rm_render_progressive): n_samples (1..64) more lens samples a pixel of the library's unbounded
    // sequence are added on the device to the frame the context keeps, and `frame` gets the mean of all of them so far.  The
    // frame begins again when `restart` is set or anything it depends on changed since the last tick (renderer, frame size, lens,
    // camera, view direction, scene).  Fills the whole patch rows of `frame`; the samples a pixel in it are left in last_samples
    // (at most RM_PROGRESSIVE_MAX_SAMPLES: further ticks change nothing).
    std::string render_progressive(framebuffer::FrameBuffer &frame, const scene::Scene &sc, double aperture, double focus, uint32_t n_samples,
                                   bool restart = false) {
        const auto t0 = std::chrono::steady_clock::now();
        const rm_params p = prepare(frame.width, frame.height, sc);
        const rm_lens lens{aperture, focus, n_samples, 0u};
        const size_t rows = frame.height - frame.height % 32;
        std::vector<double> flat(rows * frame.width * 3 + 1);                              // (+ 1: never a NULL frame)
        check(rm_render_progressive(ctx_, &p, &lens, restart ? 1 : 0, flat.data(), nullptr, &last_samples, &last_timing), ctx_);
        for (size_t y = 0; y < rows; y++)
            for (size_t x = 0; x < frame.width; x++) {
                const double *c = &flat[(y * frame.width + x) * 3];
                frame.buffer[y][x] = Vec3f{c[0], c[1], c[2]};
            }
        return status(t0, frame.width, frame.height);
    }
    // render_progressive with area lights (rm_render_progressive_soft): light l of the scene is a sphere of radius radii[l] -- one
    // radius a light, 0 for a point -- sampled at another point for every sample, so the frame converges to soft shadows.  Beyond
    // what begins a frame again in render_progressive, a changed radius does, and so does a switch between the two calls.
    std::string render_progressive_soft(framebuffer::FrameBuffer &frame, const scene::Scene &sc, const std::vector<double> &radii, double aperture,
                                        double focus, uint32_t n_samples, bool restart = false) {
        const auto t0 = std::chrono::steady_clock::now();
        const rm_params p = prepare(frame.width, frame.height, sc);
        const rm_lens lens{aperture, focus, n_samples, 0u};
        const size_t rows = frame.height - frame.height % 32;
        std::vector<double> flat(rows * frame.width * 3 + 1);                              // (+ 1: never a NULL frame)
        check(rm_render_progressive_soft(ctx_, &p, &lens, radii.data(), (uint32_t)radii.size(), restart ? 1 : 0, flat.data(), nullptr,
                                         &last_samples, &last_timing),
              ctx_);
        for (size_t y = 0; y < rows; y++)
            for (size_t x = 0; x < frame.width; x++) {
                const double *c = &flat[(y * frame.width + x) * 3];
                frame.buffer[y][x] = Vec3f{c[0], c[1], c[2]};
            }
        return status(t0, frame.width, frame.height);
    }
    // render_progressive_soft with moving spheres (rm_render_progressive_motion): shape k of the scene, a sphere, moves by
    // velocities[k] -- one vector a shape, zero for what is not a sphere -- while the shutter stands open for `shutter`, and every
    // sample sees it at a time of its own, so the frame converges to a picture blurred along the motion.  radii: one radius a light;
    // empty: point lights.  Beyond what begins a frame again in render_progressive_soft, a changed velocity or shutter does, and so
    // does a switch between the calls.  Every ray of such a frame tests every primitive: a hierarchy holds for spheres that stand still.
    std::string render_progressive_motion(framebuffer::FrameBuffer &frame, const scene::Scene &sc, const std::vector<Vec3f> &velocities,
                                          double shutter, uint32_t n_samples, const std::vector<double> &radii = {}, double aperture = 0.,
                                          double focus = 1., bool restart = false) {
        return tick_with_velocities(false, frame, sc, velocities, shutter, n_samples, radii, aperture, focus, restart);
    }
    // render_progressive_motion in which every shape moves (rm_render_progressive_moving): a velocity on a polygon or a mesh is
    // obeyed -- the plane point and the vertices, every triangle's centre and vertices move as the reference's offset() moves them,
    // the normals stay.  The frame is not render_progressive_motion's: a switch between the two begins it again.
    std::string render_progressive_moving(framebuffer::FrameBuffer &frame, const scene::Scene &sc, const std::vector<Vec3f> &velocities,
                                          double shutter, uint32_t n_samples, const std::vector<double> &radii = {}, double aperture = 0.,
                                          double focus = 1., bool restart = false) {
        return tick_with_velocities(true, frame, sc, velocities, shutter, n_samples, radii, aperture, focus, restart);
    }
    // A swept hierarchy of the uploaded scene (rm_swept_build): its hierarchies' boxes refitted to bound every primitive at every
    // offset within lo[k] .. hi[k] of its shape k (three numbers a shape each).  render_progressive_moving and
    // render_converging_moving build their own from the velocities; this one serves a host that drives the device calls itself
    // (accumulate_swept_device below).  Stale once another scene is uploaded; hand it back with swept_free.
    rm_swept *swept(const std::vector<double> &lo, const std::vector<double> &hi) {
        if (lo.size() != hi.size() || lo.size() % 3 != 0) throw std::invalid_argument("swept: lo and hi hold three numbers a shape");
        rm_swept *out = nullptr;
        check(rm_swept_build(ctx_, lo.data(), hi.data(), (uint32_t)(lo.size() / 3), &out), ctx_);
        return out;
    }
    void swept_free(rm_swept *s) { rm_swept_free(ctx_, s); }
    // rm_accumulate_swept_device: rm_accumulate_moving_device through `s`, whose extents hold every row of the shape table; device
    // pointers and the stream are the caller's
    void accumulate_swept_device(const rm_params &p, const rm_lens &lens, const void *device_table, const void *device_light_offsets,
                                 uint32_t n_lights, const void *device_shape_offsets, uint32_t n_shapes, const rm_swept *s, uint32_t n_before,
                                 void *device_sum, void *device_mean, void *device_rgb8, void *hip_stream) {
        check(rm_accumulate_swept_device(ctx_, &p, &lens, device_table, device_light_offsets, n_lights, device_shape_offsets, n_shapes, s, n_before,
                                         device_sum, device_mean, device_rgb8, hip_stream),
              ctx_);
    }
    // ... and rm_accumulate_converging_swept_device, likewise
    void accumulate_converging_swept_device(const rm_params &p, const rm_lens &lens, const rm_converge &converge, const void *device_table,
                                            uint32_t table_rows, const void *device_light_offsets, uint32_t n_lights,
                                            const void *device_shape_offsets, uint32_t n_shapes, const rm_swept *s, bool fresh,
                                            const rm_converge_frame &buffers, void *hip_stream) {
        check(rm_accumulate_converging_swept_device(ctx_, &p, &lens, &converge, device_table, table_rows, device_light_offsets, n_lights,
                                                    device_shape_offsets, n_shapes, s, fresh ? 1 : 0, &buffers, hip_stream),
              ctx_);
    }
    // rm_accumulate_camera_swept_device: rm_accumulate_camera_device with a shape table through `s` (a handle of swept(); the boxes
    // are in world space, so no camera row matters).  A NULL shape table is refused: the flat call keeps the hierarchy then.
    void accumulate_camera_swept_device(const rm_params &p, const rm_lens &lens, const void *device_table, const void *device_camera_rows,
                                        const void *device_light_offsets, uint32_t n_lights, const void *device_shape_offsets, uint32_t n_shapes,
                                        const rm_swept *s, uint32_t n_before, void *device_sum, void *device_mean, void *device_rgb8,
                                        void *hip_stream) {
        check(rm_accumulate_camera_swept_device(ctx_, &p, &lens, device_table, device_camera_rows, device_light_offsets, n_lights,
                                                device_shape_offsets, n_shapes, s, n_before, device_sum, device_mean, device_rgb8, hip_stream),
              ctx_);
    }
    // ... and rm_accumulate_converging_camera_swept_device, likewise
    void accumulate_converging_camera_swept_device(const rm_params &p, const rm_lens &lens, const rm_converge &converge, const void *device_table,
                                                   uint32_t table_rows, const void *device_camera_rows, const void *device_light_offsets,
                                                   uint32_t n_lights, const void *device_shape_offsets, uint32_t n_shapes, const rm_swept *s,
                                                   bool fresh, const rm_converge_frame &buffers, void *hip_stream) {
        check(rm_accumulate_converging_camera_swept_device(ctx_, &p, &lens, &converge, device_table, table_rows, device_camera_rows,
                                                           device_light_offsets, n_lights, device_shape_offsets, n_shapes, s, fresh ? 1 : 0,
                                                           &buffers, hip_stream),
              ctx_);
    }
    // rm_swept_tick_info: whether the last sampled-frame tick's launch walked a swept hierarchy, and how many the ticks have built
    rm_swept_tick_report swept_tick_info() {
        rm_swept_tick_report out{};
        check(rm_swept_tick_info(ctx_, &out), ctx_);
        return out;
    }
    // The tick of the two calls above; any_shape: the second
    std::string tick_with_velocities(bool any_shape, framebuffer::FrameBuffer &frame, const scene::Scene &sc,
                                     const std::vector<Vec3f> &velocities, double shutter, uint32_t n_samples, const std::vector<double> &radii,
                                     double aperture, double focus, bool restart) {
        const auto t0 = std::chrono::steady_clock::now();
        const rm_params p = prepare(frame.width, frame.height, sc);
        const rm_lens lens{aperture, focus, n_samples, 0u};
        const size_t rows = frame.height - frame.height % 32;
        std::vector<double> flat(rows * frame.width * 3 + 1);                              // (+ 1: never a NULL frame)
        std::vector<rm_vec3> v;
        for (const Vec3f &e : velocities) v.push_back(e.c());
        const double *r = radii.empty() ? nullptr : radii.data();
        check(any_shape ? rm_render_progressive_moving(ctx_, &p, &lens, r, (uint32_t)radii.size(), v.data(), (uint32_t)v.size(), shutter,
                                                       restart ? 1 : 0, flat.data(), nullptr, &last_samples, &last_timing)
                        : rm_render_progressive_motion(ctx_, &p, &lens, r, (uint32_t)radii.size(), v.data(), (uint32_t)v.size(), shutter,
                                                       restart ? 1 : 0, flat.data(), nullptr, &last_samples, &last_timing),
              ctx_);
        for (size_t y = 0; y < rows; y++)
            for (size_t x = 0; x < frame.width; x++) {
                const double *c = &flat[(y * frame.width + x) * 3];
                frame.buffer[y][x] = Vec3f{c[0], c[1], c[2]};
            }
        return status(t0, frame.width, frame.height);
    }
    // A tick of a converging frame (rm_render_converging): render_progressive -- with area lights where `radii` holds one radius a
    // light; empty: point lights -- that casts its n_samples more samples only for the pixels still noisy and their neighbours.  A
    // pixel is settled once it has converge.min_samples samples and the standard error of the mean of r + g + b is at most
    // converge.tolerance; none gets more than converge.max_samples.  The frame is the context's own for this call
    // (render_progressive's is left alone) and begins again as render_progressive_soft's does.  Returns the tick's report, also left
    // in last_report: listed == 0 says the picture is finished, and further ticks change nothing.
    rm_converge_report render_converging(framebuffer::FrameBuffer &frame, const scene::Scene &sc, const rm_converge &converge, uint32_t n_samples,
                                         const std::vector<double> &radii = {}, double aperture = 0., double focus = 1., bool restart = false) {
        const rm_params p = prepare(frame.width, frame.height, sc);
        const rm_lens lens{aperture, focus, n_samples, 0u};
        const size_t rows = frame.height - frame.height % 32;
        std::vector<double> flat(rows * frame.width * 3 + 1);                              // (+ 1: never a NULL frame)
        check(rm_render_converging(ctx_, &p, &lens, &converge, radii.empty() ? nullptr : radii.data(), (uint32_t)radii.size(), restart ? 1 : 0,
                                   flat.data(), nullptr, &last_report, &last_timing),
              ctx_);
        last_samples = last_report.max_count;
        for (size_t y = 0; y < rows; y++)
            for (size_t x = 0; x < frame.width; x++) {
                const double *c = &flat[(y * frame.width + x) * 3];
                frame.buffer[y][x] = Vec3f{c[0], c[1], c[2]};
            }
        return last_report;
    }
    // render_progressive_soft with one bounce of diffuse light (rm_render_progressive_bounce): where a sample first hits a surface
    // that is not glass, one more ray leaves it in a cosine-distributed direction, and what it brings back, times `strength` and the
    // surface's diffusion and diffuse colour, is added.  radii: one radius a light; empty: point lights.  Static scene, standing
    // camera.  Beyond what begins a frame again in render_progressive_soft, a changed strength does, and so does a switch between
    // the calls.
    std::string render_progressive_bounce(framebuffer::FrameBuffer &frame, const scene::Scene &sc, uint32_t n_samples, double strength = 1.,
                                          const std::vector<double> &radii = {}, double aperture = 0., double focus = 1., bool restart = false) {
        const auto t0 = std::chrono::steady_clock::now();
        const rm_params p = prepare(frame.width, frame.height, sc);
        const rm_lens lens{aperture, focus, n_samples, 0u};
        const size_t rows = frame.height - frame.height % 32;
        std::vector<double> flat(rows * frame.width * 3 + 1);                              // (+ 1: never a NULL frame)
        check(rm_render_progressive_bounce(ctx_, &p, &lens, radii.empty() ? nullptr : radii.data(), (uint32_t)radii.size(), strength,
                                           restart ? 1 : 0, flat.data(), nullptr, &last_samples, &last_timing),
              ctx_);
        for (size_t y = 0; y < rows; y++)
            for (size_t x = 0; x < frame.width; x++) {
                const double *c = &flat[(y * frame.width + x) * 3];
                frame.buffer[y][x] = Vec3f{c[0], c[1], c[2]};
            }
        return status(t0, frame.width, frame.height);
    }
    // render_converging with one bounce of diffuse light (rm_render_converging_bounce), as render_progressive_bounce adds it.  The
    // frame is render_converging's own: beyond what begins it again there, a changed strength does, a switch between the two calls
    // does, and every camera move does, history or not.  Returns the tick's report, also left in last_report.
    rm_converge_report render_converging_bounce(framebuffer::FrameBuffer &frame, const scene::Scene &sc, const rm_converge &converge,
                                                uint32_t n_samples, double strength = 1., const std::vector<double> &radii = {},
                                                double aperture = 0., double focus = 1., bool restart = false) {
        const rm_params p = prepare(frame.width, frame.height, sc);
        const rm_lens lens{aperture, focus, n_samples, 0u};
        const size_t rows = frame.height - frame.height % 32;
        std::vector<double> flat(rows * frame.width * 3 + 1);                              // (+ 1: never a NULL frame)
        check(rm_render_converging_bounce(ctx_, &p, &lens, &converge, radii.empty() ? nullptr : radii.data(), (uint32_t)radii.size(), strength,
                                          restart ? 1 : 0, flat.data(), nullptr, &last_report, &last_timing),
              ctx_);
        last_samples = last_report.max_count;
        for (size_t y = 0; y < rows; y++)
            for (size_t x = 0; x < frame.width; x++) {
                const double *c = &flat[(y * frame.width + x) * 3];
                frame.buffer[y][x] = Vec3f{c[0], c[1], c[2]};
            }
        return last_report;
    }
    // The variance-guided filter (include/rusty_marcher_amd.h, "variance-guided filter").  rm_denoise_workspace: the bytes
    // denoise_device's workspace needs for `p`
    static size_t denoise_workspace(const rm_params &p) {
        size_t bytes = 0;
        check(rm_denoise_workspace(&p, &bytes), nullptr);
        return bytes;
    }
    // rm_denoise_device for a host that keeps its own device buffers: the filter over a converging frame's sum, stats and count --
    // and, where device_hits is not NULL, the hits of rm_primary_hits_device as the guide -- into device_out and, where given,
    // device_variance and device_rgb8.  Asynchronous on hip_stream
    void denoise_device(const rm_params &p, const rm_denoise &denoise, const void *device_sum, const void *device_stats, const void *device_count,
                        const void *device_hits, void *device_workspace, void *device_out, void *device_variance, void *device_rgb8,
                        void *hip_stream) {
        check(rm_denoise_device(ctx_, &p, &denoise, device_sum, device_stats, device_count, device_hits, device_workspace, device_out,
                                device_variance, device_rgb8, hip_stream),
              ctx_);
    }
    // Temporal reprojection (include/rusty_marcher_amd.h, "temporal reprojection").  rm_reproject_device for a host that keeps
    // its own device buffers: carries the converging frame prev_sum, prev_stats, prev_count, sampled from previous_view whose hits
    // are prev_hits, to the view cur_hits was made for, into out_sum, out_stats, out_count; out_carried and out_carried_total may
    // be NULL.  Asynchronous on hip_stream
    void reproject_device(const rm_params &p, const rm_reproject &reproject, const rm_view &previous_view, const void *prev_sum,
                          const void *prev_stats, const void *prev_count, const void *prev_hits, const void *cur_hits, void *out_sum,
                          void *out_stats, void *out_count, void *out_carried, void *out_carried_total, void *hip_stream) {
        check(rm_reproject_device(ctx_, &p, &reproject, &previous_view, prev_sum, prev_stats, prev_count, prev_hits, cur_hits, out_sum, out_stats,
                                  out_count, out_carried, out_carried_total, hip_stream),
              ctx_);
    }
    // History for render_converging (rm_converge_history): a camera move then carries the frame to the new view rather than
    // beginning it again.  NULL turns it off.  The default holds starting values, not tuned ones; max_history bounds how long
    // view-dependent light is carried as if it stuck to the surface
    void converge_history(const rm_reproject *reproject) { check(rm_converge_history(ctx_, reproject), ctx_); }
    void keep_history(const rm_reproject &reproject = rm_reproject{.1, .9, 32u, 0u}) { converge_history(&reproject); }
    void drop_history() { converge_history(nullptr); }
    // rm_converge_history_info: tells a reprojected tick from one that began again
    rm_history_report history_info() {
        rm_history_report out{};
        check(rm_converge_history_info(ctx_, &out), ctx_);
        return out;
    }
    // The converging frame the last render_converging* call built, filtered into `frame` (rm_render_denoised); the converging
    // frame itself is left alone and its next tick continues it.  guides: steer the filter by the hits under the pixels as well --
    // the pinhole view: off under a wide aperture, a moving camera or strongly moving shapes.  The defaults are starting values,
    // not tuned ones
    std::string render_denoised(framebuffer::FrameBuffer &frame, const scene::Scene &sc,
                                const rm_denoise &denoise = rm_denoise{4., .1, 1e-10, 1., 5u, 5u}, bool guides = true) {
        const auto t0 = std::chrono::steady_clock::now();
        const rm_params p = prepare(frame.width, frame.height, sc);
        const size_t rows = frame.height - frame.height % 32;
        std::vector<double> flat(rows * frame.width * 3 + 1);                              // (+ 1: never a NULL frame)
        check(rm_render_denoised(ctx_, &p, &denoise, guides ? 1 : 0, flat.data(), nullptr, &last_timing), ctx_);
        for (size_t y = 0; y < rows; y++)
            for (size_t x = 0; x < frame.width; x++) {
                const double *c = &flat[(y * frame.width + x) * 3];
                frame.buffer[y][x] = Vec3f{c[0], c[1], c[2]};
            }
        return status(t0, frame.width, frame.height);
    }
    // render_converging with moving spheres (rm_render_converging_motion): shape k of the scene, a sphere, moves by velocities[k] --
    // one vector a shape, zero for what is not a sphere -- while the shutter stands open for `shutter`, and every sample sees it at
    // a time of its own; only the pixels still noisy, the blurred band among them, go on being sampled.  The frame is
    // render_converging's own: beyond what begins it again there, a changed velocity or shutter does, and so does a switch between
    // the two calls.  Every ray of such a frame tests every primitive: a hierarchy holds for spheres that stand still.
    rm_converge_report render_converging_motion(framebuffer::FrameBuffer &frame, const scene::Scene &sc, const std::vector<Vec3f> &velocities,
                                                double shutter, const rm_converge &converge, uint32_t n_samples,
                                                const std::vector<double> &radii = {}, double aperture = 0., double focus = 1.,
                                                bool restart = false) {
        return converging_tick_with_velocities(false, frame, sc, velocities, shutter, converge, n_samples, radii, aperture, focus, restart);
    }
    // render_converging_motion in which every shape moves (rm_render_converging_moving): a velocity on a polygon or a mesh is obeyed
    // -- the plane point and the vertices, every triangle's centre and vertices move as the reference's offset() moves them, the
    // normals stay.  The frame is not render_converging_motion's: a switch between the two begins it again.
    rm_converge_report render_converging_moving(framebuffer::FrameBuffer &frame, const scene::Scene &sc, const std::vector<Vec3f> &velocities,
                                                double shutter, const rm_converge &converge, uint32_t n_samples,
                                                const std::vector<double> &radii = {}, double aperture = 0., double focus = 1.,
                                                bool restart = false) {
        return converging_tick_with_velocities(true, frame, sc, velocities, shutter, converge, n_samples, radii, aperture, focus, restart);
    }
    // The tick of the two calls above; any_shape: the second
    rm_converge_report converging_tick_with_velocities(bool any_shape, framebuffer::FrameBuffer &frame, const scene::Scene &sc,
                                                       const std::vector<Vec3f> &velocities, double shutter, const rm_converge &converge,
                                                       uint32_t n_samples, const std::vector<double> &radii, double aperture, double focus,
                                                       bool restart) {
        const rm_params p = prepare(frame.width, frame.height, sc);
        const rm_lens lens{aperture, focus, n_samples, 0u};
        const size_t rows = frame.height - frame.height % 32;
        std::vector<double> flat(rows * frame.width * 3 + 1);                              // (+ 1: never a NULL frame)
        std::vector<rm_vec3> v;
        for (const Vec3f &e : velocities) v.push_back(e.c());
        const double *r = radii.empty() ? nullptr : radii.data();
        check(any_shape ? rm_render_converging_moving(ctx_, &p, &lens, &converge, r, (uint32_t)radii.size(), v.data(), (uint32_t)v.size(), shutter,
                                                      restart ? 1 : 0, flat.data(), nullptr, &last_report, &last_timing)
                        : rm_render_converging_motion(ctx_, &p, &lens, &converge, r, (uint32_t)radii.size(), v.data(), (uint32_t)v.size(), shutter,
                                                      restart ? 1 : 0, flat.data(), nullptr, &last_report, &last_timing),
              ctx_);
        last_samples = last_report.max_count;
        for (size_t y = 0; y < rows; y++)
            for (size_t x = 0; x < frame.width; x++) {
                const double *c = &flat[(y * frame.width + x) * 3];
                frame.buffer[y][x] = Vec3f{c[0], c[1], c[2]};
            }
        return last_report;
    }
    // render_progressive_moving with a moving camera (rm_render_progressive_camera): the camera moves by motion.velocity and turns by
    // motion's rates while the shutter stands open for `shutter`, and every sample sees the scene from a camera of its own.
    // velocities: empty where no shape moves -- the scene keeps its hierarchy then.  The frame is the call's own: a switch to or from
    // another progressive call begins it again, and so does a changed motion or shutter.
    std::string render_progressive_camera(framebuffer::FrameBuffer &frame, const scene::Scene &sc, const rm_camera_motion &motion, double shutter,
                                          uint32_t n_samples, const std::vector<Vec3f> &velocities = {}, const std::vector<double> &radii = {},
                                          double aperture = 0., double focus = 1., bool restart = false) {
        const auto t0 = std::chrono::steady_clock::now();
        const rm_params p = prepare(frame.width, frame.height, sc);
        const rm_lens lens{aperture, focus, n_samples, 0u};
        const size_t rows = frame.height - frame.height % 32;
        std::vector<double> flat(rows * frame.width * 3 + 1);                              // (+ 1: never a NULL frame)
        std::vector<rm_vec3> v;
        for (const Vec3f &e : velocities) v.push_back(e.c());
        check(rm_render_progressive_camera(ctx_, &p, &lens, radii.empty() ? nullptr : radii.data(), (uint32_t)radii.size(),
                                           v.empty() ? nullptr : v.data(), (uint32_t)v.size(), shutter, &motion, restart ? 1 : 0, flat.data(),
                                           nullptr, &last_samples, &last_timing),
              ctx_);
        for (size_t y = 0; y < rows; y++)
            for (size_t x = 0; x < frame.width; x++) {
                const double *c = &flat[(y * frame.width + x) * 3];
                frame.buffer[y][x] = Vec3f{c[0], c[1], c[2]};
            }
        return status(t0, frame.width, frame.height);
    }
    // render_converging_moving with a moving camera (rm_render_converging_camera): motion and velocities as
    // render_progressive_camera's; only the pixels still noisy go on being sampled.  The frame is the call's own.
    rm_converge_report render_converging_camera(framebuffer::FrameBuffer &frame, const scene::Scene &sc, const rm_camera_motion &motion,
                                                double shutter, const rm_converge &converge, uint32_t n_samples,
                                                const std::vector<Vec3f> &velocities = {}, const std::vector<double> &radii = {},
                                                double aperture = 0., double focus = 1., bool restart = false) {
        const rm_params p = prepare(frame.width, frame.height, sc);
        const rm_lens lens{aperture, focus, n_samples, 0u};
        const size_t rows = frame.height - frame.height % 32;
        std::vector<double> flat(rows * frame.width * 3 + 1);                              // (+ 1: never a NULL frame)
        std::vector<rm_vec3> v;
        for (const Vec3f &e : velocities) v.push_back(e.c());
        check(rm_render_converging_camera(ctx_, &p, &lens, &converge, radii.empty() ? nullptr : radii.data(), (uint32_t)radii.size(),
                                          v.empty() ? nullptr : v.data(), (uint32_t)v.size(), shutter, &motion, restart ? 1 : 0, flat.data(),
                                          nullptr, &last_report, &last_timing),
              ctx_);
        last_samples = last_report.max_count;
        for (size_t y = 0; y < rows; y++)
            for (size_t x = 0; x < frame.width; x++) {
                const double *c = &flat[(y * frame.width + x) * 3];
                frame.buffer[y][x] = Vec3f{c[0], c[1], c[2]};
            }
        return last_report;
    }
    // The oriented camera: the view direction of every later render / render_display / pick (nullptr: the reference's fixed
    // view, down -z with +y up).  It stays with the context; the position is the scene's camera, as before.
    void orient(const rm_camera_basis *basis) { check(rm_camera_orient(context(), basis), ctx_); }
    // ... towards `target` from `eye` (the caller's sc.camera); returns the basis
    rm_camera_basis look_at(Vec3f eye, Vec3f target, Vec3f up = Vec3f{0., 1., 0.}) {
        rm_camera_basis b;
        check(rm_camera_basis_look_at(eye.c(), target.c(), up.c(), &b));
        orient(&b);
        return b;
    }
    // ... turned by yaw / pitch / roll (radians; positive yaw turns left, positive pitch looks up) from what the context holds
    rm_camera_basis turn(double yaw, double pitch = 0., double roll = 0.) {
        rm_camera_basis b, out;
        check(rm_camera_get(context(), nullptr, &b, nullptr), ctx_);
        check(rm_camera_basis_turn(&b, yaw, pitch, roll, &out));
        orient(&out);
        return out;
    }
    rm_ctx *context() { if (!ctx_) check(rm_init(0, &ctx_)); return ctx_; }

  private:
    rm_ctx *ctx_ = nullptr;
    // the whole Scene goes to every call, as the reference hands it to render() (the library copies only what changed)
    void upload(const scene::Scene &sc) {
        if (!ctx_) check(rm_init(0, &ctx_));
        bool owned = false;
        rm_scene *flat = sc.flatten(&owned);
        rm_scene_desc d;
        check(rm_scene_get_desc(flat, &d));
        const rm_status up = rm_scene_upload(ctx_, &d);
        if (owned) rm_scene_free(flat);
        check(up, ctx_);
    }
    rm_params prepare(size_t width_px, size_t height_px, const scene::Scene &sc, bool announce = true) {
        if (!ctx_) check(rm_init(0, &ctx_));
        if (announce) {
            if (height_px % 32 != 0 || width_px % 32 != 0) std::printf("Dimensions mismatch\n");
            std::printf("Rendering using patches of size %d, using %zu patches overall\n", 32, (height_px / 32) * (width_px / 32));
        }
        upload(sc);
        rm_params p;
        rm_create_renderer(fov, height, width, &p);
        p.frame_width = (uint32_t)width_px;
        p.frame_height = (uint32_t)height_px;
        p.max_depth = max_depth;
        p.flags = flags;
        return p;
    }
    static std::string status(std::chrono::steady_clock::time_point t0, size_t width_px, size_t height_px) {
        const uint64_t ms = (uint64_t)std::chrono::duration_cast<std::chrono::milliseconds>(
                                std::chrono::steady_clock::now() - t0).count();
        char buf[256];
        rm_format_status(buf, sizeof buf, ms, (uint32_t)width_px, (uint32_t)height_px);
        std::printf("%s\n", buf);
        return buf;
    }
};
inline Renderer create_renderer(double fov, double height, double width) {   // renderer.rs:25-33: (fov, height, width)
    return Renderer(fov, height, width);
}

// FrameBuffer::normalize + to_vec (framebuffer.rs:40-77) run on the frame the renderer's context
// holds on the device (rm_postprocess): what save_to_file needs when the f64 frame was never
// fetched.  `frame` gives the size.
inline std::vector<uint8_t> to_vec_on_device(Renderer &r, size_t width, size_t height, bool normalize) {
    std::vector<uint8_t> out(width * height * 3);
    check(rm_postprocess(r.context(), nullptr, (uint32_t)width, (uint32_t)height, normalize ? 1 : 0, out.data(), nullptr),
          r.context());
    return out;
}
inline void write_ppm(const std::string &filename, size_t width, size_t height, const std::vector<uint8_t> &rgb) {
    std::ofstream f(filename, std::ios::binary);
    f << "P6\n" << width << " " << height << "\n255\n";
    f.write(reinterpret_cast<const char *>(rgb.data()), (std::streamsize)rgb.size());
}
}  // namespace renderer

}  // namespace rusty_marcher
#endif
