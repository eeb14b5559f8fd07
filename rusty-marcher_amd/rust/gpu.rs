//! engine/src/gpu.rs -- Rust side of the MI355X backend (drop-in for the Rayon patch
//! loop of renderer.rs:63-108).  UNVERIFIED: written against include/rusty_marcher_amd.h,
//! not compiled -- the build image has no rustc/cargo.
//!
//! Edition 2015 like the rest of the crate (bare `use geometry::..` paths).
//! Link with:  cargo:rustc-link-lib=dylib=rusty_marcher_amd  (build.rs)

use std::ffi::CStr;
use std::os::raw::{c_char, c_int, c_void};
use std::ptr;

use framebuffer::FrameBuffer;
use geometry::Vec3f;
use shapes::Reflectance;

// ---- mirrors of the C structs (include/rusty_marcher_amd.h) -------------------------

#[repr(C)]
#[derive(Copy, Clone)]
pub struct RmVec3 {
    pub x: f64,
    pub y: f64,
    pub z: f64,
}

impl From<Vec3f> for RmVec3 {
    fn from(v: Vec3f) -> RmVec3 {
        RmVec3 { x: v.x, y: v.y, z: v.z }
    }
}

#[repr(C)]
#[derive(Copy, Clone)]
pub struct RmReflectance {
    pub diffusion: f64,
    pub diffuse_color: RmVec3,
    pub specular: f64,
    pub specular_exponent: f64,
    pub is_glass_like: i32,
    pub _pad: i32,
    pub reflection: f64,
    pub refractive_index: f64,
}

impl From<Reflectance> for RmReflectance {
    fn from(r: Reflectance) -> RmReflectance {
        RmReflectance {
            diffusion: r.diffusion,
            diffuse_color: r.diffuse_color.into(),
            specular: r.specular,
            specular_exponent: r.specular_exponent,
            is_glass_like: r.is_glass_like as i32,
            _pad: 0,
            reflection: r.reflection,
            refractive_index: r.refractive_index,
        }
    }
}

#[repr(C)]
pub struct RmSceneDesc {
    pub shapes: *const c_void,
    pub n_shapes: u32,
    pub spheres: *const c_void,
    pub n_spheres: u32,
    pub polygons: *const c_void,
    pub n_polygons: u32,
    pub polygon_vertices: *const RmVec3,
    pub n_polygon_vertices: u32,
    pub triangles: *const c_void,
    pub n_triangles: u32,
    pub lights: *const c_void,
    pub n_lights: u32,
    pub camera: RmVec3,
}

#[repr(C)]
pub struct RmParams {
    pub fov: f64,
    pub half_fov: f64,
    pub height: f64,
    pub width: f64,
    pub ratio: f64,
    pub frame_width: u32,
    pub frame_height: u32,
    pub max_depth: u32,
    pub patch_size: u32,
    pub background: RmVec3,
    pub patch_row_begin: u32,
    pub patch_row_end: u32,
    pub flags: u32,
    pub patch_row_stride: u32,
}

#[repr(C)]
#[derive(Default)]
pub struct RmTiming {
    pub kernel_ms: f64,
    pub d2h_ms: f64,
    pub total_ms: f64,
}

#[repr(C)]
#[derive(Default)]
pub struct RmFrameTimes {
    pub kernel_ms: f64,
    pub gather_ms: f64,
    pub total_ms: f64,
}

/// One answer of find_closest_intersect (shapes.rs:110-143): what `Gpu::pick` returns.
/// `shape` indexes `Scene.shapes` (not wrapped to u8); `element` is the triangle inside an `Obj`.
#[repr(C)]
#[derive(Copy, Clone)]
pub struct RmHit {
    pub t: f64,
    pub point: RmVec3,
    pub normal: RmVec3,
    pub shape: u32,
    pub element: u32,
    pub hit: i32,
    pub _pad: u32,
}

/// `rm_range`: the closed range [t_min, t_max] of the ray parameter a ranged query accepts hits in (16 bytes).
#[repr(C)]
#[derive(Copy, Clone)]
pub struct RmRange {
    pub t_min: f64,
    pub t_max: f64,
}

/// `rm_shading`: background and depth cap of a radiance query over a ray list (32 bytes).
#[repr(C)]
#[derive(Copy, Clone)]
pub struct RmShading {
    pub background: RmVec3,
    pub max_depth: u32,
    pub _pad: u32,
}

/// `rm_refine`: what an adaptive anti-aliasing call refines -- n x n samples (n in 1..8) for every pixel whose contrast
/// is > threshold (16 bytes).
#[repr(C)]
#[derive(Copy, Clone)]
pub struct RmRefine {
    pub n: u32,
    pub _pad: u32,
    pub threshold: f64,
}

/// `rm_lens`: the thin lens of a depth-of-field frame -- its radius, the distance of the plane in focus along the view
/// direction, rays a pixel (1..64) (24 bytes).
#[repr(C)]
#[derive(Copy, Clone)]
pub struct RmLens {
    pub aperture: f64,
    pub focus: f64,
    pub n_samples: u32,
    pub _pad: u32,
}

/// `rm_converge`: when a pixel of a converging frame is settled -- the standard error of the mean of r + g + b it may keep
/// (< 0: no pixel ever settles), the fewest samples a settled pixel has, the most any pixel gets (16 bytes).
#[repr(C)]
#[derive(Copy, Clone)]
pub struct RmConverge {
    pub tolerance: f64,
    pub min_samples: u32,
    pub max_samples: u32,
}

/// `rm_converge_frame`: the device buffers of a converging frame -- sum, stats, count, workspace; mean, rgb8 and mask may be
/// null (56 bytes).
#[repr(C)]
#[derive(Copy, Clone)]
pub struct RmConvergeFrame {
    pub sum: *mut c_void,
    pub stats: *mut c_void,
    pub count: *mut c_void,
    pub workspace: *mut c_void,
    pub mean: *mut c_void,
    pub rgb8: *mut c_void,
    pub mask: *mut c_void,
}

/// `rm_converge_report`: what a tick of a converging frame reports; `listed == 0` says the picture is finished (24 bytes).
#[repr(C)]
#[derive(Copy, Clone, Default)]
pub struct RmConvergeReport {
    pub samples_cast: u64,
    pub listed: u32,
    pub passes: u32,
    pub max_count: u32,
    pub _pad: u32,
}

/// `rm_denoise`: the variance-guided filter's control -- the luminance edge stop in standard errors, the plane-distance edge stop
/// relative to 1 + t, the luminance denominator's epsilon, the variance of a pixel with fewer than two samples, the iterations
/// (0..5, iteration i has step 1 << i) and how often the normals' dot product is squared (0..8) (40 bytes).
#[repr(C)]
#[derive(Copy, Clone)]
pub struct RmDenoise {
    pub sigma_l: f64,
    pub sigma_z: f64,
    pub epsilon: f64,
    pub fallback_variance: f64,
    pub iterations: u32,
    pub normal_squarings: u32,
}

impl Default for RmDenoise {
    /// Starting values, not tuned ones.
    fn default() -> RmDenoise {
        RmDenoise { sigma_l: 4., sigma_z: 0.1, epsilon: 1e-10, fallback_variance: 1., iterations: 5, normal_squarings: 5 }
    }
}

/// `rm_view`: a camera as `rm_camera_get` reports it, position and basis (96 bytes).
#[repr(C)]
#[derive(Copy, Clone)]
pub struct RmView {
    pub position: RmVec3,
    pub basis: RmCameraBasis,
}

/// `rm_reproject`: the temporal reprojection's control -- the plane-distance gate relative to 1 + t, the dot product of the
/// normals a tap must exceed, and the most samples a pixel may carry (24 bytes).
#[repr(C)]
#[derive(Copy, Clone)]
pub struct RmReproject {
    pub sigma_z: f64,
    pub min_normal_dot: f64,
    pub max_history: u32,
    pub _pad: u32,
}

impl Default for RmReproject {
    /// Starting values, not tuned ones.
    fn default() -> RmReproject {
        RmReproject { sigma_z: 0.1, min_normal_dot: 0.9, max_history: 32, _pad: 0 }
    }
}

/// `rm_history_report`: what the converging tick did with its history (24 bytes).
#[repr(C)]
#[derive(Copy, Clone, Default)]
pub struct RmHistoryReport {
    /// Frames the ticks have begun from history since the context was made.
    pub reprojections: u64,
    /// The last `render_converging` tick began its frame from history: 1, else 0.
    pub last_reprojected: u32,
    /// Pixels that carried history at the last reprojection, and those of the frame's rows that did not.
    pub carried: u32,
    pub without: u32,
    pub _pad: u32,
}

/// `rm_camera_motion`: how the camera moves while the shutter stands open -- world units a unit of time, and yaw, pitch and roll
/// in radians a unit of time about the axes and with the signs of `basis_turn` (48 bytes).
#[repr(C)]
#[derive(Copy, Clone)]
pub struct RmCameraMotion {
    pub velocity: RmVec3,
    pub yaw: f64,
    pub pitch: f64,
    pub roll: f64,
}

/// `rm_lights_visible`'s modes: the decision direct_lighting takes / the shadow ray ended at the light.
pub const RM_LIGHTS_AS_RENDERED: u32 = 0;
pub const RM_LIGHTS_CLIPPED: u32 = 1;

/// `rm_camera_basis`: the oriented camera's view direction, three world-space unit vectors (72 bytes).
/// The reference's fixed view is right (1,0,0), up (0,1,0), forward (0,0,-1).
#[repr(C)]
#[derive(Copy, Clone)]
pub struct RmCameraBasis {
    pub right: RmVec3,
    pub up: RmVec3,
    pub forward: RmVec3,
}

/// `rm_swept_tick_report`: what the ticks that move a shape did (8 bytes).
#[repr(C)]
#[derive(Copy, Clone, Default)]
pub struct RmSweptTickReport {
    /// The last sampled-frame tick's launch walked a swept hierarchy: 1, else 0.
    pub walked_swept: u32,
    /// Hierarchies the ticks have built over the context's life.
    pub builds: u32,
}

pub enum RmScene {}
pub enum RmCtx {}
pub enum RmSwept {}

// Every entry point of include/rusty_marcher_amd.h, in its order (tests/test_rust_binding.py
// checks names, arity and argument classes against the header).
#[link(name = "rusty_marcher_amd")]
#[allow(dead_code)]
extern "C" {
    fn rm_reflectance_default(out: *mut RmReflectance);
    fn rm_create_renderer(fov: f64, height: f64, width: f64, out: *mut RmParams);
    fn rm_scene_new(out: *mut *mut RmScene) -> c_int;
    fn rm_scene_free(scene: *mut RmScene);
    fn rm_scene_create_default(out: *mut *mut RmScene) -> c_int;
    fn rm_scene_add_sphere(scene: *mut RmScene, center: RmVec3, radius: f64, r: *const RmReflectance) -> c_int;
    fn rm_scene_add_polygon(scene: *mut RmScene, vertices: *const RmVec3, n_vertices: u32, r: *const RmReflectance) -> c_int;
    fn rm_scene_add_mesh(scene: *mut RmScene, tri_xyz: *const f64, n_triangles: u32, offset: RmVec3) -> c_int;
    fn rm_scene_add_light(scene: *mut RmScene, position: RmVec3, color: RmVec3, intensity: f64) -> c_int;
    fn rm_scene_offset_shape(scene: *mut RmScene, shape_index: u32, offset: RmVec3) -> c_int;
    fn rm_scene_set_camera(scene: *mut RmScene, camera: RmVec3) -> c_int;
    fn rm_scene_offset_camera(scene: *mut RmScene, offset: RmVec3) -> c_int;
    fn rm_scene_load_obj(scene: *mut RmScene, path: *const c_char, offset: RmVec3, n_models_out: *mut u32) -> c_int;
    fn rm_scene_open_obj(path: *const c_char, out: *mut *mut RmScene) -> c_int;
    fn rm_scene_get_desc(scene: *const RmScene, out: *mut RmSceneDesc) -> c_int;
    fn rm_format_status(buf: *mut c_char, buflen: usize, ms: u64, frame_width: u32, frame_height: u32) -> c_int;
    fn rm_init(device_ordinal: c_int, out: *mut *mut RmCtx) -> c_int;
    fn rm_destroy(ctx: *mut RmCtx);
    fn rm_last_error(ctx: *const RmCtx) -> *const c_char;
    fn rm_scene_upload(ctx: *mut RmCtx, desc: *const RmSceneDesc) -> c_int;
    fn rm_scene_uploads(ctx: *mut RmCtx, calls: *mut u64, copies: *mut u64) -> c_int;
    fn rm_camera_update(ctx: *mut RmCtx, camera: RmVec3) -> c_int;
    fn rm_camera_orient(ctx: *mut RmCtx, basis: *const RmCameraBasis) -> c_int;
    fn rm_camera_look_at(ctx: *mut RmCtx, eye: RmVec3, target: RmVec3, up_hint: RmVec3) -> c_int;
    fn rm_camera_get(ctx: *mut RmCtx, position: *mut RmVec3, basis: *mut RmCameraBasis, oriented: *mut c_int) -> c_int;
    fn rm_camera_basis_look_at(eye: RmVec3, target: RmVec3, up_hint: RmVec3, out: *mut RmCameraBasis) -> c_int;
    fn rm_camera_basis_turn(input: *const RmCameraBasis, yaw: f64, pitch: f64, roll: f64, out: *mut RmCameraBasis) -> c_int;
    fn rm_camera_basis_check(basis: *const RmCameraBasis) -> c_int;
    fn rm_render(ctx: *mut RmCtx, params: *const RmParams, host_rgb: *mut f64, timing: *mut RmTiming) -> c_int;
    fn rm_render_rows(ctx: *mut RmCtx, params: *const RmParams, rows: *const *mut f64, timing: *mut RmTiming) -> c_int;
    fn rm_render_display(ctx: *mut RmCtx, params: *const RmParams, host_rgb8: *mut u8, timing: *mut RmTiming) -> c_int;
    fn rm_fetch_rows(ctx: *mut RmCtx, rows: *const *mut f64, frame_width: u32, frame_height: u32, patch_row_begin: u32, patch_row_end: u32) -> c_int;
    fn rm_hostio_stats(ctx: *mut RmCtx, bytes_copied: *mut u64, patches: *mut u64, patches_sent: *mut u64, threads: *mut c_int) -> c_int;
    fn rm_render_device(ctx: *mut RmCtx, params: *const RmParams, device_rgb: *mut c_void, hip_stream: *mut c_void) -> c_int;
    fn rm_render_device_u8(ctx: *mut RmCtx, params: *const RmParams, device_rgb: *mut c_void, device_rgb8: *mut c_void, hip_stream: *mut c_void) -> c_int;
    fn rm_tile_stats(ctx: *mut RmCtx, hip_stream: *mut c_void, tiles: *mut u32, tiles_listed: *mut u32) -> c_int;
    fn rm_launch_stats(ctx: *mut RmCtx, workgroups: *mut u32, tail_patches: *mut u32) -> c_int;
    fn rm_device_framebuffer(ctx: *mut RmCtx, device_rgb: *mut *mut c_void, bytes: *mut usize) -> c_int;
    fn rm_postprocess(ctx: *mut RmCtx, device_rgb: *mut c_void, frame_width: u32, frame_height: u32, normalize: c_int, host_rgb8: *mut u8, max_out: *mut f64) -> c_int;
    // interactive loop / several GPUs (one process per GPU): host/rm_walk.cpp is the same
    // sequence in C++ -- rm_camera_update between frames, up to 4 frames in flight
    fn rm_buffer_alloc(ctx: *mut RmCtx, bytes: usize, device_ptr: *mut *mut c_void) -> c_int;
    fn rm_buffer_free(ctx: *mut RmCtx, device_ptr: *mut c_void);
    fn rm_buffer_read(ctx: *mut RmCtx, device_ptr: *const c_void, host_dst: *mut c_void, bytes: usize) -> c_int;
    fn rm_buffer_write(ctx: *mut RmCtx, device_ptr: *mut c_void, host_src: *const c_void, bytes: usize) -> c_int;
    fn rm_host_alloc(ctx: *mut RmCtx, bytes: usize, host_ptr: *mut *mut c_void) -> c_int;
    fn rm_host_free(ctx: *mut RmCtx, host_ptr: *mut c_void);
    fn rm_comm_unique_id(id_out: *mut c_void) -> c_int; // 128 bytes
    fn rm_comm_init(ctx: *mut RmCtx, id: *const c_void, rank: c_int, world: c_int) -> c_int;
    fn rm_comm_destroy(ctx: *mut RmCtx);
    fn rm_comm_exchange(ctx: *mut RmCtx, all_ranks: c_int) -> c_int;
    fn rm_exchange_layout(params: *const RmParams, world: c_int, rows_per_rank: *mut u32, chunk_bytes: *mut usize) -> c_int;
    fn rm_frame_submit(ctx: *mut RmCtx, params: *const RmParams, device_rgb: *mut c_void, device_gather8: *mut c_void, device_display8: *mut c_void, slot: u32) -> c_int;
    fn rm_frame_submit_to_host(ctx: *mut RmCtx, params: *const RmParams, device_rgb: *mut c_void, device_gather8: *mut c_void, device_display8: *mut c_void, host_display8: *mut c_void, slot: u32) -> c_int;
    fn rm_frame_wait(ctx: *mut RmCtx, slot: u32) -> c_int;
    fn rm_frame_wait_for(ctx: *mut RmCtx, slot: u32, timeout_ms: u32) -> c_int;
    fn rm_frame_submit_f64(ctx: *mut RmCtx, params: *const RmParams, device_gather64: *mut c_void, device_frame64: *mut c_void, slot: u32) -> c_int;
    fn rm_frame_timing_enable(ctx: *mut RmCtx, on: c_int) -> c_int;
    fn rm_frame_timing(ctx: *mut RmCtx, slot: u32, out: *mut RmFrameTimes) -> c_int;
    fn rm_comm_info(ctx: *mut RmCtx, rank: *mut c_int, world: *mut c_int, n_communicators: *mut c_int) -> c_int;
    fn rm_intersect_rays(ctx: *mut RmCtx, origins: *const RmVec3, directions: *const RmVec3, n_rays: u32, hits: *mut RmHit) -> c_int;
    fn rm_occluded_rays(ctx: *mut RmCtx, origins: *const RmVec3, directions: *const RmVec3, n_rays: u32, occluded: *mut u8) -> c_int;
    fn rm_intersect_rays_device(ctx: *mut RmCtx, device_origins: *const c_void, device_directions: *const c_void, n_rays: u32, device_hits: *mut c_void, hip_stream: *mut c_void) -> c_int;
    fn rm_occluded_rays_device(ctx: *mut RmCtx, device_origins: *const c_void, device_directions: *const c_void, n_rays: u32, device_occluded: *mut c_void, hip_stream: *mut c_void) -> c_int;
    fn rm_pick(ctx: *mut RmCtx, params: *const RmParams, x: u32, y: u32, hit: *mut RmHit) -> c_int;
    fn rm_primary_hits_device(ctx: *mut RmCtx, params: *const RmParams, device_hits: *mut c_void, hip_stream: *mut c_void) -> c_int;
    fn rm_intersect_rays_ranged(ctx: *mut RmCtx, origins: *const RmVec3, directions: *const RmVec3, ranges: *const RmRange, n_rays: u32, hits: *mut RmHit) -> c_int;
    fn rm_occluded_rays_ranged(ctx: *mut RmCtx, origins: *const RmVec3, directions: *const RmVec3, ranges: *const RmRange, n_rays: u32, occluded: *mut u8) -> c_int;
    fn rm_intersect_rays_ranged_device(ctx: *mut RmCtx, device_origins: *const c_void, device_directions: *const c_void, device_ranges: *const c_void, n_rays: u32, device_hits: *mut c_void, hip_stream: *mut c_void) -> c_int;
    fn rm_occluded_rays_ranged_device(ctx: *mut RmCtx, device_origins: *const c_void, device_directions: *const c_void, device_ranges: *const c_void, n_rays: u32, device_occluded: *mut c_void, hip_stream: *mut c_void) -> c_int;
    fn rm_visible_segments(ctx: *mut RmCtx, from: *const RmVec3, to: *const RmVec3, n: u32, skin: f64, visible: *mut u8) -> c_int;
    fn rm_visible_segments_device(ctx: *mut RmCtx, device_from: *const c_void, device_to: *const c_void, n: u32, skin: f64, device_visible: *mut c_void, hip_stream: *mut c_void) -> c_int;
    fn rm_lights_visible(ctx: *mut RmCtx, points: *const RmVec3, normals: *const RmVec3, n_points: u32, n_lights: u32, mode: u32, lit: *mut u8) -> c_int;
    fn rm_lights_visible_device(ctx: *mut RmCtx, device_points: *const c_void, device_normals: *const c_void, n_points: u32, n_lights: u32, mode: u32, device_lit: *mut c_void, hip_stream: *mut c_void) -> c_int;
    fn rm_radiance_rays(ctx: *mut RmCtx, origins: *const RmVec3, directions: *const RmVec3, n_rays: u32, shading: *const RmShading, rgb: *mut RmVec3) -> c_int;
    fn rm_radiance_rays_device(ctx: *mut RmCtx, device_origins: *const c_void, device_directions: *const c_void, n_rays: u32, shading: *const RmShading, device_rgb: *mut c_void, hip_stream: *mut c_void) -> c_int;
    fn rm_radiance_samples(ctx: *mut RmCtx, params: *const RmParams, xy: *const f64, n: u32, rgb: *mut RmVec3) -> c_int;
    fn rm_radiance_samples_device(ctx: *mut RmCtx, params: *const RmParams, device_xy: *const c_void, n: u32, device_rgb: *mut c_void, hip_stream: *mut c_void) -> c_int;
    fn rm_refine_workspace(params: *const RmParams, bytes: *mut usize) -> c_int;
    fn rm_refine_device(ctx: *mut RmCtx, params: *const RmParams, refine: *const RmRefine, device_rgb: *mut c_void, device_workspace: *mut c_void, device_mask: *mut c_void, hip_stream: *mut c_void) -> c_int;
    fn rm_render_antialiased(ctx: *mut RmCtx, params: *const RmParams, refine: *const RmRefine, host_rgb: *mut f64, n_refined: *mut u32, timing: *mut RmTiming) -> c_int;
    fn rm_lens_table(n_samples: u32, table: *mut f64) -> c_int;
    fn rm_render_lens_device(ctx: *mut RmCtx, params: *const RmParams, lens: *const RmLens, device_table: *const c_void, device_rgb: *mut c_void, hip_stream: *mut c_void) -> c_int;
    fn rm_render_lens(ctx: *mut RmCtx, params: *const RmParams, lens: *const RmLens, table: *const f64, host_rgb: *mut f64, timing: *mut RmTiming) -> c_int;
    fn rm_lens_sequence(first: u32, count: u32, table: *mut f64) -> c_int;
    fn rm_accumulate_lens_device(ctx: *mut RmCtx, params: *const RmParams, lens: *const RmLens, device_table: *const c_void, n_before: u32, device_sum: *mut c_void, device_mean: *mut c_void, device_rgb8: *mut c_void, hip_stream: *mut c_void) -> c_int;
    fn rm_render_progressive(ctx: *mut RmCtx, params: *const RmParams, lens: *const RmLens, restart: c_int, host_rgb: *mut f64, host_rgb8: *mut u8, n_total: *mut u32, timing: *mut RmTiming) -> c_int;
    fn rm_light_sequence(first: u32, count: u32, radii: *const f64, n_lights: u32, offsets: *mut f64) -> c_int;
    fn rm_accumulate_soft_device(ctx: *mut RmCtx, params: *const RmParams, lens: *const RmLens, device_table: *const c_void, device_offsets: *const c_void, n_lights: u32, n_before: u32, device_sum: *mut c_void, device_mean: *mut c_void, device_rgb8: *mut c_void, hip_stream: *mut c_void) -> c_int;
    fn rm_render_progressive_soft(ctx: *mut RmCtx, params: *const RmParams, lens: *const RmLens, radii: *const f64, n_lights: u32, restart: c_int, host_rgb: *mut f64, host_rgb8: *mut u8, n_total: *mut u32, timing: *mut RmTiming) -> c_int;
    fn rm_motion_sequence(first: u32, count: u32, velocities: *const RmVec3, n_shapes: u32, shutter: f64, offsets: *mut f64) -> c_int;
    fn rm_accumulate_motion_device(ctx: *mut RmCtx, params: *const RmParams, lens: *const RmLens, device_table: *const c_void, device_light_offsets: *const c_void, n_lights: u32, device_shape_offsets: *const c_void, n_shapes: u32, n_before: u32, device_sum: *mut c_void, device_mean: *mut c_void, device_rgb8: *mut c_void, hip_stream: *mut c_void) -> c_int;
    fn rm_render_progressive_motion(ctx: *mut RmCtx, params: *const RmParams, lens: *const RmLens, radii: *const f64, n_lights: u32, velocities: *const RmVec3, n_shapes: u32, shutter: f64, restart: c_int, host_rgb: *mut f64, host_rgb8: *mut u8, n_total: *mut u32, timing: *mut RmTiming) -> c_int;
    fn rm_accumulate_moving_device(ctx: *mut RmCtx, params: *const RmParams, lens: *const RmLens, device_table: *const c_void, device_light_offsets: *const c_void, n_lights: u32, device_shape_offsets: *const c_void, n_shapes: u32, n_before: u32, device_sum: *mut c_void, device_mean: *mut c_void, device_rgb8: *mut c_void, hip_stream: *mut c_void) -> c_int;
    fn rm_render_progressive_moving(ctx: *mut RmCtx, params: *const RmParams, lens: *const RmLens, radii: *const f64, n_lights: u32, velocities: *const RmVec3, n_shapes: u32, shutter: f64, restart: c_int, host_rgb: *mut f64, host_rgb8: *mut u8, n_total: *mut u32, timing: *mut RmTiming) -> c_int;
    fn rm_converge_workspace(params: *const RmParams, bytes: *mut usize) -> c_int;
    fn rm_accumulate_converging_device(ctx: *mut RmCtx, params: *const RmParams, lens: *const RmLens, converge: *const RmConverge, device_table: *const c_void, table_rows: u32, device_offsets: *const c_void, n_lights: u32, fresh: c_int, buffers: *const RmConvergeFrame, hip_stream: *mut c_void) -> c_int;
    fn rm_render_converging(ctx: *mut RmCtx, params: *const RmParams, lens: *const RmLens, converge: *const RmConverge, radii: *const f64, n_lights: u32, restart: c_int, host_rgb: *mut f64, host_rgb8: *mut u8, report: *mut RmConvergeReport, timing: *mut RmTiming) -> c_int;
    fn rm_accumulate_converging_motion_device(ctx: *mut RmCtx, params: *const RmParams, lens: *const RmLens, converge: *const RmConverge, device_table: *const c_void, table_rows: u32, device_light_offsets: *const c_void, n_lights: u32, device_shape_offsets: *const c_void, n_shapes: u32, fresh: c_int, buffers: *const RmConvergeFrame, hip_stream: *mut c_void) -> c_int;
    fn rm_render_converging_motion(ctx: *mut RmCtx, params: *const RmParams, lens: *const RmLens, converge: *const RmConverge, radii: *const f64, n_lights: u32, velocities: *const RmVec3, n_shapes: u32, shutter: f64, restart: c_int, host_rgb: *mut f64, host_rgb8: *mut u8, report: *mut RmConvergeReport, timing: *mut RmTiming) -> c_int;
    fn rm_accumulate_converging_moving_device(ctx: *mut RmCtx, params: *const RmParams, lens: *const RmLens, converge: *const RmConverge, device_table: *const c_void, table_rows: u32, device_light_offsets: *const c_void, n_lights: u32, device_shape_offsets: *const c_void, n_shapes: u32, fresh: c_int, buffers: *const RmConvergeFrame, hip_stream: *mut c_void) -> c_int;
    fn rm_camera_sequence(first: u32, count: u32, motion: *const RmCameraMotion, basis: *const RmCameraBasis, shutter: f64, rows: *mut f64) -> c_int;
    fn rm_accumulate_camera_device(ctx: *mut RmCtx, params: *const RmParams, lens: *const RmLens, device_table: *const c_void, device_camera_rows: *const c_void, device_light_offsets: *const c_void, n_lights: u32, device_shape_offsets: *const c_void, n_shapes: u32, n_before: u32, device_sum: *mut c_void, device_mean: *mut c_void, device_rgb8: *mut c_void, hip_stream: *mut c_void) -> c_int;
    fn rm_accumulate_converging_camera_device(ctx: *mut RmCtx, params: *const RmParams, lens: *const RmLens, converge: *const RmConverge, device_table: *const c_void, table_rows: u32, device_camera_rows: *const c_void, device_light_offsets: *const c_void, n_lights: u32, device_shape_offsets: *const c_void, n_shapes: u32, fresh: c_int, buffers: *const RmConvergeFrame, hip_stream: *mut c_void) -> c_int;
    fn rm_render_progressive_camera(ctx: *mut RmCtx, params: *const RmParams, lens: *const RmLens, radii: *const f64, n_lights: u32, velocities: *const RmVec3, n_shapes: u32, shutter: f64, motion: *const RmCameraMotion, restart: c_int, host_rgb: *mut f64, host_rgb8: *mut u8, n_total: *mut u32, timing: *mut RmTiming) -> c_int;
    fn rm_render_converging_camera(ctx: *mut RmCtx, params: *const RmParams, lens: *const RmLens, converge: *const RmConverge, radii: *const f64, n_lights: u32, velocities: *const RmVec3, n_shapes: u32, shutter: f64, motion: *const RmCameraMotion, restart: c_int, host_rgb: *mut f64, host_rgb8: *mut u8, report: *mut RmConvergeReport, timing: *mut RmTiming) -> c_int;
    fn rm_render_converging_moving(ctx: *mut RmCtx, params: *const RmParams, lens: *const RmLens, converge: *const RmConverge, radii: *const f64, n_lights: u32, velocities: *const RmVec3, n_shapes: u32, shutter: f64, restart: c_int, host_rgb: *mut f64, host_rgb8: *mut u8, report: *mut RmConvergeReport, timing: *mut RmTiming) -> c_int;
    fn rm_swept_extents(table: *const f64, rows: u32, n_shapes: u32, lo: *mut f64, hi: *mut f64) -> c_int;
    fn rm_swept_motion_extents(velocities: *const RmVec3, n_shapes: u32, shutter: f64, lo: *mut f64, hi: *mut f64) -> c_int;
    fn rm_swept_build(ctx: *mut RmCtx, lo: *const f64, hi: *const f64, n_shapes: u32, out: *mut *mut RmSwept) -> c_int;
    fn rm_swept_free(ctx: *mut RmCtx, swept: *mut RmSwept);
    fn rm_accumulate_swept_device(ctx: *mut RmCtx, params: *const RmParams, lens: *const RmLens, device_table: *const c_void, device_light_offsets: *const c_void, n_lights: u32, device_shape_offsets: *const c_void, n_shapes: u32, swept: *const RmSwept, n_before: u32, device_sum: *mut c_void, device_mean: *mut c_void, device_rgb8: *mut c_void, hip_stream: *mut c_void) -> c_int;
    fn rm_accumulate_converging_swept_device(ctx: *mut RmCtx, params: *const RmParams, lens: *const RmLens, converge: *const RmConverge, device_table: *const c_void, table_rows: u32, device_light_offsets: *const c_void, n_lights: u32, device_shape_offsets: *const c_void, n_shapes: u32, swept: *const RmSwept, fresh: c_int, buffers: *const RmConvergeFrame, hip_stream: *mut c_void) -> c_int;
    fn rm_accumulate_camera_swept_device(ctx: *mut RmCtx, params: *const RmParams, lens: *const RmLens, device_table: *const c_void, device_camera_rows: *const c_void, device_light_offsets: *const c_void, n_lights: u32, device_shape_offsets: *const c_void, n_shapes: u32, swept: *const RmSwept, n_before: u32, device_sum: *mut c_void, device_mean: *mut c_void, device_rgb8: *mut c_void, hip_stream: *mut c_void) -> c_int;
    fn rm_accumulate_converging_camera_swept_device(ctx: *mut RmCtx, params: *const RmParams, lens: *const RmLens, converge: *const RmConverge, device_table: *const c_void, table_rows: u32, device_camera_rows: *const c_void, device_light_offsets: *const c_void, n_lights: u32, device_shape_offsets: *const c_void, n_shapes: u32, swept: *const RmSwept, fresh: c_int, buffers: *const RmConvergeFrame, hip_stream: *mut c_void) -> c_int;
    fn rm_swept_tick_info(ctx: *mut RmCtx, out: *mut RmSweptTickReport) -> c_int;
    fn rm_bounce_sequence(first: u32, count: u32, table: *mut f64) -> c_int;
    fn rm_accumulate_bounce_device(ctx: *mut RmCtx, params: *const RmParams, lens: *const RmLens, device_table: *const c_void, device_offsets: *const c_void, n_lights: u32, device_bounce: *const c_void, strength: f64, n_before: u32, device_sum: *mut c_void, device_mean: *mut c_void, device_rgb8: *mut c_void, hip_stream: *mut c_void) -> c_int;
    fn rm_accumulate_converging_bounce_device(ctx: *mut RmCtx, params: *const RmParams, lens: *const RmLens, converge: *const RmConverge, device_table: *const c_void, table_rows: u32, device_offsets: *const c_void, n_lights: u32, device_bounce: *const c_void, strength: f64, fresh: c_int, buffers: *const RmConvergeFrame, hip_stream: *mut c_void) -> c_int;
    fn rm_render_progressive_bounce(ctx: *mut RmCtx, params: *const RmParams, lens: *const RmLens, radii: *const f64, n_lights: u32, strength: f64, restart: c_int, host_rgb: *mut f64, host_rgb8: *mut u8, n_total: *mut u32, timing: *mut RmTiming) -> c_int;
    fn rm_render_converging_bounce(ctx: *mut RmCtx, params: *const RmParams, lens: *const RmLens, converge: *const RmConverge, radii: *const f64, n_lights: u32, strength: f64, restart: c_int, host_rgb: *mut f64, host_rgb8: *mut u8, report: *mut RmConvergeReport, timing: *mut RmTiming) -> c_int;
    fn rm_abi_version() -> u32;
    fn rm_denoise_workspace(params: *const RmParams, bytes: *mut usize) -> c_int;
    fn rm_denoise_device(ctx: *mut RmCtx, params: *const RmParams, denoise: *const RmDenoise, device_sum: *const c_void, device_stats: *const c_void, device_count: *const c_void, device_hits: *const c_void, device_workspace: *mut c_void, device_out: *mut c_void, device_variance: *mut c_void, device_rgb8: *mut c_void, hip_stream: *mut c_void) -> c_int;
    fn rm_render_denoised(ctx: *mut RmCtx, params: *const RmParams, denoise: *const RmDenoise, guides: c_int, host_rgb: *mut f64, host_rgb8: *mut u8, timing: *mut RmTiming) -> c_int;
    fn rm_reproject_device(ctx: *mut RmCtx, params: *const RmParams, reproject: *const RmReproject, previous_view: *const RmView, prev_sum: *const c_void, prev_stats: *const c_void, prev_count: *const c_void, prev_hits: *const c_void, cur_hits: *const c_void, out_sum: *mut c_void, out_stats: *mut c_void, out_count: *mut c_void, out_carried: *mut c_void, out_carried_total: *mut c_void, hip_stream: *mut c_void) -> c_int;
    fn rm_converge_history(ctx: *mut RmCtx, reproject: *const RmReproject) -> c_int;
    fn rm_converge_history_info(ctx: *mut RmCtx, report: *mut RmHistoryReport) -> c_int;
    fn rm_build_info() -> *const c_char;
    fn rm_device_info(ctx: *mut RmCtx, name_buf: *mut c_char, buflen: usize, n_cus: *mut c_int, lds_bytes: *mut usize) -> c_int;
    fn rm_kernel_name(ctx: *mut RmCtx, params: *const RmParams, buf: *mut c_char, buflen: usize) -> c_int;
}

/// The reference's failure mode on this path is a panic.
fn check(status: c_int, ctx: *const RmCtx) {
    if status != 0 {
        let msg = unsafe { CStr::from_ptr(rm_last_error(ctx)) }.to_string_lossy().into_owned();
        panic!("rusty_marcher_amd: status {}: {}", status, msg);
    }
}

/// What `trait Shape` lacks for a GPU backend: a way to hand over the primitive's
/// parameters (sphere.rs:6-11 and polygon.rs:6-12 keep their fields private).
/// Each implementor adds itself to the flat scene; see INTEGRATION.md for the three
/// five-line impls.
pub struct SceneSink {
    scene: *mut RmScene,
}

impl SceneSink {
    pub fn sphere(&mut self, center: Vec3f, radius: f64, r: Reflectance) {
        let rr: RmReflectance = r.into();
        check(unsafe { rm_scene_add_sphere(self.scene, center.into(), radius, &rr) }, ptr::null());
    }
    pub fn polygon(&mut self, vertices: &[Vec3f], r: Reflectance) {
        let v: Vec<RmVec3> = vertices.iter().map(|p| (*p).into()).collect();
        let rr: RmReflectance = r.into();
        check(unsafe { rm_scene_add_polygon(self.scene, v.as_ptr(), v.len() as u32, &rr) }, ptr::null());
    }
    /// One `Obj`: triangles as 9 f64 each (already offset: pass Vec3f::zero()), or the
    /// un-offset vertices plus the offsets applied so far through `offset_last`.
    pub fn mesh(&mut self, tri_xyz: &[f64], offset: Vec3f) {
        check(
            unsafe { rm_scene_add_mesh(self.scene, tri_xyz.as_ptr(), (tri_xyz.len() / 9) as u32, offset.into()) },
            ptr::null(),
        );
    }
    pub fn offset_shape(&mut self, index: u32, off: Vec3f) {
        check(unsafe { rm_scene_offset_shape(self.scene, index, off.into()) }, ptr::null());
    }
}

/// One GPU.  Owned by `Renderer` (renderer.rs:17-23 gains a `gpu: RefCell<Gpu>` field) or by
/// `Win`.  The page-locked staging frame the copies go through belongs to the library's context
/// (include/rusty_marcher_amd.h, rm_render_rows): nothing to allocate, grow or free here.
pub struct Gpu {
    ctx: *mut RmCtx,
}

/// `FrameBuffer.buffer` is `Vec<Vec<Vec3f>>` (framebuffer.rs:6-10): one heap allocation per scan
/// line.  With `#[repr(C)]` on `Vec3f` (geometry.rs:4-8: three f64, x y z -- INTEGRATION.md
/// section 3d, the fourth one-line patch) a row is `width * 3` doubles and the library fills the
/// rows in place.
///
/// `buffer`, `width` and `height` are all `pub` (framebuffer.rs:6-10), so nothing but this check stands between a
/// FrameBuffer whose fields disagree and a write beyond a row's allocation: the library writes `width * 3` doubles
/// into each of `height` rows.  A panic here is the reference's own failure mode for such a frame (its scatter,
/// renderer.rs:92-108, indexes out of bounds).
fn row_pointers(frame: &mut FrameBuffer) -> Vec<*mut f64> {
    // the cast below reads a Vec3f as three consecutive f64: true only with `#[repr(C)]`
    const _VEC3F_IS_THREE_F64: [(); 24] = [(); ::std::mem::size_of::<Vec3f>()];
    assert!(frame.buffer.len() >= frame.height, "FrameBuffer: {} rows for a height of {}", frame.buffer.len(), frame.height);
    for (y, row) in frame.buffer.iter().enumerate() {
        assert!(row.len() == frame.width, "FrameBuffer: row {} holds {} pixels for a width of {}", y, row.len(), frame.width);
    }
    frame.buffer.iter_mut().map(|row| row.as_mut_ptr() as *mut f64).collect()
}

impl Gpu {
    pub fn new(device: i32) -> Gpu {
        let mut ctx: *mut RmCtx = ptr::null_mut();
        check(unsafe { rm_init(device, &mut ctx) }, ptr::null());
        Gpu { ctx }
    }

    /// flatten Scene -> rm_scene (shapes in list order: ties, shapes.rs:130) and hand it to the
    /// context.  render() gets the whole Scene every call (main.rs:331-333), so the flat copy is
    /// rebuilt every call (microseconds for the reference's scenes); rm_scene_upload compares
    /// it with the description the resident device image was built from and copies nothing when
    /// they are the same -- camera moves included, the camera is a kernel argument.
    fn upload(&mut self, scene: &::scene::Scene) {
        let mut raw: *mut RmScene = ptr::null_mut();
        check(unsafe { rm_scene_new(&mut raw) }, ptr::null());
        {
            let mut sink = SceneSink { scene: raw };
            for shape in &scene.shapes {
                shape.describe(&mut sink); // the added trait method
            }
        }
        for l in &scene.lights {
            // colours are already L-inf normalised (lights.rs:10-16); normalising again is a no-op
            check(unsafe { rm_scene_add_light(raw, l.position.into(), l.color.into(), l.intensity) }, ptr::null());
        }
        check(unsafe { rm_scene_set_camera(raw, scene.camera.into()) }, ptr::null());
        let mut desc: RmSceneDesc = unsafe { ::std::mem::zeroed() };
        check(unsafe { rm_scene_get_desc(raw, &mut desc) }, ptr::null());
        let st = unsafe { rm_scene_upload(self.ctx, &desc) };
        unsafe { rm_scene_free(raw) };
        check(st, self.ctx);
    }

    fn params(fov: f64, height: f64, width: f64, frame_width: usize, frame_height: usize) -> RmParams {
        if (frame_height % 32 != 0) || (frame_width % 32 != 0) {
            println!("Dimensions mismatch") // renderer.rs:49-51
        }
        let mut p: RmParams = unsafe { ::std::mem::zeroed() };
        unsafe { rm_create_renderer(fov, height, width, &mut p) };
        p.frame_width = frame_width as u32; // renderer.rs:53-54 read the FrameBuffer, not the Renderer
        p.frame_height = frame_height as u32;
        p.max_depth = 3; // renderer.rs:262
        p
    }

    fn status(now: ::std::time::Instant, frame_width: usize, frame_height: usize) -> String {
        // renderer.rs:111-125
        let ms = now.elapsed().as_secs() * 1_000 + u64::from(now.elapsed().subsec_nanos()) / 1_000_000;
        let mut buf = [0 as c_char; 256];
        unsafe { rm_format_status(buf.as_mut_ptr(), buf.len(), ms, frame_width as u32, frame_height as u32) };
        let message = unsafe { CStr::from_ptr(buf.as_ptr()) }.to_string_lossy().into_owned();
        println!("{}", message);
        message
    }

    /// Body of `Renderer::render` (renderer.rs:36-126) with the Rayon loop and the serial
    /// scatter replaced by one library call that fills `frame.buffer`'s rows in place.  The rows
    /// below the last whole patch row keep their previous contents (renderer.rs:53): the library
    /// never touches them.
    pub fn render(
        &mut self,
        fov: f64,
        height: f64,
        width: f64,
        frame: &mut FrameBuffer,
        scene: &::scene::Scene,
    ) -> String {
        let now = ::std::time::Instant::now();
        self.upload(scene);
        let p = Gpu::params(fov, height, width, frame.width, frame.height);
        let rows = row_pointers(frame);
        let mut timing = RmTiming::default();
        check(unsafe { rm_render_rows(self.ctx, &p, rows.as_ptr(), &mut timing) }, self.ctx);
        Gpu::status(now, frame.width, frame.height)
    }

    /// `render` with adaptive anti-aliasing: the frame is rendered once, then every pixel that differs from a left / right /
    /// upper / lower neighbour by more than `threshold` in a channel is replaced by the mean of `n` x `n` radiance samples
    /// (`n` in 1..8) -- found, shaded and resolved on the GPU in one library call.  Fills the whole patch rows of
    /// `frame.buffer`; returns the status string and the number of pixels refined.
    pub fn render_antialiased(
        &mut self,
        fov: f64,
        height: f64,
        width: f64,
        frame: &mut FrameBuffer,
        scene: &::scene::Scene,
        n: u32,
        threshold: f64,
    ) -> (String, u32) {
        let now = ::std::time::Instant::now();
        self.upload(scene);
        let p = Gpu::params(fov, height, width, frame.width, frame.height);
        let refine = RmRefine { n: n, _pad: 0, threshold: threshold };
        let rows = frame.height - frame.height % 32;
        let mut flat = vec![0f64; rows * frame.width * 3];
        let mut refined: u32 = 0;
        let mut timing = RmTiming::default();
        check(
            unsafe { rm_render_antialiased(self.ctx, &p, &refine, flat.as_mut_ptr(), &mut refined, &mut timing) },
            self.ctx,
        );
        for y in 0..rows {
            assert!(frame.buffer[y].len() == frame.width, "FrameBuffer: row {} holds {} pixels for a width of {}", y, frame.buffer[y].len(), frame.width);
            for x in 0..frame.width {
                let c = &flat[(y * frame.width + x) * 3..(y * frame.width + x) * 3 + 3];
                frame.buffer[y][x] = Vec3f { x: c[0], y: c[1], z: c[2] };
            }
        }
        (Gpu::status(now, frame.width, frame.height), refined)
    }

    /// `render` through a thin lens: `n_samples` rays a pixel (1..64), each from a point of its own of a lens of radius
    /// `aperture` towards the point its sample ray reaches at the distance `focus` along the view direction -- what lies at
    /// that distance is sharp, the rest blurs with the aperture.  The sample table is the library's (`rm_lens_table`);
    /// sampled, shaded and averaged on the GPU in one library call.  Fills the whole patch rows of `frame.buffer`.
    pub fn render_lens(
        &mut self,
        fov: f64,
        height: f64,
        width: f64,
        frame: &mut FrameBuffer,
        scene: &::scene::Scene,
        aperture: f64,
        focus: f64,
        n_samples: u32,
    ) -> String {
        let now = ::std::time::Instant::now();
        self.upload(scene);
        let p = Gpu::params(fov, height, width, frame.width, frame.height);
        let lens = RmLens { aperture: aperture, focus: focus, n_samples: n_samples, _pad: 0 };
        let mut table = vec![0f64; 4 * 64]; // (room for the most rows there can be)
        check(unsafe { rm_lens_table(n_samples, table.as_mut_ptr()) }, ptr::null());
        let rows = frame.height - frame.height % 32;
        let mut flat = vec![0f64; rows * frame.width * 3 + 1]; // (+ 1: never a dangling frame pointer)
        let mut timing = RmTiming::default();
        check(
            unsafe { rm_render_lens(self.ctx, &p, &lens, table.as_ptr(), flat.as_mut_ptr(), &mut timing) },
            self.ctx,
        );
        for y in 0..rows {
            assert!(frame.buffer[y].len() == frame.width, "FrameBuffer: row {} holds {} pixels for a width of {}", y, frame.buffer[y].len(), frame.width);
            for x in 0..frame.width {
                let c = &flat[(y * frame.width + x) * 3..(y * frame.width + x) * 3 + 3];
                frame.buffer[y][x] = Vec3f { x: c[0], y: c[1], z: c[2] };
            }
        }
        Gpu::status(now, frame.width, frame.height)
    }

    /// A tick of a standing view: `n_samples` (1..64) more lens samples a pixel of the library's unbounded sequence are added
    /// on the GPU to the frame the context keeps, and `frame.buffer` gets the mean of all of them so far; `display`, where
    /// given, gets its `to_vec` bytes (resized to width * height * 3).  The frame begins again when `restart` is set or
    /// anything it depends on changed since the last tick: the renderer, the frame's size, the lens, the camera, the view
    /// direction, the scene.  This is what the window's idle handler calls while no key is pressed.  Fills the
    /// whole patch rows; returns the status string and the samples a pixel in the frame (at most 65536: further ticks
    /// change nothing).
    pub fn render_progressive(
        &mut self,
        fov: f64,
        height: f64,
        width: f64,
        frame: &mut FrameBuffer,
        scene: &::scene::Scene,
        aperture: f64,
        focus: f64,
        n_samples: u32,
        restart: bool,
        display: Option<&mut Vec<u8>>,
    ) -> (String, u32) {
        let now = ::std::time::Instant::now();
        self.upload(scene);
        let p = Gpu::params(fov, height, width, frame.width, frame.height);
        let lens = RmLens { aperture: aperture, focus: focus, n_samples: n_samples, _pad: 0 };
        let rows = frame.height - frame.height % 32;
        let mut flat = vec![0f64; rows * frame.width * 3 + 1]; // (+ 1: never a dangling frame pointer)
        let bytes: *mut u8 = match display {
            Some(d) => {
                d.resize(frame.width * frame.height * 3, 0);
                d.as_mut_ptr()
            }
            None => ptr::null_mut(),
        };
        let mut total: u32 = 0;
        let mut timing = RmTiming::default();
        check(
            unsafe { rm_render_progressive(self.ctx, &p, &lens, if restart { 1 } else { 0 }, flat.as_mut_ptr(), bytes, &mut total, &mut timing) },
            self.ctx,
        );
        for y in 0..rows {
            assert!(frame.buffer[y].len() == frame.width, "FrameBuffer: row {} holds {} pixels for a width of {}", y, frame.buffer[y].len(), frame.width);
            for x in 0..frame.width {
                let c = &flat[(y * frame.width + x) * 3..(y * frame.width + x) * 3 + 3];
                frame.buffer[y][x] = Vec3f { x: c[0], y: c[1], z: c[2] };
            }
        }
        (Gpu::status(now, frame.width, frame.height), total)
    }

    /// The device call under `render_progressive` for a host that keeps its own device buffers (`rm_buffer_alloc`):
    /// `n_samples` rows of `device_table` -- rows of `lens_sequence`, written there by the caller -- are cast for every pixel
    /// and added to `device_sum`, which holds `n_before` samples a pixel already (0: it is not read); the mean goes to
    /// `device_mean` and its display bytes to `device_rgb8` where these are not null.  Asynchronous on `hip_stream`; the
    /// scene is the one the context holds.
    pub fn accumulate_lens(
        &mut self,
        fov: f64,
        height: f64,
        width: f64,
        frame_width: usize,
        frame_height: usize,
        aperture: f64,
        focus: f64,
        n_samples: u32,
        device_table: *const c_void,
        n_before: u32,
        device_sum: *mut c_void,
        device_mean: *mut c_void,
        device_rgb8: *mut c_void,
        hip_stream: *mut c_void,
    ) {
        let p = Gpu::params(fov, height, width, frame_width, frame_height);
        let lens = RmLens { aperture: aperture, focus: focus, n_samples: n_samples, _pad: 0 };
        check(
            unsafe { rm_accumulate_lens_device(self.ctx, &p, &lens, device_table, n_before, device_sum, device_mean, device_rgb8, hip_stream) },
            self.ctx,
        );
    }

    /// Rows `first .. first + count` of the library's unbounded sample sequence, four f64 (dx, dy, u, v) a row.
    pub fn lens_sequence(first: u32, count: u32) -> Vec<f64> {
        let mut table = vec![0f64; 4 * count as usize + 1]; // (+ 1: never a dangling pointer)
        check(unsafe { rm_lens_sequence(first, count, table.as_mut_ptr()) }, ptr::null());
        table.truncate(4 * count as usize);
        table
    }

    /// `render_progressive` with area lights: light l of the scene is a sphere of radius `radii[l]` -- one radius a light, 0 for
    /// a point -- sampled at another point for every sample, so the frame converges to soft shadows.  Beyond what begins a
    /// frame again in `render_progressive`, a changed radius does, and so does a switch between the two calls.
    pub fn render_progressive_soft(
        &mut self,
        fov: f64,
        height: f64,
        width: f64,
        frame: &mut FrameBuffer,
        scene: &::scene::Scene,
        radii: &[f64],
        aperture: f64,
        focus: f64,
        n_samples: u32,
        restart: bool,
        display: Option<&mut Vec<u8>>,
    ) -> (String, u32) {
        let now = ::std::time::Instant::now();
        self.upload(scene);
        let p = Gpu::params(fov, height, width, frame.width, frame.height);
        let lens = RmLens { aperture: aperture, focus: focus, n_samples: n_samples, _pad: 0 };
        let rows = frame.height - frame.height % 32;
        let mut flat = vec![0f64; rows * frame.width * 3 + 1]; // (+ 1: never a dangling frame pointer)
        let bytes: *mut u8 = match display {
            Some(d) => {
                d.resize(frame.width * frame.height * 3, 0);
                d.as_mut_ptr()
            }
            None => ptr::null_mut(),
        };
        let mut total: u32 = 0;
        let mut timing = RmTiming::default();
        check(
            unsafe {
                rm_render_progressive_soft(self.ctx, &p, &lens, radii.as_ptr(), radii.len() as u32, if restart { 1 } else { 0 }, flat.as_mut_ptr(), bytes, &mut total, &mut timing)
            },
            self.ctx,
        );
        for y in 0..rows {
            assert!(frame.buffer[y].len() == frame.width, "FrameBuffer: row {} holds {} pixels for a width of {}", y, frame.buffer[y].len(), frame.width);
            for x in 0..frame.width {
                let c = &flat[(y * frame.width + x) * 3..(y * frame.width + x) * 3 + 3];
                frame.buffer[y][x] = Vec3f { x: c[0], y: c[1], z: c[2] };
            }
        }
        (Gpu::status(now, frame.width, frame.height), total)
    }

    /// The device call under `render_progressive_soft`: `accumulate_lens` with `device_offsets`, `n_samples` x `n_lights` x 3
    /// f64 -- rows of `light_sequence`, or any offsets of the caller's making -- that move light l of sample row s.
    /// `n_lights` is the resident scene's.
    pub fn accumulate_soft(
        &mut self,
        fov: f64,
        height: f64,
        width: f64,
        frame_width: usize,
        frame_height: usize,
        aperture: f64,
        focus: f64,
        n_samples: u32,
        device_table: *const c_void,
        device_offsets: *const c_void,
        n_lights: u32,
        n_before: u32,
        device_sum: *mut c_void,
        device_mean: *mut c_void,
        device_rgb8: *mut c_void,
        hip_stream: *mut c_void,
    ) {
        let p = Gpu::params(fov, height, width, frame_width, frame_height);
        let lens = RmLens { aperture: aperture, focus: focus, n_samples: n_samples, _pad: 0 };
        check(
            unsafe {
                rm_accumulate_soft_device(self.ctx, &p, &lens, device_table, device_offsets, n_lights, n_before, device_sum, device_mean, device_rgb8, hip_stream)
            },
            self.ctx,
        );
    }

    /// Rows `first .. first + count` of the library's light offset sequence for lights of the radii `radii`: three f64 a light,
    /// `radii.len()` lights a row.
    pub fn light_sequence(first: u32, count: u32, radii: &[f64]) -> Vec<f64> {
        let n = 3 * radii.len() * count as usize;
        let mut offsets = vec![0f64; n + 1]; // (+ 1: never a dangling pointer)
        check(unsafe { rm_light_sequence(first, count, radii.as_ptr(), radii.len() as u32, offsets.as_mut_ptr()) }, ptr::null());
        offsets.truncate(n);
        offsets
    }

    /// `render_progressive_soft` with moving spheres: shape k of the scene, a sphere, moves by `velocities[k]` -- one vector a
    /// shape, zero for what is not a sphere -- while the shutter stands open for `shutter`, and every sample sees it at a time of
    /// its own, so the frame converges to a picture blurred along the motion.  `radii`: one radius a light; `None`: point
    /// lights.  Beyond what begins a frame again in `render_progressive_soft`, a changed velocity or shutter does, and so does a
    /// switch between the calls.  Every ray of such a frame tests every primitive: a hierarchy holds for spheres that stand still.
    pub fn render_progressive_motion(
        &mut self,
        fov: f64,
        height: f64,
        width: f64,
        frame: &mut FrameBuffer,
        scene: &::scene::Scene,
        radii: Option<&[f64]>,
        velocities: &[Vec3f],
        shutter: f64,
        aperture: f64,
        focus: f64,
        n_samples: u32,
        restart: bool,
        display: Option<&mut Vec<u8>>,
    ) -> (String, u32) {
        let now = ::std::time::Instant::now();
        self.upload(scene);
        let p = Gpu::params(fov, height, width, frame.width, frame.height);
        let lens = RmLens { aperture: aperture, focus: focus, n_samples: n_samples, _pad: 0 };
        let rows = frame.height - frame.height % 32;
        let mut flat = vec![0f64; rows * frame.width * 3 + 1]; // (+ 1: never a dangling frame pointer)
        let bytes: *mut u8 = match display {
            Some(d) => {
                d.resize(frame.width * frame.height * 3, 0);
                d.as_mut_ptr()
            }
            None => ptr::null_mut(),
        };
        let v: Vec<RmVec3> = velocities.iter().map(|v| RmVec3 { x: v.x, y: v.y, z: v.z }).collect();
        let (radii_ptr, n_lights) = match radii {
            Some(r) => (r.as_ptr(), r.len() as u32),
            None => (ptr::null(), 0),
        };
        let mut total: u32 = 0;
        let mut timing = RmTiming::default();
        check(
            unsafe {
                rm_render_progressive_motion(self.ctx, &p, &lens, radii_ptr, n_lights, v.as_ptr(), v.len() as u32, shutter, if restart { 1 } else { 0 }, flat.as_mut_ptr(), bytes, &mut total, &mut timing)
            },
            self.ctx,
        );
        for y in 0..rows {
            assert!(frame.buffer[y].len() == frame.width, "FrameBuffer: row {} holds {} pixels for a width of {}", y, frame.buffer[y].len(), frame.width);
            for x in 0..frame.width {
                let c = &flat[(y * frame.width + x) * 3..(y * frame.width + x) * 3 + 3];
                frame.buffer[y][x] = Vec3f { x: c[0], y: c[1], z: c[2] };
            }
        }
        (Gpu::status(now, frame.width, frame.height), total)
    }

    /// The device call under `render_progressive_motion`: `accumulate_soft` with `device_shape_offsets`, `n_samples` x `n_shapes`
    /// x 3 f64 -- rows of `motion_sequence`, or any offsets of the caller's making -- that move the sphere that is shape k of
    /// sample row s.  `n_lights` and `n_shapes` are the resident scene's; a caller with point lights passes zeros.
    pub fn accumulate_motion(
        &mut self,
        fov: f64,
        height: f64,
        width: f64,
        frame_width: usize,
        frame_height: usize,
        aperture: f64,
        focus: f64,
        n_samples: u32,
        device_table: *const c_void,
        device_light_offsets: *const c_void,
        n_lights: u32,
        device_shape_offsets: *const c_void,
        n_shapes: u32,
        n_before: u32,
        device_sum: *mut c_void,
        device_mean: *mut c_void,
        device_rgb8: *mut c_void,
        hip_stream: *mut c_void,
    ) {
        let p = Gpu::params(fov, height, width, frame_width, frame_height);
        let lens = RmLens { aperture: aperture, focus: focus, n_samples: n_samples, _pad: 0 };
        check(
            unsafe {
                rm_accumulate_motion_device(self.ctx, &p, &lens, device_table, device_light_offsets, n_lights, device_shape_offsets, n_shapes, n_before, device_sum, device_mean, device_rgb8, hip_stream)
            },
            self.ctx,
        );
    }

    /// `render_progressive_motion` in which every shape moves: a velocity on a polygon or a mesh is obeyed -- the plane point and
    /// the vertices, every triangle's centre and vertices move as the reference's `offset()` moves them, the normals stay.  The
    /// frame is not `render_progressive_motion`'s: a switch between the two begins it again.
    pub fn render_progressive_moving(
        &mut self,
        fov: f64,
        height: f64,
        width: f64,
        frame: &mut FrameBuffer,
        scene: &::scene::Scene,
        radii: Option<&[f64]>,
        velocities: &[Vec3f],
        shutter: f64,
        aperture: f64,
        focus: f64,
        n_samples: u32,
        restart: bool,
        display: Option<&mut Vec<u8>>,
    ) -> (String, u32) {
        let now = ::std::time::Instant::now();
        self.upload(scene);
        let p = Gpu::params(fov, height, width, frame.width, frame.height);
        let lens = RmLens { aperture: aperture, focus: focus, n_samples: n_samples, _pad: 0 };
        let rows = frame.height - frame.height % 32;
        let mut flat = vec![0f64; rows * frame.width * 3 + 1]; // (+ 1: never a dangling frame pointer)
        let bytes: *mut u8 = match display {
            Some(d) => {
                d.resize(frame.width * frame.height * 3, 0);
                d.as_mut_ptr()
            }
            None => ptr::null_mut(),
        };
        let v: Vec<RmVec3> = velocities.iter().map(|v| RmVec3 { x: v.x, y: v.y, z: v.z }).collect();
        let (radii_ptr, n_lights) = match radii {
            Some(r) => (r.as_ptr(), r.len() as u32),
            None => (ptr::null(), 0),
        };
        let mut total: u32 = 0;
        let mut timing = RmTiming::default();
        check(
            unsafe {
                rm_render_progressive_moving(self.ctx, &p, &lens, radii_ptr, n_lights, v.as_ptr(), v.len() as u32, shutter, if restart { 1 } else { 0 }, flat.as_mut_ptr(), bytes, &mut total, &mut timing)
            },
            self.ctx,
        );
        for y in 0..rows {
            assert!(frame.buffer[y].len() == frame.width, "FrameBuffer: row {} holds {} pixels for a width of {}", y, frame.buffer[y].len(), frame.width);
            for x in 0..frame.width {
                let c = &flat[(y * frame.width + x) * 3..(y * frame.width + x) * 3 + 3];
                frame.buffer[y][x] = Vec3f { x: c[0], y: c[1], z: c[2] };
            }
        }
        (Gpu::status(now, frame.width, frame.height), total)
    }

    /// The device call under `render_progressive_moving`: `accumulate_motion` in which the rows of every shape are read and move
    /// it, sphere, polygon or mesh.  `device_shape_offsets` must not be null when the scene holds any shape.
    pub fn accumulate_moving(
        &mut self,
        fov: f64,
        height: f64,
        width: f64,
        frame_width: usize,
        frame_height: usize,
        aperture: f64,
        focus: f64,
        n_samples: u32,
        device_table: *const c_void,
        device_light_offsets: *const c_void,
        n_lights: u32,
        device_shape_offsets: *const c_void,
        n_shapes: u32,
        n_before: u32,
        device_sum: *mut c_void,
        device_mean: *mut c_void,
        device_rgb8: *mut c_void,
        hip_stream: *mut c_void,
    ) {
        let p = Gpu::params(fov, height, width, frame_width, frame_height);
        let lens = RmLens { aperture: aperture, focus: focus, n_samples: n_samples, _pad: 0 };
        check(
            unsafe {
                rm_accumulate_moving_device(self.ctx, &p, &lens, device_table, device_light_offsets, n_lights, device_shape_offsets, n_shapes, n_before, device_sum, device_mean, device_rgb8, hip_stream)
            },
            self.ctx,
        );
    }

    /// A swept hierarchy of the uploaded scene: its hierarchies' boxes refitted to bound every primitive at every offset within
    /// `lo[k] .. hi[k]` of its shape k (three f64 a shape each, finite, lo <= hi).  Stale once another scene is uploaded; hand it
    /// back with `swept_free`.
    pub fn swept(&mut self, lo: &[f64], hi: &[f64]) -> *mut RmSwept {
        assert!(lo.len() == hi.len() && lo.len() % 3 == 0, "swept: lo and hi hold three numbers a shape");
        let mut out: *mut RmSwept = std::ptr::null_mut();
        check(unsafe { rm_swept_build(self.ctx, lo.as_ptr(), hi.as_ptr(), (lo.len() / 3) as u32, &mut out) }, self.ctx);
        out
    }

    /// Releases a handle of `swept` (waits for the device).
    pub fn swept_free(&mut self, swept: *mut RmSwept) {
        unsafe { rm_swept_free(self.ctx, swept) };
    }

    /// The per-shape componentwise minimum and maximum of a host shape offset table of `rows` rows: (lo, hi).
    pub fn swept_extents(table: &[f64], rows: u32, n_shapes: u32) -> (Vec<f64>, Vec<f64>) {
        assert!(table.len() == 3 * rows as usize * n_shapes as usize, "swept_extents: the table holds rows x n_shapes x 3 numbers");
        let (mut lo, mut hi) = (vec![0f64; 3 * n_shapes as usize], vec![0f64; 3 * n_shapes as usize]);
        check(unsafe { rm_swept_extents(table.as_ptr(), rows, n_shapes, lo.as_mut_ptr(), hi.as_mut_ptr()) }, std::ptr::null());
        (lo, hi)
    }

    /// The extents that hold every row of `motion_sequence(.., velocities, shutter)`: (lo, hi).
    pub fn swept_motion_extents(velocities: &[Vec3f], shutter: f64) -> (Vec<f64>, Vec<f64>) {
        let v: Vec<RmVec3> = velocities.iter().map(|v| RmVec3 { x: v.x, y: v.y, z: v.z }).collect();
        let (mut lo, mut hi) = (vec![0f64; 3 * v.len()], vec![0f64; 3 * v.len()]);
        check(unsafe { rm_swept_motion_extents(v.as_ptr(), v.len() as u32, shutter, lo.as_mut_ptr(), hi.as_mut_ptr()) }, std::ptr::null());
        (lo, hi)
    }

    /// `accumulate_moving` through the swept hierarchy `swept`, whose extents hold every row of the shape table: the same bytes,
    /// with the scene's hierarchies walked.
    pub fn accumulate_swept(
        &mut self,
        fov: f64,
        height: f64,
        width: f64,
        frame_width: usize,
        frame_height: usize,
        aperture: f64,
        focus: f64,
        n_samples: u32,
        device_table: *const c_void,
        device_light_offsets: *const c_void,
        n_lights: u32,
        device_shape_offsets: *const c_void,
        n_shapes: u32,
        swept: *const RmSwept,
        n_before: u32,
        device_sum: *mut c_void,
        device_mean: *mut c_void,
        device_rgb8: *mut c_void,
        hip_stream: *mut c_void,
    ) {
        let p = Gpu::params(fov, height, width, frame_width, frame_height);
        let lens = RmLens { aperture: aperture, focus: focus, n_samples: n_samples, _pad: 0 };
        check(
            unsafe {
                rm_accumulate_swept_device(self.ctx, &p, &lens, device_table, device_light_offsets, n_lights, device_shape_offsets, n_shapes, swept, n_before, device_sum, device_mean, device_rgb8, hip_stream)
            },
            self.ctx,
        );
    }

    /// `accumulate_converging_moving` through the swept hierarchy `swept`.
    pub fn accumulate_converging_swept(
        &mut self,
        fov: f64,
        height: f64,
        width: f64,
        frame_width: usize,
        frame_height: usize,
        aperture: f64,
        focus: f64,
        n_samples: u32,
        converge: RmConverge,
        device_table: *const c_void,
        table_rows: u32,
        device_light_offsets: *const c_void,
        n_lights: u32,
        device_shape_offsets: *const c_void,
        n_shapes: u32,
        swept: *const RmSwept,
        fresh: bool,
        buffers: RmConvergeFrame,
        hip_stream: *mut c_void,
    ) {
        let p = Gpu::params(fov, height, width, frame_width, frame_height);
        let lens = RmLens { aperture: aperture, focus: focus, n_samples: n_samples, _pad: 0 };
        check(
            unsafe {
                rm_accumulate_converging_swept_device(self.ctx, &p, &lens, &converge, device_table, table_rows, device_light_offsets, n_lights, device_shape_offsets, n_shapes, swept, if fresh { 1 } else { 0 }, &buffers, hip_stream)
            },
            self.ctx,
        );
    }

    /// Rows `first .. first + count` of the library's shape offset sequence for shapes of the velocities `velocities` and a
    /// shutter open for `shutter`: three f64 a shape, `velocities.len()` shapes a row.
    pub fn motion_sequence(first: u32, count: u32, velocities: &[Vec3f], shutter: f64) -> Vec<f64> {
        let n = 3 * velocities.len() * count as usize;
        let v: Vec<RmVec3> = velocities.iter().map(|v| RmVec3 { x: v.x, y: v.y, z: v.z }).collect();
        let mut offsets = vec![0f64; n + 1]; // (+ 1: never a dangling pointer)
        check(unsafe { rm_motion_sequence(first, count, v.as_ptr(), v.len() as u32, shutter, offsets.as_mut_ptr()) }, ptr::null());
        offsets.truncate(n);
        offsets
    }

    /// A tick of a converging frame: `render_progressive` -- with area lights where `radii` is given, one radius a light; `None`:
    /// point lights -- that casts its `n_samples` more samples only for the pixels still noisy and their neighbours.  A pixel is
    /// settled once it has `converge.min_samples` samples and the standard error of the mean of r + g + b is at most
    /// `converge.tolerance`; none gets more than `converge.max_samples`.  The frame is the context's own for this call --
    /// `render_progressive`'s is left alone -- and begins again as `render_progressive_soft`'s does; `converge` and `n_samples`
    /// may change while it goes on.  Returns the status string and the tick's report: `listed == 0` says the picture is
    /// finished, and further ticks launch nothing.
    pub fn render_converging(
        &mut self,
        fov: f64,
        height: f64,
        width: f64,
        frame: &mut FrameBuffer,
        scene: &::scene::Scene,
        converge: RmConverge,
        radii: Option<&[f64]>,
        aperture: f64,
        focus: f64,
        n_samples: u32,
        restart: bool,
        display: Option<&mut Vec<u8>>,
    ) -> (String, RmConvergeReport) {
        let now = ::std::time::Instant::now();
        self.upload(scene);
        let p = Gpu::params(fov, height, width, frame.width, frame.height);
        let lens = RmLens { aperture: aperture, focus: focus, n_samples: n_samples, _pad: 0 };
        let rows = frame.height - frame.height % 32;
        let mut flat = vec![0f64; rows * frame.width * 3 + 1]; // (+ 1: never a dangling frame pointer)
        let bytes: *mut u8 = match display {
            Some(d) => {
                d.resize(frame.width * frame.height * 3, 0);
                d.as_mut_ptr()
            }
            None => ptr::null_mut(),
        };
        let (radii_ptr, n_lights) = match radii {
            Some(r) => (r.as_ptr(), r.len() as u32),
            None => (ptr::null(), 0),
        };
        let mut report = RmConvergeReport::default();
        let mut timing = RmTiming::default();
        check(
            unsafe {
                rm_render_converging(self.ctx, &p, &lens, &converge, radii_ptr, n_lights, if restart { 1 } else { 0 }, flat.as_mut_ptr(), bytes, &mut report, &mut timing)
            },
            self.ctx,
        );
        for y in 0..rows {
            assert!(frame.buffer[y].len() == frame.width, "FrameBuffer: row {} holds {} pixels for a width of {}", y, frame.buffer[y].len(), frame.width);
            for x in 0..frame.width {
                let c = &flat[(y * frame.width + x) * 3..(y * frame.width + x) * 3 + 3];
                frame.buffer[y][x] = Vec3f { x: c[0], y: c[1], z: c[2] };
            }
        }
        (Gpu::status(now, frame.width, frame.height), report)
    }

    /// `render_progressive_soft` with one bounce of diffuse light: where a sample first hits a surface that is not glass, one more
    /// ray leaves it in a cosine-distributed direction, and what it brings back, times `strength` and the surface's diffusion and
    /// diffuse colour, is added.  `radii`: one radius a light; `None`: point lights.  Static scene, standing camera.  Beyond what
    /// begins a frame again in `render_progressive_soft`, a changed strength does, and so does a switch between the calls.
    pub fn render_progressive_bounce(
        &mut self,
        fov: f64,
        height: f64,
        width: f64,
        frame: &mut FrameBuffer,
        scene: &::scene::Scene,
        strength: f64,
        radii: Option<&[f64]>,
        aperture: f64,
        focus: f64,
        n_samples: u32,
        restart: bool,
        display: Option<&mut Vec<u8>>,
    ) -> (String, u32) {
        let now = ::std::time::Instant::now();
        self.upload(scene);
        let p = Gpu::params(fov, height, width, frame.width, frame.height);
        let lens = RmLens { aperture: aperture, focus: focus, n_samples: n_samples, _pad: 0 };
        let rows = frame.height - frame.height % 32;
        let mut flat = vec![0f64; rows * frame.width * 3 + 1]; // (+ 1: never a dangling frame pointer)
        let bytes: *mut u8 = match display {
            Some(d) => {
                d.resize(frame.width * frame.height * 3, 0);
                d.as_mut_ptr()
            }
            None => ptr::null_mut(),
        };
        let (radii_ptr, n_lights) = match radii {
            Some(r) => (r.as_ptr(), r.len() as u32),
            None => (ptr::null(), 0),
        };
        let mut total: u32 = 0;
        let mut timing = RmTiming::default();
        check(
            unsafe {
                rm_render_progressive_bounce(self.ctx, &p, &lens, radii_ptr, n_lights, strength, if restart { 1 } else { 0 }, flat.as_mut_ptr(), bytes, &mut total, &mut timing)
            },
            self.ctx,
        );
        for y in 0..rows {
            assert!(frame.buffer[y].len() == frame.width, "FrameBuffer: row {} holds {} pixels for a width of {}", y, frame.buffer[y].len(), frame.width);
            for x in 0..frame.width {
                let c = &flat[(y * frame.width + x) * 3..(y * frame.width + x) * 3 + 3];
                frame.buffer[y][x] = Vec3f { x: c[0], y: c[1], z: c[2] };
            }
        }
        (Gpu::status(now, frame.width, frame.height), total)
    }

    /// `render_converging` with one bounce of diffuse light, as `render_progressive_bounce` adds it.  The frame is
    /// `render_converging`'s own: beyond what begins it again there, a changed strength does, a switch between the two calls
    /// does, and every camera move does, history or not.
    pub fn render_converging_bounce(
        &mut self,
        fov: f64,
        height: f64,
        width: f64,
        frame: &mut FrameBuffer,
        scene: &::scene::Scene,
        converge: RmConverge,
        strength: f64,
        radii: Option<&[f64]>,
        aperture: f64,
        focus: f64,
        n_samples: u32,
        restart: bool,
        display: Option<&mut Vec<u8>>,
    ) -> (String, RmConvergeReport) {
        let now = ::std::time::Instant::now();
        self.upload(scene);
        let p = Gpu::params(fov, height, width, frame.width, frame.height);
        let lens = RmLens { aperture: aperture, focus: focus, n_samples: n_samples, _pad: 0 };
        let rows = frame.height - frame.height % 32;
        let mut flat = vec![0f64; rows * frame.width * 3 + 1]; // (+ 1: never a dangling frame pointer)
        let bytes: *mut u8 = match display {
            Some(d) => {
                d.resize(frame.width * frame.height * 3, 0);
                d.as_mut_ptr()
            }
            None => ptr::null_mut(),
        };
        let (radii_ptr, n_lights) = match radii {
            Some(r) => (r.as_ptr(), r.len() as u32),
            None => (ptr::null(), 0),
        };
        let mut report = RmConvergeReport::default();
        let mut timing = RmTiming::default();
        check(
            unsafe {
                rm_render_converging_bounce(self.ctx, &p, &lens, &converge, radii_ptr, n_lights, strength, if restart { 1 } else { 0 }, flat.as_mut_ptr(), bytes, &mut report, &mut timing)
            },
            self.ctx,
        );
        for y in 0..rows {
            assert!(frame.buffer[y].len() == frame.width, "FrameBuffer: row {} holds {} pixels for a width of {}", y, frame.buffer[y].len(), frame.width);
            for x in 0..frame.width {
                let c = &flat[(y * frame.width + x) * 3..(y * frame.width + x) * 3 + 3];
                frame.buffer[y][x] = Vec3f { x: c[0], y: c[1], z: c[2] };
            }
        }
        (Gpu::status(now, frame.width, frame.height), report)
    }

    /// The device call under `render_progressive_bounce`: `accumulate_soft` with `device_bounce`, `n_samples` x 2 f64 -- rows of
    /// `bounce_sequence`, or any points of [0, 1) of the caller's making -- and the strength.
    pub fn accumulate_bounce(
        &mut self,
        fov: f64,
        height: f64,
        width: f64,
        frame_width: usize,
        frame_height: usize,
        aperture: f64,
        focus: f64,
        n_samples: u32,
        device_table: *const c_void,
        device_offsets: *const c_void,
        n_lights: u32,
        device_bounce: *const c_void,
        strength: f64,
        n_before: u32,
        device_sum: *mut c_void,
        device_mean: *mut c_void,
        device_rgb8: *mut c_void,
        hip_stream: *mut c_void,
    ) {
        let p = Gpu::params(fov, height, width, frame_width, frame_height);
        let lens = RmLens { aperture: aperture, focus: focus, n_samples: n_samples, _pad: 0 };
        check(
            unsafe {
                rm_accumulate_bounce_device(self.ctx, &p, &lens, device_table, device_offsets, n_lights, device_bounce, strength, n_before, device_sum, device_mean, device_rgb8, hip_stream)
            },
            self.ctx,
        );
    }

    /// The device call under `render_converging_bounce`: `accumulate_converging` with `device_bounce`, `table_rows` x 2 f64, and
    /// the strength.
    pub fn accumulate_converging_bounce(
        &mut self,
        fov: f64,
        height: f64,
        width: f64,
        frame_width: usize,
        frame_height: usize,
        aperture: f64,
        focus: f64,
        n_samples: u32,
        converge: RmConverge,
        device_table: *const c_void,
        table_rows: u32,
        device_offsets: *const c_void,
        n_lights: u32,
        device_bounce: *const c_void,
        strength: f64,
        fresh: bool,
        buffers: RmConvergeFrame,
        hip_stream: *mut c_void,
    ) {
        let p = Gpu::params(fov, height, width, frame_width, frame_height);
        let lens = RmLens { aperture: aperture, focus: focus, n_samples: n_samples, _pad: 0 };
        check(
            unsafe {
                rm_accumulate_converging_bounce_device(self.ctx, &p, &lens, &converge, device_table, table_rows, device_offsets, n_lights, device_bounce, strength, if fresh { 1 } else { 0 }, &buffers, hip_stream)
            },
            self.ctx,
        );
    }

    /// Rows `first .. first + count` of the library's bounce sequence: two f64 a row, points of [0, 1).
    pub fn bounce_sequence(first: u32, count: u32) -> Vec<f64> {
        let n = 2 * count as usize;
        let mut table = vec![0f64; n + 1]; // (+ 1: never a dangling pointer)
        check(unsafe { rm_bounce_sequence(first, count, table.as_mut_ptr()) }, ptr::null());
        table.truncate(n);
        table
    }

    /// The device call under `render_converging` for a host that keeps its own device buffers (`rm_buffer_alloc`): one pass
    /// over `buffers` -- the pixels still noisy and their neighbours are listed in `buffers.workspace`
    /// (`converge_workspace` bytes) and sampled, each from the row of `device_table` its own count says.  `device_table`
    /// holds the first `table_rows >= converge.max_samples` rows of `lens_sequence`, `device_offsets` as many of
    /// `light_sequence` or null for point lights.  With `fresh` the buffers are not read.  Asynchronous on `hip_stream`.
    pub fn accumulate_converging(
        &mut self,
        fov: f64,
        height: f64,
        width: f64,
        frame_width: usize,
        frame_height: usize,
        aperture: f64,
        focus: f64,
        n_samples: u32,
        converge: RmConverge,
        device_table: *const c_void,
        table_rows: u32,
        device_offsets: *const c_void,
        n_lights: u32,
        fresh: bool,
        buffers: RmConvergeFrame,
        hip_stream: *mut c_void,
    ) {
        let p = Gpu::params(fov, height, width, frame_width, frame_height);
        let lens = RmLens { aperture: aperture, focus: focus, n_samples: n_samples, _pad: 0 };
        check(
            unsafe {
                rm_accumulate_converging_device(self.ctx, &p, &lens, &converge, device_table, table_rows, device_offsets, n_lights, if fresh { 1 } else { 0 }, &buffers, hip_stream)
            },
            self.ctx,
        );
    }

    /// `render_converging` with moving spheres: shape k of the scene, a sphere, moves by `velocities[k]` -- one vector a shape,
    /// zero for what is not a sphere -- while the shutter stands open for `shutter`, and every sample sees it at a time of its
    /// own; only the pixels still noisy, the blurred band among them, go on being sampled.  The frame is `render_converging`'s
    /// own: beyond what begins it again there, a changed velocity or shutter does, and so does a switch between the two calls.
    /// Every ray of such a frame tests every primitive: a hierarchy holds for spheres that stand still.
    pub fn render_converging_motion(
        &mut self,
        fov: f64,
        height: f64,
        width: f64,
        frame: &mut FrameBuffer,
        scene: &::scene::Scene,
        converge: RmConverge,
        radii: Option<&[f64]>,
        velocities: &[Vec3f],
        shutter: f64,
        aperture: f64,
        focus: f64,
        n_samples: u32,
        restart: bool,
        display: Option<&mut Vec<u8>>,
    ) -> (String, RmConvergeReport) {
        let now = ::std::time::Instant::now();
        self.upload(scene);
        let p = Gpu::params(fov, height, width, frame.width, frame.height);
        let lens = RmLens { aperture: aperture, focus: focus, n_samples: n_samples, _pad: 0 };
        let rows = frame.height - frame.height % 32;
        let mut flat = vec![0f64; rows * frame.width * 3 + 1]; // (+ 1: never a dangling frame pointer)
        let bytes: *mut u8 = match display {
            Some(d) => {
                d.resize(frame.width * frame.height * 3, 0);
                d.as_mut_ptr()
            }
            None => ptr::null_mut(),
        };
        let v: Vec<RmVec3> = velocities.iter().map(|v| RmVec3 { x: v.x, y: v.y, z: v.z }).collect();
        let (radii_ptr, n_lights) = match radii {
            Some(r) => (r.as_ptr(), r.len() as u32),
            None => (ptr::null(), 0),
        };
        let mut report = RmConvergeReport::default();
        let mut timing = RmTiming::default();
        check(
            unsafe {
                rm_render_converging_motion(self.ctx, &p, &lens, &converge, radii_ptr, n_lights, v.as_ptr(), v.len() as u32, shutter, if restart { 1 } else { 0 }, flat.as_mut_ptr(), bytes, &mut report, &mut timing)
            },
            self.ctx,
        );
        for y in 0..rows {
            assert!(frame.buffer[y].len() == frame.width, "FrameBuffer: row {} holds {} pixels for a width of {}", y, frame.buffer[y].len(), frame.width);
            for x in 0..frame.width {
                let c = &flat[(y * frame.width + x) * 3..(y * frame.width + x) * 3 + 3];
                frame.buffer[y][x] = Vec3f { x: c[0], y: c[1], z: c[2] };
            }
        }
        (Gpu::status(now, frame.width, frame.height), report)
    }

    /// The device call under `render_converging_motion`: `accumulate_converging` with `device_shape_offsets`, `table_rows` x
    /// `n_shapes` x 3 f64 -- rows of `motion_sequence`, or any offsets of the caller's making -- that move the sphere that is
    /// shape k for the sample that is row r of the tables.  `n_lights` and `n_shapes` are the resident scene's; a caller with
    /// point lights passes zeros.
    pub fn accumulate_converging_motion(
        &mut self,
        fov: f64,
        height: f64,
        width: f64,
        frame_width: usize,
        frame_height: usize,
        aperture: f64,
        focus: f64,
        n_samples: u32,
        converge: RmConverge,
        device_table: *const c_void,
        table_rows: u32,
        device_light_offsets: *const c_void,
        n_lights: u32,
        device_shape_offsets: *const c_void,
        n_shapes: u32,
        fresh: bool,
        buffers: RmConvergeFrame,
        hip_stream: *mut c_void,
    ) {
        let p = Gpu::params(fov, height, width, frame_width, frame_height);
        let lens = RmLens { aperture: aperture, focus: focus, n_samples: n_samples, _pad: 0 };
        check(
            unsafe {
                rm_accumulate_converging_motion_device(self.ctx, &p, &lens, &converge, device_table, table_rows, device_light_offsets, n_lights, device_shape_offsets, n_shapes, if fresh { 1 } else { 0 }, &buffers, hip_stream)
            },
            self.ctx,
        );
    }

    /// `render_converging_motion` in which every shape moves: a velocity on a polygon or a mesh is obeyed -- the plane point and
    /// the vertices, every triangle's centre and vertices move as the reference's `offset()` moves them, the normals stay.  The
    /// frame is not `render_converging_motion`'s: a switch between the two begins it again.
    pub fn render_converging_moving(
        &mut self,
        fov: f64,
        height: f64,
        width: f64,
        frame: &mut FrameBuffer,
        scene: &::scene::Scene,
        converge: RmConverge,
        radii: Option<&[f64]>,
        velocities: &[Vec3f],
        shutter: f64,
        aperture: f64,
        focus: f64,
        n_samples: u32,
        restart: bool,
        display: Option<&mut Vec<u8>>,
    ) -> (String, RmConvergeReport) {
        let now = ::std::time::Instant::now();
        self.upload(scene);
        let p = Gpu::params(fov, height, width, frame.width, frame.height);
        let lens = RmLens { aperture: aperture, focus: focus, n_samples: n_samples, _pad: 0 };
        let rows = frame.height - frame.height % 32;
        let mut flat = vec![0f64; rows * frame.width * 3 + 1]; // (+ 1: never a dangling frame pointer)
        let bytes: *mut u8 = match display {
            Some(d) => {
                d.resize(frame.width * frame.height * 3, 0);
                d.as_mut_ptr()
            }
            None => ptr::null_mut(),
        };
        let v: Vec<RmVec3> = velocities.iter().map(|v| RmVec3 { x: v.x, y: v.y, z: v.z }).collect();
        let (radii_ptr, n_lights) = match radii {
            Some(r) => (r.as_ptr(), r.len() as u32),
            None => (ptr::null(), 0),
        };
        let mut report = RmConvergeReport::default();
        let mut timing = RmTiming::default();
        check(
            unsafe {
                rm_render_converging_moving(self.ctx, &p, &lens, &converge, radii_ptr, n_lights, v.as_ptr(), v.len() as u32, shutter, if restart { 1 } else { 0 }, flat.as_mut_ptr(), bytes, &mut report, &mut timing)
            },
            self.ctx,
        );
        for y in 0..rows {
            assert!(frame.buffer[y].len() == frame.width, "FrameBuffer: row {} holds {} pixels for a width of {}", y, frame.buffer[y].len(), frame.width);
            for x in 0..frame.width {
                let c = &flat[(y * frame.width + x) * 3..(y * frame.width + x) * 3 + 3];
                frame.buffer[y][x] = Vec3f { x: c[0], y: c[1], z: c[2] };
            }
        }
        (Gpu::status(now, frame.width, frame.height), report)
    }

    /// The device call under `render_converging_moving`: `accumulate_converging_motion` in which the row of every shape is read
    /// -- sphere, polygon or mesh -- so `device_shape_offsets` may be null only for a scene with no shape.
    pub fn accumulate_converging_moving(
        &mut self,
        fov: f64,
        height: f64,
        width: f64,
        frame_width: usize,
        frame_height: usize,
        aperture: f64,
        focus: f64,
        n_samples: u32,
        converge: RmConverge,
        device_table: *const c_void,
        table_rows: u32,
        device_light_offsets: *const c_void,
        n_lights: u32,
        device_shape_offsets: *const c_void,
        n_shapes: u32,
        fresh: bool,
        buffers: RmConvergeFrame,
        hip_stream: *mut c_void,
    ) {
        let p = Gpu::params(fov, height, width, frame_width, frame_height);
        let lens = RmLens { aperture: aperture, focus: focus, n_samples: n_samples, _pad: 0 };
        check(
            unsafe {
                rm_accumulate_converging_moving_device(self.ctx, &p, &lens, &converge, device_table, table_rows, device_light_offsets, n_lights, device_shape_offsets, n_shapes, if fresh { 1 } else { 0 }, &buffers, hip_stream)
            },
            self.ctx,
        );
    }

    /// `render_progressive_moving` with a moving camera: the camera moves by `motion.velocity` and turns by the rates of `motion`
    /// while the shutter stands open for `shutter`, and every sample sees the scene from a camera of its own.  `velocities`:
    /// `None` where no shape moves -- the scene keeps its hierarchy then.  The frame is the call's own: a switch to or from
    /// another progressive call begins it again, and so does a changed motion or shutter.
    pub fn render_progressive_camera(
        &mut self,
        fov: f64,
        height: f64,
        width: f64,
        frame: &mut FrameBuffer,
        scene: &::scene::Scene,
        radii: Option<&[f64]>,
        velocities: Option<&[Vec3f]>,
        shutter: f64,
        motion: RmCameraMotion,
        aperture: f64,
        focus: f64,
        n_samples: u32,
        restart: bool,
        display: Option<&mut Vec<u8>>,
    ) -> (String, u32) {
        let now = ::std::time::Instant::now();
        self.upload(scene);
        let p = Gpu::params(fov, height, width, frame.width, frame.height);
        let lens = RmLens { aperture: aperture, focus: focus, n_samples: n_samples, _pad: 0 };
        let rows = frame.height - frame.height % 32;
        let mut flat = vec![0f64; rows * frame.width * 3 + 1]; // (+ 1: never a dangling frame pointer)
        let bytes: *mut u8 = match display {
            Some(d) => {
                d.resize(frame.width * frame.height * 3, 0);
                d.as_mut_ptr()
            }
            None => ptr::null_mut(),
        };
        let v: Option<Vec<RmVec3>> = velocities.map(|vs| vs.iter().map(|v| RmVec3 { x: v.x, y: v.y, z: v.z }).collect());
        let (v_ptr, n_shapes) = match v {
            Some(ref v) => (v.as_ptr(), v.len() as u32),
            None => (ptr::null(), 0),
        };
        let (radii_ptr, n_lights) = match radii {
            Some(r) => (r.as_ptr(), r.len() as u32),
            None => (ptr::null(), 0),
        };
        let mut total: u32 = 0;
        let mut timing = RmTiming::default();
        check(
            unsafe {
                rm_render_progressive_camera(self.ctx, &p, &lens, radii_ptr, n_lights, v_ptr, n_shapes, shutter, &motion, if restart { 1 } else { 0 }, flat.as_mut_ptr(), bytes, &mut total, &mut timing)
            },
            self.ctx,
        );
        for y in 0..rows {
            assert!(frame.buffer[y].len() == frame.width, "FrameBuffer: row {} holds {} pixels for a width of {}", y, frame.buffer[y].len(), frame.width);
            for x in 0..frame.width {
                let c = &flat[(y * frame.width + x) * 3..(y * frame.width + x) * 3 + 3];
                frame.buffer[y][x] = Vec3f { x: c[0], y: c[1], z: c[2] };
            }
        }
        (Gpu::status(now, frame.width, frame.height), total)
    }

    /// The device call under `render_progressive_camera`: `accumulate_moving` with `device_camera_rows`, `n_samples` x 12 f64 --
    /// rows of `camera_sequence`, or any of the caller's making -- whose row s is the camera of sample s.  A null
    /// `device_shape_offsets` says that no shape moves.
    pub fn accumulate_camera(
        &mut self,
        fov: f64,
        height: f64,
        width: f64,
        frame_width: usize,
        frame_height: usize,
        aperture: f64,
        focus: f64,
        n_samples: u32,
        device_table: *const c_void,
        device_camera_rows: *const c_void,
        device_light_offsets: *const c_void,
        n_lights: u32,
        device_shape_offsets: *const c_void,
        n_shapes: u32,
        n_before: u32,
        device_sum: *mut c_void,
        device_mean: *mut c_void,
        device_rgb8: *mut c_void,
        hip_stream: *mut c_void,
    ) {
        let p = Gpu::params(fov, height, width, frame_width, frame_height);
        let lens = RmLens { aperture: aperture, focus: focus, n_samples: n_samples, _pad: 0 };
        check(
            unsafe {
                rm_accumulate_camera_device(self.ctx, &p, &lens, device_table, device_camera_rows, device_light_offsets, n_lights, device_shape_offsets, n_shapes, n_before, device_sum, device_mean, device_rgb8, hip_stream)
            },
            self.ctx,
        );
    }

    /// Rows `first .. first + count` of the library's camera sequence: twelve f64 a row -- the offset, right, up, forward -- for a
    /// camera that moves by `motion` from `basis` while the shutter stands open for `shutter`.  Row s is at the time
    /// `motion_sequence` gives row s.
    pub fn camera_sequence(first: u32, count: u32, motion: RmCameraMotion, basis: RmCameraBasis, shutter: f64) -> Vec<f64> {
        let n = 12 * count as usize;
        let mut rows = vec![0f64; n + 1]; // (+ 1: never a dangling pointer)
        check(unsafe { rm_camera_sequence(first, count, &motion, &basis, shutter, rows.as_mut_ptr()) }, ptr::null());
        rows.truncate(n);
        rows
    }

    /// `render_converging_moving` with a moving camera: `motion` and `velocities` as `render_progressive_camera`'s; only the
    /// pixels still noisy go on being sampled.  The frame is the call's own.
    pub fn render_converging_camera(
        &mut self,
        fov: f64,
        height: f64,
        width: f64,
        frame: &mut FrameBuffer,
        scene: &::scene::Scene,
        converge: RmConverge,
        radii: Option<&[f64]>,
        velocities: Option<&[Vec3f]>,
        shutter: f64,
        motion: RmCameraMotion,
        aperture: f64,
        focus: f64,
        n_samples: u32,
        restart: bool,
        display: Option<&mut Vec<u8>>,
    ) -> (String, RmConvergeReport) {
        let now = ::std::time::Instant::now();
        self.upload(scene);
        let p = Gpu::params(fov, height, width, frame.width, frame.height);
        let lens = RmLens { aperture: aperture, focus: focus, n_samples: n_samples, _pad: 0 };
        let rows = frame.height - frame.height % 32;
        let mut flat = vec![0f64; rows * frame.width * 3 + 1]; // (+ 1: never a dangling frame pointer)
        let bytes: *mut u8 = match display {
            Some(d) => {
                d.resize(frame.width * frame.height * 3, 0);
                d.as_mut_ptr()
            }
            None => ptr::null_mut(),
        };
        let v: Option<Vec<RmVec3>> = velocities.map(|vs| vs.iter().map(|v| RmVec3 { x: v.x, y: v.y, z: v.z }).collect());
        let (v_ptr, n_shapes) = match v {
            Some(ref v) => (v.as_ptr(), v.len() as u32),
            None => (ptr::null(), 0),
        };
        let (radii_ptr, n_lights) = match radii {
            Some(r) => (r.as_ptr(), r.len() as u32),
            None => (ptr::null(), 0),
        };
        let mut report = RmConvergeReport::default();
        let mut timing = RmTiming::default();
        check(
            unsafe {
                rm_render_converging_camera(self.ctx, &p, &lens, &converge, radii_ptr, n_lights, v_ptr, n_shapes, shutter, &motion, if restart { 1 } else { 0 }, flat.as_mut_ptr(), bytes, &mut report, &mut timing)
            },
            self.ctx,
        );
        for y in 0..rows {
            assert!(frame.buffer[y].len() == frame.width, "FrameBuffer: row {} holds {} pixels for a width of {}", y, frame.buffer[y].len(), frame.width);
            for x in 0..frame.width {
                let c = &flat[(y * frame.width + x) * 3..(y * frame.width + x) * 3 + 3];
                frame.buffer[y][x] = Vec3f { x: c[0], y: c[1], z: c[2] };
            }
        }
        (Gpu::status(now, frame.width, frame.height), report)
    }

    /// The device call under `render_converging_camera`: `accumulate_converging_moving` with `device_camera_rows`, `table_rows` x
    /// 12 f64.  A null `device_shape_offsets` says that no shape moves.
    pub fn accumulate_converging_camera(
        &mut self,
        fov: f64,
        height: f64,
        width: f64,
        frame_width: usize,
        frame_height: usize,
        aperture: f64,
        focus: f64,
        n_samples: u32,
        converge: RmConverge,
        device_table: *const c_void,
        table_rows: u32,
        device_camera_rows: *const c_void,
        device_light_offsets: *const c_void,
        n_lights: u32,
        device_shape_offsets: *const c_void,
        n_shapes: u32,
        fresh: bool,
        buffers: RmConvergeFrame,
        hip_stream: *mut c_void,
    ) {
        let p = Gpu::params(fov, height, width, frame_width, frame_height);
        let lens = RmLens { aperture: aperture, focus: focus, n_samples: n_samples, _pad: 0 };
        check(
            unsafe {
                rm_accumulate_converging_camera_device(self.ctx, &p, &lens, &converge, device_table, table_rows, device_camera_rows, device_light_offsets, n_lights, device_shape_offsets, n_shapes, if fresh { 1 } else { 0 }, &buffers, hip_stream)
            },
            self.ctx,
        );
    }

    /// `accumulate_camera` with a shape table through the swept hierarchy `swept` (a handle of `swept`, whose extents hold every row
    /// of the shape table; the boxes are in world space, so no camera row matters): the same bytes, with the scene's hierarchies
    /// walked.  A null `device_shape_offsets` is refused: nothing moves then, and `accumulate_camera` keeps the hierarchy.
    pub fn accumulate_camera_swept(
        &mut self,
        fov: f64,
        height: f64,
        width: f64,
        frame_width: usize,
        frame_height: usize,
        aperture: f64,
        focus: f64,
        n_samples: u32,
        device_table: *const c_void,
        device_camera_rows: *const c_void,
        device_light_offsets: *const c_void,
        n_lights: u32,
        device_shape_offsets: *const c_void,
        n_shapes: u32,
        swept: *const RmSwept,
        n_before: u32,
        device_sum: *mut c_void,
        device_mean: *mut c_void,
        device_rgb8: *mut c_void,
        hip_stream: *mut c_void,
    ) {
        let p = Gpu::params(fov, height, width, frame_width, frame_height);
        let lens = RmLens { aperture: aperture, focus: focus, n_samples: n_samples, _pad: 0 };
        check(
            unsafe {
                rm_accumulate_camera_swept_device(self.ctx, &p, &lens, device_table, device_camera_rows, device_light_offsets, n_lights, device_shape_offsets, n_shapes, swept, n_before, device_sum, device_mean, device_rgb8, hip_stream)
            },
            self.ctx,
        );
    }

    /// `accumulate_converging_camera` with a shape table through the swept hierarchy `swept`.
    pub fn accumulate_converging_camera_swept(
        &mut self,
        fov: f64,
        height: f64,
        width: f64,
        frame_width: usize,
        frame_height: usize,
        aperture: f64,
        focus: f64,
        n_samples: u32,
        converge: RmConverge,
        device_table: *const c_void,
        table_rows: u32,
        device_camera_rows: *const c_void,
        device_light_offsets: *const c_void,
        n_lights: u32,
        device_shape_offsets: *const c_void,
        n_shapes: u32,
        swept: *const RmSwept,
        fresh: bool,
        buffers: RmConvergeFrame,
        hip_stream: *mut c_void,
    ) {
        let p = Gpu::params(fov, height, width, frame_width, frame_height);
        let lens = RmLens { aperture: aperture, focus: focus, n_samples: n_samples, _pad: 0 };
        check(
            unsafe {
                rm_accumulate_converging_camera_swept_device(self.ctx, &p, &lens, &converge, device_table, table_rows, device_camera_rows, device_light_offsets, n_lights, device_shape_offsets, n_shapes, swept, if fresh { 1 } else { 0 }, &buffers, hip_stream)
            },
            self.ctx,
        );
    }

    /// What the ticks that move a shape did: whether the last sampled-frame tick's launch walked a swept hierarchy, and how many
    /// hierarchies the ticks have built over the context's life.  Host state only.
    pub fn swept_tick_info(&mut self) -> RmSweptTickReport {
        let mut out = RmSweptTickReport::default();
        check(unsafe { rm_swept_tick_info(self.ctx, &mut out) }, self.ctx);
        out
    }

    /// Bytes of device memory the workspace of `denoise_device` needs for a frame of that size.
    pub fn denoise_workspace(fov: f64, height: f64, width: f64, frame_width: usize, frame_height: usize) -> usize {
        let p = Gpu::params(fov, height, width, frame_width, frame_height);
        let mut bytes: usize = 0;
        check(unsafe { rm_denoise_workspace(&p, &mut bytes) }, ptr::null());
        bytes
    }

    /// The variance-guided filter for a host that keeps its own device buffers: an edge-avoiding a-trous filter over a
    /// converging frame's `device_sum`, `device_stats` and `device_count` -- and, where `device_hits` is not null, the hits of
    /// `rm_primary_hits_device` as the guide -- into `device_out` and, where not null, `device_variance` and `device_rgb8`.
    /// `device_workspace` holds `denoise_workspace` bytes.  Asynchronous on `hip_stream`.
    pub fn denoise_device(
        &mut self,
        fov: f64,
        height: f64,
        width: f64,
        frame_width: usize,
        frame_height: usize,
        denoise: RmDenoise,
        device_sum: *const c_void,
        device_stats: *const c_void,
        device_count: *const c_void,
        device_hits: *const c_void,
        device_workspace: *mut c_void,
        device_out: *mut c_void,
        device_variance: *mut c_void,
        device_rgb8: *mut c_void,
        hip_stream: *mut c_void,
    ) {
        let p = Gpu::params(fov, height, width, frame_width, frame_height);
        check(
            unsafe {
                rm_denoise_device(self.ctx, &p, &denoise, device_sum, device_stats, device_count, device_hits, device_workspace, device_out, device_variance, device_rgb8, hip_stream)
            },
            self.ctx,
        );
    }

    /// The converging frame the last `render_converging*` call built, filtered into `frame`; the converging frame itself is left
    /// alone and its next tick continues it.  `guides`: steer the filter by the hits under the pixels as well -- the pinhole
    /// view: off under a wide aperture, a moving camera or strongly moving shapes.  `RmDenoise::default()` holds starting
    /// values, not tuned ones.
    pub fn render_denoised(
        &mut self,
        fov: f64,
        height: f64,
        width: f64,
        frame: &mut FrameBuffer,
        scene: &::scene::Scene,
        denoise: RmDenoise,
        guides: bool,
        display: Option<&mut Vec<u8>>,
    ) -> String {
        let now = ::std::time::Instant::now();
        self.upload(scene);
        let p = Gpu::params(fov, height, width, frame.width, frame.height);
        let rows = frame.height - frame.height % 32;
        let mut flat = vec![0f64; rows * frame.width * 3 + 1]; // (+ 1: never a dangling frame pointer)
        let bytes: *mut u8 = match display {
            Some(d) => {
                d.resize(frame.width * frame.height * 3, 0);
                d.as_mut_ptr()
            }
            None => ptr::null_mut(),
        };
        let mut timing = RmTiming::default();
        check(unsafe { rm_render_denoised(self.ctx, &p, &denoise, if guides { 1 } else { 0 }, flat.as_mut_ptr(), bytes, &mut timing) }, self.ctx);
        for y in 0..rows {
            assert!(frame.buffer[y].len() == frame.width, "FrameBuffer: row {} holds {} pixels for a width of {}", y, frame.buffer[y].len(), frame.width);
            for x in 0..frame.width {
                let c = &flat[(y * frame.width + x) * 3..(y * frame.width + x) * 3 + 3];
                frame.buffer[y][x] = Vec3f { x: c[0], y: c[1], z: c[2] };
            }
        }
        Gpu::status(now, frame.width, frame.height)
    }

    /// Temporal reprojection for a host that keeps its own device buffers: carries the converging frame `prev_sum`, `prev_stats`,
    /// `prev_count`, sampled from `previous_view` whose hits are `prev_hits`, to the view `cur_hits` was made for, into `out_sum`,
    /// `out_stats` and `out_count`; `out_carried` (a byte a pixel) and `out_carried_total` (one u32 on the device) may be null.
    /// Asynchronous on `hip_stream`.
    pub fn reproject_device(
        &mut self,
        fov: f64,
        height: f64,
        width: f64,
        frame_width: usize,
        frame_height: usize,
        reproject: RmReproject,
        previous_view: RmView,
        prev_sum: *const c_void,
        prev_stats: *const c_void,
        prev_count: *const c_void,
        prev_hits: *const c_void,
        cur_hits: *const c_void,
        out_sum: *mut c_void,
        out_stats: *mut c_void,
        out_count: *mut c_void,
        out_carried: *mut c_void,
        out_carried_total: *mut c_void,
        hip_stream: *mut c_void,
    ) {
        let p = Gpu::params(fov, height, width, frame_width, frame_height);
        check(
            unsafe {
                rm_reproject_device(self.ctx, &p, &reproject, &previous_view, prev_sum, prev_stats, prev_count, prev_hits, cur_hits, out_sum, out_stats, out_count, out_carried, out_carried_total, hip_stream)
            },
            self.ctx,
        );
    }

    /// History for `render_converging`: with `Some(settings)` a camera move no longer begins the frame again but carries it to
    /// the new view; `None` turns that off.  `RmReproject::default()` holds starting values, not tuned ones; `max_history`
    /// bounds how long view-dependent light is carried as if it stuck to the surface.
    pub fn converge_history(&mut self, reproject: Option<RmReproject>) {
        let r = match reproject.as_ref() {
            Some(r) => r as *const RmReproject,
            None => ptr::null(),
        };
        check(unsafe { rm_converge_history(self.ctx, r) }, self.ctx);
    }

    /// What the ticks did with their history: tells a reprojected tick from one that began again.
    pub fn history_info(&mut self) -> RmHistoryReport {
        let mut out = RmHistoryReport::default();
        check(unsafe { rm_converge_history_info(self.ctx, &mut out) }, self.ctx);
        out
    }

    /// Bytes of device memory the list of `accumulate_converging` needs for a frame of that size.
    pub fn converge_workspace(fov: f64, height: f64, width: f64, frame_width: usize, frame_height: usize) -> usize {
        let p = Gpu::params(fov, height, width, frame_width, frame_height);
        let mut bytes: usize = 0;
        check(unsafe { rm_converge_workspace(&p, &mut bytes) }, ptr::null());
        bytes
    }

    /// `render` with a device-resident FrameBuffer: the f64 frame stays on the GPU and only
    /// `fb.to_vec()` comes back -- what update_raytrace_image hands to the pixbuf
    /// (main.rs:337-346).  `display` is resized to width * height * 3; bytes of rows below the
    /// last whole patch row keep their contents.  `fetch` brings the f64 rows over when
    /// save_to_file wants them (main.rs:353-357).
    pub fn render_display(
        &mut self,
        fov: f64,
        height: f64,
        width: f64,
        frame_width: usize,
        frame_height: usize,
        scene: &::scene::Scene,
        display: &mut Vec<u8>,
    ) -> String {
        let now = ::std::time::Instant::now();
        self.upload(scene);
        let p = Gpu::params(fov, height, width, frame_width, frame_height);
        display.resize(frame_width * frame_height * 3, 0);
        let mut timing = RmTiming::default();
        check(unsafe { rm_render_display(self.ctx, &p, display.as_mut_ptr(), &mut timing) }, self.ctx);
        Gpu::status(now, frame_width, frame_height)
    }

    /// What `render` shows at pixel (x = column, y = row) of a `frame_width` x `frame_height` frame: the closest hit
    /// of the ray renderer.rs:80 casts there -- the same direction as the frame's, bit for bit -- or None where that ray
    /// leaves the scene.  `hit.shape` indexes `scene.shapes` (click-to-pick).
    pub fn pick(
        &mut self,
        fov: f64,
        height: f64,
        width: f64,
        frame_width: usize,
        frame_height: usize,
        scene: &::scene::Scene,
        x: u32,
        y: u32,
    ) -> Option<RmHit> {
        self.upload(scene);
        let mut p: RmParams = unsafe { ::std::mem::zeroed() };
        unsafe { rm_create_renderer(fov, height, width, &mut p) };
        p.frame_width = frame_width as u32;
        p.frame_height = frame_height as u32;
        let mut hit: RmHit = unsafe { ::std::mem::zeroed() };
        check(unsafe { rm_pick(self.ctx, &p, x, y, &mut hit) }, self.ctx);
        if hit.hit != 0 {
            Some(hit)
        } else {
            None
        }
    }

    /// Can `a` see `b` in `scene`?  Nothing may lie on the segment between `skin` and its length less `skin` -- the guard
    /// against the surfaces the two points lie on (the render's own is 1e-3).
    pub fn visible(&mut self, scene: &::scene::Scene, a: Vec3f, b: Vec3f, skin: f64) -> bool {
        self.upload(scene);
        let (from, to): (RmVec3, RmVec3) = (a.into(), b.into());
        let mut seen: u8 = 0;
        check(unsafe { rm_visible_segments(self.ctx, &from, &to, 1, skin, &mut seen) }, self.ctx);
        seen != 0
    }

    /// Which of `scene.lights` reach the surface point `point` with normal `normal` (a `pick`'s, say): one bool per
    /// light.  `clipped` false: the decision direct_lighting takes (renderer.rs:166-174), where a shape behind the light
    /// shadows; true: the shadow ray ends at the light.
    pub fn lit_by(&mut self, scene: &::scene::Scene, point: Vec3f, normal: Vec3f, clipped: bool) -> Vec<bool> {
        self.upload(scene);
        let (p, n): (RmVec3, RmVec3) = (point.into(), normal.into());
        let mut lit = vec![0u8; scene.lights.len()];
        let mode = if clipped { RM_LIGHTS_CLIPPED } else { RM_LIGHTS_AS_RENDERED };
        check(unsafe { rm_lights_visible(self.ctx, &p, &n, 1, lit.len() as u32, mode, lit.as_mut_ptr()) }, self.ctx);
        lit.iter().map(|&b| b != 0).collect()
    }

    /// What comes back along rays of the caller's own in `scene`: cast_ray (renderer.rs:254-309) with the depth cap
    /// `max_depth` and the render's background, one colour per ray.  `rays`: (origin, unit direction) pairs.  A ray that
    /// leaves the scene returns zero, as a primary ray of the render does.
    pub fn radiance(&mut self, scene: &::scene::Scene, rays: &[(Vec3f, Vec3f)], max_depth: u32) -> Vec<Vec3f> {
        self.upload(scene);
        let origins: Vec<RmVec3> = rays.iter().map(|r| r.0.into()).collect();
        let directions: Vec<RmVec3> = rays.iter().map(|r| r.1.into()).collect();
        let shading = RmShading { background: RmVec3 { x: 0.1, y: 0.1, z: 0.1 }, max_depth: max_depth, _pad: 0 }; // renderer.rs:40-44
        let mut rgb = vec![RmVec3 { x: 0., y: 0., z: 0. }; rays.len()];
        check(
            unsafe { rm_radiance_rays(self.ctx, origins.as_ptr(), directions.as_ptr(), rays.len() as u32, &shading, rgb.as_mut_ptr()) },
            self.ctx,
        );
        rgb.iter().map(|c| Vec3f { x: c.x, y: c.y, z: c.z }).collect()
    }

    /// The radiance at real-valued positions (sx = column, sy = row) of the frame `render` would draw: sub-pixel samples
    /// for anti-aliasing, a sparse view.  `xy` holds the pairs back to back; integer positions are the render's own pixels.
    pub fn radiance_samples(
        &mut self,
        fov: f64,
        height: f64,
        width: f64,
        frame_width: usize,
        frame_height: usize,
        scene: &::scene::Scene,
        xy: &[f64],
    ) -> Vec<Vec3f> {
        self.upload(scene);
        let mut p: RmParams = unsafe { ::std::mem::zeroed() };
        unsafe { rm_create_renderer(fov, height, width, &mut p) };
        p.frame_width = frame_width as u32;
        p.frame_height = frame_height as u32;
        p.max_depth = 3; // renderer.rs:262
        let n = xy.len() / 2;
        let mut rgb = vec![RmVec3 { x: 0., y: 0., z: 0. }; n];
        check(unsafe { rm_radiance_samples(self.ctx, &p, xy.as_ptr(), n as u32, rgb.as_mut_ptr()) }, self.ctx);
        rgb.iter().map(|c| Vec3f { x: c.x, y: c.y, z: c.z }).collect()
    }

    /// The view direction of every later `render`, `render_display` and `pick`; None: the reference's fixed view
    /// (down -z, +y up).  It stays with the context: uploads -- every render makes one -- leave it alone.
    pub fn orient(&mut self, basis: Option<&RmCameraBasis>) {
        let p = match basis {
            Some(b) => b as *const RmCameraBasis,
            None => ::std::ptr::null(),
        };
        check(unsafe { rm_camera_orient(self.ctx, p) }, self.ctx);
    }

    /// Turns the camera that stands at `eye` (the caller's `scene.camera`: the position travels with the scene)
    /// towards `target`; returns the basis, for `turn` to go on from.
    pub fn look_at(&mut self, eye: Vec3f, target: Vec3f, up: Vec3f) -> RmCameraBasis {
        let mut b: RmCameraBasis = unsafe { ::std::mem::zeroed() };
        check(unsafe { rm_camera_basis_look_at(eye.into(), target.into(), up.into(), &mut b) }, ::std::ptr::null());
        self.orient(Some(&b));
        b
    }

    /// Turns the view by yaw / pitch / roll (radians; positive yaw turns left, positive pitch looks up) from what the
    /// context holds: the two turn buttons of INTEGRATION.md.
    pub fn turn(&mut self, yaw: f64, pitch: f64, roll: f64) -> RmCameraBasis {
        let mut b: RmCameraBasis = unsafe { ::std::mem::zeroed() };
        check(unsafe { rm_camera_get(self.ctx, ::std::ptr::null_mut(), &mut b, ::std::ptr::null_mut()) }, self.ctx);
        let mut out = b;
        check(unsafe { rm_camera_basis_turn(&b, yaw, pitch, roll, &mut out) }, ::std::ptr::null());
        self.orient(Some(&out));
        out
    }

    /// The f64 rows of the frame the last render left on the device, into `frame.buffer`.
    pub fn fetch(&mut self, frame: &mut FrameBuffer) {
        let rows = row_pointers(frame);
        // (the library refuses a FrameBuffer of another size than the frame it holds: a window resized since the render)
        check(unsafe { rm_fetch_rows(self.ctx, rows.as_ptr(), frame.width as u32, frame.height as u32, 0, 0) }, self.ctx);
    }
}

impl Drop for Gpu {
    fn drop(&mut self) {
        unsafe { rm_destroy(self.ctx) }
    }
}
