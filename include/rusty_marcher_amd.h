/*
 * rusty_marcher_amd.h -- C ABI of the MI355X render backend.
 *
 * Drop-in boundary for ONE hot path of blefaudeux/rusty-marcher: the call
 *     raymarcher.render(&mut self.fb, &self.scene)      (engine/src/main.rs:331-333)
 * i.e. Renderer::render (renderer.rs:36-126) and everything below it
 * (cast_ray, the Shape::intersect implementations, optics, lighting).
 * The reference has no FFI of its own; these are the entry points a Rust
 * `extern "C"` block for that path binds (see INTEGRATION.md for the shim).
 *
 * Conventions
 *   - plain C, plain pointers and sizes; every struct below is `#[repr(C)]`-able.
 *   - all arithmetic types are IEEE-754 binary64 (geometry.rs:4-8).
 *   - every call returns rm_status; nothing unwinds across the boundary.  The
 *     reference's failure mode is a panic, so the Rust shim turns a non-zero
 *     status into `panic!("{}", rm_last_error(..))`.
 *   - one caller at a time per rm_ctx / rm_scene (the reference calls render on
 *     the GTK main thread and blocks until the frame is complete).
 *   - the render entry points FAIL (RM_ERR_NO_DEVICE / RM_ERR_HIP) when no
 *     gfx950 device or kernel image is available; there is no CPU fallback.
 */
#ifndef RUSTY_MARCHER_AMD_H
#define RUSTY_MARCHER_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RM_ABI_VERSION 5u

typedef enum rm_status {
    RM_OK = 0,
    RM_ERR_INVALID_ARG = 1,
    RM_ERR_DIMENSIONS = 2,   /* width % 32 != 0: the reference's scatter indexes out of
                                bounds and panics (renderer.rs:92-108) */
    RM_ERR_NO_DEVICE = 3,
    RM_ERR_HIP = 4,
    RM_ERR_NO_SCENE = 5,     /* rm_render before rm_scene_upload */
    RM_ERR_SCENE_LIMIT = 6,  /* scene exceeds a documented device limit */
    RM_ERR_IO = 7,           /* file missing (obj.rs:53-56 returns None; a missing mtllib
                                panics "WOOPS", obj.rs:64) */
    RM_ERR_PARSE = 8,
    RM_ERR_DEPTH = 9,        /* max_depth outside [0, RM_MAX_DEPTH] */
    RM_ERR_COMM = 10,        /* RCCL unavailable or a collective failed (rm_comm_*, rm_frame_*) */
    RM_ERR_TIMEOUT = 11      /* rm_frame_wait*: the slot's frame did not complete in time (a peer is
                                missing or stuck in the collective); the context is not usable for
                                further frames -- report and exit (rm_destroy then releases what it
                                can without waiting for the device) */
} rm_status;

/* Recursion cap accepted by rm_render.  The reference hard-codes 3
 * (renderer.rs:262) and counts in a u8. */
#define RM_MAX_DEPTH 32u
/* The reference's patch edge (renderer.rs:47); the only value accepted. */
#define RM_PATCH_SIZE 32u

/* geometry.rs:4-8 `Vec3f` */
typedef struct rm_vec3 { double x, y, z; } rm_vec3;

/* shapes.rs:20-32 `Reflectance` (bool widened to a 32-bit int + padding) */
typedef struct rm_reflectance {
    double  diffusion;
    rm_vec3 diffuse_color;
    double  specular;
    double  specular_exponent;
    int32_t is_glass_like;
    int32_t _pad;
    double  reflection;
    double  refractive_index;
} rm_reflectance;

/* lights.rs:4-8 `Light`; colour already L-inf normalised (lights.rs:10-16) */
typedef struct rm_light { rm_vec3 position, color; double intensity; } rm_light;

/* sphere.rs:6-11 `Sphere` (bounding box dropped: never consulted, shapes.rs:34-86) */
typedef struct rm_sphere { rm_vec3 center; double radius_square; rm_reflectance reflectance; } rm_sphere;

/* polygon.rs:6-12 `ConvexPolygon`; vertices live in rm_scene_desc.polygon_vertices */
typedef struct rm_polygon {
    uint32_t first_vertex, n_vertices;
    rm_vec3  plane_normal, plane_point;
    rm_reflectance reflectance;
} rm_polygon;

/* triangle.rs:6-10 `Triangle` + its entry of Obj.reflectances (obj.rs:16) */
typedef struct rm_triangle {
    rm_vec3 vertices[3];
    rm_vec3 normal, center;
    rm_reflectance reflectance;
} rm_triangle;

typedef enum rm_shape_kind { RM_SHAPE_SPHERE = 0, RM_SHAPE_POLYGON = 1, RM_SHAPE_MESH = 2 } rm_shape_kind;

/* One element of Scene.shapes: Vec<Box<dyn Shape + Sync>> (scene.rs:11), in list
 * order (the order decides ties, shapes.rs:130 and obj.rs:198).
 * SPHERE/POLYGON: `first` indexes spheres[]/polygons[], count == 1.
 * MESH (an obj.rs `Obj`): triangles[first .. first+count). */
typedef struct rm_shape_ref { uint32_t kind, first, count, _pad; } rm_shape_ref;

/* Flat, pointer-and-size view of scene.rs:9-13 `Scene`. */
typedef struct rm_scene_desc {
    const rm_shape_ref *shapes;            uint32_t n_shapes;
    const rm_sphere    *spheres;           uint32_t n_spheres;
    const rm_polygon   *polygons;          uint32_t n_polygons;
    const rm_vec3      *polygon_vertices;  uint32_t n_polygon_vertices;
    const rm_triangle  *triangles;         uint32_t n_triangles;
    const rm_light     *lights;            uint32_t n_lights;
    rm_vec3 camera;
} rm_scene_desc;

/* renderer.rs:17-23 `Renderer` + the frame geometry render() reads from the
 * FrameBuffer (renderer.rs:49-55) + the constants it hard-codes. */
typedef struct rm_params {
    /* Renderer, as create_renderer(fov, height, width) fills it (renderer.rs:25-33) */
    double fov, half_fov, height, width, ratio;
    /* FrameBuffer.width / .height (framebuffer.rs:6-10) */
    uint32_t frame_width, frame_height;
    /* renderer.rs:262 (reference: 3) */
    uint32_t max_depth;
    /* renderer.rs:47 (must be RM_PATCH_SIZE) */
    uint32_t patch_size;
    /* renderer.rs:40-44 (reference: 0.1, 0.1, 0.1) */
    rm_vec3 background;
    /* Patch rows owned by this caller: begin, begin + stride, begin + 2 stride, ... < end.
     * end == 0 means "frame_height/32"; stride 0 or 1 means every row of [begin, end).
     * A stride of N with begin = rank deals the rows out cyclically to N GPUs (sky rows
     * are cheap, ground rows expensive).  Pixels of rows not owned are untouched. */
    uint32_t patch_row_begin, patch_row_end;
    uint32_t flags;        /* RM_FLAG_* */
    uint32_t patch_row_stride;
} rm_params;

#define RM_FLAG_NONE 0u
/* Numeric flavour of the kernel.
 * Default (flag clear): every binary64 operation separately rounded, in the reference's
 * order (sqrt then divide, hits ordered by the squared distance of shapes.rs:128): the
 * hit / miss / shadow decisions are the reference's bit for bit, including where a ray
 * lies exactly on a polygon edge and the decision is the reference's rounding noise.
 * RM_FLAG_FAST_FP (opt-in, ~20 % faster): fused multiply-add, 1/sqrt by Newton iteration,
 * hits ordered by ray parameter.  Values move by ~1e-12; decisions can differ from the
 * reference ONLY at such exact-incidence pixels (the demo scene has a handful per frame
 * for some camera positions: its triangle has small-integer coordinates).
 * The contract, as the tests hold it: a fast frame differs from the reference (by 1e-9 or
 * more on a channel) only at pixels whose reference colour itself changes under a
 * perturbation of at most 16 ulps of the primary ray's unit direction (exact zeros kept),
 * and there it shows one of those colours -- never anything else. */
#define RM_FLAG_FAST_FP 2u
/* rm_render_device_u8 only: device_rgb8 holds just the OWNED patch rows, packed -- the
 * k-th owned patch row occupies byte rows [32k, 32k + 32) of a [n_owned*32][frame_width][3]
 * buffer -- so that a rank's display bytes are one contiguous chunk for a gather. */
#define RM_FLAG_U8_COMPACT 4u
/* rm_render_device / rm_render_device_u8: device_rgb holds just the OWNED patch rows, packed
 * the same way ([n_owned*32][frame_width][3] doubles): a rank's f64 rows as one contiguous
 * chunk (what rm_frame_submit_f64 gathers). */
#define RM_FLAG_F64_COMPACT 8u

typedef struct rm_timing {
    double kernel_ms;   /* HIP-event time of the render kernel on its stream */
    double d2h_ms;      /* device -> host copy (0 when host_rgb == NULL) */
    double total_ms;    /* host wall time of the call */
} rm_timing;

typedef struct rm_scene rm_scene;   /* host-side scene builder (opaque) */
typedef struct rm_ctx rm_ctx;       /* one GPU: stream, device scene, framebuffer (opaque) */

/* ---------------------------------------------------------------------- */
/* Host side: scene construction.  Replaces the constructors the reference  */
/* runs before render(): nothing here touches the GPU.                      */
/* ---------------------------------------------------------------------- */

/* shapes.rs:49-61 Reflectance::create_default */
void rm_reflectance_default(rm_reflectance *out);

/* renderer.rs:25-33 create_renderer(fov, height, width) -- note the argument order.
 * Fills fov/half_fov/height/width/ratio, sets frame_* from (width, height) truncated,
 * max_depth = 3, patch_size = 32, background = 0.1, full band, flags = 0. */
void rm_create_renderer(double fov, double height, double width, rm_params *out);

rm_status rm_scene_new(rm_scene **out);                                   /* scene.rs:16-23 */
void      rm_scene_free(rm_scene *scene);
rm_status rm_scene_create_default(rm_scene **out);                        /* scene.rs:28-211 */
/* sphere.rs:13-24 */
rm_status rm_scene_add_sphere(rm_scene *scene, rm_vec3 center, double radius, const rm_reflectance *r);
/* polygon.rs:16-42; n_vertices < 3 -> RM_ERR_INVALID_ARG (reference asserts) */
rm_status rm_scene_add_polygon(rm_scene *scene, const rm_vec3 *vertices, uint32_t n_vertices,
                               const rm_reflectance *r);
/* One obj.rs `Obj`: n triangles as 9 doubles each; per-triangle colour ramp of
 * obj.rs:125-138; then Obj::offset(offset) (obj.rs:24-29, triangle.rs:19-24). */
rm_status rm_scene_add_mesh(rm_scene *scene, const double *tri_xyz, uint32_t n_triangles, rm_vec3 offset);
/* lights.rs:10-16 */
rm_status rm_scene_add_light(rm_scene *scene, rm_vec3 position, rm_vec3 color, double intensity);
/* ConvexPolygon::offset (polygon.rs:44-49) / Obj::offset (obj.rs:24-29): moves shape
 * `shape_index` of the list (plane point or triangle centres, and vertices; normals
 * are kept).  Spheres have no offset method in the reference -> RM_ERR_INVALID_ARG. */
rm_status rm_scene_offset_shape(rm_scene *scene, uint32_t shape_index, rm_vec3 offset);
rm_status rm_scene_set_camera(rm_scene *scene, rm_vec3 camera);
rm_status rm_scene_offset_camera(rm_scene *scene, rm_vec3 offset);       /* scene.rs:25-27 */
/* obj.rs:44-151 obj::load: appends one MESH shape per model of the file, each
 * moved by `offset`; *n_models_out (optional) receives the model count. */
rm_status rm_scene_load_obj(rm_scene *scene, const char *path, rm_vec3 offset, uint32_t *n_models_out);
/* main.rs:261-327 Win::open_obj: new scene = load(path) offset by (0,0,-500) + the
 * two hard-coded lights. */
rm_status rm_scene_open_obj(const char *path, rm_scene **out);
/* Flat view; pointers stay valid until the scene is next modified or freed. */
rm_status rm_scene_get_desc(const rm_scene *scene, rm_scene_desc *out);

/* renderer.rs:111-121: "Scene rendered in {} ms ({} fps, {:.2} MP/s)".
 * Returns the length written (snprintf semantics). */
int rm_format_status(char *buf, size_t buflen, uint64_t ms, uint32_t frame_width, uint32_t frame_height);

/* ---------------------------------------------------------------------- */
/* Device side: the render path.                                            */
/* ---------------------------------------------------------------------- */

/* Binds HIP device `device_ordinal` (one process per GPU), creates its stream. */
rm_status rm_init(int device_ordinal, rm_ctx **out);
void      rm_destroy(rm_ctx *ctx);
/* Last error text of `ctx`; ctx == NULL -> last error of a host-side call or of a
 * failed rm_init on this thread.  Never NULL. */
const char *rm_last_error(const rm_ctx *ctx);

/* Copies the scene into device memory (arrays are copied; caller keeps ownership).  The
 * reference hands its whole Scene to every render() call (main.rs:331-333); a scene whose
 * device image equals the resident one is recognised and not copied again (cameras apart:
 * the camera is not part of the image), so a host may simply upload before every frame. */
rm_status rm_scene_upload(rm_ctx *ctx, const rm_scene_desc *desc);
/* How often rm_scene_upload was called on this context, and how often it had to copy. */
rm_status rm_scene_uploads(rm_ctx *ctx, uint64_t *calls, uint64_t *copies);
/* scene.rs:25-27 without re-upload: replaces the camera of the uploaded scene. */
rm_status rm_camera_update(rm_ctx *ctx, rm_vec3 camera);

/*
 * Renderer::render (renderer.rs:36-126) for the patch rows of params' band.
 * host_rgb: [frame_height][frame_width][3] doubles row-major (framebuffer.rs:12-22
 * flattened), caller-allocated; only the band's rows are written, so rows
 * >= frame_height - frame_height%32 keep their previous contents exactly as in the
 * reference.  NULL leaves the result in the context's device framebuffer.
 * Blocks until host_rgb is filled (or, for NULL, until the kernel has finished).
 * The device -> host copy dominates the call (48.7 MB at 1080p: ~0.9 ms over PCIe against
 * 0.08 ms of kernel; black patches are not sent, see rm_render_rows); a window wants
 * rm_render_display (3 B/pixel), a render loop rm_frame_submit_to_host.
 */
rm_status rm_render(rm_ctx *ctx, const rm_params *params, double *host_rgb, rm_timing *timing);

/*
 * Renderer::render into the reference's ACTUAL render target: framebuffer.rs:6-22 is
 * `buffer: Vec<Vec<Vec3f>>`, one heap allocation per scan line, filled by the serial scatter of
 * renderer.rs:92-108.  rows[y] points at row y: frame_width * 3 doubles (x, y, z of each Vec3f --
 * `#[repr(C)]` on geometry.rs:4-8); frame_height pointers, of which only
 * those of the band's rows are read (the others may be NULL: rows >= frame_height -
 * frame_height % 32 keep their contents, renderer.rs:53).  Blocks until the rows are filled, bit
 * for bit what rm_render writes into a flat array.
 * Inside: one launch, then the frame crosses the PCIe link into a page-locked staging buffer of
 * the context in chunks while a few host threads (RM_HOST_THREADS, default min(8, cores))
 * scatter the chunks that have arrived into the rows.  Patches that are black -- +0.0 in every
 * channel of all 1,024 pixels: what primary rays that leave the scene produce, renderer.rs:305 --
 * are not sent: a kernel packs the others, the host writes the zeros itself (frames of 2 MB and
 * more; RM_HOST_PACK=0|1 forces).  rm_render takes the same path into its flat array.
 */
rm_status rm_render_rows(rm_ctx *ctx, const rm_params *params, double *const *rows, rm_timing *timing);

/*
 * Renderer::render with a DEVICE-RESIDENT FrameBuffer: the f64 frame stays in the context's
 * device framebuffer (rm_device_framebuffer, rm_fetch_rows, rm_postprocess(ctx, NULL, ..)) and
 * only `fb.to_vec()` of the band -- the bytes update_raytrace_image hands to the pixbuf,
 * main.rs:337-346; (255 * clamp(f, 0, 1)) as u8, framebuffer.rs:40-55,80-82 -- comes back:
 * host_rgb8 is [frame_height][frame_width][3] bytes, only the band's rows are written.  3 B/pixel
 * instead of 24: one launch, then one copy-engine transfer (RM_DISPLAY_SUBBANDS=n renders n sub-bands, the bytes
 * of one crossing the link while the next renders: measured and slower, default 1).  Blocks until host_rgb8 is filled.
 * host_rgb8 from rm_host_alloc is written by the copy engine directly; any other memory is
 * reached through the context's staging buffer.
 */
rm_status rm_render_display(rm_ctx *ctx, const rm_params *params, uint8_t *host_rgb8, rm_timing *timing);

/*
 * f64 rows of the device-resident frame on demand (save_to_file, main.rs:353-357: normalize +
 * write_ppm read the f64 values): patch rows [patch_row_begin, patch_row_end) -- end 0 = all
 * whole patch rows -- of the frame the last rm_render / rm_render_rows / rm_render_display left
 * on the device, into rows[y] (as rm_render_rows).  frame_width x frame_height is the size of the
 * FrameBuffer `rows` belongs to -- frame_height pointers to frame_width * 3 doubles each: it must be
 * the size of the resident frame (a window that has been resized since holds another), else
 * RM_ERR_INVALID_ARG and nothing is read or written (ABI 5; ABI 4 took no size and trusted the caller).
 */
rm_status rm_fetch_rows(rm_ctx *ctx, double *const *rows, uint32_t frame_width, uint32_t frame_height,
                        uint32_t patch_row_begin, uint32_t patch_row_end);

/* What the last rm_render / rm_render_rows / rm_fetch_rows / rm_render_display of this context
 * moved: bytes that crossed the link, 32x32 patches of the band, patches among them that were
 * sent (the others were black and written by the host), and the host threads that scatter. */
rm_status rm_hostio_stats(rm_ctx *ctx, uint64_t *bytes_copied, uint64_t *patches, uint64_t *patches_sent, int *threads);

/*
 * Same kernel, asynchronous, into a caller-owned DEVICE buffer with the same
 * [frame_height][frame_width][3] layout, enqueued on `hip_stream` (a hipStream_t;
 * NULL = HIP's default stream).  Returns once enqueued; ordering with the caller's
 * other work is that stream's.
 */
rm_status rm_render_device(rm_ctx *ctx, const rm_params *params, void *device_rgb, void *hip_stream);

/*
 * rm_render_device that ALSO writes the band's display bytes: device_rgb8 is a
 * [frame_height][frame_width][3] byte buffer receiving `fb.to_vec()` of the rendered
 * pixels (framebuffer.rs:40-55: (255 * clamp(f, 0, 1)) as u8, no normalisation -- what
 * update_raytrace_image hands to the pixbuf, main.rs:337-346), fused into the kernel's
 * epilogue.  3 B/pixel instead of 24: the payload a multi-GPU gather or a D2H copy for
 * display needs.  max_depth must be >= 1.
 */
rm_status rm_render_device_u8(rm_ctx *ctx, const rm_params *params, void *device_rgb, void *device_rgb8,
                              void *hip_stream);

/* Tile classification (the launch in front of the render launch: one lane per 16x4 tile tests the cone of
 * the tile's primary rays against every primitive's bounds -- the BoundingBox the reference computes and never
 * consults, shapes.rs:34-86; tiles nothing can be hit in are filled with the primary-miss value there,
 * renderer.rs:305, and never get a wave): the tiles of the last render launch of this context and how
 * many of them the classification listed for rendering (all of them when it was off: RM_TILE_CLASSIFY=0,
 * small frames, scenes of many primitives).  hip_stream: the stream that launch was enqueued on (NULL: whichever
 * the context's last render launch went to).  Waits for the device. */
rm_status rm_tile_stats(rm_ctx *ctx, void *hip_stream, uint32_t *tiles, uint32_t *tiles_listed);

/* The geometry of the context's last render launch: its workgroups (one wave each), and how many 32x32 patches of
 * it were handed to its sky tail -- patches that the previous frames of the same view on the stream found nothing to
 * hit in get ONE wave instead of sixteen (it looks at this launch's own classification of the patch, stores the
 * primary-miss value of renderer.rs:305 over the patch when that still says sky, and renders the patch itself when
 * it does not).  Only the launch's geometry is carried from frame to frame; RM_SKY_TAIL=0 switches it off.
 * Does not wait for the device. */
rm_status rm_launch_stats(rm_ctx *ctx, uint32_t *workgroups, uint32_t *tail_patches);

/* Device framebuffer of the last rm_render(.., NULL, ..) and its size in bytes. */
rm_status rm_device_framebuffer(rm_ctx *ctx, void **device_rgb, size_t *bytes);

/*
 * framebuffer.rs:58-77 normalize + :40-55 to_vec/:80-82 quantize, on the device.
 * device_rgb: [h][w][3] doubles (NULL = the context's framebuffer).  The global max
 * is taken over ALL h*w pixels (unrendered rows included, as the reference does).
 *   normalize != 0 : scales device_rgb in place by 1/max (if max > 0), as
 *                    FrameBuffer::normalize does before write_ppm (main.rs:355-356)
 *   host_rgb8      : optional [h][w][3] bytes, receives to_vec() of the result
 *   max_out        : optional, receives the global max found (0 when !normalize)
 */
rm_status rm_postprocess(rm_ctx *ctx, void *device_rgb, uint32_t frame_width, uint32_t frame_height,
                         int normalize, uint8_t *host_rgb8, double *max_out);

/* ---- device buffers for hosts without HIP bindings -------------------------------------
 * The device-pointer entry points (rm_render_device*, rm_frame_submit) take plain
 * hipMalloc'ed pointers; a host that links no HIP runtime of its own (the Rust shim) gets
 * them here.  rm_buffer_alloc zero-fills (create_frame_buffer does, framebuffer.rs:12-22);
 * rm_buffer_read is synchronous and does not order itself after work in flight: call it
 * after rm_frame_wait / on buffers no launch is still writing. */
rm_status rm_buffer_alloc(rm_ctx *ctx, size_t bytes, void **device_ptr);
void rm_buffer_free(rm_ctx *ctx, void *device_ptr);
rm_status rm_buffer_read(rm_ctx *ctx, const void *device_ptr, void *host_dst, size_t bytes);
/* Synchronous host -> device copy (e.g. a FrameBuffer's contents for rm_postprocess). */
rm_status rm_buffer_write(rm_ctx *ctx, void *device_ptr, const void *host_src, size_t bytes);
/* Page-locked host memory: the destination rm_frame_submit can copy a finished display
 * frame into asynchronously (a pageable destination would make the copy synchronous). */
rm_status rm_host_alloc(rm_ctx *ctx, size_t bytes, void **host_ptr);
void rm_host_free(rm_ctx *ctx, void *host_ptr);

/* ---- multi-GPU frames: one process per GPU, RCCL over xGMI ----------------------------
 * Replaces, for N GPUs, what renderer.rs:63-108 does with N Rayon workers: the patch rows
 * of a frame are owned cyclically (rank r renders patch rows r, r+N, r+2N, ... so that
 * every rank gets its share of cheap sky and expensive ground rows), each rank's f64 rows
 * stay in its own `device_rgb` (a distributed FrameBuffer), and ONE RCCL exchange per frame
 * completes the display frame (`to_vec` bytes, framebuffer.rs:40-55) at the consumer, RANK 0
 * (the reference has one window, main.rs:337-346): every peer sends its chunk straight to rank 0
 * over its own xGMI link, all at once (grouped ncclSend / ncclRecv).  rm_comm_exchange(ctx, 1)
 * on every rank selects an in-place ncclAllGather instead (the frame on every rank).  Up to RM_MAX_FRAME_SLOTS frames are in flight; a slot has a stream of its
 * own (render, gather, de-interleave in order on the stream); every rank must submit the
 * same sequence of (frame, slot) pairs.  All slots share ONE communicator unless
 * RM_SLOT_COMMS=1 is exported on EVERY rank (then each slot gets one split off the first;
 * the ranks agree by an all-reduce whether every split succeeded, else all keep the one).
 *
 * Bootstrap: rank 0 calls rm_comm_unique_id and hands the RM_COMM_ID_BYTES to the other
 * ranks by any channel (a file, a socket, torch.distributed's store); every rank then
 * calls rm_comm_init.  id == NULL sets rank/world without a transport: the layout is that
 * of `world` ranks but nothing is exchanged (single-GPU tests of the N-GPU layout).
 */
#define RM_COMM_ID_BYTES 128u
#define RM_MAX_FRAME_SLOTS 4u
rm_status rm_comm_unique_id(void *id_out /* RM_COMM_ID_BYTES */);
rm_status rm_comm_init(rm_ctx *ctx, const void *id, int rank, int world);
void rm_comm_destroy(rm_ctx *ctx);   /* also done by rm_destroy */
/* all_ranks = 0 (default): the chunks are gathered at rank 0; 1: all-gathered, every rank ends
 * up with the whole gather buffer.  The same on every rank, before the first submit. */
rm_status rm_comm_exchange(rm_ctx *ctx, int all_ranks);

/* Layout of the gather buffer for `world` ranks: world chunks of rows_per_rank patch rows
 * (32 * frame_width * 3 bytes each); chunk k holds patch rows k, k+world, ... packed. */
rm_status rm_exchange_layout(const rm_params *params, int world, uint32_t *rows_per_rank, size_t *chunk_bytes);

/*
 * One frame, asynchronously: renders this rank's rows into device_rgb ([H][W][3] f64,
 * only the owned rows are written) and their display bytes into this rank's chunk of
 * device_gather8 (world * chunk_bytes), gathers the chunks there (at rank 0; with
 * rm_comm_exchange(ctx, 1) on every rank), and -- where device_display8 is not NULL (the
 * consumer: rank 0) -- writes the [32*n_patch_rows][W][3] image-order display frame.
 * params->patch_row_* must be zero.
 * All four buffers belong to `slot` until rm_frame_wait(slot) returns or the slot is
 * submitted again (a slot's frames are ordered); two slots must not share a buffer.
 */
rm_status rm_frame_submit(rm_ctx *ctx, const rm_params *params, void *device_rgb, void *device_gather8,
                          void *device_display8, uint32_t slot);
/* The same, and the display frame is then copied into host_display8 (rm_host_alloc'ed,
 * 32 * n_patch_rows * W * 3 bytes) on the slot's stream: after rm_frame_wait(slot) the bytes
 * of fb.to_vec() are in host memory (main.rs:337-346 hands them to the pixbuf). */
rm_status rm_frame_submit_to_host(rm_ctx *ctx, const rm_params *params, void *device_rgb, void *device_gather8,
                                  void *device_display8, void *host_display8, uint32_t slot);
/* Blocks the host until the slot's last frame is complete on this rank.  With a
 * communicator the wait is bounded: RM_ERR_TIMEOUT after RM_FRAME_TIMEOUT_MS (environment,
 * default 60000; 0 = wait for ever) -- a peer that never joins the collective must not hang
 * the host. */
rm_status rm_frame_wait(rm_ctx *ctx, uint32_t slot);
/* The same with an explicit bound in milliseconds (0 = wait for ever). */
rm_status rm_frame_wait_for(rm_ctx *ctx, uint32_t slot, uint32_t timeout_ms);

/*
 * The f64 frame itself (framebuffer.rs:6-22: the reference's render target is f64) to the
 * consumer: this rank's rows are rendered packed (RM_FLAG_F64_COMPACT) straight into its
 * chunk of device_gather64 (world * 8 * chunk_bytes of rm_exchange_layout), ONE exchange
 * completes the buffer at rank 0 (on every rank with rm_comm_exchange(ctx, 1)), and -- where
 * device_frame64 is not NULL --
 * the [32*n_patch_rows][W][3] f64 frame is written in image order, bit-identical to the
 * single-GPU frame.  8x the bytes of the display path: at 1080p ~6 MB per peer per frame.
 * Frames in flight (slots) overlap one frame's gather with the next frame's render.
 */
rm_status rm_frame_submit_f64(rm_ctx *ctx, const rm_params *params, void *device_gather64, void *device_frame64,
                              uint32_t slot);

/* Device times of the slot's last completed frame (call after rm_frame_wait): render kernel,
 * collective, and everything of the frame on its stream.  The stamps are three more events
 * per frame in the slot's stream and are recorded only after rm_frame_timing_enable(ctx, 1)
 * (a diagnostic: they cost a frame in flight ~15 us). */
typedef struct rm_frame_times { double kernel_ms, gather_ms, total_ms; } rm_frame_times;
rm_status rm_frame_timing_enable(rm_ctx *ctx, int on);
rm_status rm_frame_timing(rm_ctx *ctx, uint32_t slot, rm_frame_times *out);

/* What the communicator itself reports (ncclCommUserRank / ncclCommCount) and how many
 * communicators the slots use; world 1 / rank 0 / 0 communicators without one. */
rm_status rm_comm_info(rm_ctx *ctx, int *rank, int *world, int *n_communicators);


/* ---- ray queries: the resident scene asked about rays of the caller's own ----------------
 * The render's intersection engine without the shading: find_closest_intersect
 * (shapes.rs:110-143) and intersect_shape_set (shapes.rs:92-108) for rays the caller names,
 * the ray under a pixel (click-to-pick), and a per-pixel hit buffer of a frame.  Added under
 * ABI version 5 (RM_ABI_VERSION did not move); a host detects them by " queries" in
 * rm_build_info().
 *
 * Semantics common to every query:
 *   - Scene: the one resident from rm_scene_upload (RM_ERR_NO_SCENE without one).  Ray lists
 *     carry their own origins; rm_pick / rm_primary_hits_device cast from the context's
 *     current camera (rm_camera_update) with the params' Renderer and frame geometry.
 *   - Numeric flavour: always the strict default, whatever params->flags says; hit / miss /
 *     shape decisions are the reference's bit for bit.  A render with RM_FLAG_FAST_FP may
 *     therefore disagree with a pick at exact-incidence pixels (a ray on a polygon edge).
 *     params->flags may carry RM_FLAG_FAST_FP (ignored) and nothing else, and the band must
 *     be the default one (patch_row_begin = patch_row_end = 0, stride 0 or 1): anything
 *     else is RM_ERR_INVALID_ARG.
 *   - Directions must be unit length within the reference's own assert,
 *     |(x*x + y*y) + z*z - 1| < 1e-4 (sphere.rs:31, polygon.rs:62, triangle.rs:53).  The host
 *     entry points check it, and that every component of origin and direction is finite:
 *     RM_ERR_INVALID_ARG naming the first bad ray in rm_last_error, nothing computed.  For the
 *     device entry points it is a precondition: a bad ray gets an unspecified answer for
 *     that ray, never a fault.  Every admitted ray gets the reference's answer, but only rays
 *     with |d.d - 1| <= 1e-14 (a direction normalised in doubles) are walked through the
 *     scene's hierarchy: a group of 64 consecutive rays that holds any other one -- unit only
 *     to float precision, say -- tests every primitive for all 64 (the same for the ranged
 *     and the radiance rays below).  Normalise in doubles where speed matters.
 *   - Occlusion is intersect_shape_set exactly: a hit ANYWHERE along the ray, t in
 *     [0, inf) -- the reference has no maximum distance, so a shadow ray aimed at a light
 *     counts as blocked by a shape BEHIND the light.  (The ranged queries below bound the ray:
 *     rm_occluded_rays_ranged, rm_visible_segments, rm_lights_visible with RM_LIGHTS_CLIPPED.)
 *   - n_rays == 0 is RM_OK and does nothing.
 *   - Device variants are asynchronous on hip_stream (a hipStream_t; NULL = HIP's default
 *     stream), as rm_render_device is; host variants and rm_pick block until the answer is
 *     there.
 *   - Queries leave every piece of render state alone (per-stream tags, classification and
 *     order state, feedback sets, the resident frame): a frame rendered after any sequence
 *     of queries is byte-identical to the frame rendered without them.  A pixel query at a
 *     frame geometry other than the last render's rebuilds the backproject tables the two
 *     share: the next render rebuilds them once more, its output does not change.
 */

/* One answer of find_closest_intersect (shapes.rs:110-143) for one ray. */
typedef struct rm_hit {
    double   t;         /* the hit lies at origin + t * direction */
    rm_vec3  point;     /* Intersection.point  (shapes.rs:3-8) */
    rm_vec3  normal;    /* Intersection.normal */
    uint32_t shape;     /* index into Scene.shapes (shapes.rs:140's shape_hit, NOT wrapped to u8) */
    uint32_t element;   /* triangle index inside the Obj for a mesh shape; 0 for sphere / polygon */
    int32_t  hit;       /* 1 hit, 0 miss; every other field is 0 on a miss */
    uint32_t _pad;
} rm_hit;               /* 72 bytes */

/* Closest hit of n_rays rays: origins[i] + t directions[i] (host arrays) into hits[i]. */
rm_status rm_intersect_rays(rm_ctx *ctx, const rm_vec3 *origins, const rm_vec3 *directions,
                            uint32_t n_rays, rm_hit *hits);
/* intersect_shape_set of n_rays rays: occluded[i] = 1 where anything is hit, else 0. */
rm_status rm_occluded_rays(rm_ctx *ctx, const rm_vec3 *origins, const rm_vec3 *directions,
                           uint32_t n_rays, uint8_t *occluded);
/* The same on device buffers (n_rays rm_vec3 each; n_rays rm_hit / bytes out). */
rm_status rm_intersect_rays_device(rm_ctx *ctx, const void *device_origins, const void *device_directions,
                                   uint32_t n_rays, void *device_hits, void *hip_stream);
rm_status rm_occluded_rays_device(rm_ctx *ctx, const void *device_origins, const void *device_directions,
                                  uint32_t n_rays, void *device_occluded, void *hip_stream);
/*
 * What is under pixel (x, y) -- x the column, y the row -- of the frame render() would draw
 * with `params`: the ray renderer.rs:80 casts there, backproject(x, y) (renderer.rs:128-135)
 * from the camera, its direction bit-identical to the strict render kernel's.  Pixels
 * outside frame_width x frame_height are RM_ERR_INVALID_ARG; the frame_height % 32 rows the
 * render leaves untouched are answered all the same.  frame_width need not be a multiple of 32.
 */
rm_status rm_pick(rm_ctx *ctx, const rm_params *params, uint32_t x, uint32_t y, rm_hit *hit);
/*
 * rm_pick for every pixel rm_render_device writes with the same params (the whole patch rows,
 * rows >= frame_height - frame_height % 32 untouched): device_hits is
 * [frame_height][frame_width] rm_hit.  frame_width % 32 != 0 is RM_ERR_DIMENSIONS, as for the
 * render.
 */
rm_status rm_primary_hits_device(rm_ctx *ctx, const rm_params *params, void *device_hits, void *hip_stream);

/* ---- ranged ray queries: segments, point visibility, light visibility ----------------------
 * The ray queries above answer for rays that run to infinity, as the reference's do.  These take a
 * closed range [t_min, t_max] of the ray parameter, 0 <= t_min <= t_max, t_max = +inf allowed.
 * Additive to ABI version 5; a host detects them by " ranges" in rm_build_info().  The numeric
 * flavour is the strict one, and everything "Semantics common to every query" says holds: the
 * resident scene, unit directions, device variants asynchronous on hip_stream, no render state
 * touched (they read the scene image, the pid map and the lights).
 *
 * Each primitive offers the candidates the reference forms, with the reference's arithmetic:
 *   - sphere: the two roots t0 = tca - thc, t1 = tca + thc (sphere.rs:43-45).  The candidate is t0
 *     if it lies in the range, else t1 if it lies in the range, else none.  For [0, +inf] that is
 *     the reference's `if t0 < 0 { t1 }` followed by `if t < 0 { None }`.
 *   - polygon and triangle: the one `dist` of polygon.rs:71-76 / triangle.rs:62-67, accepted when
 *     it lies in the range and passes the unchanged inside test.
 * Closest hit: accepted candidates are ordered as before, by |p - o|^2 with p = o + d t
 * (shapes.rs:128), exact ties to list order; rm_hit.t is the accepted parameter -- a sphere whose
 * near root lies before t_min is hit at its far root -- point and normal those of that point.
 * Occlusion: a ray is occluded when any primitive has an accepted candidate.
 * With {0, +inf} on every ray both give byte for byte what rm_intersect_rays / rm_occluded_rays give.
 *
 * Host variants check, before anything is launched, what the unranged ones check and: no NaN in a
 * range, t_min >= 0, t_max >= t_min; finite segment endpoints, from != to; finite points and
 * normals, a non-zero normal; skin finite and >= 0; mode 0 or 1.  RM_ERR_INVALID_ARG names the
 * first offender in rm_last_error and nothing is computed.  For the device variants the
 * per-element conditions are preconditions: a bad element gets an unspecified answer for that
 * element, never a fault.  n == 0 is RM_OK and does nothing.
 */
typedef struct rm_range { double t_min, t_max; } rm_range;   /* 16 bytes */

/* rm_intersect_rays / rm_occluded_rays with ranges[i] on ray i. */
rm_status rm_intersect_rays_ranged(rm_ctx *ctx, const rm_vec3 *origins, const rm_vec3 *directions,
                                   const rm_range *ranges, uint32_t n_rays, rm_hit *hits);
rm_status rm_occluded_rays_ranged(rm_ctx *ctx, const rm_vec3 *origins, const rm_vec3 *directions,
                                  const rm_range *ranges, uint32_t n_rays, uint8_t *occluded);
rm_status rm_intersect_rays_ranged_device(rm_ctx *ctx, const void *device_origins, const void *device_directions,
                                          const void *device_ranges, uint32_t n_rays, void *device_hits,
                                          void *hip_stream);
rm_status rm_occluded_rays_ranged_device(rm_ctx *ctx, const void *device_origins, const void *device_directions,
                                         const void *device_ranges, uint32_t n_rays, void *device_occluded,
                                         void *hip_stream);
/*
 * Can from[i] see to[i]?  With v = to[i] - from[i] the ray is from[i] along normalized(v), its
 * length L = sqrt(v.v) -- the sqrt and reciprocal the strict normalized() forms -- and the range
 * [skin, L - skin]: visible[i] = 1 when nothing is accepted in it, else 0.  skin (>= 0, finite) is
 * the caller's guard against the surfaces the endpoints lie on; the render's own is 1e-3.  A range
 * that comes out empty, L - skin < skin, is visible.
 */
rm_status rm_visible_segments(rm_ctx *ctx, const rm_vec3 *from, const rm_vec3 *to, uint32_t n, double skin,
                              uint8_t *visible);
rm_status rm_visible_segments_device(rm_ctx *ctx, const void *device_from, const void *device_to, uint32_t n,
                                     double skin, void *device_visible, void *hip_stream);
/*
 * Which lights reach a surface point: lit is [n_points][n_lights] bytes.  For point P, normal N and
 * light j, renderer.rs:166-174 exactly, each operation rounded once:
 * light_dir = normalized(light.position - P); the origin is P - N.scaled(1e-3) if light_dir . N < 0,
 * else P + N.scaled(1e-3).
 *   RM_LIGHTS_AS_RENDERED: lit = !intersect_shape_set(origin, light_dir), unbounded: bit for bit
 *     the decision direct_lighting takes, a shape BEHIND the light shadows.
 *   RM_LIGHTS_CLIPPED: the same ray in the range [0, |light.position - P|] (the norm normalized
 *     computed): a shape behind the light no longer shadows.
 * n_lights must be the resident scene's (it sizes lit), else RM_ERR_INVALID_ARG; a scene without
 * lights is RM_OK and writes nothing.
 */
#define RM_LIGHTS_AS_RENDERED 0u
#define RM_LIGHTS_CLIPPED 1u
rm_status rm_lights_visible(rm_ctx *ctx, const rm_vec3 *points, const rm_vec3 *normals, uint32_t n_points,
                            uint32_t n_lights, uint32_t mode, uint8_t *lit);
rm_status rm_lights_visible_device(rm_ctx *ctx, const void *device_points, const void *device_normals,
                                   uint32_t n_points, uint32_t n_lights, uint32_t mode, void *device_lit,
                                   void *hip_stream);

/* ---- the oriented camera: look-at and turn for renders and pixel queries ------------------
 *
 * The reference's camera is a point (scene.rs:12) that always looks down -z with +y up
 * (backproject, renderer.rs:128-135).  A context can be given a view direction as well: three
 * world-space unit vectors, right, up and forward.  The fixed view is right (1,0,0), up (0,1,0),
 * forward (0,0,-1).  Additive to ABI version 5; a host detects it by " camera" in
 * rm_build_info().
 *
 * With bx = 2 (x / width - 0.5) half_fov ratio and by = -2 (y / height - 0.5) half_fov, the two
 * numbers backproject forms for pixel (x, y), the primary ray of the pixel leaves the camera
 * position along, per component c,
 *     d.c = (bx * right.c + by * up.c) + forward.c
 * (strict flavour: two products and two sums, each rounded once, in this order, no fused
 * multiply-add; the fast flavour may contract), normalised as every direction is.  Nothing else
 * changes: same patches and rows, same shading, same frame formats.
 *
 * The oriented state belongs to the context, like rm_camera_update's position: it is off after
 * rm_init, survives rm_scene_upload (which still sets the position from desc.camera), and holds
 * for every render entry point, every stream and frame slot, rm_pick and rm_primary_hits_device.
 * The ray-list queries take the caller's rays and are not concerned.  While it is off every
 * launch runs the fixed view's kernels and gives the fixed view's frames bit for bit.  A basis
 * whose nine components compare equal (==) to the fixed view's turns it off again rather than
 * on: "identity" never differs from "unset".
 *
 * A basis is accepted when all nine numbers are finite, every vector's squared length is
 * within 1e-12 of 1 and every pairwise dot product within 1e-12 of 0; otherwise
 * RM_ERR_INVALID_ARG, and the context keeps what it had.  Left-handed bases are accepted (the
 * picture is mirrored).
 */
typedef struct rm_camera_basis {
    rm_vec3 right, up, forward;
} rm_camera_basis;

/* Sets the context's view direction; basis == NULL resets it to the fixed view. */
rm_status rm_camera_orient(rm_ctx *ctx, const rm_camera_basis *basis);
/* rm_camera_update(eye) and rm_camera_orient(rm_camera_basis_look_at(eye, target, up_hint)) in
 * one call; on failure neither is changed.  Needs an uploaded scene, as rm_camera_update. */
rm_status rm_camera_look_at(rm_ctx *ctx, rm_vec3 eye, rm_vec3 target, rm_vec3 up_hint);
/* What the context renders with: position, basis (the fixed view's while the state is off),
 * and whether the oriented state is on.  Every out-pointer is optional. */
rm_status rm_camera_get(rm_ctx *ctx, rm_vec3 *position, rm_camera_basis *basis, int *oriented);
/* Host arithmetic only -- no GPU, no context:
 * forward = unit(target - eye), right = unit(forward x up_hint), up = right x forward.
 * RM_ERR_INVALID_ARG for eye == target, an up_hint parallel to the line of sight (or zero),
 * non-finite input.  eye (0,0,0), target (0,0,-1), up_hint (0,1,0) gives a basis that compares
 * equal to the fixed view. */
rm_status rm_camera_basis_look_at(rm_vec3 eye, rm_vec3 target, rm_vec3 up_hint, rm_camera_basis *out);
/* Turns a basis about its own axes, in this order: yaw about up, pitch about right, roll about
 * forward (radians), then makes it orthonormal again (a thousand small turns still pass the
 * check; handedness is kept).  Positive yaw turns left (counter-clockwise seen from the tip of
 * up: the fixed view yawed by pi/2 looks down -x), positive pitch looks up (forward towards
 * up), positive roll tips the camera's up towards its right.  in == out is allowed. */
rm_status rm_camera_basis_turn(const rm_camera_basis *in, double yaw, double pitch, double roll, rm_camera_basis *out);
/* RM_OK where rm_camera_orient would accept the basis. */
rm_status rm_camera_basis_check(const rm_camera_basis *basis);

/* ---- radiance queries: the caller's rays and sub-pixel samples, shaded ---------------------
 * The queries above stop before shading.  These return what cast_ray (renderer.rs:254-309) returns
 * along a ray: closest hit, direct lighting, reflected and refracted children -- for rays the caller
 * names, and for real-valued sample positions of the frame `params` describes (anti-aliasing, a
 * sparse second view).  Additive to ABI version 5; a host detects them by " radiance" in
 * rm_build_info().  Everything "Semantics common to every query" says holds: the resident scene
 * (RM_ERR_NO_SCENE without one), the strict numeric flavour whatever params->flags says
 * (RM_FLAG_FAST_FP tolerated and ignored, no other flag), the default band only, device variants
 * asynchronous on hip_stream and host variants blocking, n == 0 is RM_OK, no render state touched.
 *
 *   - Depth.  Every ray is cast as the render casts a primary ray, n_recursion = 1, with the cap
 *     max_depth in place of the reference's 3.  A ray that leaves the scene returns exactly
 *     (+0, +0, +0), not the background (renderer.rs:302-306); a child that leaves the scene adds its
 *     weight times the background, and so does a child beyond the cap (renderer.rs:262-264).
 *     max_depth == 0 returns the background for every ray; max_depth > RM_MAX_DEPTH is RM_ERR_DEPTH.
 *   - Viewer direction.  direct_lighting's dir_to_viewer is normalize(origin - point)
 *     (renderer.rs:149), and that is what the specular term takes at every ray step, formed from
 *     the step's own origin and hit point -- not the ray's direction turned round.  The two agree
 *     to rounding wherever the hit lies a way down the ray; they do not for a ray that starts ON
 *     a surface: point == origin gives the zero vector (the reference adds no specular light
 *     there), and a hit an ulp or two from the origin gives what the rounding of
 *     origin + dir * t left.  Everything else -- the intersection tests, the reflected and
 *     refracted children -- takes the caller's direction as it is, as the reference does.
 *   - Shadow rays are walked without the per-primitive occluder masks of the render (they hold for
 *     rays cast from near the scene; a ray list has no such bound).  The decisions are the same.
 *   - Sample rays.  A sample (sx, sy), sx the real-valued column and sy the row, is the ray
 *     backproject (renderer.rs:128-135) would form there: with params' Renderer
 *         bx = 2 * (sx / width - 0.5) * half_fov * ratio
 *         by = -2 * (sy / height - 0.5) * half_fov
 *     every operation rounded once, in this order, with exact divisions -- for integer (sx, sy) the
 *     numbers of the render's own pixel, bit for bit, and there is no pixel-centre offset.  The ray
 *     leaves the context's camera position along normalized(bx, by, -1), or under an oriented
 *     context along normalized((bx * right + by * up) + forward) as the camera section states it.
 *     frame_width need not be a multiple of 32, and the frame_height % 32 rows the render leaves
 *     untouched are answered too, as for rm_pick.  max_depth and background are params'.
 *   - The host variants check everything before anything is launched: what the ray queries check
 *     of origins and directions; shading != NULL and a finite background; samples finite with
 *     0 <= sx < frame_width and 0 <= sy < frame_height.  RM_ERR_INVALID_ARG names the first offender
 *     in rm_last_error, nothing is computed and the output is untouched.  For the device variants
 *     the per-element conditions are preconditions: a bad element gets an unspecified answer for
 *     that element, never a fault.
 */
typedef struct rm_shading {
    rm_vec3  background;
    uint32_t max_depth;
    uint32_t _pad;
} rm_shading;           /* 32 bytes */

/* rgb[i] = cast_ray(origins[i], directions[i], scene.shapes, scene.lights, background, 1) with the cap max_depth. */
rm_status rm_radiance_rays(rm_ctx *ctx, const rm_vec3 *origins, const rm_vec3 *directions, uint32_t n_rays,
                           const rm_shading *shading, rm_vec3 *rgb);
rm_status rm_radiance_rays_device(rm_ctx *ctx, const void *device_origins, const void *device_directions,
                                  uint32_t n_rays, const rm_shading *shading, void *device_rgb, void *hip_stream);
/* xy: n pairs (sx, sy) of real-valued pixel coordinates; rgb[i] the radiance along the ray of sample i. */
rm_status rm_radiance_samples(rm_ctx *ctx, const rm_params *params, const double *xy, uint32_t n, rm_vec3 *rgb);
rm_status rm_radiance_samples_device(rm_ctx *ctx, const rm_params *params, const void *device_xy, uint32_t n,
                                     void *device_rgb, void *hip_stream);

/* ---- adaptive anti-aliasing: refine only the high-contrast pixels of a rendered frame --------
 * A render casts one ray a pixel; these calls find the pixels that differ strongly from a neighbour
 * and replace those alone by the mean of n x n radiance samples, on the device, in place.  Additive
 * to ABI version 5; a host detects them by " antialias" in rm_build_info().
 *
 * Let rows = frame_height - frame_height % 32, the rows a render writes, and f the frame
 * rm_render_device wrote for `params`: [frame_height][frame_width][3] doubles, the plain layout (no
 * compact flag), the default band.
 *
 *   - Contrast.  The contrast of pixel (x, y), y < rows, is the largest |f[y][x][c] - f[q][c]| over
 *     the three channels c and over its up-to-four neighbours q (left, right, above, below) that lie
 *     in [0, frame_width) x [0, rows): row rows - 1 never looks at row rows, and a pixel without a
 *     neighbour has contrast 0.  It is taken on the radiance as rendered, neither normalised nor
 *     clamped; a NaN makes its comparisons false.
 *   - Mask.  A pixel is refined iff its contrast is > threshold.  threshold = +inf refines nothing,
 *     a negative threshold every pixel of [0, rows).  The mask is the unrefined frame's for every
 *     pixel: it is complete before any pixel is overwritten.
 *   - Refined value.  The mean of the radiance at (x + i/n, y + j/n), i, j in 0..n-1.  Each sample
 *     is what rm_radiance_samples returns for that position with the same params: the "sample rays"
 *     rule above (the oriented context's where the context is oriented), the strict flavour,
 *     params' max_depth and background, occluder masks off.  The samples are summed per channel in
 *     the order j outer, i inner, by plain additions, and the sum is divided once by (double)(n*n).
 *     All n*n samples are cast, the one at i = j = 0 included: a frame refined with a negative
 *     threshold is the supersampled frame.
 *   - Unrefined pixels keep the bytes the render wrote; rows from `rows` on are not touched.
 *
 * rm_refine_device is asynchronous on hip_stream: no host synchronisation, nothing copied back.
 * After it the first uint32_t of the workspace holds the number of refined pixels and their indices
 * y * frame_width + x follow, in no particular order -- the list is an output.  device_mask, where
 * given, gets 1 or 0 for every pixel of [0, rows) and is untouched below.  Everything "Semantics
 * common to every query" says holds: the resident scene (RM_ERR_NO_SCENE without one),
 * RM_FLAG_FAST_FP tolerated and ignored and any other flag RM_ERR_INVALID_ARG, the default band
 * only, no render state touched; frame_width % 32 != 0 is RM_ERR_DIMENSIONS and max_depth >
 * RM_MAX_DEPTH is RM_ERR_DEPTH.  n outside 1..8, a NaN threshold, a non-finite background, or a
 * NULL refine, frame or workspace is RM_ERR_INVALID_ARG with the offender named in rm_last_error;
 * nothing is launched then.  rows == 0 is RM_OK and does nothing.  All state lives in the
 * workspace: two calls with different workspaces may be in flight on different streams.
 *
 * rm_render_antialiased is what a host calls for an anti-aliased frame: it renders exactly as
 * rm_render does with params (the render state advances as a render's does), refines the context's
 * resident frame on the context's stream with a workspace the context owns (grown on demand, freed
 * by rm_destroy), copies the rows [0, rows) to host_rgb and the count to n_refined, and blocks.
 * Compact flags or a non-default band are RM_ERR_INVALID_ARG.  timing->kernel_ms covers render plus
 * refine.
 */
typedef struct rm_refine {
    uint32_t n;           /* n x n samples a refined pixel, 1..8 */
    uint32_t _pad;
    double   threshold;   /* a pixel is refined iff its contrast is > threshold */
} rm_refine;            /* 16 bytes */

/* bytes of device memory rm_refine_device needs for `params`: 4 * (1 + rows * frame_width), rounded up to 256 */
rm_status rm_refine_workspace(const rm_params *params, size_t *bytes);
/* refines, in place, a frame rm_render_device wrote with the same params, camera and scene */
rm_status rm_refine_device(rm_ctx *ctx, const rm_params *params, const rm_refine *refine, void *device_rgb,
                           void *device_workspace, void *device_mask /* optional: [frame_height][frame_width] bytes */,
                           void *hip_stream);
/* rm_render + refine + copy */
rm_status rm_render_antialiased(rm_ctx *ctx, const rm_params *params, const rm_refine *refine, double *host_rgb,
                                uint32_t *n_refined /* optional */, rm_timing *timing /* optional */);

/* ---- thin-lens camera: depth-of-field frames sampled and resolved on the device -------------
 * Every camera above is a point.  These calls render a frame through a lens of radius `aperture`
 * that is sharp at the distance `focus` along the context's forward direction: n_samples rays a
 * pixel, each through a point of the lens of its own, formed, shaded and averaged on the device --
 * no ray list, no sample in global memory.  Additive to ABI version 5; a host detects them by
 * " lens" in rm_build_info().
 *
 * A sample table is n_samples rows of four doubles (dx, dy, u, v): (dx, dy) a sub-pixel offset,
 * 0 <= dx, dy < 1, and (u, v) a point of the unit disc, u*u + v*v <= 1.  Let rows = frame_height -
 * frame_height % 32.  For pixel (x, y), y < rows, and table row s:
 *
 *   1. Direction.  sx = x + dx, sy = y + dy; D is the un-normalised direction of the "sample rays"
 *      rule above at (sx, sy): per component (bx * right + by * up) + forward with the context's
 *      basis, exactly (bx, by, -1) under a context that is not oriented.  The forward component of
 *      D in the camera frame is exactly 1, so cam + D * focus lies in the plane in focus.
 *   2. Focus point.  Per component F.c = cam.c + D.c * focus: one product and one sum, each
 *      rounded once, no fused multiply-add.
 *   3. Lens point.  au = aperture * u, av = aperture * v; per component
 *      O.c = cam.c + ((au * right.c) + (av * up.c)), the fixed view's right (1,0,0) and up (0,1,0)
 *      under a context that is not oriented.
 *   4. Ray.  Origin O, direction normalized(F - O).  Exception: when aperture == 0 the ray is the
 *      sample ray itself, origin cam and direction normalized(D).  A lens frame with aperture 0 and
 *      the table (i/n, j/n, 0, 0), j outer and i inner, is therefore the supersampled frame: byte
 *      for byte what rm_refine_device leaves at a negative threshold.
 *   5. Radiance.  What rm_radiance_rays returns for that ray with params' max_depth and background:
 *      n_recursion = 1, a primary ray that leaves the scene returns (+0, +0, +0), the strict
 *      flavour, occluder masks off.
 *   6. Pixel value.  The samples are summed per channel in table order by plain additions and the
 *      sum is divided once by (double)n_samples.  max_depth == 0 writes the background.
 *   7. Rows from `rows` on are neither read nor written.  Render state is neither read nor
 *      written; the context's camera position and basis are read, nothing else of the context.
 *
 * rm_lens_table fills the library's own table, host arithmetic only (no context, no GPU, no libm
 * beyond sqrt), every operation rounded once in this order: m = ceil(sqrt(n_samples)) as an
 * integer; row s has i = s % m, j = s / m, dx = i / m, dy = j / m; the lens cell is decorrelated
 * from the pixel cell, a = (2*j + 1) / m - 1, b = (2*(m - 1 - i) + 1) / m - 1, and mapped to the
 * disc by u = a * sqrt(1 - b*b/2), v = b * sqrt(1 - a*a/2).  n_samples == 1 gives (0, 0, 0, 0).
 * n_samples outside 1..64 or a NULL table is RM_ERR_INVALID_ARG.
 *
 * rm_render_lens_device is asynchronous on hip_stream: no host synchronisation.  device_table is
 * n_samples * 4 doubles in device memory (rm_buffer_alloc / rm_buffer_write), device_rgb is
 * [frame_height][frame_width][3] doubles, the plain layout.  The table's contents are a
 * precondition here: a bad row gives unspecified pixels, never a fault.  rm_render_lens takes the
 * table from host memory, checks every entry of it (finite, 0 <= dx, dy < 1, u*u + v*v <= 1 +
 * 1e-12), stages it into a buffer the context owns, renders on the context's stream into a lens
 * frame the context owns (grown on demand, freed by rm_destroy; not the resident frame of
 * rm_render), copies the rows [0, rows) to host_rgb and blocks.  timing->kernel_ms is the launch.
 *
 * Checked before anything is launched, the offender named in rm_last_error, nothing computed and
 * the output untouched: everything rm_refine_device checks of params (RM_ERR_NO_SCENE;
 * RM_FLAG_FAST_FP tolerated and ignored, any other flag RM_ERR_INVALID_ARG; the default band only;
 * frame_width % 32 != 0 is RM_ERR_DIMENSIONS, and so is rows * frame_width >= 2^31; max_depth >
 * RM_MAX_DEPTH is RM_ERR_DEPTH; a finite background); lens, table and frame not NULL; aperture
 * finite and >= 0; focus finite and > 0; n_samples in 1..64.  rows == 0 is RM_OK and does nothing.
 */
typedef struct rm_lens {
    double   aperture;    /* lens radius, world units; finite, >= 0 */
    double   focus;       /* distance of the plane in focus along `forward`; finite, > 0 */
    uint32_t n_samples;   /* rays a pixel, 1..64 */
    uint32_t _pad;
} rm_lens;              /* 24 bytes */

/* the library's sample table for n_samples rays a pixel: n_samples * 4 doubles */
rm_status rm_lens_table(uint32_t n_samples, double *table);
rm_status rm_render_lens_device(rm_ctx *ctx, const rm_params *params, const rm_lens *lens, const void *device_table,
                                void *device_rgb, void *hip_stream);
rm_status rm_render_lens(rm_ctx *ctx, const rm_params *params, const rm_lens *lens, const double *table,
                         double *host_rgb, rm_timing *timing /* optional */);

/* ---- progressive frames: lens samples accumulated across calls on the device ----------------
 * A lens frame is finished in one call, with at most 64 samples a pixel.  These calls refine a
 * standing view instead: every call casts a few more samples and continues a per-pixel sum, so a
 * viewer adds samples a tick while nothing moves and starts again when anything does.  Additive to
 * ABI version 5; a host detects them by " progressive" in rm_build_info().
 *
 * rm_lens_sequence fills rows first .. first + count - 1 of one fixed sample sequence, count * 4
 * doubles (dx, dy, u, v) per the sample table's conventions above; every prefix of the sequence is
 * well spread.  Host arithmetic only (no context, no GPU, no libm beyond sqrt), every operation
 * rounded once in this order.  For index s and base b, in uint64_t: r = 0, q = 1; while s > 0:
 * r = r*b + s % b, q *= b, s /= b; phi_b(s) = (double)r / (double)q, one division (s = 0 gives 0).
 * Row s is dx = phi_2(s), dy = phi_3(s); a = 2. * phi_5(s) - 1., b = 2. * phi_7(s) - 1.;
 * u = a * sqrt(1. - b*b/2.), v = b * sqrt(1. - a*a/2.), the map of rm_lens_table.  Row 0 is
 * (0, 0, -sqrt(.5), -sqrt(.5)); every row satisfies the table conditions rm_render_lens checks.
 * first + count > RM_PROGRESSIVE_MAX_SAMPLES is RM_ERR_INVALID_ARG; count == 0 is RM_OK, nothing is
 * written and table may be NULL; a NULL table with count > 0 is RM_ERR_INVALID_ARG.
 *
 * rm_accumulate_lens_device is asynchronous on hip_stream: no host synchronisation.  It neither
 * reads nor writes render state, as rm_render_lens_device.  lens->n_samples (1..64) rows of
 * device_table are cast for every pixel of [0, rows) x [0, frame_width), rows = frame_height -
 * frame_height % 32; rays and radiance are exactly steps 1-5 of the thin-lens camera, the
 * aperture == 0 exception included.  device_sum, device_mean and device_rgb8 are
 * [frame_height][frame_width][3] in the plain layout, the first two of doubles, the third of bytes:
 *
 *   Sum.    Per channel, S starts as device_sum[pix] when n_before > 0.  When n_before == 0 it
 *           starts as the first sample itself, and device_sum is not read and may hold anything.
 *           The remaining samples are added in table order by plain additions, and S is stored to
 *           device_sum[pix].
 *   Mean.   S / (double)(n_before + n_samples), one division, is stored to device_mean where given.
 *   Bytes.  (uint8_t)(255. * fmin(fmax(mean, 0.), 1.)) per channel -- to_vec, the rule of the
 *           display bytes of rm_render_display -- is stored to device_rgb8 where given.
 *   max_depth == 0: every sample is the background.
 *   Rows from `rows` on are neither read nor written in any of the three buffers.
 *
 * So with n_before == 0, device_mean is byte for byte what rm_render_lens_device writes for the
 * same table; and passes over consecutive slices of one table T of at most 64 rows, each taking the
 * previous total as n_before, are the same left fold as one lens launch: the last device_mean is
 * byte for byte the lens frame of T.
 *
 * Checked before anything is launched, the offender named in rm_last_error, nothing computed and
 * no buffer touched: everything rm_render_lens_device checks of params and lens; device_table and
 * device_sum not NULL; device_mean != device_sum; n_before + n_samples <=
 * RM_PROGRESSIVE_MAX_SAMPLES, else RM_ERR_INVALID_ARG.  rows == 0 is RM_OK and does nothing.
 *
 * rm_render_progressive is the call a viewer makes every tick.  The context owns a sum, a mean and
 * a byte buffer (grown on demand, freed by rm_destroy; not the resident frame of rm_render and not
 * the lens frame of rm_render_lens), a staged table, the number N of samples in the sum and a key:
 * the bytes of params' fov, half_fov, height, width, ratio, frame_width, frame_height, max_depth and
 * background, of lens->aperture and lens->focus, of the context's camera position, oriented flag
 * and basis, and of the `copies` counter of rm_scene_uploads.  RM_FLAG_FAST_FP is tolerated,
 * ignored and not part of the key.  If restart != 0, or the key differs from the previous
 * successful call's, or there was none, N = 0.  The call stages rows [N, N + n_samples) of
 * rm_lens_sequence, launches the accumulation on the context's stream with n_before = N, sets
 * N += n_samples, copies the rows [0, rows) of the mean to host_rgb and of the bytes to host_rgb8
 * where given and the total to *n_total, and blocks until all that is done.  If N + n_samples >
 * RM_PROGRESSIVE_MAX_SAMPLES nothing is launched, the outputs are the frame as it stands and the
 * call returns RM_OK with *n_total = N: ticking a converged picture is not an error.  The checks
 * are the device call's of params and lens; a refused call changes neither N nor the key.  rows == 0
 * is RM_OK, does nothing and reports a total of 0.  timing->kernel_ms is the launch.  The call
 * changes no frame any other entry point produces and leaves the launch and upload counters of
 * renders alone, as the lens calls do.
 */
#define RM_PROGRESSIVE_MAX_SAMPLES 65536u

rm_status rm_lens_sequence(uint32_t first, uint32_t count, double *table);
rm_status rm_accumulate_lens_device(rm_ctx *ctx, const rm_params *params, const rm_lens *lens, const void *device_table,
                                    uint32_t n_before, void *device_sum, void *device_mean /* optional */,
                                    void *device_rgb8 /* optional */, void *hip_stream);
rm_status rm_render_progressive(rm_ctx *ctx, const rm_params *params, const rm_lens *lens, int restart,
                                double *host_rgb /* optional */, uint8_t *host_rgb8 /* optional */,
                                uint32_t *n_total /* optional */, rm_timing *timing /* optional */);

/* ---- area lights: soft shadows in progressive frames -----------------------------------------
 * Every light of a scene is a point, so every shadow edge is hard however many samples a frame
 * holds.  These calls give each sample of a progressive frame light positions of its own: a light
 * of radius r is sampled on the sphere of radius r about its position, and the mean converges to a
 * picture with penumbrae.  Additive to ABI version 5; a host detects them by " soft" in
 * rm_build_info().
 *
 * A light offset table is [n_samples][n_lights][3] doubles in world units.  For sample row s and
 * light l the light stands at P'.c = P.c + off[s][l].c per component, P the resident scene's
 * position: one addition, rounded once.  Everything direct_lighting does for that light takes P' in
 * place of P -- light_dir = normalized(P' - point), the side test, the shadow ray's origin and
 * direction, the diffuse and the specular term -- at every ray step of the sample: the primary hit
 * and the reflected and refracted children.  Colour and intensity are the scene's; there is no
 * fall-off with distance and shadow rays are unbounded, as rendered.  Everything else is steps 1-5
 * of the thin-lens camera and the sum, mean and bytes of the progressive frames, word for word.
 * With every offset +0. or -0. a frame is byte for byte what rm_accumulate_lens_device writes,
 * for light coordinates that are not -0. (-0. + +0. is +0.).
 *
 * rm_light_sequence fills rows first .. first + count - 1 of one fixed offset sequence,
 * count * n_lights * 3 doubles.  Host arithmetic only (no context, no GPU, no libm beyond sqrt and
 * floor), every operation rounded once in this order.  With phi_b as in rm_lens_sequence, for index
 * s and light l: x = phi_11(s) + (double)l * 0.6180339887498949, x = x - floor(x);
 * y = phi_13(s) + (double)l * 0.6180339887498949, y = y - floor(y); a = 2.*x - 1., b = 2.*y - 1.;
 * u = a * sqrt(1. - b*b/2.), v = b * sqrt(1. - a*a/2.); r2 = u*u + v*v,
 * h = 2. * sqrt(fmax(1. - r2, 0.)); e = (u*h, v*h, 1. - 2.*r2) -- the disc of rm_lens_table lifted
 * to the unit sphere -- and off[s][l] = (radii[l]*e.x, radii[l]*e.y, radii[l]*e.z).  A radius of 0
 * gives zeros.  first + count > RM_PROGRESSIVE_MAX_SAMPLES, a radius that is not a finite number
 * >= 0, and a NULL radii or offsets with something to write are RM_ERR_INVALID_ARG, nothing is
 * written; count == 0 or n_lights == 0 is RM_OK, nothing is written.
 *
 * rm_accumulate_soft_device is rm_accumulate_lens_device with the offset table: asynchronous on
 * hip_stream, neither reading nor writing render state, the same checks, and: n_lights must be the
 * resident scene's (as rm_lights_visible requires); device_offsets must not be NULL when
 * n_lights > 0 -- a scene without lights takes a NULL table.  lens->n_samples rows of
 * device_offsets are read.  Their contents are a precondition: a non-finite offset gives
 * unspecified pixels, never a fault.
 *
 * rm_render_progressive_soft is the viewer's tick with area lights: rm_render_progressive on the
 * same context-owned sum, mean and bytes and the same count N, with the key extended by n_lights
 * and the bytes of radii (rm_render_progressive counts as "no radii").  So the frame begins again
 * when a radius changes, when a caller switches between the two calls in either direction, and on
 * everything that begins it again in rm_render_progressive; it continues otherwise.  The call
 * stages rows [N, N + n_samples) of rm_lens_sequence and of rm_light_sequence (buffers the context
 * owns, grown on demand, freed by rm_destroy).  Checked before anything else happens: radii finite
 * and >= 0 (NULL only when n_lights == 0), n_lights the resident scene's; a refused call changes
 * neither N nor the key.  Saturation, rows == 0, timing and the counters are rm_render_progressive's.
 */
rm_status rm_light_sequence(uint32_t first, uint32_t count, const double *radii, uint32_t n_lights, double *offsets);
rm_status rm_accumulate_soft_device(rm_ctx *ctx, const rm_params *params, const rm_lens *lens, const void *device_table,
                                    const void *device_offsets, uint32_t n_lights, uint32_t n_before, void *device_sum,
                                    void *device_mean /* optional */, void *device_rgb8 /* optional */, void *hip_stream);
rm_status rm_render_progressive_soft(rm_ctx *ctx, const rm_params *params, const rm_lens *lens, const double *radii,
                                     uint32_t n_lights, int restart, double *host_rgb /* optional */,
                                     uint8_t *host_rgb8 /* optional */, uint32_t *n_total /* optional */,
                                     rm_timing *timing /* optional */);

/* ---- moving spheres: motion blur in progressive frames ----------------------------------------
 * A scene whose spheres move renders as one frozen instant, however many samples a frame holds.
 * These calls give each sample of a progressive frame sphere positions of its own -- a sphere of
 * velocity v is seen where it stands at the sample's own time within the shutter -- and the mean
 * converges to a picture blurred along the motion.  Additive to ABI version 5; a host detects them
 * by " motion" in rm_build_info().
 *
 * Spheres only in these calls.  The reference has no offset for spheres, so one addition per
 * component defines a moved sphere.  Polygons and meshes move in the calls of the next section,
 * "moving shapes": the reference defines their offset itself and the device records hold the very
 * quantities it moves, so that is bit for bit too; these calls keep refusing such a velocity.
 *
 * A shape offset table is [n_samples][n_shapes][3] doubles in world units, indexed by the shape's
 * index in the scene's shape list: the index rm_scene_offset_shape takes and rm_hit.shape reports.
 * For sample row s and a shape k that is a sphere the centre is C'.c = C.c + off[s][k].c per
 * component, C the resident scene's: one addition, rounded once.  C' takes C's place in everything
 * the sample does with that sphere, at every ray step: the closest-hit test, every shadow test and
 * the normal normalized(point - C'), for the primary hit and for the reflected and refracted
 * children.  radius_square and the material are the scene's.  Rows of shapes that are not spheres
 * are never read.  Everything else is the area lights' frame word for word: steps 1-5 of the
 * thin-lens camera, the light offset table, and the sum, mean and bytes of the progressive frames.
 * With every shape offset +0. or -0. a frame is byte for byte what rm_accumulate_soft_device writes
 * for the same tables, for centre coordinates that are not -0. (-0. + +0. is +0.).
 *
 * Cost: the kernels of these calls test every primitive against every ray (the flat walk, what
 * RM_DISABLE_BVH=1 selects elsewhere), whatever hierarchies the scene image holds: a hierarchy's
 * boxes hold for the uploaded centres only.  A scene of hundreds of spheres or a mesh pays for it.
 *
 * rm_motion_sequence fills rows first .. first + count - 1 of one fixed offset sequence,
 * count * n_shapes * 3 doubles.  Host arithmetic only (no context, no GPU, no libm), every
 * operation rounded once.  With phi_b as in rm_lens_sequence -- bases 2, 3, 5, 7, 11 and 13 are the
 * lens' and the lights' -- for index s: t = shutter * phi_17(s), and off[s][k].c =
 * velocities[k].c * t.  Row 0 is the scene as uploaded, at shutter open.  first + count >
 * RM_PROGRESSIVE_MAX_SAMPLES, a velocity component or a shutter that is not finite, shutter < 0,
 * and a NULL velocities or offsets with something to write are RM_ERR_INVALID_ARG, nothing is
 * written; count == 0 or n_shapes == 0 is RM_OK, nothing is written.
 *
 * rm_accumulate_motion_device is rm_accumulate_soft_device with one more pair of arguments:
 * asynchronous on hip_stream, neither reading nor writing render state, the same checks, and:
 * n_shapes must be the resident scene's shape count; device_shape_offsets must not be NULL when the
 * scene holds a sphere.  Both tables are required where their count is not zero -- a caller with
 * point lights passes zeros -- and lens->n_samples rows of each are read.  Their contents are a
 * precondition: a non-finite offset gives unspecified pixels, never a fault.
 *
 * rm_render_progressive_motion is the viewer's tick: rm_render_progressive_soft on the same
 * context-owned sum, mean and bytes and the same count N, with the key extended by n_shapes, the
 * bytes of velocities and of shutter.  radii == NULL is "no radii" (point lights, n_lights is not
 * looked at) and stages zeros.  So the frame begins again when a velocity or the shutter changes,
 * when a caller switches between the three calls, and on everything that begins it again in
 * rm_render_progressive_soft; it continues otherwise.  The call stages rows [N, N + n_samples) of
 * rm_lens_sequence, rm_light_sequence and rm_motion_sequence (buffers the context owns).  Checked
 * before anything else happens: rm_render_progressive_soft's checks (the radii only where given),
 * n_shapes the resident scene's, velocities and shutter as rm_motion_sequence demands, and a
 * velocity that is not zero for a shape that is not a sphere -- RM_ERR_INVALID_ARG, the shape named
 * in rm_last_error; a refused call changes neither N nor the key.  Saturation, rows == 0, timing
 * and the counters are rm_render_progressive's.
 */
rm_status rm_motion_sequence(uint32_t first, uint32_t count, const rm_vec3 *velocities, uint32_t n_shapes, double shutter,
                             double *offsets);
rm_status rm_accumulate_motion_device(rm_ctx *ctx, const rm_params *params, const rm_lens *lens, const void *device_table,
                                      const void *device_light_offsets, uint32_t n_lights, const void *device_shape_offsets,
                                      uint32_t n_shapes, uint32_t n_before, void *device_sum, void *device_mean /* optional */,
                                      void *device_rgb8 /* optional */, void *hip_stream);
rm_status rm_render_progressive_motion(rm_ctx *ctx, const rm_params *params, const rm_lens *lens,
                                       const double *radii /* NULL: point lights */, uint32_t n_lights,
                                       const rm_vec3 *velocities, uint32_t n_shapes, double shutter, int restart,
                                       double *host_rgb /* optional */, uint8_t *host_rgb8 /* optional */,
                                       uint32_t *n_total /* optional */, rm_timing *timing /* optional */);

/* ---- moving shapes: motion blur for spheres, polygons and meshes -------------------------------
 * The moving spheres' calls obey a velocity on a sphere alone.  These obey one on any shape: the
 * fourth member of the progressive family, beside plain, area lights and moving spheres.  Additive
 * to ABI version 5; a host detects them by " moving-shapes" in rm_build_info().
 *
 * The shape offset table is the moving spheres': [n_samples][n_shapes][3] doubles in the order of
 * the scene's shape list.  For sample row s and shape k:
 *   sphere:   as in "moving spheres": C' = C + off[s][k].
 *   polygon:  plane_point' = plane_point + off[s][k] and every vertex v' = v + off[s][k]
 *             (polygon.rs:44-49); only x and y of a vertex are ever used (polygon.rs:54-56).  The
 *             normal and the material are the scene's.
 *   Obj:      every triangle gets center' = center + off[s][k] and v' = v + off[s][k]
 *             (triangle.rs:19-24, obj.rs:24-29).  The normals and the per-triangle materials are
 *             the scene's.
 * Each is one addition per component, rounded once.  The moved record takes the stored one's place
 * in everything the sample does with that primitive, at every ray step and for the reflected and
 * refracted children too: the closest-hit test (a polygon's fifth and further vertices included)
 * and every shadow test -- where two shadow rays share a walk, the plane numerator they share is
 * formed from the moved point.  A hit's point is orig + dir * t and its normal the stored one.
 * The hit tests form (p + off) - orig and (v + off) - a, what the reference forms after offset(),
 * so a sample is the reference's render of the moved scene operation for operation.
 *
 * Rows of every shape are read, so the whole table is a precondition: a non-finite entry gives
 * non-finite pixels, never a fault.  With every offset +0. or -0. a pass is byte for byte
 * rm_accumulate_motion_device's for the same tables, for stored coordinates that are not -0.; with
 * zero rows for every shape that is not a sphere it is byte for byte the moving spheres' pass with
 * those sphere rows.
 *
 * Cost: the moving spheres' -- the flat walk whatever hierarchies the scene image holds, no cull,
 * no occluder masks, no tile masks -- plus three per-lane loads a shape and walk and one addition
 * at each use of a coordinate.
 *
 * rm_accumulate_moving_device has rm_accumulate_motion_device's argument list and checks, except
 * that device_shape_offsets must not be NULL when the scene holds any shape.
 *
 * rm_render_progressive_moving has rm_render_progressive_motion's argument list and is the same
 * tick on the same context-owned sum, mean, bytes and count N, with the same checks but for the
 * refusal of a velocity on a shape that is not a sphere.  Its frames are not the moving spheres':
 * switching between the two calls begins the frame again, equal velocities or not.  The tables are
 * rm_lens_sequence's, rm_light_sequence's and rm_motion_sequence's rows [N, N + n_samples).
 *
 * Not here: moving shapes in converging frames, rotation or deformation.
 */
rm_status rm_accumulate_moving_device(rm_ctx *ctx, const rm_params *params, const rm_lens *lens, const void *device_table,
                                      const void *device_light_offsets, uint32_t n_lights, const void *device_shape_offsets,
                                      uint32_t n_shapes, uint32_t n_before, void *device_sum, void *device_mean /* optional */,
                                      void *device_rgb8 /* optional */, void *hip_stream);
rm_status rm_render_progressive_moving(rm_ctx *ctx, const rm_params *params, const rm_lens *lens,
                                       const double *radii /* NULL: point lights */, uint32_t n_lights,
                                       const rm_vec3 *velocities, uint32_t n_shapes, double shutter, int restart,
                                       double *host_rgb /* optional */, uint8_t *host_rgb8 /* optional */,
                                       uint32_t *n_total /* optional */, rm_timing *timing /* optional */);

/* ---- converging frames: progressive frames that sample only the pixels still noisy ------------
 * A pass of a progressive frame casts n_samples rays for every pixel, however long most of them
 * have stopped changing.  These calls keep a sample count and an error estimate per pixel, list the
 * pixels still noisy on the device, and shade the listed pixels alone -- each continuing the sample
 * sequence where that pixel stopped.  A viewer learns when the picture is finished: nothing is
 * listed.  Additive to ABI version 5; a host detects them by " converge" in rm_build_info().
 *
 * Let rows = frame_height - frame_height % 32 and ns = lens->n_samples.  The per-pixel state is
 * three buffers in the plain layout: sum, [frame_height][frame_width][3] doubles as in the
 * progressive frames; stats, [frame_height][frame_width][2] doubles (Y, Q): the sums of y and of
 * y*y over the pixel's samples, y = (r + g) + b per sample; count, [frame_height][frame_width]
 * uint32_t: the pixel's number of samples n.  With fresh != 0 every n counts as 0 and none of the
 * three buffers is read.
 *
 *   Select.  Complete before any pixel is sampled.  Let nd = (double)n, m2 = Q - (Y*Y)/nd.
 *            capped(p): n + ns > max_samples.  unsettled(p): tolerance < 0, or
 *            n < max(min_samples, 2), or !(m2 <= (tolerance*tolerance) * (nd * (nd - 1.))) -- every
 *            operation rounded once, no fused multiply-add, so a NaN leaves the pixel unsettled.
 *            m2 / (nd (nd - 1)) is the squared standard error of the mean of y.
 *            noisy(p) = !capped(p) && unsettled(p).  A pixel is listed iff it is not capped and it
 *            or one of its up-to-four neighbours in [0, frame_width) x [0, rows) is noisy: the
 *            neighbourhood of the adaptive anti-aliasing.  The widening keeps a silhouette's
 *            neighbours sampling.  A pixel whose first samples all missed a thin feature is the
 *            estimate's known weak spot; min_samples is the guard against it.
 *            After the call the first uint32_t of the workspace holds the number of listed pixels
 *            and their indices y * frame_width + x follow, in no particular order.  mask, where
 *            given, gets 1 or 0 for every pixel of [0, rows).
 *   Sample.  A listed pixel with count n casts rows n .. n + ns - 1 of device_table, a prefix of
 *            rm_lens_sequence table_rows rows long, table_rows >= max_samples.  Where
 *            device_offsets is given the pixel also takes the same rows of that prefix of
 *            rm_light_sequence ([table_rows][n_lights][3]) and n_lights must be the resident
 *            scene's; NULL: every light is the scene's point.  Rays and radiance are steps 1-5 of
 *            the thin-lens camera, word for word, with the area lights' rule for the lights.
 *   Fold.    S, Y and Q start as the first sample's values (r, g, b; y; y*y) when n == 0, else
 *            from the buffers; the remaining samples are added in table order by plain additions;
 *            count = n + ns.  The mean is S / (double)(n + ns) and the bytes follow the progressive
 *            frames' rule; both are stored where those buffers are given.  A pixel that is not
 *            listed keeps every byte of every buffer.  Rows from `rows` on are neither read nor
 *            written.
 *
 * So the fold is a left fold in table order: a pixel with count c holds, byte for byte, the sum and
 * the mean rm_accumulate_lens_device (with offsets: rm_accumulate_soft_device) leaves after c
 * samples of the sequence, however the passes were sliced.  And with tolerance < 0 a run of passes
 * is byte for byte the plain run in sum, mean and bytes, every count the plain run's total.
 *
 * rm_accumulate_converging_device is asynchronous on hip_stream, neither reads nor writes render
 * state and keeps all of its state in the caller's buffers (a memset of the workspace's first word,
 * the select launch, the shade launch).  The workspace has rm_converge_workspace bytes,
 * rm_refine_workspace's size.  Checked before anything is launched, the offender named in
 * rm_last_error, no buffer touched: everything rm_accumulate_soft_device checks of params, lens and
 * the table (n_lights only where device_offsets is given); tolerance not NaN; ns <= max_samples <=
 * min(table_rows, RM_PROGRESSIVE_MAX_SAMPLES); converge, buffers, sum, stats, count and workspace
 * not NULL; mean != sum.  rows == 0 is RM_OK and does nothing.  The tables' contents and a count
 * buffer that this call or zeros filled are preconditions; a count from elsewhere gives unspecified
 * pixels, never a fault.
 *
 * rm_render_converging is the viewer's tick.  The context owns state of its own for it -- the six
 * buffers, the resident prefix of both sequences (appended to as the frame grows, never staged
 * again whole), the pass total N (a bound on every pixel's count: a pass that listed something sets
 * N = max(N, min(N + ns, max_samples)), whatever ns and max_samples were tick by tick), the passes and samples so
 * far, and the key of rm_render_progressive_soft: radii == NULL is "no radii" (point lights,
 * n_lights ignored) -- and shares none of it with rm_render_progressive: neither call disturbs the
 * other's frame.  The fields of rm_converge and n_samples are not part of the key: a viewer may
 * tighten the tolerance and continue.  restart != 0, another key or no successful call before
 * begin the frame again (fresh, N = 0).  The call runs one pass on the context's stream, copies the
 * rows [0, rows) of the mean and the bytes where asked, fills *report and blocks.  If the previous
 * tick of the same frame listed 0 pixels with the same rm_converge and n_samples, nothing is
 * launched, the frame stands and report->listed is 0: ticking a finished picture is not an error.
 * Checks: rm_render_progressive_soft's (radii only where given), tolerance not NaN, ns <=
 * max_samples <= RM_PROGRESSIVE_MAX_SAMPLES; a refused call changes nothing of the state.
 * rows == 0 is RM_OK with a report of zeros.  timing->kernel_ms covers the three steps.
 */
typedef struct rm_converge {
    double   tolerance;    /* standard error of y = (r + g) + b a pixel may keep; < 0: no pixel ever settles; NaN refused */
    uint32_t min_samples;  /* a pixel with fewer samples is never settled */
    uint32_t max_samples;  /* a pixel is never sampled beyond this many; n_samples..RM_PROGRESSIVE_MAX_SAMPLES */
} rm_converge;             /* 16 bytes */

typedef struct rm_converge_frame {   /* device memory, the plain layout */
    void *sum;         /* [frame_height][frame_width][3] doubles */
    void *stats;       /* [frame_height][frame_width][2] doubles */
    void *count;       /* [frame_height][frame_width] uint32_t */
    void *workspace;   /* rm_converge_workspace bytes */
    void *mean;        /* optional: the sum's shape */
    void *rgb8;        /* optional: [frame_height][frame_width][3] bytes */
    void *mask;        /* optional: [frame_height][frame_width] bytes */
} rm_converge_frame;     /* 56 bytes */

typedef struct rm_converge_report {
    uint64_t samples_cast;   /* over the frame's life: the sum of listed * n_samples over its passes */
    uint32_t listed;         /* pixels this call listed and sampled (0: the picture is finished) */
    uint32_t passes;         /* passes the frame has run */
    uint32_t max_count;      /* N: no pixel's count exceeds it */
    uint32_t _pad;
} rm_converge_report;      /* 24 bytes */

/* bytes of device memory the list needs for `params`: rm_refine_workspace's */
rm_status rm_converge_workspace(const rm_params *params, size_t *bytes);
rm_status rm_accumulate_converging_device(rm_ctx *ctx, const rm_params *params, const rm_lens *lens, const rm_converge *converge,
                                          const void *device_table, uint32_t table_rows, const void *device_offsets /* optional */,
                                          uint32_t n_lights, int fresh, const rm_converge_frame *buffers, void *hip_stream);
rm_status rm_render_converging(rm_ctx *ctx, const rm_params *params, const rm_lens *lens, const rm_converge *converge,
                               const double *radii /* NULL: point lights */, uint32_t n_lights, int restart,
                               double *host_rgb /* optional */, uint8_t *host_rgb8 /* optional */,
                               rm_converge_report *report /* optional */, rm_timing *timing /* optional */);

/* ---- converging frames with moving spheres: motion blur, noisy pixels only ---------------------
 * The converging frames sample the lens and the lights; the moving spheres sample time.  These
 * calls do both: a moving sphere leaves a band of pixels that settle slowly, the rest of the
 * picture settles after min_samples, and only the band goes on being sampled.  Additive to ABI
 * version 5; a host detects them by " converge-motion" in rm_build_info().
 *
 * A pass is rm_accumulate_converging_device's word for word -- select, the rows a listed pixel
 * casts, fold, mean, bytes, list and mask -- with one rule added, the moving spheres':
 *   - a listed pixel with count n casts rows n .. n + ns - 1 of the three tables;
 *   - for row r the sphere that is shape k of the scene stands at C'.c = C.c + shape_offsets[r][k].c
 *     per component, C the resident scene's: one addition, rounded once;
 *   - C' takes C's place in the closest-hit test, both shadow tests and the normal, at every
 *     bounce;
 *   - the shape offset table is [table_rows][n_shapes][3] doubles in the order of the scene's shape
 *     list, a prefix of rm_motion_sequence in the tick; the device's spheres are found in it
 *     through the queries' pid map.  Rows of shapes that are not spheres are never read.
 * The light offset table is [table_rows][n_lights][3] and required where the scene has lights (a
 * caller with point lights passes zeros), as in rm_accumulate_motion_device.
 *
 * Two consequences:
 *   - with every shape offset +0. or -0. a pass is byte for byte rm_accumulate_converging_device's
 *     for the same light offsets -- sum, stats, count, mean, bytes, mask, and the list as a set --
 *     for centre coordinates that are not -0. (-0. + +0. is +0.);
 *   - the fold is a left fold in table order: a pixel with count c holds byte for byte the sum and
 *     the mean rm_accumulate_motion_device leaves after c rows of the same three tables, however
 *     the passes were sliced.  With tolerance < 0 a run of passes is the plain motion run byte for
 *     byte in sum, mean and bytes.
 *
 * Cost: as the moving spheres', the kernel tests every primitive against every ray (the flat walk),
 * whatever hierarchies the scene image holds.
 *
 * rm_accumulate_converging_motion_device is asynchronous on hip_stream, neither reads nor writes
 * render state and keeps all of its state in the caller's buffers.  Its checks are
 * rm_accumulate_converging_device's and rm_accumulate_motion_device's together: n_lights must be
 * the resident scene's and device_light_offsets not NULL when it has lights; n_shapes must be the
 * resident scene's shape count and device_shape_offsets not NULL when it holds a sphere.  A refused
 * call names the offender in rm_last_error and touches no buffer.  The tables' contents are a
 * precondition: a non-finite offset gives unspecified pixels, never a fault.
 *
 * rm_render_converging_motion is the viewer's tick: rm_render_converging on the same context-owned
 * state -- the two ticks share one frame -- with a third resident prefix, the shape offsets
 * (rm_motion_sequence of velocities and shutter, appended to as the frame grows), and the key
 * extended by n_shapes, the bytes of velocities and of shutter.  So the frame begins again when a
 * velocity or the shutter changes, when a caller switches between the two ticks (velocities of zero
 * are velocities, not the plain call), and on everything that begins it again in
 * rm_render_converging; rm_converge and n_samples stay outside the key.  radii == NULL is "no
 * radii" and stages light offsets of zero for every light of the scene.  Checked before anything
 * else happens: rm_render_converging's checks, n_shapes the resident scene's, velocities and
 * shutter as rm_motion_sequence demands, and a velocity that is not zero for a shape that is not a
 * sphere -- RM_ERR_INVALID_ARG, the shape named in rm_last_error; a refused call changes nothing of
 * the state.  A finished picture launches nothing.  The report, rows == 0 and timing are
 * rm_render_converging's.
 */
rm_status rm_accumulate_converging_motion_device(rm_ctx *ctx, const rm_params *params, const rm_lens *lens,
                                                 const rm_converge *converge, const void *device_table, uint32_t table_rows,
                                                 const void *device_light_offsets, uint32_t n_lights,
                                                 const void *device_shape_offsets, uint32_t n_shapes, int fresh,
                                                 const rm_converge_frame *buffers, void *hip_stream);
rm_status rm_render_converging_motion(rm_ctx *ctx, const rm_params *params, const rm_lens *lens, const rm_converge *converge,
                                      const double *radii /* NULL: point lights */, uint32_t n_lights,
                                      const rm_vec3 *velocities, uint32_t n_shapes, double shutter, int restart,
                                      double *host_rgb /* optional */, uint8_t *host_rgb8 /* optional */,
                                      rm_converge_report *report /* optional */, rm_timing *timing /* optional */);

/* ---- converging frames with moving shapes: every shape blurs, noisy pixels only ----------------
 * The moving shapes (above) blur polygons and meshes in progressive frames, which sample every
 * pixel in every pass; the converging frames with moving spheres sample the noisy pixels alone but
 * move spheres only.  These calls do both: a moving floor quad or mesh leaves its band of slow
 * pixels, and only the band goes on being sampled.  Additive to ABI version 5; a host detects them
 * by " converge-moving" in rm_build_info().
 *
 * A pass is rm_accumulate_converging_motion_device's word for word -- select, the rows a listed
 * pixel casts, the light offsets, fold, mean, bytes, list and mask -- with the moving shapes' one
 * rule in place of the moving spheres':
 *   - the lane that casts sample s of a listed pixel with count n holds table row r = n + s;
 *   - for that lane shape k of the scene stands at its record plus shape_offsets[r][k], one
 *     addition a component, rounded once: a sphere's centre as in the moving spheres; a polygon's
 *     plane point and every vertex, the pool vertices of a polygon with more than four included;
 *     an Obj's every triangle, centre and vertices;
 *   - normals and materials stay as stored;
 *   - the moved record is used in the closest-hit walk, in both shadow walks and for the children;
 *   - the shape offset table is [table_rows][n_shapes][3] doubles in the order of the scene's shape
 *     list, a prefix of rm_motion_sequence in the tick.  Rows of every shape are read, so the whole
 *     table is a precondition whenever the scene holds any shape; it may be NULL only for a scene
 *     with no shape.
 *
 * Three consequences:
 *   - zero offsets: with every shape offset +0. or -0. a pass writes
 *     rm_accumulate_converging_motion_device's bytes -- sum, stats, count, mean, bytes, mask, and
 *     the list as a set -- for coordinates that are not -0.; with rows of zero for everything but
 *     the spheres it writes that call's bytes for those sphere rows;
 *   - own count: the fold stays a left fold in table order, so a pixel with count c holds byte for
 *     byte the sum, the mean and the display bytes rm_accumulate_moving_device leaves after c rows
 *     of the same three tables, however the passes were sliced;
 *   - negative tolerance: with tolerance < 0 a run of passes is the plain moving-shapes run byte
 *     for byte in sum, mean and bytes.
 *
 * Cost: the flat walk of the moving spheres, which a mesh pays in full, and the additions of the
 * rule at every polygon and triangle test.
 *
 * rm_accumulate_converging_moving_device is asynchronous on hip_stream, neither reads nor writes
 * render state and keeps all of its state in the caller's buffers.  Its argument list and checks
 * are rm_accumulate_converging_motion_device's, and as rm_accumulate_moving_device it refuses a
 * NULL device_shape_offsets whenever n_shapes > 0.  A refused call names the offender in
 * rm_last_error and touches no buffer.  The tables' contents are a precondition: a non-finite
 * offset gives unspecified pixels, never a fault.
 *
 * rm_render_converging_moving is rm_render_converging_motion's tick, argument for argument, on the
 * same context-owned state, in which a velocity on any shape is obeyed.  Its frames are its own:
 * a switch between this call and rm_render_converging_motion with equal velocities, or
 * rm_render_converging, begins the frame again.  It keeps a shape table whenever the scene holds a
 * shape (rm_render_converging_motion keeps none for a scene without spheres).  Checks:
 * rm_render_converging_motion's without the refusal of a velocity on a shape that is not a sphere;
 * the older calls' refusals stay as they are.
 */
rm_status rm_accumulate_converging_moving_device(rm_ctx *ctx, const rm_params *params, const rm_lens *lens,
                                                 const rm_converge *converge, const void *device_table, uint32_t table_rows,
                                                 const void *device_light_offsets, uint32_t n_lights,
                                                 const void *device_shape_offsets, uint32_t n_shapes, int fresh,
                                                 const rm_converge_frame *buffers, void *hip_stream);
rm_status rm_render_converging_moving(rm_ctx *ctx, const rm_params *params, const rm_lens *lens, const rm_converge *converge,
                                      const double *radii /* NULL: point lights */, uint32_t n_lights,
                                      const rm_vec3 *velocities, uint32_t n_shapes, double shutter, int restart,
                                      double *host_rgb /* optional */, uint8_t *host_rgb8 /* optional */,
                                      rm_converge_report *report /* optional */, rm_timing *timing /* optional */);

/* ---- moving camera: shutter blur of the view, in progressive and in converging frames ----------
 * The sampled frames give every sample a lens point, light positions and shape positions of its
 * own; these calls give it a camera of its own as well: the sixth and seventh members of the
 * family.  Additive to ABI version 5; a host detects them by " moving-camera" in rm_build_info().
 *
 * A camera table is [rows][12] doubles: (off.x, off.y, off.z, right.xyz, up.xyz, forward.xyz).  The
 * sample that is row r of the tables sees the camera at cam'.c = cam.c + off[r].c -- one addition,
 * rounded once, cam the context's position -- with the row's own basis: absolute, not an offset.
 * Steps 1-4 of the thin-lens camera take cam' and the row's basis in place of the context's, word
 * for word:
 *   D = (bx*right + by*up) + forward      always the oriented formula, whatever the context's
 *                                         oriented flag says;
 *   F.c = cam'.c + D.c*focus;   O.c = cam'.c + ((au*right.c) + (av*up.c));
 *   aperture == 0 keeps origin cam' and direction normalized(D).
 * Step 5 and everything after it is the member's underneath: the light rule, the shape rule, fold,
 * mean, bytes, stats and count.  A static scene keeps its hierarchy: no box, pid map or record
 * depends on where a ray starts.
 *
 * Consequences:
 *   - with every off +0. or -0. and every basis row equal to the basis of an ORIENTED context, a
 *     pass is byte for byte the underlying pass -- rm_accumulate_soft_device where no shape table is
 *     given, rm_accumulate_moving_device where one is, rm_accumulate_converging_device (with
 *     offsets) and rm_accumulate_converging_moving_device for the converging calls -- for camera
 *     coordinates that are not -0.;
 *   - under a context that is not oriented the pass still uses the oriented formula with the rows
 *     as given.  Against the fixed view's pass it may differ in the sign of a zero direction
 *     component (by is -0 on the row sy = height/2, and (bx*0 + by*1) + 0 is +0), so that
 *     comparison holds to the parity bound, not to bytes;
 *   - with every row holding the same off and the same basis B, a pass is byte for byte the
 *     underlying pass of a context whose camera was set to fl(cam + off) by rm_camera_update and to
 *     B by rm_camera_orient.
 *
 * rm_camera_motion: velocity in world units a unit of time; yaw, pitch and roll in radians a unit
 * of time, about the axes and with the signs of rm_camera_basis_turn.
 *
 * rm_camera_sequence is host arithmetic only.  Row s: t = shutter * phi_17(s), the same instant
 * rm_motion_sequence gives row s, so the camera and the shapes of a sample share it; off =
 * velocity.c * t; the basis is rm_camera_basis_turn(basis, yaw*t, pitch*t, roll*t).  Where all
 * three rates compare equal to 0 every row holds `basis` byte for byte, with no
 * re-orthonormalisation: a camera that only translates keeps the context's basis exactly.
 * Refusals are rm_motion_sequence's, a non-finite motion, and a basis rm_camera_basis_check
 * refuses; a refused call writes nothing.
 *
 * rm_accumulate_camera_device has rm_accumulate_moving_device's checks.  device_camera_rows must
 * not be NULL.  device_shape_offsets == NULL is allowed: no shape moves, n_shapes is not looked at
 * and the launch takes the static scene's kernels.  The tables' contents are a precondition: a
 * non-finite entry gives unspecified pixels (a ray that is not a number hits nothing), never a
 * fault; nothing read from a camera row forms an address.  rm_accumulate_converging_camera_device is rm_accumulate_converging_moving_device's
 * list plus device_camera_rows of table_rows rows, and allows a NULL shape table likewise.  The
 * lane that casts sample s of a listed pixel with count n holds row r = n + s of all four tables;
 * the select rule is unchanged.  So a pixel with count c holds byte for byte what
 * rm_accumulate_camera_device leaves after c rows, however the passes were sliced.
 *
 * The ticks are rm_render_progressive_moving's and rm_render_converging_moving's on the same
 * context-owned state, with `motion` (not NULL, six finite numbers) and a staged slice, or a fourth
 * resident prefix, of rm_camera_sequence, whose `basis` is what rm_camera_get reports.  The key is
 * extended by the bytes of *motion and the shutter, and the frames are their own: a switch to or
 * from any sibling tick begins the frame again.  velocities == NULL: no shape moves, no shape
 * table is kept and the static scene's kernels run; velocities given, zeros included, are the
 * moving shapes' rules.  Saturation, rows == 0, refusals that change neither N nor key, timing and
 * report are the siblings'.
 *
 * Cost: the member's underneath plus twelve per-lane loads and three additions a group of rays.
 * Not here: camera paths that are not linear within the shutter (the device calls take any table).
 */
typedef struct rm_camera_motion {
    rm_vec3 velocity;
    double  yaw, pitch, roll;
} rm_camera_motion;        /* 48 bytes */

rm_status rm_camera_sequence(uint32_t first, uint32_t count, const rm_camera_motion *motion, const rm_camera_basis *basis,
                             double shutter, double *rows);
rm_status rm_accumulate_camera_device(rm_ctx *ctx, const rm_params *params, const rm_lens *lens, const void *device_table,
                                      const void *device_camera_rows, const void *device_light_offsets, uint32_t n_lights,
                                      const void *device_shape_offsets /* NULL: no shape moves */, uint32_t n_shapes,
                                      uint32_t n_before, void *device_sum, void *device_mean /* optional */,
                                      void *device_rgb8 /* optional */, void *hip_stream);
rm_status rm_accumulate_converging_camera_device(rm_ctx *ctx, const rm_params *params, const rm_lens *lens,
                                                 const rm_converge *converge, const void *device_table, uint32_t table_rows,
                                                 const void *device_camera_rows, const void *device_light_offsets,
                                                 uint32_t n_lights, const void *device_shape_offsets /* NULL: no shape moves */,
                                                 uint32_t n_shapes, int fresh, const rm_converge_frame *buffers, void *hip_stream);
rm_status rm_render_progressive_camera(rm_ctx *ctx, const rm_params *params, const rm_lens *lens,
                                       const double *radii /* NULL: point lights */, uint32_t n_lights,
                                       const rm_vec3 *velocities /* NULL: no shape moves */, uint32_t n_shapes, double shutter,
                                       const rm_camera_motion *motion, int restart,
                                       double *host_rgb /* optional */, uint8_t *host_rgb8 /* optional */,
                                       uint32_t *n_total /* optional */, rm_timing *timing /* optional */);
rm_status rm_render_converging_camera(rm_ctx *ctx, const rm_params *params, const rm_lens *lens, const rm_converge *converge,
                                      const double *radii /* NULL: point lights */, uint32_t n_lights,
                                      const rm_vec3 *velocities /* NULL: no shape moves */, uint32_t n_shapes, double shutter,
                                      const rm_camera_motion *motion, int restart,
                                      double *host_rgb /* optional */, uint8_t *host_rgb8 /* optional */,
                                      rm_converge_report *report /* optional */, rm_timing *timing /* optional */);

/* ---- swept hierarchies: motion blur that keeps the scene's hierarchies ----------------------------
 * The moving shapes' passes walk flat: a hierarchy's boxes hold for the uploaded positions only.
 * A swept hierarchy is the resident scene image with the boxes of its sphere and triangle
 * hierarchies refitted, so that each bounds its primitives at every position their shapes can take
 * within given per-shape offset extents.  The topology -- child refs, leaf order, pid map, list-order
 * keys -- is the image's.  The passes below walk it with the moving shapes' rule applied inside the
 * leaves; the hierarchy only decides which primitives are tested, so a swept pass leaves byte for
 * byte what its flat sibling leaves.  Additive to ABI version 5; a host detects them by
 * " swept-hierarchy" in rm_build_info().
 *
 * Extents: lo and hi, [n_shapes][3] doubles each in the order of the scene's shape list, promise
 *   lo[k].c <= shape_offsets[r][k].c <= hi[k].c    for every row r any pass with this handle reads.
 * They must be finite with lo <= hi; anything else is refused and the shape named.  The extents of a
 * polygon are checked and not otherwise used: polygons have no hierarchy and are walked flat.
 * rm_swept_extents gives the per-shape componentwise minimum and maximum of a host table of `rows`
 * rows (rows >= 1).  rm_swept_motion_extents gives the extents of rm_motion_sequence's rows, all of
 * them: row s holds fl(v.c * t) with 0 <= t <= shutter, so lo.c = min(0, fl(v.c * shutter)) and
 * hi.c = max(0, fl(v.c * shutter)).  Both are host arithmetic only.
 *
 * Contract: a table row outside the extents a handle was built with gives unspecified pixels -- a
 * box may miss its primitive, and the shape be missed for that sample.  It is never a fault: nothing
 * read from a row or a box forms an address.
 *
 * rm_swept_build refits the resident image and uploads the result (it waits for the copy).  n_shapes
 * must be the resident scene's count.  For a scene whose image holds no hierarchy it succeeds, and
 * the passes walk flat.  The handle belongs to the context and to the scene as it stands: after an
 * upload that changes the resident image it is stale, and only rm_swept_free takes it.
 * rm_swept_free waits for the device, so no pass is still walking the handle's boxes when they go;
 * NULL is allowed.  rm_destroy releases the handles nobody freed.
 *
 * rm_accumulate_swept_device has rm_accumulate_moving_device's argument list and checks, and
 * rm_accumulate_converging_swept_device rm_accumulate_converging_moving_device's, plus the handle
 * behind n_shapes.  Both refuse a NULL handle, one that is not this context's (or was freed), and one built
 * before the scene last changed; a refused call names the offender in rm_last_error and touches no buffer.  Both are
 * asynchronous on the caller's stream and keep no state of their own, as their siblings.
 *
 * The ticks rm_render_progressive_moving and rm_render_converging_moving keep their signatures,
 * frames, keys and bytes.  Where the resident image holds a hierarchy they build a swept hierarchy
 * from rm_swept_motion_extents of their velocities and shutter and launch the swept kernels; they
 * build it again when the scene, a velocity or the shutter changes -- what begins the frame again
 * anyway.  RM_SWEPT_BVH=0 in the environment of rm_init makes them walk flat as before.
 *
 * The moving spheres' ticks and the moving camera's walk one too: "swept hierarchies under a moving
 * camera", below.  Staying flat: the moving spheres' DEVICE calls (rm_accumulate_motion_device,
 * rm_accumulate_converging_motion_device) -- a caller's table may hold non-zero rows they ignore,
 * which no extents could be read from; a caller who wants a hierarchy there has
 * rm_accumulate_swept_device, with rows of zero for everything but the spheres.  Not here either:
 * the bundle cull and occluder masks under motion, rotation.
 */
typedef struct rm_swept rm_swept;   /* a swept hierarchy of the resident scene (opaque) */

rm_status rm_swept_extents(const double *table, uint32_t rows, uint32_t n_shapes, double *lo, double *hi);
rm_status rm_swept_motion_extents(const rm_vec3 *velocities, uint32_t n_shapes, double shutter, double *lo, double *hi);
rm_status rm_swept_build(rm_ctx *ctx, const double *lo, const double *hi, uint32_t n_shapes, rm_swept **out);
void      rm_swept_free(rm_ctx *ctx, rm_swept *swept);
rm_status rm_accumulate_swept_device(rm_ctx *ctx, const rm_params *params, const rm_lens *lens, const void *device_table,
                                     const void *device_light_offsets, uint32_t n_lights, const void *device_shape_offsets,
                                     uint32_t n_shapes, const rm_swept *swept, uint32_t n_before, void *device_sum,
                                     void *device_mean /* optional */, void *device_rgb8 /* optional */, void *hip_stream);
rm_status rm_accumulate_converging_swept_device(rm_ctx *ctx, const rm_params *params, const rm_lens *lens,
                                                const rm_converge *converge, const void *device_table, uint32_t table_rows,
                                                const void *device_light_offsets, uint32_t n_lights,
                                                const void *device_shape_offsets, uint32_t n_shapes, const rm_swept *swept,
                                                int fresh, const rm_converge_frame *buffers, void *hip_stream);

/* ---- swept hierarchies under a moving camera -----------------------------------------------------
 * A shot in which the camera pans and something in the scene moves is the ordinary motion-blur
 * shot.  These calls are the moving camera's with a shape table, through a swept hierarchy: camera
 * rule, moved lights and the moving shapes' rule applied inside the leaves.  Additive to ABI
 * version 5; a host detects them by " swept-camera" in rm_build_info().
 *
 * Handles come from rm_swept_build, and the extents from rm_swept_extents or
 * rm_swept_motion_extents, as they are: the boxes are in world space and bound primitives, not
 * rays, so they hold wherever a ray starts and whichever way it looks.  No extents call takes a
 * camera table.
 *
 * rm_accumulate_camera_swept_device has rm_accumulate_camera_device's argument list and checks, and
 * rm_accumulate_converging_camera_swept_device rm_accumulate_converging_camera_device's, plus the
 * handle behind n_shapes and its three refusals (NULL, not this context's or freed, built before the
 * scene last changed).  A NULL device_shape_offsets is refused here: without a shape table nothing
 * moves, and the flat calls keep the hierarchy already.  A refused call names the offender in
 * rm_last_error and touches no buffer.  Both are asynchronous on the caller's stream and keep no
 * state of their own.
 *
 * Contract: the swept calls'.  With every shape row inside the handle's extents a pass leaves byte
 * for byte what the flat camera call leaves given the same tables -- sum, mean and display bytes;
 * for the converging call stats, counts, list and workspace as well.  A shape row outside the
 * extents gives unspecified pixels, never a fault: nothing read from an offset row, a box or a
 * camera row forms an address.  For an image without a hierarchy the flat kernels run.
 *
 * The ticks.  Every tick that moves a shape walks a swept hierarchy where the resident image holds
 * one: rm_render_progressive_moving and rm_render_converging_moving as before,
 * rm_render_progressive_camera and rm_render_converging_camera given velocities, and the moving
 * spheres' rm_render_progressive_motion and rm_render_converging_motion in a scene with spheres.
 * The last two launch the moving shapes' swept kernels: they refuse a velocity on anything but a
 * sphere, so their table's other rows are zeros, and such a pass writes the moving spheres' bytes
 * ("moving shapes", zero offsets).  Signatures, frames, keys and bytes of all six stay what they
 * were.  They share one hierarchy, kept until the scene, a velocity or the shutter changes: a
 * camera tick behind a moving shapes' tick with the same velocities and shutter builds nothing.  A
 * call about to be refused builds nothing.  RM_SWEPT_BVH=0 returns all six to the flat walk.
 *
 * rm_swept_tick_info says what the ticks did; it reads host state only and launches nothing.
 * walked_swept: 1 where the launch of the last tick of the sampled-frame family (any
 * rm_render_progressive* or rm_render_converging* call) walked a swept hierarchy; every such tick
 * clears it first, so a refused, saturated or finished tick leaves 0.  builds: the hierarchies the
 * ticks have built over the context's life (rm_swept_build's handles are not counted).
 */
typedef struct rm_swept_tick_report {
    uint32_t walked_swept;
    uint32_t builds;
} rm_swept_tick_report;    /* 8 bytes */

rm_status rm_accumulate_camera_swept_device(rm_ctx *ctx, const rm_params *params, const rm_lens *lens, const void *device_table,
                                            const void *device_camera_rows, const void *device_light_offsets, uint32_t n_lights,
                                            const void *device_shape_offsets, uint32_t n_shapes, const rm_swept *swept,
                                            uint32_t n_before, void *device_sum, void *device_mean /* optional */,
                                            void *device_rgb8 /* optional */, void *hip_stream);
rm_status rm_accumulate_converging_camera_swept_device(rm_ctx *ctx, const rm_params *params, const rm_lens *lens,
                                                       const rm_converge *converge, const void *device_table, uint32_t table_rows,
                                                       const void *device_camera_rows, const void *device_light_offsets,
                                                       uint32_t n_lights, const void *device_shape_offsets, uint32_t n_shapes,
                                                       const rm_swept *swept, int fresh, const rm_converge_frame *buffers,
                                                       void *hip_stream);
rm_status rm_swept_tick_info(rm_ctx *ctx, rm_swept_tick_report *out);

/* ---- variance-guided filter: an edge-avoiding filter for converging frames ------------------------
 * A converging frame is grainy for most of the ticks it takes to settle.  These calls are the
 * reconstruction filter for it: the spatial filter of SVGF, an edge-avoiding a-trous wavelet filter
 * steered by the per-pixel variance the converging frames keep anyway (sum, stats, count) and, where
 * the caller has them, by the hits under the pixels (rm_primary_hits_device).  A settled pixel has a
 * tiny variance and passes almost untouched, a noisy one borrows from neighbours on the same surface,
 * nothing crosses a silhouette.  Additive to ABI version 5; a host detects them by " denoise" in
 * rm_build_info().
 *
 * The rule.  Every operation is IEEE binary64, rounded once, no fused multiply-add, and only
 * + - * / and comparisons occur, so a restatement in any language gives the same bytes.  Let
 * rows = frame_height - frame_height % 32 and W = frame_width (W % 32 == 0).  Inputs over rows
 * [0, rows), the plain layout: sum [H][W][3] and stats [H][W][2] (Y, Q) of doubles, count [H][W]
 * of uint32_t -- the converging frames' three -- and optionally hits [H][W] of rm_hit.
 *
 *   Start.  nd = (double)n.  C0 = S / nd per channel when n > 0, else 0.  With
 *           m2 = Q - (Y*Y)/nd, m2 < 0 replaced by 0: V0 = m2 / (nd * (nd - 1.)) when n >= 2, else
 *           V0 = fallback_variance.  V is the variance of the mean of y = (r + g) + b.
 *   Iteration i = 0 .. iterations - 1, step s = 1 << i, from C, V to C', V', for pixel p:
 *           y(q) = (C[q].r + C[q].g) + C[q].b.
 *           g: the 3x3 prefilter of V about p -- taps dy = -1..1 outer, dx = -1..1 inner, one pixel
 *           apart whatever s, those in [0, W) x [0, rows) only, weights k(dx)*k(dy) with
 *           k = {1/4, 1/2, 1/4}; g = (sum of weight*V[q]) / (sum of weights), both sums left folds
 *           from +0.
 *           den = (sigma_l*sigma_l)*g + epsilon.
 *           The taps run dy = -2..2 outer, dx = -2..2 inner, q = p + s*(dx, dy).  A tap is skipped
 *           when q is outside [0, W) x [0, rows), when count[q] == 0, or when the guide rejects it.
 *           Otherwise w = ((h(dx)*h(dy)) * wl) * wn * wz, multiplied left to right, with
 *           h = {1/16, 1/4, 3/8, 1/4, 1/16}; a = y(p) - y(q); wl = den / (den + a*a), or 1. when
 *           count[p] == 0.
 *           The guide, where hits is given (hit != 0 is a hit).  Both pixels missed: wn = wz = 1.
 *           Exactly one missed: skipped.  Both hit and `shape` differs: skipped (`element` is not
 *           compared: a mesh is one surface).  Otherwise, N, P, t being the hit's normal, point
 *           and t: d = (N_p.x*N_q.x + N_p.y*N_q.y) + N_p.z*N_q.z, the tap is skipped unless d > 0,
 *           and wn is d squared normal_squarings times (wn = wn*wn);
 *           e = (N_p.x*(P_q.x-P_p.x) + N_p.y*(P_q.y-P_p.y)) + N_p.z*(P_q.z-P_p.z),
 *           sz = sigma_z*(1. + t_p), dz = sz*sz, wz = dz / (dz + e*e).  Without hits
 *           wn = wz = 1. and nothing is rejected.
 *           Left folds from +0. in tap order: sw += w; sc[c] += w*C[q][c]; sv += (w*w)*V[q].
 *           If sw > 0: C'[p] = sc / sw, V'[p] = sv / (sw*sw); else C'[p] = C[p], V'[p] = V[p].
 *   End.    device_out gets C and device_variance, where given, V after `iterations` iterations
 *           (0: C0, V0), and device_rgb8, where given, the display bytes of C by the progressive
 *           frames' rule.  Rows from `rows` on are neither read nor written in any buffer.
 *
 * So with iterations == 0 the output is byte for byte the mean rm_accumulate_converging_device
 * wrote for every pixel with n > 0; a pixel with count == 0 is a hole that takes no part as a tap
 * and is filled from the neighbours the guide admits; and two regions with different shape ids never
 * mix -- a picture that is exactly 1. on one shape and 0. on the other comes back exactly.
 * Nothing read from count, hits or a pixel's value forms an address: NaN, infinity or a count from
 * elsewhere give unspecified pixels, never a fault.
 *
 * rm_denoise_device is asynchronous on hip_stream, neither reads nor writes render state and keeps
 * all of its state in the caller's buffers: one prepare launch and one launch an iteration.  The
 * workspace has rm_denoise_workspace bytes, a function of params alone (frame_width % 32 != 0:
 * RM_ERR_DIMENSIONS), and holds nothing a later call needs.  Checked before anything is launched,
 * the offender named in rm_last_error, no buffer touched: of params what
 * rm_accumulate_converging_device checks of its frame (flags, band, patch_size, an empty frame,
 * frame_width % 32, fewer than 2^31 pixels) -- the filter looks at neither the resident scene nor
 * max_depth or the background, and asks for none --; denoise not NULL and every field in the range
 * its line states, a NaN refused; sum, stats, count, workspace and out not NULL; out none of sum,
 * stats, count, hits.  rows == 0 is RM_OK and does nothing.
 *
 * rm_render_denoised is the viewer's tick: it filters the context's converging frame -- the
 * buffers of whichever rm_render_converging* tick ran last -- into buffers of its own, copies the
 * rows [0, rows) of the result and its bytes where asked, and blocks.  It changes nothing of the
 * converging state: the next converging tick continues the same frame, byte for byte as if the
 * filter had not run.  It is refused with RM_ERR_INVALID_ARG where no converging frame exists (no
 * tick has succeeded, or the last one failed half-way) or its frame_width x frame_height are not
 * params'.  With guides != 0 it first fills a hit buffer of the context's with
 * rm_primary_hits_device's launch on the context's stream (a scene must be resident, as for that
 * call).  THE GUIDE IS THE PINHOLE VIEW FROM THE CONTEXT'S CAMERA AS IT STANDS: under a wide
 * aperture, under a moving camera and on strongly moving shapes the picture's edges are not where
 * the guide's are, the filter blurs wrongly, and guides should be 0.  timing->kernel_ms covers the
 * guide's and the filter's launches.
 */
typedef struct rm_denoise {
    double   sigma_l;            /* luminance edge stop, in standard errors; finite, >= 0 */
    double   sigma_z;            /* plane-distance edge stop, relative to 1 + t; finite, > 0 */
    double   epsilon;            /* added to the luminance denominator; finite, > 0 */
    double   fallback_variance;  /* variance of y for a pixel with n < 2; finite, >= 0 */
    uint32_t iterations;         /* 0..5; iteration i has step 1 << i */
    uint32_t normal_squarings;   /* 0..8: the normal weight is dot^(2^k) */
} rm_denoise;                    /* 40 bytes */

rm_status rm_denoise_workspace(const rm_params *params, size_t *bytes);
rm_status rm_denoise_device(rm_ctx *ctx, const rm_params *params, const rm_denoise *denoise,
                            const void *device_sum, const void *device_stats, const void *device_count,
                            const void *device_hits /* optional */, void *device_workspace,
                            void *device_out /* [H][W][3] doubles */, void *device_variance /* optional [H][W] */,
                            void *device_rgb8 /* optional */, void *hip_stream);
rm_status rm_render_denoised(rm_ctx *ctx, const rm_params *params, const rm_denoise *denoise, int guides,
                             double *host_rgb /* optional */, uint8_t *host_rgb8 /* optional */, rm_timing *timing /* optional */);

/* ---- temporal reprojection: converging frames carried across camera moves --------------------------
 * A converging frame is keyed on the camera's position and basis, so a camera move begins it again
 * and throws away every sample the device held.  These calls are the other half of SVGF: the sums a
 * frame held for one view are carried to another view of the same scene.  Every pixel of the new
 * view finds the point under it in the previous view's picture, takes the samples around that
 * position that lie on the same surface, and begins with their mean and the smallest of their
 * counts.  Additive to ABI version 5; a host detects them by " reproject" in rm_build_info().
 *
 * The rule.  Every operation is IEEE binary64, rounded once, in the written order, no fused
 * multiply-add.  Let rows = frame_height - frame_height % 32 and W = frame_width (W % 32 == 0).
 * Buffers are rm_converge_frame's (sum [H][W][3], stats [H][W][2], count [H][W]) and
 * rm_primary_hits_device's ([H][W] rm_hit): prev_* are the previous view's frame and its hits,
 * cur_hits the hits of the view the new frame will be sampled from, previous_view the previous
 * camera as rm_camera_get reported it.  For pixel p = (x, y), y < rows:
 *
 *   a. cur_hits[p].hit == 0: the pixel carries nothing (sky costs nothing to sample again).
 *   b. With P, N, t the current hit's point, normal and t, and E, R, U, F the previous view's
 *      position, right, up and forward: v = P - E; zf = (v.x*F.x + v.y*F.y) + v.z*F.z, and xr, yu
 *      likewise with R and U.  The pixel carries nothing unless zf > 0.
 *   c. The sample position, the inverse of the sample-ray formula of the radiance section:
 *          sx = (((xr / zf) / ratio) / half_fov / 2. + 0.5) * width
 *          sy = (((yu / zf) / half_fov) / -2. + 0.5) * height
 *   d. The range check, in doubles, before any conversion to an integer: the pixel carries nothing
 *      unless sx > -1. && sx < W && sy > -1. && sy < rows (a NaN fails every comparison).  Then
 *      x0 = floor(sx), fx = sx - x0, y0 = floor(sy), fy = sy - y0.
 *   e. The four bilinear taps run j = 0..1 outer, i = 0..1 inner: q = (x0 + i, y0 + j),
 *      wb = (i ? fx : 1. - fx) * (j ? fy : 1. - fy).  A tap is skipped when wb > 0 is false; when q
 *      is outside [0, W) x [0, rows); when prev_count[q] == 0; when prev_hits[q].hit == 0; when
 *      prev_hits[q].shape != cur_hits[p].shape (`element` is not compared, as in the filter); when
 *      d = (N.x*Nq.x + N.y*Nq.y) + N.z*Nq.z is not > min_normal_dot; or when e*e <= dz is false,
 *      with e = (N.x*(Pq.x-P.x) + N.y*(Pq.y-P.y)) + N.z*(Pq.z-P.z), sz = sigma_z*(1. + t),
 *      dz = sz*sz.
 *   f. Left folds from +0. in tap order, nq = (double)prev_count[q]: sw += wb;
 *      sc[c] += wb * (prev_sum[q][c] / nq); s1 += wb * (prev_stats[q][0] / nq);
 *      s2 += wb * (prev_stats[q][1] / nq); nmin = min(nmin, prev_count[q]).
 *   g. If sw > 0: n' = min(nmin, max_history), nd = (double)n', out_sum[p][c] = (sc[c] / sw) * nd,
 *      out_stats[p][k] = (s_k / sw) * nd, out_count[p] = n', carried = 1.  Otherwise sum and stats
 *      are +0., the count is 0 and carried = 0.  out_carried_total, where given, is zeroed by the
 *      call on the stream and then receives the number of carried pixels, one atomic add a wave.
 *   Rows from `rows` on are neither read nor written in any buffer.
 *
 * So: only + - * /, floor, comparisons and integer-to-double conversions occur, and a restatement
 * in any language gives the same bytes.  A previous picture that is exactly n * 1. on one shape and
 * n * 0. on another comes back exactly n' * 1. and n' * 0.: sc and sw are the same fold, so
 * nothing crosses a silhouette.  A point that was hidden, outside the previous frustum or behind
 * the previous camera carries nothing.  The carried second moment minus the square of the carried
 * first is never negative beyond rounding, because both are convex combinations, so the standard
 * error the converging rule forms of them stays meaningful.  Data DOES form addresses here -- that
 * is the nature of a gather along motion, and unlike the filter -- but no address is formed before
 * the range check in doubles: NaN, infinity or a hit buffer from elsewhere give pixels without
 * history or unspecified values, never a fault.
 *
 * rm_reproject_device is asynchronous on hip_stream, reads no render state and keeps no state of
 * its own.  Checked before anything is launched, the offender named in rm_last_error, no buffer
 * touched: of params what rm_denoise_device checks; reproject and previous_view not NULL and every
 * field in the range its line states, a NaN refused; a finite position and a basis
 * rm_camera_basis_check accepts; the five inputs and out_sum, out_stats, out_count not NULL; no
 * out_* equal to any input.  rows == 0 is RM_OK and does nothing.
 *
 * History in the tick.  History is a state of the context, off after rm_init;
 * rm_converge_history(ctx, settings) turns it on (or changes its settings), NULL turns it off.
 * While it is off every tick is byte for byte what it was: no allocation, no launch.  While it is
 * on, rm_render_converging -- the static scene, with or without radii, and no other tick -- keeps a
 * hit buffer for the frame's view, filled with rm_primary_hits_device's launch on the context's
 * stream when a frame begins, or by the first tick that finds the continuing frame without one.
 * Where the tick finds a frame other than the kept one, it reprojects rather than begins again
 * when the identity differs ONLY in the camera's position, its basis and whether it is oriented,
 * restart was not asked, the kept frame has run at least one pass and has a hit buffer.  It then
 * fills a second hit buffer for the new view, runs rm_reproject_device's launch from the kept
 * buffers and the kept view into a second set of sum, stats and count (and writes the mean
 * out_sum / n' and its bytes for every pixel, which the pass overwrites where it samples), swaps the
 * two sets and the two hit buffers, sets N = min(N, max_history), begins passes, listed and
 * samples_cast of the report at 0 -- so a "finished" frame is never assumed -- and runs the pass
 * with fresh = 0: a pixel with carried count n' casts rows n' .. n' + n_samples - 1, as any pixel
 * with that count does.  Every other cause begins the frame again as before: the scene, params,
 * the lens, the radii, another tick of the family.  rm_render_converging_motion, _moving and
 * _camera keep beginning again: their history would need motion vectors, which are not built.  A
 * refused call changes nothing of the state; a failure half-way leaves no frame, as before.  The
 * doubled buffers exist only while history is on: rm_destroy releases them, and so does turning
 * history off.  timing->kernel_ms covers the hit launch, the reprojection and the pass.
 *
 * WHAT HISTORY COSTS.  "A pixel with c samples holds what the plain frame holds after c" holds for
 * frames that were never reprojected; A REPROJECTED FRAME TRADES THAT PROMISE FOR HISTORY: its sums
 * are interpolated, not folded.  The guide is the pinhole view: under a wide aperture the carried
 * history is blurred across what the guide calls one surface, as the filter's section warns.
 * View-dependent light (mirror, glass) is carried as if it were stuck to the surface; max_history
 * bounds how long that error lives and should stay well under max_samples.  The bindings' default
 * of 32 is a starting value, not a tuned one.
 *
 * rm_converge_history_info tells a reprojected tick from one that quietly began again.
 */
typedef struct rm_view { rm_vec3 position; rm_camera_basis basis; } rm_view;   /* 96 bytes: a camera as rm_camera_get reports it */
typedef struct rm_reproject {
    double   sigma_z;          /* plane-distance gate, relative to 1 + t; finite, > 0 */
    double   min_normal_dot;   /* a tap is admitted only when N_p.N_q > this; finite, in [-1, 1) */
    uint32_t max_history;      /* no carried count exceeds it; 1..RM_PROGRESSIVE_MAX_SAMPLES */
    uint32_t _pad;
} rm_reproject;                /* 24 bytes */
typedef struct rm_history_report {
    uint64_t reprojections;    /* frames the ticks have begun from history since rm_init */
    uint32_t last_reprojected; /* 1: the last rm_render_converging tick began its frame from history */
    uint32_t carried;          /* pixels that carried history at the last reprojection */
    uint32_t without;          /* pixels of [0, rows) that did not */
    uint32_t _pad;
} rm_history_report;           /* 24 bytes */

rm_status rm_reproject_device(rm_ctx *ctx, const rm_params *params, const rm_reproject *reproject,
                              const rm_view *previous_view,
                              const void *prev_sum, const void *prev_stats, const void *prev_count, const void *prev_hits,
                              const void *cur_hits,
                              void *out_sum, void *out_stats, void *out_count,
                              void *out_carried /* optional: [H][W] bytes, 1 where history was carried */,
                              void *out_carried_total /* optional: one uint32_t on the device */,
                              void *hip_stream);
rm_status rm_converge_history(rm_ctx *ctx, const rm_reproject *reproject /* NULL: off */);
rm_status rm_converge_history_info(rm_ctx *ctx, rm_history_report *report);

/* ---- diffuse bounce: one bounce of indirect light in sampled frames ----------------------------
 * Every sampled frame shades a hit with direct light plus the constant background.  These calls
 * give each sample of a progressive or a converging frame one more ray: where the sample's camera
 * ray first hits a surface that is not glass, a ray leaves that point in a cosine-distributed
 * direction, and what comes back along it, scaled by the surface's diffuse colour, is added to the
 * sample.  The mean converges to a picture in which surfaces light each other.  Static scene,
 * standing camera; lens and area lights as in the members underneath.  Additive to ABI version 5;
 * a host detects them by " bounce" in rm_build_info().
 *
 * A bounce table is [rows][2] doubles, points of [0,1)^2.  The rule, every operation rounded once
 * in this order, no contraction.  A sample bounces only when its camera ray (depth 1) has its first
 * hit on a surface with is_glass_like == false; P (the hit point), N (its normal) and mat are the
 * hit's as every sampled frame shades it, dir is the camera ray's direction.  (t0, t1) is the
 * sample's row of the table, pix = y * frame_width + x of the sample's pixel.
 *  1. shift:  h = pix as a 32-bit word; h ^= h>>16; h *= 0x7feb352d; h ^= h>>15; h *= 0x846ca68b;
 *     h ^= h>>16 (mod 2^32).  sx = (double)(h & 0xffff) / 65536., sy = (double)(h >> 16) / 65536.;
 *     x = t0 + sx, x = x - floor(x); y = t1 + sy, y = y - floor(y).  Nothing read from a buffer
 *     forms an address.
 *  2. disc:   a = 2.*x - 1., b = 2.*y - 1.; sA = sqrt(1. - a*a/2.), sB = sqrt(1. - b*b/2.);
 *     u = a*sB, v = b*sA; w = sqrt(fmax(1. - (u*u + v*v), 0.)) -- the disc of rm_lens_sequence.
 *     That map is not area preserving, so the sample carries the weight
 *     k = 1.2732395447351628 * (sA*sB - (a*a*b*b) / (4.*sA*sB)), its Jacobian times 4/pi.  sA and
 *     sB lie in [sqrt(1/2), 1]: nothing divides by zero, 0 <= k <= 4/pi, and the weighted samples
 *     are cosine-distributed (the mean of k is 1, of k*w 2/3).
 *  3. frame:  Nf = dot(dir, N) < 0. ? N : -N; sg = Nf.z < 0. ? -1. : 1.; q = -1. / (sg + Nf.z)
 *     (|sg + Nf.z| >= 1); c = Nf.x*Nf.y*q; T = (1. + sg*Nf.x*Nf.x*q, sg*c, -sg*Nf.x);
 *     B = (c, sg + Nf.y*Nf.y*q, -Nf.y); omega = normalized((T*u + B*v) + Nf*w);
 *     O' = P + Nf * 1e-3.
 *  4. light:  the sample's radiance is A + tint * S per channel, where A is what the member
 *     underneath returns for the sample (background + direct light of the hit), tint is
 *     mat.diffuse_color and S is cast_ray(O', omega, n_recursion = 2, max_depth) of the reference
 *     with every term scaled by wb = (strength * mat.diffusion) * k: the sum, in the order the
 *     kernels of every sampled frame walk a ray's tree, of weight * (background + direct light) at
 *     a hit, weight * background where a ray leaves the scene or lies beyond the cap, with the
 *     weight wb at the bounce ray and times reflection or (1 - reflection) at each child.  The
 *     sample's lights (moved by its row of the offset table) shade every hit of the bounce's tree.
 *     A bounce beyond the cap (max_depth == 1) returns the background: A + tint * (background * wb).
 * Glass first hits, misses and max_depth == 0 are the member underneath, unchanged.  With
 * strength == 0 nothing is cast and no operation on a value differs from the member underneath:
 * rm_accumulate_bounce_device writes rm_accumulate_soft_device's bytes,
 * rm_accumulate_converging_bounce_device writes rm_accumulate_converging_device's.  The tests hold
 * a frame to the reference's cast_ray within 1e-9 a channel of the mean; the largest deviations
 * seen are in DESIGN.md.
 *
 * rm_bounce_sequence fills rows first .. first + count - 1 of one fixed table, count * 2 doubles:
 * row s = (phi_19(s), phi_23(s)), phi_b as in rm_lens_sequence.  Host arithmetic only.
 * first + count > RM_PROGRESSIVE_MAX_SAMPLES and a NULL table with something to write are
 * RM_ERR_INVALID_ARG; count == 0 is RM_OK, nothing is written.  The device calls take any table.
 *
 * rm_accumulate_bounce_device is rm_accumulate_soft_device with the bounce table and the strength:
 * the same checks, and device_bounce must not be NULL and strength must be a finite number >= 0,
 * else RM_ERR_INVALID_ARG.  lens->n_samples rows of device_bounce are read (with strength == 0
 * none).  Their contents are a precondition: a non-finite entry gives unspecified pixels, never a
 * fault.  rm_accumulate_converging_bounce_device is rm_accumulate_converging_device with the same
 * two: table_rows rows of device_bounce are resident, and a pixel's sample takes the bounce row of
 * its table row.
 *
 * rm_render_progressive_bounce and rm_render_converging_bounce are the ticks: rm_render_progressive_soft
 * and rm_render_converging (radii NULL: point lights) on the same context-owned state, with the key
 * extended by the strength -- a strength of 0 is not "no bounce".  So a frame begins again when the
 * strength changes, when a caller switches between one of these and another tick in either
 * direction, and on everything that begins the tick underneath again -- a camera move included:
 * rm_converge_history does not reach these frames.  The progressive tick stages rows
 * [N, N + n_samples) of rm_bounce_sequence beside the others, the converging tick keeps a third
 * resident prefix of 2 columns.  Checked before anything else happens: what the tick underneath
 * checks, and the strength; a refused call changes nothing.  rm_render_denoised serves the
 * converging tick as it serves the others; its guide is still the pinhole view.
 */
rm_status rm_bounce_sequence(uint32_t first, uint32_t count, double *table);
rm_status rm_accumulate_bounce_device(rm_ctx *ctx, const rm_params *params, const rm_lens *lens, const void *device_table,
                                      const void *device_offsets, uint32_t n_lights, const void *device_bounce, double strength,
                                      uint32_t n_before, void *device_sum, void *device_mean /* optional */,
                                      void *device_rgb8 /* optional */, void *hip_stream);
rm_status rm_accumulate_converging_bounce_device(rm_ctx *ctx, const rm_params *params, const rm_lens *lens,
                                                 const rm_converge *converge, const void *device_table, uint32_t table_rows,
                                                 const void *device_offsets /* optional */, uint32_t n_lights,
                                                 const void *device_bounce, double strength, int fresh,
                                                 const rm_converge_frame *frame, void *hip_stream);
rm_status rm_render_progressive_bounce(rm_ctx *ctx, const rm_params *params, const rm_lens *lens, const double *radii /* optional */,
                                       uint32_t n_lights, double strength, int restart, double *host_rgb /* optional */,
                                       uint8_t *host_rgb8 /* optional */, uint32_t *n_total /* optional */,
                                       rm_timing *timing /* optional */);
rm_status rm_render_converging_bounce(rm_ctx *ctx, const rm_params *params, const rm_lens *lens, const rm_converge *converge,
                                      const double *radii /* optional */, uint32_t n_lights, double strength, int restart,
                                      double *host_rgb /* optional */, uint8_t *host_rgb8 /* optional */,
                                      rm_converge_report *report /* optional */, rm_timing *timing /* optional */);

/* Library / device introspection for harnesses. */
uint32_t    rm_abi_version(void);
const char *rm_build_info(void);
rm_status   rm_device_info(rm_ctx *ctx, char *name_buf, size_t buflen, int *n_cus, size_t *lds_bytes);
/* Name of the kernel a render of the uploaded scene with `params` launches, as a kernel trace
 * (rocprofv3) prints it: ties a measured launch to its profile. */
rm_status   rm_kernel_name(rm_ctx *ctx, const rm_params *params, char *buf, size_t buflen);

#ifdef __cplusplus
}
#endif
#endif /* RUSTY_MARCHER_AMD_H */
