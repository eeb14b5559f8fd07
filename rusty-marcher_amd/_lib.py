"""ctypes binding of include/rusty_marcher_amd.h (the C ABI) -- loads the in-tree
librusty_marcher_amd.so and fails loudly when it is missing.  No fallback."""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("RM_LIB_PATH") or os.path.join(_HERE, "lib", "librusty_marcher_amd.so")   # RM_LIB_PATH: dev knob for A/B builds

RM_OK = 0
RM_ERR_INVALID_ARG, RM_ERR_DIMENSIONS, RM_ERR_NO_DEVICE, RM_ERR_HIP = 1, 2, 3, 4
RM_ERR_NO_SCENE, RM_ERR_SCENE_LIMIT, RM_ERR_IO, RM_ERR_PARSE, RM_ERR_DEPTH = 5, 6, 7, 8, 9
RM_ERR_COMM, RM_ERR_TIMEOUT = 10, 11
RM_FLAG_FAST_FP, RM_FLAG_U8_COMPACT, RM_FLAG_F64_COMPACT = 2, 4, 8
RM_MAX_DEPTH = 32
RM_COMM_ID_BYTES, RM_MAX_FRAME_SLOTS = 128, 4
RM_PATCH_SIZE = 32
RM_SHAPE_SPHERE, RM_SHAPE_POLYGON, RM_SHAPE_MESH = 0, 1, 2
RM_LIGHTS_AS_RENDERED, RM_LIGHTS_CLIPPED = 0, 1

STATUS_NAMES = {0: "RM_OK", 1: "RM_ERR_INVALID_ARG", 2: "RM_ERR_DIMENSIONS", 3: "RM_ERR_NO_DEVICE",
                4: "RM_ERR_HIP", 5: "RM_ERR_NO_SCENE", 6: "RM_ERR_SCENE_LIMIT", 7: "RM_ERR_IO",
                8: "RM_ERR_PARSE", 9: "RM_ERR_DEPTH", 10: "RM_ERR_COMM", 11: "RM_ERR_TIMEOUT"}


class rm_vec3(C.Structure):
    _fields_ = [("x", C.c_double), ("y", C.c_double), ("z", C.c_double)]


class rm_reflectance(C.Structure):
    _fields_ = [("diffusion", C.c_double), ("diffuse_color", rm_vec3), ("specular", C.c_double),
                ("specular_exponent", C.c_double), ("is_glass_like", C.c_int32), ("_pad", C.c_int32),
                ("reflection", C.c_double), ("refractive_index", C.c_double)]


class rm_light(C.Structure):
    _fields_ = [("position", rm_vec3), ("color", rm_vec3), ("intensity", C.c_double)]


class rm_sphere(C.Structure):
    _fields_ = [("center", rm_vec3), ("radius_square", C.c_double), ("reflectance", rm_reflectance)]


class rm_polygon(C.Structure):
    _fields_ = [("first_vertex", C.c_uint32), ("n_vertices", C.c_uint32), ("plane_normal", rm_vec3),
                ("plane_point", rm_vec3), ("reflectance", rm_reflectance)]


class rm_triangle(C.Structure):
    _fields_ = [("vertices", rm_vec3 * 3), ("normal", rm_vec3), ("center", rm_vec3),
                ("reflectance", rm_reflectance)]


class rm_shape_ref(C.Structure):
    _fields_ = [("kind", C.c_uint32), ("first", C.c_uint32), ("count", C.c_uint32), ("_pad", C.c_uint32)]


class rm_scene_desc(C.Structure):
    _fields_ = [("shapes", C.POINTER(rm_shape_ref)), ("n_shapes", C.c_uint32),
                ("spheres", C.POINTER(rm_sphere)), ("n_spheres", C.c_uint32),
                ("polygons", C.POINTER(rm_polygon)), ("n_polygons", C.c_uint32),
                ("polygon_vertices", C.POINTER(rm_vec3)), ("n_polygon_vertices", C.c_uint32),
                ("triangles", C.POINTER(rm_triangle)), ("n_triangles", C.c_uint32),
                ("lights", C.POINTER(rm_light)), ("n_lights", C.c_uint32),
                ("camera", rm_vec3)]


class rm_params(C.Structure):
    _fields_ = [("fov", C.c_double), ("half_fov", C.c_double), ("height", C.c_double),
                ("width", C.c_double), ("ratio", C.c_double),
                ("frame_width", C.c_uint32), ("frame_height", C.c_uint32),
                ("max_depth", C.c_uint32), ("patch_size", C.c_uint32),
                ("background", rm_vec3),
                ("patch_row_begin", C.c_uint32), ("patch_row_end", C.c_uint32),
                ("flags", C.c_uint32), ("patch_row_stride", C.c_uint32)]


class rm_timing(C.Structure):
    _fields_ = [("kernel_ms", C.c_double), ("d2h_ms", C.c_double), ("total_ms", C.c_double)]


class rm_frame_times(C.Structure):
    _fields_ = [("kernel_ms", C.c_double), ("gather_ms", C.c_double), ("total_ms", C.c_double)]


class rm_hit(C.Structure):
    """One answer of find_closest_intersect (shapes.rs:110-143): the ray queries' record."""
    _fields_ = [("t", C.c_double), ("point", rm_vec3), ("normal", rm_vec3), ("shape", C.c_uint32),
                ("element", C.c_uint32), ("hit", C.c_int32), ("_pad", C.c_uint32)]


class rm_range(C.Structure):
    """The closed range [t_min, t_max] of the ray parameter a ranged query accepts hits in (16 bytes)."""
    _fields_ = [("t_min", C.c_double), ("t_max", C.c_double)]


class rm_shading(C.Structure):
    """Background and depth cap of a radiance query over a ray list (32 bytes)."""
    _fields_ = [("background", rm_vec3), ("max_depth", C.c_uint32), ("_pad", C.c_uint32)]


class rm_refine(C.Structure):
    """What an adaptive anti-aliasing call refines: n x n samples for every pixel whose contrast is > threshold (16 bytes)."""
    _fields_ = [("n", C.c_uint32), ("_pad", C.c_uint32), ("threshold", C.c_double)]


class rm_lens(C.Structure):
    """The thin lens of a depth-of-field frame: radius, distance of the plane in focus, rays a pixel (24 bytes)."""
    _fields_ = [("aperture", C.c_double), ("focus", C.c_double), ("n_samples", C.c_uint32), ("_pad", C.c_uint32)]


class rm_converge(C.Structure):
    """When a pixel of a converging frame is settled: standard error it may keep, fewest and most samples (16 bytes)."""
    _fields_ = [("tolerance", C.c_double), ("min_samples", C.c_uint32), ("max_samples", C.c_uint32)]


class rm_converge_frame(C.Structure):
    """The device buffers of a converging frame: sum, stats, count, workspace; optional mean, rgb8, mask (56 bytes)."""
    _fields_ = [("sum", C.c_void_p), ("stats", C.c_void_p), ("count", C.c_void_p), ("workspace", C.c_void_p),
                ("mean", C.c_void_p), ("rgb8", C.c_void_p), ("mask", C.c_void_p)]


class rm_converge_report(C.Structure):
    """What a tick of a converging frame reports (24 bytes)."""
    _fields_ = [("samples_cast", C.c_uint64), ("listed", C.c_uint32), ("passes", C.c_uint32), ("max_count", C.c_uint32),
                ("_pad", C.c_uint32)]


class rm_camera_basis(C.Structure):
    """The oriented camera's view direction: three world-space unit vectors (72 bytes)."""
    _fields_ = [("right", rm_vec3), ("up", rm_vec3), ("forward", rm_vec3)]


class rm_camera_motion(C.Structure):
    """How the camera moves while the shutter stands open: velocity, and yaw, pitch and roll rates in radians (48 bytes)."""
    _fields_ = [("velocity", rm_vec3), ("yaw", C.c_double), ("pitch", C.c_double), ("roll", C.c_double)]


class rm_swept_tick_report(C.Structure):
    """What the ticks that move a shape did: whether the last sampled-frame tick's launch walked a swept hierarchy, and how many
    hierarchies the ticks have built over the context's life (8 bytes)."""
    _fields_ = [("walked_swept", C.c_uint32), ("builds", C.c_uint32)]


class rm_denoise(C.Structure):
    """The variance-guided filter's control: luminance and plane-distance edge stops, the luminance denominator's epsilon, the
    variance of a pixel with fewer than two samples, iterations (0..5) and squarings of the normals' dot product (0..8) (40 bytes)."""
    _fields_ = [("sigma_l", C.c_double), ("sigma_z", C.c_double), ("epsilon", C.c_double), ("fallback_variance", C.c_double),
                ("iterations", C.c_uint32), ("normal_squarings", C.c_uint32)]


class rm_view(C.Structure):
    """A camera as rm_camera_get reports it: position and basis (96 bytes)."""
    _fields_ = [("position", rm_vec3), ("basis", rm_camera_basis)]


class rm_reproject(C.Structure):
    """The temporal reprojection's control: the plane-distance gate, the least dot product of the normals a tap is admitted with,
    and the most samples a pixel may carry (24 bytes)."""
    _fields_ = [("sigma_z", C.c_double), ("min_normal_dot", C.c_double), ("max_history", C.c_uint32), ("_pad", C.c_uint32)]


class rm_history_report(C.Structure):
    """What the converging tick did with its history: frames begun from history, whether the last tick was one, and the pixels
    that carried history at the last reprojection and those that did not (24 bytes)."""
    _fields_ = [("reprojections", C.c_uint64), ("last_reprojected", C.c_uint32), ("carried", C.c_uint32), ("without", C.c_uint32),
                ("_pad", C.c_uint32)]


_P = C.POINTER
_VP = C.c_void_p

# name -> (restype, argtypes); every symbol include/rusty_marcher_amd.h declares
SIGNATURES = {
    "rm_reflectance_default": (None, [_P(rm_reflectance)]),
    "rm_create_renderer": (None, [C.c_double, C.c_double, C.c_double, _P(rm_params)]),
    "rm_scene_new": (C.c_int, [_P(_VP)]),
    "rm_scene_free": (None, [_VP]),
    "rm_scene_create_default": (C.c_int, [_P(_VP)]),
    "rm_scene_add_sphere": (C.c_int, [_VP, rm_vec3, C.c_double, _P(rm_reflectance)]),
    "rm_scene_add_polygon": (C.c_int, [_VP, _P(rm_vec3), C.c_uint32, _P(rm_reflectance)]),
    "rm_scene_add_mesh": (C.c_int, [_VP, _P(C.c_double), C.c_uint32, rm_vec3]),
    "rm_scene_add_light": (C.c_int, [_VP, rm_vec3, rm_vec3, C.c_double]),
    "rm_scene_offset_shape": (C.c_int, [_VP, C.c_uint32, rm_vec3]),
    "rm_scene_set_camera": (C.c_int, [_VP, rm_vec3]),
    "rm_scene_offset_camera": (C.c_int, [_VP, rm_vec3]),
    "rm_scene_load_obj": (C.c_int, [_VP, C.c_char_p, rm_vec3, _P(C.c_uint32)]),
    "rm_scene_open_obj": (C.c_int, [C.c_char_p, _P(_VP)]),
    "rm_scene_get_desc": (C.c_int, [_VP, _P(rm_scene_desc)]),
    "rm_format_status": (C.c_int, [C.c_char_p, C.c_size_t, C.c_uint64, C.c_uint32, C.c_uint32]),
    "rm_init": (C.c_int, [C.c_int, _P(_VP)]),
    "rm_destroy": (None, [_VP]),
    "rm_last_error": (C.c_char_p, [_VP]),
    "rm_scene_upload": (C.c_int, [_VP, _P(rm_scene_desc)]),
    "rm_scene_uploads": (C.c_int, [_VP, _P(C.c_uint64), _P(C.c_uint64)]),
    "rm_camera_update": (C.c_int, [_VP, rm_vec3]),
    "rm_camera_orient": (C.c_int, [_VP, _P(rm_camera_basis)]),
    "rm_camera_look_at": (C.c_int, [_VP, rm_vec3, rm_vec3, rm_vec3]),
    "rm_camera_get": (C.c_int, [_VP, _P(rm_vec3), _P(rm_camera_basis), _P(C.c_int)]),
    "rm_camera_basis_look_at": (C.c_int, [rm_vec3, rm_vec3, rm_vec3, _P(rm_camera_basis)]),
    "rm_camera_basis_turn": (C.c_int, [_P(rm_camera_basis), C.c_double, C.c_double, C.c_double, _P(rm_camera_basis)]),
    "rm_camera_basis_check": (C.c_int, [_P(rm_camera_basis)]),
    "rm_render": (C.c_int, [_VP, _P(rm_params), _P(C.c_double), _P(rm_timing)]),
    "rm_render_rows": (C.c_int, [_VP, _P(rm_params), _P(_P(C.c_double)), _P(rm_timing)]),
    "rm_render_display": (C.c_int, [_VP, _P(rm_params), _P(C.c_uint8), _P(rm_timing)]),
    "rm_fetch_rows": (C.c_int, [_VP, _P(_P(C.c_double)), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32]),
    "rm_hostio_stats": (C.c_int, [_VP, _P(C.c_uint64), _P(C.c_uint64), _P(C.c_uint64), _P(C.c_int)]),
    "rm_render_device": (C.c_int, [_VP, _P(rm_params), _VP, _VP]),
    "rm_render_device_u8": (C.c_int, [_VP, _P(rm_params), _VP, _VP, _VP]),
    "rm_tile_stats": (C.c_int, [_VP, _VP, _P(C.c_uint32), _P(C.c_uint32)]),
    "rm_launch_stats": (C.c_int, [_VP, _P(C.c_uint32), _P(C.c_uint32)]),
    "rm_device_framebuffer": (C.c_int, [_VP, _P(_VP), _P(C.c_size_t)]),
    "rm_postprocess": (C.c_int, [_VP, _VP, C.c_uint32, C.c_uint32, C.c_int, _P(C.c_uint8), _P(C.c_double)]),
    "rm_buffer_alloc": (C.c_int, [_VP, C.c_size_t, _P(_VP)]),
    "rm_buffer_free": (None, [_VP, _VP]),
    "rm_buffer_read": (C.c_int, [_VP, _VP, _VP, C.c_size_t]),
    "rm_buffer_write": (C.c_int, [_VP, _VP, _VP, C.c_size_t]),
    "rm_host_alloc": (C.c_int, [_VP, C.c_size_t, _P(_VP)]),
    "rm_host_free": (None, [_VP, _VP]),
    "rm_frame_submit_to_host": (C.c_int, [_VP, _P(rm_params), _VP, _VP, _VP, _VP, C.c_uint32]),
    "rm_comm_unique_id": (C.c_int, [_VP]),
    "rm_comm_init": (C.c_int, [_VP, _VP, C.c_int, C.c_int]),
    "rm_comm_destroy": (None, [_VP]),
    "rm_comm_exchange": (C.c_int, [_VP, C.c_int]),
    "rm_exchange_layout": (C.c_int, [_P(rm_params), C.c_int, _P(C.c_uint32), _P(C.c_size_t)]),
    "rm_frame_submit": (C.c_int, [_VP, _P(rm_params), _VP, _VP, _VP, C.c_uint32]),
    "rm_frame_wait": (C.c_int, [_VP, C.c_uint32]),
    "rm_frame_wait_for": (C.c_int, [_VP, C.c_uint32, C.c_uint32]),
    "rm_frame_submit_f64": (C.c_int, [_VP, _P(rm_params), _VP, _VP, C.c_uint32]),
    "rm_frame_timing_enable": (C.c_int, [_VP, C.c_int]),
    "rm_frame_timing": (C.c_int, [_VP, C.c_uint32, _P(rm_frame_times)]),
    "rm_comm_info": (C.c_int, [_VP, _P(C.c_int), _P(C.c_int), _P(C.c_int)]),
    "rm_intersect_rays": (C.c_int, [_VP, _P(rm_vec3), _P(rm_vec3), C.c_uint32, _P(rm_hit)]),
    "rm_occluded_rays": (C.c_int, [_VP, _P(rm_vec3), _P(rm_vec3), C.c_uint32, _P(C.c_uint8)]),
    "rm_intersect_rays_device": (C.c_int, [_VP, _VP, _VP, C.c_uint32, _VP, _VP]),
    "rm_occluded_rays_device": (C.c_int, [_VP, _VP, _VP, C.c_uint32, _VP, _VP]),
    "rm_pick": (C.c_int, [_VP, _P(rm_params), C.c_uint32, C.c_uint32, _P(rm_hit)]),
    "rm_primary_hits_device": (C.c_int, [_VP, _P(rm_params), _VP, _VP]),
    "rm_intersect_rays_ranged": (C.c_int, [_VP, _P(rm_vec3), _P(rm_vec3), _P(rm_range), C.c_uint32, _P(rm_hit)]),
    "rm_occluded_rays_ranged": (C.c_int, [_VP, _P(rm_vec3), _P(rm_vec3), _P(rm_range), C.c_uint32, _P(C.c_uint8)]),
    "rm_intersect_rays_ranged_device": (C.c_int, [_VP, _VP, _VP, _VP, C.c_uint32, _VP, _VP]),
    "rm_occluded_rays_ranged_device": (C.c_int, [_VP, _VP, _VP, _VP, C.c_uint32, _VP, _VP]),
    "rm_visible_segments": (C.c_int, [_VP, _P(rm_vec3), _P(rm_vec3), C.c_uint32, C.c_double, _P(C.c_uint8)]),
    "rm_visible_segments_device": (C.c_int, [_VP, _VP, _VP, C.c_uint32, C.c_double, _VP, _VP]),
    "rm_lights_visible": (C.c_int, [_VP, _P(rm_vec3), _P(rm_vec3), C.c_uint32, C.c_uint32, C.c_uint32, _P(C.c_uint8)]),
    "rm_lights_visible_device": (C.c_int, [_VP, _VP, _VP, C.c_uint32, C.c_uint32, C.c_uint32, _VP, _VP]),
    "rm_radiance_rays": (C.c_int, [_VP, _P(rm_vec3), _P(rm_vec3), C.c_uint32, _P(rm_shading), _P(rm_vec3)]),
    "rm_radiance_rays_device": (C.c_int, [_VP, _VP, _VP, C.c_uint32, _P(rm_shading), _VP, _VP]),
    "rm_radiance_samples": (C.c_int, [_VP, _P(rm_params), _P(C.c_double), C.c_uint32, _P(rm_vec3)]),
    "rm_radiance_samples_device": (C.c_int, [_VP, _P(rm_params), _VP, C.c_uint32, _VP, _VP]),
    "rm_refine_workspace": (C.c_int, [_P(rm_params), _P(C.c_size_t)]),
    "rm_refine_device": (C.c_int, [_VP, _P(rm_params), _P(rm_refine), _VP, _VP, _VP, _VP]),
    "rm_render_antialiased": (C.c_int, [_VP, _P(rm_params), _P(rm_refine), _P(C.c_double), _P(C.c_uint32), _P(rm_timing)]),
    "rm_lens_table": (C.c_int, [C.c_uint32, _P(C.c_double)]),
    "rm_render_lens_device": (C.c_int, [_VP, _P(rm_params), _P(rm_lens), _VP, _VP, _VP]),
    "rm_render_lens": (C.c_int, [_VP, _P(rm_params), _P(rm_lens), _P(C.c_double), _P(C.c_double), _P(rm_timing)]),
    "rm_lens_sequence": (C.c_int, [C.c_uint32, C.c_uint32, _P(C.c_double)]),
    "rm_accumulate_lens_device": (C.c_int, [_VP, _P(rm_params), _P(rm_lens), _VP, C.c_uint32, _VP, _VP, _VP, _VP]),
    "rm_render_progressive": (C.c_int, [_VP, _P(rm_params), _P(rm_lens), C.c_int, _P(C.c_double), _P(C.c_uint8), _P(C.c_uint32), _P(rm_timing)]),
    "rm_light_sequence": (C.c_int, [C.c_uint32, C.c_uint32, _P(C.c_double), C.c_uint32, _P(C.c_double)]),
    "rm_accumulate_soft_device": (C.c_int, [_VP, _P(rm_params), _P(rm_lens), _VP, _VP, C.c_uint32, C.c_uint32, _VP, _VP, _VP, _VP]),
    "rm_render_progressive_soft": (C.c_int, [_VP, _P(rm_params), _P(rm_lens), _P(C.c_double), C.c_uint32, C.c_int, _P(C.c_double),
                                             _P(C.c_uint8), _P(C.c_uint32), _P(rm_timing)]),
    "rm_motion_sequence": (C.c_int, [C.c_uint32, C.c_uint32, _P(rm_vec3), C.c_uint32, C.c_double, _P(C.c_double)]),
    "rm_accumulate_motion_device": (C.c_int, [_VP, _P(rm_params), _P(rm_lens), _VP, _VP, C.c_uint32, _VP, C.c_uint32, C.c_uint32, _VP, _VP,
                                              _VP, _VP]),
    "rm_render_progressive_motion": (C.c_int, [_VP, _P(rm_params), _P(rm_lens), _P(C.c_double), C.c_uint32, _P(rm_vec3), C.c_uint32,
                                               C.c_double, C.c_int, _P(C.c_double), _P(C.c_uint8), _P(C.c_uint32), _P(rm_timing)]),
    "rm_accumulate_moving_device": (C.c_int, [_VP, _P(rm_params), _P(rm_lens), _VP, _VP, C.c_uint32, _VP, C.c_uint32, C.c_uint32, _VP, _VP,
                                              _VP, _VP]),
    "rm_render_progressive_moving": (C.c_int, [_VP, _P(rm_params), _P(rm_lens), _P(C.c_double), C.c_uint32, _P(rm_vec3), C.c_uint32,
                                               C.c_double, C.c_int, _P(C.c_double), _P(C.c_uint8), _P(C.c_uint32), _P(rm_timing)]),
    "rm_converge_workspace": (C.c_int, [_P(rm_params), _P(C.c_size_t)]),
    "rm_accumulate_converging_device": (C.c_int, [_VP, _P(rm_params), _P(rm_lens), _P(rm_converge), _VP, C.c_uint32, _VP, C.c_uint32, C.c_int,
                                                  _P(rm_converge_frame), _VP]),
    "rm_render_converging": (C.c_int, [_VP, _P(rm_params), _P(rm_lens), _P(rm_converge), _P(C.c_double), C.c_uint32, C.c_int,
                                       _P(C.c_double), _P(C.c_uint8), _P(rm_converge_report), _P(rm_timing)]),
    "rm_accumulate_converging_motion_device": (C.c_int, [_VP, _P(rm_params), _P(rm_lens), _P(rm_converge), _VP, C.c_uint32, _VP, C.c_uint32, _VP,
                                                         C.c_uint32, C.c_int, _P(rm_converge_frame), _VP]),
    "rm_render_converging_motion": (C.c_int, [_VP, _P(rm_params), _P(rm_lens), _P(rm_converge), _P(C.c_double), C.c_uint32, _P(rm_vec3),
                                              C.c_uint32, C.c_double, C.c_int, _P(C.c_double), _P(C.c_uint8), _P(rm_converge_report),
                                              _P(rm_timing)]),
    "rm_accumulate_converging_moving_device": (C.c_int, [_VP, _P(rm_params), _P(rm_lens), _P(rm_converge), _VP, C.c_uint32, _VP, C.c_uint32, _VP,
                                                         C.c_uint32, C.c_int, _P(rm_converge_frame), _VP]),
    "rm_render_converging_moving": (C.c_int, [_VP, _P(rm_params), _P(rm_lens), _P(rm_converge), _P(C.c_double), C.c_uint32, _P(rm_vec3),
                                              C.c_uint32, C.c_double, C.c_int, _P(C.c_double), _P(C.c_uint8), _P(rm_converge_report),
                                              _P(rm_timing)]),
    "rm_camera_sequence": (C.c_int, [C.c_uint32, C.c_uint32, _P(rm_camera_motion), _P(rm_camera_basis), C.c_double, _P(C.c_double)]),
    "rm_accumulate_camera_device": (C.c_int, [_VP, _P(rm_params), _P(rm_lens), _VP, _VP, _VP, C.c_uint32, _VP, C.c_uint32, C.c_uint32, _VP, _VP,
                                              _VP, _VP]),
    "rm_accumulate_converging_camera_device": (C.c_int, [_VP, _P(rm_params), _P(rm_lens), _P(rm_converge), _VP, C.c_uint32, _VP, _VP, C.c_uint32,
                                                         _VP, C.c_uint32, C.c_int, _P(rm_converge_frame), _VP]),
    "rm_render_progressive_camera": (C.c_int, [_VP, _P(rm_params), _P(rm_lens), _P(C.c_double), C.c_uint32, _P(rm_vec3), C.c_uint32,
                                               C.c_double, _P(rm_camera_motion), C.c_int, _P(C.c_double), _P(C.c_uint8), _P(C.c_uint32),
                                               _P(rm_timing)]),
    "rm_render_converging_camera": (C.c_int, [_VP, _P(rm_params), _P(rm_lens), _P(rm_converge), _P(C.c_double), C.c_uint32, _P(rm_vec3),
                                              C.c_uint32, C.c_double, _P(rm_camera_motion), C.c_int, _P(C.c_double), _P(C.c_uint8),
                                              _P(rm_converge_report), _P(rm_timing)]),
    "rm_swept_extents": (C.c_int, [_P(C.c_double), C.c_uint32, C.c_uint32, _P(C.c_double), _P(C.c_double)]),
    "rm_swept_motion_extents": (C.c_int, [_P(rm_vec3), C.c_uint32, C.c_double, _P(C.c_double), _P(C.c_double)]),
    "rm_swept_build": (C.c_int, [_VP, _P(C.c_double), _P(C.c_double), C.c_uint32, _P(_VP)]),
    "rm_swept_free": (None, [_VP, _VP]),
    "rm_accumulate_swept_device": (C.c_int, [_VP, _P(rm_params), _P(rm_lens), _VP, _VP, C.c_uint32, _VP, C.c_uint32, _VP, C.c_uint32, _VP, _VP,
                                             _VP, _VP]),
    "rm_accumulate_converging_swept_device": (C.c_int, [_VP, _P(rm_params), _P(rm_lens), _P(rm_converge), _VP, C.c_uint32, _VP, C.c_uint32, _VP,
                                                        C.c_uint32, _VP, C.c_int, _P(rm_converge_frame), _VP]),
    "rm_accumulate_camera_swept_device": (C.c_int, [_VP, _P(rm_params), _P(rm_lens), _VP, _VP, _VP, C.c_uint32, _VP, C.c_uint32, _VP, C.c_uint32,
                                                    _VP, _VP, _VP, _VP]),
    "rm_accumulate_converging_camera_swept_device": (C.c_int, [_VP, _P(rm_params), _P(rm_lens), _P(rm_converge), _VP, C.c_uint32, _VP, _VP,
                                                               C.c_uint32, _VP, C.c_uint32, _VP, C.c_int, _P(rm_converge_frame), _VP]),
    "rm_swept_tick_info": (C.c_int, [_VP, _P(rm_swept_tick_report)]),
    "rm_denoise_workspace": (C.c_int, [_P(rm_params), _P(C.c_size_t)]),
    "rm_denoise_device": (C.c_int, [_VP, _P(rm_params), _P(rm_denoise), _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "rm_render_denoised": (C.c_int, [_VP, _P(rm_params), _P(rm_denoise), C.c_int, _P(C.c_double), _P(C.c_uint8), _P(rm_timing)]),
    "rm_reproject_device": (C.c_int, [_VP, _P(rm_params), _P(rm_reproject), _P(rm_view), _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "rm_converge_history": (C.c_int, [_VP, _P(rm_reproject)]),
    "rm_converge_history_info": (C.c_int, [_VP, _P(rm_history_report)]),
    "rm_bounce_sequence": (C.c_int, [C.c_uint32, C.c_uint32, _P(C.c_double)]),
    "rm_accumulate_bounce_device": (C.c_int, [_VP, _P(rm_params), _P(rm_lens), _VP, _VP, C.c_uint32, _VP, C.c_double, C.c_uint32, _VP, _VP,
                                              _VP, _VP]),
    "rm_accumulate_converging_bounce_device": (C.c_int, [_VP, _P(rm_params), _P(rm_lens), _P(rm_converge), _VP, C.c_uint32, _VP, C.c_uint32, _VP,
                                                         C.c_double, C.c_int, _P(rm_converge_frame), _VP]),
    "rm_render_progressive_bounce": (C.c_int, [_VP, _P(rm_params), _P(rm_lens), _P(C.c_double), C.c_uint32, C.c_double, C.c_int,
                                               _P(C.c_double), _P(C.c_uint8), _P(C.c_uint32), _P(rm_timing)]),
    "rm_render_converging_bounce": (C.c_int, [_VP, _P(rm_params), _P(rm_lens), _P(rm_converge), _P(C.c_double), C.c_uint32, C.c_double,
                                              C.c_int, _P(C.c_double), _P(C.c_uint8), _P(rm_converge_report), _P(rm_timing)]),
    "rm_abi_version": (C.c_uint32, []),
    "rm_build_info": (C.c_char_p, []),
    "rm_device_info": (C.c_int, [_VP, C.c_char_p, C.c_size_t, _P(C.c_int), _P(C.c_size_t)]),
    "rm_kernel_name": (C.c_int, [_VP, _P(rm_params), C.c_char_p, C.c_size_t]),
}

# ... and the one internal hook with a prototype here (not part of the ABI; rm_plan.cpp): header[19], integer_exponents,
# max_depth -> variant[3] = bvh, pow_mode, stack; total, rays_per_pixel, n_cus, per_cu, max_blocks -> *grid
INTERNAL_SIGNATURES = {
    "rmi_shading_launch": (C.c_int, [_P(C.c_uint32), C.c_uint32, C.c_uint32, _P(C.c_uint32), C.c_uint32, C.c_uint32, C.c_int32, C.c_int32,
                                     C.c_uint32, _P(C.c_uint32)]),
}

_lib = None


class BackendError(RuntimeError):
    """Non-zero rm_status.  The reference's failure mode on this path is a panic."""

    def __init__(self, status, message):
        super().__init__("%s: %s" % (STATUS_NAMES.get(status, status), message))
        self.status = status


def lib():
    """The loaded C-ABI library.  Raises if the HIP extension has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                "%s is missing: build it with `make -C rusty-marcher_amd/csrc` "
                "(or __graft_entry__.build()); there is no CPU fallback" % LIB_PATH)
        # One HIP runtime per process: the PyTorch wheel carries its own libamdhip64.so.7.
        # Importing torch first makes the dynamic loader resolve this library's
        # NEEDED libamdhip64.so.7 to that already-loaded copy (same SONAME), so device
        # pointers and streams are shared with torch.  Loaded the other way round, the
        # process would hold two runtimes and the second finds no device.
        import torch  # noqa: F401
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in list(SIGNATURES.items()) + list(INTERNAL_SIGNATURES.items()):
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def check(status, ctx=None):
    if status != RM_OK:
        msg = lib().rm_last_error(ctx)
        raise BackendError(status, msg.decode() if msg else "")


def camera_basis(b):
    """rm_camera_basis from one, or from three vectors (right, up, forward)."""
    if isinstance(b, rm_camera_basis):
        return b
    right, up, forward = b
    return rm_camera_basis(vec3(right), vec3(up), vec3(forward))


def vec3(v):
    if isinstance(v, rm_vec3):
        return v
    if hasattr(v, "x"):
        return rm_vec3(float(v.x), float(v.y), float(v.z))
    x, y, z = v
    return rm_vec3(float(x), float(y), float(z))
