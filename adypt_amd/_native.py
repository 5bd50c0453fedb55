"""ctypes binding of adypt_amd/libadypt_hip.so (C-ABI: include/adypt_hip.h + include/adypt_host.h).

The library is built in-tree by ``adypt_amd/csrc/Makefile`` (``__graft_entry__.build()``).  There is no Python or
CPU fallback for the GPU path: if the shared object is missing, importing this module raises, and without a HIP
device ``adypt_create`` fails with ``ADYPT_E_NO_DEVICE``.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("ADYPT_LIB", os.path.join(_HERE, "libadypt_hip.so"))  # ADYPT_LIB: measurement-only variant builds

ADYPT_OK = 0
E_INVALID, E_NO_DEVICE, E_HIP, E_OOM, E_STACK_OVERFLOW, E_BAD_MATERIAL, E_IO, E_PARSE, E_STATE = range(-1, -10, -1)
_ERR_NAMES = {E_INVALID: "ADYPT_E_INVALID", E_NO_DEVICE: "ADYPT_E_NO_DEVICE", E_HIP: "ADYPT_E_HIP", E_OOM: "ADYPT_E_OOM",
              E_STACK_OVERFLOW: "ADYPT_E_STACK_OVERFLOW", E_BAD_MATERIAL: "ADYPT_E_BAD_MATERIAL", E_IO: "ADYPT_E_IO",
              E_PARSE: "ADYPT_E_PARSE", E_STATE: "ADYPT_E_STATE"}


class AdyptError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__("%s (%d): %s" % (_ERR_NAMES.get(code, "ADYPT_E_?"), code, msg))
        self.code = code


class Texture(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("rgb", C.c_void_p)]


class Struct(C.Structure):
    """A C struct whose fields make a dict by name."""

    def as_dict(self) -> dict:
        return {k: getattr(self, k) for k, _ in self._fields_}


class SceneDesc(C.Structure):
    _fields_ = [("nodes", C.c_void_p), ("n_nodes", C.c_int64), ("tri_indices", C.c_void_p), ("n_refs", C.c_int64),
                ("woop", C.c_void_p), ("triangles", C.c_void_p), ("n_tris", C.c_int64), ("materials", C.c_void_p),
                ("n_mats", C.c_int64), ("textures", C.c_void_p), ("n_textures", C.c_int32), ("width", C.c_int32),
                ("height", C.c_int32), ("device", C.c_int32), ("tile_rank", C.c_int32), ("tile_nranks", C.c_int32)]


class PtParams(C.Structure):
    _fields_ = [("stack_size", C.c_int32), ("max_bounce", C.c_int32), ("subpixel", C.c_int32), ("tmp_lifetime", C.c_int32),
                ("ray_tmin", C.c_float), ("clamp", C.c_float), ("sun", C.c_float * 3), ("shift_seed", C.c_uint32)]


class Hit(C.Structure):
    _fields_ = [("ref_idx", C.c_int32), ("tri_id", C.c_int32), ("u", C.c_float), ("v", C.c_float), ("t", C.c_float),
                ("nodes", C.c_uint32), ("tris", C.c_uint32), ("hash", C.c_uint32), ("max_depth", C.c_uint32)]


class Stats(Struct):
    _fields_ = [("rays", C.c_uint64), ("nodes_visited", C.c_uint64), ("tris_tested", C.c_uint64), ("hits", C.c_uint64),
                ("shaded", C.c_uint64), ("stack_overflows", C.c_uint64), ("bad_materials", C.c_uint64),
                ("max_stack", C.c_uint32), ("trace_launches", C.c_uint32), ("trace_ms", C.c_double), ("shade_ms", C.c_double),
                ("path_ms", C.c_double), ("path_launches", C.c_uint32), ("audit_errors", C.c_uint32), ("path_rays", C.c_uint64),
                ("path_nodes", C.c_uint64), ("path_tris", C.c_uint64), ("path_hits", C.c_uint64), ("path_shaded", C.c_uint64)]


class Noise(Struct):
    _fields_ = [("mean_noise", C.c_double), ("worst_block", C.c_double), ("worst_index", C.c_int32), ("spp", C.c_int32),
                ("pixels", C.c_int64)]


class Adaptive(C.Structure):
    """adypt_adaptive: what adypt_trace_adaptive reports."""
    _fields_ = [("noise", Noise), ("blocks", C.c_int32), ("blocks_frozen", C.c_int32), ("pixel_samples", C.c_int64)]

    def as_dict(self):
        d = self.noise.as_dict()
        d.update(blocks=self.blocks, blocks_frozen=self.blocks_frozen, pixel_samples=self.pixel_samples)
        return d


class HistoryPlanParams(C.Structure):
    """adypt_history_plan_params."""
    _fields_ = [("target", C.c_int32), ("min_spp", C.c_int32), ("max_spp", C.c_int32), ("step", C.c_int32), ("tolerance_permille", C.c_int32),
                ("history_cap", C.c_float), ("follow_motion", C.c_int32), ("moments", C.c_int32)]


class HistoryPlan(Struct):
    """adypt_history_plan: what adypt_plan_by_history and adypt_trace_by_history report."""
    _fields_ = [("blocks", C.c_int32), ("want_min", C.c_int32), ("want_max", C.c_int32), ("spp", C.c_int32), ("pixels", C.c_int64),
                ("pixels_with_history", C.c_int64), ("pixel_samples", C.c_int64), ("mean_reach", C.c_double), ("capture_ms", C.c_float),
                ("reach_ms", C.c_float), ("device_bytes", C.c_int64)]


class DenoiseParams(C.Structure):
    """adypt_denoise_params."""
    _fields_ = [("levels", C.c_int32), ("sigma_l", C.c_float), ("sigma_z", C.c_float)]


class TemporalParams(C.Structure):
    """adypt_temporal_params."""
    _fields_ = [("history_cap", C.c_float), ("commit", C.c_int32)]


class DenoiseMotion(Struct):
    """adypt_denoise_motion."""
    _fields_ = [("have_snapshot", C.c_int32), ("snapshot_ms", C.c_float), ("n_tris", C.c_int64), ("device_bytes", C.c_int64)]


class RectifyParams(C.Structure):
    """adypt_rectify_params."""
    _fields_ = [("radius", C.c_int32), ("gamma", C.c_float)]


class DenoiseRectify(Struct):
    """adypt_denoise_rectify."""
    _fields_ = [("have", C.c_int32), ("radius", C.c_int32), ("gamma", C.c_float), ("window_ms", C.c_float), ("device_bytes", C.c_int64)]


class DenoiseMoments(Struct):
    """adypt_denoise_moments."""
    _fields_ = [("have", C.c_int32), ("variance_ms", C.c_float), ("pixels_spatial", C.c_int64), ("device_bytes", C.c_int64)]


class SpecularParams(C.Structure):
    """adypt_specular_params."""
    _fields_ = [("bounces", C.c_int32)]


class DenoiseSpecular(Struct):
    """adypt_denoise_specular_info."""
    _fields_ = [("have", C.c_int32), ("bounces", C.c_int32), ("chain_ms", C.c_float), ("rays", C.c_int64), ("pixels_followed", C.c_int64),
                ("pixels_escaped", C.c_int64), ("pixels_truncated", C.c_int64), ("device_bytes", C.c_int64)]


class DenoiseVirtual(Struct):
    """adypt_denoise_virtual."""
    _fields_ = [("have", C.c_int32), ("bounces", C.c_int32), ("pixels_followed", C.c_int64), ("pixels_with_history", C.c_int64), ("device_bytes", C.c_int64)]


class BvhParams(C.Structure):
    _fields_ = [("max_spatial_depth", C.c_int32), ("triangle_sah", C.c_float), ("node_sah", C.c_float)]


class Config(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("bvh", BvhParams),
                ("invocation_size", C.c_int32), ("stack_size", C.c_int32), ("max_bounce", C.c_int32), ("subpixel", C.c_int32),
                ("tmp_lifetime", C.c_int32), ("ray_tmin", C.c_float), ("clamp", C.c_float), ("sun", C.c_float * 3),
                ("speed", C.c_float), ("mouse_sensitive", C.c_float), ("fov", C.c_float), ("yaw", C.c_float),
                ("pitch", C.c_float), ("position", C.c_float * 3), ("obj_filename", C.c_char * 1024),
                ("bvh_filename", C.c_char * 1024)]


class BuildInfo(C.Structure):
    _fields_ = [("sbvh_nodes", C.c_int64), ("refs", C.c_int64), ("wide_nodes", C.c_int64), ("sbvh_ms", C.c_double),
                ("wide_ms", C.c_double)]


class RebuildInfo(Struct):
    """adypt_rebuild_info."""
    _fields_ = [("n_nodes", C.c_int64), ("n_refs", C.c_int64), ("levels", C.c_int32), ("binary_depth", C.c_int32)]


class TreeCost(Struct):
    """adypt_tree_cost."""
    _fields_ = [("cost", C.c_double), ("inner_q", C.c_uint64), ("leaf_q", C.c_uint64), ("n_nodes", C.c_int64)]


class PosePolicy(C.Structure):
    """adypt_pose_policy."""
    _fields_ = [("rebuild_above", C.c_double), ("method", C.c_int32), ("radius", C.c_int32), ("split_budget", C.c_double)]


class PoseOutcome(C.Structure):
    """adypt_pose_outcome."""
    _fields_ = [("built", TreeCost), ("refitted", TreeCost), ("now", TreeCost), ("rebuilt", C.c_int32), ("rebuild", RebuildInfo), ("cost_ms", C.c_float)]

    def as_dict(self):
        return {"built": self.built.as_dict(), "refitted": self.refitted.as_dict(), "now": self.now.as_dict(), "rebuilt": int(self.rebuilt),
                "rebuild": self.rebuild.as_dict(), "cost_ms": float(self.cost_ms)}


class PoseBinding(Struct):
    """adypt_pose_binding."""
    _fields_ = [("kind", C.c_int32), ("n_matrices", C.c_int32), ("n_tris", C.c_int64), ("device_bytes", C.c_int64)]


class MorphBinding(Struct):
    """adypt_morph_binding."""
    _fields_ = [("n_targets", C.c_int32), ("n_entries", C.c_int64), ("n_tris_touched", C.c_int64), ("device_bytes", C.c_int64)]


class MeshBinding(Struct):
    """adypt_mesh_binding."""
    _fields_ = [("n_vertices", C.c_int64), ("n_tris", C.c_int64), ("max_valence", C.c_int32), ("device_bytes", C.c_int64)]


class AppearanceInfo(Struct):
    """adypt_appearance_info."""
    _fields_ = [("n_mats", C.c_int64), ("n_texels", C.c_int64), ("device_bytes", C.c_int64), ("reclassed", C.c_int64), ("n_textures", C.c_int32),
                ("staged_ms", C.c_float), ("packed_ms", C.c_float), ("classified_ms", C.c_float)]


# every symbol include/*.h declares, with its signature (tests/test_abi.py checks the export list against the headers)
_SIGS = {
    # adypt_hip.h
    "adypt_abi_version": (C.c_int, []),
    "adypt_enable_test_hooks": (C.c_int, [C.c_uint64]),
    "adypt_test_hooks_enabled": (C.c_int, []),
    "adypt_create": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(SceneDesc)]),
    "adypt_destroy": (None, [C.c_void_p]),
    "adypt_last_error": (C.c_char_p, [C.c_void_p]),
    "adypt_set_params": (C.c_int, [C.c_void_p, C.POINTER(PtParams)]),
    "adypt_set_camera": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "adypt_trace_primary": (C.c_int, [C.c_void_p, C.c_int]),
    "adypt_trace_spp": (C.c_int, [C.c_void_p, C.c_int]),
    "adypt_reset": (C.c_int, [C.c_void_p]),
    "adypt_get_spp": (C.c_int, [C.c_void_p]),
    "adypt_set_frames_in_flight": (C.c_int, [C.c_void_p, C.c_int]),
    "adypt_get_frames_in_flight": (C.c_int, [C.c_void_p]),
    "adypt_set_pipeline": (C.c_int, [C.c_void_p, C.c_int]),
    "adypt_get_pipeline": (C.c_int, [C.c_void_p]),
    "adypt_set_lookahead": (C.c_int, [C.c_void_p, C.c_int]),
    "adypt_get_lookahead_frames": (C.c_int, [C.c_void_p]),
    "adypt_read_radiance": (C.c_int, [C.c_void_p, C.c_void_p]),
    "adypt_read_hits": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "adypt_trace_rays": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int]),
    "adypt_trace_rays_any": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int]),
    "adypt_set_instrumentation": (C.c_int, [C.c_void_p, C.c_int]),
    "adypt_get_stats": (C.c_int, [C.c_void_p, C.POINTER(Stats)]),
    "adypt_reset_stats": (C.c_int, [C.c_void_p]),
    "adypt_get_wave_profile": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]),
    "adypt_read_root_card": (C.c_int, [C.c_void_p, C.c_void_p]),
    "adypt_get_shader_clock": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]),
    "adypt_local_pixel_count": (C.c_int64, [C.c_void_p]),
    "adypt_set_sun_visibility": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "adypt_trace_spp_async": (C.c_int, [C.c_void_p, C.c_int]),
    "adypt_wait": (C.c_int, [C.c_void_p]),
    "adypt_read_display": (C.c_int, [C.c_void_p, C.c_void_p]),
    "adypt_local_radiance_device": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
    "adypt_copy_local_radiance": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64]),
    "adypt_assemble_radiance": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "adypt_shard_block_count": (C.c_int64, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "adypt_untile_host": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    # noise statistics
    "adypt_set_noise_stats": (C.c_int, [C.c_void_p, C.c_int]),
    "adypt_get_noise_stats": (C.c_int, [C.c_void_p]),
    "adypt_get_noise": (C.c_int, [C.c_void_p, C.POINTER(Noise)]),
    "adypt_read_noise": (C.c_int, [C.c_void_p, C.c_void_p]),
    "adypt_read_noise_moments": (C.c_int, [C.c_void_p, C.c_void_p]),
    "adypt_read_block_noise": (C.c_int64, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]),
    "adypt_trace_until": (C.c_int, [C.c_void_p, C.c_double, C.c_int, C.c_int, C.c_int, C.POINTER(Noise)]),
    "adypt_trace_adaptive": (C.c_int, [C.c_void_p, C.c_double, C.c_int, C.c_int, C.c_int, C.POINTER(Adaptive)]),
    "adypt_read_block_spp": (C.c_int64, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]),
    "adypt_plan_by_history": (C.c_int, [C.c_void_p, C.POINTER(HistoryPlanParams), C.POINTER(HistoryPlan)]),
    "adypt_trace_by_history": (C.c_int, [C.c_void_p, C.POINTER(HistoryPlanParams), C.POINTER(HistoryPlan)]),
    "adypt_read_history_reach": (C.c_int, [C.c_void_p, C.c_void_p]),
    "adypt_read_sample_plan": (C.c_int64, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]),
    "adypt_read_history_bins": (C.c_int64, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]),
    "adypt_multi_plan_by_history": (C.c_int, [C.c_void_p, C.POINTER(HistoryPlanParams), C.POINTER(HistoryPlan)]),
    "adypt_multi_trace_by_history": (C.c_int, [C.c_void_p, C.POINTER(HistoryPlanParams), C.POINTER(HistoryPlan)]),
    "adypt_multi_read_history_reach": (C.c_int, [C.c_void_p, C.c_void_p]),
    "adypt_multi_read_sample_plan": (C.c_int64, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]),
    "adypt_multi_read_history_bins": (C.c_int64, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]),
    "adypt_multi_trace_adaptive": (C.c_int, [C.c_void_p, C.c_double, C.c_int, C.c_int, C.c_int, C.POINTER(Adaptive)]),
    "adypt_multi_set_noise_stats": (C.c_int, [C.c_void_p, C.c_int]),
    "adypt_multi_get_noise": (C.c_int, [C.c_void_p, C.POINTER(Noise)]),
    "adypt_multi_read_noise": (C.c_int, [C.c_void_p, C.c_void_p]),
    "adypt_multi_trace_until": (C.c_int, [C.c_void_p, C.c_double, C.c_int, C.c_int, C.c_int, C.POINTER(Noise)]),
    # denoising
    "adypt_denoise": (C.c_int, [C.c_void_p, C.POINTER(DenoiseParams)]),
    "adypt_read_denoised": (C.c_int, [C.c_void_p, C.c_void_p]),
    "adypt_read_denoise_guides": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "adypt_get_denoise_timing": (C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.c_int]),
    "adypt_denoise_temporal": (C.c_int, [C.c_void_p, C.POINTER(DenoiseParams), C.POINTER(TemporalParams)]),
    "adypt_denoise_history_reset": (C.c_int, [C.c_void_p]),
    "adypt_read_denoise_history": (C.c_int, [C.c_void_p, C.c_void_p]),
    "adypt_get_denoise_merge_ms": (C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
    "adypt_multi_denoise_temporal": (C.c_int, [C.c_void_p, C.POINTER(DenoiseParams), C.POINTER(TemporalParams)]),
    "adypt_multi_denoise_history_reset": (C.c_int, [C.c_void_p]),
    "adypt_multi_read_denoise_history": (C.c_int, [C.c_void_p, C.c_void_p]),
    "adypt_multi_get_denoise_merge_ms": (C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
    "adypt_denoise_temporal_motion": (C.c_int, [C.c_void_p, C.POINTER(DenoiseParams), C.POINTER(TemporalParams)]),
    "adypt_read_denoise_motion": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "adypt_get_denoise_motion": (C.c_int, [C.c_void_p, C.POINTER(DenoiseMotion)]),
    "adypt_multi_denoise_temporal_motion": (C.c_int, [C.c_void_p, C.POINTER(DenoiseParams), C.POINTER(TemporalParams)]),
    "adypt_multi_read_denoise_motion": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "adypt_multi_get_denoise_motion": (C.c_int, [C.c_void_p, C.POINTER(DenoiseMotion)]),
    "adypt_denoise_temporal_rectified": (C.c_int, [C.c_void_p, C.POINTER(DenoiseParams), C.POINTER(TemporalParams), C.POINTER(RectifyParams), C.c_int]),
    "adypt_read_denoise_rectify": (C.c_int, [C.c_void_p, C.c_void_p]),
    "adypt_get_denoise_rectify": (C.c_int, [C.c_void_p, C.POINTER(DenoiseRectify)]),
    "adypt_multi_denoise_temporal_rectified": (C.c_int, [C.c_void_p, C.POINTER(DenoiseParams), C.POINTER(TemporalParams), C.POINTER(RectifyParams), C.c_int]),
    "adypt_multi_read_denoise_rectify": (C.c_int, [C.c_void_p, C.c_void_p]),
    "adypt_multi_get_denoise_rectify": (C.c_int, [C.c_void_p, C.POINTER(DenoiseRectify)]),
    "adypt_denoise_temporal_moments": (C.c_int, [C.c_void_p, C.POINTER(DenoiseParams), C.POINTER(TemporalParams), C.c_int]),
    "adypt_read_denoise_variance": (C.c_int, [C.c_void_p, C.c_void_p]),
    "adypt_get_denoise_moments": (C.c_int, [C.c_void_p, C.POINTER(DenoiseMoments)]),
    "adypt_multi_denoise_temporal_moments": (C.c_int, [C.c_void_p, C.POINTER(DenoiseParams), C.POINTER(TemporalParams), C.c_int]),
    "adypt_multi_read_denoise_variance": (C.c_int, [C.c_void_p, C.c_void_p]),
    "adypt_multi_get_denoise_moments": (C.c_int, [C.c_void_p, C.POINTER(DenoiseMoments)]),
    "adypt_denoise_specular": (C.c_int, [C.c_void_p, C.POINTER(DenoiseParams), C.POINTER(SpecularParams)]),
    "adypt_read_denoise_guides_specular": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "adypt_get_denoise_specular": (C.c_int, [C.c_void_p, C.POINTER(DenoiseSpecular)]),
    "adypt_multi_denoise_specular": (C.c_int, [C.c_void_p, C.POINTER(DenoiseParams), C.POINTER(SpecularParams)]),
    "adypt_multi_read_denoise_guides_specular": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "adypt_multi_get_denoise_specular": (C.c_int, [C.c_void_p, C.POINTER(DenoiseSpecular)]),
    "adypt_denoise_temporal_specular": (C.c_int, [C.c_void_p, C.POINTER(DenoiseParams), C.POINTER(TemporalParams), C.POINTER(SpecularParams)]),
    "adypt_read_denoise_virtual": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "adypt_get_denoise_virtual": (C.c_int, [C.c_void_p, C.POINTER(DenoiseVirtual)]),
    "adypt_multi_denoise_temporal_specular": (C.c_int, [C.c_void_p, C.POINTER(DenoiseParams), C.POINTER(TemporalParams), C.POINTER(SpecularParams)]),
    "adypt_multi_read_denoise_virtual": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "adypt_multi_get_denoise_virtual": (C.c_int, [C.c_void_p, C.POINTER(DenoiseVirtual)]),
    "adypt_multi_denoise": (C.c_int, [C.c_void_p, C.POINTER(DenoiseParams)]),
    "adypt_multi_read_denoised": (C.c_int, [C.c_void_p, C.c_void_p]),
    "adypt_multi_read_denoise_guides": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    # moving geometry
    "adypt_update_triangles": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p]),
    "adypt_read_bvh": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "adypt_get_refit_timing": (C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.c_int]),
    "adypt_multi_update_triangles": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p]),
    # rebuilding the tree on the GPU
    "adypt_rebuild_bvh": (C.c_int, [C.c_void_p, C.POINTER(BvhParams), C.POINTER(RebuildInfo)]),
    "adypt_get_rebuild_timing": (C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.c_int]),
    "adypt_get_bvh_sizes": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "adypt_read_tri_indices": (C.c_int, [C.c_void_p, C.c_void_p]),
    "adypt_rebuild_bvh_ploc": (C.c_int, [C.c_void_p, C.POINTER(BvhParams), C.c_int, C.POINTER(RebuildInfo)]),
    "adypt_multi_rebuild_bvh": (C.c_int, [C.c_void_p, C.POINTER(BvhParams), C.POINTER(RebuildInfo)]),
    "adypt_multi_rebuild_bvh_ploc": (C.c_int, [C.c_void_p, C.POINTER(BvhParams), C.c_int, C.POINTER(RebuildInfo)]),
    "adypt_rebuild_bvh_ploc_split": (C.c_int, [C.c_void_p, C.POINTER(BvhParams), C.c_int, C.c_double, C.POINTER(RebuildInfo)]),
    "adypt_multi_rebuild_bvh_ploc_split": (C.c_int, [C.c_void_p, C.POINTER(BvhParams), C.c_int, C.c_double, C.POINTER(RebuildInfo)]),
    "adypt_get_rebuild_presplit": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32)]),
    "adypt_read_ref_boxes": (C.c_int64, [C.c_void_p, C.c_void_p]),
    # replacing the triangles on the GPU
    "adypt_set_triangles": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(BvhParams), C.c_int, C.c_int, C.c_double, C.POINTER(RebuildInfo)]),
    "adypt_create_from_triangles": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(SceneDesc), C.POINTER(BvhParams), C.c_int, C.c_int, C.c_double, C.POINTER(RebuildInfo)]),
    "adypt_get_triangle_count": (C.c_int64, [C.c_void_p]),
    "adypt_read_triangle_records": (C.c_int, [C.c_void_p, C.c_void_p]),
    "adypt_get_set_triangles_timing": (C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.c_int]),
    "adypt_multi_set_triangles": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(BvhParams), C.c_int, C.c_int, C.c_double, C.POINTER(RebuildInfo)]),
    "adypt_create_multi_from_triangles": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(SceneDesc), C.POINTER(C.c_int), C.c_int, C.POINTER(BvhParams), C.c_int, C.c_int, C.c_double,
                                                    C.POINTER(RebuildInfo)]),
    # refit or rebuild by the tree's SAH cost
    "adypt_get_tree_cost": (C.c_int, [C.c_void_p, C.POINTER(BvhParams), C.POINTER(TreeCost)]),
    "adypt_update_triangles_auto": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.POINTER(BvhParams), C.POINTER(PosePolicy), C.POINTER(PoseOutcome)]),
    "adypt_multi_get_tree_cost": (C.c_int, [C.c_void_p, C.POINTER(BvhParams), C.POINTER(TreeCost)]),
    "adypt_multi_update_triangles_auto": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.POINTER(BvhParams), C.POINTER(PosePolicy), C.POINTER(PoseOutcome)]),
    # posing on the GPU
    "adypt_bind_parts": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32]),
    "adypt_bind_skin": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32]),
    "adypt_pose": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(BvhParams), C.POINTER(PosePolicy), C.POINTER(PoseOutcome)]),
    "adypt_unbind_pose": (C.c_int, [C.c_void_p]),
    "adypt_get_pose_binding": (C.c_int, [C.c_void_p, C.POINTER(PoseBinding)]),
    "adypt_multi_bind_parts": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32]),
    "adypt_multi_bind_skin": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32]),
    "adypt_multi_pose": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(BvhParams), C.POINTER(PosePolicy), C.POINTER(PoseOutcome)]),
    "adypt_multi_unbind_pose": (C.c_int, [C.c_void_p]),
    "adypt_multi_get_pose_binding": (C.c_int, [C.c_void_p, C.POINTER(PoseBinding)]),
    # morph targets in front of the matrices
    "adypt_bind_morph": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32]),
    "adypt_pose_morph": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.POINTER(BvhParams), C.POINTER(PosePolicy), C.POINTER(PoseOutcome)]),
    "adypt_unbind_morph": (C.c_int, [C.c_void_p]),
    "adypt_get_morph_binding": (C.c_int, [C.c_void_p, C.POINTER(MorphBinding)]),
    "adypt_multi_bind_morph": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32]),
    "adypt_multi_pose_morph": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.POINTER(BvhParams), C.POINTER(PosePolicy), C.POINTER(PoseOutcome)]),
    "adypt_multi_unbind_morph": (C.c_int, [C.c_void_p]),
    "adypt_multi_get_morph_binding": (C.c_int, [C.c_void_p, C.POINTER(MorphBinding)]),
    # an indexed mesh posed by its vertices
    "adypt_bind_mesh": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64]),
    "adypt_pose_vertices": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(BvhParams), C.POINTER(PosePolicy), C.POINTER(PoseOutcome)]),
    "adypt_read_vertex_normals": (C.c_int, [C.c_void_p, C.c_void_p]),
    "adypt_get_mesh_timing": (C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.c_int]),
    "adypt_unbind_mesh": (C.c_int, [C.c_void_p]),
    "adypt_get_mesh_binding": (C.c_int, [C.c_void_p, C.POINTER(MeshBinding)]),
    "adypt_multi_bind_mesh": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64]),
    "adypt_multi_pose_vertices": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(BvhParams), C.POINTER(PosePolicy), C.POINTER(PoseOutcome)]),
    "adypt_multi_read_vertex_normals": (C.c_int, [C.c_void_p, C.c_void_p]),
    "adypt_multi_unbind_mesh": (C.c_int, [C.c_void_p]),
    "adypt_multi_get_mesh_binding": (C.c_int, [C.c_void_p, C.POINTER(MeshBinding)]),
    # materials, textures and triangle attributes changed on the GPU
    "adypt_set_materials": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32]),
    "adypt_update_texture": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32]),
    "adypt_set_triangle_attributes": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p]),
    "adypt_read_material_records": (C.c_int, [C.c_void_p, C.c_void_p]),
    "adypt_read_texels": (C.c_int, [C.c_void_p, C.c_void_p]),
    "adypt_get_appearance": (C.c_int, [C.c_void_p, C.POINTER(AppearanceInfo)]),
    "adypt_multi_set_materials": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32]),
    "adypt_multi_update_texture": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32]),
    "adypt_multi_set_triangle_attributes": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p]),
    # native multi-GPU (RCCL inside the library)
    "adypt_create_multi": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(SceneDesc), C.POINTER(C.c_int), C.c_int]),
    "adypt_destroy_multi": (None, [C.c_void_p]),
    "adypt_multi_last_error": (C.c_char_p, [C.c_void_p]),
    "adypt_multi_setup_seconds": (C.c_double, [C.c_void_p, C.c_int]),
    "adypt_multi_device_count": (C.c_int, [C.c_void_p]),
    "adypt_multi_context": (C.c_void_p, [C.c_void_p, C.c_int]),
    "adypt_multi_set_params": (C.c_int, [C.c_void_p, C.POINTER(PtParams)]),
    "adypt_multi_set_camera": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "adypt_multi_set_lookahead": (C.c_int, [C.c_void_p, C.c_int]),
    "adypt_multi_trace_primary": (C.c_int, [C.c_void_p, C.c_int]),
    "adypt_multi_trace_spp": (C.c_int, [C.c_void_p, C.c_int]),
    "adypt_multi_reset": (C.c_int, [C.c_void_p]),
    "adypt_multi_get_spp": (C.c_int, [C.c_void_p]),
    "adypt_multi_set_sun_visibility": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "adypt_multi_set_instrumentation": (C.c_int, [C.c_void_p, C.c_int]),
    "adypt_multi_get_stats": (C.c_int, [C.c_void_p, C.POINTER(Stats)]),
    "adypt_multi_read_display": (C.c_int, [C.c_void_p, C.c_void_p]),
    "adypt_multi_read_radiance": (C.c_int, [C.c_void_p, C.c_void_p]),
    "adypt_multi_gather_radiance": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
    "adypt_multi_comm_init": (C.c_int, [C.c_void_p]),
    "adypt_multi_comm_ranks": (C.c_int, [C.c_void_p]),
    "adypt_comm_ranks": (C.c_int, [C.c_void_p]),
    "adypt_set_fused_bounces": (C.c_int, [C.c_void_p, C.c_int]),
    "adypt_get_fused_bounces": (C.c_int, [C.c_void_p]),
    "adypt_comm_unique_id": (C.c_int, [C.c_char_p]),
    "adypt_comm_init": (C.c_int, [C.c_void_p, C.c_char_p]),
    "adypt_comm_gather_radiance": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
    "adypt_comm_read_radiance": (C.c_int, [C.c_void_p, C.c_void_p]),
    "adypt_comm_allreduce": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.c_int, C.c_int]),
    "adypt_comm_barrier": (C.c_int, [C.c_void_p]),
    "adypt_device_synchronize": (C.c_int, [C.c_void_p]),
    # adypt_host.h
    "adypt_config_default": (None, [C.POINTER(Config)]),
    "adypt_config_load": (C.c_int, [C.c_char_p, C.POINTER(Config)]),
    "adypt_config_parse": (C.c_int, [C.c_char_p, C.POINTER(Config)]),
    "adypt_config_json": (C.c_size_t, [C.POINTER(Config), C.c_char_p, C.c_size_t]),
    "adypt_config_save": (C.c_int, [C.c_char_p, C.POINTER(Config)]),
    "adypt_host_last_error": (C.c_char_p, []),
    "adypt_camera_control": (None, [C.POINTER(Config), C.c_uint32, C.c_float, C.c_float, C.c_float]),
    "adypt_scene_load": (C.c_int, [C.c_char_p, C.POINTER(C.c_void_p)]),
    "adypt_scene_free": (None, [C.c_void_p]),
    "adypt_scene_triangles": (C.c_int64, [C.c_void_p, C.POINTER(C.c_void_p)]),
    "adypt_scene_materials": (C.c_int64, [C.c_void_p, C.POINTER(C.c_void_p)]),
    "adypt_scene_textures": (C.c_int32, [C.c_void_p, C.POINTER(C.c_void_p)]),
    "adypt_scene_aabb": (None, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "adypt_scene_warnings": (C.c_char_p, [C.c_void_p]),
    "adypt_scene_from_arrays": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.POINTER(C.c_void_p)]),
    "adypt_host_set_threads": (C.c_int, [C.c_int]),
    "adypt_host_get_threads": (C.c_int, []),
    "adypt_host_selftest_sort": (C.c_int, [C.c_int64, C.c_uint32, C.c_int, C.c_int, C.c_int64]),
    "adypt_bvh_build": (C.c_int, [C.c_void_p, C.POINTER(BvhParams), C.POINTER(C.c_void_p), C.POINTER(BuildInfo)]),
    "adypt_bvh_build_linear": (C.c_int, [C.c_void_p, C.POINTER(BvhParams), C.POINTER(C.c_void_p), C.POINTER(BuildInfo)]),
    "adypt_lbvh_keys": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p]),
    "adypt_bvh_build_ploc": (C.c_int, [C.c_void_p, C.POINTER(BvhParams), C.c_int, C.POINTER(C.c_void_p), C.POINTER(BuildInfo)]),
    "adypt_ploc_tree": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p]),
    "adypt_bvh_build_ploc_split": (C.c_int, [C.c_void_p, C.POINTER(BvhParams), C.c_int, C.c_double, C.POINTER(C.c_void_p), C.POINTER(BuildInfo)]),
    "adypt_bvh_ref_boxes": (C.c_int64, [C.c_void_p, C.POINTER(C.c_void_p)]),
    "adypt_presplit_refs": (C.c_int64, [C.c_void_p, C.c_int64, C.c_double, C.c_int64, C.POINTER(C.c_int32), C.c_void_p, C.c_void_p]),
    "adypt_bvh_load": (C.c_int, [C.c_char_p, C.POINTER(BvhParams), C.POINTER(C.c_void_p)]),
    "adypt_bvh_save": (C.c_int, [C.c_void_p, C.c_char_p, C.POINTER(BvhParams)]),
    "adypt_bvh_free": (None, [C.c_void_p]),
    "adypt_bvh_nodes": (C.c_int64, [C.c_void_p, C.POINTER(C.c_void_p)]),
    "adypt_bvh_tri_indices": (C.c_int64, [C.c_void_p, C.POINTER(C.c_void_p)]),
    "adypt_bvh_refit": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64]),
    "adypt_bvh_cost": (C.c_int, [C.c_void_p, C.c_int64, C.POINTER(BvhParams), C.POINTER(TreeCost)]),
    "adypt_woop_matrices": (None, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "adypt_pack_triangles": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p]),
    "adypt_pack_appearance": (C.c_int64, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "adypt_pose_triangles": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    "adypt_pose_triangles_morph": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                             C.c_int32, C.c_void_p]),
    "adypt_morph_diff": (C.c_int64, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "adypt_mesh_normals": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p]),
    "adypt_mesh_triangles": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "adypt_weld_triangles": (C.c_int64, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "adypt_decode_root_card": (None, [C.c_void_p, C.c_int, C.c_void_p]),
    "adypt_camera_matrices": (None, [C.c_float, C.c_float, C.c_float, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "adypt_sobol_points": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "adypt_shift_bytes": (None, [C.c_uint32, C.c_int, C.c_int, C.c_void_p]),
    "adypt_save_exr": (C.c_int, [C.c_char_p, C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "adypt_save_png": (C.c_int, [C.c_char_p, C.c_void_p, C.c_int, C.c_int]),
    "adypt_load_image_rgb8": (C.c_int, [C.c_char_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "adypt_load_exr": (C.c_int, [C.c_char_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "adypt_free": (None, [C.c_void_p]),
}

EXPORTS = tuple(_SIGS)

if not os.path.exists(LIB_PATH):
    raise ImportError("adypt_amd: %s is missing — build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                      "(hipcc --offload-arch=gfx950); there is no fallback implementation" % LIB_PATH)

def _share_torch_hip_runtime() -> None:
    """PyTorch-ROCm wheels bundle their own HIP runtime (torch/lib/libamdhip64.so, SONAME libamdhip64.so.7) and load it
    by file name, so a process that loads libadypt_hip.so (bound to /opt/rocm's copy) *before* `import torch` ends up with
    two runtimes, and the one that touches the GPU second finds no device.  Pre-loading torch's copy — without importing
    torch — makes both bind to the same runtime whatever the import order.  ADYPT_NO_TORCH_RUNTIME=1 disables this."""
    import importlib.util
    import sys
    if "torch" in sys.modules or os.environ.get("ADYPT_NO_TORCH_RUNTIME"):
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        return
    if spec is None or not spec.origin:
        return
    rt = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
    if os.path.exists(rt):
        try:
            C.CDLL(rt, mode=C.RTLD_GLOBAL)
        except OSError:
            return
        # the RCCL that goes with that runtime (the library dlopens RCCL on first use of the native multi-GPU path)
        rccl = os.path.join(os.path.dirname(rt), "librccl.so")
        if os.path.exists(rccl):
            os.environ.setdefault("ADYPT_RCCL_LIB", rccl)


_share_torch_hip_runtime()
lib = C.CDLL(LIB_PATH)
for _name, (_res, _args) in _SIGS.items():
    _fn = getattr(lib, _name)  # AttributeError here = the library does not export what the headers declare
    _fn.restype = _res
    _fn.argtypes = _args
if lib.adypt_abi_version() != 4:
    raise ImportError("adypt_amd: ABI version mismatch")


def check(code: int, ctx=None) -> None:
    if code == ADYPT_OK:
        return
    msg = lib.adypt_last_error(ctx)
    if (not msg) and ctx is not None:
        msg = b""
    host = lib.adypt_host_last_error()
    text = (msg or b"").decode("utf-8", "replace") or (host or b"").decode("utf-8", "replace")
    raise AdyptError(code, text)


def check_host(code: int) -> None:
    if code != ADYPT_OK:
        raise AdyptError(code, (lib.adypt_host_last_error() or b"").decode("utf-8", "replace"))
