"""ctypes plumbing over the C ABI of ``csrc/libmcpt_hip.so`` (``include/mcpt.h``).

This is NOT the product's host layer -- that is C++ (``host/``: ``Model`` / ``Scene`` / ``Render`` with the
reference's method names, and the ``mcpt_cli`` driver).  Python exists here only so that ``tests/``,
``bench.py`` and ``__graft_entry__.py`` can call the same C entry points, and so that ``torch`` can lend
device memory, streams and ``torch.distributed`` (RCCL) to the multi-GPU bench.

There is no CPU fallback: if the HIP library is missing this module raises at load time, and
``Renderer`` raises when ``mcpt_create`` finds no device.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import numpy as np

from . import scenes  # noqa: F401  (re-export)
# mcpt_rebuild_trees' options, info and builder constants; tests/test_rebuild.py holds their layout to the header
from .rebuild_abi import REBUILD_DEVICE, REBUILD_HOST, REBUILD_SAME, RebuildInfo, RebuildOpts  # noqa: F401
# mcpt_get_skin_info's struct and the influence count; tests/test_skin.py holds the layout to the header
from .skin_abi import SKIN_DUAL_QUATERNION, SKIN_INFLUENCES, SKIN_LINEAR, SkinInfo  # noqa: F401
# mcpt_set_vertex_morph's and mcpt_get_morph_info's structs and the flattening of a target list; tests/test_morph.py holds the layouts to the header
from .morph_abi import MORPH_MAX_TARGETS, MorphInfo, MorphTargets, flatten_targets, targets_struct  # noqa: F401
# mcpt_set_vertex_keyframes' options, mcpt_get_keyframe_info's struct and the interpolation and wrap constants; tests/test_keyframes.py holds the layouts to the header
from .keyframe_abi import KEYFRAMES_CATMULL_ROM, KEYFRAMES_CLAMP, KEYFRAMES_LINEAR, KEYFRAMES_LOOP, KEYFRAMES_MAX, KeyframeInfo, KeyframeOpts  # noqa: F401
# mcpt_update_parts' record, mcpt_get_parts_info's struct, the owner ids and route bits, and the owners a set of faces gives its records; tests/test_parts.py holds the layouts to the header
from .parts_abi import (OWNER_GROUPS, OWNER_KEYFRAMES, OWNER_MORPH, OWNER_NONE, OWNER_SKIN, PARTS_MORPH_THEN_SKIN, ROUTE_GROUPS, ROUTE_KEYFRAMES,  # noqa: F401
                        ROUTE_MORPH, ROUTE_SKIN, PartsInfo, SceneUpdate, owners_from_faces)
# mcpt_set_auto_normals' and mcpt_get_normals_info's structs and the mask of the normals a set of faces uses; tests/test_normals.py holds the layouts to the header
from .normals_abi import NORMALS_AREA, NORMALS_OFF, NormalsInfo, NormalsOpts, normal_mask_from_faces  # noqa: F401
# mcpt_get_visibility_info's struct and the mask that hides a set of materials' faces; tests/test_visibility.py holds the layout to the header
from .visibility_abi import VisibilityInfo, visibility_from_materials  # noqa: F401
# mcpt_set_camera_model's struct, mcpt_get_camera_model's info and the model constants; tests/test_camera_ref.py holds the layouts to the header
from .camera_abi import (CAMERA_EQUIRECT, CAMERA_MAX_BLADES, CAMERA_ORTHOGRAPHIC, CAMERA_PINHOLE, CAMERA_THIN_LENS, CameraModel, CameraModelInfo,  # noqa: F401
                         camera_model)
# mcpt_bake_point, mcpt_get_bake_info's struct, the constants, the makers of bake-point lists and Renderer's baking methods; tests/test_bake_ref.py holds the layouts to the header
from .bake_abi import (BAKE_BACK_SIDE, BAKE_DIFFUSE, BAKE_DIRECT_MIS, BAKE_DIRECT_OFF, BAKE_IRRADIANCE, BAKE_MAX_POINTS, BakeInfo, BakeMethods, BakePoint, bake_points, lightmap_points,  # noqa: F401
                       vertex_bake_points)
# mcpt_get_sh_info's struct, the constants, the host-only helpers and Renderer's light-probe methods; tests/test_shprobe_ref.py holds the layout to the header
from .shprobe_abi import SH_DIRECTIONS, SH_IRRADIANCE, SH_MAX_PROBES, SH_RADIANCE, ShInfo, ShProbeMethods, sh_eval, sh_grid  # noqa: F401

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libmcpt_hip.so")

MCPT_OK = 0
INTEGRATOR_MIS = 0
INTEGRATOR_RECURSIVE_NEE = 1
FLAG_CORRECT_SHADOW_T2 = 0x1
FLAG_DETERMINISTIC = 0x2
FLAG_COUNT_TRAVERSAL = 0x4
FLAG_GPU_BVH_BUILD = 0x8
FLAG_REFERENCE_TIE_ORDER = 0x10
FLAG_DYNAMIC = 0x20
DENOISE_SPLIT_EMISSION = 0x1          # mcpt_denoise_opts::flags
DENOISE_CLAMP_FIREFLIES = 0x2


class Texture(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("rgb", C.POINTER(C.c_float))]


class MaterialC(C.Structure):
    _fields_ = [("ks", C.c_double * 3), ("ns", C.c_double), ("radiance", C.c_double * 3),
                ("map_kd", C.c_int32), ("reserved", C.c_int32)]


class CameraC(C.Structure):
    _fields_ = [("eye", C.c_double * 3), ("lookat", C.c_double * 3), ("up", C.c_double * 3),
                ("fovy", C.c_double), ("width", C.c_int32), ("height", C.c_int32)]


class SceneDesc(C.Structure):
    _fields_ = [("vertex", C.POINTER(C.c_double)), ("n_vertex", C.c_uint32),
                ("normal", C.POINTER(C.c_double)), ("n_normal", C.c_uint32),
                ("texcoord", C.POINTER(C.c_double)), ("n_texcoord", C.c_uint32),
                ("face", C.POINTER(C.c_int32)), ("n_face", C.c_uint32),
                ("materials", C.POINTER(MaterialC)), ("n_materials", C.c_uint32),
                ("textures", C.POINTER(Texture)), ("n_textures", C.c_uint32),
                ("camera", CameraC)]


class Opts(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("device", C.c_int32), ("max_depth", C.c_uint32),
                ("integrator", C.c_uint32), ("flags", C.c_uint32), ("samples_per_item", C.c_uint32),
                ("reserved", C.c_uint32 * 4)]


class Counters(C.Structure):
    _fields_ = [("paths", C.c_uint64), ("rays_primary", C.c_uint64), ("rays_continuation", C.c_uint64),
                ("rays_shadow", C.c_uint64), ("box_tests", C.c_uint64), ("tri_tests", C.c_uint64),
                ("shaded_hits", C.c_uint64), ("texel_fetches", C.c_uint64),
                ("self_shadow_tests", C.c_uint64), ("self_shadow_hits", C.c_uint64),
                ("kernel_ms", C.c_double), ("kernel_ms_total", C.c_double), ("launches", C.c_uint64),
                ("trace_ms_total", C.c_double), ("shade_ms_total", C.c_double), ("iterations", C.c_uint64),
                ("stack_spills", C.c_uint64), ("debug", C.c_uint64 * 4)]

    @property
    def rays(self) -> int:
        return int(self.rays_primary + self.rays_continuation + self.rays_shadow)

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class SceneInfo(C.Structure):
    _fields_ = [("n_tris", C.c_uint32), ("n_lights", C.c_uint32), ("n_nodes", C.c_uint32),
                ("bvh_depth", C.c_uint32), ("max_leaf", C.c_uint32), ("width", C.c_uint32),
                ("height", C.c_uint32), ("device_bytes", C.c_uint64), ("bvh_build_ms", C.c_double),
                ("upload_ms", C.c_double), ("wide_width", C.c_uint32), ("wide_nodes", C.c_uint32), ("wide_depth", C.c_uint32),
                ("bvh_builder", C.c_uint32), ("traversal_bytes", C.c_uint64), ("centre", C.c_double * 3), ("wide_tree_hash", C.c_uint64)]


class DenoiseOpts(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("iterations", C.c_uint32), ("sigma_color", C.c_float),
                ("sigma_normal", C.c_float), ("sigma_depth", C.c_float), ("flags", C.c_uint32), ("firefly_clamp", C.c_float),
                ("reserved", C.c_uint32 * 1)]


class AdaptiveOpts(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("min_spp", C.c_uint32), ("max_spp", C.c_uint32), ("threshold", C.c_float),
                ("reserved", C.c_uint32 * 4)]


class AdaptiveStats(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("passes", C.c_uint32), ("pixel_samples", C.c_uint64),
                ("tiles_converged", C.c_uint32), ("tiles_capped", C.c_uint32), ("reserved", C.c_uint32 * 4)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved"}


class UpdateInfo(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("updates", C.c_uint32), ("last_update_ms", C.c_double),
                ("wide_area_ratio", C.c_double), ("reserved", C.c_uint32 * 4)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved"}


class ReprojectOpts(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("feature_spp", C.c_uint32), ("feature_seed", C.c_uint64), ("max_history", C.c_float),
                ("depth_tolerance", C.c_float), ("normal_threshold", C.c_float), ("reserved", C.c_uint32 * 3)]


class ReprojectInfo(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("reprojections", C.c_uint32), ("pixels_reused", C.c_uint64), ("last_ms", C.c_double),
                ("reserved", C.c_uint32 * 4)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved"}


class MaterialInfo(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("updates", C.c_uint32), ("n_lights", C.c_uint32), ("reserved0", C.c_uint32), ("last_ms", C.c_double),
                ("reserved", C.c_uint32 * 4)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if not k.startswith("reserved")}


class TransformInfo(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("n_groups", C.c_uint32), ("updates", C.c_uint32), ("reserved0", C.c_uint32), ("last_ms", C.c_double),
                ("reserved", C.c_uint32 * 4)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if not k.startswith("reserved")}


def texture_to_float(img_u8: np.ndarray) -> np.ndarray:
    """What stbi_loadf gives the reference for an 8-bit image (model.cpp:8-23; stb_image.h:1553,1849):
    (c/255)^2.2 per channel, row 0 = first row of the file."""
    x = img_u8.astype(np.float32) / np.float32(255.0)
    return np.power(x, np.float32(2.2)).astype(np.float32)


def material_texels(m: "scenes.Material") -> np.ndarray:
    """The (h, w, 3) fp32 texels mcpt_create gets for a scenes.Material: its image, or its constant Kd as a 1x1 texture."""
    if m.texture is not None and m.texture.dtype == np.float32:
        return np.ascontiguousarray(m.texture)                    # already what stbi_loadf would return (tests feed reference texels)
    if m.texture is not None:
        return np.ascontiguousarray(texture_to_float(m.texture))
    return np.asarray(m.kd, np.float32).reshape(1, 1, 3).copy()   # Texture(Color3f kd): kd parsed with stof (model.cpp:189-193)


def _materials_c(materials, map_kd=None):
    out = (MaterialC * len(materials))()
    for i, m in enumerate(materials):
        mc = out[i]
        for k in range(3):
            mc.ks[k] = float(m.ks[k]); mc.radiance[k] = float(m.radiance[k])
        mc.ns = float(m.ns)
        mc.map_kd = i if map_kd is None else int(map_kd[i])
    return out


class DescHolder:
    """Builds an mcpt_scene_desc from a scenes.SceneData and keeps the backing arrays alive."""

    def __init__(self, scene: "scenes.SceneData"):
        self.vertex = np.ascontiguousarray(scene.vertex, np.float64)
        self.normal = np.ascontiguousarray(scene.normal, np.float64)
        self.texcoord = np.ascontiguousarray(scene.texcoord, np.float64)
        self.face = np.ascontiguousarray(scene.face, np.int32)
        self.tex_arrays = []
        n = len(scene.materials)
        self.materials = _materials_c(scene.materials)
        self.textures = (Texture * n)()
        for i, m in enumerate(scene.materials):
            t = material_texels(m)
            self.tex_arrays.append(t)
            self.textures[i].width = t.shape[1]
            self.textures[i].height = t.shape[0]
            self.textures[i].rgb = t.ctypes.data_as(C.POINTER(C.c_float))
        d = SceneDesc()
        d.vertex = self.vertex.ctypes.data_as(C.POINTER(C.c_double)); d.n_vertex = self.vertex.shape[0]
        d.normal = self.normal.ctypes.data_as(C.POINTER(C.c_double)); d.n_normal = self.normal.shape[0]
        d.texcoord = self.texcoord.ctypes.data_as(C.POINTER(C.c_double)); d.n_texcoord = self.texcoord.shape[0]
        d.face = self.face.ctypes.data_as(C.POINTER(C.c_int32)); d.n_face = self.face.shape[0]
        d.materials = C.cast(self.materials, C.POINTER(MaterialC)); d.n_materials = n
        d.textures = C.cast(self.textures, C.POINTER(Texture)); d.n_textures = n
        cam = scene.camera
        for k in range(3):
            d.camera.eye[k] = cam.eye[k]; d.camera.lookat[k] = cam.lookat[k]; d.camera.up[k] = cam.up[k]
        d.camera.fovy = cam.fovy; d.camera.width = cam.width; d.camera.height = cam.height
        self.desc = d


_lib = None


def load_library() -> C.CDLL:
    """Load csrc/libmcpt_hip.so.  Raises if it has not been built -- there is nothing to fall back to."""
    global _lib
    if _lib is not None:
        return _lib
    try:          # torch bundles its own libamdhip64: let it load first so both sides share one HIP runtime in this process
        import torch  # noqa: F401
    except Exception:
        pass
    path = os.environ.get("MCPT_LIB_PATH", LIB_PATH)     # developer override: A/B another build of the same ABI
    if not os.path.exists(path):
        raise RuntimeError("libmcpt_hip.so not built (%s): run `python -c 'import __graft_entry__ as g; g.build()'` "
                           "or `make -C monte-carlo-path-tracer_amd/csrc`.  No CPU fallback exists." % path)
    lib = C.CDLL(path)
    P = C.POINTER
    vp = C.c_void_p
    sigs = {
        "mcpt_create": [P(SceneDesc), P(Opts), P(vp)],
        "mcpt_destroy": [vp],
        "mcpt_check_scene": [P(SceneDesc), P(SceneInfo)],
        "mcpt_get_scene_info": [vp, P(SceneInfo)],
        "mcpt_render": [vp, C.c_uint32, C.c_uint64, C.c_uint32],
        "mcpt_render_tiles": [vp, C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32],
        "mcpt_sync": [vp],
        "mcpt_read_accum": [vp, vp],
        "mcpt_write_accum": [vp, vp],
        "mcpt_clear_accum": [vp],
        "mcpt_tonemap": [vp, vp, C.c_int],
        "mcpt_get_counters": [vp, P(Counters)],
        "mcpt_reset_counters": [vp],
        "mcpt_bind_accum": [vp, vp],
        "mcpt_clone_to_device": [vp, C.c_int32, P(vp)],
        "mcpt_tonemap_buffer": [vp, vp, vp, C.c_int],
        "mcpt_tonemap_map": [vp, C.c_int, C.POINTER(C.c_void_p)],
        "mcpt_accum_device_ptr": [vp, P(vp)],
        "mcpt_set_stream": [vp, vp],
        "mcpt_set_null_stream": [vp],
        "mcpt_probe_trace4": [vp, C.c_uint32, vp, vp, vp, C.c_int, vp, vp, vp, vp],
        "mcpt_probe_trace": [vp, C.c_uint32, vp, vp, vp, vp, C.c_int, vp, vp, vp, vp],
        "mcpt_probe_cast_ray": [vp, C.c_uint32, vp, vp, vp],
        "mcpt_probe_hit_shade": [vp, C.c_uint32, vp, vp, vp, vp, vp],
        "mcpt_probe_bsdf": [vp, C.c_uint32, vp, vp, vp, vp, vp, vp, vp, vp],
        "mcpt_probe_sample_light": [vp, C.c_uint32, vp, vp, vp],
        "mcpt_probe_paths": [vp, C.c_uint32, vp, vp, C.c_uint64, vp],
        "mcpt_probe_rng": [vp, C.c_uint32, vp, C.c_uint64, vp],
        "mcpt_probe_texture": [vp, C.c_uint32, C.c_uint32, vp, vp],
        "mcpt_render_features": [vp, C.c_uint32, C.c_uint64],
        "mcpt_read_features": [vp, vp],
        "mcpt_denoise": [vp, vp, P(DenoiseOpts)],
        "mcpt_probe_denoise": [vp, vp, vp, vp, P(DenoiseOpts), vp],
        "mcpt_read_denoised": [vp, vp],
        "mcpt_denoised_device_ptr": [vp, P(vp)],
        "mcpt_read_emission": [vp, vp],
        "mcpt_render_tile_list": [vp, C.c_uint32, C.c_uint64, C.c_uint32, vp, C.c_uint32],
        "mcpt_render_adaptive": [vp, C.c_uint64, C.c_uint32, P(AdaptiveOpts), P(AdaptiveStats)],
        "mcpt_read_tile_error": [vp, vp],
        "mcpt_probe_tile_error": [vp, vp, vp, C.c_float, C.c_uint32, vp, vp, P(C.c_uint32)],
        "mcpt_set_camera": [vp, P(CameraC)],
        "mcpt_update_vertices": [vp, vp, C.c_uint32, vp, C.c_uint32],
        "mcpt_get_update_info": [vp, P(UpdateInfo)],
        "mcpt_probe_validate_trees": [vp],
        "mcpt_set_camera_reproject": [vp, P(CameraC), P(ReprojectOpts)],
        "mcpt_get_reproject_info": [vp, P(ReprojectInfo)],
        "mcpt_probe_reproject": [vp, P(CameraC), P(CameraC), vp, vp, vp, P(ReprojectOpts), vp, P(C.c_uint64)],
        "mcpt_update_vertices_reproject": [vp, vp, C.c_uint32, vp, C.c_uint32, P(CameraC), P(ReprojectOpts)],
        "mcpt_probe_first_hits": [vp, vp, vp],
        "mcpt_probe_reproject_motion": [vp, P(CameraC), P(CameraC), vp, vp, vp, vp, vp, vp, vp, P(ReprojectOpts), vp, P(C.c_uint64)],
        "mcpt_update_materials": [vp, P(MaterialC), C.c_uint32],
        "mcpt_update_texture": [vp, C.c_uint32, P(Texture)],
        "mcpt_get_material_info": [vp, P(MaterialInfo)],
        "mcpt_probe_lights": [vp, C.c_uint32, vp, vp, vp, P(C.c_uint32)],
        "mcpt_probe_face_classes": [vp, vp],
        "mcpt_set_vertex_groups": [vp, vp, C.c_uint32, vp, C.c_uint32, C.c_uint32],
        "mcpt_update_transforms": [vp, vp, C.c_uint32],
        "mcpt_update_transforms_reproject": [vp, vp, C.c_uint32, P(CameraC), P(ReprojectOpts)],
        "mcpt_get_transform_info": [vp, P(TransformInfo)],
        "mcpt_set_vertex_skin": [vp, vp, vp, C.c_uint32, vp, vp, C.c_uint32, C.c_uint32],
        "mcpt_update_skin": [vp, vp, C.c_uint32],
        "mcpt_update_skin_reproject": [vp, vp, C.c_uint32, P(CameraC), P(ReprojectOpts)],
        "mcpt_get_skin_info": [vp, P(SkinInfo)],
        "mcpt_set_skin_mode": [vp, C.c_uint32],
        "mcpt_get_skin_mode": [vp, P(C.c_uint32)],
        "mcpt_set_vertex_morph": [vp, P(MorphTargets), C.c_uint32, P(MorphTargets), C.c_uint32],
        "mcpt_update_morph": [vp, vp, C.c_uint32, vp, C.c_uint32],
        "mcpt_update_morph_reproject": [vp, vp, C.c_uint32, vp, C.c_uint32, P(CameraC), P(ReprojectOpts)],
        "mcpt_get_morph_info": [vp, P(MorphInfo)],
        "mcpt_probe_vertices": [vp, vp, vp],
        "mcpt_set_vertex_keyframes": [vp, vp, C.c_uint32, vp, C.c_uint32, C.c_uint32, P(KeyframeOpts)],
        "mcpt_update_keyframes": [vp, C.c_double],
        "mcpt_update_keyframes_reproject": [vp, C.c_double, P(CameraC), P(ReprojectOpts)],
        "mcpt_get_keyframe_info": [vp, P(KeyframeInfo)],
        "mcpt_set_vertex_owners": [vp, vp, C.c_uint32, vp, C.c_uint32],
        "mcpt_update_parts": [vp, P(SceneUpdate)],
        "mcpt_update_parts_reproject": [vp, P(SceneUpdate), P(CameraC), P(ReprojectOpts)],
        "mcpt_get_parts_info": [vp, P(PartsInfo)],
        "mcpt_set_auto_normals": [vp, vp, C.c_uint32, P(NormalsOpts)],
        "mcpt_update_normals": [vp],
        "mcpt_get_normals_info": [vp, P(NormalsInfo)],
        "mcpt_rebuild_trees": [vp, P(RebuildOpts)],
        "mcpt_get_rebuild_info": [vp, P(RebuildInfo)],
        "mcpt_set_face_visibility": [vp, vp, C.c_uint32],
        "mcpt_set_face_visibility_reproject": [vp, vp, C.c_uint32, P(CameraC), P(ReprojectOpts)],
        "mcpt_get_visibility_info": [vp, P(VisibilityInfo)],
        "mcpt_probe_triangles": [vp, vp, vp],
        "mcpt_set_camera_model": [vp, P(CameraModel)],
        "mcpt_get_camera_model": [vp, P(CameraModel), P(CameraModelInfo)],
        "mcpt_render_camera": [vp, C.c_uint32, C.c_uint64, C.c_uint32],
        "mcpt_autofocus": [vp, C.c_int32, C.c_int32, P(C.c_double)],
        "mcpt_probe_camera_rays": [vp, C.c_uint32, vp, C.c_uint32, C.c_uint64, vp, vp],
        "mcpt_set_bake_points": [vp, vp, C.c_uint32],
        "mcpt_bake": [vp, C.c_uint32, C.c_uint64, C.c_uint32],
        "mcpt_clear_bake": [vp],
        "mcpt_read_bake": [vp, C.c_uint32, vp],
        "mcpt_read_bake_film": [vp, vp],
        "mcpt_get_bake_info": [vp, P(BakeInfo)],
        "mcpt_probe_bake_rays": [vp, C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint32, vp, vp, vp, vp],
        "mcpt_lightmap_points": [P(SceneDesc), C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, P(C.c_uint32)],
        "mcpt_set_bake_direct": [vp, C.c_uint32],
        "mcpt_probe_bake_direct": [vp, C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint32, vp, vp],
        "mcpt_set_sh_probes": [vp, vp, C.c_uint32],
        "mcpt_bake_sh": [vp, C.c_uint32, C.c_uint64, C.c_uint32],
        "mcpt_clear_sh": [vp],
        "mcpt_read_sh": [vp, C.c_uint32, vp],
        "mcpt_read_sh_film": [vp, vp, vp],
        "mcpt_get_sh_info": [vp, P(ShInfo)],
        "mcpt_probe_sh_rays": [vp, C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint32, vp, vp],
        "mcpt_read_sh_pass": [vp, vp, vp],
        "mcpt_sh_grid": [vp, vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, vp, P(C.c_uint32)],
        "mcpt_sh_eval": [vp, vp, vp],
    }
    for name, args in sigs.items():
        if not hasattr(lib, name) and "MCPT_LIB_PATH" in os.environ:
            continue                                     # developer A/B against an older build of the library
        fn = getattr(lib, name)
        fn.argtypes = args
        fn.restype = C.c_int
    lib.mcpt_last_error.restype = C.c_char_p
    lib.mcpt_abi_version.restype = C.c_uint32
    _lib = lib
    return lib


EXPORTED_SYMBOLS = [
    "mcpt_create", "mcpt_destroy", "mcpt_clone_to_device", "mcpt_tonemap_buffer", "mcpt_check_scene", "mcpt_get_scene_info", "mcpt_last_error", "mcpt_abi_version",
    "mcpt_render", "mcpt_render_tiles", "mcpt_sync", "mcpt_read_accum", "mcpt_write_accum", "mcpt_clear_accum", "mcpt_tonemap", "mcpt_tonemap_map",
    "mcpt_get_counters", "mcpt_reset_counters", "mcpt_bind_accum", "mcpt_accum_device_ptr", "mcpt_set_stream",
    "mcpt_set_null_stream", "mcpt_probe_trace", "mcpt_probe_trace4", "mcpt_probe_cast_ray", "mcpt_probe_hit_shade", "mcpt_probe_bsdf", "mcpt_probe_sample_light",
    "mcpt_probe_paths", "mcpt_probe_rng", "mcpt_probe_texture",
    "mcpt_render_features", "mcpt_read_features", "mcpt_denoise", "mcpt_read_denoised", "mcpt_denoised_device_ptr", "mcpt_read_emission",
    "mcpt_probe_denoise",
    "mcpt_render_tile_list", "mcpt_render_adaptive", "mcpt_read_tile_error", "mcpt_probe_tile_error",
    "mcpt_set_camera", "mcpt_update_vertices", "mcpt_get_update_info", "mcpt_probe_validate_trees",
    "mcpt_set_camera_reproject", "mcpt_get_reproject_info", "mcpt_probe_reproject",
    "mcpt_update_vertices_reproject", "mcpt_probe_first_hits", "mcpt_probe_reproject_motion",
    "mcpt_update_materials", "mcpt_update_texture", "mcpt_get_material_info", "mcpt_probe_lights", "mcpt_probe_face_classes",
    "mcpt_set_vertex_groups", "mcpt_update_transforms", "mcpt_update_transforms_reproject", "mcpt_get_transform_info",
    "mcpt_set_vertex_skin", "mcpt_update_skin", "mcpt_update_skin_reproject", "mcpt_get_skin_info",
    "mcpt_set_skin_mode", "mcpt_get_skin_mode",
    "mcpt_set_vertex_morph", "mcpt_update_morph", "mcpt_update_morph_reproject", "mcpt_get_morph_info", "mcpt_probe_vertices",
    "mcpt_set_vertex_keyframes", "mcpt_update_keyframes", "mcpt_update_keyframes_reproject", "mcpt_get_keyframe_info",
    "mcpt_set_vertex_owners", "mcpt_update_parts", "mcpt_update_parts_reproject", "mcpt_get_parts_info",
    "mcpt_set_auto_normals", "mcpt_update_normals", "mcpt_get_normals_info",
    "mcpt_rebuild_trees", "mcpt_get_rebuild_info",
    "mcpt_set_face_visibility", "mcpt_set_face_visibility_reproject", "mcpt_get_visibility_info", "mcpt_probe_triangles",
    "mcpt_set_camera_model", "mcpt_get_camera_model", "mcpt_render_camera", "mcpt_autofocus", "mcpt_probe_camera_rays",
    "mcpt_set_bake_points", "mcpt_bake", "mcpt_clear_bake", "mcpt_read_bake", "mcpt_read_bake_film", "mcpt_get_bake_info", "mcpt_probe_bake_rays", "mcpt_lightmap_points",
    "mcpt_set_bake_direct", "mcpt_probe_bake_direct",
    "mcpt_set_sh_probes", "mcpt_bake_sh", "mcpt_clear_sh", "mcpt_read_sh", "mcpt_read_sh_film", "mcpt_get_sh_info", "mcpt_probe_sh_rays", "mcpt_read_sh_pass", "mcpt_sh_grid",
    "mcpt_sh_eval",
]


class McptError(RuntimeError):
    pass


def _camera_c(camera) -> CameraC:
    c = CameraC()
    for k in range(3):
        c.eye[k] = camera.eye[k]; c.lookat[k] = camera.lookat[k]; c.up[k] = camera.up[k]
    c.fovy = camera.fovy; c.width = camera.width; c.height = camera.height
    return c


def _reproject_opts(feature_spp=0, feature_seed=0, max_history=0.0, depth_tolerance=0.0, normal_threshold=0.0) -> ReprojectOpts:
    o = ReprojectOpts()
    o.struct_size = C.sizeof(ReprojectOpts); o.feature_spp = feature_spp; o.feature_seed = feature_seed
    o.max_history = max_history; o.depth_tolerance = depth_tolerance; o.normal_threshold = normal_threshold
    return o


def _denoise_opts(iterations, sigma_color, sigma_normal, sigma_depth, split_emission, clamp_fireflies, firefly_clamp) -> DenoiseOpts:
    o = DenoiseOpts()
    o.struct_size = C.sizeof(DenoiseOpts); o.iterations = iterations
    o.sigma_color = sigma_color; o.sigma_normal = sigma_normal; o.sigma_depth = sigma_depth
    o.flags = (DENOISE_SPLIT_EMISSION if split_emission else 0) | (DENOISE_CLAMP_FIREFLIES if clamp_fireflies else 0)
    o.firefly_clamp = firefly_clamp
    return o


def _camera_and_opts(camera, opts):
    """The last two arguments of an update_*_reproject call: the camera (None: the view stays) and reproject_camera's options, both by reference."""
    return None if camera is None else C.byref(_camera_c(camera)), C.byref(_reproject_opts(**opts))


def _ptr(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def groups_from_faces(scene: "scenes.SceneData", face_group):
    """Per-vertex and per-normal group ids (two uint32 arrays, for Renderer.set_vertex_groups) from one id per face: a vertex or normal takes
    the group of the faces that use it, one no face uses gets group 0.  Raises ValueError when faces of two groups share a vertex or a normal --
    the caller duplicates it then."""
    fg = np.ascontiguousarray(face_group, np.int64).reshape(-1)
    if fg.shape[0] != scene.face.shape[0] or (fg.size and fg.min() < 0):
        raise ValueError("groups_from_faces: need one group id >= 0 per face")
    out = []
    for what, col, n in (("vertex", 0, scene.vertex.shape[0]), ("normal", 1, scene.normal.shape[0])):
        idx = scene.face[:, :, col].astype(np.int64).reshape(-1); g = np.repeat(fg, 3)
        lo = np.full(n, np.iinfo(np.int64).max, np.int64); hi = np.full(n, -1, np.int64)
        np.minimum.at(lo, idx, g); np.maximum.at(hi, idx, g)
        shared = np.flatnonzero((hi >= 0) & (lo != hi))
        if shared.size:
            raise ValueError("groups_from_faces: %s %d is used by faces of groups %d and %d" % (what, shared[0], lo[shared[0]], hi[shared[0]]))
        out.append(np.where(hi >= 0, hi, 0).astype(np.uint32))
    return out[0], out[1]


def skin_normals_from_faces(scene: "scenes.SceneData", vertex_bone, vertex_weight):
    """Per-normal bone ids and weights ((n_normal, 4) uint32 and float64, for Renderer.set_vertex_skin) from the per-vertex ones: a normal takes
    the influences of the vertex it is paired with in a face corner, one no face uses gets bone 0 with weight 1.  Raises ValueError naming the
    normal when two corners pair it with vertices whose influence records differ -- the caller duplicates it then."""
    nv, nn = scene.vertex.shape[0], scene.normal.shape[0]
    vb = np.ascontiguousarray(vertex_bone, np.uint32).reshape(-1, SKIN_INFLUENCES); vw = np.ascontiguousarray(vertex_weight, np.float64).reshape(-1, SKIN_INFLUENCES)
    if vb.shape[0] != nv or vw.shape[0] != nv:
        raise ValueError("skin_normals_from_faces: need %d bone ids and weights per vertex" % SKIN_INFLUENCES)
    vi = scene.face[:, :, 0].astype(np.int64).reshape(-1); ni = scene.face[:, :, 1].astype(np.int64).reshape(-1)
    first = np.full(nn, -1, np.int64)
    first[ni[::-1]] = vi[::-1]                                    # per normal the vertex of its first corner
    mine = first[ni]
    differ = np.any(vb[vi] != vb[mine], axis=1) | np.any(vw[vi].view(np.uint64) != vw[mine].view(np.uint64), axis=1)
    if differ.any():
        k = int(np.flatnonzero(differ)[0])
        raise ValueError("skin_normals_from_faces: normal %d is paired with vertices %d and %d, whose influences differ" % (ni[k], mine[k], vi[k]))
    nb = np.zeros((nn, SKIN_INFLUENCES), np.uint32); nw = np.zeros((nn, SKIN_INFLUENCES), np.float64); nw[:, 0] = 1.0
    used = first >= 0
    nb[used] = vb[first[used]]; nw[used] = vw[first[used]]
    return nb, nw


def check_scene(scene: "scenes.SceneData"):
    """Host-only validation + BVH build (no device needed).  Returns (status, SceneInfo, message)."""
    lib = load_library()
    holder = DescHolder(scene)
    info = SceneInfo()
    st = lib.mcpt_check_scene(C.byref(holder.desc), C.byref(info))
    return st, info, (lib.mcpt_last_error() or b"").decode() if st != MCPT_OK else ""


class Renderer(BakeMethods, ShProbeMethods):
    """One mcpt_ctx = one scene on one GPU (the reference's ``Render`` object).  Surface baking: bake_abi.BakeMethods; light
    probes: shprobe_abi.ShProbeMethods."""

    def __init__(self, scene: "scenes.SceneData", max_depth=0, integrator=INTEGRATOR_MIS, flags=0, device=0,
                 samples_per_item=0):
        self.lib = load_library()
        self.holder = DescHolder(scene)
        self.tex_arrays = list(self.holder.tex_arrays)            # the texels the context holds now (update_materials / update_texture replace entries)
        self.width, self.height = scene.camera.width, scene.camera.height
        o = Opts()
        o.struct_size = C.sizeof(Opts); o.device = device; o.max_depth = max_depth
        o.integrator = integrator; o.flags = flags; o.samples_per_item = samples_per_item
        self.ctx = C.c_void_p()
        self._check(self.lib.mcpt_create(C.byref(self.holder.desc), C.byref(o), C.byref(self.ctx)))

    def clone(self, device=0) -> "Renderer":
        """A second Renderer for the same scene (mcpt_clone_to_device): no flatten, no BVH build."""
        other = Renderer.__new__(Renderer)
        other.lib = self.lib; other.holder = self.holder; other.width, other.height = self.width, self.height
        other.tex_arrays = list(self.tex_arrays)
        other.ctx = C.c_void_p()
        self._check(self.lib.mcpt_clone_to_device(self.ctx, int(device), C.byref(other.ctx)))
        return other

    def _check(self, status):
        if status != MCPT_OK:
            raise McptError("mcpt status %d: %s" % (status, (self.lib.mcpt_last_error() or b"").decode()))

    def close(self):
        if getattr(self, "ctx", None) is not None and self.ctx.value:
            self.lib.mcpt_destroy(self.ctx)
            self.ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- hot path
    def render(self, spp: int, seed: int = 0, first_sample: int = 0):
        self._check(self.lib.mcpt_render(self.ctx, spp, seed, first_sample))

    def render_tiles(self, spp: int, seed: int, first_sample: int, tile_mod: int, tile_rem: int):
        """One interleaved share of the image: the 8x8 tiles t with t % tile_mod == tile_rem."""
        self._check(self.lib.mcpt_render_tiles(self.ctx, spp, seed, first_sample, tile_mod, tile_rem))

    def render_tile_list(self, spp: int, seed: int, first_sample: int, tiles):
        """The 8x8 tiles in `tiles` (row-major tile numbers, distinct, any order) only."""
        t = np.ascontiguousarray(tiles, np.uint32).reshape(-1)
        self._check(self.lib.mcpt_render_tile_list(self.ctx, spp, seed, first_sample, _ptr(t), t.size))

    @property
    def tiles_shape(self):
        return (self.height + 7) // 8, (self.width + 7) // 8

    def render_adaptive(self, seed: int = 0, first_sample: int = 0, min_spp: int = 0, max_spp: int = 0, threshold: float = 0.0) -> AdaptiveStats:
        """Adaptive sampling per 8x8 tile; 0 = the default of each option.  Adds to the film."""
        o = AdaptiveOpts()
        o.struct_size = C.sizeof(AdaptiveOpts); o.min_spp = min_spp; o.max_spp = max_spp; o.threshold = threshold
        st = AdaptiveStats()
        st.struct_size = C.sizeof(AdaptiveStats)
        self._check(self.lib.mcpt_render_adaptive(self.ctx, seed, first_sample, C.byref(o), C.byref(st)))
        return st

    def tile_error(self) -> np.ndarray:
        """(tiles_y, tiles_x) E_t of the last pass of the last render_adaptive call."""
        out = np.zeros(self.tiles_shape, np.float32)
        self._check(self.lib.mcpt_read_tile_error(self.ctx, _ptr(out)))
        return out

    def probe_tile_error(self, h: np.ndarray, o: np.ndarray, threshold: float, max_spp: int):
        """The error + compaction kernels on two caller films: ((tiles_y, tiles_x) E_t, active tile list in ascending order)."""
        a = np.ascontiguousarray(h, np.float32); b = np.ascontiguousarray(o, np.float32)
        assert a.size == b.size == self.width * self.height * 4
        err = np.zeros(self.tiles_shape, np.float32)
        lst = np.zeros(err.size, np.uint32)
        n = C.c_uint32(0)
        self._check(self.lib.mcpt_probe_tile_error(self.ctx, _ptr(a), _ptr(b), threshold, max_spp, _ptr(err), _ptr(lst), C.byref(n)))
        return err, lst[:n.value].copy()

    # ---- live scenes
    def set_camera(self, camera):
        """A new camera (scenes.Camera) for the same film size; free.  The caller clears the film when the old samples no longer belong."""
        c = _camera_c(camera)
        self._check(self.lib.mcpt_set_camera(self.ctx, C.byref(c)))

    # ---- temporal reprojection
    def reproject_camera(self, camera, feature_spp=0, feature_seed=0, max_history=0.0, depth_tolerance=0.0, normal_threshold=0.0):
        """set_camera that carries the film over: the bound film becomes the old film looked up at the new view's surface points, at most
        max_history samples per pixel (0 = the default of each option).  Asynchronous.  Afterwards the context holds the new view's features."""
        c = _camera_c(camera)
        o = _reproject_opts(feature_spp, feature_seed, max_history, depth_tolerance, normal_threshold)
        self._check(self.lib.mcpt_set_camera_reproject(self.ctx, C.byref(c), C.byref(o)))

    def reproject_info(self) -> ReprojectInfo:
        i = ReprojectInfo()
        self._check(self.lib.mcpt_get_reproject_info(self.ctx, C.byref(i)))
        return i

    def probe_reproject(self, old_camera, new_camera, old_film, old_feat, new_feat, max_history=0.0, depth_tolerance=0.0, normal_threshold=0.0):
        """The reprojection kernel alone on caller data of this context's film size: ((h, w, 4) film, pixels reused)."""
        a = np.ascontiguousarray(old_film, np.float32); fo = np.ascontiguousarray(old_feat, np.float32); fn = np.ascontiguousarray(new_feat, np.float32)
        n = self.width * self.height
        assert a.size == 4 * n and fo.size == 8 * n and fn.size == 8 * n
        co, cn = _camera_c(old_camera), _camera_c(new_camera)
        o = _reproject_opts(0, 0, max_history, depth_tolerance, normal_threshold)
        out = np.zeros((self.height, self.width, 4), np.float32)
        reused = C.c_uint64(0)
        self._check(self.lib.mcpt_probe_reproject(self.ctx, C.byref(co), C.byref(cn), _ptr(a), _ptr(fo), _ptr(fn), C.byref(o), _ptr(out), C.byref(reused)))
        return out, int(reused.value)

    # ---- motion-vector reprojection
    def update_vertices_reproject(self, vertex, normal=None, camera=None, **opts):
        """update_vertices that carries the film over (optionally with a camera move in the same call): the bound film becomes the old film looked
        up where the new view's surface points were before the update.  opts: reproject_camera's.  Needs FLAG_DYNAMIC.  Asynchronous."""
        v = np.ascontiguousarray(vertex, np.float64).reshape(-1, 3)
        n = None if normal is None else np.ascontiguousarray(normal, np.float64).reshape(-1, 3)
        c, o = _camera_and_opts(camera, opts)
        self._check(self.lib.mcpt_update_vertices_reproject(self.ctx, _ptr(v), v.shape[0], _ptr(n), 0 if n is None else n.shape[0], c, o))

    def probe_first_hits(self):
        """The first-hit kernel on the current scene and camera: ((h, w) face, -1 = miss; (h, w, 3) {u, v, t})."""
        face = np.zeros((self.height, self.width), np.int32); uvt = np.zeros((self.height, self.width, 3), np.float32)
        self._check(self.lib.mcpt_probe_first_hits(self.ctx, _ptr(face), _ptr(uvt)))
        return face, uvt

    def probe_reproject_motion(self, old_camera, new_camera, old_film, old_feat, new_feat, hit_face, hit_uv, old_vertex=None, old_normal=None,
                               max_history=0.0, depth_tolerance=0.0, normal_threshold=0.0):
        """The motion kernel alone on caller data of this context's film size: ((h, w, 4) film, pixels reused).  hit_face / hit_uv: per pixel
        of the new view a face (-1 = miss) and its (u, v); old_vertex / old_normal: None = the context's current arrays."""
        a = np.ascontiguousarray(old_film, np.float32); fo = np.ascontiguousarray(old_feat, np.float32); fn = np.ascontiguousarray(new_feat, np.float32)
        hf = np.ascontiguousarray(hit_face, np.int32); uv = np.ascontiguousarray(hit_uv, np.float32)
        n = self.width * self.height
        assert a.size == 4 * n and fo.size == 8 * n and fn.size == 8 * n and hf.size == n and uv.size == 2 * n
        info = self.holder
        ov = None if old_vertex is None else np.ascontiguousarray(old_vertex, np.float64).reshape(-1, 3)
        on = None if old_normal is None else np.ascontiguousarray(old_normal, np.float64).reshape(-1, 3)
        assert ov is None or ov.shape == info.vertex.shape
        assert on is None or on.shape == info.normal.shape
        co, cn = _camera_c(old_camera), _camera_c(new_camera)
        o = _reproject_opts(0, 0, max_history, depth_tolerance, normal_threshold)
        out = np.zeros((self.height, self.width, 4), np.float32)
        reused = C.c_uint64(0)
        self._check(self.lib.mcpt_probe_reproject_motion(self.ctx, C.byref(co), C.byref(cn), _ptr(ov), _ptr(on), _ptr(a), _ptr(fo), _ptr(fn), _ptr(hf), _ptr(uv),
                                                         C.byref(o), _ptr(out), C.byref(reused)))
        return out, int(reused.value)

    def update_vertices(self, vertex, normal=None):
        """New positions (and optionally normals) for the same faces: refits both trees on the device.  Needs FLAG_DYNAMIC."""
        v = np.ascontiguousarray(vertex, np.float64).reshape(-1, 3)
        n = None if normal is None else np.ascontiguousarray(normal, np.float64).reshape(-1, 3)
        self._check(self.lib.mcpt_update_vertices(self.ctx, _ptr(v), v.shape[0], _ptr(n), 0 if n is None else n.shape[0]))

    # ---- rigid parts moved by per-group transforms
    def set_vertex_groups(self, vertex_group, normal_group, n_groups: int):
        """A group id per vertex and per normal (groups_from_faces derives them from faces); the scene as it is now becomes the rest pose
        update_transforms moves.  Needs FLAG_DYNAMIC.  Synchronous."""
        vg = np.ascontiguousarray(vertex_group, np.uint32).reshape(-1); ng = np.ascontiguousarray(normal_group, np.uint32).reshape(-1)
        self._check(self.lib.mcpt_set_vertex_groups(self.ctx, _ptr(vg), vg.size, _ptr(ng) if ng.size else None, ng.size, int(n_groups)))

    @staticmethod
    def _matrices(matrices) -> np.ndarray:
        m = np.ascontiguousarray(matrices, np.float64)
        if m.size % 12:
            raise ValueError("need (n_groups, 3, 4) matrices")
        return m.reshape(-1, 3, 4)

    def update_transforms(self, matrices):
        """One row-major 3x4 matrix [A | t] per group, applied to the REST pose on the device (never accumulated), then update_vertices' refit:
        only the matrices cross the bus.  Asynchronous; the caller clears the film."""
        m = self._matrices(matrices)
        self._check(self.lib.mcpt_update_transforms(self.ctx, _ptr(m), m.shape[0]))

    def update_transforms_reproject(self, matrices, camera=None, **opts):
        """update_transforms that carries the film over, as update_vertices_reproject does; opts: reproject_camera's."""
        m = self._matrices(matrices)
        c, o = _camera_and_opts(camera, opts)
        self._check(self.lib.mcpt_update_transforms_reproject(self.ctx, _ptr(m), m.shape[0], c, o))

    def transform_info(self) -> TransformInfo:
        i = TransformInfo()
        self._check(self.lib.mcpt_get_transform_info(self.ctx, C.byref(i)))
        return i

    # ---- deforming parts: linear-blend skinning
    def set_vertex_skin(self, vertex_bone, vertex_weight, normal_bone, normal_weight, n_bones: int):
        """Four bone ids and weights per vertex and per normal (skin_normals_from_faces derives the normals' from the vertices'); the scene as it
        is now becomes the rest pose update_skin deforms.  Weights are used as given.  Needs FLAG_DYNAMIC.  Synchronous."""
        vb = np.ascontiguousarray(vertex_bone, np.uint32).reshape(-1, SKIN_INFLUENCES); vw = np.ascontiguousarray(vertex_weight, np.float64).reshape(-1, SKIN_INFLUENCES)
        nb = np.ascontiguousarray(normal_bone, np.uint32).reshape(-1, SKIN_INFLUENCES); nw = np.ascontiguousarray(normal_weight, np.float64).reshape(-1, SKIN_INFLUENCES)
        if vb.shape != vw.shape or nb.shape != nw.shape:
            raise ValueError("need as many weights as bone ids")
        self._check(self.lib.mcpt_set_vertex_skin(self.ctx, _ptr(vb), _ptr(vw), vb.shape[0], _ptr(nb) if nb.size else None, _ptr(nw) if nw.size else None,
                                                  nb.shape[0], int(n_bones)))

    def update_skin(self, matrices):
        """One row-major 3x4 matrix [A | t] per bone, blended per record by its four weights and applied to the skin's REST pose on the device
        (never accumulated), then update_vertices' refit: only the matrices cross the bus.  Asynchronous; the caller clears the film."""
        m = self._matrices(matrices)
        self._check(self.lib.mcpt_update_skin(self.ctx, _ptr(m), m.shape[0]))

    def update_skin_reproject(self, matrices, camera=None, **opts):
        """update_skin that carries the film over, as update_vertices_reproject does; opts: reproject_camera's."""
        m = self._matrices(matrices)
        c, o = _camera_and_opts(camera, opts)
        self._check(self.lib.mcpt_update_skin_reproject(self.ctx, _ptr(m), m.shape[0], c, o))

    def skin_info(self) -> SkinInfo:
        i = SkinInfo()
        self._check(self.lib.mcpt_get_skin_info(self.ctx, C.byref(i)))
        return i

    # ---- deforming parts: dual-quaternion skinning
    def set_skin_mode(self, mode: int):
        """SKIN_LINEAR (the default) or SKIN_DUAL_QUATERNION: how update_skin, update_skin_reproject and update_morph with bones blend a record's
        bones from now on.  Dual-quaternion mode keeps the volume of a twisted part and takes rigid bones only (rotation and translation); slot 0
        of a record is its pivot.  Sticky: survives set_vertex_skin, clone and rebuild.  Needs FLAG_DYNAMIC.  Synchronous."""
        self._check(self.lib.mcpt_set_skin_mode(self.ctx, int(mode)))

    def skin_mode(self) -> int:
        m = C.c_uint32()
        self._check(self.lib.mcpt_get_skin_mode(self.ctx, C.byref(m)))
        return int(m.value)

    # ---- deforming parts: morph targets
    def set_vertex_morph(self, vertex_targets, normal_targets=None):
        """Morph targets (blend shapes): each argument a list with one (index array, (n, 3) delta array) pair per target -- the records the target
        displaces, strictly ascending, and their displacements; normal_targets=None leaves the normals unmorphed, otherwise it has as many
        targets as vertex_targets (one weight drives both).  The scene as it is now becomes the rest pose update_morph deforms.  Needs
        FLAG_DYNAMIC.  Synchronous."""
        v, keep_v = targets_struct(vertex_targets)
        n, keep_n = (None, None) if normal_targets is None else targets_struct(normal_targets)
        self._check(self.lib.mcpt_set_vertex_morph(self.ctx, C.byref(v), self.holder.desc.n_vertex, None if n is None else C.byref(n), self.holder.desc.n_normal))

    @staticmethod
    def _weights_and_bones(weights, bones):
        w = np.ascontiguousarray(weights, np.float64).reshape(-1)
        m = None if bones is None else Renderer._matrices(bones)
        return w, m

    def update_morph(self, weights, bones=None):
        """One weight per target: every vertex and normal becomes its REST pose plus the weighted displacements of its entries, summed on the
        device in a fixed order (never accumulated over calls), then update_vertices' refit: only the weights cross the bus.  bones: one 3x4
        matrix per bone of the skin set with set_vertex_skin -- morph, then skin, in one call.  Asynchronous; the caller clears the film."""
        w, m = self._weights_and_bones(weights, bones)
        self._check(self.lib.mcpt_update_morph(self.ctx, _ptr(w), w.shape[0], _ptr(m), 0 if m is None else m.shape[0]))

    def update_morph_reproject(self, weights, bones=None, camera=None, **opts):
        """update_morph that carries the film over, as update_vertices_reproject does; opts: reproject_camera's."""
        w, m = self._weights_and_bones(weights, bones)
        c, o = _camera_and_opts(camera, opts)
        self._check(self.lib.mcpt_update_morph_reproject(self.ctx, _ptr(w), w.shape[0], _ptr(m), 0 if m is None else m.shape[0], c, o))

    def morph_info(self) -> MorphInfo:
        i = MorphInfo()
        self._check(self.lib.mcpt_get_morph_info(self.ctx, C.byref(i)))
        return i

    # ---- baked vertex animation: keyframes played by time
    def set_vertex_keyframes(self, vertex_frames, normal_frames=None, start_time=0.0, frame_time=1.0, interpolation=KEYFRAMES_LINEAR, wrap=KEYFRAMES_CLAMP):
        """The keyframes of a baked animation, uploaded once: vertex_frames (n_frames, n_vertex, 3), normal_frames None or (n_frames, n_normal, 3)
        (None: every update writes the normals the scene has now); frame k lies at start_time + k * frame_time.  interpolation: KEYFRAMES_LINEAR
        or KEYFRAMES_CATMULL_ROM; wrap: KEYFRAMES_CLAMP or KEYFRAMES_LOOP.  Independent of groups, skin and morph.  Needs FLAG_DYNAMIC.
        Synchronous."""
        v = np.ascontiguousarray(vertex_frames, np.float64)
        n = None if normal_frames is None else np.ascontiguousarray(normal_frames, np.float64)
        if v.ndim != 3 or v.shape[2] != 3 or (n is not None and (n.ndim != 3 or n.shape[2] != 3 or n.shape[0] != v.shape[0])):
            raise ValueError("need (n_frames, n, 3) arrays with as many normal frames as vertex frames")
        o = KeyframeOpts()
        o.struct_size = C.sizeof(KeyframeOpts); o.interpolation = int(interpolation); o.wrap = int(wrap)
        o.start_time = float(start_time); o.frame_time = float(frame_time)
        self._check(self.lib.mcpt_set_vertex_keyframes(self.ctx, _ptr(v), v.shape[1], _ptr(n), self.holder.desc.n_normal if n is None else n.shape[1],
                                                       v.shape[0], C.byref(o)))

    def update_keyframes(self, time):
        """The scene at `time` of the keyframes' clock: every vertex and normal interpolated on the device from 2 or 4 frames (on a keyframe:
        that frame, bit for bit), then update_vertices' refit: only the time crosses the bus.  Asynchronous; the caller clears the film."""
        self._check(self.lib.mcpt_update_keyframes(self.ctx, float(time)))

    def update_keyframes_reproject(self, time, camera=None, **opts):
        """update_keyframes that carries the film over, as update_vertices_reproject does; opts: reproject_camera's."""
        c, o = _camera_and_opts(camera, opts)
        self._check(self.lib.mcpt_update_keyframes_reproject(self.ctx, float(time), c, o))

    def keyframe_info(self) -> KeyframeInfo:
        i = KeyframeInfo()
        self._check(self.lib.mcpt_get_keyframe_info(self.ctx, C.byref(i)))
        return i

    # ---- each part driven by its own deformer in one update call
    def set_vertex_owners(self, vertex_owner, normal_owner):
        """One owner id (OWNER_NONE / _GROUPS / _SKIN / _MORPH / _KEYFRAMES) per vertex and per normal (owners_from_faces derives them from
        faces): the one route of update_parts that writes the record.  Calling it again replaces the owners.  Needs FLAG_DYNAMIC.  Synchronous."""
        vo = np.ascontiguousarray(vertex_owner, np.uint8).reshape(-1); no = np.ascontiguousarray(normal_owner, np.uint8).reshape(-1)
        self._check(self.lib.mcpt_set_vertex_owners(self.ctx, _ptr(vo), vo.size, _ptr(no) if no.size else None, no.size))

    def clear_vertex_owners(self):
        """Drops the owners and frees what they hold on the device; update_parts refuses from then on."""
        self._check(self.lib.mcpt_set_vertex_owners(self.ctx, None, 0, None, 0))

    def _scene_update(self, groups, bones, weights, time, morph_then_skin, routes):
        """(the record, the arrays it points into).  The routes run are those whose payload is given -- bones mean the skin route, and with
        morph_then_skin also the skin behind the morph --, or exactly `routes` (a ROUTE_* mask) when that is given."""
        u = SceneUpdate(); keep = []
        u.struct_size = C.sizeof(SceneUpdate)
        if groups is not None:
            m = self._matrices(groups); keep.append(m)
            u.routes |= ROUTE_GROUPS; u.group_m3x4 = m.ctypes.data; u.n_groups = m.shape[0]
        if bones is not None:
            m = self._matrices(bones); keep.append(m)
            u.routes |= ROUTE_SKIN; u.bone_m3x4 = m.ctypes.data; u.n_bones = m.shape[0]
        if weights is not None:
            w = np.ascontiguousarray(weights, np.float64).reshape(-1); keep.append(w)
            u.routes |= ROUTE_MORPH; u.morph_weight = w.ctypes.data; u.n_targets = w.shape[0]
        if time is not None:
            u.routes |= ROUTE_KEYFRAMES; u.time = float(time)
        if morph_then_skin:
            u.flags |= PARTS_MORPH_THEN_SKIN
        if routes is not None:
            u.routes = int(routes)
        return u, keep

    def update_parts(self, groups=None, bones=None, weights=None, time=None, morph_then_skin=False, routes=None):
        """Several deformers in one call, each writing only the records it owns (set_vertex_owners), then ONE normals pass and ONE refit.  The
        routes run are those whose payload is given: groups (update_transforms' matrices), bones (update_skin's), weights (update_morph's), time
        (update_keyframes').  morph_then_skin: the morph's records are morphed, then skinned by `bones`.  routes: a ROUTE_* mask that replaces
        the one derived from the payloads (e.g. ROUTE_MORPH alone with bones that only the morph uses).  Records of owner NONE, and of owners
        whose route does not run, keep their bits.  Asynchronous; the caller clears the film."""
        u, keep = self._scene_update(groups, bones, weights, time, morph_then_skin, routes)
        self._check(self.lib.mcpt_update_parts(self.ctx, C.byref(u)))

    def update_parts_reproject(self, groups=None, bones=None, weights=None, time=None, morph_then_skin=False, routes=None, camera=None, **opts):
        """update_parts that carries the film over, as update_vertices_reproject does; opts: reproject_camera's."""
        u, keep = self._scene_update(groups, bones, weights, time, morph_then_skin, routes)
        c, o = _camera_and_opts(camera, opts)
        self._check(self.lib.mcpt_update_parts_reproject(self.ctx, C.byref(u), c, o))

    def parts_info(self) -> PartsInfo:
        i = PartsInfo()
        self._check(self.lib.mcpt_get_parts_info(self.ctx, C.byref(i)))
        return i

    def vertices(self):
        """(vertex, normal): the context's current vertices and normals as the device holds them, (n, 3) float64 each -- whatever update call
        wrote them.  Needs FLAG_DYNAMIC.  Synchronous; touches nothing."""
        v = np.empty((self.holder.desc.n_vertex, 3), np.float64); n = np.empty((self.holder.desc.n_normal, 3), np.float64)
        self._check(self.lib.mcpt_probe_vertices(self.ctx, _ptr(v), _ptr(n)))
        return v, n

    # ---- smooth normals recomputed on the device after every update
    def set_auto_normals(self, mask=None, mode: int = NORMALS_AREA):
        """From now on every scene update (update_vertices / _transforms / _skin / _morph and their _reproject forms) recomputes the normal
        records chosen by `mask` (one byte per normal, != 0 = recompute; None = all) from the deformed faces: the normalised sum of the
        area-weighted face normals, in a fixed order.  The scene as it is now is the reference pose that fixes each face's side.  For the
        chosen records this OVERRIDES what the update wrote, caller-supplied normals included.  mode=NORMALS_OFF frees the lists.  Needs
        FLAG_DYNAMIC.  Synchronous."""
        m = None if mask is None else np.ascontiguousarray(mask, np.uint8).reshape(-1)
        o = NormalsOpts()
        o.struct_size = C.sizeof(NormalsOpts); o.mode = int(mode)
        self._check(self.lib.mcpt_set_auto_normals(self.ctx, _ptr(m), self.holder.desc.n_normal if m is None else m.shape[0], C.byref(o)))

    def update_normals(self):
        """The normals pass and the refit on the scene as it is: nothing moves.  Needs set_auto_normals.  Asynchronous; the caller clears the film."""
        self._check(self.lib.mcpt_update_normals(self.ctx))

    def normals_info(self) -> NormalsInfo:
        i = NormalsInfo()
        self._check(self.lib.mcpt_get_normals_info(self.ctx, C.byref(i)))
        return i

    # ---- faces shown and hidden on the device
    def _visibility_mask(self, mask):
        m = None if mask is None else np.ascontiguousarray(np.asarray(mask) != 0, np.uint8).reshape(-1)
        return m, self.holder.desc.n_face if m is None else m.shape[0]

    def set_face_visibility(self, mask):
        """One entry per face of the scene (visibility_from_materials builds one), != 0 = visible; None = every face visible and the mask freed.
        Hidden faces cannot be hit by any ray and are no lights; the mask is sticky through every later update.  A scene update without a source:
        nothing moves, the light list is rebuilt, both trees are refitted.  Needs FLAG_DYNAMIC.  Asynchronous; the caller clears the film."""
        m, n = self._visibility_mask(mask)
        self._check(self.lib.mcpt_set_face_visibility(self.ctx, _ptr(m), n))

    def set_face_visibility_reproject(self, mask, camera=None, **opts):
        """set_face_visibility that carries the film over, as update_vertices_reproject does; opts: reproject_camera's."""
        m, n = self._visibility_mask(mask)
        c, o = _camera_and_opts(camera, opts)
        self._check(self.lib.mcpt_set_face_visibility_reproject(self.ctx, _ptr(m), n, c, o))

    def visibility_info(self) -> VisibilityInfo:
        i = VisibilityInfo()
        self._check(self.lib.mcpt_get_visibility_info(self.ctx, C.byref(i)))
        return i

    def probe_triangles(self, boxes=True):
        """Per face, in Model::face order, as the device holds them: ((n_face, 9) fp32 {first corner, edge 1, edge 2}, (n_face, 6) fp32 refit box
        {lo, hi}).  boxes=False: the records alone (the boxes exist once a scene update has run since creation or the last rebuild)."""
        nf = self.holder.desc.n_face
        rec = np.zeros((nf, 9), np.float32); box = np.zeros((nf, 6), np.float32) if boxes else None
        self._check(self.lib.mcpt_probe_triangles(self.ctx, _ptr(rec), _ptr(box)))
        return (rec, box) if boxes else rec

    # ---- camera models through a ray-generation stage
    def set_camera_model(self, model: int = CAMERA_PINHOLE, lens_radius=0.0, focus_distance=0.0, blades=0, blade_rotation=0.0, ortho_height=0.0):
        """The camera model render_camera and probe_camera_rays use from now on: CAMERA_PINHOLE, CAMERA_THIN_LENS (lens_radius >= 0,
        focus_distance > 0, blades 0 = disk or 3..16 = polygon turned by blade_rotation radians), CAMERA_ORTHOGRAPHIC (ortho_height > 0: the
        film's height in world units) or CAMERA_EQUIRECT.  Fields of other models are ignored.  render() and every other call stay pinhole."""
        m = camera_model(model, lens_radius, focus_distance, blades, blade_rotation, ortho_height)
        self._check(self.lib.mcpt_set_camera_model(self.ctx, C.byref(m)))

    def camera_model(self) -> CameraModel:
        m = CameraModel()
        self._check(self.lib.mcpt_get_camera_model(self.ctx, C.byref(m), None))
        return m

    def camera_model_info(self) -> CameraModelInfo:
        m = CameraModel(); i = CameraModelInfo()
        self._check(self.lib.mcpt_get_camera_model(self.ctx, C.byref(m), C.byref(i)))
        return i

    def render_camera(self, spp: int, seed: int = 0, first_sample: int = 0):
        """`spp` samples of the set camera model added to every pixel of the bound film: per sample the ray kernel, then the wavefront pipeline.
        With CAMERA_PINHOLE the film is render()'s, bit for bit.  Needs the wavefront pipeline (INTEGRATOR_MIS)."""
        self._check(self.lib.mcpt_render_camera(self.ctx, spp, seed, first_sample))

    def autofocus(self, px: int, py: int) -> float:
        """The focus_distance that makes pixel (px, py) sharp: the distance of its pixel-centre first hit along the view direction."""
        out = C.c_double(0.0)
        self._check(self.lib.mcpt_autofocus(self.ctx, int(px), int(py), C.byref(out)))
        return float(out.value)

    def probe_camera_rays(self, xy, sample: int = 0, seed: int = 0):
        """The set model's primary rays for pixels xy (n, 2) of sample `sample`: ((n, 3) float64 origins in DEVICE coordinates -- world less
        info().centre --, (n, 3) float64 directions holding fp32 values)."""
        xy = np.ascontiguousarray(xy, np.int32).reshape(-1, 2)
        o = np.zeros((xy.shape[0], 3), np.float64); d = np.zeros((xy.shape[0], 3), np.float64)
        self._check(self.lib.mcpt_probe_camera_rays(self.ctx, xy.shape[0], _ptr(xy), sample, seed, _ptr(o), _ptr(d)))
        return o, d

    # ---- material, light and texture edits
    def update_materials(self, materials, map_kd=None):
        """New ks / ns / radiance for the same number of materials (a list of scenes.Material); map_kd: per material the index of the creation
        texture it maps, None = its own.  Every material whose texels (built as DescHolder builds them) differ from the ones held gets them
        replaced (update_texture; same size only).  Asynchronous; the caller clears the film."""
        mats = _materials_c(materials, map_kd)
        self._check(self.lib.mcpt_update_materials(self.ctx, mats, len(materials)))
        for i, m in enumerate(materials[:len(self.tex_arrays)]):
            t = material_texels(m)
            if t.shape != self.tex_arrays[i].shape or not np.array_equal(t, self.tex_arrays[i]):
                self.update_texture(i, t)

    def update_texture(self, index: int, array):
        """New (h, w, 3) fp32 texels for texture `index`, of the size it was created with; a 1x1 texture is a constant Kd colour."""
        t = np.ascontiguousarray(array, np.float32)
        if t.ndim != 3 or t.shape[2] != 3:
            raise ValueError("update_texture: need an (h, w, 3) array")
        tex = Texture()
        tex.width = t.shape[1]; tex.height = t.shape[0]; tex.rgb = t.ctypes.data_as(C.POINTER(C.c_float))
        self._check(self.lib.mcpt_update_texture(self.ctx, int(index), C.byref(tex)))
        if 0 <= index < len(self.tex_arrays):
            self.tex_arrays[index] = t.copy()

    def material_info(self) -> MaterialInfo:
        i = MaterialInfo()
        self._check(self.lib.mcpt_get_material_info(self.ctx, C.byref(i)))
        return i

    def probe_lights(self):
        """The light list as the device holds it: ((n,) face in Model::face order, (n, 13) {area, radiance, n0, n1, n2}, (n, 9) fp64 corners)."""
        cap = max(1, int(self.info().n_lights))
        face = np.zeros(cap, np.int32); rec = np.zeros((cap, 13), np.float32); pos = np.zeros((cap, 9), np.float64)
        n = C.c_uint32(0)
        self._check(self.lib.mcpt_probe_lights(self.ctx, cap, _ptr(face), _ptr(rec), _ptr(pos), C.byref(n)))
        return face[:n.value].copy(), rec[:n.value].copy(), pos[:n.value].copy()

    def probe_face_classes(self) -> np.ndarray:
        """(n_face,) uint8: the lobe class (0 diffuse, 1 Blinn-Phong, 2 mirror) every face's hits are shaded with."""
        out = np.zeros(self.holder.face.shape[0], np.uint8)
        self._check(self.lib.mcpt_probe_face_classes(self.ctx, _ptr(out)))
        return out

    def update_info(self) -> UpdateInfo:
        i = UpdateInfo()
        self._check(self.lib.mcpt_get_update_info(self.ctx, C.byref(i)))
        return i

    # ---- new trees for the geometry as it is now
    def rebuild(self, builder: int = REBUILD_SAME):
        """Both trees built anew for the context's current vertices, in place; film, counters, features, groups, skin, morph targets, materials and lights stay.
        builder: REBUILD_SAME (the one the context was created with), REBUILD_HOST or REBUILD_DEVICE.  Needs FLAG_DYNAMIC.  Synchronous."""
        o = RebuildOpts()
        o.struct_size = C.sizeof(RebuildOpts); o.builder = int(builder)
        self._check(self.lib.mcpt_rebuild_trees(self.ctx, C.byref(o)))

    def rebuild_info(self) -> RebuildInfo:
        i = RebuildInfo()
        self._check(self.lib.mcpt_get_rebuild_info(self.ctx, C.byref(i)))
        return i

    def validate_trees(self):
        """The host soundness walks over the context's current device trees; raises McptError with the walk's message if one fails."""
        self._check(self.lib.mcpt_probe_validate_trees(self.ctx))

    def sync(self):
        self._check(self.lib.mcpt_sync(self.ctx))

    def read_accum(self) -> np.ndarray:
        out = np.zeros((self.height, self.width, 4), np.float32)
        self._check(self.lib.mcpt_read_accum(self.ctx, _ptr(out)))
        return out

    def write_accum(self, rgba: np.ndarray):
        a = np.ascontiguousarray(rgba, np.float32)
        assert a.size == self.width * self.height * 4
        self._check(self.lib.mcpt_write_accum(self.ctx, _ptr(a)))

    def clear(self):
        self._check(self.lib.mcpt_clear_accum(self.ctx))

    def tonemap(self, flip_y=False) -> np.ndarray:
        out = np.zeros((self.height, self.width, 3), np.uint8)
        self._check(self.lib.mcpt_tonemap(self.ctx, _ptr(out), 1 if flip_y else 0))
        return out

    def tonemap_map(self, flip_y=False) -> np.ndarray:
        """mcpt_tonemap_map: a copy of the context's own pinned image (the C pointer stays valid until the next tonemap call)."""
        p = C.c_void_p()
        self._check(self.lib.mcpt_tonemap_map(self.ctx, 1 if flip_y else 0, C.byref(p)))
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(self.height, self.width, 3)).copy()

    def accum_device_ptr(self) -> int:
        p = C.c_void_p()
        self._check(self.lib.mcpt_accum_device_ptr(self.ctx, C.byref(p)))
        return p.value

    def tonemap_buffer(self, device_ptr: int, flip_y=False) -> np.ndarray:
        out = np.zeros((self.height, self.width, 3), np.uint8)
        self._check(self.lib.mcpt_tonemap_buffer(self.ctx, C.c_void_p(device_ptr), _ptr(out), 1 if flip_y else 0))
        return out

    def counters(self) -> Counters:
        c = Counters()
        self._check(self.lib.mcpt_get_counters(self.ctx, C.byref(c)))
        return c

    def reset_counters(self):
        self._check(self.lib.mcpt_reset_counters(self.ctx))

    def info(self) -> SceneInfo:
        i = SceneInfo()
        self._check(self.lib.mcpt_get_scene_info(self.ctx, C.byref(i)))
        return i

    def bind_accum(self, device_ptr: int):
        self._check(self.lib.mcpt_bind_accum(self.ctx, C.c_void_p(device_ptr)))

    def set_stream(self, hip_stream: int):
        """A caller-owned stream handle; 0 = back to the context's own stream (see set_null_stream for the default stream)."""
        self._check(self.lib.mcpt_set_stream(self.ctx, C.c_void_p(hip_stream)))

    def set_null_stream(self):
        """Order the context's work with the device's legacy default stream (torch's default stream has handle 0)."""
        self._check(self.lib.mcpt_set_null_stream(self.ctx))

    def set_torch_stream(self, stream):
        """Bind a torch.cuda.Stream: its handle, or the legacy default stream when the handle is 0."""
        h = int(stream.cuda_stream)
        if h:
            self.set_stream(h)
        else:
            self.set_null_stream()

    # ---- denoised preview
    def render_features(self, spp: int = 4, seed: int = 0):
        """First-hit feature buffers from the camera rays of samples 0 .. spp-1 of `seed` (asynchronous)."""
        self._check(self.lib.mcpt_render_features(self.ctx, spp, seed))

    def features(self) -> np.ndarray:
        """(h, w, 8): albedo rgb, coverage, normal xyz, depth."""
        out = np.zeros((self.height, self.width, 8), np.float32)
        self._check(self.lib.mcpt_read_features(self.ctx, _ptr(out)))
        return out

    def denoise(self, iterations=0, sigma_color=0.0, sigma_normal=0.0, sigma_depth=0.0, device_ptr: Optional[int] = None,
                split_emission=False, clamp_fireflies=False, firefly_clamp=0.0) -> np.ndarray:
        """A-trous filter of the context film (or of the device film at `device_ptr`): (h, w, 4) records {r, g, b, 1}.  split_emission: emitted
        light is kept apart from the reflected light the filter works on; clamp_fireflies: a pixel more than firefly_clamp times brighter than
        its brightest neighbour is scaled down to that (0 = the default)."""
        o = _denoise_opts(iterations, sigma_color, sigma_normal, sigma_depth, split_emission, clamp_fireflies, firefly_clamp)
        self._check(self.lib.mcpt_denoise(self.ctx, None if device_ptr is None else C.c_void_p(device_ptr), C.byref(o)))
        out = np.zeros((self.height, self.width, 4), np.float32)
        self._check(self.lib.mcpt_read_denoised(self.ctx, _ptr(out)))
        return out

    def probe_denoise(self, film, feat, emis=None, iterations=0, sigma_color=0.0, sigma_normal=0.0, sigma_depth=0.0,
                      split_emission=False, clamp_fireflies=False, firefly_clamp=0.0) -> np.ndarray:
        """The filter alone on a caller film (h, w, 4), features (h, w, 8) and -- with split_emission, and only then -- emission (h, w, 4):
        what denoise() would return for them.  The context's own features, emission and denoised film are untouched."""
        a = np.ascontiguousarray(film, np.float32); b = np.ascontiguousarray(feat, np.float32)
        e = None if emis is None else np.ascontiguousarray(emis, np.float32)
        n = self.width * self.height
        assert a.size == 4 * n and b.size == 8 * n and (e is None or e.size == 4 * n)
        o = _denoise_opts(iterations, sigma_color, sigma_normal, sigma_depth, split_emission, clamp_fireflies, firefly_clamp)
        out = np.zeros((self.height, self.width, 4), np.float32)
        self._check(self.lib.mcpt_probe_denoise(self.ctx, _ptr(a), _ptr(b), None if e is None else _ptr(e), C.byref(o), _ptr(out)))
        return out

    def emission(self) -> np.ndarray:
        """(h, w, 4): emitted radiance rgb of the first hits / spp and their share of the spp, for the features held (after a split denoise)."""
        out = np.zeros((self.height, self.width, 4), np.float32)
        self._check(self.lib.mcpt_read_emission(self.ctx, _ptr(out)))
        return out

    def denoised_device_ptr(self) -> int:
        p = C.c_void_p()
        self._check(self.lib.mcpt_denoised_device_ptr(self.ctx, C.byref(p)))
        return p.value

    # ---- probes
    def probe_trace(self, origin, direction, t1=None, t2=None, any_hit=False):
        o = np.ascontiguousarray(origin, np.float64).reshape(-1, 3); d = np.ascontiguousarray(direction, np.float64).reshape(-1, 3)
        n = o.shape[0]
        t1 = np.full(n, 1e-4) if t1 is None else np.ascontiguousarray(t1, np.float64)
        t2 = np.full(n, np.finfo(np.float64).max) if t2 is None else np.ascontiguousarray(t2, np.float64)
        ot = np.zeros(n, np.float32); tri = np.zeros(n, np.int32); u = np.zeros(n, np.float32); v = np.zeros(n, np.float32)
        self._check(self.lib.mcpt_probe_trace(self.ctx, n, _ptr(o), _ptr(d), _ptr(t1), _ptr(t2), 1 if any_hit else 0,
                                              _ptr(ot), _ptr(tri), _ptr(u), _ptr(v)))
        return ot, tri, u, v

    def probe_trace4(self, origin, direction, t2=None, any_hit=False):
        """BVH::hit / has_hit through the production wf_trace8_kernel (8-wide compressed tree)."""
        o = np.ascontiguousarray(origin, np.float64).reshape(-1, 3); d = np.ascontiguousarray(direction, np.float64).reshape(-1, 3)
        n = o.shape[0]
        t2 = np.full(n, np.finfo(np.float64).max) if t2 is None else np.ascontiguousarray(t2, np.float64)
        ot = np.zeros(n, np.float32); tri = np.zeros(n, np.int32); u = np.zeros(n, np.float32); v = np.zeros(n, np.float32)
        self._check(self.lib.mcpt_probe_trace4(self.ctx, n, _ptr(o), _ptr(d), _ptr(t2), 1 if any_hit else 0,
                                               _ptr(ot), _ptr(tri), _ptr(u), _ptr(v)))
        return ot, tri, u, v

    def probe_hit_shade(self, face, u, v, direction):
        face = np.ascontiguousarray(face, np.int32); u = np.ascontiguousarray(u, np.float32); v = np.ascontiguousarray(v, np.float32)
        d = np.ascontiguousarray(direction, np.float64).reshape(-1, 3); n = face.shape[0]
        out = np.zeros((n, 6), np.float32)
        self._check(self.lib.mcpt_probe_hit_shade(self.ctx, n, _ptr(face), _ptr(u), _ptr(v), _ptr(d), _ptr(out)))
        return out

    def probe_cast_ray(self, xy, xi):
        xy = np.ascontiguousarray(xy, np.int32).reshape(-1, 2); xi = np.ascontiguousarray(xi, np.float32).reshape(-1, 2)
        out = np.zeros((xy.shape[0], 6), np.float32)
        self._check(self.lib.mcpt_probe_cast_ray(self.ctx, xy.shape[0], _ptr(xy), _ptr(xi), _ptr(out)))
        return out

    def probe_bsdf(self, normal, wi, kd, ks, ns, wo, xi):
        arrs = [np.ascontiguousarray(a, np.float32) for a in (normal, wi, kd, ks, ns, wo, xi)]
        n = arrs[4].shape[0]
        out = np.zeros((n, 12), np.float32)
        self._check(self.lib.mcpt_probe_bsdf(self.ctx, n, *[_ptr(a) for a in arrs], _ptr(out)))
        return out

    def probe_sample_light(self, point, xi):
        p = np.ascontiguousarray(point, np.float64).reshape(-1, 3); xi = np.ascontiguousarray(xi, np.float32).reshape(-1, 3)
        out = np.zeros((p.shape[0], 10), np.float32)
        self._check(self.lib.mcpt_probe_sample_light(self.ctx, p.shape[0], _ptr(p), _ptr(xi), _ptr(out)))
        return out

    def probe_paths(self, origin, direction, seed=0):
        o = np.ascontiguousarray(origin, np.float64).reshape(-1, 3); d = np.ascontiguousarray(direction, np.float64).reshape(-1, 3)
        out = np.zeros((o.shape[0], 3), np.float32)
        self._check(self.lib.mcpt_probe_paths(self.ctx, o.shape[0], _ptr(o), _ptr(d), seed, _ptr(out)))
        return out

    def probe_texture(self, material, uv):
        uv = np.ascontiguousarray(uv, np.float32).reshape(-1, 2)
        out = np.zeros((uv.shape[0], 3), np.float32)
        self._check(self.lib.mcpt_probe_texture(self.ctx, material, uv.shape[0], _ptr(uv), _ptr(out)))
        return out

    def probe_rng(self, pixel_sample_block, seed=0):
        k = np.ascontiguousarray(pixel_sample_block, np.uint32).reshape(-1, 3)
        out = np.zeros((k.shape[0], 4), np.float32)
        self._check(self.lib.mcpt_probe_rng(self.ctx, k.shape[0], _ptr(k), seed, _ptr(out)))
        return out
