"""ctypes mirror of include/mcpt.h's camera-model section: mcpt_camera_model, mcpt_camera_model_info and the model constants.
Re-exported by the package; tests/test_camera_ref.py holds the structs' sizes and offsets to the header."""
import ctypes as C

CAMERA_PINHOLE = 0
CAMERA_THIN_LENS = 1
CAMERA_ORTHOGRAPHIC = 2
CAMERA_EQUIRECT = 3
CAMERA_MAX_BLADES = 16


class CameraModel(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("model", C.c_uint32), ("lens_radius", C.c_double), ("focus_distance", C.c_double),
                ("blades", C.c_uint32), ("reserved0", C.c_uint32), ("blade_rotation", C.c_double), ("ortho_height", C.c_double),
                ("reserved", C.c_uint32 * 4)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if not k.startswith("reserved")}


class CameraModelInfo(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("model", C.c_uint32), ("renders", C.c_uint32), ("reserved0", C.c_uint32), ("passes", C.c_uint64),
                ("last_stage_ms", C.c_double), ("device_bytes", C.c_uint64), ("reserved", C.c_uint32 * 4)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if not k.startswith("reserved")}


def camera_model(model=CAMERA_PINHOLE, lens_radius=0.0, focus_distance=0.0, blades=0, blade_rotation=0.0, ortho_height=0.0) -> CameraModel:
    """The struct mcpt_set_camera_model takes, with this library's struct_size."""
    m = CameraModel()
    m.struct_size = C.sizeof(CameraModel); m.model = int(model); m.lens_radius = float(lens_radius); m.focus_distance = float(focus_distance)
    m.blades = int(blades); m.blade_rotation = float(blade_rotation); m.ortho_height = float(ortho_height)
    return m
