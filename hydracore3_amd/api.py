"""ctypes binding of the C ABI in include/hydra_hip.h (hydracore3_amd/libhydra_hip.so).

`HipIntegrator` mirrors the slice of the reference's `Integrator` / `IntegratorDR` class surface that the hot path
needs (integrator_pt.h:123-703, diff_render/integrator_dr.h:27-136): same method names, same argument meaning, same
ownership rules (the caller owns ``out_color`` and it is accumulated into; ``m_randomGens`` lives with the integrator).

There is NO CPU fallback: if the HIP library is missing or no GPU is visible this module raises.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from .scene import HIT_DTYPE, Params, SceneData, SceneDesc

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("HYDRA_HIP_LIB", os.path.join(_HERE, "libhydra_hip.so"))   # override: A/B builds of the kernels

# every symbol include/hydra_hip.h declares: name -> (restype, argtypes)
_vp, _u32, _u64, _f, _i, _sz = C.c_void_p, C.c_uint32, C.c_uint64, C.c_float, C.c_int, C.c_size_t
ABI = {
    "hpt_create": (_i, [_i, C.POINTER(_vp)]),
    "hpt_destroy": (None, [_vp]),
    "hpt_last_error": (C.c_char_p, [_vp]),
    "hpt_device_info": (_i, [_vp, C.POINTER(_i), C.POINTER(_i), C.c_char_p, _sz]),
    "hpt_set_optics": (_i, [_vp, _vp, _u32, _f, _f]),
    "hpt_plastic_precompute": (_i, [_f, _f, _f, _vp, _vp, _vp, C.POINTER(_f), C.POINTER(_f)]),
    "hpt_decode_jpeg": (_i, [_vp, _u64, C.POINTER(_u32), C.POINTER(_u32), _vp, _u64]),
    "hpt_film_precompute": (_i, [_vp, _vp, _u64, C.POINTER(_u64), C.POINTER(_i)]),
    "hpt_device_malloc": (_i, [_vp, _sz, C.POINTER(_vp)]),
    "hpt_device_free": (_i, [_vp, _vp]),
    "hpt_device_copy": (_i, [_vp, _vp, _vp, _sz, _i]),
    "hpt_device_memset": (_i, [_vp, _vp, _i, _sz]),
    "hpt_clear_geom": (_i, [_vp]),
    "hpt_add_geom_triangles3f": (_u32, [_vp, _vp, _sz, _vp, _sz, _u32, _sz]),
    "hpt_update_geom_triangles3f": (_i, [_vp, _u32, _vp, _sz, _vp, _sz, _u32, _sz]),
    "hpt_clear_scene": (_i, [_vp]),
    "hpt_add_instance": (_u32, [_vp, _u32, _vp]),
    "hpt_update_instance": (_i, [_vp, _u32, _vp]),
    "hpt_commit_scene": (_i, [_vp, _u32]),
    "hpt_ray_query_nearest": (_i, [_vp, _vp, _vp, _u32, _vp]),
    "hpt_ray_query_any": (_i, [_vp, _vp, _vp, _u32, _vp]),
    "hpt_ray_query_nearest_motion": (_i, [_vp, _vp, _vp, _u32, _f, _vp]),
    "hpt_ray_query_any_motion": (_i, [_vp, _vp, _vp, _u32, _f, _vp]),
    "hpt_add_instance_motion": (_u32, [_vp, _u32, _vp, _u32]),
    "hpt_upload_scene": (_i, [_vp, C.POINTER(SceneDesc)]),
    "hpt_update_params": (_i, [_vp, C.POINTER(Params)]),
    "hpt_update_materials": (_i, [_vp, _sz, _sz, _vp]),
    "hpt_update_lights": (_i, [_vp, _sz, _sz, _vp]),
    "hpt_update_mat_id_offsets": (_i, [_vp, _vp, _sz]),
    "hpt_pack_xy": (_i, [_vp, _u32, _u32]),
    "hpt_get_packed_xy": (_i, [_vp, _vp, _u32]),
    "hpt_init_random_gens": (_i, [_vp, _u32]),
    "hpt_init_random_gens_from": (_i, [_vp, _u32, _u32]),
    "hpt_get_random_gens": (_i, [_vp, _vp, _u32]),
    "hpt_set_random_gens": (_i, [_vp, _vp, _u32]),
    "hpt_path_trace_block": (_i, [_vp, _u32, _u32, _u32, _vp, _u32]),
    "hpt_naive_path_trace_block": (_i, [_vp, _u32, _u32, _u32, _vp, _u32]),
    "hpt_path_trace_block_dev": (_i, [_vp, _u32, _u32, _u32, _vp, _u32, _i, _vp]),
    "hpt_path_trace_from_input_rays_block": (_i, [_vp, _u32, _u32, _vp, _vp, _vp, _u32]),
    "hpt_path_trace_from_input_rays_block_dev": (_i, [_vp, _u32, _u32, _vp, _vp, _vp, _u32, _vp]),
    "hpt_set_tid_interleave": (_i, [_vp, _u32, _u32]),
    "hpt_put_diff_tex2d": (_i, [_vp, _u32, _u32, _u32, _u32, C.POINTER(_u64), C.POINTER(_u64)]),
    "hpt_reset_diff_tex": (_i, [_vp]),
    "hpt_put_diff_lights": (_i, [_vp, _u32, _u32, C.POINTER(_u64), C.POINTER(_u64)]),
    "hpt_path_trace_dr": (_i, [_vp, _u32, _u32, _u32, _vp, _u32, _vp, _vp, _vp, _sz, C.POINTER(_f)]),
    "hpt_path_trace_dr_dev": (_i, [_vp, _u32, _u32, _u32, _vp, _u32, _vp, _vp, _vp, _sz, _vp, _vp]),
    "hpt_path_trace_vjp": (_i, [_vp, _u32, _u32, _u32, _vp, _u32, _vp, _vp, _vp, _sz]),
    "hpt_path_trace_vjp_dev": (_i, [_vp, _u32, _u32, _u32, _vp, _u32, _vp, _vp, _vp, _sz, _vp]),
    "hpt_ray_trace_dr": (_i, [_vp, _u32, _u32, _vp, _u32, _vp, _vp, _vp, _sz, C.POINTER(_f)]),
    "hpt_ray_trace_dr_dev": (_i, [_vp, _u32, _u32, _vp, _u32, _vp, _vp, _vp, _sz, _vp, _vp, _vp]),
    "hpt_adam_step_dev": (_i, [_vp, _vp, _vp, _vp, _vp, _sz, _i, _vp]),
    "hpt_image2d4f_regularizer_dev": (_i, [_vp, _i, _i, _vp, _vp, _vp]),
    "hpt_image2d4f_regularizer": (_i, [_vp, _i, _i, _vp, _vp]),
    "hpt_get_execution_time": (_i, [_vp, C.c_char_p, C.POINTER(_f)]),
    "hpt_set_instrumentation": (_i, [_vp, _i]),
    "hpt_get_counters": (_i, [_vp, C.POINTER(_u64)]),
    "hpt_get_dr_counters": (_i, [_vp, C.POINTER(_u64)]),
    "hpt_set_launch_config": (_i, [_vp, _i]),
    "hpt_set_accel_layout": (_i, [_vp, _i]),
    "hpt_set_schedule": (_i, [_vp, _i, _i, _i, _i]),
    "hpt_comm_get_unique_id": (_i, [_vp, _vp]),
    "hpt_comm_init": (_i, [_vp, _i, _i, _vp]),
    "hpt_comm_destroy": (_i, [_vp]),
    "hpt_reduce_framebuffer": (_i, [_vp, _vp, _sz, _i, _vp]),
    "hpt_allreduce_grad": (_i, [_vp, _vp, _sz, _vp]),
    "hpt_get_schedule": (_i, [_vp, C.POINTER(_i), C.POINTER(_u32)]),
    "hpt_get_last_launch": (_i, [_vp, C.POINTER(_u32)]),
    "hpt_get_stack_witness": (_i, [_vp, C.POINTER(_u64)]),
    "hpt_get_accel_info": (_i, [_vp, C.POINTER(_f)]),
    "hpt_set_option": (_i, [_vp, C.c_char_p, _i]),
    "hpt_get_commit_time": (_i, [_vp, C.POINTER(_f)]),
    "hpt_get_refit_info": (_i, [_vp, C.POINTER(_f)]),
    "hpt_get_build_info": (_i, [_vp, C.POINTER(_f)]),
    "hpt_read_accel": (_i, [_vp, _i, _vp, _u64, C.POINTER(_u64), C.POINTER(_u32)]),
    "hpt_get_two_level_info": (_i, [_vp, C.POINTER(_f)]),
    "hpt_read_accel_two_level": (_i, [_vp, _i, _vp, _u64, C.POINTER(_u64), C.POINTER(_u32)]),
    "hpt_last_kernel_ms": (_i, [_vp, C.POINTER(_f)]),
    "hpt_eval_gbuffer": (_i, [_vp, _u32, _vp]),
    "hpt_eval_gbuffer_dev": (_i, [_vp, _u32, _vp, _vp, _vp]),
    "hpt_denoise_frame": (_i, [_vp, _u32, _u32, _vp, _vp, _vp, _vp]),
    "hpt_denoise_frame_dev": (_i, [_vp, _u32, _u32, _vp, _vp, _vp, _vp, _vp]),
    "hpt_denoise_frame_var": (_i, [_vp, _u32, _u32, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "hpt_denoise_frame_var_dev": (_i, [_vp, _u32, _u32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "hpt_cast_single_ray_block": (_i, [_vp, _u32, _vp, _u32]),
    "hpt_cast_single_ray_block_dev": (_i, [_vp, _u32, _vp, _u32, _vp]),
    "hpt_ray_trace_block": (_i, [_vp, _u32, _u32, _vp, _u32]),
    "hpt_ray_trace_block_dev": (_i, [_vp, _u32, _u32, _vp, _u32, _vp]),
    "hpt_qmc_table": (_i, [_vp]),
    "hpt_qmc_layout": (_i, [_i, _i, _i, _vp]),
    "hpt_qmc_sample_count": (_u32, [_u32, _u32]),
    "hpt_path_trace_qmc_block": (_i, [_vp, _u32, _u32, _vp, _u32]),
    "hpt_path_trace_qmc_block_dev": (_i, [_vp, _u32, _u32, _vp, _u32, _vp, _vp, _vp]),
    "hpt_path_trace_qmc_block_dev2": (_i, [_vp, _u32, _u32, _vp, _u32, _vp, _vp, _vp, _vp]),
    "hpt_kmlt_state_size": (_u32, [_u32]),
    "hpt_path_trace_pss_dev": (_i, [_vp, _vp, _u32, _u32, _vp, _vp, _vp]),
    "hpt_path_trace_pss_dev2": (_i, [_vp, _vp, _u32, _u32, _vp, _vp, _vp, _vp, _vp]),
    "hpt_kmlt_chain_count": (_i, [_vp, _u32, _u32, C.POINTER(_u32), C.POINTER(_u32)]),
    "hpt_path_trace_kmlt_block": (_i, [_vp, _u32, _u32, _vp, _u32]),
    "hpt_path_trace_kmlt_block_dev": (_i, [_vp, _u32, _u32, _vp, _u32, _i, _vp, _vp, _vp]),
    "hpt_cam_create": (_i, [_vp, _i, C.POINTER(_vp)]),
    "hpt_cam_destroy": (None, [_vp]),
    "hpt_cam_set_parameters": (_i, [_vp, _u32, _u32, _vp, _i]),
    "hpt_cam_set_lens": (_i, [_vp, _vp, _u32, _f, _f]),
    "hpt_cam_set_batch_size": (_i, [_vp, _u32]),
    "hpt_cam_make_rays_block": (_i, [_vp, _vp, _vp, _u32, _i]),
    "hpt_cam_make_rays_block_dev": (_i, [_vp, _vp, _vp, _u32, _i, _vp]),
    "hpt_cam_add_samples_contribution_block": (_i, [_vp, _vp, _vp, _u32, _u32, _u32, _i]),
    "hpt_cam_add_samples_contribution_block_dev": (_i, [_vp, _vp, _vp, _u32, _u32, _u32, _i, _vp]),
    "hpt_cam_read_state": (_i, [_vp, _vp, _vp, _vp, _u32]),
    "hpt_cam_render_dev": (_i, [_vp, _vp, _vp, _u32, _vp]),
    "hpt_cam_get_execution_time": (_i, [_vp, C.c_char_p, C.POINTER(_f)]),
    "hpt_path_trace_block_counts": (_i, [_vp, _u32, _u32, _u32, _vp, _u32, _vp, _vp]),
    "hpt_path_trace_block_counts_dev": (_i, [_vp, _u32, _u32, _u32, _vp, _u32, _i, _vp, _vp, _vp]),
    "hpt_adaptive_plan": (_i, [_vp, _u32, _u32, _vp, _vp, _vp, _vp]),
    "hpt_adaptive_plan_dev": (_i, [_vp, _u32, _u32, _vp, _vp, _vp, _vp, _vp]),
    "hpt_adaptive_resolve": (_i, [_vp, _u32, _u32, _u32, _vp, _vp, _vp]),
    "hpt_adaptive_resolve_dev": (_i, [_vp, _u32, _u32, _u32, _vp, _vp, _vp, _vp]),
    "hpt_adaptive_variance": (_i, [_vp, _u32, _u32, _vp, _vp]),
    "hpt_adaptive_variance_dev": (_i, [_vp, _u32, _u32, _vp, _vp, _vp]),
    "hpt_path_trace_block_adaptive": (_i, [_vp, _u32, _u32, _u32, _vp, _vp, _u32, _vp, _vp]),
    "hpt_path_trace_block_adaptive_dev": (_i, [_vp, _u32, _u32, _u32, _vp, _vp, _u32, _vp, _vp, _vp]),
}

# adaptive sampling: hpt_pixel_moments, one 16-byte record per tid; hpt_adaptive_info, the planner's and the loop's 32-byte report
MOMENTS_DTYPE = np.dtype([("sumY", np.float32), ("sumY2", np.float32), ("passes", np.uint32), ("reserved", np.uint32)])
ADAPTIVE_INFO_DTYPE = np.dtype([("passes", np.uint64), ("pixels", np.uint32), ("maxPasses", np.uint32), ("nonfinite", np.uint32), ("rounds", np.uint32),
                                ("deviceMs", np.float32), ("reserved", np.uint32)])
assert MOMENTS_DTYPE.itemsize == 16 and ADAPTIVE_INFO_DTYPE.itemsize == 32


# passes a pixel may be given per round when the caller names no `step`: the sweep of profiles/adaptive.md (c) has its shortest wall time there (16 / 64 /
# 256 / 1024 / 4096 -> 633 / 487 / 462 / 506 / 832 ms). It rests on ONE scene (the Cornell box at 1024 x 1024, one tolerance). The C ABI has no default:
# hpt_adaptive_params.step below 1 is HPT_ERR_ARG.
ADAPTIVE_STEP_DEFAULT = 256


class ADAPTIVE_PARAMS(C.Structure):
    """hpt_adaptive_params (include/hydra_hip.h): 6 dwords. tol and the pass limits are the caller's; step defaults to ADAPTIVE_STEP_DEFAULT."""
    _fields_ = [("tol", _f), ("lumFloor", _f), ("minPasses", _u32), ("maxPasses", _u32), ("step", _u32), ("dilate", _u32)]

# hpt_gbuffer_pixel = Integrator::GBufferPixel (integrator_pt.h:187-198): 15 dwords
GBUFFER_SAMPLES = 16
GBUFFER_DTYPE = np.dtype([("depth", np.float32), ("norm", np.float32, (3,)), ("texc", np.float32, (2,)), ("rgba", np.float32, (4,)),
                          ("shadow", np.float32), ("coverage", np.float32), ("matId", np.int32), ("objId", np.int32), ("instId", np.int32)])
assert GBUFFER_DTYPE.itemsize == 60

# the single-level tree as hpt_read_accel returns it (hpt_types.h: BvhNode, BvhTri)
BVH_NODE_DTYPE = np.dtype([("q", np.float32, (12,)), ("ref0", np.uint32), ("ref1", np.uint32), ("pad0", np.uint32), ("pad1", np.uint32)])
BVH_TRI_DTYPE = np.dtype([("v0", np.float32, (3,)), ("primId", np.uint32), ("e1", np.float32, (3,)), ("instId", np.uint32), ("e2", np.float32, (3,)), ("pad1", np.uint32)])
assert BVH_NODE_DTYPE.itemsize == 64 and BVH_TRI_DTYPE.itemsize == 48
# the instance records of the two-level layout as hpt_read_accel_two_level returns them (hpt_types.h: BvhInst)
BVH_INST_DTYPE = np.dtype([("rows", np.float32, (3, 4)), ("root", np.uint32), ("geomId", np.uint32), ("moving", np.uint32), ("pad1", np.uint32)])
assert BVH_INST_DTYPE.itemsize == 64



class DENOISE_PARAMS(C.Structure):
    """hpt_denoise_params (include/hydra_hip.h): 7 dwords."""
    _fields_ = [("iterations", _u32), ("normalSquarings", _u32), ("flags", _u32),
                ("normConst", _f), ("sigmaColor", _f), ("sigmaDepth", _f), ("sigmaAlbedo", _f)]


DENOISE_DEMODULATE = 1
# the defaults of HipIntegrator.denoise, as the header states them (chosen on the quality check of profiles/denoise.md)
DENOISE_DEFAULTS = {"iterations": 5, "normal_squarings": 7, "sigma_color": 0.6, "sigma_depth": 0.05, "sigma_albedo": 0.1, "demodulate": True}


class DENOISE_VAR_PARAMS(C.Structure):
    """hpt_denoise_var_params (include/hydra_hip.h): 4 dwords."""
    _fields_ = [("sigmaLum", _f), ("varFloor", _f), ("prefilter", _u32), ("reserved", _u32)]


# the defaults of HipIntegrator.denoise_var (chosen on the quality check of profiles/denoise_var.md); the other parameters: DENOISE_DEFAULTS, sigma_color 0
DENOISE_VAR_DEFAULTS = {"sigma_lum": 2.0, "var_floor": 1e-4, "prefilter": True}

_LIB = None


class HydraHipError(RuntimeError):
    pass


def load_library():
    """dlopen the in-tree HIP library and bind every ABI symbol; raises if it has not been built."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise HydraHipError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                                "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in ABI.items():
            fn = getattr(lib, name)          # AttributeError if the library lacks a declared symbol
            fn.restype, fn.argtypes = res, args
        _LIB = lib
    return _LIB


def qmc_table():
    """qmc::init (mlt/rnd_qmc.cpp): the 11 x 31 Niederreiter base-2 table, uint32 [11, 31]. Host code: needs the library, no GPU."""
    out = np.zeros((11, 31), np.uint32)
    if load_library().hpt_qmc_table(out.ctypes.data) != 0:
        raise HydraHipError("hpt_qmc_table failed")
    return out


def qmc_layout(dof, spectral, motion):
    """IntegratorQMC::EnableQMC: the dimension offsets {"dof", "spd", "motion", "mat", "lgt"} of a scene with these features (0 = pseudo)."""
    out = np.zeros(5, np.uint32)
    if load_library().hpt_qmc_layout(int(bool(dof)), int(bool(spectral)), int(bool(motion)), out.ctypes.data) != 0:
        raise HydraHipError("hpt_qmc_layout failed")
    return dict(zip(("dof", "spd", "motion", "mat", "lgt"), (int(v) for v in out)))


def qmc_sample_count(pixels_num, pass_num):
    """Samples of one PathTraceBlockQMC call: min(2^32 - 1, pixelsNum * a_passNum)."""
    return int(load_library().hpt_qmc_sample_count(pixels_num, pass_num))


def kmlt_state_size(trace_depth):
    """IntegratorKMLT's m_randsPerThread: AlignedSize(10 * traceDepth + 6, 16) floats per primary-sample-space vector. Host code: no GPU."""
    return int(load_library().hpt_kmlt_state_size(trace_depth))


class KmltRecords(C.Structure):
    """hpt_kmlt_records: device pointers, each may be null."""
    _fields_ = [(n, _vp) for n in ("isLarge", "accepted", "a", "color", "pixel", "oldPixel", "initColor", "initPixel", "proposals", "contribAtX", "contribAtY")]


COUNTER_NAMES = ("rays", "nodes", "tris", "surface_hits", "shadow_rays", "paths", "instances_entered", "tex_fetches",
                 "cyc_queue_regen", "cyc_trace_nearest", "cyc_shade", "cyc_trace_shadow", "cyc_path_end", "loop_trips", "wave_node_iters", "wave_tri_iters")


class DevArray:
    """A float32 array in HBM owned through the C ABI's hpt_device_* helpers (tests and tools that do not link the HIP runtime)."""

    def __init__(self, integ, ptr, shape):
        self.integ, self.ptr, self.shape = integ, ptr, tuple(shape)
        self.size = int(np.prod(self.shape)) if self.shape else 1
        self.nbytes = self.size * 4

    def upload(self, host):
        host = np.ascontiguousarray(host, np.float32)
        assert host.size == self.size
        self.integ._chk(self.integ.L.hpt_device_copy(self.integ.h, self.ptr, host.ctypes.data, self.nbytes, 1))

    def download(self):
        out = np.zeros(self.shape, np.float32)
        self.integ._chk(self.integ.L.hpt_device_copy(self.integ.h, out.ctypes.data, self.ptr, self.nbytes, 2))
        return out

    def free(self):
        if self.ptr:
            self.integ._chk(self.integ.L.hpt_device_free(self.integ.h, self.ptr))
            self.ptr = None


class HipIntegrator:
    """Integrator-shaped front end of the HIP core. One instance = one hpt_ctx = one GPU."""

    def __init__(self, scene: SceneData = None, params: Params = None, device: int = 0, accel_layout: int = 0):
        self.L = load_library()
        h = _vp()
        rc = self.L.hpt_create(device, C.byref(h))
        if rc != 0:
            raise HydraHipError(f"hpt_create(device={device}) failed with code {rc}: no usable MI355X / HIP device")
        self.h = h
        self.device = device
        self.grad_size = 0               # floats of a_data the registered differentiable textures occupy (PutDiffTex2D)
        self.scene = None
        self.params = None
        self.W = self.H = self.N = 0
        self._qmc_spectral = False       # set_option("qmc_spectral", 1) was called
        if accel_layout:
            self._chk(self.L.hpt_set_accel_layout(self.h, accel_layout))   # 1 = two-level TLAS/BLAS, 2 = single-level, 3 = triangle sweep (tiny scenes)
        if scene is not None:
            self.LoadScene(scene, params)

    def __del__(self):
        try:
            if getattr(self, "h", None):
                self.L.hpt_destroy(self.h)
                self.h = None
        except Exception:
            pass

    def _chk(self, rc):
        if rc != 0:
            raise HydraHipError(f"hydra_hip error {rc}: {self.L.hpt_last_error(self.h).decode()}")

    # ---- LoadScene / CommitDeviceData / UpdateMembersPlainData / PackXYBlock (main.cpp:249-267) ---------------------
    def LoadScene(self, scene: SceneData, params: Params = None):
        self.scene = scene
        self._desc = scene.desc()
        self.CommitDeviceData()
        self.UpdateMembersPlainData(params if params is not None else scene.params())
        lines = np.ascontiguousarray(scene.lens_lines, np.float32).reshape(-1, 4)       # m_lines / m_physSize (lens simulation; none: off)
        self._chk(self.L.hpt_set_optics(self.h, lines.ctypes.data if lines.size else None, lines.shape[0], float(scene.phys_size[0]), float(scene.phys_size[1])))
        self.PackXYBlock(self.W, self.H, 1)
        self.InitRandomGens(self.N)

    def CommitDeviceData(self):
        self._chk(self.L.hpt_upload_scene(self.h, C.byref(self._desc)))

    def UpdateMembersPlainData(self, params: Params):
        self.params = params
        self._chk(self.L.hpt_update_params(self.h, C.byref(params)))
        self.W, self.H = params.winWidth, params.winHeight
        self.N = self.W * self.H

    def PackXYBlock(self, tidX, tidY, a_passNum=1):
        self._chk(self.L.hpt_pack_xy(self.h, tidX, tidY))

    def InitRandomGens(self, a_maxThreads, first_seed=0):
        """Integrator::InitRandomGens; first_seed != 0 seeds the generators as threads first_seed.. of one larger call (sample sharding)."""
        self._chk(self.L.hpt_init_random_gens_from(self.h, a_maxThreads, first_seed))

    def packed_xy(self):
        out = np.zeros(self.N, np.uint32)
        self._chk(self.L.hpt_get_packed_xy(self.h, out.ctypes.data, self.N))
        return out

    def random_gens(self):
        out = np.zeros((self.N, 2), np.uint32)
        self._chk(self.L.hpt_get_random_gens(self.h, out.ctypes.data, self.N))
        return out

    def set_random_gens(self, gens):
        gens = np.ascontiguousarray(gens, np.uint32).reshape(-1, 2)      # one uint2 per thread
        self._chk(self.L.hpt_set_random_gens(self.h, gens.ctypes.data, gens.shape[0]))

    def Update_m_materials(self, first, mats):
        mats = np.ascontiguousarray(mats)
        self._chk(self.L.hpt_update_materials(self.h, first, mats.size, mats.ctypes.data))

    def Update_m_lights(self, first, lights):
        lights = np.ascontiguousarray(lights)
        self._chk(self.L.hpt_update_lights(self.h, first, lights.size, lights.ctypes.data))

    def Update_m_matIdOffsets(self, mat_vert_offset):
        """Integrator::Update_m_matIdOffsets (integrator_pt.h:470): re-upload m_matVertOffset (uint32 [numGeoms, 2])."""
        mvo = np.ascontiguousarray(mat_vert_offset, np.uint32)
        self._chk(self.L.hpt_update_mat_id_offsets(self.h, mvo.ctypes.data, mvo.size // 2))

    # ---- the hot path -----------------------------------------------------------------------------------------------
    def PathTraceBlock(self, tid, channels, out_color, a_passNum, tid_begin=0):
        """Integrator::PathTraceBlock(tid, channels, out_color, a_passNum); `tid` = number of threads (pixels)."""
        assert out_color.dtype == np.float32 and out_color.flags["C_CONTIGUOUS"]
        self._chk(self.L.hpt_path_trace_block(self.h, tid_begin, tid, channels, out_color.ctypes.data, a_passNum))

    def NaivePathTraceBlock(self, tid, channels, out_color, a_passNum, tid_begin=0):
        assert out_color.dtype == np.float32 and out_color.flags["C_CONTIGUOUS"]
        self._chk(self.L.hpt_naive_path_trace_block(self.h, tid_begin, tid, channels, out_color.ctypes.data, a_passNum))

    def path_trace_block_dev(self, dev_ptr, pass_num, tid_begin=0, tid_count=None, channels=4, naive=False, stream=None):
        tid_count = self.N - tid_begin if tid_count is None else tid_count
        self._chk(self.L.hpt_path_trace_block_dev(self.h, tid_begin, tid_count, channels, dev_ptr, pass_num, int(naive), stream))

    # ---- adaptive sampling (no counterpart in the reference) ---------------------------------------------
    @staticmethod
    def _adaptive_params(params=None, **kw):
        return params if params is not None else ADAPTIVE_PARAMS(float(kw["tol"]), float(kw["lum_floor"]), int(kw["min_passes"]), int(kw["max_passes"]),
                                                                 int(kw.get("step", ADAPTIVE_STEP_DEFAULT)), int(kw.get("dilate", 0)))

    @staticmethod
    def _info(rec):
        return {k: (float(rec[k]) if k == "deviceMs" else int(rec[k])) for k in ("passes", "pixels", "maxPasses", "nonfinite", "rounds", "deviceMs")}

    def PathTraceBlockCounts(self, tid, channels, out_color, a_passNum, pass_counts=None, moments=None, tid_begin=0):
        """PathTraceBlock with pass_counts[tid] passes for pixel tid (uint32 [winWidth * winHeight], absolute tid; None: a_passNum everywhere) and,
        with moments (MOMENTS_DTYPE [winWidth * winHeight]), every sample's luminance added to the pixel's record. Both arrays are updated in place."""
        assert out_color.dtype == np.float32 and out_color.flags["C_CONTIGUOUS"]
        assert pass_counts is None or (pass_counts.dtype == np.uint32 and pass_counts.flags["C_CONTIGUOUS"] and pass_counts.size == self.N)
        assert moments is None or (moments.dtype == MOMENTS_DTYPE and moments.flags["C_CONTIGUOUS"] and moments.size == self.N)
        self._chk(self.L.hpt_path_trace_block_counts(self.h, tid_begin, tid, channels, out_color.ctypes.data, a_passNum,
                                                     None if pass_counts is None else pass_counts.ctypes.data, None if moments is None else moments.ctypes.data))

    def PathTraceBlockCounts_dev(self, dev_ptr, pass_num, counts_ptr=None, moments_ptr=None, tid_begin=0, tid_count=None, channels=4, naive=False, stream=None):
        tid_count = self.N - tid_begin if tid_count is None else tid_count
        self._chk(self.L.hpt_path_trace_block_counts_dev(self.h, tid_begin, tid_count, channels, dev_ptr, pass_num, int(naive), counts_ptr, moments_ptr, stream))

    def AdaptivePlan(self, moments, tid=None, tid_begin=0, params=None, **kw):
        """The planner: (pass counts uint32 [winWidth * winHeight] with the window filled in, totals as a dict). kw: tol, lum_floor, min_passes,
        max_passes, step (default ADAPTIVE_STEP_DEFAULT), dilate (default 0)."""
        assert moments.dtype == MOMENTS_DTYPE and moments.flags["C_CONTIGUOUS"] and moments.size == self.N
        p = self._adaptive_params(params, **kw)
        counts, info = np.zeros(self.N, np.uint32), np.zeros(1, ADAPTIVE_INFO_DTYPE)
        self._chk(self.L.hpt_adaptive_plan(self.h, tid_begin, self.N - tid_begin if tid is None else tid, C.byref(p), moments.ctypes.data, counts.ctypes.data, info.ctypes.data))
        return counts, self._info(info[0])

    def AdaptivePlan_dev(self, moments_ptr, counts_ptr, info_ptr, tid=None, tid_begin=0, params=None, stream=None, **kw):
        p = self._adaptive_params(params, **kw)
        self._chk(self.L.hpt_adaptive_plan_dev(self.h, tid_begin, self.N - tid_begin if tid is None else tid, C.byref(p), moments_ptr, counts_ptr, info_ptr, stream))

    def AdaptiveResolve(self, frame, moments, out=None, tid=None, tid_begin=0):
        """frame / passes per pixel for the first three channels (a pixel without passes: 0; a fourth channel: copied). out None: in place."""
        assert frame.dtype == np.float32 and frame.flags["C_CONTIGUOUS"] and frame.size % self.N == 0
        assert moments.dtype == MOMENTS_DTYPE and moments.flags["C_CONTIGUOUS"] and moments.size == self.N
        out = frame if out is None else out
        assert out.dtype == np.float32 and out.flags["C_CONTIGUOUS"] and out.size == frame.size
        self._chk(self.L.hpt_adaptive_resolve(self.h, tid_begin, self.N - tid_begin if tid is None else tid, frame.size // self.N, frame.ctypes.data, moments.ctypes.data, out.ctypes.data))
        return out

    def AdaptiveResolve_dev(self, frame_ptr, moments_ptr, out_ptr, channels=4, tid=None, tid_begin=0, stream=None):
        self._chk(self.L.hpt_adaptive_resolve_dev(self.h, tid_begin, self.N - tid_begin if tid is None else tid, channels, frame_ptr, moments_ptr, out_ptr, stream))

    def AdaptiveVariance(self, moments, tid=None, tid_begin=0, out=None):
        """The variance plane denoise_var reads: float32 [winHeight, winWidth], the estimated variance of each window pixel's mean luminance
        (DESIGN.md 2.12b). out None: a plane of zeros is written into; pixels outside the window keep their contents."""
        assert moments.dtype == MOMENTS_DTYPE and moments.flags["C_CONTIGUOUS"] and moments.size == self.N
        out = np.zeros((self.H, self.W), np.float32) if out is None else out
        assert out.dtype == np.float32 and out.flags["C_CONTIGUOUS"] and out.size == self.N
        self._chk(self.L.hpt_adaptive_variance(self.h, tid_begin, self.N - tid_begin if tid is None else tid, moments.ctypes.data, out.ctypes.data))
        return out

    def AdaptiveVariance_dev(self, moments_ptr, out_ptr, tid=None, tid_begin=0, stream=None):
        self._chk(self.L.hpt_adaptive_variance_dev(self.h, tid_begin, self.N - tid_begin if tid is None else tid, moments_ptr, out_ptr, stream))

    def PathTraceBlockAdaptive(self, tid, channels, out_color, max_rounds, moments=None, tid_begin=0, params=None, **kw):
        """The adaptive loop: min_passes everywhere, then up to max_rounds rounds of plan + render. out_color is accumulated into (un-normalised);
        moments, when given, receives the window's records (zeroed first). Returns the loop's report as a dict."""
        assert out_color.dtype == np.float32 and out_color.flags["C_CONTIGUOUS"] and out_color.size == self.N * channels
        assert moments is None or (moments.dtype == MOMENTS_DTYPE and moments.flags["C_CONTIGUOUS"] and moments.size == self.N)
        p = self._adaptive_params(params, **kw)
        info = np.zeros(1, ADAPTIVE_INFO_DTYPE)
        self._chk(self.L.hpt_path_trace_block_adaptive(self.h, tid_begin, tid, channels, out_color.ctypes.data, C.byref(p), max_rounds,
                                                       None if moments is None else moments.ctypes.data, info.ctypes.data))
        return self._info(info[0])

    def PathTraceBlockAdaptive_dev(self, dev_ptr, max_rounds, moments_ptr=None, tid_begin=0, tid_count=None, channels=4, params=None, stream=None, **kw):
        p = self._adaptive_params(params, **kw)
        info = np.zeros(1, ADAPTIVE_INFO_DTYPE)
        self._chk(self.L.hpt_path_trace_block_adaptive_dev(self.h, tid_begin, self.N - tid_begin if tid_count is None else tid_count, channels, dev_ptr, C.byref(p),
                                                           max_rounds, moments_ptr, info.ctypes.data, stream))
        return self._info(info[0])

    def PathTraceFromInputRaysBlock(self, tid, channels, in_rayPosAndNear, in_rayDirAndFar, out_color, a_passNum):
        """Integrator::PathTraceFromInputRaysBlock; rays: float32 [tid, 4] (RayPosAndW / RayDirAndT), camera space."""
        for a in (in_rayPosAndNear, in_rayDirAndFar, out_color):
            assert a.dtype == np.float32 and a.flags["C_CONTIGUOUS"]
        self._chk(self.L.hpt_path_trace_from_input_rays_block(self.h, tid, channels, in_rayPosAndNear.ctypes.data, in_rayDirAndFar.ctypes.data, out_color.ctypes.data, a_passNum))

    def CastSingleRayBlock(self, tid, out_color, a_passNum=1):
        """Integrator::CastSingleRayBlock(tid, out_color, a_passNum) (integrator_pt.h:254): out_color float32 [winHeight, winWidth, 4]; the
        first tid pixels of m_packedXY are ASSIGNED (base colour x texture, fourth float 0; a miss: four zeros), the others keep their contents."""
        assert out_color.dtype == np.float32 and out_color.flags["C_CONTIGUOUS"] and out_color.size == self.N * 4
        self._chk(self.L.hpt_cast_single_ray_block(self.h, tid, out_color.ctypes.data, a_passNum))

    def RayTraceBlock(self, tid, channels, out_color, a_passNum=1):
        """Integrator::RayTraceBlock(tid, channels, out_color, a_passNum) (integrator_pt.h:263): one Whitted path per pixel, ADDED to the first three
        of the pixel's `channels` floats. channels 3 or 4; 1 and 2 raise; above 4 nothing is written (out_color may then be any float32 array)."""
        assert out_color.dtype == np.float32 and out_color.flags["C_CONTIGUOUS"] and (channels not in (3, 4) or out_color.size == self.N * channels)
        self._chk(self.L.hpt_ray_trace_block(self.h, tid, channels, out_color.ctypes.data, a_passNum))

    def cast_single_ray_block_dev(self, dev_ptr, tid=None, pass_num=1, stream=None):
        """CastSingleRayBlock on a device frame of winWidth * winHeight * 4 floats; asynchronous on `stream`."""
        self._chk(self.L.hpt_cast_single_ray_block_dev(self.h, self.N if tid is None else tid, dev_ptr, pass_num, stream))

    def ray_trace_block_dev(self, dev_ptr, tid=None, channels=4, pass_num=1, stream=None):
        """RayTraceBlock on a device frame of winWidth * winHeight * channels floats; asynchronous on `stream`."""
        self._chk(self.L.hpt_ray_trace_block_dev(self.h, self.N if tid is None else tid, channels, dev_ptr, pass_num, stream))

    # ---- IntegratorQMC (mlt/integrator_qmc.cpp) -----------------------------------------------------------------------
    def PathTraceBlockQMC(self, pixelsNum, channels, out_color, a_passNum):
        """IntegratorQMC::PathTraceBlock(pixelsNum, channels, out_color, a_passNum): min(2^32 - 1, pixelsNum * a_passNum) samples of the
        Niederreiter sequence, each ADDED (float atomics) to the pixel its first two dimensions select; out_color float32 [winHeight, winWidth, channels].
        After set_option("qmc_spectral", 1) a spectral scene is served; channels above 4 are then wavelength layers: out_color float32
        [channels, winHeight, winWidth] (without the option the library refuses them, whatever the array's size)."""
        served = channels in (1, 3, 4) or (channels > 4 and self._qmc_spectral)
        assert out_color.dtype == np.float32 and out_color.flags["C_CONTIGUOUS"] and (not served or out_color.size == self.N * channels)
        self._chk(self.L.hpt_path_trace_qmc_block(self.h, pixelsNum, channels, out_color.ctypes.data, a_passNum))

    def path_trace_qmc_block_dev(self, dev_ptr, pass_num, pixels_num=None, channels=4, sample_color_ptr=None, sample_pixel_ptr=None, stream=None,
                                 sample_waves_ptr=None):
        """PathTraceBlockQMC on a device frame (may be None when both record pointers are given); asynchronous on `stream`. sample_waves_ptr: the
        third record of spectral QMC (hpt_path_trace_qmc_block_dev2), four wavelengths per sample."""
        if sample_waves_ptr is not None:
            self._chk(self.L.hpt_path_trace_qmc_block_dev2(self.h, self.N if pixels_num is None else pixels_num, channels, dev_ptr, pass_num,
                                                           sample_color_ptr, sample_pixel_ptr, sample_waves_ptr, stream))
            return
        self._chk(self.L.hpt_path_trace_qmc_block_dev(self.h, self.N if pixels_num is None else pixels_num, channels, dev_ptr, pass_num,
                                                      sample_color_ptr, sample_pixel_ptr, stream))

    def render_qmc(self, spp, channels=4, frame=True, records=False, pixels_num=None, waves=False):
        """One PathTraceBlockQMC call through the device-pointer form. Returns (frame or None, colours [S, 4] or None, pixel indices [S] or None):
        the frame is the atomic sum (zeros before the call), the records are the per-sample values in sample order. waves=True (spectral QMC,
        implies records): a fourth element, the samples' wavelengths [S, 4]. channels above 4: the frame is [channels, H, W] wavelength layers
        and a colour record is the sample's four exposure * accumColor[i]."""
        pixels_num = self.N if pixels_num is None else pixels_num
        records = records or waves
        S = qmc_sample_count(pixels_num, spp)
        img = np.zeros((self.H, self.W, channels) if channels <= 4 else (channels, self.H, self.W), np.float32) if frame else None
        col = np.zeros((S, 4), np.float32) if records else None
        pix = np.zeros(S, np.uint32) if records else None
        wav = np.zeros((S, 4), np.float32) if waves else None
        ptrs = []

        def dev(nbytes):
            p = _vp()
            self._chk(self.L.hpt_device_malloc(self.h, max(nbytes, 16), C.byref(p)))
            ptrs.append(p)
            return p
        try:
            d_img = dev(img.nbytes) if frame else None
            d_col = dev(col.nbytes) if records else None
            d_pix = dev(pix.nbytes) if records else None
            d_wav = dev(wav.nbytes) if waves else None
            if frame:
                self._chk(self.L.hpt_device_copy(self.h, d_img, img.ctypes.data, img.nbytes, 1))
            self.path_trace_qmc_block_dev(d_img, spp, pixels_num, channels, d_col, d_pix, sample_waves_ptr=d_wav)
            if frame:
                self._chk(self.L.hpt_device_copy(self.h, img.ctypes.data, d_img, img.nbytes, 2))
            if records:
                self._chk(self.L.hpt_device_copy(self.h, col.ctypes.data, d_col, col.nbytes, 2))
                self._chk(self.L.hpt_device_copy(self.h, pix.ctypes.data, d_pix, pix.nbytes, 2))
            if waves:
                self._chk(self.L.hpt_device_copy(self.h, wav.ctypes.data, d_wav, wav.nbytes, 2))
        finally:
            for p in ptrs:
                self.L.hpt_device_free(self.h, p)
        return (img, col, pix, wav) if waves else (img, col, pix)

    # ---- IntegratorKMLT (mlt/integrator_kmlt.cpp) ---------------------------------------------------------------------
    def _dev_scope(self):
        """(alloc, free_all) over hpt_device_malloc: alloc(nbytes) -> device pointer."""
        ptrs = []

        def dev(nbytes):
            p = _vp()
            self._chk(self.L.hpt_device_malloc(self.h, max(int(nbytes), 16), C.byref(p)))
            ptrs.append(p)
            return p

        def free_all():
            for p in ptrs:
                self.L.hpt_device_free(self.h, p)
        return dev, free_all

    def path_trace_pss(self, x, waves=False, accum=False):
        """IntegratorKMLT::PathTraceF for the vectors x, float32 [n, stride] with stride >= kmlt_state_size(traceDepth): returns
        (colours float32 [n, 4], pixel indices uint32 [n]). Every random number of path i is read from x[i]; m_randomGens is not touched.
        Spectral MLT (set_option("kmlt_spectral", 1) on a spectral scene): waves=True appends the paths' wavelengths [n, 4], accum=True their
        raw exposure * accumColor [n, 4] (hpt_path_trace_pss_dev2), in that order."""
        x = np.ascontiguousarray(x, np.float32)
        assert x.ndim == 2
        n, stride = x.shape
        col, pix = np.zeros((n, 4), np.float32), np.zeros(n, np.uint32)
        extra = [np.zeros((n, 4), np.float32) if want else None for want in (waves, accum)]
        dev, free_all = self._dev_scope()
        try:
            d_x, d_col, d_pix = dev(x.nbytes), dev(col.nbytes), dev(pix.nbytes)
            d_extra = [dev(e.nbytes) if e is not None else None for e in extra]
            if n:
                self._chk(self.L.hpt_device_copy(self.h, d_x, x.ctypes.data, x.nbytes, 1))
            if waves or accum:
                self._chk(self.L.hpt_path_trace_pss_dev2(self.h, d_x, n, stride, d_col, d_pix, d_extra[0], d_extra[1], None))
            else:
                self._chk(self.L.hpt_path_trace_pss_dev(self.h, d_x, n, stride, d_col, d_pix, None))
            if n:
                self._chk(self.L.hpt_device_copy(self.h, col.ctypes.data, d_col, col.nbytes, 2))
                self._chk(self.L.hpt_device_copy(self.h, pix.ctypes.data, d_pix, pix.nbytes, 2))
                for e, d in zip(extra, d_extra):
                    if e is not None:
                        self._chk(self.L.hpt_device_copy(self.h, e.ctypes.data, d, e.nbytes, 2))
        finally:
            free_all()
        return (col, pix) + tuple(e for e in extra if e is not None)

    def PathTraceBlockKMLT(self, pixelsNum, channels, out_color, a_passNum):
        """IntegratorKMLT::PathTraceBlock(pixelsNum, channels, out_color, a_passNum): Markov chains in primary sample space, then the brightness
        normalisation; out_color float32 [winHeight, winWidth, 4], zero-filled by the caller."""
        assert out_color.dtype == np.float32 and out_color.flags["C_CONTIGUOUS"] and (channels != 4 or out_color.size == self.N * 4)
        self._chk(self.L.hpt_path_trace_kmlt_block(self.h, pixelsNum, channels, out_color.ctypes.data, a_passNum))

    def kmlt_chain_count(self, spp, pixels_num=None):
        """(C, steps) of a PathTraceBlockKMLT call made now: the library's answer (hpt_kmlt_chain_count) for the option "kmlt_chains" or the
        default, one chain per lane of the resident grid, at most pixelsNum * spp. Raises where the call would refuse the chain count."""
        chains, steps = _u32(0), _u32(0)
        self._chk(self.L.hpt_kmlt_chain_count(self.h, self.N if pixels_num is None else pixels_num, spp, C.byref(chains), C.byref(steps)))
        return int(chains.value), int(steps.value)

    def render_kmlt(self, spp, chains=None, normalize=True, records=False, proposals=False, unnormalised=False):
        """One PathTraceBlockKMLT call through the device-pointer form, on a zero-filled frame. chains: sets the option "kmlt_chains" (None: as the
        context has it). Returns a dict: "frame" [H, W, 4]; "stats" = [avgBrightness, actualBrightness, acceptance rate, normConst]; "chains",
        "steps"; with records: "isLarge", "accepted" (uint8 [C, steps]), "a" [C, steps], "color" [C, steps, 4], "pixel", "oldPixel" (uint32
        [C, steps]), "initColor" [C, 4], "initPixel" [C], "contribAtX", "contribAtY" [C, steps, 4] (.w: 1 when added to the frame); with proposals: "proposals" [C, steps, state size]; with unnormalised (and normalize):
        "frame_unnormalised", the raw sums of the same run (the normalisation is then made by a second call, normalize = 2)."""
        if chains is not None:
            self.set_option("kmlt_chains", int(chains))
        Cn, steps = self.kmlt_chain_count(spp)                   # the record arrays are sized by what the library will run
        n = kmlt_state_size(self.params.traceDepth)
        img = np.zeros((self.H, self.W, 4), np.float32)
        stats = np.zeros(4, np.float64)
        host = {}
        if records:
            host.update(isLarge=np.zeros((Cn, steps), np.uint8), accepted=np.zeros((Cn, steps), np.uint8), a=np.zeros((Cn, steps), np.float32),
                        color=np.zeros((Cn, steps, 4), np.float32), pixel=np.zeros((Cn, steps), np.uint32), oldPixel=np.zeros((Cn, steps), np.uint32),
                        initColor=np.zeros((Cn, 4), np.float32), initPixel=np.zeros(Cn, np.uint32),
                        contribAtX=np.zeros((Cn, steps, 4), np.float32), contribAtY=np.zeros((Cn, steps, 4), np.float32))
        if proposals:
            host["proposals"] = np.zeros((Cn, steps, n), np.float32)
        out = {"chains": Cn, "steps": steps}
        dev, free_all = self._dev_scope()
        try:
            d_img, d_stats = dev(img.nbytes), dev(stats.nbytes)
            self._chk(self.L.hpt_device_copy(self.h, d_img, img.ctypes.data, img.nbytes, 1))
            rec = KmltRecords()
            d_rec = {k: dev(v.nbytes) for k, v in host.items()}
            for k, p in d_rec.items():
                setattr(rec, k, p)
            two = bool(normalize) and unnormalised
            self._chk(self.L.hpt_path_trace_kmlt_block_dev(self.h, self.N, 4, d_img, spp, 0 if two else int(bool(normalize)), C.byref(rec) if host else None, d_stats, None))
            if two:
                raw = np.zeros_like(img)
                self._chk(self.L.hpt_device_copy(self.h, raw.ctypes.data, d_img, img.nbytes, 2))
                out["frame_unnormalised"] = raw
                self._chk(self.L.hpt_path_trace_kmlt_block_dev(self.h, self.N, 4, d_img, spp, 2, None, d_stats, None))
            self._chk(self.L.hpt_device_copy(self.h, img.ctypes.data, d_img, img.nbytes, 2))
            self._chk(self.L.hpt_device_copy(self.h, stats.ctypes.data, d_stats, stats.nbytes, 2))
            for k, v in host.items():
                if v.nbytes:
                    self._chk(self.L.hpt_device_copy(self.h, v.ctypes.data, d_rec[k], v.nbytes, 2))
        finally:
            free_all()
        out.update(frame=img, stats=stats, **host)
        return out

    def render(self, spp, channels=4, naive=False):
        img = np.zeros((self.H, self.W, channels), np.float32)
        (self.NaivePathTraceBlock if naive else self.PathTraceBlock)(self.N, channels, img, spp)
        return img

    def EvalGBuffer(self, blockNum=None, samples=False, out=None):
        """Integrator::EvalGBuffer(blockNum, out_gbuffer) (integrator_pt.h:251): a GBUFFER_DTYPE array [winHeight, winWidth]; the records of
        pixels past blockNum (in m_packedXY order) keep what `out` held (zeros without `out`). samples=True also returns the [blockNum, 16]
        records of the single samples as they are before the reduction (device-pointer form of the call)."""
        blockNum = self.N if blockNum is None else int(blockNum)
        if out is None:
            out = np.zeros((self.H, self.W), GBUFFER_DTYPE)
        assert out.dtype == GBUFFER_DTYPE and out.flags["C_CONTIGUOUS"] and out.size == self.N
        if not samples:
            self._chk(self.L.hpt_eval_gbuffer(self.h, blockNum, out.ctypes.data))
            return out
        raw = np.zeros((blockNum, GBUFFER_SAMPLES), GBUFFER_DTYPE)
        d_out, d_raw = _vp(), _vp()
        self._chk(self.L.hpt_device_malloc(self.h, out.nbytes, C.byref(d_out)))
        try:
            self._chk(self.L.hpt_device_malloc(self.h, max(raw.nbytes, 60), C.byref(d_raw)))
            try:
                self._chk(self.L.hpt_device_copy(self.h, d_out, out.ctypes.data, out.nbytes, 1))
                self._chk(self.L.hpt_eval_gbuffer_dev(self.h, blockNum, d_out, d_raw, None))
                self._chk(self.L.hpt_device_copy(self.h, out.ctypes.data, d_out, out.nbytes, 2))      # synchronous copies on the null stream: after the kernel
                if raw.nbytes:
                    self._chk(self.L.hpt_device_copy(self.h, raw.ctypes.data, d_raw, raw.nbytes, 2))
            finally:
                self.L.hpt_device_free(self.h, d_raw)
        finally:
            self.L.hpt_device_free(self.h, d_out)
        return out, raw

    @staticmethod
    def denoise_params(norm_const=1.0, iterations=None, normal_squarings=None, sigma_color=None, sigma_depth=None, sigma_albedo=None, demodulate=None):
        """A DENOISE_PARAMS; None takes the default of DENOISE_DEFAULTS."""
        d = DENOISE_DEFAULTS
        pick = lambda v, k: d[k] if v is None else v
        return DENOISE_PARAMS(int(pick(iterations, "iterations")), int(pick(normal_squarings, "normal_squarings")),
                              DENOISE_DEMODULATE if pick(demodulate, "demodulate") else 0, float(norm_const),
                              float(pick(sigma_color, "sigma_color")), float(pick(sigma_depth, "sigma_depth")), float(pick(sigma_albedo, "sigma_albedo")))

    def denoise(self, frame, gbuffer=None, norm_const=1.0, iterations=None, normal_squarings=None, sigma_color=None, sigma_depth=None,
                sigma_albedo=None, demodulate=None):
        """DenoiseFrame: the a-trous filter over frame, float32 [height, width, 4] (scaled by norm_const, e.g. 1 / spp), guided by
        gbuffer, a GBUFFER_DTYPE array [height, width]; None: EvalGBuffer() of the loaded scene. Returns a new float32 [height, width, 4]."""
        frame = np.ascontiguousarray(frame, np.float32)
        assert frame.ndim == 3 and frame.shape[2] == 4
        if gbuffer is None:
            gbuffer = self.EvalGBuffer()
        gbuffer = np.ascontiguousarray(gbuffer)
        assert gbuffer.dtype == GBUFFER_DTYPE and gbuffer.shape == frame.shape[:2]
        p = self.denoise_params(norm_const, iterations, normal_squarings, sigma_color, sigma_depth, sigma_albedo, demodulate)
        out = np.zeros_like(frame)
        self._chk(self.L.hpt_denoise_frame(self.h, frame.shape[1], frame.shape[0], frame.ctypes.data, gbuffer.ctypes.data, C.byref(p), out.ctypes.data))
        return out

    def denoise_dev(self, color_ptr, gbuffer_ptr, out_ptr, width=None, height=None, params=None, stream=None, **kw):
        """DenoiseFrame on device pointers (frame of width * height * 4 floats, width * height G-buffer records, output frame); asynchronous on
        `stream`. params: a DENOISE_PARAMS, or the keyword arguments of denoise_params."""
        p = params if params is not None else self.denoise_params(**kw)
        self._chk(self.L.hpt_denoise_frame_dev(self.h, self.W if width is None else width, self.H if height is None else height,
                                               color_ptr, gbuffer_ptr, C.byref(p), out_ptr, stream))

    @staticmethod
    def denoise_var_params(sigma_lum=None, var_floor=None, prefilter=None):
        """A DENOISE_VAR_PARAMS; None takes the default of DENOISE_VAR_DEFAULTS."""
        d = DENOISE_VAR_DEFAULTS
        pick = lambda v, k: d[k] if v is None else v
        return DENOISE_VAR_PARAMS(float(pick(sigma_lum, "sigma_lum")), float(pick(var_floor, "var_floor")), 1 if pick(prefilter, "prefilter") else 0, 0)

    def denoise_var(self, frame, variance, gbuffer=None, norm_const=1.0, iterations=None, normal_squarings=None, sigma_depth=None, sigma_albedo=None,
                    demodulate=None, sigma_lum=None, var_floor=None, prefilter=True, return_variance=False):
        """DenoiseFrameVar: denoise() with a luminance stop scaled by `variance`, float32 [height, width] (AdaptiveVariance's plane;
        scaled by norm_const ** 2 inside). Returns a new float32 [height, width, 4], with return_variance also the filtered variance [height, width]."""
        frame = np.ascontiguousarray(frame, np.float32)
        assert frame.ndim == 3 and frame.shape[2] == 4
        variance = np.ascontiguousarray(variance, np.float32)
        assert variance.shape == frame.shape[:2]
        if gbuffer is None:
            gbuffer = self.EvalGBuffer()
        gbuffer = np.ascontiguousarray(gbuffer)
        assert gbuffer.dtype == GBUFFER_DTYPE and gbuffer.shape == frame.shape[:2]
        p = self.denoise_params(norm_const, iterations, normal_squarings, 0.0, sigma_depth, sigma_albedo, demodulate)
        vp = self.denoise_var_params(sigma_lum, var_floor, prefilter)
        out = np.zeros_like(frame)
        out_var = np.zeros_like(variance) if return_variance else None
        self._chk(self.L.hpt_denoise_frame_var(self.h, frame.shape[1], frame.shape[0], frame.ctypes.data, gbuffer.ctypes.data, variance.ctypes.data, C.byref(p), C.byref(vp),
                                               out.ctypes.data, None if out_var is None else out_var.ctypes.data))
        return (out, out_var) if return_variance else out

    def denoise_var_dev(self, color_ptr, gbuffer_ptr, variance_ptr, out_ptr, out_var_ptr=None, width=None, height=None, params=None, var_params=None, stream=None,
                        sigma_lum=None, var_floor=None, prefilter=None, **kw):
        """DenoiseFrameVar on device pointers; asynchronous on `stream`. params / var_params: the two records, or the keyword arguments of
        denoise_params (sigma_color is 0 here) and of denoise_var_params."""
        p = params if params is not None else self.denoise_params(**dict(kw, sigma_color=0.0))
        vp = var_params if var_params is not None else self.denoise_var_params(sigma_lum, var_floor, prefilter)
        self._chk(self.L.hpt_denoise_frame_var_dev(self.h, self.W if width is None else width, self.H if height is None else height,
                                                   color_ptr, gbuffer_ptr, variance_ptr, C.byref(p), C.byref(vp), out_ptr, out_var_ptr, stream))

    def GetExecutionTime(self, name):
        out = (C.c_float * 4)(0, 0, 0, 0)
        self._chk(self.L.hpt_get_execution_time(self.h, name.encode(), out))
        return list(out)

    def last_kernel_ms(self):
        ms = C.c_float(0)
        self._chk(self.L.hpt_last_kernel_ms(self.h, C.byref(ms)))
        return ms.value

    # ---- ISceneObject queries -----------------------------------------------------------------------------------------
    def RayQuery_NearestHitMotion(self, pos_near, dir_far, time):
        pos_near = np.ascontiguousarray(pos_near, np.float32)
        dir_far = np.ascontiguousarray(dir_far, np.float32)
        out = np.zeros(pos_near.shape[0], HIT_DTYPE)
        self._chk(self.L.hpt_ray_query_nearest_motion(self.h, pos_near.ctypes.data, dir_far.ctypes.data, pos_near.shape[0], float(time), out.ctypes.data))
        return out

    def RayQuery_AnyHitMotion(self, pos_near, dir_far, time):
        pos_near = np.ascontiguousarray(pos_near, np.float32)
        dir_far = np.ascontiguousarray(dir_far, np.float32)
        out = np.zeros(pos_near.shape[0], np.uint32)
        self._chk(self.L.hpt_ray_query_any_motion(self.h, pos_near.ctypes.data, dir_far.ctypes.data, pos_near.shape[0], float(time), out.ctypes.data))
        return out

    def RayQuery_NearestHit(self, pos_near, dir_far):
        pos_near = np.ascontiguousarray(pos_near, np.float32)
        dir_far = np.ascontiguousarray(dir_far, np.float32)
        out = np.zeros(pos_near.shape[0], HIT_DTYPE)
        self._chk(self.L.hpt_ray_query_nearest(self.h, pos_near.ctypes.data, dir_far.ctypes.data, pos_near.shape[0], out.ctypes.data))
        return out

    def RayQuery_AnyHit(self, pos_near, dir_far):
        pos_near = np.ascontiguousarray(pos_near, np.float32)
        dir_far = np.ascontiguousarray(dir_far, np.float32)
        out = np.zeros(pos_near.shape[0], np.uint32)
        self._chk(self.L.hpt_ray_query_any(self.h, pos_near.ctypes.data, dir_far.ctypes.data, pos_near.shape[0], out.ctypes.data))
        return out

    # ---- IntegratorDR -----------------------------------------------------------------------------------------------------
    def PutDiffTex2D(self, texId, width, height, channels):
        off, size = _u64(0), _u64(0)
        rc = self.L.hpt_put_diff_tex2d(self.h, texId, width, height, channels, C.byref(off), C.byref(size))
        if rc != 0 and size.value == 0 and off.value == 0xFFFFFFFFFFFFFFFF:
            return (off.value, 0)          # reference behaviour for a bad id: message + (size_t(-1), 0)
        self._chk(rc)
        self.grad_size = off.value + size.value
        return (off.value, size.value)

    def PutDiffLights(self, first, count):
        """Registers lights [first, first + count) as differentiable (no counterpart in the reference): light first + i owns the RGB gain
        a_data[offset + 4 i + 0..2] (float 4 i + 3 is padding), a_dataGrad receives d loss / d gain there. Returns (offset, size = 4 * count)."""
        off, size = _u64(0), _u64(0)
        self._chk(self.L.hpt_put_diff_lights(self.h, first, count, C.byref(off), C.byref(size)))
        self.grad_size = off.value + size.value
        return (off.value, size.value)

    def PathTraceDR(self, tid, channels, out_color, a_passNum, a_refImg, a_data, a_dataGrad, tid_begin=0):
        a_refImg = np.ascontiguousarray(a_refImg, np.float32)
        a_data = np.ascontiguousarray(a_data, np.float32)
        assert a_dataGrad.dtype == np.float32 and a_dataGrad.size == a_data.size
        loss = C.c_float(0)
        self._chk(self.L.hpt_path_trace_dr(self.h, tid_begin, tid, channels, out_color.ctypes.data, a_passNum, a_refImg.ctypes.data,
                                           a_data.ctypes.data, a_dataGrad.ctypes.data, a_data.size, C.byref(loss)))
        return loss.value

    # ---- device-resident arrays for the *_dev entry points (hpt_device_malloc / copy / free) ---------------------------------
    def dev_array(self, host: np.ndarray):
        """Upload a float32 array; returns a DevArray (free()d with the integrator or explicitly)."""
        host = np.ascontiguousarray(host, np.float32)
        p = _vp()
        self._chk(self.L.hpt_device_malloc(self.h, host.nbytes, C.byref(p)))
        a = DevArray(self, p.value, host.shape)
        a.upload(host)
        return a

    def PathTraceDR_dev(self, out: "DevArray", a_passNum, ref: "DevArray", data: "DevArray", grad: "DevArray", loss: "DevArray", tid_begin=0, tid=None, channels=4):
        """PathTraceDR with every array resident in HBM (drmain's loop): memset(grad), memset(loss), launch. The loss word holds the
        sum over pixels of the per-sample losses / a_passNum (divide by W*H for PathTraceDR's return value)."""
        tid = self.N - tid_begin if tid is None else tid
        self._chk(self.L.hpt_device_memset(self.h, grad.ptr, 0, grad.nbytes))
        self._chk(self.L.hpt_device_memset(self.h, loss.ptr, 0, 4))
        self._chk(self.L.hpt_path_trace_dr_dev(self.h, tid_begin, tid, channels, out.ptr, a_passNum, ref.ptr, data.ptr, grad.ptr, data.size, loss.ptr, None))

    def PathTraceVJP(self, tid, channels, out_color, a_passNum, a_adjImg, a_data, a_dataGrad=None, tid_begin=0):
        """The vector-Jacobian product of PathTraceDR's frame (no counterpart in the reference): the same paths, colours and generator steps as
        PathTraceDR, out_color accumulated into, and a_dataGrad overwritten with sum over pixels, samples, c of a_adjImg[y, x, c] *
        d colour_c / d a_data - a_adjImg float32 [winHeight, winWidth, channels] = dL/d(out_color), rows in out_color's order, nothing divided by
        a_passNum. a_adjImg None: the frame only (a_dataGrad may be None and is not touched)."""
        assert out_color.dtype == np.float32 and out_color.flags["C_CONTIGUOUS"]
        a_data = np.ascontiguousarray(a_data, np.float32)
        if a_adjImg is not None:
            a_adjImg = np.ascontiguousarray(a_adjImg, np.float32)
            assert channels not in (3, 4) or a_adjImg.size == self.N * channels     # (other channel counts: the library refuses them)
        assert a_dataGrad is None or (a_dataGrad.dtype == np.float32 and a_dataGrad.flags["C_CONTIGUOUS"] and a_dataGrad.size == a_data.size)
        self._chk(self.L.hpt_path_trace_vjp(self.h, tid_begin, tid, channels, out_color.ctypes.data, a_passNum,
                                            None if a_adjImg is None else a_adjImg.ctypes.data, a_data.ctypes.data,
                                            None if a_dataGrad is None else a_dataGrad.ctypes.data, a_data.size))

    def PathTraceVJP_dev(self, out: "DevArray", a_passNum, adj: "DevArray", data: "DevArray", grad: "DevArray", tid_begin=0, tid=None, channels=4, stream=None):
        """PathTraceVJP with every array resident in HBM; asynchronous on `stream`. `grad` is ACCUMULATED into (zero it yourself); adj None
        (grad may then be None too): the frame only."""
        tid = self.N - tid_begin if tid is None else tid
        self._chk(self.L.hpt_path_trace_vjp_dev(self.h, tid_begin, tid, channels, out.ptr, a_passNum, None if adj is None else adj.ptr, data.ptr,
                                                None if grad is None else grad.ptr, data.size, stream))

    def RayTraceDR(self, tid, channels, out_color, a_passNum, a_refImg, a_data, a_dataGrad):
        """IntegratorDR::RayTraceDR(tid, channels, out_color, a_passNum, a_refImg, a_data, a_dataGrad, a_gradSize): one pinhole ray per pixel,
        base colour x texture, squared difference to a_refImg (float32 [winHeight, winWidth, channels], rows bottom-up, channels 3 or 4).
        out_color float32 [winHeight, winWidth, 4]: hit pixels ASSIGNED (colour, 0), missed pixels and pixels past tid untouched. a_dataGrad
        is overwritten. Returns the reference's value: the per-pixel losses / a_passNum, summed in float in tid order. a_data None: no
        parameter texture is fetched."""
        assert out_color.dtype == np.float32 and out_color.flags["C_CONTIGUOUS"] and out_color.size == self.N * 4
        a_refImg = np.ascontiguousarray(a_refImg, np.float32)
        assert channels not in (3, 4) or a_refImg.size == self.N * channels          # (other channel counts: the library refuses them)
        assert a_dataGrad is None or (a_dataGrad.dtype == np.float32 and a_dataGrad.flags["C_CONTIGUOUS"])
        if a_data is not None:
            a_data = np.ascontiguousarray(a_data, np.float32)
            assert a_dataGrad is None or a_dataGrad.size == a_data.size             # (a_data without a_dataGrad: a_gradSize = 0, refused by the library when a texture is registered)
        loss = C.c_float(0)
        self._chk(self.L.hpt_ray_trace_dr(self.h, tid, channels, out_color.ctypes.data, a_passNum, a_refImg.ctypes.data,
                                          None if a_data is None else a_data.ctypes.data, None if a_dataGrad is None else a_dataGrad.ctypes.data,
                                          0 if a_dataGrad is None else a_dataGrad.size, C.byref(loss)))
        return loss.value

    def RayTraceDR_dev(self, out: "DevArray", a_passNum, ref: "DevArray", data: "DevArray", grad: "DevArray", loss_per_pixel: "DevArray" = None,
                       loss: "DevArray" = None, tid=None, channels=4, stream=None):
        """RayTraceDR with every array resident in HBM; asynchronous. `grad` is ACCUMULATED into (zero it yourself); loss_per_pixel [tid] is
        assigned; `loss` (one float) is ADDED the sum of loss / a_passNum (one float atomic per wave: reproducible to rounding only)."""
        self._chk(self.L.hpt_ray_trace_dr_dev(self.h, self.N if tid is None else tid, channels, out.ptr, a_passNum, ref.ptr, None if data is None else data.ptr,
                                              None if grad is None else grad.ptr, 0 if grad is None else grad.size,
                                              None if loss_per_pixel is None else loss_per_pixel.ptr, None if loss is None else loss.ptr, stream))

    def AdamStep_dev(self, state: "DevArray", grad: "DevArray", momentum: "DevArray", gsq: "DevArray", it: int):
        """AdamOptimizer<float>::step(state, grad, iter) (diff_render/adam.h:43-62) on device arrays."""
        self._chk(self.L.hpt_adam_step_dev(self.h, state.ptr, grad.ptr, momentum.ptr, gsq.ptr, state.size, int(it), None))

    # ---- instrumentation ----------------------------------------------------------------------------------------------------
    def set_instrumentation(self, enabled: bool):
        self._chk(self.L.hpt_set_instrumentation(self.h, int(enabled)))

    def counters(self):
        out = (_u64 * 16)()
        self._chk(self.L.hpt_get_counters(self.h, out))
        return dict(zip(COUNTER_NAMES, [int(v) for v in out]))

    def dr_counters(self):
        out = (_u64 * 16)()
        self._chk(self.L.hpt_get_dr_counters(self.h, out))
        return dict(zip(("records", "records_with_taps", "cyc_record_store", "cyc_sweep", "sweep_wave_trips", "sweep_lanes", "atomic_wave_insts", "sweep_bounces", "records_stored"), [int(v) for v in out]))

    def set_tid_interleave(self, chunk: int, stride: int):
        self._chk(self.L.hpt_set_tid_interleave(self.h, chunk, stride))

    def set_schedule(self, schedule: int, refill_below: int = 0, trace_blocks_per_cu: int = 0, groups: int = 0):
        """0 automatic, 1 persistent megakernel, 2 wavefront (shade kernel + trace kernel with ray replacement), 3 megakernel with block-local ray
        repacking, 4 the wavefront schedule in one launch (block-owned slots; heavy gltf / emissive scenes, elsewhere the automatic choice). hpt_set_schedule."""
        self._chk(self.L.hpt_set_schedule(self.h, schedule, refill_below, trace_blocks_per_cu, groups))

    def Image2D4fRegularizer(self, data, grad):
        """grad += d RegLossImage2D4f / d data (diff_render/integrator_dr.cpp:361-367); float32 [h, w, 4] arrays."""
        assert data.dtype == np.float32 and grad.dtype == np.float32 and data.shape == grad.shape and data.shape[-1] == 4
        self._chk(self.L.hpt_image2d4f_regularizer(self.h, data.shape[1], data.shape[0], data.ctypes.data, grad.ctypes.data))

    def set_option(self, name: str, value: int):
        """hpt_set_option (include/hydra_hip.h lists the names). Among them "adaptive_wavefront": 0 (default) the adaptive calls - PathTraceBlockCounts
        and every round of PathTraceBlockAdaptive - run the megakernel; 1 each goes to the wavefront schedule where a PathTraceBlock of as many pixels
        as it has counts above 0 would (set_schedule). Frames, generators and moments are the same bit for bit; a count above 0xFFFFFF is refused there.
        "adaptive_spectral": 0 (default) the adaptive calls refuse a spectral context; 1 they are served there (thin films, dispersion and moving instances
        included; 1, 3 or 4 channels, no wavelength layers): a pixel given k passes is a uniform spectral PathTraceBlock pixel of k passes bit for bit, and
        the records take the luminance of what each sample adds to the frame, so AdaptivePlan, AdaptiveResolve, AdaptiveVariance and denoise_var work on
        them unchanged. Together with "adaptive_wavefront" such calls take the wavefront schedule under the same rule.
        "qmc_wavefront": 0 (default) PathTraceBlockQMC / render_qmc (and PathTraceBlockKMLT's FB_DIRECT forward) run the megakernel; 1 the call goes to
        the wavefront schedule where a PathTraceBlock of as many pixels as it has generator slots with work would (set_schedule). Sample records and
        generators are the same bit for bit; spectral, sweep-layout, thin-film, depth-0 and instrumented calls keep the megakernel; a call whose slot 0
        would run more than 0xFFFFFF samples is refused there."""
        self._chk(self.L.hpt_set_option(self.h, name.encode(), value))
        if name == "qmc_spectral":
            self._qmc_spectral = bool(value)     # PathTraceBlockQMC then takes frames of more than 4 channels
        # ("kmlt_spectral" needs no state here: path_trace_pss / render_kmlt pass through, and the library refuses what the option does not allow)

    def accel_info(self):
        out = (C.c_float * 4)()
        self._chk(self.L.hpt_get_accel_info(self.h, out))
        return {"sah_node_visits": out[0], "inst_tris": int(out[1]), "instances": int(out[2]), "flat": int(out[3]) == 1,
                "layout": ("two-level", "flat", "sweep")[int(out[3])]}

    def commit_time(self):
        """The last CommitScene: host ms, upload ms, device refit ms, refitted (bool)."""
        out = (C.c_float * 4)()
        self._chk(self.L.hpt_get_commit_time(self.h, out))
        return {"host_ms": out[0], "upload_ms": out[1], "refit_ms": out[2], "device_ms": out[2], "refitted": int(out[3]) == 1, "device_built": int(out[3]) == 2}

    def refit_info(self):
        """hpt_get_refit_info: the surface-area estimate at build time and after the last refit (equal when the last commit was a build), the levels
        a refit launches (0: the tree cannot be refitted) and whether "refit_max_sah_pct" rejected the last commit's refit."""
        out = (C.c_float * 4)()
        self._chk(self.L.hpt_get_refit_info(self.h, out))
        return {"build": out[0], "after": out[1], "levels": int(out[2]), "rejected": int(out[3]) == 1}

    def build_info(self):
        """hpt_get_build_info: the treelet passes ("device_build_quality") of the last CommitScene when it built on the device: passes run, treelets
        examined and rewritten over all passes, device ms spent in them. All zero after a host build or a refit."""
        out = (C.c_float * 4)()
        self._chk(self.L.hpt_get_build_info(self.h, out))
        return {"passes": int(out[0]), "examined": int(out[1]), "rewritten": int(out[2]), "ms": out[3]}

    def read_accel(self):
        """hpt_read_accel: the committed single-level tree as it lies in device memory: (nodes [BVH_NODE_DTYPE], tris [BVH_TRI_DTYPE], rootRef).
        A device-built tree's node array has unused entries: only what rootRef reaches is a node."""
        out = []
        root = C.c_uint32(0)
        for what, dt in ((0, BVH_NODE_DTYPE), (1, BVH_TRI_DTYPE)):
            nbytes = C.c_uint64(0)
            self._chk(self.L.hpt_read_accel(self.h, what, None, 0, C.byref(nbytes), C.byref(root)))
            a = np.zeros(nbytes.value // dt.itemsize, dt)
            if a.size:
                self._chk(self.L.hpt_read_accel(self.h, what, a.ctypes.data, a.nbytes, C.byref(nbytes), C.byref(root)))
            out.append(a)
        return out[0], out[1], int(root.value)

    def two_level_info(self):
        """hpt_get_two_level_info: what the last CommitScene did when it built the two-level layout on the device
        (set_option("device_build_two_level", 1)); every field is zero / False after any other kind of commit."""
        out = (C.c_float * 8)()
        self._chk(self.L.hpt_get_two_level_info(self.h, out))
        return {"device_built": int(out[0]) == 1, "blas_built": int(out[1]), "blas_kept": int(out[2]), "tlas_only": int(out[3]) == 1,
                "tlas_depth": int(out[4]), "blas_depth": int(out[5]), "blas_ms": out[6], "tlas_ms": out[7]}

    def read_accel_two_level(self):
        """hpt_read_accel_two_level: the committed two-level tree (either builder's) as it lies in device memory:
        (nodes [BVH_NODE_DTYPE], tris [BVH_TRI_DTYPE], insts [BVH_INST_DTYPE], TLAS rootRef)."""
        out = []
        root = C.c_uint32(0)
        for what, dt in ((0, BVH_NODE_DTYPE), (1, BVH_TRI_DTYPE), (2, BVH_INST_DTYPE)):
            nbytes = C.c_uint64(0)
            self._chk(self.L.hpt_read_accel_two_level(self.h, what, None, 0, C.byref(nbytes), C.byref(root)))
            a = np.zeros(nbytes.value // dt.itemsize, dt)
            if a.size:
                self._chk(self.L.hpt_read_accel_two_level(self.h, what, a.ctypes.data, a.nbytes, C.byref(nbytes), C.byref(root)))
            out.append(a)
        return out[0], out[1], out[2], int(root.value)

    def UpdateGeom_Triangles3f(self, geom_id, vpos, indices):
        """ISceneObject::UpdateGeom_Triangles3f (CrossRT.h:85-86): new positions (float32 [n, 3] or [n, 4]) and indices for a mesh; takes effect at the
        next CommitScene. Unchanged indices keep a committed single-level tree refittable."""
        vpos = np.ascontiguousarray(vpos, np.float32)
        assert vpos.ndim == 2 and vpos.shape[1] in (3, 4)
        indices = np.ascontiguousarray(indices, np.uint32).reshape(-1)
        self._chk(self.L.hpt_update_geom_triangles3f(self.h, geom_id, vpos.ctypes.data, vpos.shape[0], indices.ctypes.data, indices.size, 0, 4 * vpos.shape[1]))

    def UpdateInstance(self, inst_id, matrix_rowmajor):
        """ISceneObject::UpdateInstance (CrossRT.h:134); takes effect at the next CommitScene."""
        from .scene import colmajor
        cm = colmajor(np.asarray(matrix_rowmajor))
        self._chk(self.L.hpt_update_instance(self.h, inst_id, cm.ctypes.data))

    def CommitScene(self, options=4):
        """ISceneObject::CommitScene (CrossRT.h:109); options as BuildOptions (:8-14): 1 BUILD_LOW, 2 BUILD_MEDIUM (the single-level tree is built on the
        device), 4 BUILD_HIGH (the host's SAH build)."""
        self._chk(self.L.hpt_commit_scene(self.h, options))

    def last_launch(self):
        """What the last PathTrace* call walked: schedule, 4-wide compressed tree, 64-byte shading records, HBM part of the stacks, passes per
        work item of the megakernel (0: whole pixels)."""
        out = (C.c_uint32 * 5)()
        self._chk(self.L.hpt_get_last_launch(self.h, out))
        return {"schedule": int(out[0]), "wide_nodes": bool(out[1]), "shade_records": bool(out[2]), "deep_stack": bool(out[3]), "pass_slice": int(out[4])}

    def stack_witness(self):
        """With set_option("dbg_stack_witness", 1): (words of the stacks' HBM part the last launch wrote, words filled before it). hpt_get_stack_witness."""
        out = (C.c_uint64 * 2)()
        self._chk(self.L.hpt_get_stack_witness(self.h, out))
        return int(out[0]), int(out[1])

    def last_schedule(self):
        s, it = C.c_int(0), C.c_uint32(0)
        self._chk(self.L.hpt_get_schedule(self.h, C.byref(s), C.byref(it)))
        return s.value, it.value

    def set_launch_config(self, blocks_per_cu: int):
        self._chk(self.L.hpt_set_launch_config(self.h, blocks_per_cu))

    def device_info(self):
        cu, wf = C.c_int(0), C.c_int(0)
        name = C.create_string_buffer(128)
        self._chk(self.L.hpt_device_info(self.h, C.byref(cu), C.byref(wf), name, 128))
        return {"cus": cu.value, "wavefront": wf.value, "arch": name.value.decode()}


CAM_PINHOLE, CAM_TABLE_LENS = 0, 1


class CamRays:
    """ICamRaysAPI2-shaped front end (cam_plugin/CamPluginAPI.h:39-77) of the device cameras: CamPinHole (kind 0) and CamTableLens (kind 1)
    of the reference, with the reference's method names, plus render_dev (the loop of cam_plugin/main_with_cam_gpu.cpp). A camera belongs to
    the integrator it was made from and keeps it alive."""

    def __init__(self, integ: HipIntegrator, kind: int = CAM_PINHOLE):
        self.integ, self.L, self.kind = integ, integ.L, int(kind)
        self.width = self.height = self.batch = 0
        self.spectral = 0
        h = _vp()
        integ._chk(self.L.hpt_cam_create(integ.h, self.kind, C.byref(h)))
        self.h = h

    def __del__(self):
        try:
            if getattr(self, "h", None) and getattr(self.integ, "h", None):
                self.L.hpt_cam_destroy(self.h)
            self.h = None
        except Exception:
            pass

    def _chk(self, rc):
        self.integ._chk(rc)

    def SetParameters(self, a_width, a_height, projInv, spectralMode=0):
        """SetParameters(a_width, a_height, a_params): projInv = inverse4x4(perspectiveMatrix(fov, aspect, near, far)), 16 floats column-major
        (Params.projInv of the scene's camera is one); spectralMode = CamParameters::spectralMode."""
        m = np.ascontiguousarray(list(projInv) if not isinstance(projInv, np.ndarray) else projInv, np.float32).reshape(16)
        self._chk(self.L.hpt_cam_set_parameters(self.h, a_width, a_height, m.ctypes.data, int(spectralMode)))
        self.width, self.height, self.spectral = int(a_width), int(a_height), int(bool(spectralMode))

    def SetLens(self, lines, phys_size):
        """The lens table and m_physSize of CamTableLens::Init: lines float32 [n, 4] = {curvatureRadius, thickness, eta, apertureRadius}, film side first."""
        lines = np.ascontiguousarray(lines, np.float32).reshape(-1, 4)
        self._chk(self.L.hpt_cam_set_lens(self.h, lines.ctypes.data if lines.size else None, lines.shape[0], float(phys_size[0]), float(phys_size[1])))

    def SetBatchSize(self, a_tileSize):
        self._chk(self.L.hpt_cam_set_batch_size(self.h, a_tileSize))
        self.batch = int(a_tileSize)

    def MakeRaysBlock(self, out_rayPosAndNear4f, out_rayDirAndFar4f, in_blockSize, subPassId):
        """float32 [in_blockSize, 4] arrays (RayPosAndW / RayDirAndT), camera space."""
        for a in (out_rayPosAndNear4f, out_rayDirAndFar4f):
            assert a.dtype == np.float32 and a.flags["C_CONTIGUOUS"] and a.size >= 4 * in_blockSize
        self._chk(self.L.hpt_cam_make_rays_block(self.h, out_rayPosAndNear4f.ctypes.data, out_rayDirAndFar4f.ctypes.data, in_blockSize, subPassId))

    def AddSamplesContributionBlock(self, out_color4f, colors4f, in_blockSize, a_width, a_height, subPassId):
        """out_color4f float32 [a_height, a_width, 4] (rgb added to); colors4f float32 [in_blockSize, 4], or [in_blockSize] in spectral mode."""
        assert out_color4f.dtype == np.float32 and out_color4f.flags["C_CONTIGUOUS"] and out_color4f.size == a_width * a_height * 4
        assert colors4f.dtype == np.float32 and colors4f.flags["C_CONTIGUOUS"] and colors4f.size >= in_blockSize * (1 if self.spectral else 4)
        self._chk(self.L.hpt_cam_add_samples_contribution_block(self.h, out_color4f.ctypes.data, colors4f.ctypes.data, in_blockSize, a_width, a_height, subPassId))

    def make_rays_block_dev(self, pos_ptr, dir_ptr, n, sub_pass_id, stream=None):
        self._chk(self.L.hpt_cam_make_rays_block_dev(self.h, pos_ptr, dir_ptr, n, sub_pass_id, stream))

    def add_samples_contribution_block_dev(self, frame_ptr, colors_ptr, n, sub_pass_id, stream=None):
        self._chk(self.L.hpt_cam_add_samples_contribution_block_dev(self.h, frame_ptr, colors_ptr, n, self.width, self.height, sub_pass_id, stream))

    def read_state(self, n=None):
        """Host copies of the first n slots of (m_randomGens uint32 [n, 2], m_storedWaves [n], m_storedCos4 [n])."""
        n = self.batch if n is None else int(n)
        gens, waves, cos4 = np.zeros((n, 2), np.uint32), np.zeros(n, np.float32), np.zeros(n, np.float32)
        self._chk(self.L.hpt_cam_read_state(self.h, gens.ctypes.data, waves.ctypes.data, cos4.ctypes.data, n))
        return gens, waves, cos4

    def render_dev(self, frame_ptr, passes, stream=None):
        """The device-resident loop: `passes` times over the tiles of the frame, into the width * height * 4 floats at frame_ptr (added to)."""
        self._chk(self.L.hpt_cam_render_dev(self.integ.h, self.h, frame_ptr, passes, stream))

    def render(self, passes):
        """render_dev into a zeroed frame; returns float32 [height, width, 4]."""
        frame = self.integ.dev_array(np.zeros((self.height, self.width, 4), np.float32))
        try:
            self.render_dev(frame.ptr, passes)
            return frame.download()
        finally:
            frame.free()

    def GetExecutionTime(self, name):
        out = (C.c_float * 4)(0, 0, 0, 0)
        self._chk(self.L.hpt_cam_get_execution_time(self.h, name.encode(), out))
        return list(out)
