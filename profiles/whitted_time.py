"""Kernel time of CastSingleRayBlock and RayTraceBlock (device-pointer forms, HIP events: hpt_last_kernel_ms) on the Cornell box at 1024^2 and on
the 1 M-triangle interior at 1920x1080, and - for the yardstick of profiles/whitted.md - the batched ray query on the identical primary rays.
usage (GPU box): python profiles/whitted_time.py [cornell|interior|both] [--rayquery] [--repeats N]
  default      : three warm-up + N timed calls of each pass per scene, one JSON line per scene and pass (min / median / max ms, layout)
  --rayquery   : instead, the same rays (tests/raytrace_reference.eye_rays) through hpt_ray_query_nearest, three times; that entry point includes
                 the copies, so run it under `rocprofv3 --kernel-trace --stats -- python profiles/whitted_time.py <scene> --rayquery` and read
                 rayQueryKernel's time from the kernel statistics"""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
from hydracore3_amd.api import HipIntegrator  # noqa: E402
from hydracore3_amd.scene import load_hydra_xml  # noqa: E402
from hydracore3_amd.synth import interior_scene  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
which = args[0] if args else "both"
rayquery = "--rayquery" in sys.argv
repeats = int(sys.argv[sys.argv.index("--repeats") + 1]) if "--repeats" in sys.argv else 10


def scenes():
    if which in ("cornell", "both"):
        yield "cornell 1024x1024", load_hydra_xml(os.path.join(ROOT, "tests", "golden", "scenes", "test_035", "statex_00001.xml"), 1024, 1024)
    if which in ("interior", "both"):
        yield "interior-1M 1920x1080", interior_scene(1920, 1080)


for name, sc in scenes():
    gpu = HipIntegrator(sc)
    n = gpu.N
    if rayquery:
        import raytrace_reference as RT
        pos, dr = RT.eye_rays(gpu.params, gpu.packed_xy())
        for _ in range(3):
            h = gpu.RayQuery_NearestHit(pos, dr)
        print(json.dumps({"scene": name, "mode": "rayquery", "rays": int(pos.shape[0]), "hits": int((h["instId"] != 0xFFFFFFFF).sum()), "layout": gpu.accel_info()["layout"]}), flush=True)
        continue
    d_out = C.c_void_p()
    gpu._chk(gpu.L.hpt_device_malloc(gpu.h, n * 16, C.byref(d_out)))
    zero = np.zeros((gpu.H, gpu.W, 4), np.float32)
    for mode in ("CastSingleRayBlock", "RayTraceBlock"):
        gpu._chk(gpu.L.hpt_device_copy(gpu.h, d_out, zero.ctypes.data, zero.nbytes, 1))
        ms = []
        for i in range(3 + repeats):                                    # three warm-up calls
            if mode == "CastSingleRayBlock":
                gpu.cast_single_ray_block_dev(d_out)
            else:
                gpu.ray_trace_block_dev(d_out, channels=4)
            t = gpu.last_kernel_ms()                                    # synchronises on the stop event
            if i >= 3:
                ms.append(t)
        out = np.zeros_like(zero)
        gpu._chk(gpu.L.hpt_device_copy(gpu.h, out.ctypes.data, d_out, out.nbytes, 2))
        ms.sort()
        print(json.dumps({"scene": name, "mode": mode, "pixels": n, "layout": gpu.accel_info()["layout"], "trace_depth": int(sc.trace_depth), "lights": len(sc.lights),
                          "repeats": repeats, "kernel_ms_min": round(ms[0], 4), "kernel_ms_median": round(ms[len(ms) // 2], 4), "kernel_ms_max": round(ms[-1], 4),
                          "mpixels_per_s": round(n / ms[len(ms) // 2] / 1e3, 1), "finite": bool(np.isfinite(out).all()),
                          "mean_rgb": round(float(out[..., :3].mean()) / (1 if mode == "CastSingleRayBlock" else 3 + repeats), 6)}), flush=True)
    gpu._chk(gpu.L.hpt_device_free(gpu.h, d_out))
