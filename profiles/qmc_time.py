"""Kernel time of PathTraceBlockQMC against PathTraceBlock (device-pointer forms, HIP events: hpt_last_kernel_ms) on one scene.
usage (GPU box): python profiles/qmc_time.py cornell|test_228 [--size N] [--spp N] [--repeats N]
One JSON line per mode: "PathTraceBlock" (the scene's automatic kernel), "PathTraceBlock full" (force_full_materials: every BSDF branch, the
shading set the QMC kernel is built with), "PathTraceBlockQMC" (atomic frame), "PathTraceBlockQMC records only" (no frame: the run that
prices the film atomics), "PathTraceBlockQMC frame + records". Run each scene as a step of its own under `timeout`, chained with &&."""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
from hydracore3_amd.api import HipIntegrator, qmc_sample_count  # noqa: E402
from hydracore3_amd.scene import load_hydra_xml  # noqa: E402


def opt(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


which = sys.argv[1] if len(sys.argv) > 1 and not sys.argv[1].startswith("--") else "cornell"
size, spp, repeats = opt("--size", 1024), opt("--spp", 64), opt("--repeats", 5)
sc = load_hydra_xml(os.path.join(ROOT, "tests", "golden", "scenes", "test_035" if which == "cornell" else which, "statex_00001.xml"), size, size)
gpu = HipIntegrator(sc)
n, S = gpu.N, qmc_sample_count(gpu.N, spp)


def dev(nbytes):
    p = C.c_void_p()
    gpu._chk(gpu.L.hpt_device_malloc(gpu.h, nbytes, C.byref(p)))
    return p


d_out, d_col, d_pix = dev(n * 16), dev(S * 16), dev(S * 4)
zero = np.zeros((gpu.H, gpu.W, 4), np.float32)
modes = [("PathTraceBlock", lambda: gpu.path_trace_block_dev(d_out, spp)),
         ("PathTraceBlock full", lambda: gpu.path_trace_block_dev(d_out, spp)),
         ("PathTraceBlockQMC", lambda: gpu.path_trace_qmc_block_dev(d_out, spp)),
         ("PathTraceBlockQMC records only", lambda: gpu.path_trace_qmc_block_dev(None, spp, sample_color_ptr=d_col, sample_pixel_ptr=d_pix)),
         ("PathTraceBlockQMC frame + records", lambda: gpu.path_trace_qmc_block_dev(d_out, spp, sample_color_ptr=d_col, sample_pixel_ptr=d_pix))]
for mode, call in modes:
    gpu.set_option("force_full_materials", 1 if mode == "PathTraceBlock full" else 0)
    gpu._chk(gpu.L.hpt_device_copy(gpu.h, d_out, zero.ctypes.data, zero.nbytes, 1))
    ms = []
    for i in range(1 + repeats):                                        # one warm-up call
        call()
        t = gpu.last_kernel_ms()                                        # synchronises on the stop event
        if i >= 1:
            ms.append(t)
    out = np.zeros_like(zero)
    gpu._chk(gpu.L.hpt_device_copy(gpu.h, out.ctypes.data, d_out, out.nbytes, 2))
    ms.sort()
    med = ms[len(ms) // 2]
    print(json.dumps({"scene": f"{which} {size}x{size}", "mode": mode, "spp": spp, "samples": S, "layout": gpu.accel_info()["layout"], "repeats": repeats,
                      "kernel_ms_min": round(ms[0], 3), "kernel_ms_median": round(med, 3), "kernel_ms_max": round(ms[-1], 3),
                      "mpaths_per_s": round(S / med / 1e3, 1), "finite": bool(np.isfinite(out).all()),
                      "mean_rgb_per_sample": round(float(out[..., :3].mean()) / (spp * (1 + repeats)), 6)}), flush=True)
for p in (d_out, d_col, d_pix):
    gpu._chk(gpu.L.hpt_device_free(gpu.h, p))
