"""Kernel time of EvalGBuffer (hpt_eval_gbuffer_dev, HIP events: hpt_last_kernel_ms) on the Cornell box at 1024^2 and on the 1 M-triangle
interior at 1920x1080, and - for the yardstick of profiles/gbuffer.md - the batched ray query on the identical 16 rays per pixel.
usage (GPU box): python profiles/gbuffer_time.py [cornell|interior|both] [--rayquery] [--repeats N]
  default      : warm-up + N timed EvalGBuffer calls per scene, one JSON line per scene (min / median / max ms, layout)
  --rayquery   : instead, the same rays (tests/gbuffer_reference.eye_rays) through hpt_ray_query_nearest, three times; that entry point includes
                 the copies, so run it under `rocprofv3 --kernel-trace --stats -- python profiles/gbuffer_time.py <scene> --rayquery` and read
                 rayQueryKernel's time from the kernel statistics"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import ctypes as C  # noqa: E402
from hydracore3_amd.api import GBUFFER_DTYPE, HipIntegrator  # noqa: E402
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
        import gbuffer_reference as R
        pos, dr = R.eye_rays(gpu.params, gpu.packed_xy())
        pos, dr = pos.reshape(-1, 4), dr.reshape(-1, 4)
        for _ in range(3):
            h = gpu.RayQuery_NearestHit(pos, dr)
        print(json.dumps({"scene": name, "mode": "rayquery", "rays": int(pos.shape[0]), "hits": int((h["instId"] != 0xFFFFFFFF).sum()), "layout": gpu.accel_info()["layout"]}), flush=True)
        continue
    d_out, ms = C.c_void_p(), []
    gpu._chk(gpu.L.hpt_device_malloc(gpu.h, n * GBUFFER_DTYPE.itemsize, C.byref(d_out)))
    for i in range(3 + repeats):                                        # three warm-up calls
        gpu._chk(gpu.L.hpt_eval_gbuffer_dev(gpu.h, n, d_out, None, None))
        t = gpu.last_kernel_ms()                                        # synchronises on the stop event
        if i >= 3:
            ms.append(t)
    out = np.zeros((gpu.H, gpu.W), GBUFFER_DTYPE)
    gpu._chk(gpu.L.hpt_device_copy(gpu.h, out.ctypes.data, d_out, out.nbytes, 2))
    gpu._chk(gpu.L.hpt_device_free(gpu.h, d_out))
    ms.sort()
    print(json.dumps({"scene": name, "mode": "gbuffer", "pixels": n, "rays": 16 * n, "layout": gpu.accel_info()["layout"], "repeats": repeats,
                      "kernel_ms_min": round(ms[0], 4), "kernel_ms_median": round(ms[len(ms) // 2], 4), "kernel_ms_max": round(ms[-1], 4),
                      "grays_per_s": round(16 * n / ms[len(ms) // 2] / 1e6, 3), "hit_pixels": int((out["instId"] >= 0).sum()),
                      "mean_coverage": round(float(out["coverage"].mean()), 5)}), flush=True)
