"""Kernel time of RayTraceDR next to CastSingleRayBlock (device-pointer forms, HIP events: hpt_last_kernel_ms) on the Cornell box at 1024^2 and on
the 1 M-triangle interior at 1920x1080: the table of profiles/raytrace_dr.md.
usage (GPU box): python profiles/raytrace_dr_time.py [cornell|interior|both] [--repeats N]
Per scene and parameter-texture size (256^2 and 4096^2, four channels, registered on the first textures the scene's materials bind): three warm-up
+ N timed calls of each variant, one JSON line with [median, min, max] ms of
  cast            castSingleRayKernel
  forward         RayTraceDR, dr_grad_mode 0, per-pixel losses and lossAccum
  forward_no_acc  the same with lossAccumDev = NULL        (what the one-address atomic per wave costs)
  forward_bare    the same with lossPerPixelDev = NULL too
  grad            RayTraceDR with the gradient, per-pixel losses and lossAccum
  grad_no_acc     the same with lossAccumDev = NULL        (forward_no_acc -> grad_no_acc: the scatter alone)"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
from hydracore3_amd.api import HipIntegrator  # noqa: E402
from hydracore3_amd.scene import load_hydra_xml  # noqa: E402
from hydracore3_amd.synth import interior_scene  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
which = args[0] if args else "both"
repeats = int(sys.argv[sys.argv.index("--repeats") + 1]) if "--repeats" in sys.argv else 21


def scenes():
    if which in ("cornell", "both"):
        yield "cornell 1024x1024", load_hydra_xml(os.path.join(ROOT, "tests", "golden", "scenes", "test_035", "statex_00001.xml"), 1024, 1024)
    if which in ("interior", "both"):
        yield "interior-1M 1920x1080", interior_scene(1920, 1080)


def timed(gpu, call):
    ms = []
    for i in range(3 + repeats):                                        # three warm-up calls
        call()
        t = gpu.last_kernel_ms()                                        # synchronises on the stop event
        if i >= 3:
            ms.append(t)
    return [round(float(np.median(ms)), 4), round(float(np.min(ms)), 4), round(float(np.max(ms)), 4)]


for name, sc in scenes():
    tex_ids = sorted({int(m["texid"][0]) for m in np.array(sc.materials)})[:4]
    for size in (256, 4096):
        gpu = HipIntegrator(sc)
        frame = gpu.dev_array(np.zeros((sc.height, sc.width, 4), np.float32))
        rec = {"scene": name, "pixels": gpu.N, "layout": gpu.accel_info()["layout"], "tex": size, "textures": len(tex_ids), "repeats": repeats}
        rec["cast"] = timed(gpu, lambda: gpu.cast_single_ray_block_dev(frame.ptr))
        total = 0
        for t in tex_ids:
            off, sz = gpu.PutDiffTex2D(t, size, size, 4)
            total = off + sz
        ref = gpu.dev_array(np.full((sc.height, sc.width, 4), 0.25, np.float32))
        data, grad = gpu.dev_array(np.full(total, 0.5, np.float32)), gpu.dev_array(np.zeros(total, np.float32))
        px, acc = gpu.dev_array(np.zeros(gpu.N, np.float32)), gpu.dev_array(np.zeros(1, np.float32))
        rec["grad"] = timed(gpu, lambda: gpu.RayTraceDR_dev(frame, 1, ref, data, grad, px, acc))
        rec["grad_elements_touched"] = int(np.count_nonzero(grad.download()))
        rec["grad_no_acc"] = timed(gpu, lambda: gpu.RayTraceDR_dev(frame, 1, ref, data, grad, px, None))
        gpu.set_option("dr_grad_mode", 0)
        rec["forward"] = timed(gpu, lambda: gpu.RayTraceDR_dev(frame, 1, ref, data, grad, px, acc))
        rec["forward_no_acc"] = timed(gpu, lambda: gpu.RayTraceDR_dev(frame, 1, ref, data, grad, px, None))
        rec["forward_bare"] = timed(gpu, lambda: gpu.RayTraceDR_dev(frame, 1, ref, data, grad, None, None))
        print(json.dumps(rec), flush=True)
        for a in (frame, ref, data, grad, px, acc):
            a.free()
        del gpu
