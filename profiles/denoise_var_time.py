"""Kernel time of DenoiseFrameVar (hpt_denoise_frame_var_dev, HIP events: hpt_last_kernel_ms) beside DenoiseFrame on the same frame, at
1024 x 1024 and 1920 x 1080, default parameters. usage (GPU box): python profiles/denoise_var_time.py [--repeats N]
One JSON line per size:
  var_call_ms    the pack kernel and five passes of DenoiseFrameVar (min / median / max over N calls after three warm-up calls)
  var_ms_k       the same call with iterations = k, k = 1 .. 5 (median); var_pass_ms: the differences, the pass at step 2^(k-1)
  fixed_ms_k     hpt_denoise_frame_dev on the same frame and records, k = 1 .. 5; fixed_pass_ms likewise
  ratio          var_ms_5 / fixed_ms_5, and per pass
The frame is that of profiles/denoise_time.py; the variance plane is (luminance / 4)^2 of the 4-spp sum, the estimate a single sample gives."""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
from hydracore3_amd.api import GBUFFER_DTYPE, HipIntegrator  # noqa: E402

repeats = int(sys.argv[sys.argv.index("--repeats") + 1]) if "--repeats" in sys.argv else 20


def frame(w, h):
    rng = np.random.default_rng(w)
    yy, xx = np.mgrid[0:h, 0:w]
    g = np.zeros((h, w), GBUFFER_DTYPE)
    n = np.stack([0.2 * np.sin(xx / 40.0), 0.2 * np.cos(yy / 30.0), np.ones((h, w))], -1)
    g["norm"] = (n / np.linalg.norm(n, axis=-1, keepdims=True)).astype(np.float32)
    g["depth"] = (2.0 + xx / w + yy / h).astype(np.float32)
    g["rgba"][..., :3] = (0.2 + 0.6 * rng.random((h, w, 3))).astype(np.float32)
    g["rgba"][..., 3], g["coverage"] = 1.0, 1.0
    g["instId"] = (xx * 2 // w + 2 * (yy * 2 // h)).astype(np.int32)
    g["matId"] = g["objId"] = g["instId"]
    color = (g["rgba"] * rng.gamma(1.0, 4.0, (h, w, 1))).astype(np.float32)   # a 4-spp sum: mean 4, as noisy as it
    lum = 0.2126 * color[..., 0] + 0.7152 * color[..., 1] + 0.0722 * color[..., 2]
    return color, g, ((lum / 4) ** 2).astype(np.float32)


def median(v):
    return sorted(v)[len(v) // 2]


gpu = HipIntegrator()
for w, h in ((1024, 1024), (1920, 1080)):
    color, gb, var = frame(w, h)
    n = w * h
    ptr = [C.c_void_p() for _ in range(5)]
    for p, nbytes in zip(ptr, (n * 16, n * 60, n * 4, n * 16, n * 4)):
        gpu._chk(gpu.L.hpt_device_malloc(gpu.h, nbytes, C.byref(p)))
    d_color, d_gb, d_var, d_out, d_out_var = ptr
    for dev, host in ((d_color, color), (d_gb, gb), (d_var, var)):
        gpu._chk(gpu.L.hpt_device_copy(gpu.h, dev, host.ctypes.data, host.nbytes, 1))

    def timed(call):
        ms = []
        for i in range(3 + repeats):
            call()
            t = gpu.last_kernel_ms()                                      # synchronises on the stop event
            if i >= 3:
                ms.append(t)
        return ms

    fixed = {k: timed(lambda: gpu.denoise_dev(d_color, d_gb, d_out, w, h, norm_const=0.25, iterations=k)) for k in range(1, 6)}
    # the variance of a mean of four: norm_const scales the plane by 1/16 inside
    guided = {k: timed(lambda: gpu.denoise_var_dev(d_color, d_gb, d_var, d_out, d_out_var, w, h, norm_const=0.25, iterations=k)) for k in range(1, 6)}
    out = np.zeros((h, w, 4), np.float32)
    gpu._chk(gpu.L.hpt_device_copy(gpu.h, out.ctypes.data, d_out, out.nbytes, 2))
    for p in ptr:
        gpu._chk(gpu.L.hpt_device_free(gpu.h, p))
    fm, vm = {k: median(v) for k, v in fixed.items()}, {k: median(v) for k, v in guided.items()}
    fp = {1: fm[1], **{k: fm[k] - fm[k - 1] for k in range(2, 6)}}
    vp = {1: vm[1], **{k: vm[k] - vm[k - 1] for k in range(2, 6)}}
    print(json.dumps({"size": f"{w}x{h}", "pixels": n, "repeats": repeats, "device": gpu.device_info()["arch"],
                      "var_call_ms_min": round(min(guided[5]), 4), "var_call_ms_median": round(vm[5], 4), "var_call_ms_max": round(max(guided[5]), 4),
                      "fixed_call_ms_median": round(fm[5], 4), "ratio": round(vm[5] / fm[5], 4),
                      "var_ms_k": {k: round(v, 4) for k, v in vm.items()}, "fixed_ms_k": {k: round(v, 4) for k, v in fm.items()},
                      "var_pass_ms": {f"step {1 << (k - 1)}": round(v, 4) for k, v in vp.items()},
                      "fixed_pass_ms": {f"step {1 << (k - 1)}": round(v, 4) for k, v in fp.items()},
                      "pass_ratio": {f"step {1 << (k - 1)}": round(vp[k] / fp[k], 3) for k in vp},
                      "finite": bool(np.isfinite(out).all()), "mean": round(float(out[..., :3].mean()), 5)}), flush=True)
