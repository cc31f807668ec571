"""Kernel time of DenoiseFrame (hpt_denoise_frame_dev, HIP events: hpt_last_kernel_ms) at 1024 x 1024 and 1920 x 1080, default parameters.
usage (GPU box): python profiles/denoise_time.py [--repeats N] [--dump DIR]
  --dump DIR     also writes each size's filtered frame to DIR/denoise_<size>.npy (to compare two builds of the kernels bit for bit; an A/B build is
                 chosen with HYDRA_HIP_LIB, e.g. the direct-load variant: python __graft_entry__.py unit dndirect denoise,host -DHPT_DENOISE_LDS=0)
One JSON line per size:
  call_ms        the pack kernel and five passes (min / median / max over N calls after three warm-up calls)
  ms_k           the same call with iterations = k, k = 1 .. 5 (median); ms_1 = pack + the pass at step 1
  pass_ms        ms_k - ms_(k-1): the pass at step 2^(k-1), k = 2 .. 5
  copy_ms        for scale: a device-to-device copy of 32 bytes per pixel, i.e. the 64 bytes per pixel a pass must move at least (three 16-byte
                 planes read once, one written), timed with device events around 20 copies
  gpixels_per_s  pixels over the median call time
The frame is synthetic (a depth ramp, four surfaces, smooth normals, noise on the colours): the filter's time does not depend on the values
except through the taps the id test skips."""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
from hydracore3_amd.api import GBUFFER_DTYPE, HipIntegrator  # noqa: E402

repeats = int(sys.argv[sys.argv.index("--repeats") + 1]) if "--repeats" in sys.argv else 20
dump = sys.argv[sys.argv.index("--dump") + 1] if "--dump" in sys.argv else None


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
    return color, g


def median(v):
    return sorted(v)[len(v) // 2]


gpu = HipIntegrator()
hip = C.CDLL("libamdhip64.so")
for w, h in ((1024, 1024), (1920, 1080)):
    color, gb = frame(w, h)
    n = w * h
    ptr = [C.c_void_p() for _ in range(4)]
    for p, nbytes in zip(ptr, (n * 16, n * 60, n * 16, n * 32)):
        gpu._chk(gpu.L.hpt_device_malloc(gpu.h, nbytes, C.byref(p)))
    d_color, d_gb, d_out, d_copy = ptr
    gpu._chk(gpu.L.hpt_device_copy(gpu.h, d_color, color.ctypes.data, color.nbytes, 1))
    gpu._chk(gpu.L.hpt_device_copy(gpu.h, d_gb, gb.ctypes.data, gb.nbytes, 1))

    def timed(iterations):
        ms = []
        for i in range(3 + repeats):
            gpu.denoise_dev(d_color, d_gb, d_out, w, h, norm_const=0.25, iterations=iterations)
            t = gpu.last_kernel_ms()                                      # synchronises on the stop event
            if i >= 3:
                ms.append(t)
        return ms

    by_k = {k: median(timed(k)) for k in range(1, 5)}
    full = timed(5)
    by_k[5] = median(full)
    e0, e1, cms = C.c_void_p(), C.c_void_p(), C.c_float(0)
    assert hip.hipEventCreate(C.byref(e0)) == 0 and hip.hipEventCreate(C.byref(e1)) == 0
    copies = []
    for i in range(3):
        assert hip.hipEventRecord(e0, None) == 0
        for _ in range(20):
            assert hip.hipMemcpyAsync(d_copy, d_gb, C.c_size_t(n * 32), 3, None) == 0
        assert hip.hipEventRecord(e1, None) == 0 and hip.hipEventSynchronize(e1) == 0
        assert hip.hipEventElapsedTime(C.byref(cms), e0, e1) == 0
        copies.append(cms.value / 20)
    hip.hipEventDestroy(e0), hip.hipEventDestroy(e1)
    out = np.zeros((h, w, 4), np.float32)
    gpu._chk(gpu.L.hpt_device_copy(gpu.h, out.ctypes.data, d_out, out.nbytes, 2))
    for p in ptr:
        gpu._chk(gpu.L.hpt_device_free(gpu.h, p))
    if dump:
        os.makedirs(dump, exist_ok=True)
        np.save(os.path.join(dump, f"denoise_{w}x{h}.npy"), out)
    print(json.dumps({"size": f"{w}x{h}", "pixels": n, "repeats": repeats, "device": gpu.device_info()["arch"],
                      "call_ms_min": round(min(full), 4), "call_ms_median": round(by_k[5], 4), "call_ms_max": round(max(full), 4),
                      "ms_k": {k: round(v, 4) for k, v in by_k.items()},
                      "pass_ms": {f"step {1 << (k - 1)}": round(by_k[k] - by_k[k - 1], 4) for k in range(2, 6)},
                      "copy_ms": round(min(copies[1:]), 4), "gpixels_per_s": round(n / by_k[5] / 1e6, 3),
                      "finite": bool(np.isfinite(out).all()), "mean": round(float(out[..., :3].mean()), 5)}), flush=True)
