"""Measurements (a) and (b) of profiles/adaptive_spectral.md on the spectral Cornell fixture (tests/golden/scenes/test_spectral under m_spectral_mode = 1)
at the benchmark's size, 1024 x 1024: python profiles/adaptive_spectral.py
(a) a uniform spectral PathTraceBlock of 64 passes - as the benchmark runs it (schedule 0) and on the one-thread-per-pixel kernel (schedule 1), the ADAPT
    kernels' parent - against the counts call with null arrays, with 64 everywhere, and with moments: what the ADAPT form and its records cost;
(b) the loop with the Python front end's defaults (step = ADAPTIVE_STEP_DEFAULT, dilate 0) against uniform calls, by the mean relative luminance error
    against a 512-pass frame of other samples; the uniform call of the loop's error is interpolated on error ~ passes^-1/2.
Times are the launches' event pairs (hpt_last_kernel_ms; the loop sums its rounds in deviceMs). The variants of a table alternate within every
repetition: one warm-up round, then REPS rounds, min .. max. Prints one JSON line per table."""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from hydracore3_amd.api import HipIntegrator, MOMENTS_DTYPE, ADAPTIVE_STEP_DEFAULT, _vp  # noqa: E402
from hydracore3_amd.scene import load_hydra_xml  # noqa: E402

SIZE, REPS, K = 1024, 5, 64
g = HipIntegrator(load_hydra_xml(os.path.join(ROOT, "tests", "golden", "scenes", "test_spectral", "statex_00001.xml"), SIZE, SIZE, spectral=True))
g.set_option("adaptive_spectral", 1)
N = g.N
gens0 = g.random_gens()


def dev(nbytes):
    p = _vp()
    g._chk(g.L.hpt_device_malloc(g.h, nbytes, C.byref(p)))
    g._chk(g.L.hpt_device_memset(g.h, p, 0, nbytes))
    return p


d_img, d_mom, d_cnt = dev(N * 16), dev(N * 16), dev(N * 4)
cnt = np.full(N, K, np.uint32)
g._chk(g.L.hpt_device_copy(g.h, d_cnt, cnt.ctypes.data, cnt.nbytes, 1))


def span(ms):
    return {"min": round(min(ms), 3), "max": round(max(ms), 3), "all": [round(m, 3) for m in ms]}


def alternate(variants):
    """{name: f} -> {name: span}: every round runs each variant once, in order; the first round is the warm-up."""
    ms = {k: [] for k in variants}
    for r in range(REPS + 1):
        for name, f in variants.items():
            g.set_random_gens(gens0)
            f()
            t = g.last_kernel_ms()                                         # (waits for the launch's second event)
            if r:
                ms[name].append(t)
    return {k: span(v) for k, v in ms.items()}


# ---- (a) the ADAPT form and its records ------------------------------------------------------------------------------------------------------
def uniform(schedule):
    def f():
        g.set_schedule(schedule)
        g.path_trace_block_dev(d_img, K)
    return f


def counts(counts_ptr, mom_ptr):
    def f():
        g.set_schedule(0)
        g.PathTraceBlockCounts_dev(d_img, 0 if counts_ptr else K, counts_ptr, mom_ptr)
    return f


a = {"k": K, "size": SIZE}
a["ms"] = alternate({"uniform_schedule0": uniform(0), "uniform_schedule1": uniform(1), "counts_null_arrays": counts(None, None),
                     "counts_64_everywhere": counts(d_cnt, None), "counts_64_with_moments": counts(d_cnt, d_mom), "passnum_with_moments": counts(None, d_mom)})
g.set_schedule(0); g.path_trace_block_dev(d_img, K); a["uniform_schedule0_ran"] = g.last_launch()["schedule"]
g.PathTraceBlockCounts_dev(d_img, K, None, None); a["counts_ran"] = g.last_launch()["schedule"]
print(json.dumps({"a": a}), flush=True)

# ---- (b) what the loop buys ------------------------------------------------------------------------------------------------------------------
FLOOR = 0.01
xy = g.packed_xy()
pix = ((xy >> 16) * np.uint32(g.W) + (xy & 0xFFFF)).astype(np.int64)


def lum(rgb):
    return 0.2126 * rgb[..., 0] + 0.7152 * rgb[..., 1] + 0.0722 * rgb[..., 2]


def download_frame():
    img = np.zeros((N, 4), np.float32)
    g._chk(g.L.hpt_device_copy(g.h, img.ctypes.data, d_img, img.nbytes, 2))
    return img[pix].astype(np.float64)                                     # tid order


def clear():
    g._chk(g.L.hpt_device_memset(g.h, d_img, 0, N * 16)); g._chk(g.L.hpt_device_memset(g.h, d_mom, 0, N * 16))


g.set_schedule(0)
g.set_random_gens(gens0)
clear(); g.path_trace_block_dev(d_img, 512)
ref = lum(download_frame()[:, :3] / 512.0)
gens1 = g.random_gens()                                                    # the streams continue: every frame below is made of other samples than the reference


def error(frame_lum):
    return float(np.mean(np.abs(frame_lum - ref) / (np.abs(ref) + FLOOR)))


b = {"reference_passes": 512, "uniform": [], "loop": []}
for n in (16, 32, 64, 128, 256):
    ms = []
    for r in range(3):
        g.set_random_gens(gens1); clear(); g.path_trace_block_dev(d_img, n); ms.append(g.last_kernel_ms())
    b["uniform"].append({"passes": n, "ms": span(ms), "error": error(lum(download_frame()[:, :3] / n))})
mom = np.zeros(N, MOMENTS_DTYPE)
for tol, min_p, max_p in ((0.1, 8, 256), (0.05, 16, 256), (0.05, 16, 1024)):
    ms, info = [], None
    for r in range(3):
        g.set_random_gens(gens1); clear()
        info = g.PathTraceBlockAdaptive_dev(d_img, 64, d_mom, tol=tol, lum_floor=FLOOR, min_passes=min_p, max_passes=max_p)    # step and dilate: the front end's defaults
        ms.append(info["deviceMs"])
    g._chk(g.L.hpt_device_copy(g.h, mom.ctypes.data, d_mom, mom.nbytes, 2))
    e = error(lum(download_frame()[:, :3] / np.maximum(mom["passes"], 1)[:, None]))
    u = b["uniform"]
    n_equal = [r["passes"] * (r["error"] / e) ** 2 for r in u]             # error ~ passes^-1/2, from every uniform row
    near = min(range(len(u)), key=lambda i: abs(np.log(u[i]["error"] / e)))
    b["loop"].append({"tol": tol, "min_passes": min_p, "max_passes": max_p, "step": ADAPTIVE_STEP_DEFAULT, "dilate": 0, "rounds": info["rounds"], "mean_passes": info["passes"] / N,
                      "largest": info["maxPasses"], "pixels_short": info["pixels"], "device_ms": span(ms), "error": e,
                      "uniform_passes_same_error": n_equal[near], "uniform_ms_same_error": u[near]["ms"]["min"] * n_equal[near] / u[near]["passes"]})
print(json.dumps({"b": b}), flush=True)
