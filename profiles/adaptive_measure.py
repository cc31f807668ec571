"""Measurements (b) and (c) of profiles/adaptive.md on the Cornell headline shape (1024 x 1024): python profiles/adaptive_measure.py
Prints one JSON line per table."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from hydracore3_amd.api import HipIntegrator, MOMENTS_DTYPE, _vp  # noqa: E402
from hydracore3_amd.scene import load_hydra_xml  # noqa: E402
import ctypes as C  # noqa: E402

out = {}
sc = load_hydra_xml(os.path.join(ROOT, "tests", "golden", "scenes", "test_035", "statex_00001.xml"), 1024, 1024)
g = HipIntegrator(sc)
N = g.N


def dev(nbytes):
    p = _vp()
    g._chk(g.L.hpt_device_malloc(g.h, nbytes, C.byref(p)))
    g._chk(g.L.hpt_device_memset(g.h, p, 0, nbytes))
    return p


d_img, d_mom, d_cnt = dev(N * 16), dev(N * 16), dev(N * 4)


def timed(f, reps=5):
    f(); g.last_kernel_ms()
    ms = []
    for _ in range(reps):
        f()
        ms.append(g.last_kernel_ms())                       # (waits for the launch's second event)
    return [round(m, 3) for m in ms]


# (b) cost of the ADAPT form on the Cornell headline shape, k = 256 passes per pixel
K = 256
cnt = np.full(N, K, np.uint32)
g._chk(g.L.hpt_device_copy(g.h, d_cnt, cnt.ctypes.data, cnt.nbytes, 1))
out["b"] = {"k": K,
            "PathTraceBlock_whole_pixels_ms": None, "PathTraceBlock_default_ms": timed(lambda: g.path_trace_block_dev(d_img, K)),
            "counts_no_moments_ms": timed(lambda: g.PathTraceBlockCounts_dev(d_img, 0, d_cnt, None)),
            "counts_with_moments_ms": timed(lambda: g.PathTraceBlockCounts_dev(d_img, 0, d_cnt, d_mom)),
            "uniform_passnum_with_moments_ms": timed(lambda: g.PathTraceBlockCounts_dev(d_img, K, None, d_mom))}
out["b"]["default_pass_slice"] = g.last_launch()
g.set_option("pass_slice", 0)
out["b"]["PathTraceBlock_whole_pixels_ms"] = timed(lambda: g.path_trace_block_dev(d_img, K))
print(json.dumps(out["b"]), flush=True)

# (c) what adaptivity buys: the figure mean sqrt(var / n) / (|mean| + lumFloor) of a uniform call, then the loop at several steps
FLOOR = 0.01


def figure(mom):
    n = mom["passes"].astype(np.float64)
    mean = mom["sumY"].astype(np.float64) / n
    var = np.maximum(mom["sumY2"].astype(np.float64) / n - mean * mean, 0.0)
    return float(np.mean(np.sqrt(var / n) / (np.abs(mean) + FLOOR)))


g = HipIntegrator(sc)
d_img, d_mom, d_cnt = dev(N * 16), dev(N * 16), dev(N * 4)
U = 256
mom = np.zeros(N, MOMENTS_DTYPE)
g._chk(g.L.hpt_device_memset(g.h, d_mom, 0, N * 16))
g._chk(g.L.hpt_device_memset(g.h, d_img, 0, N * 16))
t0 = time.perf_counter()
g.PathTraceBlockCounts_dev(d_img, U, None, d_mom)
g._chk(g.L.hpt_device_copy(g.h, mom.ctypes.data, d_mom, mom.nbytes, 2))
uni_wall = (time.perf_counter() - t0) * 1e3
uni_ms = g.last_kernel_ms()
f_uni = figure(mom)
out["c"] = {"uniform_passes": U, "uniform_figure": f_uni, "uniform_kernel_ms": uni_ms, "uniform_wall_ms": uni_wall, "rows": []}
# a tolerance every pixel can reach within maxPasses, and rounds enough for the smallest step to get there (4096 / 16 = 256): the rows then
# differ in `step` alone, not in where a round limit cut them off
TOL, MIN_P, MAX_P, ROUNDS = 0.05, 16, 4096, 512
for step in (16, 64, 256, 1024, 4096):
    g._chk(g.L.hpt_device_memset(g.h, d_img, 0, N * 16))
    t0 = time.perf_counter()
    info = g.PathTraceBlockAdaptive_dev(d_img, ROUNDS, d_mom, tol=TOL, lum_floor=FLOOR, min_passes=MIN_P, max_passes=MAX_P, step=step, dilate=1)
    wall = (time.perf_counter() - t0) * 1e3
    g._chk(g.L.hpt_device_copy(g.h, mom.ctypes.data, d_mom, mom.nbytes, 2))
    f = figure(mom)
    n_equiv = U * (f_uni / f) ** 2                      # the figure of a uniform call falls as 1 / sqrt(passes)
    row = {"tol": TOL, "step": step, "rounds": info["rounds"], "passes_spent": info["passes"], "mean_passes": info["passes"] / N, "max_passes": info["maxPasses"],
           "pixels_short": info["pixels"], "pixels_at_cap": int((mom["passes"] >= MAX_P).sum()), "device_ms": info["deviceMs"], "wall_ms": wall, "figure": f,
           "uniform_passes_same_figure": n_equiv, "uniform_ms_same_figure": uni_ms * n_equiv / U}
    out["c"]["rows"].append(row)
    print(json.dumps(row), flush=True)
