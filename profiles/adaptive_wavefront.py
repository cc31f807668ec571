"""Measurements (a) and (b) of profiles/adaptive_wavefront.md on the bench's 1 M-triangle interior at 1920 x 1080: python profiles/adaptive_wavefront.py
(a) the adaptive loop with "adaptive_wavefront" off (every round on the megakernel) against on (per-round choice), identical parameters and generators;
(b) a bare counts call, every count 64, moments on, under the wavefront form against a uniform 64-pass wavefront PathTraceBlock: the price of the
    moments' read-modify-write and of the summary's read-back.
Times are the launches' event pairs (hpt_last_kernel_ms; the loop sums its rounds in deviceMs): one warm-up, then REPS repetitions, min .. max.
Prints one JSON line per table."""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from hydracore3_amd.api import HipIntegrator, ADAPTIVE_INFO_DTYPE, _vp  # noqa: E402
from hydracore3_amd.synth import interior_scene  # noqa: E402

W, H, REPS = 1920, 1080, 5
LOOP = dict(tol=0.05, lum_floor=0.01, min_passes=16, max_passes=128, step=32, dilate=1)
ROUNDS = 16

g = HipIntegrator(interior_scene(W, H, subdiv=int(os.environ.get("HYDRA_BENCH_SUBDIV", "4"))))
N = g.N
gens0 = g.random_gens()


def dev(nbytes):
    p = _vp()
    g._chk(g.L.hpt_device_malloc(g.h, nbytes, C.byref(p)))
    g._chk(g.L.hpt_device_memset(g.h, p, 0, nbytes))
    return p


d_img, d_mom, d_cnt, d_info = dev(N * 16), dev(N * 16), dev(N * 4), dev(32)


def span(ms):
    return {"min": round(min(ms), 2), "max": round(max(ms), 2), "all": [round(m, 2) for m in ms]}


# ---- (a) the loop ------------------------------------------------------------------------------------------------------------------------------
def loop(on):
    g.set_option("adaptive_wavefront", int(on))
    g.set_random_gens(gens0)
    g._chk(g.L.hpt_device_memset(g.h, d_img, 0, N * 16))
    return g.PathTraceBlockAdaptive_dev(d_img, ROUNDS, d_mom, **LOOP)


def round_log(on):
    """The loop's rounds replayed through the low-level entries: active pixels, passes and the schedule each round ran under."""
    g.set_option("adaptive_wavefront", int(on))
    g.set_random_gens(gens0)
    g._chk(g.L.hpt_device_memset(g.h, d_img, 0, N * 16)); g._chk(g.L.hpt_device_memset(g.h, d_mom, 0, N * 16))
    g.PathTraceBlockCounts_dev(d_img, LOOP["min_passes"], None, d_mom)
    log = [{"active": N, "passes": LOOP["min_passes"] * N, "schedule": g.last_launch()["schedule"], "ms": round(g.last_kernel_ms(), 2)}]
    info = np.zeros(1, ADAPTIVE_INFO_DTYPE)
    for _ in range(ROUNDS):
        g.AdaptivePlan_dev(d_mom, d_cnt, d_info, **LOOP)
        g._chk(g.L.hpt_device_copy(g.h, info.ctypes.data, d_info, 32, 2))
        if int(info[0]["passes"]) == 0:
            break
        g.PathTraceBlockCounts_dev(d_img, 0, d_cnt, d_mom)
        log.append({"active": int(info[0]["pixels"]), "passes": int(info[0]["passes"]), "schedule": g.last_launch()["schedule"], "ms": round(g.last_kernel_ms(), 2)})
    return log


g.set_schedule(0)
a = {"params": LOOP, "max_rounds": ROUNDS, "pixels": N}
for on in (False, True):
    loop(on)                                                               # warm-up
    infos = [loop(on) for _ in range(REPS)]
    a["on" if on else "off"] = {"device_ms": span([i["deviceMs"] for i in infos]), "rounds": infos[0]["rounds"], "passes": infos[0]["passes"], "round_log": round_log(on)}
print(json.dumps({"a": a}), flush=True)

# ---- (b) the moments and the summary ---------------------------------------------------------------------------------------------------------
K = 64
cnt = np.full(N, K, np.uint32)
g._chk(g.L.hpt_device_copy(g.h, d_cnt, cnt.ctypes.data, cnt.nbytes, 1))
g.set_schedule(2)
g.set_option("adaptive_wavefront", 1)


def timed(f):
    f(); g.last_kernel_ms()
    ms = []
    for _ in range(REPS):
        f()
        ms.append(g.last_kernel_ms())                                      # (waits for the launch's second event)
    return span(ms)


b = {"k": K, "uniform_wavefront_ms": timed(lambda: g.path_trace_block_dev(d_img, K))}
b["uniform_schedule"] = g.last_launch()["schedule"]
b["counts_with_moments_ms"] = timed(lambda: g.PathTraceBlockCounts_dev(d_img, 0, d_cnt, d_mom))
b["counts_schedule"] = g.last_launch()["schedule"]
b["counts_no_moments_ms"] = timed(lambda: g.PathTraceBlockCounts_dev(d_img, 0, d_cnt, None))
b["uniform_passnum_with_moments_ms"] = timed(lambda: g.PathTraceBlockCounts_dev(d_img, K, None, d_mom))
print(json.dumps({"b": b}), flush=True)
