"""Treelet passes of the device build (hpt_set_option("device_build_quality", p)) on the 1 M-triangle interior: CommitScene time, surface-area
estimate, depth, nodes per ray and Mpaths/s under the wavefront schedule for p = 0 .. 3, with the host's SAH tree measured in the same session.
Commits: medians of 10 after 2 warm-ups (wall around CommitScene, and hpt_get_commit_time / hpt_get_build_info); throughput: median kernel time of
3 frames after one warm-up frame (HIP events, hpt_last_kernel_ms). Clocks as found.
Run on a GPU box: python profiles/device_quality.py [--small] [--out=FILE] [spp]   (results: profiles/device_quality.md)"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from hydracore3_amd import synth
from hydracore3_amd.api import HipIntegrator

os.environ["HPT_DEBUG_ACCEL"] = "1"                                         # the depth of every tree goes to stderr with the commit
small = "--small" in sys.argv
args = [a for a in sys.argv[1:] if not a.startswith("--")]
spp = int(args[0]) if args else 8
W, H = (480, 270) if small else (1920, 1080)
sc = synth.interior_scene(W, H, subdiv=1, tex_size=16) if small else synth.interior_scene(W, H, tex_size=256)
out = {}
for name, dev, passes in [("host SAH", 0, 0)] + [(f"device, {p} passes", 1, p) for p in range(4)]:
    g = HipIntegrator(sc)
    g.set_option("device_build", dev); g.set_option("refit", 0); g.set_option("device_build_quality", passes)
    wall, devms, passms = [], [], []
    for it in range(12 if dev else 3):                                       # (the host build takes a quarter of a second: 3 commits, the last one reported)
        g.set_option("device_build", dev)                                    # uncommits: the next CommitScene builds
        t0 = time.perf_counter(); g.CommitScene(1 if dev else 4); t1 = time.perf_counter()
        if it >= 2 or not dev:
            wall.append((t1 - t0) * 1e3); devms.append(g.commit_time()["device_ms"]); passms.append(g.build_info()["ms"])
    assert bool(g.commit_time()["device_built"]) == bool(dev)
    info, binfo = g.accel_info(), g.build_info()
    g.set_schedule(2)
    frame = g.dev_array(np.zeros((H, W, 4), np.float32))
    g.path_trace_block_dev(frame.ptr, spp)
    ms = []
    for _ in range(3):
        g.path_trace_block_dev(frame.ptr, spp); ms.append(g.last_kernel_ms())
    launch = g.last_launch()
    g.set_instrumentation(True); g.set_schedule(1); g.set_option("stats_wide", 1)
    probe = np.zeros((H, W, 4), np.float32); g.InitRandomGens(g.N); g.PathTraceBlock(g.N, 4, probe, 2)
    c = g.counters()
    out[name] = {"commit_wall_ms_median": float(np.median(wall)), "commit_wall_ms_min_max": [min(wall), max(wall)], "device_ms_median": float(np.median(devms)),
                 "pass_ms_median": float(np.median(passms)), "sah_node_visits": info["sah_node_visits"], "inst_tris": info["inst_tris"], "build_info": binfo,
                 "stack": g.refit_info(), "Mpaths_per_s": W * H * spp / float(np.median(ms)) / 1e3, "kernel_ms": ms, "launch": launch,
                 "nodes_per_ray": c["nodes"] / c["rays"], "tris_per_ray": c["tris"] / c["rays"]}
    print(name, json.dumps(out[name]), flush=True)
dest = [a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--out=")]
if dest:                                                                    # every row was printed above; --out=FILE keeps them as one JSON document too
    json.dump(out, open(dest[0], "w"), indent=1)
