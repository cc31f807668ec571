"""CommitScene of two-level scenes: the host's builder against hpt_set_option("device_build_two_level", 1). Medians of --reps runs, one JSON line each.
  1  the 1 M-triangle interior forced two-level: every mesh handed in again (UpdateGeom_Triangles3f), then the commit - a full build
  2  the same scene: UpdateInstance of 5 % of the instances, then the commit (device: the TLAS kernels only)
  3  10^5 instances of one 320-triangle sphere: the full build, and the commit after UpdateInstance of 5 % of them
  4  Mpaths/s through the committed tree: legacy_materials (a moving sphere) at 1024^2 x 64 spp, the interior forced two-level at 1920 x 1080 x 8 spp
Timed: the CommitScene call alone (wall clock; the Update* calls before it are not), and PathTraceBlock's kernel time.
Usage: python profiles/device_two_level.py --mode host|device [--what 1,2,3,4] [--reps 10] [--root DIR]   (DIR: the checkout whose package is measured;
the host mode sets no option, so it runs on checkouts from before the option too)"""
import argparse
import json
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--mode", choices=("host", "device"), required=True)
ap.add_argument("--what", default="1,2,3,4")
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.root))
import numpy as np
from hydracore3_amd import synth, scene as S
from hydracore3_amd.api import HipIntegrator
from hydracore3_amd.scene import load_hydra_xml

DEVICE = args.mode == "device"
WHAT = {int(w) for w in args.what.split(",")}
OPTIONS = 1 if DEVICE else 4


def report(name, values, **extra):
    v = np.asarray(values, np.float64)
    print(json.dumps({"mode": args.mode, "measurement": name, "median": float(np.median(v)), "min": float(v.min()), "max": float(v.max()), "reps": int(v.size), **extra}), flush=True)


def context(sc, layout=1):
    g = HipIntegrator(sc, accel_layout=layout)
    if DEVICE:
        g.set_option("device_build_two_level", 1)
        g.CommitScene(OPTIONS)
        assert g.commit_time()["device_built"] and g.two_level_info()["device_built"], (g.commit_time(), g.two_level_info())
    return g


def timed_commit(g):
    t = time.perf_counter()
    g.CommitScene(OPTIONS)
    return (time.perf_counter() - t) * 1e3


def rebuild_all(g, sc):
    """Every mesh handed in again, then the commit: all BLAS and the TLAS are built."""
    for geom in range(len(sc.geom_tri_count)):
        to, vo = sc.mat_vert_offset[geom]
        nv, nt = sc.geom_vert_count[geom], sc.geom_tri_count[geom]
        g.UpdateGeom_Triangles3f(geom, sc.vpos[vo:vo + nv], np.ascontiguousarray(sc.tri_indices[3 * to:3 * (to + nt)]))
    return timed_commit(g)


def full_builds(g, sc, name):
    if DEVICE:
        g.set_option("refit", 0)                                            # a full device build, not the in-place update of every mesh
    ms, stages = [], []
    for _ in range(args.reps):
        ms.append(rebuild_all(g, sc))
        if DEVICE:
            info = g.two_level_info()
            assert info["device_built"] and info["blas_kept"] == 0, info
            stages.append((info["blas_ms"], info["tlas_ms"]))
    extra = {"blas_ms": float(np.median([s[0] for s in stages])), "tlas_ms": float(np.median([s[1] for s in stages]))} if DEVICE else {}
    report(name, ms, unit="ms", sah_node_visits=g.accel_info()["sah_node_visits"], commit=g.commit_time(), **extra)
    if DEVICE:
        g.set_option("refit", 1)
        g.CommitScene(OPTIONS)


def instance_updates(g, sc, name):
    rng = np.random.default_rng(11)
    ni = len(sc.inst_geom)
    ms, stages = [], []
    for _ in range(args.reps):
        for i in rng.choice(ni, max(1, ni // 20), replace=False):
            g.UpdateInstance(int(i), S.translate(*rng.uniform(-0.05, 0.05, 3)) @ np.asarray(sc.inst_matrices[i]))
        ms.append(timed_commit(g))
        if DEVICE:
            info = g.two_level_info()
            assert info["tlas_only"], info
            stages.append(info["tlas_ms"])
    report(name, ms, unit="ms", instances=ni, updated=max(1, ni // 20), **({"tlas_ms": float(np.median(stages))} if DEVICE else {}))


def mpaths(g, sc, spp, name):
    out = np.zeros((sc.height, sc.width, 4), np.float32)
    g.render(2)
    v = []
    for _ in range(args.reps):
        g.PathTraceBlock(g.N, 4, out, spp)
        v.append(sc.width * sc.height * spp / (g.GetExecutionTime("PathTraceBlock")[0] * 1e3))
    report(name, v, unit="Mpaths/s", sah_node_visits=g.accel_info()["sah_node_visits"], schedule=g.last_schedule()[0])


def sphere_field(n=100000):
    """n instances of one 320-triangle icosphere on a jittered grid over a floor-less scene lit by one rect light."""
    rng = np.random.default_rng(7)
    sc = S.SceneData()
    sc.width, sc.height = 256, 256
    sc.cam_pos, sc.cam_look_at, sc.cam_up = (0.0, 40.0, 120.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0)
    sc.fov, sc.trace_depth = 50.0, 4
    sc.env_color = (0.3, 0.3, 0.3, 0.0)
    sc.materials.append(S.material_lambert((0.6, 0.55, 0.5)))
    sc.lights.append(S.light_rect(S.translate(0.0, 60.0, 0.0), 20.0, 20.0, (1, 1, 1), 12.0))
    pos4, norm4, tang4, uv, idx = synth._sphere_mesh(2)
    geom = sc.add_mesh(pos4, norm4, tang4, uv, idx, np.zeros(idx.size // 3, np.uint32))
    side = int(np.ceil(n ** (1.0 / 3.0)))
    k = np.arange(n)
    grid = np.stack([k % side, (k // side) % side, k // (side * side)], 1) - side / 2.0
    centre = grid * 2.5 + rng.uniform(-0.4, 0.4, (n, 3))
    radius = rng.uniform(0.4, 1.0, n)
    for c, r in zip(centre, radius):
        sc.add_instance(geom, S.translate(*c) @ S.scale(r, r, r))
    return sc


if WHAT & {1, 2, 4}:
    t0 = time.time()
    interior = synth.interior_scene(1920, 1080, tex_size=256)
    g = context(interior)
    print(f"# interior: {sum(interior.geom_tri_count)} triangles, {len(interior.inst_geom)} instances, {time.time() - t0:.1f} s to make and load", flush=True)
    if 1 in WHAT:
        full_builds(g, interior, "1 interior-1M full build")
    if 2 in WHAT:
        instance_updates(g, interior, "2 interior-1M UpdateInstance 5 % + commit")
    if 4 in WHAT:
        fresh = context(interior)                                           # the tree as built, not as the updates left it
        mpaths(fresh, interior, 8, "4 interior-1M two-level Mpaths/s")
        del fresh
    del g
if 3 in WHAT:
    t0 = time.time()
    field = sphere_field()
    g = context(field)
    print(f"# sphere field: {sum(field.geom_tri_count)} triangles in {len(field.geom_tri_count)} mesh, {len(field.inst_geom)} instances, {time.time() - t0:.1f} s to make and load", flush=True)
    full_builds(g, field, "3 10^5 sphere instances full build")
    instance_updates(g, field, "3 10^5 sphere instances UpdateInstance 5 % + commit")
    del g
if 4 in WHAT:
    root = os.path.abspath(args.root)
    legacy = load_hydra_xml(os.path.join(root, "tests", "golden", "scenes", "legacy_materials", "statex_00001.xml"), 1024, 1024)
    g = context(legacy, layout=0)                                           # (the automatic layout keeps two-level for the moving sphere)
    assert g.accel_info()["layout"] == "two-level", g.accel_info()
    mpaths(g, legacy, 64, "4 legacy_materials Mpaths/s")
