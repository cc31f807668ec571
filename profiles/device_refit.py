"""UpdateInstance + CommitScene on the device-built tree of the 1M-triangle interior: as a device refit (hpt_set_option("device_refit", 1))
against the device rebuild that answers the same call without the option, and what the refitted trees cost a frame: Mpaths/s through the
refitted tree and through a rebuilt one after (a) 5 % of the instances moved by up to one object size, (b) the pair exchange of
tests/test_device_refit_gpu.py, with hpt_get_refit_info's estimates next to each. Clocks as found; medians of 10 after 2 warm-ups.
Run on a GPU box: python profiles/device_refit.py [--small]   (results: profiles/device_refit.md)"""
import sys, os, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from hydracore3_amd import synth, scene as S
from hydracore3_amd.api import HipIntegrator

small = "--small" in sys.argv
W, H, SPP = (480, 270, 4) if small else (1920, 1080, 4)
make = (lambda: synth.interior_scene(W, H, subdiv=2, tex_size=64)) if small else (lambda: synth.interior_scene(W, H, tex_size=256))
t0 = time.time(); sc = make(); print(f"scene synth {time.time() - t0:.2f} s, {sum(sc.geom_tri_count[g] for g in sc.inst_geom)} instanced triangles", flush=True)


def context(refit):
    g = HipIntegrator(sc, accel_layout=2)
    g.set_option("device_build", 1); g.set_option("device_refit", refit); g.CommitScene(1)
    assert g.commit_time()["device_built"]
    return g


def tables(g, scene):
    d = scene.desc(); d.vPos4f = None
    g._desc = d; g.scene = scene
    g.CommitDeviceData(); g.InitRandomGens(g.N)


def median_commit(g, label):
    """UpdateInstance(40) + CommitScene(BUILD_LOW), the instance alternating between two places: wall ms and the ms hpt_get_commit_time reports."""
    ms = [S.translate(0.3, 0.0, 0.1) @ np.asarray(sc.inst_matrices[40]), np.asarray(sc.inst_matrices[40])]
    wall, dev, kinds = [], [], set()
    for k in range(12):
        t = time.perf_counter(); g.UpdateInstance(40, ms[k & 1]); g.CommitScene(1); t = (time.perf_counter() - t) * 1e3
        ct = g.commit_time()
        kinds.add("refit" if ct["refitted"] else "device build" if ct["device_built"] else "host build")
        if k >= 2:
            wall.append(t); dev.append(ct["device_ms"])
    print(f"{label}: {sorted(kinds)}; wall median {np.median(wall):.3f} ms (min {min(wall):.3f}, max {max(wall):.3f}); "
          f"device part median {np.median(dev):.3f} ms; last commit {g.commit_time()}", flush=True)


def mpaths(g, label):
    g.render(1)
    ms = []
    for _ in range(3):
        g.render(SPP); ms.append(g.last_kernel_ms())
    info = g.refit_info()
    print(f"   {label}: {g.N * SPP / np.median(ms) / 1e3:.1f} Mpaths/s (kernel {np.median(ms):.2f} ms, schedule {g.last_schedule()[0]}, wide {g.last_launch()['wide_nodes']}); "
          f"estimate at build {info['build']:.2f}, now {info['after']:.2f} ({info['after'] / info['build']:.3f} x)", flush=True)


refit, rebuild = context(1), context(0)
print(f"device build: {refit.commit_time()}; refit levels {refit.refit_info()['levels']}", flush=True)
median_commit(refit, "device refit  ")
median_commit(rebuild, "device rebuild")
mpaths(refit, "tree as built")

rng = np.random.default_rng(11)
n = len(sc.inst_matrices)
moved = make()
some = rng.choice(np.arange(2, n), max(1, (n - 2) // 20), replace=False)
for i in some:                                                            # 5 % of the objects, by up to one object size (radius 0.18 .. 0.30)
    moved.inst_matrices[i] = S.translate(*rng.uniform(-0.5, 0.5, 3)) @ np.asarray(moved.inst_matrices[i])
exchanged = make()
for k in range((n - 2) // 2):
    a, b = 2 + k, n - 1 - k
    ma, mb = np.array(exchanged.inst_matrices[a], np.float64), np.array(exchanged.inst_matrices[b], np.float64)
    ta, tb = ma[:3, 3].copy(), mb[:3, 3].copy()
    ma[:3, 3], mb[:3, 3] = tb, ta
    exchanged.inst_matrices[a], exchanged.inst_matrices[b] = ma, mb
for name, scene in (("5 % of the instances moved", moved), ("pair exchange", exchanged)):
    print(name, flush=True)
    for g, what in ((refit, "refitted"), (rebuild, "rebuilt ")):
        for i in range(2, n):
            g.UpdateInstance(i, scene.inst_matrices[i])
        g.CommitScene(1)
        ct = g.commit_time()
        assert ct["refitted"] == (g is refit) and ct["device_built"] == (g is rebuild)
        tables(g, scene)
        mpaths(g, what)
