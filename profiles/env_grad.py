"""Measurements of the environment-map gradients (profiles/env_grad.md).

  python profiles/env_grad.py share [--spp S] [--reps R] [--size N]
      PathTraceVJP on the box fixture of tests/env_grad_cases.py at N x N pixels (default 512) under a 16 x 8 and under a 1024 x 512 map, the
      map registered, env sampling on: kernel time (device events, hpt_get_execution_time) of the call with the adjoint image and of the same
      call with a null adjoint (the same kernel, nothing swept), alternating, after a warm-up call of each; megakernel and wavefront schedule.
      The sweep's share of a call is (t_adjoint - t_null) / t_adjoint. Prints every value and one JSON line.
  python profiles/env_grad.py ab --parent-lib FILE [--rounds N]
      bench.py --workload dr / dr_interior with the parent commit's library (HYDRA_HIP_LIB=FILE) and with this tree's, alternating, same
      arguments, one card. Prints every value."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def share(spp, reps, size):
    import numpy as np
    import env_grad_cases as E
    from hydracore3_amd.api import HipIntegrator
    E.MAPS.update({"16x8": (16, 8), "1024x512": (1024, 512)})
    E.WIDTH = E.HEIGHT = size
    adj = np.random.default_rng(5).uniform(-1.0, 1.0, (size, size, 4)).astype(np.float32)
    out = {}
    for schedule in (1, 2):
        for name in ("16x8", "1024x512"):
            w, h = E.MAPS[name]
            gpu = HipIntegrator(E.box_scene(name, True))
            gpu.set_schedule(schedule)
            gpu.set_option("dr_environment", 1)
            assert tuple(gpu.PutDiffTex2D(E.ENV_TEX, w, h, 4)) == (0, w * h * 4)
            data = E.env_image(name).reshape(-1)
            grad, frame = np.zeros_like(data), np.zeros((size, size, 4), np.float32)
            t = {"null": [], "adjoint": []}
            for rep in range(reps + 1):                                   # (rep 0: the warm-up of either form)
                for kind in ("null", "adjoint"):
                    gpu.PathTraceVJP(gpu.N, 4, frame, spp, adj if kind == "adjoint" else None, data, grad if kind == "adjoint" else None)
                    assert gpu.last_schedule()[0] == schedule
                    if rep:
                        t[kind].append(gpu.GetExecutionTime("PathTraceVJP")[0])
            med = {k: float(np.median(v)) for k, v in t.items()}
            out[f"schedule {schedule}, map {name}"] = {"null_ms": t["null"], "adjoint_ms": t["adjoint"], "median_null_ms": med["null"],
                                                         "median_adjoint_ms": med["adjoint"], "sweep_share": (med["adjoint"] - med["null"]) / med["adjoint"]}
            print(f"schedule {schedule}, map {name}, {size}x{size} @ {spp} spp: null {t['null']} adjoint {t['adjoint']} "
                  f"share {out[f'schedule {schedule}, map {name}']['sweep_share']:.4f}", flush=True)
    print(json.dumps(out))


def ab(parent_lib, rounds):
    for workload in ("dr", "dr_interior"):
        for r in range(rounds):
            for who, lib in (("parent", parent_lib), ("this", None)):
                env = dict(os.environ)
                if lib:
                    env["HYDRA_HIP_LIB"] = os.path.abspath(lib)
                p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--workload", workload],
                                   capture_output=True, text=True, env=env, timeout=600)
                if p.returncode != 0:
                    print(p.stderr[-2000:])
                    sys.exit(p.returncode)
                res = json.loads(p.stdout.strip().splitlines()[-1])
                print(f"{workload} round {r} {who}: {res['value']} {res['unit']} ({res['ms_per_step']} ms per step; {res['roofline']['kernel']})", flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["share", "ab"])
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--rounds", type=int, default=2)
    a = ap.parse_args()
    if a.what == "share":
        share(a.spp, a.reps, a.size)
    else:
        ab(a.parent_lib, a.rounds)
