"""Measurements of the light-colour gradients (profiles/light_grad.md).

  python profiles/light_grad.py surcharge [--spp S] [--reps R]
      (b) PathTraceVJP on the `dr` workload's scene (test_228 class, 512 x 512) with its albedo texture registered, with and without its
      lights registered, under the megakernel and the wavefront schedule: kernel time of each call (hpt_last_kernel_ms). Prints one JSON line.
      With HYDRA_HIP_LIB pointing at the diagnostic build that sends every term straight to a global atomic
      (`python __graft_entry__.py unit lgnaive pt20,wf_shade_lights -DHPT_LGRAD_NAIVE`) the same run is (c)'s other half.
  python profiles/light_grad.py many [--spp S] [--reps R]
      (c) the same pair of timings on a scene with few words to add to and every lane adding to them: 8 point lights over a floor that fills the frame.
  python profiles/light_grad.py ab --parent-root DIR [--rounds N]
      (a) bench.py --workload dr / dr_interior of a checkout of the parent commit (DIR, its library built) and of this tree, alternating, on
      the same card; nothing registered. Prints every value."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _time_vjp(sc, tex, with_lights, schedule, spp, reps):
    import numpy as np
    from hydracore3_amd.api import HipIntegrator
    gpu = HipIntegrator(sc)
    if schedule == 2:
        gpu.set_schedule(2, 56, 0, 1)
    else:
        gpu.set_schedule(schedule)
    size = 0
    if tex is not None:
        size = sum(gpu.PutDiffTex2D(*tex))
    n = len(sc.lights)
    if with_lights:
        off, sz = gpu.PutDiffLights(0, n)
        size = off + sz
    data = np.full(max(size, 4), 0.5, np.float32)
    if with_lights:
        data[off:] = 1.0
    adj = np.random.default_rng(1).uniform(-1.0, 1.0, (gpu.H, gpu.W, 4)).astype(np.float32)
    grad, ms = np.zeros_like(data), []
    for _ in range(reps + 1):
        gpu.PathTraceVJP(gpu.N, 4, np.zeros((gpu.H, gpu.W, 4), np.float32), spp, adj, data, grad)
        ms.append(round(gpu.last_kernel_ms(), 3))
    assert gpu.last_schedule()[0] == schedule
    return ms[1:]                                                   # (the first call warms up: allocations, first launches)


def surcharge(args):
    from hydracore3_amd.synth import dr_scene
    sc, tex_id = dr_scene(os.path.join(ROOT, "tests", "golden", "scenes", "test_228", "statex_00001.xml"), 512, 512)
    out = {"lib": os.environ.get("HYDRA_HIP_LIB", "product"), "scene": "dr workload (test_228 class), 512 x 512", "spp": args.spp, "lights": len(sc.lights)}
    for schedule in (1, 2):
        for with_lights in (False, True):
            out[f"schedule {schedule}, lights {'registered' if with_lights else 'not registered'}: kernel ms"] = \
                _time_vjp(sc, (tex_id, 256, 256, 4), with_lights, schedule, args.spp, args.reps)
    print(json.dumps(out))


def many(args):
    import numpy as np
    from hydracore3_amd import scene as S
    from hydracore3_amd.synth import _quad
    sc = S.SceneData()
    sc.width, sc.height, sc.trace_depth, sc.fov = 512, 512, 4, 50.0
    sc.cam_pos, sc.cam_look_at, sc.cam_up = (0.0, 3.0, 0.01), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0)
    sc.materials.append(S.material_gltf((0.8, 0.8, 0.8, 1.0), 0.0, 0.3, 0.0, 1.5))
    sc.add_instance(sc.add_mesh(*_quad((-20, 0, 20), (40, 0, 0), (0, 0, -40), 2, 2), [0]), np.eye(4))
    for i in range(8):
        sc.lights.append(S.light_point(S.translate(-1.5 + 1.0 * (i % 4), 1.0, -0.5 + 1.0 * (i // 4)), (1.0, 0.9, 0.8), 10.0, "omni"))
    out = {"lib": os.environ.get("HYDRA_HIP_LIB", "product"), "scene": "floor filling a 512 x 512 frame under 8 point lights, depth 4", "spp": args.spp}
    for schedule in (1, 2):
        for with_lights in (False, True):
            out[f"schedule {schedule}, lights {'registered' if with_lights else 'not registered'}: kernel ms"] = _time_vjp(sc, None, with_lights, schedule, args.spp, args.reps)
    print(json.dumps(out))


def ab(args):
    trees = [("parent", os.path.abspath(args.parent_root)), ("this", ROOT)]
    for workload, extra in (("dr", []), ("dr_interior", ["--spp", "64"])):
        for r in range(args.rounds):
            for name, root in trees:
                env = {k: v for k, v in os.environ.items() if k != "HYDRA_HIP_LIB"}
                t0 = time.time()
                p = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--workload", workload, "--steps", "3", "--warmup", "1",
                                    "--no-cpu-baseline", "--no-also", "--no-build"] + extra, env=env, cwd=root, capture_output=True, text=True, timeout=600)
                line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
                value = json.loads(line[-1]).get("value") if line else None
                print(json.dumps({"workload": workload, "round": r, "lib": name, "value": value, "rc": p.returncode, "seconds": round(time.time() - t0, 1)}), flush=True)
                if p.returncode != 0:
                    print(p.stderr[-2000:], file=sys.stderr)
                    return 1
    return 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["surcharge", "many", "ab"])
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent-root", default=None)
    a = ap.parse_args()
    sys.exit({"surcharge": surcharge, "many": many, "ab": ab}[a.mode](a) or 0)
