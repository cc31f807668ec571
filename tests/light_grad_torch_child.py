"""The light-gain checks of hydracore3_amd.torch_dr, run as a process of its own by test_light_grad_gpu.py (torch's HIP runtime must come up
first, and must not be loaded into the pytest session). Prints one JSON line: {"backward[s]": the gain slice of params.grad, "adam": "ok" or what failed}."""
import json
import os
import sys
import traceback

import numpy as np
import torch

torch.cuda.init()                                       # before libhydra_hip.so brings its runtime up, as bench.py does

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

import light_grad_cases as G                            # noqa: E402
from hydracore3_amd import torch_dr                     # noqa: E402
from hydracore3_amd.api import HipIntegrator            # noqa: E402


def integrator(schedule):
    gpu = HipIntegrator(G.scene_a())
    if schedule == 2:
        gpu.set_schedule(2, 56, 0, 1)
    else:
        gpu.set_schedule(schedule)
    n = len(gpu.scene.lights)
    assert tuple(gpu.PutDiffLights(0, n)) == (0, 4 * n)
    return gpu, n


def backward(schedule):
    gpu, n = integrator(schedule)
    params = torch.tensor(G.gains(n).reshape(-1), device="cuda", requires_grad=True)
    img = torch_dr.render(gpu, params, 4)
    assert gpu.last_schedule()[0] == schedule
    (img * torch.tensor(G.adjoint(), device="cuda")).sum().backward()
    torch.cuda.synchronize()
    return [float(v) for v in params.grad.cpu().numpy()]


def adam():
    gpu, n = integrator(1)
    spp = 16
    truth = torch.tensor(G.gains(n).reshape(-1), device="cuda")
    with torch.no_grad():
        target = torch_dr.render(gpu, truth, spp) / spp
    params = torch.ones_like(truth).requires_grad_(True)
    opt = torch.optim.Adam([params], lr=0.05)
    losses = []
    for _ in range(30):
        opt.zero_grad()
        loss = ((torch_dr.render(gpu, params, spp) / spp - target)[..., :3] ** 2).mean()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    print("loss per step:", " ".join(f"{v:.5f}" for v in losses), file=sys.stderr)
    assert np.all(np.isfinite(losses)) and losses[-1] < losses[0], losses


if __name__ == "__main__":
    results = {}
    for s in G.SCHEDULES:
        try:
            results[f"backward[{s}]"] = backward(s)
        except Exception:
            results[f"backward[{s}]"] = traceback.format_exc()
    try:
        adam()
        results["adam"] = "ok"
    except Exception:
        results["adam"] = traceback.format_exc()
    print(json.dumps(results))
