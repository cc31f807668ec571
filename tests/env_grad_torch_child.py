"""The environment-map checks of hydracore3_amd.torch_dr, run as a process of its own by test_env_grad_gpu.py (torch's HIP runtime must come up
first, and must not be loaded into the pytest session). Prints one JSON line: {"backward[s]": the map's slice of params.grad, "adam": "ok" or
what failed}."""
import json
import os
import sys
import traceback

import numpy as np
import torch

torch.cuda.init()                                       # before libhydra_hip.so brings its runtime up, as bench.py does

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

import env_grad_cases as E                              # noqa: E402
from hydracore3_amd import torch_dr                     # noqa: E402
from hydracore3_amd.api import HipIntegrator            # noqa: E402


def integrator(schedule):
    gpu = HipIntegrator(E.box_scene())
    if schedule == 2:
        gpu.set_schedule(2, 56, 0, 1)
    else:
        gpu.set_schedule(schedule)
    gpu.set_option("dr_environment", 1)
    assert tuple(gpu.PutDiffTex2D(E.ENV_TEX, 4, 2, 4)) == (0, 32)
    return gpu


def backward(schedule):
    gpu = integrator(schedule)
    params = torch.tensor(E.env_image("4x2").reshape(-1), device="cuda", requires_grad=True)
    img = torch_dr.render(gpu, params, 4)
    assert gpu.last_schedule()[0] == schedule
    (img * torch.tensor(E.adjoint(), device="cuda")).sum().backward()
    torch.cuda.synchronize()
    return [float(v) for v in params.grad.cpu().numpy()]


def adam():
    gpu = integrator(1)
    spp = 16
    truth = torch.tensor(E.env_image("4x2").reshape(-1), device="cuda")
    with torch.no_grad():
        target = torch_dr.render(gpu, truth, spp) / spp
    params = torch.full_like(truth, 0.5).requires_grad_(True)                      # a grey start
    opt = torch.optim.Adam([params], lr=0.05)
    losses = []
    for _ in range(10):
        opt.zero_grad()
        loss = ((torch_dr.render(gpu, params, spp) / spp - target)[..., :3] ** 2).mean()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    print("loss per step:", " ".join(f"{v:.5f}" for v in losses), file=sys.stderr)
    assert np.all(np.isfinite(losses)) and losses[-1] < losses[0], losses


if __name__ == "__main__":
    results = {}
    for s in E.SCHEDULES:
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
