"""The checks of hydracore3_amd.torch_dr, run as a process of its own by test_vjp_gpu.py (torch's HIP runtime must come up first, and must not
be loaded into the pytest session). Prints one JSON line: {check: "ok" or what failed}."""
import json
import os
import sys
import traceback

import numpy as np
import torch

torch.cuda.init()                                       # before libhydra_hip.so brings its runtime up, as bench.py does

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

import dr_texture_cases as T                            # noqa: E402
import vjp_cases as V                                   # noqa: E402
from hydracore3_amd import torch_dr                     # noqa: E402
from hydracore3_amd.api import HipIntegrator            # noqa: E402

SPP = V.SPP
CASE = T.BY_NAME["npot"]


def integrator(schedule):
    gpu = HipIntegrator(T.scene_of(CASE))
    if schedule == 2:
        gpu.set_schedule(2, 56, 0, 1)
    else:
        gpu.set_schedule(schedule)
    T.register_gpu(gpu, CASE)
    return gpu


def render_and_backward(schedule):
    n = CASE.size()
    gpu = integrator(schedule)
    data, _ = T.inputs(CASE, gpu.scene)
    start = gpu.random_gens()
    params = torch.tensor(data, device="cuda", requires_grad=True)
    weights = V.adjoint_of(*V.grid_frames(gpu.scene)[:2])                              # any fixed image
    img = torch_dr.render(gpu, params, SPP)
    assert img.shape == (gpu.H, gpu.W, 4) and img.dtype == torch.float32 and img.is_cuda
    assert gpu.last_schedule()[0] == schedule
    after_forward = gpu.random_gens()
    # the null-adjoint frame of the binding, from the same start
    gpu.set_random_gens(start)
    frame0 = np.zeros((gpu.H, gpu.W, 4), np.float32)
    gpu.PathTraceVJP(gpu.N, 4, frame0, SPP, None, data)
    assert np.array_equal(img.detach().cpu().numpy().view(np.uint32), frame0.view(np.uint32))
    assert np.array_equal(gpu.random_gens(), after_forward)
    (img * torch.tensor(weights, device="cuda")).sum().backward()
    torch.cuda.synchronize()
    assert np.array_equal(gpu.random_gens(), after_forward)
    # the same VJP through the binding, from the same start
    gpu.set_random_gens(start)
    d_frame, d_adj, d_data, d_grad = (gpu.dev_array(a) for a in (np.zeros_like(frame0), weights, data, np.zeros(data.size, np.float32)))
    gpu.PathTraceVJP_dev(d_frame, SPP, d_adj, d_data, d_grad)
    want, got = d_grad.download(), params.grad.cpu().numpy()
    assert np.count_nonzero(want[:n]) > 0 and np.all(got[n:] == 0)
    assert np.allclose(got, want, rtol=1e-4, atol=1e-7 * np.abs(want).max())           # the floor of test_vjp_gpu._same_sums
    for bad in (params.detach()[: n - 1], params.detach().double(), params.detach().cpu(), params.detach().repeat(2)[::2]):
        try:
            torch_dr.render(gpu, bad, SPP)
        except ValueError:
            continue
        raise AssertionError(f"render accepted {tuple(bad.shape)} {bad.dtype} on {bad.device}, contiguous: {bad.is_contiguous()}")


def adam():
    n, spp = CASE.size(), 16
    gpu = integrator(1)
    data, _ = T.inputs(CASE, gpu.scene)
    truth = torch.tensor(data, device="cuda")
    with torch.no_grad():
        target = torch_dr.render(gpu, truth, spp) / spp
    params = torch.full_like(truth, 0.5).requires_grad_(True)
    opt = torch.optim.Adam([params], lr=0.05)
    losses = []
    for _ in range(10):
        opt.zero_grad()
        loss = (torch_dr.render(gpu, params, spp) / spp - target)[..., :3].abs().mean()
        loss.backward()
        opt.step()
        with torch.no_grad():
            params[:n].clamp_(0.0, 1.0)
        losses.append(float(loss.detach()))
    print("L1 loss per step:", " ".join(f"{v:.5f}" for v in losses), file=sys.stderr)
    assert np.all(np.isfinite(losses)) and losses[-1] < losses[0], losses


if __name__ == "__main__":
    results = {}
    for name, fn in [(f"render_and_backward[{s}]", lambda s=s: render_and_backward(s)) for s in T.SCHEDULES] + [("adam", adam)]:
        try:
            fn()
            results[name] = "ok"
        except Exception:
            results[name] = traceback.format_exc()
    print(json.dumps(results))
