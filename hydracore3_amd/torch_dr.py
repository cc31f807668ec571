"""The path tracer as a differentiable PyTorch op: `render(integrator, params, spp)` returns the frame summed over `spp` samples per pixel and
back-propagates any loss on it to the registered parameter textures through hpt_path_trace_vjp_dev (PathTraceVJP, include/hydra_hip.h).

api.py stays free of torch; this module sits on top of it. Importing it needs torch but no GPU. torch brings a HIP runtime of its own: let it
come up first (torch.cuda.init() or any CUDA tensor) before the first HipIntegrator is created, as bench.py does. Forward and backward trace the same paths:
forward saves m_randomGens (a host copy of 8 bytes per pixel), backward puts them back before the VJP call, which advances them as forward
did - so after backward the generators are where forward left them, and the next render draws new samples.
"""
from __future__ import annotations

import torch


def _check(integrator, params):
    if not isinstance(params, torch.Tensor):
        raise ValueError("render: params must be a torch.Tensor")
    if not params.is_cuda or params.device.index != integrator.device:
        raise ValueError(f"render: params must live on cuda:{integrator.device}, the integrator's device (got {params.device})")
    if params.dtype != torch.float32 or not params.is_contiguous():
        raise ValueError("render: params must be a contiguous float32 tensor")
    if params.numel() < integrator.grad_size or params.numel() == 0:
        raise ValueError(f"render: params holds {params.numel()} floats, the registered differentiable textures need {integrator.grad_size}")


def _stream(device, wait=False):
    """The caller's stream on `device`. wait: hpt_get_random_gens / hpt_set_random_gens copy on the null stream, which a stream of torch's does
    not order itself against - what is queued on it comes first."""
    s = torch.cuda.current_stream(device)
    if wait:
        s.synchronize()
    return s.cuda_stream


class _Render(torch.autograd.Function):
    @staticmethod
    def forward(ctx, params, integrator, spp):
        stream = _stream(params.device, wait=True)
        gens = integrator.random_gens()
        frame = torch.zeros((integrator.H, integrator.W, 4), dtype=torch.float32, device=params.device)
        integrator._chk(integrator.L.hpt_path_trace_vjp_dev(integrator.h, 0, integrator.N, 4, frame.data_ptr(), spp, None, params.data_ptr(),
                                                            None, params.numel(), stream))
        ctx.integrator, ctx.spp, ctx.gens = integrator, spp, gens
        ctx.save_for_backward(params)
        return frame

    @staticmethod
    def backward(ctx, grad_output):
        params, = ctx.saved_tensors
        integrator = ctx.integrator
        adj = grad_output.to(torch.float32).contiguous()
        scratch = torch.zeros_like(adj)
        grad = torch.zeros_like(params)
        stream = _stream(params.device, wait=True)
        integrator.set_random_gens(ctx.gens)
        integrator._chk(integrator.L.hpt_path_trace_vjp_dev(integrator.h, 0, integrator.N, 4, scratch.data_ptr(), ctx.spp, adj.data_ptr(),
                                                            params.data_ptr(), grad.data_ptr(), params.numel(), stream))
        return grad, None, None


def render(integrator, params, spp):
    """The frame of `integrator` (a HipIntegrator with its differentiable textures registered by PutDiffTex2D) with the parameters `params`:
    a [H, W, 4] float32 tensor on the GPU, the SUM over `spp` samples per pixel (divide by spp for the mean), differentiable with respect to
    `params`. params: a contiguous float32 tensor on the integrator's device with at least the registered number of elements; anything else
    raises ValueError before any device work. Each call draws new samples (m_randomGens goes on); backward replays forward's.
    Light colours need no argument of their own: the RGB gains of the lights registered by PutDiffLights are elements of `params` (at the
    offset PutDiffLights returned, four floats per light, the fourth unused), and `params.grad` receives their gradient there.
    Nor does an environment map: with set_option("dr_environment", 1) a map registered by PutDiffTex2D is a slice of `params` like any texture."""
    _check(integrator, params)
    spp = int(spp)
    if spp < 1:
        raise ValueError("render: spp must be at least 1")
    return _Render.apply(params, integrator, spp)
