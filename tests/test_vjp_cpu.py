"""PathTraceVJP without a GPU: the ABI rows and the header, the torch module's argument checks, and the oracle-only check of the bound that
test_vjp_gpu.test_four_samples_against_the_oracle_by_linearity holds the device to."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import dr_texture_cases as T
import vjp_cases as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_and_abi_binds_the_two_symbols():
    from hydracore3_amd import api
    header = open(os.path.join(ROOT, "include", "hydra_hip.h")).read()
    for name, nargs in (("hpt_path_trace_vjp", 10), ("hpt_path_trace_vjp_dev", 11)):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", header)
        assert m, f"{name} is not declared in include/hydra_hip.h"
        assert len(m.group(1).split(",")) == nargs
        assert len(api.ABI[name][1]) == nargs
    lib = api.load_library()
    assert lib.hpt_path_trace_vjp.argtypes == api.ABI["hpt_path_trace_vjp"][1]
    assert lib.hpt_path_trace_vjp_dev.argtypes == api.ABI["hpt_path_trace_vjp_dev"][1]
    assert hasattr(api.HipIntegrator, "PathTraceVJP") and hasattr(api.HipIntegrator, "PathTraceVJP_dev")
    assert lib.hpt_path_trace_vjp(None, 0, 1, 4, None, 1, None, None, None, 0) == 1          # HPT_ERR_ARG: no context (host code, no device touched)


TORCH_CHILD = """
import sys, types
sys.path.insert(0, sys.argv[1])
import numpy as np, torch
from hydracore3_amd import torch_dr
assert not torch.cuda.is_initialized()
integ = types.SimpleNamespace(device=0, grad_size=60, H=17, W=33, N=561)          # render must refuse before it touches the integrator
for bad in (torch.zeros(60, dtype=torch.float32), np.zeros(60, np.float32)):
    try:
        torch_dr.render(integ, bad, 4)
    except ValueError as e:
        assert "cuda:0" in str(e) or "Tensor" in str(e), e
    else:
        raise AssertionError("render accepted a host array")
assert not torch.cuda.is_initialized()
print("ok")
"""


def test_torch_module_imports_without_a_gpu_and_checks_its_arguments():
    """In a child process: torch loads a HIP runtime of its own, which must not come into this session (see
    test_cpu.test_no_gpu_means_loud_failure_not_fallback)."""
    r = subprocess.run([sys.executable, "-c", TORCH_CHILD, ROOT], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.split()[-1] == "ok", r.stderr[-2000:]


@pytest.mark.parametrize("name", ["npot", "single"])
def test_the_linearity_bound_is_met_by_the_oracle_alone(name):
    """G(R1) - G(R1 + D) is the VJP of A = 2 D for any R1 (vjp_cases.py), so the oracle gives it twice: from (R1, R1 + D) and from
    (R1 + sh, R1 + D + sh). The two must agree within the bound the GPU test uses - far within it: what separates them is the float32
    rounding of 2 (C - R) dC at two different R, which is what the bound's terms are sized for."""
    case = T.BY_NAME[name]
    g1, g2 = V.oracle_gradient(case, "r1"), V.oracle_gradient(case, "r2")
    v = g1 - g2
    v_shifted = V.oracle_gradient(case, "r1s") - V.oracle_gradient(case, "r2s")
    bound = V.linearity_bound(g1, g2)
    err = np.abs(v - v_shifted)
    print(f"{name}: worst |V - V_shifted| / bound = {(err / bound).max():.2e}, / max|V| = {err.max() / np.abs(v).max():.2e}; "
          f"max|V| = {np.abs(v).max():.4g}, max|G(R1)| = {np.abs(g1).max():.4g}")
    assert np.count_nonzero(v) > 0
    assert np.all(err <= bound)
    assert np.all(v[T.alpha_elements(case)] == 0)
