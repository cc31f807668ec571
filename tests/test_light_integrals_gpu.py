"""Every light type on the device against a float64 irradiance integral (tests/light_integrals_reference.py), through
PathTraceFromInputRaysBlock: the caller's rays all start at one surface point per "pixel", so the estimator's only randomness is the light
sample, and for point and directional lights there is none. Figures and the mutation table: profiles/light_integrals.md.

Per case, point and channel: exactly 0.0 where the integral is 0; |value - I| <= DELTA_BOUND * I for the delta lights (four times the
oracle's own worst error); |mean - I| <= 5 sigma / sqrt(N) for the sampled ones, sigma from the float64 quadrature. Then the device against
the oracle on the same rays and generators, at the bar of test_gpu_parity.py::test_path_trace_from_input_rays_block_matches_oracle.

Out of the integral's reach (asserted device == oracle only, figures in the profile note): the sampled environment map under MIS, whose
two pdfs are evaluated half a texel apart (clight.h:199)."""
import numpy as np
import pytest

import light_integrals_reference as LR
from hydracore3_amd import scene as S

pytestmark = pytest.mark.gpu

PARITY_PASSES = 16               # passes of the device == oracle comparison (the oracle is the slow side)


def _device(case, pass_num=None, schedule=0):
    from hydracore3_amd.api import HipIntegrator
    sc = case.scene()
    gpu = HipIntegrator(sc, case.params(sc))
    if schedule:
        gpu.set_schedule(schedule)
    pos, dr = case.rays()
    out = np.zeros((pos.shape[0], 4), np.float32)
    gpu.PathTraceFromInputRaysBlock(pos.shape[0], 4, pos, dr, out, case.pass_num if pass_num is None else pass_num)
    return gpu, out


@pytest.mark.parametrize("name", list(LR.CASES))
def test_device_matches_the_integral(name):
    case = LR.CASES[name]
    gpu, out = _device(case)
    assert gpu.last_launch()["schedule"] == 1                        # input rays: the persistent megakernel serves them, whatever is asked
    LR.check_against_integral(case, out, "device")


@pytest.mark.parametrize("name", list(LR.CASES))
def test_device_matches_the_oracle_on_the_same_rays(name):
    from oracle.orc import OracleIntegrator
    case = LR.CASES[name]
    passes = min(case.pass_num, PARITY_PASSES)
    gpu, og = _device(case, passes)
    sc = case.scene()
    cpu = OracleIntegrator(sc, case.params(sc))
    pos, dr = case.rays()
    oc = np.zeros_like(og)
    cpu.path_trace_from_input_rays_block(pos, dr, oc, passes, 4)
    dlt = (og[:, :3].astype(np.float64) - oc[:, :3]) / passes
    assert float(np.sqrt(np.mean(np.sum(dlt * dlt, -1)))) < 1e-3
    assert np.array_equal((og == 0), (oc == 0))                       # the same samples are dark
    assert np.array_equal(gpu.random_gens(), cpu.random_gens())


def test_every_forced_schedule_serves_input_rays_with_the_megakernel():
    """Only the megakernel takes input rays (the wavefront, block-local and streaming schedules fall back to it): forcing each gives the
    automatic run's bits, so case 1 under the automatic schedule is case 1 under every schedule that serves input rays."""
    case = LR.CASES["rect"]
    _, ref = _device(case, 8)
    for schedule in (1, 2, 3, 4):
        gpu, out = _device(case, 8, schedule)
        assert gpu.last_launch()["schedule"] == 1, schedule
        assert np.array_equal(out, ref), schedule


def test_env_map_under_mis_device_equals_oracle():
    """The sampled environment map under INTEGRATOR_MIS_PT: evalMap2DPdf and envLightSampleRev read the table half a texel apart, so the two
    MIS weights need not sum to one and no integral is asserted; device == oracle is, and both are printed against the integral."""
    from oracle.orc import OracleIntegrator
    env = LR.CASES["env"]
    case = LR.Case("env_mis", [], env.points, 64, 64, integrator=S.INTEGRATOR_MIS_PT, env=env.env)
    gpu, og = _device(case)
    sc = case.scene()
    cpu = OracleIntegrator(sc, case.params(sc))
    pos, dr = case.rays()
    oc = np.zeros_like(og)
    cpu.path_trace_from_input_rays_block(pos, dr, oc, case.pass_num, 4)
    I, _ = case.moments()
    print("env under MIS, mean / I: device", (case.point_means(og)[:, :3] / I).mean(0), "oracle", (case.point_means(oc)[:, :3] / I).mean(0))
    dlt = (og[:, :3].astype(np.float64) - oc[:, :3]) / case.pass_num
    assert float(np.sqrt(np.mean(np.sum(dlt * dlt, -1)))) < 1e-3
    assert np.array_equal(gpu.random_gens(), cpu.random_gens())
