"""Spectral QMC without a GPU: the numpy restatement (tests/qmc_spectral_reference.py) pinned to the CPU oracle's spectral PathTraceBlock on a
sky with a spectrum, the wavelength-layer index at hand-computed values, the spectral layouts of hpt_qmc_layout against EnableQMC's table, and
the ABI surface of the new entry."""
import os
import re
import subprocess

import numpy as np
import pytest

import kmlt_reference as K
import qmc_spectral_reference as QS
from hydracore3_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _spectrum(k):
    lam = np.arange(471, dtype=np.float64)
    return (0.75 + 0.5 * np.sin(lam / (23.0 + 9.0 * k) + k) + 0.001 * lam * (k % 3)).astype(np.float32)


def _sky_scene(w, h, response=None):
    sc = synth.furnace_plane(w, h, env=(0.5, 0.25, 2.0))
    sc.cam_pos, sc.cam_look_at, sc.cam_up = (0.0, 5.0, 0.0), (0.0, 10.0, 0.0), (0.0, 0.0, 1.0)
    sc.spectral_mode = 1
    sc.spec_values = np.concatenate([_spectrum(k) for k in range(4)])
    sc.spec_offset_sz = [(471 * k, 471) for k in range(4)]
    sc.env_spec_id, sc.env_spec_mult = 0, 2.5
    sc.exposure_mult = 1.5
    if response is not None:
        sc.cam_response_spectrum_id, sc.cam_response_type = response
    return sc


@pytest.mark.parametrize("response", [None, ((1, 2, 3), 0), ((1, -1, 3), 1)], ids=["cie", "response-xyz", "response-rgb"])
def test_the_restatement_equals_the_oracle_on_a_sky_with_a_spectrum(response):
    """One sample per pixel of a 16 x 16 window that sees only the environment: the pixel's generator draws the lens float4, then the
    wavelength float (GetRandomNumbersSpec of the base class); the path leaves the scene with throughput 1, so accumColor is the
    environment's spectrum at the four wavelengths and the pixel is exposure * SpectralCamRespoceToRGB of it. Every operation of that chain is
    a float32 add, multiply, divide, floor or conversion - no libm call - so the comparison is bit for bit."""
    from oracle.orc import OracleIntegrator
    w = h = 16
    sc = _sky_scene(w, h, response)
    cpu = OracleIntegrator(sc)
    xy = np.asarray(cpu.packed_xy(), np.uint32).reshape(-1)
    gens = K.Gens.from_states(np.asarray(cpu.random_gens(), np.uint32).reshape(-1, 2))
    img = cpu.render(1)
    gens.float4()                                                         # GetRandomNumbersLens
    u = gens.float1()                                                     # GetRandomNumbersSpec: the pseudo wave sample
    waves = QS.sample_wavelengths(u)
    want = QS.contribution(QS.spectral_cam_response_to_rgb(QS.env_spectrum(sc, waves), waves, sc), sc.exposure_mult, 4)
    pixel = ((xy >> np.uint32(16)) * np.uint32(w) + (xy & np.uint32(0xFFFF))).astype(np.int64)
    got = np.asarray(img, np.float32).reshape(w * h, 4)[pixel]
    assert len(np.unique(got[:, :3], axis=0)) > 100
    diff = np.flatnonzero(np.any(got[:, :3].view(np.uint32) != want[:, :3].view(np.uint32), axis=1))
    assert diff.size == 0, (diff[:8], got[diff[:4]], want[diff[:4]])
    assert np.array_equal(np.asarray(cpu.random_gens(), np.uint32).reshape(-1, 2), gens.states())


def test_layer_index_at_hand_computed_wavelengths():
    """t = (lambda - 360) / 470, layer = min(int(channels * t), channels - 1). By hand:
    5 layers - the edge between layers 0 and 1 is 360 + 94 = 454 nm: t = 0.2f, 5 * 0.2f = 1.0000000149 rounds to 1.0f -> 1; 453 nm: 93 / 470 * 5 =
    0.989 -> 0; 455 nm: 1.011 -> 1.  8 layers - the edge is 418.75 nm: 58.75 / 470 = 0.125 exactly -> 1; 418.5 nm: 0.9957 -> 0; 419 nm: 1.0043 -> 1.
    31 layers - the edge between 9 and 10 is 511.6129... nm, not a float: 511.5 nm: 151.5 / 470 * 31 = 9.9926 -> 9; 511.625 nm: 10.0008 -> 10;
    511.75 nm: 10.009 -> 10; 595 nm: t = 0.5, 15.5 -> 15.  LAMBDA_MIN -> 0; LAMBDA_MAX: t = 1, channels * 1 = channels, clamped to channels - 1."""
    cases = {5: [(360.0, 0), (830.0, 4), (454.0, 1), (453.0, 0), (455.0, 1)],
             8: [(360.0, 0), (830.0, 7), (418.75, 1), (418.5, 0), (419.0, 1)],
             31: [(360.0, 0), (830.0, 30), (511.5, 9), (511.625, 10), (511.75, 10), (595.0, 15)]}
    for channels, rows in cases.items():
        lam = np.asarray([r[0] for r in rows], np.float32)
        assert QS.layer_index(lam, channels).tolist() == [r[1] for r in rows], channels


def test_sample_wavelengths_by_hand():
    """u = 0.5: 360 + 0.5 * 470 = 595, then + 117.5 each, wrapped past 830: 712.5, 830 (not above 830: kept), 947.5 -> 360 + 117.5 = 477.5.
    u = 1 (the sampler reaches it): 830, 947.5 -> 477.5, 595, 712.5. u = 0.25: 477.5, 595, 712.5, 830."""
    got = QS.sample_wavelengths(np.asarray([0.5, 1.0, 0.25], np.float32))
    assert got.tolist() == [[595.0, 712.5, 830.0, 477.5], [830.0, 477.5, 595.0, 712.5], [477.5, 595.0, 712.5, 830.0]]


def test_spectral_layouts_equal_enable_qmc():
    """IntegratorQMC::EnableQMC (integrator_qmc.cpp:28-83), the four branches with m_spectral_mode on, written out by hand:
    (dof, motion) -> (m_qmcDofDim, m_qmcSpdDim, m_qmcMotionDim, m_qmcMatDim, m_qmcLgtDim)."""
    from hydracore3_amd import api
    table = {
        (True, True): (2, 4, 5, 0, 0),       # (0,1) pixel; (2,3) lens; (4,5) spd and motion; materials and lights stay pseudo
        (True, False): (2, 4, 0, 5, 7),      # (0,1) pixel; (2,3) lens; (4) spd; (5,6) mat; (7,8,9) light
        (False, True): (2, 3, 2, 4, 6),      # (0,1) pixel; (2,3) motion and spd; (4,5) mat; (6,7,8) light
        (False, False): (2, 4, 0, 2, 5),     # (0,1) pixel; (2,3) mat; (4) spd; (5,6,7) light
    }
    for (dof, motion), want in table.items():
        lay = api.qmc_layout(dof, True, motion)
        assert (lay["dof"], lay["spd"], lay["motion"], lay["mat"], lay["lgt"]) == want, (dof, motion, lay)
        assert lay["spd"] != 0                                             # every spectral layout takes the wave sample from the sequence
    assert [k for k, v in table.items() if v[1] != 4] == [(False, True)]


def test_the_new_symbol_is_declared_bound_and_exported():
    from hydracore3_amd import api
    name = "hpt_path_trace_qmc_block_dev2"
    hdr = open(os.path.join(ROOT, "include", "hydra_hip.h")).read()
    assert re.search(r"\b" + name + r"\s*\(", hdr) and name in api.ABI
    lib = api.load_library()
    assert hasattr(lib, name)
    nm = subprocess.run(["nm", "-D", "--defined-only", api.LIB_PATH], capture_output=True, text=True).stdout
    assert name in set(re.findall(r" T (hpt_[a-z0-9_]+)", nm))
    assert lib.hpt_path_trace_qmc_block_dev2(None, 16, 4, None, 1, None, None, None, None) == 1      # HPT_ERR_ARG: a null context
    assert "qmc_spectral" in hdr
    assert any(u[0].startswith("qmc_spectral") for u in __import__("__graft_entry__").UNITS)
