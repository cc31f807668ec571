"""The fixtures of the environment-map DR tests are not vacuous (checked through the oracle's forward PathTraceBlock, no GPU), the oracle alone
stays within the parity bar test_env_grad_gpu.py holds the device to, and the ABI header documents the option."""
import os

import numpy as np
import pytest

import env_grad_cases as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _oracle_frame(sc, spp, integrator=None, depth=None):
    from hydracore3_amd import scene as S
    from oracle.orc import OracleIntegrator
    sc.cam_respoce_rgb, sc.exposure_mult = (1.0, 1.0, 1.0, 1.0), 1.0
    o = OracleIntegrator(sc, sc.params(S.INTEGRATOR_MIS_PT if integrator is None else integrator, 0, depth))
    return o.render(spp), o


def test_every_texel_of_the_small_map_lights_the_plane():
    """(P) at the forward integrator's depth 2 (= PathTraceDR's depth 1), with and without env sampling: the frame under "texel k = 1" is
    brighter than the black map's in some pixel, for each of the 8 texels."""
    for sample in (True, False):
        f0, _ = _oracle_frame(E.with_map(E.plane_scene("4x2", sample), E.basis_image("4x2")), 4, depth=2)
        assert f0[..., :3].max() == 0.0                                  # nothing but the map lights (P)
        for k in range(8):
            fk, _ = _oracle_frame(E.with_map(E.plane_scene("4x2", sample), E.basis_image("4x2", k, 1)), 4, depth=2)
            lit = int(np.count_nonzero(fk[..., 1] > 0.0))
            print(f"sampling {sample}: texel {k} lights {lit} of {E.N} pixels")
            assert lit > 0, f"texel {k} lights no pixel (sampling {sample})"


def test_the_map_matters_on_the_box_scene():
    """(B) with sampling: at least 5 % of the pixels change when the map is zeroed; the texel chosen for the occlusion test changes none,
    however bright it is."""
    base, _ = _oracle_frame(E.box_scene("8x4", True), 4)
    black, _ = _oracle_frame(E.with_map(E.box_scene("8x4", True), E.basis_image("8x4")), 4)
    changed = float(np.mean(np.any(base[..., :3] != black[..., :3], axis=-1)))
    print(f"(B): {changed:.3f} of the pixels change when the map is zeroed")
    assert changed >= 0.05
    for k in E.below_horizon_texels("8x4"):
        img = E.env_image("8x4")
        img[k // 8, k % 8, :3] = 1000.0
        bright, _ = _oracle_frame(E.with_map(E.box_scene("8x4", True), img), 4)
        assert np.array_equal(bright, base), f"texel {k} is seen by some path of the forward integrator"


@pytest.mark.parametrize("mode", ["mis_sampled", "mis_unsampled", "shadow_sampled"])
def test_the_oracle_alone_meets_the_parity_bar(mode):
    """Two oracle runs of (P) from the same generators are one frame: the bar of test_env_grad_gpu.py's forward test (no pixel over it, no
    divergent generator) is met by the reference itself, and under the shadow integrator with sampling the sky adds nothing."""
    from conftest import assert_pixel_parity
    from hydracore3_amd import scene as S
    integ = S.INTEGRATOR_SHADOW_PT if mode == "shadow_sampled" else S.INTEGRATOR_MIS_PT
    a, oa = _oracle_frame(E.plane_scene("4x2", mode != "mis_unsampled"), 1, integ, 2)
    b, ob = _oracle_frame(E.plane_scene("4x2", mode != "mis_unsampled"), 1, integ, 2)
    assert_pixel_parity(a, b, 1, oa, ob, what=f"oracle vs oracle, {mode}: ")
    assert a[..., :3].max() > 0.0


def test_the_header_documents_the_option():
    text = open(os.path.join(ROOT, "include", "hydra_hip.h")).read()
    assert text.count('"dr_environment"') >= 2                           # the option list and hpt_put_diff_tex2d
