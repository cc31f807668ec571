"""Light-colour gradients without a GPU: the entry point is declared, exported and bound, torch_dr imports, and the fixture scenes of
test_light_grad_gpu.py are not vacuous (checked through the oracle's PathTraceBlock)."""
import copy
import ctypes
import os
import re

import numpy as np
import pytest

import light_grad_cases as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_point_is_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "hydra_hip.h")).read()
    assert re.search(r"int\s+hpt_put_diff_lights\(hpt_ctx\* ctx, uint32_t firstLight, uint32_t count, uint64_t\* outOffset, uint64_t\* outSize\);", header)
    lib = ctypes.CDLL(os.path.join(ROOT, "hydracore3_amd", "libhydra_hip.so"))
    assert hasattr(lib, "hpt_put_diff_lights")
    off, size = ctypes.c_uint64(1), ctypes.c_uint64(2)
    assert lib.hpt_put_diff_lights(None, 0, 1, ctypes.byref(off), ctypes.byref(size)) == 1      # HPT_ERR_ARG without a context, nothing written
    assert (off.value, size.value) == (1, 2)


def test_api_binds_it():
    from hydracore3_amd import api
    assert "hpt_put_diff_lights" in api.ABI
    L = api.load_library()                                                           # raises if the library lacks a declared symbol
    assert len(L.hpt_put_diff_lights.argtypes) == 5
    assert "offset" in api.HipIntegrator.PutDiffLights.__doc__


def test_torch_dr_imports_without_a_gpu():
    torch = pytest.importorskip("torch")
    from hydracore3_amd import torch_dr
    assert "PutDiffLights" in torch_dr.render.__doc__
    with pytest.raises(ValueError):
        torch_dr.render(None, np.zeros(4, np.float32), 1)
    del torch


@pytest.mark.parametrize("scene", [G.scene_a, G.scene_b], ids=["A", "B"])
def test_fixture_is_not_vacuous(scene):
    """Every light lights more than 5 % of the pixels of its single-light frame and every area light's mesh shows; scene B's F_0 is not black."""
    from oracle.orc import OracleIntegrator
    sc, spp, frames = scene(), 4, {}
    for l in [None] + list(range(len(sc.lights))):
        one = copy.copy(sc)
        one.lights = list(G.only_light(sc, l))
        frames[l] = OracleIntegrator(one).render(spp)
    assert len(sc.lights) == 6
    assert (frames[None][..., :3].max() > 0.0) == (scene is G.scene_b)
    for l in range(len(sc.lights)):
        assert G.lit_fraction(frames[l], frames[None]) > 0.05, (l, G.lit_fraction(frames[l], frames[None]))
    for l in G.AREA_LIGHTS:
        assert G.emitter_pixels(frames[l], sc.lights[l], spp) > 0, l
