"""The sweep's pair cull (csrc/hpt_types.h: sweepPairPlane / sweepPairMayReach, used by csrc/hpt_device.h: traceSweep) on the CPU, and on
the GPU: frames and generator states with the cull on and off."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sweep_pair_cull_is_conservative(tmp_path):
    """Four million rays against random quads (scales 1e-3 ... 1e4, axis-aligned and oblique, bent, paired with the padding record): origins
    moved off the quad by the renderer's offset rule, grazing directions, segments that end just short of the plane. Whenever the cull skips a
    pair, the exact float triangle tests reject both triangles; the wall a ray leaves is culled (tests/cpp/sweep_cull_test.cpp, plain g++,
    -ffp-contract=off as the library)."""
    exe = str(tmp_path / "sweep_cull_test")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", os.path.join(ROOT, "tests", "cpp", "sweep_cull_test.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "all conservative" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("spectral", [False, True])
def test_sweep_cull_keeps_frames_and_generators_bit_identical(spectral):
    """test_035 (the Cornell box: a sweep scene) rendered with sweep_cull 1 and 0: equal frames and generator states, bit
    for bit, in RGB and in spectral mode."""
    import sys
    sys.path.insert(0, ROOT)
    from hydracore3_amd.api import HipIntegrator
    from hydracore3_amd.scene import load_hydra_xml

    sc = load_hydra_xml(os.path.join(ROOT, "tests", "golden", "scenes", "test_035", "statex_00001.xml"), 96, 64, spectral=spectral)
    out = {}
    for mode in (0, 1):
        g = HipIntegrator(sc)
        g.set_option("sweep_cull", mode)
        img = np.zeros((sc.height, sc.width, 4), np.float32)
        g.PathTraceBlock(g.N, 4, img, 8)
        out[mode] = (img, g.random_gens())
    for mode in (1,):
        assert np.array_equal(out[mode][0].view(np.uint32), out[0][0].view(np.uint32)), f"frame differs with sweep_cull {mode}"
        assert np.array_equal(out[mode][1], out[0][1]), f"generator states differ with sweep_cull {mode}"
    assert out[0][0][..., :3].mean() > 0
