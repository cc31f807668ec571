"""The sweep's per-lane pair pass (csrc/hpt_types.h: sweepPairBox / sweepBoxMayHit, used by csrc/hpt_device.h: traceSweep) on the CPU,
and on the GPU: frames, generator states, DR results and ray-query hits with the per-lane pass on and off."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENE = os.path.join(ROOT, "tests", "golden", "scenes", "test_035", "statex_00001.xml")


def test_sweep_pair_box_is_conservative(tmp_path):
    """Millions of ray intervals against random quads (scales 1e-3 ... 1e4, axis-aligned, oblique, thin, far from the origin, lone triangles
    beside the padding record): rays through edges and corners, grazing, leaving the quad from the renderer's offset, axis-parallel, intervals
    that end or start on the exact test's own t. Whenever the pair box rejects the interval, the exact float triangle tests reject both
    triangles (tests/cpp/sweep_lane_box_test.cpp, plain g++, -ffp-contract=off as the library)."""
    exe = str(tmp_path / "sweep_lane_box_test")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", os.path.join(ROOT, "tests", "cpp", "sweep_lane_box_test.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "all conservative" in r.stdout, r.stdout + r.stderr


def _integrator(spectral=False, width=96, height=64):
    sys.path.insert(0, ROOT)
    from hydracore3_amd.api import HipIntegrator
    from hydracore3_amd.scene import load_hydra_xml
    sc = load_hydra_xml(SCENE, width, height, spectral=spectral)
    return sc, HipIntegrator(sc)


@pytest.mark.gpu
@pytest.mark.parametrize("spectral", [False, True])
def test_sweep_lanes_keep_frames_and_generators_bit_identical(spectral):
    """test_035 (a sweep scene) rendered with sweep_lanes 1 and 0: equal frames and generator states, bit for bit, in RGB and in spectral
    mode, with the pair cull on and off."""
    out = {}
    for cull in (1, 0):
        for lanes in (0, 1):
            sc, g = _integrator(spectral)
            assert g.accel_info()["layout"] == "sweep"
            g.set_option("sweep_cull", cull)
            g.set_option("sweep_lanes", lanes)
            img = np.zeros((sc.height, sc.width, 4), np.float32)
            g.PathTraceBlock(g.N, 4, img, 8)
            out[cull, lanes] = (img, g.random_gens())
    for key in out:
        assert np.array_equal(out[key][0].view(np.uint32), out[1, 0][0].view(np.uint32)), f"frame differs with sweep_cull, sweep_lanes = {key}"
        assert np.array_equal(out[key][1], out[1, 0][1]), f"generator states differ with sweep_cull, sweep_lanes = {key}"
    assert out[1, 0][0][..., :3].mean() > 0


@pytest.mark.gpu
def test_sweep_lanes_keep_dr_results():
    """PathTraceDR on test_035 with sweep_lanes 1 and 0: the same frame and generators bit for bit; the same loss and gradient up to the order
    of the gradient's float atomics."""
    out = {}
    for lanes in (0, 1):
        sc, g = _integrator(False, 32, 32)
        g.set_option("sweep_lanes", lanes)
        off, size = g.PutDiffTex2D(1, 256, 256, 4)
        rng = np.random.default_rng(5)
        data = rng.uniform(0.2, 0.9, size).astype(np.float32)
        ref = rng.uniform(0.0, 0.5, (sc.height, sc.width, 4)).astype(np.float32)
        img = np.zeros((sc.height, sc.width, 4), np.float32)
        grad = np.zeros_like(data)
        loss = g.PathTraceDR(g.N, 4, img, 4, ref, data, grad)
        out[lanes] = (img, g.random_gens(), loss, grad)
    assert np.array_equal(out[1][0].view(np.uint32), out[0][0].view(np.uint32))
    assert np.array_equal(out[1][1], out[0][1])
    assert out[1][2] == pytest.approx(out[0][2], rel=1e-6)
    assert np.count_nonzero(out[0][3]) > 100
    assert np.allclose(out[1][3], out[0][3], rtol=1e-5, atol=1e-7 * np.abs(out[0][3]).max())


def _rays(n, seed):
    """Random rays in and around the box, and rays aimed at the quads' edges and corners (the vertices of test_035, nudged by a few ulp)."""
    rng = np.random.default_rng(seed)
    pos = np.zeros((n, 4), np.float32)
    dr = np.zeros((n, 4), np.float32)
    pos[:, :3] = rng.uniform(-6.0, 6.0, (n, 3))
    d = rng.normal(size=(n, 3))
    half = n // 2
    # the second half aims at points on the box's edges and corners: lattice points of the scene's coordinates, nudged
    tgt = rng.choice(np.array([-4.0, -2.0, -1.0, -0.5, 0.0, 0.5, 1.0, 2.0, 4.0], np.float32), (n - half, 3))
    tgt += rng.choice([0.0, 1e-6, -1e-6, 1e-4], (n - half, 3))
    d[half:] = tgt - pos[half:, :3]
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    dr[:, :3] = d
    dr[:, 3] = np.float32(3.402823466e+38)
    return pos, dr


@pytest.mark.gpu
def test_sweep_lanes_keep_ray_query_hits():
    """RayQuery_NearestHit / AnyHit on test_035 with sweep_lanes 1 and 0: equal hits (t, u, v, prim, inst) and occlusion flags for random and
    edge-aimed rays, with open and finite tfar, tnear 0 and tnear > 0, and tnear < 0."""
    _, g = _integrator()
    pos, dr = _rays(40000, 17)
    variants = [(pos, dr)]
    dr2 = dr.copy(); dr2[:, 3] = np.random.default_rng(4).uniform(0.5, 12.0, len(dr)).astype(np.float32)
    variants.append((pos, dr2))
    pos2 = pos.copy(); pos2[:, 3] = np.random.default_rng(6).uniform(0.0, 3.0, len(pos)).astype(np.float32)
    variants.append((pos2, dr2))
    pos3 = pos.copy(); pos3[:, 3] = -1.0
    variants.append((pos3, dr))
    res = {}
    for lanes in (0, 1):
        g.set_option("sweep_lanes", lanes)
        res[lanes] = [(g.RayQuery_NearestHit(p, d), g.RayQuery_AnyHit(p, d)) for p, d in variants]
    hits = 0
    for (h0, a0), (h1, a1) in zip(res[0], res[1]):
        assert np.array_equal(h0.view(np.uint8), h1.view(np.uint8))
        assert np.array_equal(a0, a1)
        hits += int(a0.sum())
    assert hits > 1000


@pytest.mark.gpu
def test_sweep_lanes_take_the_per_lane_pass():
    """The per-lane pass runs at all: in the instrumented kernels, sweep_lanes 1 tests fewer triangles per ray than sweep_lanes 0 (each lane
    only its candidate pairs), and its triangle trips keep fewer than all 64 lanes busy (the wave-uniform loop keeps every lane busy)."""
    c = {}
    for lanes in (0, 1):
        sc, g = _integrator()
        g.set_option("sweep_lanes", lanes)
        g.set_instrumentation(True)
        img = np.zeros((sc.height, sc.width, 4), np.float32)
        g.PathTraceBlock(g.N, 4, img, 4)
        c[lanes] = g.counters()
    per_ray = {k: c[k]["tris"] / c[k]["rays"] for k in c}
    assert per_ray[1] < 0.8 * per_ray[0], per_ray
    assert c[1]["tris"] < 64 * c[1]["wave_tri_iters"] * 0.9
