"""Spectral MLT without a GPU: the vector builder of tests/kmlt_spectral_reference.py pinned to the CPU oracle's spectral PathTraceBlock on a sky
with a spectrum (the wavelengths derived from slot 4 are the ones the oracle's pass uses), the ABI surface of the new entry, the option and the
new translation units."""
import os
import re
import subprocess

import numpy as np
import pytest

import kmlt_reference as K
import kmlt_spectral_reference as KS
import qmc_spectral_reference as QS
from test_qmc_spectral_cpu import _sky_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("response", [None, ((1, 2, 3), 0), ((1, -1, 3), 1)], ids=["cie", "response-xyz", "response-rgb"])
def test_slot_4_holds_the_wavelength_sample_of_the_oracle_s_spectral_pass(response):
    """One pass of the oracle over a 16 x 16 window that sees only the environment. The builder puts the float the base class draws after the
    lens float4 into slot 4; SampleWavelengths of that slot gives the path's wavelengths; the pixel the oracle writes is exposure *
    SpectralCamRespoceToRGB(environment spectrum at those wavelengths) bit for bit (no libm call on the way), so the wavelengths are the ones
    the oracle's pass used: another float of the stream gives other wavelengths and, on this spectrum, another colour."""
    from oracle.orc import OracleIntegrator
    w = h = 16
    sc = _sky_scene(w, h, response)
    cpu = OracleIntegrator(sc)
    xy = np.asarray(cpu.packed_xy(), np.uint32).reshape(-1)
    before = np.asarray(cpu.random_gens(), np.uint32).reshape(-1, 2).copy()
    x, u = KS.base_vectors(before, xy, cpu.params, motion=False)
    assert x.shape == (w * h, K.state_size(cpu.params.traceDepth)) and np.array_equal(x[:, KS.WAVE_SLOT], u)
    g = K.Gens.from_states(before)
    lens = g.float4()
    assert np.array_equal(u, g.float1())                                  # the draw after the lens float4, nothing in between without motion
    assert np.array_equal(x[:, 2:4], lens[:, 2:4]) and np.all(x[:, KS.TIME_SLOT] == 0.0)
    waves = QS.sample_wavelengths(x[:, KS.WAVE_SLOT])
    assert np.array_equal(waves, QS.sample_wavelengths(u)) and waves.min() >= QS.LAMBDA_MIN and waves.max() <= QS.LAMBDA_MAX
    img = cpu.render(1)
    want = QS.contribution(QS.spectral_cam_response_to_rgb(QS.env_spectrum(sc, waves), waves, sc), sc.exposure_mult, 4)
    pixel = ((xy >> np.uint32(16)) * np.uint32(w) + (xy & np.uint32(0xFFFF))).astype(np.int64)
    got = np.asarray(img, np.float32).reshape(w * h, 4)[pixel]
    assert len(np.unique(got[:, :3], axis=0)) > 100
    diff = np.flatnonzero(np.any(got[:, :3].view(np.uint32) != want[:, :3].view(np.uint32), axis=1))
    assert diff.size == 0, (diff[:8], got[diff[:4]], want[diff[:4]])
    assert np.array_equal(np.asarray(cpu.random_gens(), np.uint32).reshape(-1, 2), g.states())   # the miss draws nothing more
    # the film point of the vector falls into the pixel it was built for
    px = np.minimum((x[:, 0] * np.float32(w)).astype(np.uint32), w - 1)
    py = np.minimum((x[:, 1] * np.float32(h)).astype(np.uint32), h - 1)
    assert np.array_equal(py * np.uint32(w) + px, pixel.astype(np.uint32))


def test_the_time_is_drawn_before_the_wavelength_sample():
    """With moving instances the base class draws the time between the lens float4 and the wavelength float (integrator_pt.cpp:114-118)."""
    gens = K.Gens.init(np.arange(1, 65)).states()
    xy = (np.arange(64, dtype=np.uint32) // 8 << 16) | (np.arange(64, dtype=np.uint32) % 8)

    class P:
        traceDepth, winStartX, winStartY, fbWidth, fbHeight = 2, 0, 0, 8, 8
    x, u = KS.base_vectors(gens, xy, P, motion=True)
    g = K.Gens.from_states(gens)
    g.float4()
    assert np.array_equal(x[:, KS.TIME_SLOT], g.float1()) and np.array_equal(u, g.float1())
    o = K.BOUNCE_START
    assert np.array_equal(x[:, o + 3], g.float1())                        # the light selection float comes before the light float4
    assert np.array_equal(x[:, o:o + 3], g.float4()[:, :3]) and np.array_equal(x[:, o + K.MATS_ID:o + K.MATS_ID + 4], g.float4())
    x0, u0 = KS.base_vectors(gens, xy, P, motion=False)
    assert np.array_equal(u0, x[:, KS.TIME_SLOT]) and np.all(x0[:, KS.TIME_SLOT] == 0.0)


def test_colour_from_raw_is_the_conversion_at_exposure_one():
    sc = _sky_scene(8, 8)
    sc.exposure_mult = 1.0
    waves = QS.sample_wavelengths(np.asarray([0.0, 0.25, 0.6], np.float32))
    raw = QS.env_spectrum(sc, waves)
    plain, term = KS.colour_from_raw(raw, waves, sc), KS.colour_from_raw(raw, waves, sc, True)
    assert plain.shape == (3, 4) and np.all(plain[:, 3] == 0.0) and np.any(plain != term)
    assert np.array_equal(plain[:, :3], QS.spectral_cam_response_to_rgb(raw, waves, sc))
    sc.exposure_mult = 1.5
    with pytest.raises(AssertionError):
        KS.colour_from_raw(raw, waves, sc)


def test_the_statistics_are_summed_in_the_kernel_s_order():
    """kmltStatsKernel: thread t adds elements t, t + 256, ... in order, then the LDS fold. By hand: v[0] = 1e16, v[256] = 0.5, v[1] = -1e16 -
    thread 0 forms 1e16 + 0.5 = 1e16 (an ulp there is 2), thread 1 holds -1e16, the fold gives 0; in index order the sum would be 0.5.
    Fold order: sh[0] + sh[128] first, then + (sh[64] + sh[192]): 1e16, 0.5, -1e16 at 0, 128, 64 give (1e16 + 0.5) + (-1e16) = 0, while
    1e16, -1e16, 0.5 at 0, 128, 64 give (1e16 - 1e16) + 0.5 = 0.5. Then a scalar loop of the same order on 1000 random values, and the four
    statistics on a small case worked out by hand."""
    v = np.zeros(300)
    v[0], v[256], v[1] = 1e16, 0.5, -1e16
    assert KS._block_sum(v) == 0.0 and (v[0] + v[1]) + v[256] == 0.5
    v = np.zeros(256)
    v[0], v[128], v[64] = 1e16, 0.5, -1e16
    assert KS._block_sum(v) == 0.0
    v[128], v[64] = -1e16, 0.5
    assert KS._block_sum(v) == 0.5
    rng = np.random.default_rng(11)
    v = rng.random(1000) * 10.0 ** rng.integers(-8, 8, 1000)
    sh = [0.0] * 256
    for t in range(256):
        for i in range(t, 1000, 256):
            sh[t] += float(v[i])
    o = 128
    while o:
        for t in range(o):
            sh[t] += sh[t + o]
        o >>= 1
    assert KS._block_sum(v) == sh[0]
    # three chains (one without a large step), a frame of two pixels, pixelsNum = 2, passNum = 3
    frame = np.asarray([[0.5, 0.25, 0.25, 0.0], [1.0, 2.0, 3.0, 0.0]], np.float32)
    got = KS.stats_kernel(np.asarray([1.5, 0.0, 0.75]), np.asarray([3, 0, 1]), np.asarray([2, 1, 1]), frame, 2, 3)
    avg = (1.5 / 3.0 + 0.75) / 2.0
    actual = (float(K.contrib_func(frame[0, :3])) + float(K.contrib_func(frame[1, :3]))) / 2.0
    assert got.tolist() == [avg, actual, 4.0 / 6.0, float(np.float32(3.0) * np.float32(avg / actual))]
    assert np.array_equal(got, K.normalisation(np.asarray([1.5, 0.0, 0.75]), np.asarray([3, 0, 1]), np.asarray([2, 1, 1]), frame, 2, 3))
    assert KS.stats_kernel(np.zeros(2), np.zeros(2, np.int64), np.zeros(2), frame, 2, 1)[3] == 1.0
    # the per-chain sums: one double addition per large step, in step order, accepted or not
    col = np.zeros((1, 3, 4), np.float32)
    col[0, :, 0] = [3.0, 6.0, 9.0]
    acc, n = KS.chain_sums(np.asarray([[1, 0, 1]], np.uint8), col)
    y = K.contrib_func(col[0, :, :3]).astype(np.float64)
    assert n.tolist() == [2] and acc.tolist() == [0.0 + y[0] + y[2]]


def test_the_new_symbol_option_and_units_are_declared_bound_and_exported():
    from hydracore3_amd import api
    name = "hpt_path_trace_pss_dev2"
    hdr = open(os.path.join(ROOT, "include", "hydra_hip.h")).read()
    assert re.search(r"\b" + name + r"\s*\(", hdr) and name in api.ABI
    assert '"kmlt_spectral"' in hdr
    lib = api.load_library()
    assert hasattr(lib, name)
    nm = subprocess.run(["nm", "-D", "--defined-only", api.LIB_PATH], capture_output=True, text=True).stdout
    assert name in set(re.findall(r" T (hpt_[a-z0-9_]+)", nm))
    assert lib.hpt_path_trace_pss_dev2(None, None, 1, 16, None, None, None, None, None) == 1       # HPT_ERR_ARG: a null context
    units = __import__("__graft_entry__").UNITS
    kmlt = [u for u in units if u[0].startswith("kmlt_spectral")]
    assert len(kmlt) == 4 and all(u[1] == "hpt_spectral.hip" for u in kmlt)
    assert sorted(u[2][0] for u in kmlt) == sorted(f"-DHPT_SPEC_INST={i}" for i in (9, 10, 11, 12))
    adapter = open(os.path.join(ROOT, "hydracore3_amd", "csrc", "integrator_hip.h")).read()
    assert "EnableSpectralKMLT" in adapter
