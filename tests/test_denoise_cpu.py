"""DenoiseFrame without a GPU: the numpy float32 restatement (tests/denoise_reference.py) against things that do not come from it - a B3
convolution computed in float64, constants, hard id edges, the footprint of an impulse, planted NaN / Inf pixels, the oracle's own converged
frame - and the Python front end against the C header."""
import os
import re

import numpy as np
import pytest

import denoise_reference as D
from conftest import ROOT, scene_path
from hydracore3_amd.api import GBUFFER_DTYPE

# 25 products, 24 additions per sum and one division, each rounded to float32: the bound the issue sets for a 5 x 5 pass
REL_25 = 32 * 2.0 ** -24


def uniform_gbuffer(h, w, albedo=(0.5, 0.5, 0.5), depth=2.0):
    g = np.zeros((h, w), GBUFFER_DTYPE)
    g["norm"] = (0, 0, 1)
    g["depth"], g["coverage"] = depth, 1.0
    g["rgba"] = (*albedo, 1.0)
    return g                                                              # ids 0


def random_gbuffer(h, w, seed, ids=3):
    rng = np.random.default_rng(seed)
    g = np.zeros((h, w), GBUFFER_DTYPE)
    n = rng.normal(size=(h, w, 3))
    g["norm"] = (n / np.linalg.norm(n, axis=-1, keepdims=True)).astype(np.float32)
    g["depth"] = rng.uniform(0.5, 8.0, (h, w)).astype(np.float32)
    g["rgba"][..., :3] = rng.uniform(0.0, 1.0, (h, w, 3)).astype(np.float32)
    g["rgba"][..., 3] = 1.0
    g["instId"] = rng.integers(0, ids, (h, w))
    g["matId"] = rng.integers(0, ids, (h, w))
    g["objId"] = g["instId"]
    return g


def b3_convolution_f64(img, step=1):
    """Border-renormalised 5 x 5 B3 convolution of [H, W, C] in float64, written pixel by pixel."""
    k = np.array([1, 4, 6, 4, 1], np.float64) / 16
    H, W = img.shape[:2]
    out = np.zeros(img.shape, np.float64)
    for y in range(H):
        for x in range(W):
            sw, sc = 0.0, np.zeros(img.shape[2])
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    qy, qx = y + step * dy, x + step * dx
                    if 0 <= qy < H and 0 <= qx < W:
                        sw += k[dy + 2] * k[dx + 2]
                        sc += k[dy + 2] * k[dx + 2] * img[qy, qx].astype(np.float64)
            out[y, x] = sc / sw
    return out


def test_all_stops_off_is_the_b3_convolution():
    rng = np.random.default_rng(1)
    color = rng.uniform(0.1, 1.0, (11, 14, 4)).astype(np.float32)
    got = D.denoise(color, uniform_gbuffer(11, 14), iterations=1, normal_squarings=0, flags=0, sigma_color=0, sigma_depth=0, sigma_albedo=0)
    want = b3_convolution_f64(color[..., :3])
    rel = np.abs(got[..., :3].astype(np.float64) - want) / want
    print("B3 convolution: worst relative error", rel.max(), "bound", REL_25)
    assert rel.max() <= REL_25
    assert np.array_equal(got[..., 3], color[..., 3])                     # alpha: color.a * 1, filtered no further


def test_constant_image_stays_constant_over_a_random_gbuffer():
    color = np.full((13, 17, 4), 0.37, np.float32)
    got = D.denoise(color, random_gbuffer(13, 17, 2), iterations=3, flags=0)
    rel = np.abs(got[..., :3].astype(np.float64) - np.float64(np.float32(0.37))) / 0.37
    print("constant image: worst relative error per pass", rel.max() / 3)
    assert rel.max() <= 3 * REL_25                                        # the bound of one pass, three passes


def test_nothing_leaks_across_an_id_edge():
    g = uniform_gbuffer(12, 20)
    g["instId"][:, 10:] = 1
    color = np.zeros((12, 20, 4), np.float32)
    color[:, :10, :3], color[:, 10:, :3] = 1.25, 5.0
    got = D.denoise(color, g, iterations=4, flags=0)                      # steps 1 .. 8: every pixel has taps on the other side
    for side, v in ((np.s_[:, :10], 1.25), (np.s_[:, 10:], 5.0)):
        rel = np.abs(got[side][..., :3].astype(np.float64) - v) / v
        assert rel.max() <= 4 * REL_25, (v, rel.max())
    g2 = uniform_gbuffer(12, 20)
    g2["matId"][:6] = 3                                                   # the same with a material edge across the rows
    c2 = np.zeros((12, 20, 4), np.float32)
    c2[:6, :, :3], c2[6:, :, :3] = 0.5, 2.0
    got = D.denoise(c2, g2, iterations=4, flags=0)
    assert np.abs(got[:6, :, :3] - 0.5).max() <= 0.5 * 4 * REL_25 and np.abs(got[6:, :, :3] - 2.0).max() <= 2.0 * 4 * REL_25


def test_impulse_after_two_iterations_has_support_of_six_pixels():
    color = np.zeros((21, 23, 4), np.float32)
    color[10, 11, :3] = 1.0
    got = D.denoise(color, uniform_gbuffer(21, 23), iterations=2, flags=0, sigma_color=0, sigma_depth=0, sigma_albedo=0)
    support = np.zeros((21, 23), bool)
    support[10 - 6:10 + 7, 11 - 6:11 + 7] = True                          # 2 * 1 + 2 * 2 = 6 to each side
    for ch in range(3):
        assert np.array_equal(got[..., ch] != 0, support)
    assert np.all(got[..., :3] >= 0)


def test_planted_nan_and_inf_pixels_are_rebuilt_from_their_neighbours():
    color = np.full((9, 12, 4), 0.75, np.float32)
    color[4, 5, 0], color[2, 2, 1], color[7, 10, 2], color[0, 0, :3] = np.nan, np.inf, -np.inf, np.nan
    got = D.denoise(color, uniform_gbuffer(9, 12), iterations=2, flags=0)
    assert np.isfinite(got).all()
    assert np.abs(got[..., :3].astype(np.float64) - 0.75).max() <= 0.75 * 2 * REL_25


def test_isolated_nan_pixel_gives_zero():
    g = uniform_gbuffer(7, 7)
    g["instId"][3, 3] = 42                                                # no tap shares its id, and its own tap is skipped
    color = np.full((7, 7, 4), 0.5, np.float32)
    color[3, 3, :3] = np.nan
    got = D.denoise(color, g, iterations=2, flags=1)
    assert np.array_equal(got[3, 3], np.array([0, 0, 0, 0.5], np.float32))
    assert np.isfinite(got).all()


def ulp_distance(a, b):
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    ia, ib = np.where(ia < 0, -(ia & 0x7FFFFFFF), ia), np.where(ib < 0, -(ib & 0x7FFFFFFF), ib)
    return np.abs(ia - ib)


@pytest.mark.parametrize("albedo", [0.5, 0.25, 2.0 ** -6])
def test_demodulation_with_a_constant_albedo_is_the_identity(albedo):
    """With one albedo a everywhere the albedo stop is 1 and the colour stop sees (c_p - c_q)^2 / a^2 against sigmaColor^2, so the plain run to compare with has
    sigmaColor * a. For a power of two the division, the scaled sigma and the multiplication are exact scalings and the two runs agree to the bit
    (2 ulp, the bound the issue sets, covers it); for another albedo each of the 25 products per pass rounds on its own and no bound of a
    few ulp can be derived, so such values are not in the cases (measured with the colour stop off: albedo 0.7 / 0.3 / 0.9 give 3 ... 5 ulp after
    1 ... 5 iterations; profiles/denoise.md)."""
    rng = np.random.default_rng(5)
    color = rng.uniform(0.05, 2.0, (10, 13, 4)).astype(np.float32)
    g = random_gbuffer(10, 13, 6, ids=1)
    g["rgba"][..., :3] = albedo
    plain = D.denoise(color, g, iterations=3, flags=0, sigma_color=0.6 * albedo)
    demod = D.denoise(color, g, iterations=3, flags=1, sigma_color=0.6)
    worst = int(ulp_distance(plain, demod).max())
    print("demodulate / remodulate: worst distance in ulp", worst)
    assert worst <= 2


_cornell = {}


def cornell_inputs():
    """test_035 at 64 x 64 from the CPU oracle: the 4-spp and the 512-spp frame (sums), and the restated G-buffer. Computed once."""
    if not _cornell:
        import gbuffer_reference as R
        from hydracore3_amd.scene import load_hydra_xml
        from oracle.orc import OracleIntegrator
        sc = load_hydra_xml(scene_path("test_035"), 64, 64)
        _cornell["noisy"] = OracleIntegrator(sc).render(4)
        _cornell["converged"] = OracleIntegrator(sc).render(512)
        cpu = OracleIntegrator(sc)
        _cornell["gbuffer"] = R.eval_gbuffer(sc, cpu)[0]
        _cornell["scene"] = sc
    return _cornell


def test_filtered_4spp_frame_is_closer_to_the_converged_frame():
    """The quality condition: strictly lower mean squared error against the oracle's 512-spp frame than the unfiltered 4-spp frame has."""
    from hydracore3_amd.api import DENOISE_DEFAULTS as d
    c = cornell_inputs()
    ref = c["converged"][..., :3].astype(np.float64) / 512
    noisy = c["noisy"]
    out = D.denoise(noisy, c["gbuffer"], iterations=d["iterations"], normal_squarings=d["normal_squarings"], flags=int(d["demodulate"]),
                    norm_const=0.25, sigma_color=d["sigma_color"], sigma_depth=d["sigma_depth"], sigma_albedo=d["sigma_albedo"])
    mse_noisy = float(np.mean((noisy[..., :3].astype(np.float64) / 4 - ref) ** 2))
    mse_out = float(np.mean((out[..., :3].astype(np.float64) - ref) ** 2))
    print(f"test_035 64x64: MSE 4 spp {mse_noisy:.6e}, filtered {mse_out:.6e}, ratio {mse_out / mse_noisy:.4f}")
    assert np.isfinite(out).all()
    assert mse_out < mse_noisy


def test_front_end_declares_the_entry_points_and_the_struct():
    import ctypes as C
    from hydracore3_amd import api
    assert "hpt_denoise_frame" in api.ABI and "hpt_denoise_frame_dev" in api.ABI
    assert hasattr(api.HipIntegrator, "denoise") and hasattr(api.HipIntegrator, "denoise_dev")
    hdr = open(os.path.join(ROOT, "include", "hydra_hip.h")).read()
    body = re.search(r"typedef\s+struct\s+hpt_denoise_params\s*\{(.*?)\}\s*hpt_denoise_params\s*;", hdr, re.S).group(1)
    fields = []
    for decl in filter(None, (x.strip() for x in body.split(";"))):
        ctype, names = decl.split(None, 1)
        assert ctype in ("float", "uint32_t"), ctype
        fields += [(n.strip(), C.c_float if ctype == "float" else C.c_uint32) for n in names.split(",")]
    assert fields == list(api.DENOISE_PARAMS._fields_)
    assert C.sizeof(api.DENOISE_PARAMS) == 4 * len(fields) == 28
    # the defaults the header's comment states are the ones the front end passes
    d = api.DENOISE_DEFAULTS
    assert re.search(rf"Defaults {d['sigma_color']}, {d['sigma_depth']}, {d['sigma_albedo']}\b", hdr), "the header's comment states other default sigmas"
    p = api.HipIntegrator.denoise_params(norm_const=0.25)
    assert (p.iterations, p.normalSquarings, p.flags, p.normConst) == (5, 7, 1, 0.25)
