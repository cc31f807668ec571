"""DenoiseFrameVar without a GPU: the surface of the four new entry points, the struct against the header, and the numpy float32 restatement
(tests/denoise_var_reference.py) against things that do not come from it - records worked out by hand, the existing DenoiseFrame restatement, a
float64 convolution, impulses, constants, hard edges, and the CPU oracle's converged frame."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import adaptive_reference as R
import denoise_reference as D
import denoise_var_reference as V
from conftest import ROOT
from test_denoise_cpu import REL_25, cornell_inputs, random_gbuffer, uniform_gbuffer
from test_denoise_gpu import assert_equal_bits, synthetic

SYMBOLS = ["hpt_adaptive_variance", "hpt_adaptive_variance_dev", "hpt_denoise_frame_var", "hpt_denoise_frame_var_dev"]
HDR = os.path.join(ROOT, "include", "hydra_hip.h")
f32 = np.float32
OFF = dict(sigma_depth=0.0, sigma_albedo=0.0, sigma_lum=0.0, normal_squarings=0, flags=0)      # every stop off: the plain B3 filter


def _header():
    return re.sub(r"/\*.*?\*/", " ", open(HDR).read(), flags=re.S)


@pytest.mark.parametrize("name", SYMBOLS)
def test_symbol_is_declared_bound_exported_and_null_safe(name):
    from hydracore3_amd import api
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", _header(), flags=re.S)
    assert m, f"{name} is not declared in include/hydra_hip.h"
    nargs = len(m.group(1).split(","))
    assert name in api.ABI and len(api.ABI[name][1]) == nargs, (name, nargs)
    lib = api.load_library()
    nm = subprocess.run(["nm", "-D", "--defined-only", api.LIB_PATH], capture_output=True, text=True).stdout
    assert re.search(r" T " + name + r"$", nm, flags=re.M)
    canary = np.full(64, 0xA5A5A5A5, np.uint32)                            # a null context: HPT_ERR_ARG and nothing written through any pointer
    args = [None] + [canary.ctypes.data if t is C.c_void_p else 1 for t in api.ABI[name][1][1:]]
    assert getattr(lib, name)(*args) == 1
    assert (canary == 0xA5A5A5A5).all()


def test_struct_layout_matches_the_header_and_the_front_end_has_the_methods():
    from hydracore3_amd import api
    body = re.search(r"typedef struct hpt_denoise_var_params\s*\{(.*?)\}\s*hpt_denoise_var_params\s*;", _header(), flags=re.S).group(1)
    fields = [(n, {"float": C.c_float, "uint32_t": C.c_uint32}[t]) for t, n in re.findall(r"(float|uint32_t)\s+(\w+)\s*;", body)]
    assert fields == list(api.DENOISE_VAR_PARAMS._fields_) and [n for n, _ in fields] == ["sigmaLum", "varFloor", "prefilter", "reserved"]
    assert C.sizeof(api.DENOISE_VAR_PARAMS) == 16 and C.sizeof(api.DENOISE_PARAMS) == 28
    for m in ("AdaptiveVariance", "AdaptiveVariance_dev", "denoise_var", "denoise_var_dev"):
        assert hasattr(api.HipIntegrator, m)
    d = api.DENOISE_VAR_DEFAULTS
    p = api.HipIntegrator.denoise_var_params()
    assert (p.sigmaLum, p.varFloor, p.prefilter, p.reserved) == (f32(d["sigma_lum"]), f32(d["var_floor"]), int(d["prefilter"]), 0)
    assert d["sigma_lum"] > 0 and d["var_floor"] > 0


def _v(rec):
    m = np.zeros(1, R.MOMENTS_DTYPE)
    m[0] = (f32(rec[0]), f32(rec[1]), rec[2], 0)
    return float(V.variance_of_mean(m, np.zeros(1, np.uint32), 0, 1, 1, 1)[0])


def test_variance_of_the_mean_on_hand_worked_records():
    assert _v((123.0, 456.0, 0)) == 0.0                                   # no passes, whatever the sums hold
    assert _v((3.0, 9.0, 1)) == 9.0                                       # one sample: sumY^2, 100 % relative error
    assert _v((4.0, 10.0, 2)) == 1.0                                      # samples 1 and 3: mean 2, var 10 / 2 - 4 = 1, v = 1 / (2 - 1)
    assert _v((8.0, 16.0, 4)) == 0.0                                      # four samples of 2: 16 / 4 - 4 = 0
    assert _v((8.0, 20.0, 4)) == float(f32(1.0) / f32(3.0))               # samples {1, 3, 1, 3}: var 1, v = 1 / 3
    # 3 - 2^-22 over 3 rounds to 1 - 2^-24, the mean is 1: the difference is -2^-24 and is clamped to 0
    assert f32(f32(2.9999998) / f32(3.0)) - f32(1.0) < 0 and _v((3.0, 2.9999998, 3)) == 0.0
    for rec in ((np.nan, 1.0, 5), (1.0, np.inf, 6), (-np.inf, 1.0, 2), (np.nan, np.nan, 1)):
        assert _v(rec) == 0.0, rec
    assert _v((3e38, 3e38, 1)) == np.inf                                  # (the filter's preparation takes a non-finite entry as 0)


def test_variance_plane_is_placed_through_a_tile_swizzled_packed_xy():
    w, h, tile = 16, 8, 8
    xy = R.packed_xy(w, h, tile)
    m = np.zeros(w * h, R.MOMENTS_DTYPE)
    m["passes"] = 2
    m["sumY"] = np.arange(w * h, dtype=f32) * 2                           # two samples t - 1 and t + 1 ... any pair with spread: sumY2 below
    t = np.arange(w * h, dtype=np.float64)
    m["sumY2"] = ((t - 1) ** 2 + (t + 1) ** 2).astype(f32)                # mean t, var 1 -> v = 1 exactly while the squares are exact (t < 2^11)
    m["sumY2"][70] = f32(2 * 70.0 ** 2 + 8)                               # tid 70: samples 68, 72 -> var 4
    keep = np.full(w * h, -7.0, f32)
    out = V.variance_of_mean(m, xy, 60, 20, w, h, out=keep.copy()).reshape(h, w)
    written = np.zeros((h, w), bool)
    for tid in range(60, 80):
        x, y = int(xy[tid]) & 0xFFFF, int(xy[tid]) >> 16
        written[y, x] = True
        assert out[y, x] == (4.0 if tid == 70 else 1.0), (tid, x, y)
    assert written[7, 7] and written[0, 8]                                # tids 63 and 64: the window crosses the seam between tile 0 and tile 1
    assert (out[~written] == -7.0).all() and written.sum() == 20


@pytest.mark.parametrize("flags", [0, 1])
def test_sigma_lum_zero_is_denoise_frame_without_its_colour_stop(flags):
    """The tie to the existing definition: with the luminance stop off the colours are DenoiseFrame's at sigmaColor 0, bit for bit, for any plane."""
    color, gb = synthetic(21, 37, 7)
    rng = np.random.default_rng(3)
    want = D.denoise(color, gb, iterations=3, flags=flags, norm_const=0.5, sigma_color=0.0)
    for var in (np.zeros((21, 37), f32), rng.uniform(0, 5, (21, 37)).astype(f32), np.full((21, 37), np.nan, f32)):
        for pre in (False, True):
            got, _ = V.denoise_var(color, gb, var, iterations=3, flags=flags, norm_const=0.5, sigma_lum=0.0, prefilter_on=pre)
            assert_equal_bits(got, want, f"flags {flags}, prefilter {pre}")


def _squared_b3_f64(v):
    k = np.array([1, 4, 6, 4, 1], np.float64) / 16
    H, W = v.shape
    out = np.zeros((H, W))
    for y in range(H):
        for x in range(W):
            sw = s2 = 0.0
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    qy, qx = y + dy, x + dx
                    if 0 <= qy < H and 0 <= qx < W:
                        h = k[dy + 2] * k[dx + 2]
                        sw += h
                        s2 += h * h * float(v[qy, qx])
            out[y, x] = s2 / (sw * sw)
    return out


def test_variance_propagates_with_the_squared_weights():
    rng = np.random.default_rng(11)
    color = rng.uniform(0.1, 1.0, (11, 14, 4)).astype(f32)
    var = rng.uniform(0.01, 2.0, (11, 14)).astype(f32)
    _, got = V.denoise_var(color, uniform_gbuffer(11, 14), var, iterations=1, **OFF)
    want = _squared_b3_f64(var)                                            # every pixel: those whose footprint leaves the frame included
    rel = np.abs(got.astype(np.float64) - want) / want
    print("variance through one pass: worst relative error", rel.max())
    assert rel.max() <= 1e-6
    _, flat = V.denoise_var(color, uniform_gbuffer(11, 14), np.full((11, 14), 0.75, f32), iterations=1, **OFF)
    # sum h^2 = (sum k^2)^2, sum k^2 = (1 + 16 + 36 + 16 + 1) / 256 = 70 / 256 = 35 / 128
    want_flat = 0.75 * (35 / 128) ** 2
    assert np.abs(flat[2:-2, 2:-2].astype(np.float64) - want_flat).max() <= 1e-6 * want_flat
    assert (flat[0, 0] > flat[5, 5]) and abs(float(flat[0, 0]) - 0.75 * (53 / 256) ** 2 / (11 / 16) ** 4) <= 1e-6       # corner: k = {6, 4, 1} / 16


def test_prefilter_of_an_impulse():
    v = np.zeros((9, 11), f32)
    v[4, 5] = 1.0
    p = V.prefilter(v)
    assert p[4, 5] == 0.25 and p[4, 4] == p[4, 6] == p[3, 5] == p[5, 5] == 0.125 and p[3, 4] == p[5, 6] == 0.0625
    assert p[4, 7] == 0 and p[2, 5] == 0 and np.count_nonzero(p) == 9
    c = np.zeros((9, 11), f32)
    c[0, 0] = 1.0
    assert V.prefilter(c)[0, 0] == f32(4 / 9)                             # (1/4) / (1/4 + 1/8 + 1/8 + 1/16) = (1/4) / (9/16)
    assert V.prefilter(np.ones((1, 1), f32))[0, 0] == 1.0


def test_constants_stay_constant_over_a_random_gbuffer():
    color = np.full((13, 17, 4), 0.37, f32)
    got, var = V.denoise_var(color, random_gbuffer(13, 17, 2), np.full((13, 17), 0.02, f32), iterations=3, flags=0)
    rel = np.abs(got[..., :3].astype(np.float64) - np.float64(f32(0.37))) / 0.37
    assert rel.max() <= 3 * REL_25
    assert np.isfinite(var).all() and (var >= 0).all() and var.max() <= 0.02 * (1 + 3 * REL_25)      # a convex combination never raises it


def test_stops_still_hold_for_colour_and_variance():
    g = uniform_gbuffer(12, 20)
    g["instId"][:, 10:] = 1
    color = np.zeros((12, 20, 4), f32)
    color[:, :10, :3], color[:, 10:, :3] = 1.25, 5.0
    var = np.zeros((12, 20), f32)
    var[:, :10], var[:, 10:] = 0.5, 8.0
    got, gv = V.denoise_var(color, g, var, iterations=4, flags=0)
    for side, c, v in ((np.s_[:, :10], 1.25, 0.5), (np.s_[:, 10:], 5.0, 8.0)):
        assert (np.abs(got[side][..., :3].astype(np.float64) - c) / c).max() <= 4 * REL_25
        assert gv[side].max() <= v * (1 + 4 * REL_25) and gv[side].min() > 0          # 8.0 never reaches the left half
    # a planted NaN / Inf colour is rebuilt from its neighbours, and so is its variance; NaN / Inf / negative variances count as 0
    color = np.full((9, 12, 4), 0.75, f32)
    color[4, 5, 0], color[2, 2, 1], color[7, 10, 2], color[0, 0, :3] = np.nan, np.inf, -np.inf, np.nan
    var = np.full((9, 12), 0.01, f32)
    var[4, 5], var[1, 1], var[6, 6], var[8, 11] = np.nan, np.inf, -3.0, 0.0
    got, gv = V.denoise_var(color, uniform_gbuffer(9, 12), var, iterations=2, flags=0)
    assert np.isfinite(got).all() and np.isfinite(gv).all() and (gv >= 0).all()
    assert np.abs(got[..., :3].astype(np.float64) - 0.75).max() <= 0.75 * 2 * REL_25
    assert gv.max() <= 0.01 * (1 + 2 * REL_25)


def test_the_stop_follows_the_variance():
    """One surface, grey luminance 1 left of column 16 and 1 + d right of it, sigmaLum 4, three iterations (steps 1, 2, 4), d = 0.5.

    Every stop but x_l is 1 here (one normal, one depth... the depth and albedo terms are switched off), so a tap across the edge weighs
    h / (1 + x_l) with x_l = dl^2 / (16 v + varFloor), a tap on the pixel's own side h. A pixel beside the edge has at most the columns dx = +1, +2
    across it, 5/16 of the kernel's mass, and 11/16 on its own side (clipped rows scale both alike).

    v = 1e-6 d^2: x_l >= (0.99 d)^2 / (16e-6 d^2) > 61000 as long as no pixel has moved by 0.005 d, and the variance only shrinks from pass to
    pass. A pass moves a pixel by at most d (5/16) / (11/16) / (1 + x_l) < 7.5e-6 d: three passes 2.3e-5 d, plus the rounding of three
    passes, 3 * 32 * 2^-24 * 1.5 = 1.7e-5 d at values of 1.5. Bound: 1e-4 d.

    v = 100 d^2: the weights of pass i lie in [h / (1 + x_i), h] with x_i <= d^2 / (16 v_i); v_1 = 100 d^2 and a pass leaves at least
    (35/128)^2 / (1 + x_i)^2 of the variance, so x_1 <= 1/1600, x_2 <= 0.0084, x_3 <= 0.113. A weighted mean whose weights are perturbed by a
    relative x over values spanning d moves by at most x d, and the B3 passes after it do not amplify that (they are convex combinations): the result
    is within (x_1 + x_2 + x_3) d < 0.123 d of the plain three-pass B3 filter of the step. The plain filter's composed 1D kernel has mass
    344 / 4096 at offset 0 (a + 2 b + 4 c = 0: 6 (36 + 4 + 4) + 2 * 4 (6 + 4)), so the pixel left of the edge receives (1 - 0.084) / 2 = 0.458 of
    the step: it moves by at least 0.458 d - 0.123 d = 0.335 d. Bound: 0.25 d, the issue's."""
    d = 0.5
    color = np.zeros((24, 32, 4), f32)
    color[:, :16, :3], color[:, 16:, :3] = 1.0, 1.0 + d
    g = uniform_gbuffer(24, 32)
    kw = dict(iterations=3, flags=0, sigma_depth=0.0, sigma_albedo=0.0, sigma_lum=4.0, var_floor=1e-12)
    tight, _ = V.denoise_var(color, g, np.full((24, 32), 1e-6 * d * d, f32), **kw)
    moved = np.abs(tight[..., :3].astype(np.float64) - color[..., :3])
    print("small variance: the frame moves by at most", moved.max() / d, "d")
    assert moved.max() < 1e-4 * d
    loose, _ = V.denoise_var(color, g, np.full((24, 32), 100 * d * d, f32), **kw)
    left, right = loose[:, 15, 0].astype(np.float64) - 1.0, (1.0 + d) - loose[:, 16, 0].astype(np.float64)
    print("large variance: the edge pixels move by", left.min() / d, "...", left.max() / d, "d")
    assert left.min() > 0.25 * d and right.min() > 0.25 * d


_passes = {}


def cornell_passes():
    """Four successive one-pass renders of test_035 at 64 x 64 on one OracleIntegrator, and the records the restatement accumulates from them."""
    if not _passes:
        from oracle.orc import OracleIntegrator
        cpu = OracleIntegrator(cornell_inputs()["scene"])
        frames = [cpu.render(1) for _ in range(4)]
        m = np.zeros(64 * 64, R.MOMENTS_DTYPE)
        R.accumulate(m, [(R.luminance(f[..., :3]).reshape(-1), np.ones(64 * 64, bool)) for f in frames])
        _passes["frames"], _passes["moments"] = frames, m
        _passes["variance"] = V.variance_of_mean(m, R.packed_xy(64, 64, 1), 0, 64 * 64, 64, 64).reshape(64, 64)
    return _passes


def quality(out, noisy_mean, ref):
    """(ratio of MSEs over the whole frame, over the dim pixels: neither the 4-spp nor the 512-spp frame above 2; profiles/denoise.md)."""
    dim = (noisy_mean.max(-1) <= 2) & (ref.max(-1) <= 2)
    e_out, e_in = (out[..., :3].astype(np.float64) - ref) ** 2, (noisy_mean - ref) ** 2
    return float(e_out.mean() / e_in.mean()), float(e_out[dim].mean() / e_in[dim].mean())


def test_variance_guided_4spp_frame_is_closer_to_the_converged_frame():
    """The quality condition on the CPU oracle, with the front end's defaults. The variance plane is that of the mean of the four samples, so the
    frame handed over is the mean as well (the 4-spp sum times 1/4, exact) and norm_const is 1, as after AdaptiveResolve."""
    from hydracore3_amd import api
    c, p = cornell_inputs(), cornell_passes()
    total = ((p["frames"][0] + p["frames"][1]) + p["frames"][2]) + p["frames"][3]
    assert_equal_bits(total, c["noisy"], "the sum of four one-pass renders vs the 4-spp render")      # the oracle carries its generators from call to call
    ref = c["converged"][..., :3].astype(np.float64) / 512
    mean = c["noisy"] * f32(0.25)
    assert (p["variance"] > 0).any() and np.isfinite(p["variance"]).all()
    d, dv = api.DENOISE_DEFAULTS, api.DENOISE_VAR_DEFAULTS
    out, out_var = V.denoise_var(mean, c["gbuffer"], p["variance"], iterations=d["iterations"], normal_squarings=d["normal_squarings"], flags=int(d["demodulate"]),
                                 sigma_depth=d["sigma_depth"], sigma_albedo=d["sigma_albedo"], sigma_lum=dv["sigma_lum"], var_floor=dv["var_floor"],
                                 prefilter_on=dv["prefilter"])
    whole, dim = quality(out, mean[..., :3].astype(np.float64), ref)
    print(f"test_035 64x64, variance-guided: MSE ratio whole frame {whole:.4f} (fixed stop: 0.9909), dim pixels {dim:.4f} (fixed stop: 0.546)")
    assert np.isfinite(out).all() and np.isfinite(out_var).all()
    assert whole < 1.0 and dim < 1.0
