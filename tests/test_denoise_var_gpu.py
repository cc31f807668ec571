"""DenoiseFrameVar and hpt_adaptive_variance on the GPU against the numpy float32 restatement (tests/denoise_var_reference.py), compared as
uint32 views: equality is the bar."""
import ctypes as C

import numpy as np
import pytest

import adaptive_reference as R
import denoise_reference as D
import denoise_var_reference as V
from conftest import scene_path
from hydracore3_amd.api import DENOISE_DEFAULTS, DENOISE_PARAMS, DENOISE_VAR_DEFAULTS, DENOISE_VAR_PARAMS, GBUFFER_DTYPE, MOMENTS_DTYPE
from test_denoise_gpu import assert_equal_bits, device_denoise, params_of, synthetic

HPT_ERR_ARG = 1
_vp = C.c_void_p
f32 = np.float32


def variance_plane(h, w, seed):
    """Positive over four decades, with a 0, a negative, a NaN, a +Inf and a 1e30 entry planted (the first pixels in a frame too small for all)."""
    rng = np.random.default_rng(seed)
    v = (10.0 ** rng.uniform(-4.0, 0.0, (h, w))).astype(f32)
    flat = v.reshape(-1)
    at = np.linspace(0, flat.size - 1, 5).astype(int) if flat.size >= 5 else np.arange(flat.size)
    for i, bad in zip(at, (0.0, -0.5, np.nan, np.inf, 1e30)):
        flat[i] = bad
    return v


def var_params_of(kw):
    d = dict(iterations=DENOISE_DEFAULTS["iterations"], normal_squarings=DENOISE_DEFAULTS["normal_squarings"], flags=int(DENOISE_DEFAULTS["demodulate"]),
             norm_const=1.0, sigma_depth=DENOISE_DEFAULTS["sigma_depth"], sigma_albedo=DENOISE_DEFAULTS["sigma_albedo"],
             sigma_lum=DENOISE_VAR_DEFAULTS["sigma_lum"], var_floor=DENOISE_VAR_DEFAULTS["var_floor"], prefilter_on=DENOISE_VAR_DEFAULTS["prefilter"])
    d.update(kw)
    return d


def device_denoise_var(g, color, var, gb, kw, return_variance=True):
    d = var_params_of(kw)
    return g.denoise_var(color, var, gb, norm_const=d["norm_const"], iterations=d["iterations"], normal_squarings=d["normal_squarings"], sigma_depth=d["sigma_depth"],
                         sigma_albedo=d["sigma_albedo"], demodulate=bool(d["flags"]), sigma_lum=d["sigma_lum"], var_floor=d["var_floor"], prefilter=d["prefilter_on"],
                         return_variance=return_variance)


def check(g, color, var, gb, kw, what):
    got, got_v = device_denoise_var(g, color, var, gb, kw)
    want, want_v = V.denoise_var(color, gb, var, **var_params_of(kw))
    assert_equal_bits(got, want, what + ": colours")
    assert_equal_bits(got_v[..., None], want_v[..., None], what + ": outVar")
    return got, got_v


@pytest.fixture(scope="module")
def gpu():
    from hydracore3_amd.api import HipIntegrator
    return HipIntegrator()                                                # a created context only


# the sizes of test_denoise_gpu.py: the tile halo leaves the frame on every side, a last wave is partly filled, the LDS path (steps 1, 2) and the direct one run
SIZES = [(1, 1, {}), (5, 3, {}), (17, 9, {}), (67, 33, {"iterations": 3}), (64, 48, {"iterations": 5})]


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,kw", SIZES, ids=[f"{w}x{h}" for w, h, _ in SIZES])
def test_synthetic_frames_equal_the_restatement(gpu, w, h, kw):
    color, gb = synthetic(h, w, 100 + w)
    var = variance_plane(h, w, 200 + w)
    if w >= 17:
        assert np.isnan(var).any() and np.isinf(var).any() and (var < 0).any() and (var == 0).any() and (var == f32(1e30)).any()
        good = var[np.isfinite(var) & (var > 0) & (var < 1e29)]
        assert good.max() / good.min() > 1e3
    check(gpu, color, var, gb, kw, f"{w} x {h}")


VARIANTS = {"sigma_lum 0": {"sigma_lum": 0.0}, "no prefilter": {"prefilter_on": False}, "no demodulation": {"flags": 0},
            "var_floor 1e-12": {"var_floor": 1e-12}, "var_floor 1": {"var_floor": 1.0},
            "one iteration": {"iterations": 1}, "two iterations": {"iterations": 2}, "eight iterations": {"iterations": 8},
            "norm_const 0.25": {"norm_const": 0.25}, "sigma_depth 0": {"sigma_depth": 0.0}, "sigma_albedo 0": {"sigma_albedo": 0.0}}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(VARIANTS))
def test_each_parameter(gpu, name):
    color, gb = synthetic(21, 37, 7)
    var = variance_plane(21, 37, 8)
    kw = dict({"iterations": 3}, **VARIANTS[name])
    got, _ = check(gpu, color, var, gb, kw, name)
    if name == "sigma_lum 0":                                             # the tie to DenoiseFrame, on the device as well
        assert_equal_bits(got, device_denoise(gpu, color, gb, {"iterations": 3, "sigma_color": 0.0}), "sigma_lum 0 vs DenoiseFrame at sigma_color 0")


@pytest.mark.gpu
def test_out_var_null(gpu):
    color, gb = synthetic(21, 37, 7)
    var = variance_plane(21, 37, 8)
    got = device_denoise_var(gpu, color, var, gb, {"iterations": 3}, return_variance=False)
    assert_equal_bits(got, V.denoise_var(color, gb, var, **var_params_of({"iterations": 3}))[0], "outVar NULL")


@pytest.mark.gpu
def test_adaptive_variance_equals_the_restatement():
    from hydracore3_amd.api import HipIntegrator
    from hydracore3_amd.scene import load_hydra_xml
    w, h = 24, 16
    g = HipIntegrator(load_hydra_xml(scene_path("test_035"), w, h))
    xy = g.packed_xy()
    seams = [t for t in range(1, g.N) if (xy[t] >> 16) < (xy[t - 1] >> 16)]            # a tile ends where y steps back
    begin = seams[0] if seams else w                                      # the first tid of the second tile (row-major: of the second row)
    count = g.N - begin - 37
    rng = np.random.default_rng(5)
    m = np.zeros(g.N, MOMENTS_DTYPE)
    m["passes"] = rng.integers(0, 9, g.N)
    y = rng.uniform(0.0, 3.0, (g.N, 8)).astype(f32)
    for k in range(8):                                                    # plausible records: sums of the first `passes` of eight samples
        take = m["passes"] > k
        m["sumY"] = np.where(take, m["sumY"] + y[:, k], m["sumY"])
        m["sumY2"] = np.where(take, m["sumY2"] + y[:, k] * y[:, k], m["sumY2"])
    crafted = [(123.0, 456.0, 0), (3.0, 9.0, 1), (4.0, 10.0, 2), (8.0, 16.0, 4), (8.0, 20.0, 4), (3.0, 2.9999998, 3), (np.nan, 1.0, 5), (1.0, np.inf, 6),
               (-np.inf, 1.0, 2), (3e38, 3e38, 1)]
    for i, (a, b, n) in enumerate(crafted):
        m[begin + 3 + i] = (f32(a), f32(b), n, 0)
    recs = R.crafted_records()
    m[begin + 40:begin + 40 + len(recs)] = recs
    canary = np.full((h, w), -7.0, f32)
    want = V.variance_of_mean(m, xy, begin, count, w, h, out=canary.copy()).reshape(h, w)
    got = g.AdaptiveVariance(m, tid=count, tid_begin=begin, out=canary.copy())
    assert_equal_bits(got[..., None], want[..., None], "hpt_adaptive_variance")
    assert (got == -7.0).sum() == g.N - count and (want > 0).sum() > count // 2
    # refusals: a null pointer, a window past the packed range; nothing is written
    out = canary.copy()
    for args, word in (((begin, count, None, out.ctypes.data), "moments"), ((begin, count, m.ctypes.data, None), "outVar"),
                       ((begin, g.N - begin + 1, m.ctypes.data, out.ctypes.data), "tid range")):
        rc, rd = g.L.hpt_adaptive_variance(g.h, *args), g.L.hpt_adaptive_variance_dev(g.h, *args, None)
        msg = g.L.hpt_last_error(g.h).decode()
        assert rc == rd == HPT_ERR_ARG and word in msg and "AdaptiveVariance" in msg, (rc, rd, msg)
        assert (out == -7.0).all()


@pytest.mark.gpu
def test_adaptive_frame_resident_on_the_device_end_to_end():
    """test_035 at 64 x 64 on a non-default stream: the adaptive loop, resolve, variance plane, G-buffer and the filter hand their arrays over on
    the device; the host-pointer forms on downloaded copies give the same bits, and both equal the restatement."""
    from hydracore3_amd.api import HipIntegrator
    from hydracore3_amd.scene import load_hydra_xml
    g = HipIntegrator(load_hydra_xml(scene_path("test_035"), 64, 64))
    n = g.N
    sizes = dict(frame=n * 16, mom=n * 16, var=n * 4, gb=n * 60, out=n * 16, out_var=n * 4)
    d = {k: _vp() for k in sizes}
    for k, nbytes in sizes.items():
        g._chk(g.L.hpt_device_malloc(g.h, nbytes, C.byref(d[k])))
    try:
        g._chk(g.L.hpt_device_memset(g.h, d["frame"], 0, n * 16))
        hip = C.CDLL("libamdhip64.so")
        sp = _vp()
        assert hip.hipStreamCreate(C.byref(sp)) == 0 and sp.value
        info = g.PathTraceBlockAdaptive_dev(d["frame"], 2, d["mom"], tol=0.25, lum_floor=0.05, min_passes=2, max_passes=8, step=16, dilate=1, stream=sp)
        g.AdaptiveResolve_dev(d["frame"], d["mom"], d["frame"], stream=sp)
        g.AdaptiveVariance_dev(d["mom"], d["var"], stream=sp)
        g._chk(g.L.hpt_eval_gbuffer_dev(g.h, n, d["gb"], None, sp))
        g.denoise_var_dev(d["frame"], d["gb"], d["var"], d["out"], d["out_var"], stream=sp)
        assert hip.hipStreamSynchronize(sp) == 0
        assert g.last_kernel_ms() > 0.0
        frame, out = np.zeros((64, 64, 4), f32), np.zeros((64, 64, 4), f32)
        var, out_var = np.zeros((64, 64), f32), np.zeros((64, 64), f32)
        gb, mom = np.zeros((64, 64), GBUFFER_DTYPE), np.zeros(n, MOMENTS_DTYPE)
        for host, key in ((frame, "frame"), (out, "out"), (var, "var"), (out_var, "out_var"), (gb, "gb"), (mom, "mom")):
            g._chk(g.L.hpt_device_copy(g.h, host.ctypes.data, d[key], host.nbytes, 2))
        assert hip.hipStreamDestroy(sp) == 0
    finally:
        for p in d.values():
            g.L.hpt_device_free(g.h, p)
    print("adaptive loop:", info, "passes", np.unique(mom["passes"]))
    assert mom["passes"].min() >= 2 and mom["passes"].max() <= 8 and len(np.unique(mom["passes"])) > 1, "the pass counts do not differ between pixels"
    assert len(np.unique(var)) > 16 and np.isfinite(var).all()
    assert_equal_bits(var[..., None], V.variance_of_mean(mom, g.packed_xy(), 0, n, 64, 64).reshape(64, 64, 1), "variance plane vs restatement")
    assert_equal_bits(g.AdaptiveVariance(mom)[..., None], var[..., None], "host-pointer AdaptiveVariance vs device form")
    host, host_v = g.denoise_var(frame, var, gb, return_variance=True)
    assert_equal_bits(host, out, "host-pointer form vs device-pointer form")
    assert_equal_bits(host_v[..., None], out_var[..., None], "host-pointer form vs device-pointer form: outVar")
    want, want_v = V.denoise_var(frame, gb, var, **var_params_of({}))
    assert_equal_bits(out, want, "device vs restatement")
    assert_equal_bits(out_var[..., None], want_v[..., None], "device vs restatement: outVar")


@pytest.mark.gpu
def test_denoise_frame_is_untouched_and_scratch_regrows():
    from hydracore3_amd.api import HipIntegrator
    g = HipIntegrator()
    for w, h in ((9, 7), (80, 50), (9, 7)):
        color, gb = synthetic(h, w, w * h)
        var = variance_plane(h, w, w + h)
        check(g, color, var, gb, {}, f"{w} x {h} after another size")
        assert_equal_bits(device_denoise(g, color, gb, {}), D.denoise(color, gb, **params_of({})), f"DenoiseFrame at {w} x {h} after DenoiseFrameVar")
        check(g, color, var, gb, {"iterations": 2}, f"{w} x {h} after DenoiseFrame")


@pytest.mark.gpu
def test_timing_slot(gpu):
    color, gb = synthetic(48, 64, 3)
    device_denoise(gpu, color, gb, {})
    before = gpu.GetExecutionTime("DenoiseFrame")
    device_denoise_var(gpu, color, variance_plane(48, 64, 4), gb, {})
    slots = gpu.GetExecutionTime("DenoiseFrameVar")
    assert slots[0] > 0.0 and slots[0] == gpu.last_kernel_ms()
    assert slots[1] > 0.0 and slots[2] > 0.0
    assert gpu.GetExecutionTime("DenoiseFrame") == before                 # a slot of its own


@pytest.mark.gpu
def test_refusals_by_code_and_message(gpu):
    g = gpu
    color, gb = synthetic(6, 8, 1)
    var = variance_plane(6, 8, 2)
    out = np.full((6, 8, 4), 7.0, f32)
    out_var = np.full((6, 8), 7.0, f32)
    ok = g.denoise_params(sigma_color=0.0)
    okv = g.denoise_var_params()

    def call(width=8, height=6, c=color.ctypes.data, gbuf=gb.ctypes.data, v=var.ctypes.data, p=ok, pv=okv, o=out.ctypes.data, ov=out_var.ctypes.data):
        a = (g.h, width, height, c, gbuf, v, None if p is None else C.byref(p), None if pv is None else C.byref(pv), o, ov)
        rc = g.L.hpt_denoise_frame_var(*a)
        rd = g.L.hpt_denoise_frame_var_dev(*a, None)                       # refused before any pointer is used
        assert rc == rd, (rc, rd)
        return rc, g.L.hpt_last_error(g.h).decode()

    def mod(base, **kw):
        p = type(base).from_buffer_copy(bytes(base))
        for k, val in kw.items():
            setattr(p, k, val)
        return p

    nan, inf = float("nan"), float("inf")
    cases = [(dict(c=None), "color"), (dict(gbuf=None), "gbuffer"), (dict(p=None), "params"), (dict(o=None), "out"),
             (dict(width=0), "width"), (dict(height=0), "height"),
             (dict(p=mod(ok, iterations=0)), "iterations"), (dict(p=mod(ok, iterations=9)), "iterations"), (dict(p=mod(ok, normalSquarings=9)), "normalSquarings"),
             (dict(p=mod(ok, sigmaColor=-1.0)), "sigmaColor"), (dict(p=mod(ok, sigmaDepth=nan)), "sigmaDepth"), (dict(p=mod(ok, sigmaAlbedo=inf)), "sigmaAlbedo"),
             (dict(p=mod(ok, normConst=-0.5)), "normConst"), (dict(p=mod(ok, normConst=inf)), "normConst"),
             (dict(p=mod(ok, flags=2)), "flags"), (dict(p=mod(ok, flags=0x80000001)), "flags"),
             (dict(o=color.ctypes.data), "aliases"), (dict(o=color.ctypes.data + 16), "aliases"),
             (dict(v=None), "variance"), (dict(pv=None), "var_params"),
             (dict(pv=mod(okv, sigmaLum=-1.0)), "sigmaLum"), (dict(pv=mod(okv, sigmaLum=nan)), "sigmaLum"), (dict(pv=mod(okv, sigmaLum=inf)), "sigmaLum"),
             (dict(pv=mod(okv, varFloor=0.0)), "varFloor"), (dict(pv=mod(okv, varFloor=-1e-3)), "varFloor"), (dict(pv=mod(okv, varFloor=nan)), "varFloor"),
             (dict(pv=mod(okv, varFloor=inf)), "varFloor"), (dict(pv=mod(okv, reserved=1)), "reserved"),
             (dict(p=mod(ok, sigmaColor=0.6)), "sigmaColor"),
             (dict(o=var.ctypes.data), "out aliases variance"), (dict(v=out.ctypes.data + 64), "out aliases variance"),
             (dict(ov=color.ctypes.data + 32), "outVar aliases color"), (dict(ov=gb.ctypes.data + 60), "outVar aliases gbuffer"),
             (dict(ov=var.ctypes.data + 4), "outVar aliases variance"), (dict(ov=out.ctypes.data + 6 * 8 * 16 - 4), "outVar aliases out")]
    for kw, word in cases:
        rc, msg = call(**kw)
        assert rc == HPT_ERR_ARG and word in msg and "DenoiseFrameVar" in msg, (kw, rc, msg)
        assert np.all(out == 7.0) and np.all(out_var == 7.0), f"written after a refusal ({word})"
    a = (8, 6, color.ctypes.data, gb.ctypes.data, var.ctypes.data, C.byref(ok), C.byref(okv), out.ctypes.data, out_var.ctypes.data)
    assert g.L.hpt_denoise_frame_var(None, *a) == HPT_ERR_ARG and g.L.hpt_denoise_frame_var_dev(None, *a, None) == HPT_ERR_ARG
    assert np.all(out == 7.0) and np.all(out_var == 7.0)
    assert g.L.hpt_denoise_frame_var(g.h, *a) == 0 and not np.all(out == 7.0) and not np.all(out_var == 7.0)
    want, want_v = V.denoise_var(color, gb, var, **var_params_of({}))
    assert_equal_bits(out, want, "the good call")
    assert_equal_bits(out_var[..., None], want_v[..., None], "the good call: outVar")
