"""DenoiseFrame on the GPU against the numpy float32 restatement (tests/denoise_reference.py), compared as uint32 views: equality is the bar."""
import ctypes as C

import numpy as np
import pytest

import denoise_reference as D
from conftest import scene_path
from hydracore3_amd.api import DENOISE_DEFAULTS, DENOISE_PARAMS, GBUFFER_DTYPE

HPT_ERR_ARG = 1
_vp = C.c_void_p


def synthetic(h, w, seed):
    """A frame and a G-buffer with everything the filter branches on: three surfaces with id edges (an instance edge, a material edge inside
    one instance), a block of misses as EvalGBuffer writes them, smooth and random normals, a depth ramp, zero albedo, NaN / Inf colours."""
    rng = np.random.default_rng(seed)
    g = np.zeros((h, w), GBUFFER_DTYPE)
    n = rng.normal(size=(h, w, 3)) * 0.15 + np.array([0.2, 0.1, 1.0])
    g["norm"] = (n / np.linalg.norm(n, axis=-1, keepdims=True)).astype(np.float32)
    yy, xx = np.mgrid[0:h, 0:w]
    g["depth"] = (2.0 + 0.05 * xx + 0.02 * yy + rng.uniform(0, 0.01, (h, w))).astype(np.float32)
    g["rgba"][..., :3] = rng.uniform(0.05, 1.0, (h, w, 3)).astype(np.float32)
    g["rgba"][..., 3], g["coverage"] = 1.0, 1.0
    g["instId"] = (xx * 3 // max(w, 1)).astype(np.int32)                  # three vertical bands
    g["matId"] = g["instId"] + (yy > h // 2)                              # a material edge across each band
    g["objId"] = g["instId"]
    miss = (yy < max(h // 4, 1)) & (xx >= w - max(w // 4, 1))             # the top right corner sees the background
    g["depth"][miss], g["norm"][miss], g["rgba"][miss], g["coverage"][miss] = 0.0, (0, 0, 1), 0.0, 0.0
    g["instId"][miss] = g["matId"][miss] = g["objId"][miss] = -1
    zero = rng.random((h, w)) < 0.05
    g["rgba"][zero, :3] = 0.0                                             # zero albedo under demodulation: the floor of 1e-3
    color = (rng.uniform(0.0, 2.0, (h, w, 4)) * (g["rgba"][..., :3].mean(-1, keepdims=True) + 0.1)).astype(np.float32)
    color[..., 3] = rng.uniform(0.0, 4.0, (h, w)).astype(np.float32)
    bad = rng.random((h, w))
    color[bad < 0.03, 0] = np.nan
    color[(bad >= 0.03) & (bad < 0.05), 1] = np.inf
    color[(bad >= 0.05) & (bad < 0.06), 2] = -np.inf
    return color, g


def params_of(kw):
    d = dict(iterations=DENOISE_DEFAULTS["iterations"], normal_squarings=DENOISE_DEFAULTS["normal_squarings"], flags=int(DENOISE_DEFAULTS["demodulate"]),
             norm_const=1.0, sigma_color=DENOISE_DEFAULTS["sigma_color"], sigma_depth=DENOISE_DEFAULTS["sigma_depth"], sigma_albedo=DENOISE_DEFAULTS["sigma_albedo"])
    d.update(kw)
    return d


def device_denoise(g, color, gb, kw):
    d = params_of(kw)
    return g.denoise(color, gb, norm_const=d["norm_const"], iterations=d["iterations"], normal_squarings=d["normal_squarings"], sigma_color=d["sigma_color"],
                     sigma_depth=d["sigma_depth"], sigma_albedo=d["sigma_albedo"], demodulate=bool(d["flags"]))


def assert_equal_bits(got, want, what):
    a, b = np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32)
    diff = a != b
    if diff.any():
        y, x, ch = np.argwhere(diff)[0]
        raise AssertionError(f"{what}: {int(diff.sum())} of {diff.size} floats differ; first at (y {y}, x {x}, channel {ch}): device {got[y, x, ch]!r} "
                             f"({a[y, x, ch]:#010x}) restatement {want[y, x, ch]!r} ({b[y, x, ch]:#010x})")


@pytest.fixture(scope="module")
def gpu():
    from hydracore3_amd.api import HipIntegrator
    return HipIntegrator()                                                # a created context only: no scene, no PackXYBlock, no generators


# 1 x 1; 5 x 3: smaller than the footprint at any step; 17 x 9; 67 x 33: no multiple of the 32 x 8 tile, a last wave partly filled, 3 x 5 blocks;
# 64 x 48 with 5 iterations: step 16 reaches past half the height. Steps 1 and 2 run from an LDS tile whose halo leaves the frame on every side
# here, steps 4 and up from direct loads: every case with three or more iterations takes both paths.
SIZES = [(1, 1, {}), (5, 3, {}), (17, 9, {}), (67, 33, {"iterations": 3}), (64, 48, {"iterations": 5})]


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,kw", SIZES, ids=[f"{w}x{h}" for w, h, _ in SIZES])
def test_synthetic_frames_equal_the_restatement(gpu, w, h, kw):
    color, gb = synthetic(h, w, 100 + w)
    kw = dict(kw, norm_const=0.25)
    got = device_denoise(gpu, color, gb, kw)
    want = D.denoise(color, gb, **params_of(kw))
    if w >= 17:
        assert not np.isfinite(color[..., :3]).all() and (gb["instId"] < 0).any() and (gb["rgba"][..., :3] == 0).any()
    assert_equal_bits(got, want, f"{w} x {h}")


VARIANTS = {"sigma_color 0": {"sigma_color": 0.0}, "sigma_depth 0": {"sigma_depth": 0.0}, "sigma_albedo 0": {"sigma_albedo": 0.0},
            "no demodulation": {"flags": 0}, "no squaring": {"normal_squarings": 0}, "eight squarings": {"normal_squarings": 8},
            "one iteration": {"iterations": 1}, "two iterations": {"iterations": 2}, "wide sigmas": {"sigma_color": 4.0, "sigma_depth": 1.0, "sigma_albedo": 2.0}}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(VARIANTS))
def test_each_term_switched_off_and_the_other_parameters(gpu, name):
    color, gb = synthetic(21, 37, 7)
    kw = dict({"iterations": 3}, **VARIANTS[name])
    assert_equal_bits(device_denoise(gpu, color, gb, kw), D.denoise(color, gb, **params_of(kw)), name)


@pytest.mark.gpu
def test_eight_iterations(gpu):
    color, gb = synthetic(40, 35, 9)
    kw = {"iterations": 8}                                                # step 128: only the centre tap is inside the frame
    assert_equal_bits(device_denoise(gpu, color, gb, kw), D.denoise(color, gb, **params_of(kw)), "8 iterations")


@pytest.mark.gpu
def test_scratch_regrows_between_calls_of_different_sizes():
    from hydracore3_amd.api import HipIntegrator
    g = HipIntegrator()
    for w, h in ((9, 7), (80, 50), (9, 7), (33, 70)):
        color, gb = synthetic(h, w, w * h)
        assert_equal_bits(device_denoise(g, color, gb, {}), D.denoise(color, gb, **params_of({})), f"{w} x {h} after another size")


@pytest.mark.gpu
def test_rendered_frame_and_gbuffer_resident_on_the_device():
    """test_035 at 64 x 64: 4 spp from PathTraceBlock and the records of EvalGBuffer, both made on the device and handed over there, filtered on a
    non-default stream; the host-pointer form on downloaded copies gives the same bits, and both equal the restatement."""
    from hydracore3_amd.api import HipIntegrator
    from hydracore3_amd.scene import load_hydra_xml
    sc = load_hydra_xml(scene_path("test_035"), 64, 64)
    g = HipIntegrator(sc)
    n = g.N
    ptrs = [_vp() for _ in range(3)]
    for p, nbytes in zip(ptrs, (n * 16, n * 60, n * 16)):
        g._chk(g.L.hpt_device_malloc(g.h, nbytes, C.byref(p)))
    d_frame, d_gb, d_out = ptrs
    try:
        g._chk(g.L.hpt_device_memset(g.h, d_frame, 0, n * 16))
        hip = C.CDLL("libamdhip64.so")                                    # the runtime the library is linked against
        sp = _vp()
        assert hip.hipStreamCreate(C.byref(sp)) == 0 and sp.value
        g.path_trace_block_dev(d_frame, 4, stream=sp)
        g._chk(g.L.hpt_eval_gbuffer_dev(g.h, n, d_gb, None, sp))
        g.denoise_dev(d_frame, d_gb, d_out, norm_const=0.25, stream=sp)
        assert hip.hipStreamSynchronize(sp) == 0
        assert g.last_kernel_ms() > 0.0
        frame, out = np.zeros((64, 64, 4), np.float32), np.zeros((64, 64, 4), np.float32)
        gb = np.zeros((64, 64), GBUFFER_DTYPE)
        for host, dev in ((frame, d_frame), (gb, d_gb), (out, d_out)):
            g._chk(g.L.hpt_device_copy(g.h, host.ctypes.data, dev, host.nbytes, 2))
        assert hip.hipStreamDestroy(sp) == 0
    finally:
        for p in ptrs:
            g.L.hpt_device_free(g.h, p)
    assert frame[..., :3].mean() > 0 and (gb["instId"] >= 0).any()
    assert_equal_bits(g.denoise(frame, gb, norm_const=0.25), out, "host-pointer form vs device-pointer form")
    assert_equal_bits(out, D.denoise(frame, gb, **params_of({"norm_const": 0.25})), "device vs restatement")
    assert_equal_bits(g.denoise(frame, norm_const=0.25), out, "gbuffer=None: EvalGBuffer made by the call")


@pytest.mark.gpu
def test_timing_slot(gpu):
    color, gb = synthetic(48, 64, 3)
    device_denoise(gpu, color, gb, {})
    slots = gpu.GetExecutionTime("DenoiseFrame")
    assert slots[0] > 0.0 and slots[0] == gpu.last_kernel_ms()
    assert slots[1] > 0.0 and slots[2] > 0.0


@pytest.mark.gpu
def test_refusals_by_code_and_message(gpu):
    g = gpu
    color, gb = synthetic(6, 8, 1)
    out = np.full((6, 8, 4), 7.0, np.float32)
    ok = g.denoise_params()

    def call(width=8, height=6, c=color.ctypes.data, gbuf=gb.ctypes.data, p=ok, o=out.ctypes.data):
        rc = g.L.hpt_denoise_frame(g.h, width, height, c, gbuf, None if p is None else C.byref(p), o)
        rd = g.L.hpt_denoise_frame_dev(g.h, width, height, c, gbuf, None if p is None else C.byref(p), o, None)   # refused before any pointer is used
        assert rc == rd, (rc, rd)
        return rc, g.L.hpt_last_error(g.h).decode()

    def mod(**kw):
        p = DENOISE_PARAMS.from_buffer_copy(bytes(ok))
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    cases = [(dict(c=None), "color"), (dict(gbuf=None), "gbuffer"), (dict(p=None), "params"), (dict(o=None), "out"),
             (dict(width=0), "width"), (dict(height=0), "height"),
             (dict(p=mod(iterations=0)), "iterations"), (dict(p=mod(iterations=9)), "iterations"), (dict(p=mod(normalSquarings=9)), "normalSquarings"),
             (dict(p=mod(sigmaColor=-1.0)), "sigmaColor"), (dict(p=mod(sigmaDepth=float("nan"))), "sigmaDepth"), (dict(p=mod(sigmaAlbedo=float("inf"))), "sigmaAlbedo"),
             (dict(p=mod(normConst=-0.5)), "normConst"), (dict(p=mod(normConst=float("inf"))), "normConst"),
             (dict(p=mod(flags=2)), "flags"), (dict(p=mod(flags=0x80000001)), "flags"),
             (dict(o=color.ctypes.data), "aliases"), (dict(o=color.ctypes.data + 16), "aliases")]
    for kw, word in cases:
        rc, msg = call(**kw)
        assert rc == HPT_ERR_ARG and word in msg and "DenoiseFrame" in msg, (kw, rc, msg)
        assert np.all(out == 7.0), f"out written after a refusal ({word})"
    assert g.L.hpt_denoise_frame(None, 8, 6, color.ctypes.data, gb.ctypes.data, C.byref(ok), out.ctypes.data) == HPT_ERR_ARG
    rc, _ = g.L.hpt_denoise_frame(g.h, 8, 6, color.ctypes.data, gb.ctypes.data, C.byref(ok), out.ctypes.data), None
    assert rc == 0 and not np.all(out == 7.0)
