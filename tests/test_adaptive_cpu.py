"""Adaptive sampling without a GPU: the surface of the new entry points (declared, bound, exported, null-safe), the record layouts against the
header, and the numpy restatement (tests/adaptive_reference.py) against records whose answers are worked out by hand below."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import adaptive_reference as R
from conftest import ROOT

SYMBOLS = ["hpt_path_trace_block_counts", "hpt_path_trace_block_counts_dev", "hpt_adaptive_plan", "hpt_adaptive_plan_dev", "hpt_adaptive_resolve",
           "hpt_adaptive_resolve_dev", "hpt_path_trace_block_adaptive", "hpt_path_trace_block_adaptive_dev"]
HDR = os.path.join(ROOT, "include", "hydra_hip.h")


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
    # a null context: HPT_ERR_ARG, and nothing is written through any pointer (each points at a canary)
    canary = np.full(64, 0xA5A5A5A5, np.uint32)
    args = []
    for i, t in enumerate(api.ABI[name][1]):
        if i == 0:
            args.append(None)
        elif t is C.c_void_p:
            args.append(canary.ctypes.data)
        else:
            args.append(1)
    assert getattr(lib, name)(*args) == 1
    assert (canary == 0xA5A5A5A5).all()


def test_record_layouts_match_the_header():
    from hydracore3_amd import api
    hdr = _header()

    def fields(struct):
        body = re.search(r"typedef struct " + struct + r"\s*\{(.*?)\}", hdr, flags=re.S).group(1)
        return [(t, n) for t, n in re.findall(r"(float|uint32_t|uint64_t)\s+(\w+)\s*;", body)]

    np_of = {"float": np.float32, "uint32_t": np.uint32, "uint64_t": np.uint64}
    for struct, dt, size in (("hpt_pixel_moments", api.MOMENTS_DTYPE, 16), ("hpt_adaptive_info", api.ADAPTIVE_INFO_DTYPE, 32)):
        f = fields(struct)
        assert [n for _, n in f] == list(dt.names) and [np.dtype(np_of[t]) for t, _ in f] == [dt[n] for n in dt.names], (struct, f)
        assert dt.itemsize == size and dt.isalignedstruct is False and sum(dt[n].itemsize for n in dt.names) == size     # no padding
    assert api.MOMENTS_DTYPE == R.MOMENTS_DTYPE
    f = fields("hpt_adaptive_params")
    assert [(n, t) for t, n in f] == [(n, {C.c_float: "float", C.c_uint32: "uint32_t"}[t]) for n, t in api.ADAPTIVE_PARAMS._fields_]
    assert C.sizeof(api.ADAPTIVE_PARAMS) == 24


def test_luminance_and_moments_bookkeeping():
    # exactly representable values: y = (0.2126f * 2 + 0.7152f * 4) + 0.0722f * 8 with every step rounded to f32, worked out in float64 here
    f = np.float32
    a = f(np.float64(f(0.2126)) * 2.0); b = f(np.float64(f(0.7152)) * 4.0); c = f(np.float64(f(0.0722)) * 8.0)
    want = f(np.float64(f(np.float64(a) + np.float64(b))) + np.float64(c))
    assert R.luminance(np.array([[2.0, 4.0, 8.0]], f))[0] == want
    assert np.isnan(R.luminance(np.array([[np.nan, 1.0, 1.0]], f))[0]) and np.isposinf(R.luminance(np.array([[np.inf, 1.0, 1.0]], f))[0])
    m = R.accumulate(np.zeros(2, R.MOMENTS_DTYPE), [(np.array([1.0, 2.0], f), np.array([True, True])), (np.array([3.0, 5.0], f), np.array([True, False])),
                                                     (np.array([np.inf, 0.5], f), np.array([False, True]))])
    assert m["sumY"].tolist() == [4.0, 2.5] and m["sumY2"].tolist() == [10.0, 4.25] and m["passes"].tolist() == [2, 2] and not m["reserved"].any()


def _total(rec, tol=0.5, lum_floor=0.5, min_passes=2):
    m = np.zeros(1, R.MOMENTS_DTYPE)
    m[0] = (np.float32(rec[0]), np.float32(rec[1]), rec[2], 0)
    t, bad = R.total_passes(m, tol, lum_floor, min_passes)
    return int(t[0]), bool(bad[0])


def test_total_passes_on_hand_computed_records():
    assert _total((123.0, 456.0, 0)) == (2, False)                         # no passes: minPasses, whatever the sums hold
    # 3 - 2^-22 over 3 rounds to 1 - 2^-24, the mean is 1: the variance comes out as -2^-24 and is clamped to 0
    assert np.float32(np.float32(2.9999998) / np.float32(3.0)) - np.float32(1.0) < 0 and _total((3.0, 2.9999998, 3)) == (2, False)
    assert _total((np.nan, 1.0, 5)) == (5, True) and _total((1.0, np.inf, 6)) == (6, True) and _total((-np.inf, 1.0, 2)) == (2, True)
    assert _total((np.nan, np.nan, 0)) == (2, False)                       # (a record without passes is never counted as non-finite)
    # mean 0, variance 1e12, den = 0.5 * 0.5: tf = 1.6e13 >= 2^31
    assert _total((0.0, 2e12, 2)) == (0x7FFFFFFF, False)
    assert _total((0.0, float(2.0 ** 31) * 0.0625 * 2, 2)) == (0x7FFFFFFF, False)      # tf = 2^31 exactly
    assert _total((0.0, float(2.0 ** 30) * 0.0625 * 2, 2)) == (1 << 30, False)         # tf = 2^30: still converted
    # den = 1e-15 * 1e-15 = 1e-30 is a normal f32, den * den underflows to 0: 0 / 0 counts as 0, v / 0 as "more than can be counted"
    assert np.float32(1e-30) * np.float32(1e-30) == 0
    assert _total((0.0, 0.0, 3), tol=1e-15, lum_floor=1e-15) == (2, False)
    assert _total((0.0, 3.0, 3), tol=1e-15, lum_floor=1e-15) == (0x7FFFFFFF, False)
    # samples {1, 3, 1, 3}: mean 2, variance 1, den = 0.5 * 2.5 = 1.25, tf = 0.64 -> 1, below minPasses
    assert _total((8.0, 20.0, 4)) == (2, False) and _total((8.0, 20.0, 4), min_passes=10) == (10, False)
    # mean 2, variance 5: tf = 5 / 1.5625 = 3.2 -> 4; at tol 0.125: den = 0.3125, tf = 51.2 -> 52
    assert _total((8.0, 36.0, 4)) == (4, False) and _total((8.0, 36.0, 4), tol=0.125) == (52, False)


def test_plan_clips_to_the_pass_limit_and_to_step():
    xy = R.packed_xy(4, 1, 1)
    m = np.zeros(4, R.MOMENTS_DTYPE)
    m[0] = (8.0, 36.0, 4, 0)          # asks for 52 in all: 48 more
    m[1] = (100.0, 300.0, 50, 0)      # already past maxPasses
    m[2] = (8.0, 20.0, 4, 0)          # mean 2, variance 1, den = 0.125 * 2.5: tf = 10.24 -> 11 in all, 7 more
    m[3] = (np.nan, 0.0, 9, 0)        # not finite: keeps its 9
    kw = dict(tol=0.125, lum_floor=0.5, min_passes=2)
    assert R.need_image(m, xy, 0, 4, 4, 1, **kw).tolist() == [48, 0, 7, 0]
    c, info = R.plan(m, xy, 0, 4, 4, 1, max_passes=1000, step=1000, dilate=0, **kw)
    assert c.tolist() == [48, 0, 7, 0] and info == {"passes": 55, "pixels": 2, "maxPasses": 50, "nonfinite": 1}
    assert R.plan(m, xy, 0, 4, 4, 1, max_passes=40, step=1000, dilate=0, **kw)[0].tolist() == [36, 0, 7, 0]      # 40 - 4
    assert R.plan(m, xy, 0, 4, 4, 1, max_passes=40, step=16, dilate=0, **kw)[0].tolist() == [16, 0, 7, 0]
    # dilated: pixel 1 sees 48 but sits at 50 passes and has no room; pixel 3 takes its neighbour's 7
    assert R.plan(m, xy, 0, 4, 4, 1, max_passes=40, step=16, dilate=1, **kw)[0].tolist() == [16, 0, 7, 7]
    m[1]["passes"] = 30               # room for 10
    assert R.plan(m, xy, 0, 4, 4, 1, max_passes=40, step=16, dilate=1, **kw)[0].tolist() == [16, 10, 7, 7]
    # a window: pixel 0 lies outside it, reads 0 in the need image and gets no count; pixel 1 is left with its right-hand neighbour's 7
    assert R.plan(m, xy, 1, 3, 4, 1, max_passes=40, step=16, dilate=1, **kw)[0].tolist() == [0, 7, 7, 7]


def test_dilation_at_the_corners_and_across_a_tile_seam():
    w, h, tile = 16, 8, 8
    xy = R.packed_xy(w, h, tile)
    assert xy[63] == (7 << 16 | 7) and xy[64] == 8 and xy[7] == 7 and xy[8] == (1 << 16)           # tid order is not pixel order
    tid_of = {(int(v) & 0xFFFF, int(v) >> 16): t for t, v in enumerate(xy)}
    kw = dict(tol=0.125, lum_floor=0.5, min_passes=1, max_passes=1 << 20, step=1 << 20)

    def counts_for(needy):
        m = np.zeros(w * h, R.MOMENTS_DTYPE)
        m[:] = (5.0, 25.0, 1, 0)                                           # one sample of 5: variance 0, asks for minPasses = what it has
        for p in needy:
            m[tid_of[p]] = (8.0, 36.0, 4, 0)                               # 48 more
        c, info = R.plan(m, xy, 0, w * h, w, h, dilate=1, **kw)
        return {p for p in tid_of if c[tid_of[p]] == 48}, c, info

    for corner, want in (((0, 0), {(0, 0), (1, 0), (0, 1), (1, 1)}), ((15, 0), {(15, 0), (14, 0), (15, 1), (14, 1)}),
                         ((0, 7), {(0, 7), (1, 7), (0, 6), (1, 6)}), ((15, 7), {(15, 7), (14, 7), (15, 6), (14, 6)})):
        got, c, info = counts_for([corner])
        assert got == want and info["pixels"] == 4 and int(c.sum()) == 4 * 48
    # (7, 3) is the last column of tile 0: its right-hand neighbours (8, 2..4) live 40 and more tids away, in tile 1
    got, c, _ = counts_for([(7, 3)])
    assert got == {(x, y) for x in (6, 7, 8) for y in (2, 3, 4)}
    assert abs(tid_of[(8, 3)] - tid_of[(7, 3)]) > 8
    c0, _ = R.plan(np.zeros(w * h, R.MOMENTS_DTYPE), xy, 0, w * h, w, h, dilate=0, **kw)
    assert (c0 == 1).all()                                                 # records without passes: minPasses everywhere


def test_resolve_divides_three_channels_and_copies_the_fourth():
    xy = R.packed_xy(2, 2, 1)
    m = np.zeros(4, R.MOMENTS_DTYPE)
    m["passes"] = [4, 0, 3, 1]
    frame = np.arange(1, 17, dtype=np.float32)
    out = R.resolve(frame, m, xy, 0, 4, 2, 4)
    assert out.tolist()[:8] == [0.25, 0.5, 0.75, 4.0, 0.0, 0.0, 0.0, 8.0]
    assert out[8] == np.float32(9.0) / np.float32(3.0) and out[11] == 12.0 and out.tolist()[12:] == [13.0, 14.0, 15.0, 16.0]
    assert R.resolve(frame[:4], m, xy, 0, 4, 2, 1).tolist() == [0.25, 0.0, 1.0, 4.0]
    keep = np.full(16, -1.0, np.float32)
    assert R.resolve(frame, m, xy, 2, 1, 2, 4, out=keep).tolist()[:8] == [-1.0] * 8                 # outside the window: untouched


def test_step_default_of_the_python_front_end():
    """`step` defaults to the value chosen from the sweep in profiles/adaptive.md (one scene); every other parameter is the caller's."""
    from hydracore3_amd import api
    p = api.HipIntegrator._adaptive_params(tol=0.1, lum_floor=0.01, min_passes=4, max_passes=64)
    assert p.step == api.ADAPTIVE_STEP_DEFAULT == 256 and p.dilate == 0 and (p.minPasses, p.maxPasses) == (4, 64)
    assert api.HipIntegrator._adaptive_params(tol=0.1, lum_floor=0.01, min_passes=4, max_passes=64, step=7).step == 7
    with pytest.raises(KeyError):
        api.HipIntegrator._adaptive_params(lum_floor=0.01, min_passes=4, max_passes=64)
