"""The hand-over between pass slices of the persistent megakernel (csrc/hpt_kernels.hip: pathTraceKernel<.., SLICED>): the lane that finishes a
slice posts the pixel and its generator as five tagged 64-bit words (csrc/hpt_types.h: sliceWordPack) with relaxed atomics, and the lane that
holds the next slice takes them when all five carry its tag - no release, no acquire, no store to the frame before the pixel's last slice.
Frames and generators must equal whole-pixel items (pass_slice 0) bit for bit, for slices of 1, 2, 3 and 5 passes of 8 and of 7 (a short last
slice), where the chains of waiting lanes are longest (far fewer pixels than lanes), where takers are lanes that still hold work (two pixels
per lane), with one channel, with a tid interleave, and in a second call that finds the first call's tags. The words themselves are checked on
the host (tests/cpp/slice_mailbox_test.cpp, built with the address and undefined-behaviour sanitizers)."""
import os
import subprocess

import numpy as np
import pytest

from conftest import scene_path
from hydracore3_amd.scene import load_hydra_xml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SLICES = [1, 2, 3, 5]
PASSES = [8, 7]


def test_tagged_words_round_trip(tmp_path):
    """All-ones, NaN and negative-zero payloads come back bit for bit; a word is taken by the slice after its writer only; tag 0 by none."""
    exe = str(tmp_path / "slice_mailbox_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "cpp", "slice_mailbox_test.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "cases passed" in r.stdout, r.stdout + r.stderr


def _render(sc, slice_, spp, channels=4, calls=1, ranks=0, blocks_per_cu=0):
    """Frame and generators after `calls` PathTraceBlock calls of `spp` passes with pass_slice = slice_; the slices the launches report."""
    from hydracore3_amd.api import HipIntegrator
    from hydracore3_amd.sharding import tid_interleave
    g = HipIntegrator(sc)
    g.set_option("pass_slice", slice_)
    if blocks_per_cu:
        g.set_launch_config(blocks_per_cu)
    img = np.zeros((sc.height, sc.width, channels), np.float32)
    used = []
    for _ in range(calls):
        for r in range(max(ranks, 1)):
            begin, count = 0, g.N
            if ranks:
                begin, count, chunk, stride = tid_interleave(r, ranks, g.N)
                g.set_tid_interleave(chunk, stride)
            g.PathTraceBlock(count, channels, img, spp, tid_begin=begin)     # (a lane that gave up waiting makes this raise: HPT_ERR_STATE)
            used.append(g.last_launch()["pass_slice"])
    assert g.last_launch()["schedule"] == 1, "the test is about the persistent megakernel"
    return img, g.random_gens(), used


SHAPES = {
    # name: (width, height, keyword arguments of _render, launches per render)
    "small_frame": (64, 64, {}, 1),                                  # 4096 pixels on a grid of far more lanes: every slice of a pixel is drawn at once
    "two_pixels_per_lane": (512, 256, {"blocks_per_cu": 1}, 1),      # takers are lanes that have finished one pixel and draw a later slice of another
    "one_channel": (64, 48, {"channels": 1}, 1),
    "interleaved_ranks": (96, 64, {"ranks": 2}, 2),                  # chunk 1024, stride 2: each rank's mailbox records lie between the other's
    "two_calls": (64, 64, {"calls": 2}, 2),                          # the second call must not take a tag the first one left
}
_scenes, _refs = {}, {}


def _scene(shape):
    w, h = SHAPES[shape][:2]
    if (w, h) not in _scenes:
        _scenes[(w, h)] = load_hydra_xml(scene_path("test_035"), w, h)
    return _scenes[(w, h)]


def _reference(shape, spp):
    """Whole-pixel items: rendered once per shape and pass count, shared by the slices."""
    if (shape, spp) not in _refs:
        ref = _render(_scene(shape), 0, spp, **SHAPES[shape][2])
        assert all(u == 0 for u in ref[2])
        for a in ref[:2]:
            a.setflags(write=False)
        _refs[(shape, spp)] = ref
    return _refs[(shape, spp)]


@pytest.mark.gpu
@pytest.mark.parametrize("spp", PASSES)
@pytest.mark.parametrize("slice_", SLICES)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_sliced_frame_and_generators_equal_whole_pixels(shape, slice_, spp):
    ref = _reference(shape, spp)
    got = _render(_scene(shape), slice_, spp, **SHAPES[shape][2])
    what = f"{shape}, slice {slice_} of {spp} passes"
    assert got[2] == [slice_] * SHAPES[shape][3], f"{what}: the launches report slices {got[2]}"
    assert np.isfinite(got[0]).all() and got[0][..., :3].mean() > 0, what
    assert np.array_equal(got[0].view(np.uint32), ref[0].view(np.uint32)), f"{what}: the frame differs from pass_slice 0"
    assert np.array_equal(got[1], ref[1]), f"{what}: the generators differ from pass_slice 0"


@pytest.mark.gpu
def test_second_call_with_other_slices_ignores_the_first_calls_tags():
    """Slice 1 of 8 passes leaves tags 1 ... 7 behind; the next call on the context, slice 3 of 7 passes, waits for tags 1 and 2."""
    from hydracore3_amd.api import HipIntegrator
    sc = _scene("small_frame")
    out = []
    for slices in ((0, 0), (1, 3)):
        g = HipIntegrator(sc)
        img = np.zeros((sc.height, sc.width, 4), np.float32)
        for s, spp in zip(slices, (8, 7)):
            g.set_option("pass_slice", s)
            g.PathTraceBlock(g.N, 4, img, spp)
            assert g.last_launch()["pass_slice"] == s
        out.append((img, g.random_gens()))
    assert np.array_equal(out[0][0].view(np.uint32), out[1][0].view(np.uint32)), "the frame differs from pass_slice 0"
    assert np.array_equal(out[0][1], out[1][1]), "the generators differ from pass_slice 0"
