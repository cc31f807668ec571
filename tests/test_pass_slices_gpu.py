"""Pass slices of the persistent megakernel (hpt_set_option("pass_slice", n); csrc/hpt_kernels.hip, csrc/hpt_types.h: passSliceItem): a pixel
handed out in work items of n passes must give the frame and the generator states of whole-pixel items (pass_slice 0) bit for bit - the
passes of a pixel run in the same order from the same generator, and its value is summed in the same order. The item arithmetic is checked
on the host (tests/cpp/pass_slice_items_test.cpp, built with the address and undefined-behaviour sanitizers)."""
import os
import subprocess

import numpy as np
import pytest

from conftest import scene_path
from hydracore3_amd.scene import load_hydra_xml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pass_slice_items_cover_every_pass_once(tmp_path):
    """passNum in {1, 7, 8, 1024} x slice in {0, 1, 2, 3, 8, 2000}, contiguous windows and tid interleaves: every (tid, pass) exactly once, a
    tid's slices in ascending item order, an item's predecessor at a smaller item index."""
    exe = str(tmp_path / "pass_slice_items_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "cpp", "pass_slice_items_test.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "cases passed" in r.stdout, r.stdout + r.stderr


def _render(sc, slice_, spp, channels=4, calls=1, ranks=0):
    """Frame and generators after `calls` PathTraceBlock calls of `spp` passes with pass_slice = slice_; the slice the last launch reports."""
    from hydracore3_amd.api import HipIntegrator
    from hydracore3_amd.sharding import tid_interleave
    g = HipIntegrator(sc)
    g.set_option("pass_slice", slice_)
    img = np.zeros((sc.height, sc.width, channels), np.float32)
    used = []
    for _ in range(calls):
        if ranks:
            for r in range(ranks):
                begin, count, chunk, stride = tid_interleave(r, ranks, g.N)
                g.set_tid_interleave(chunk, stride)
                g.PathTraceBlock(count, channels, img, spp, tid_begin=begin)
                used.append(g.last_launch()["pass_slice"])
        else:
            g.PathTraceBlock(g.N, channels, img, spp)
            used.append(g.last_launch()["pass_slice"])
    assert g.last_launch()["schedule"] == 1, "the test is about the persistent megakernel"
    return img, g.random_gens(), used


def _same(a, b, what):
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)), f"{what}: the frame differs from pass_slice 0"
    assert np.array_equal(a[1], b[1]), f"{what}: the generators differ from pass_slice 0"
    assert a[0][..., :3].mean() > 0


@pytest.fixture(scope="module")
def cornell64():
    sc = load_hydra_xml(scene_path("test_035"), 64, 64)
    return sc, {ch: _render(sc, 0, 7, channels=ch) for ch in (1, 4)}


@pytest.mark.gpu
@pytest.mark.parametrize("channels", [1, 4])
@pytest.mark.parametrize("slice_", [1, 2, 8])
def test_slices_of_a_small_frame_wait_for_each_other(cornell64, slice_, channels):
    """64 x 64 at 7 spp: with slices 1 and 2 (uneven last slice) there are fewer items than lanes, every slice of a pixel is drawn at once and all
    but the first wait for their predecessors; slice 8 >= the passes is the whole pixel again."""
    sc, ref = cornell64
    got = _render(sc, slice_, 7, channels=channels)
    _same(got, ref[channels], f"slice {slice_}, {channels} channel(s)")
    assert got[2] == [slice_ if slice_ < 7 else 0] and ref[channels][2] == [0]


@pytest.mark.gpu
def test_more_pixels_than_lanes_and_a_second_call():
    """640 x 512 at 4 spp, slice 1: more pixels than lanes, so a predecessor has usually finished before its successor is drawn; two calls,
    the second onto the non-zero frame and from the generators the first left."""
    sc = load_hydra_xml(scene_path("test_035"), 640, 512)
    ref, got = _render(sc, 0, 4, calls=2), _render(sc, 1, 4, calls=2)
    _same(got, ref, "640 x 512, slice 1, two calls")
    assert got[2] == [1, 1]


@pytest.mark.gpu
def test_tid_interleave_ranks_sum_to_the_frame():
    """Chunk 1024, stride 2 on 96 x 64 (six chunks: three per rank): both ranks rendered into one frame with slice 2 of 5 passes."""
    sc = load_hydra_xml(scene_path("test_035"), 96, 64)
    ref, got = _render(sc, 0, 5), _render(sc, 2, 5, ranks=2)
    _same(got, ref, "interleaved ranks")
    assert got[2] == [2, 2]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["typed_materials", "legacy_materials"])
def test_kernels_with_every_bsdf_branch_and_moving_instances(name):
    """typed_materials runs the instantiation with every BSDF branch, legacy_materials (a moving instance) the motion one."""
    sc = load_hydra_xml(scene_path(name), 64, 48)
    assert name != "legacy_materials" or sc.inst_motion
    ref, got = _render(sc, 0, 6), _render(sc, 2, 6)
    _same(got, ref, name)
    assert got[2] == [2]


@pytest.mark.gpu
def test_dr_and_input_rays_keep_whole_pixels():
    """PathTraceDR and PathTraceFromInputRays ignore the option: the launch reports slice 0."""
    from hydracore3_amd.api import HipIntegrator
    sc = load_hydra_xml(scene_path("test_035"), 32, 32)
    g = HipIntegrator(sc)
    g.set_option("pass_slice", 2)
    img = np.zeros((sc.height, sc.width, 4), np.float32)
    g.PathTraceBlock(g.N, 4, img, 4)
    assert g.last_launch()["pass_slice"] == 2
    off, size = g.PutDiffTex2D(1, 256, 256, 4)
    data = np.full(size, 0.5, np.float32)
    g.PathTraceDR(g.N, 4, img, 4, np.zeros_like(img), data, np.zeros_like(data))
    assert g.last_launch()["pass_slice"] == 0
    g.PathTraceBlock(g.N, 4, img, 4)
    assert g.last_launch()["pass_slice"] == 2
    pos = np.zeros((g.N, 4), np.float32)
    dirs = np.zeros((g.N, 4), np.float32); dirs[:, 2] = -1.0
    g.PathTraceFromInputRaysBlock(g.N, 4, pos, dirs, np.zeros((g.N, 4), np.float32), 4)
    assert g.last_launch()["pass_slice"] == 0
