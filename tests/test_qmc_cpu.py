"""The Niederreiter sampler of the QMC integrator, without a GPU: the table hpt_qmc_table builds against the numbers the reference's own
program printed (tests/golden/qmc/niederreiter_11x31.json), the numpy rndFloat of tests/qmc_reference.py against the recorded bit patterns,
hpt_qmc_layout against EnableQMC's eight layouts, the (0, 2)-sequence property of dimensions 0 and 1, the sample-count cap, the exports."""
import os
import re
import subprocess

import numpy as np
import pytest

import qmc_reference as Q
from conftest import ROOT


def test_table_equals_the_words_the_reference_printed():
    from hydracore3_amd import api
    table, _ = Q.load_fixture()
    got = api.qmc_table()
    assert got.shape == (11, 31) and got.dtype == np.uint32
    assert np.array_equal(got, table), np.argwhere(got != table)[:8]
    # what the issue states about the first three dimensions
    assert [hex(v) for v in table[0, :4]] == ["0x40000000", "0x20000000", "0x10000000", "0x8000000"]
    assert [hex(v) for v in table[1, :4]] == ["0x40000000", "0x60000000", "0x50000000", "0x78000000"]
    assert [hex(v) for v in table[2, :4]] == ["0x60000000", "0x48000000", "0x38000000", "0x7a000000"]
    assert int(table.max()) < 2 ** 31


def test_numpy_rnd_float_equals_the_recorded_bit_patterns():
    table, rec = Q.load_fixture()
    assert len(rec) >= 300
    for p in (0, 1, 2 ** 31 - 1, 2 ** 32 - 1):
        assert p in set(rec[:, 0].tolist())
    for dim in range(Q.DIMENSIONS):
        sel = rec[rec[:, 1] == dim]
        got = Q.rnd_float(table, sel[:, 0].astype(np.uint32), dim).view(np.uint32)
        assert np.array_equal(got, sel[:, 2].astype(np.uint32)), (dim, sel[got != sel[:, 2].astype(np.uint32)][:4])
    # pos = 0 gives 2^-31; bit 31 of pos selects nothing; all 31 bits set in dimension 0 give exactly 1.0
    assert Q.rnd_float(table, 0, 0)[0] == np.float32(2.0 ** -31)
    assert Q.rnd_float(table, 0x80000000, 5)[0] == Q.rnd_float(table, 0, 5)[0]
    assert Q.rnd_float(table, 0x7FFFFFFF, 0)[0] == np.float32(1.0)


def test_layout_equals_enable_qmc_for_all_eight_feature_sets():
    from hydracore3_amd import api
    names = ("dof", "spd", "motion", "mat", "lgt")
    for (dof, spd, motion), want in Q.LAYOUTS.items():
        got = api.qmc_layout(dof, spd, motion)
        assert tuple(got[n] for n in names) == want, ((dof, spd, motion), got)
    assert len(Q.LAYOUTS) == 8
    full = api.qmc_layout(True, True, True)
    assert full["mat"] == 0 and full["lgt"] == 0                       # the layout that leaves the first bounce to the pseudo generator


@pytest.mark.parametrize("w,h,spp", [(32, 32, 2), (128, 64, 8), (64, 64, 4)])
def test_power_of_two_frames_get_exactly_spp_samples_per_pixel(w, h, spp):
    """Dimensions 0 and 1 form a (0, 2)-sequence: with W, H and spp powers of two, every W*H*spp consecutive samples put spp in each pixel
    (64 x 64 x 4 is the size checked against the reference's binary: minimum 4, maximum 4)."""
    table, _ = Q.load_fixture()
    _, _, pix = Q.sample_pixels(table, w * h * spp, w, h)
    counts = np.bincount(pix, minlength=w * h)
    assert counts.min() == spp and counts.max() == spp


def test_non_power_of_two_window_and_the_clamp_at_one():
    """A 48 x 20 window: the counts are those of the restatement written out sample by sample in Python integers and floats of 24 bits, and
    they sum to S; the sample index with all 31 bits set gives u0 = 1.0, whose pixel is clamped into the last column."""
    table, _ = Q.load_fixture()
    w, h, spp = 48, 20, 3
    S = w * h * spp
    x, y, pix = Q.sample_pixels(table, S, w, h)
    counts = np.bincount(pix, minlength=w * h)
    want = np.zeros(w * h, np.int64)
    for s in range(S):                                                  # the same numbers, one sample at a time, exact rational arithmetic
        r0 = r1 = 0
        for bit in range(31):
            if (s >> bit) & 1:
                r0 ^= int(table[0, bit]); r1 ^= int(table[1, bit])
        u0 = float(np.float32(r0 + 1)) / 2.0 ** 31
        u1 = float(np.float32(r1 + 1)) / 2.0 ** 31
        px = min(int(float(np.float32(np.float32(u0) * np.float32(w)))), w - 1)
        py = min(int(float(np.float32(np.float32(u1) * np.float32(h)))), h - 1)
        want[py * w + px] += 1
    assert np.array_equal(counts, want) and counts.sum() == S
    xs, ys, _ = Q.sample_pixels(table, np.array([0x7FFFFFFF], np.uint32), w, h)
    assert Q.rnd_float(table, 0x7FFFFFFF, 0)[0] == np.float32(1.0) and int(xs[0]) == w - 1 and int(ys[0]) < h
    xs2, _, _ = Q.sample_pixels(table, np.array([0xFFFFFFFF], np.uint32), w, h)
    assert int(xs2[0]) == w - 1


def test_sample_count_is_capped_at_two_to_the_32_minus_one():
    from hydracore3_amd import api
    assert api.qmc_sample_count(64 * 64, 4) == 64 * 64 * 4
    assert api.qmc_sample_count(0, 7) == 0 and api.qmc_sample_count(7, 0) == 0
    assert api.qmc_sample_count(65536, 65535) == 65536 * 65535
    assert api.qmc_sample_count(65536, 65536) == 2 ** 32 - 1
    assert api.qmc_sample_count(1920 * 1080, 4096) == 2 ** 32 - 1
    assert api.qmc_sample_count(2 ** 32 - 1, 2 ** 32 - 1) == 2 ** 32 - 1


def test_the_new_symbols_are_declared_bound_and_exported():
    from hydracore3_amd import api
    names = {"hpt_qmc_table", "hpt_qmc_layout", "hpt_qmc_sample_count", "hpt_path_trace_qmc_block", "hpt_path_trace_qmc_block_dev"}
    hdr = open(os.path.join(ROOT, "include", "hydra_hip.h")).read()
    assert names <= set(re.findall(r"\b(hpt_[a-z0-9_]+)\s*\(", hdr)) and names <= set(api.ABI)
    lib = api.load_library()
    nm = subprocess.run(["nm", "-D", "--defined-only", api.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (hpt_[a-z0-9_]+)", nm))
    for n in names:
        assert hasattr(lib, n) and n in exported
    assert hasattr(api.HipIntegrator, "PathTraceBlockQMC")
    # a null output is an argument error, not a crash; neither function needs a context
    assert lib.hpt_qmc_table(None) == 1 and lib.hpt_qmc_layout(0, 0, 0, None) == 1
