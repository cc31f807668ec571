"""Treelet restructuring of device-built trees (hpt_set_option("device_build_quality", passes)) without a GPU: the subset recurrence restated in
numpy (tests/treelet_reference.py) against the enumeration of every topology, the header's scalar form (csrc/treelet_opt.h, built with the
address and undefined-behaviour sanitizers as a stand-alone program) against the same enumeration and against the numpy form partition by
partition, and the ABI surface of hpt_get_build_info and of the option."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import treelet_reference as TR
from conftest import ROOT

f32 = np.float32


# ---- 1. the recurrence against enumeration ----------------------------------------------------------------------------------------------------
def _boxes(kind, k, rng):
    c = rng.uniform(0, 10, (k, 3)); e = rng.uniform(0, 3, (k, 3))
    if kind == "coincident":
        c[:] = c[0]; e[:] = e[0]
    elif kind == "points":
        c[:] = 1.5; e[:] = 0.0
    elif kind == "flat":
        e[np.arange(k), np.where(np.arange(k) % 2, 1, 2)] = 0.0
    elif kind == "pairs":
        c[1::2] = c[0:2 * (k // 2):2]; e[1::2] = e[0:2 * (k // 2):2]
    elif kind == "outlier":
        c = rng.uniform(0, 1, (k, 3)); e = rng.uniform(0, 0.5, (k, 3)); c[k // 2] += 1.0e4
    lo = c.astype(f32)
    return np.concatenate([lo, (lo + e.astype(f32)).astype(f32)], axis=1)


@pytest.mark.parametrize("k", [2, 3, 4, 5, 6, 7])
def test_recurrence_equals_the_minimum_over_every_topology(k):
    """k leaf boxes, random and degenerate: the recurrence's optimum is, bit for bit, the least cost among all (2k - 3)!! topologies (10 395 at
    k = 7), each summed by the recurrence's own formula, and the topology its partitions describe costs exactly that."""
    rng = np.random.default_rng(100 + k)
    for kind in ("random", "random", "coincident", "points", "flat", "pairs", "outlier"):
        boxes = _boxes(kind, k, rng)
        area, cost, part = TR.optimize(boxes)
        full = (1 << k) - 1
        costs = TR.enumerated_costs(area, k)
        assert costs.size == TR.topology_count(k) == {2: 1, 3: 3, 4: 15, 5: 105, 6: 945, 7: 10395}[k]
        assert costs.min() == cost[full], (kind, costs.min(), cost[full])
        got, mask = TR.topology_cost(area, TR.topology(part, full))
        assert mask == full and got == cost[full], (kind, got, cost[full])
        if kind == "points":
            assert cost[full] == 0.0
        # every split ties exactly (all sums are 0, or multiples of one area that are the same float up to five leaves, whichever way they are
        # associated): the lowest mask, i.e. the lowest leaf alone, wins
        if kind == "points" or (kind == "coincident" and k <= 5):
            assert all(int(part[s]) == (s & -s) for s in range(1, full + 1) if s & (s - 1))
        if kind == "random" and k >= 4:
            assert np.unique(costs).size > 1                                   # (the optimum is a choice)


# ---- 2. the header's scalar form ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def header_cases(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("treelet") / "treelet_opt_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "cpp", "treelet_opt_test.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "cases passed" in r.stdout and "FAILED" not in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    cases = re.findall(r"^case (\w+) k=(\d) boxes=([0-9a-f,]+) parts=([0-9a-f]+) cost=([0-9a-f]{8}) topologies=(\d+)$", r.stdout, re.M)
    return cases


def test_header_equals_enumeration_under_the_sanitizers(header_cases):
    """The program itself compares treeletOptimize with its own enumeration of every topology (it fails otherwise); every k and every kind ran."""
    assert len(header_cases) == 6 * 8
    assert {int(k) for _, k, *_ in header_cases} == {2, 3, 4, 5, 6, 7}
    assert {kind for kind, *_ in header_cases} == {"random", "coincident", "points", "flat", "pairs", "outlier"}
    for _, k, _, _, _, count in header_cases:
        assert int(count) == TR.topology_count(int(k))


def test_header_and_numpy_choose_the_same_partitions(header_cases):
    """On the boxes the program printed: the numpy form chooses the partition the header chose for EVERY subset (the tie rule included: the
    coincident and paired boxes tie) and reaches the same optimum bit for bit."""
    ties = 0
    for kind, k, boxes, parts, cost, _ in header_cases:
        k = int(k)
        b = np.array([int(w, 16) for w in boxes.split(",")], np.uint32).view(f32).reshape(k, 6)
        want = np.array([int(parts[2 * j:2 * j + 2], 16) for j in range(len(parts) // 2)], np.uint8)
        area, c, part = TR.optimize(b)
        assert want.size == (1 << k) - 1
        assert np.array_equal(part[1:], want), (kind, k, part[1:], want)
        assert c[(1 << k) - 1].view(np.uint32) == int(cost, 16), (kind, k)
        ties += kind in ("coincident", "pairs", "points")
    assert ties == 18


# ---- 3. ABI ------------------------------------------------------------------------------------------------------------------------------------------
def test_header_declares_build_info_and_the_front_end_binds_it():
    from hydracore3_amd import api
    hdr = open(os.path.join(ROOT, "include", "hydra_hip.h")).read()
    m = re.search(r"\bint\s+hpt_get_build_info\s*\(([^)]*)\)\s*;", hdr)
    assert m, "hpt_get_build_info is not declared in include/hydra_hip.h"
    assert "hpt_get_build_info" in api.ABI and len(api.ABI["hpt_get_build_info"][1]) == len(m.group(1).split(",")) == 2
    assert hasattr(api.HipIntegrator, "build_info")
    assert '"device_build_quality"' in hdr, "the option is not documented in include/hydra_hip.h"


def test_library_exports_build_info_and_refuses_null_handles():
    from hydracore3_amd import api
    lib = api.load_library()
    nm = subprocess.run(["nm", "-D", "--defined-only", api.LIB_PATH], capture_output=True, text=True).stdout
    assert "hpt_get_build_info" in set(re.findall(r" T (hpt_[a-z0-9_]+)", nm))
    buf = (C.c_float * 4)(7.0, 7.0, 7.0, 7.0)
    assert lib.hpt_get_build_info(None, buf) == 1                                   # HPT_ERR_ARG, no device touched
    assert list(buf) == [7.0] * 4
    # the option's checks that need no context: a null handle, a null name and a negative value are argument errors before the name is read
    assert lib.hpt_set_option(None, b"device_build_quality", 1) == 1
    assert lib.hpt_set_option(None, b"device_build_quality", 5) == 1
    assert lib.hpt_set_option(None, b"device_build_quality", -1) == 1
    src = open(os.path.join(ROOT, "hydracore3_amd", "csrc", "hpt_host.hip")).read()
    m = re.search(r'k == "device_build_quality"\) \{ if \(value > (\d+)\) return c->fail\(HPT_ERR_ARG, "device_build_quality: ([^"]+)"\)', src)
    assert m and int(m.group(1)) == 4 and "0" in m.group(2) and "1..4" in m.group(2)
