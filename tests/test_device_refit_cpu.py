"""The refit of device-built trees without a GPU: the ABI surface of hpt_get_refit_info and hpt_read_accel (declared, bound, exported, null-safe)
and the numpy reader of the read-back tree (tests/accel_reference.py) on a hand-built three-node tree with known numbers."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import accel_reference as AR
from conftest import ROOT

SYMBOLS = ["hpt_get_refit_info", "hpt_read_accel"]


# ---- 1. ABI ---------------------------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_refit_symbols_and_the_front_end_binds_them():
    from hydracore3_amd import api
    hdr = open(os.path.join(ROOT, "include", "hydra_hip.h")).read()
    for name in SYMBOLS:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
        assert m, f"{name} is not declared in include/hydra_hip.h"
        assert name in api.ABI, f"{name} is not in api.ABI"
        assert len(api.ABI[name][1]) == len(m.group(1).split(",")), (name, m.group(1))
    assert len(api.ABI["hpt_get_refit_info"][1]) == 2 and len(api.ABI["hpt_read_accel"][1]) == 6
    for meth in ("refit_info", "read_accel", "UpdateGeom_Triangles3f"):
        assert hasattr(api.HipIntegrator, meth)
    for opt in ('"device_refit"', '"refit_max_sah_pct"'):
        assert opt in hdr, f"{opt} is not documented in include/hydra_hip.h"
    assert api.BVH_NODE_DTYPE == AR.NODE_DTYPE and api.BVH_TRI_DTYPE == AR.TRI_DTYPE


def test_library_exports_the_refit_symbols_and_null_handles_are_refused():
    from hydracore3_amd import api
    lib = api.load_library()
    nm = subprocess.run(["nm", "-D", "--defined-only", api.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (hpt_[a-z0-9_]+)", nm))
    assert set(SYMBOLS) <= exported
    buf = (C.c_float * 4)()
    nbytes, root = C.c_uint64(7), C.c_uint32(7)
    assert lib.hpt_get_refit_info(None, buf) == 1                                 # HPT_ERR_ARG, no device touched
    assert lib.hpt_read_accel(None, 0, None, 0, C.byref(nbytes), C.byref(root)) == 1
    assert lib.hpt_read_accel(None, 1, buf, 16, None, None) == 1
    assert nbytes.value == 7 and root.value == 7


# ---- 2. the reader on a tree with known numbers ---------------------------------------------------------------------------------------------------
def _box(lo, hi):
    return [lo[0], hi[0], lo[1], hi[1], lo[2], hi[2]]


def _leaf(first, count):
    return AR.REF_LEAF | (count << 28) | first


def _tree():
    """Root 0 over nodes 1 and 2. Node 1: box [0,1] x [0,2] x [0,3] (half-area 1*2 + 2*3 + 3*1 = 11), leaves of records {0, 1} and {2}.
    Node 2: box [2,4] x [0,1] x [0,1] (half-area 2*1 + 1*1 + 1*2 = 5), leaves of records {3, 4} and {5}. The root's box is their union
    [0,4] x [0,2] x [0,3]: half-area 4*2 + 2*3 + 3*4 = 26. The estimate: 1 + (11 + 5) / 26."""
    nodes = np.zeros(4, AR.NODE_DTYPE)                                             # (entry 3 is unused, as in a device-built array)
    nodes[0] = (_box((0, 0, 0), (1, 2, 3)) + _box((2, 0, 0), (4, 1, 1)), 1, 2, 0, 0)
    nodes[1] = (_box((0, 0, 0), (1, 1, 3)) + _box((0, 1, 0), (1, 2, 1)), _leaf(0, 2), _leaf(2, 1), 0, 0)
    nodes[2] = (_box((2, 0, 0), (3, 1, 1)) + _box((3, 0, 0), (4, 1, 1)), _leaf(3, 2), _leaf(5, 1), 0, 0)
    nodes[3] = ([9] * 12, 77, 78, 0, 0)
    verts = np.array([[[0, 0, 0], [1, 0, 0], [0, 1, 3]], [[1, 1, 1], [0, 0, 2], [1, 0, 3]], [[0, 1, 0], [1, 2, 1], [0, 2, 0]],
                      [[2, 0, 0], [3, 1, 1], [2, 1, 0]], [[3, 0, 1], [2, 0, 1], [3, 1, 0]], [[3, 0, 0], [4, 1, 1], [4, 0, 0]]], np.float64)
    return nodes, verts


def test_reader_on_a_hand_built_tree():
    nodes, verts = _tree()
    assert AR.reachable(nodes, 0) in ([0, 1, 2], [0, 2, 1])
    assert np.array_equal(AR.record_counts(nodes, 0, 6), np.ones(6, np.int64))
    assert AR.height(nodes, 0) == 1 and AR.height(nodes, 1) == 0 and AR.height(nodes, _leaf(0, 2)) == -1
    assert AR.containment_violations(nodes, 0, verts) == []
    assert AR.sah_estimate(nodes, 0) == 1.0 + 16.0 / 26.0
    assert AR.sah_estimate(nodes, 1) == 1.0                                        # no inner child: the root's own visit
    assert AR.sah_estimate(nodes, _leaf(0, 2)) == 0.0
    # a vertex outside its leaf's box
    v = verts.copy(); v[2, 1, 1] = 2.25
    bad = AR.containment_violations(nodes, 0, v)
    assert len(bad) == 2 and all("vertex" in b for b in bad) and "node 1 child 1" in bad[0] and "node 0 child 0" in bad[1]
    # an inner child's box that contains its vertices but not the box stored below it
    n2 = nodes.copy(); n2["q"][2][6 + 5] = 1.5
    bad = AR.containment_violations(n2, 0, verts)
    assert len(bad) == 1 and "node 0 child 1" in bad[0] and "box 1 stored in node 2" in bad[0]
    # a record reached twice, a record never reached
    n3 = nodes.copy(); n3["ref1"][2] = _leaf(4, 1)
    assert list(AR.record_counts(n3, 0, 6)) == [1, 1, 1, 1, 2, 0]
    # an absent child is neither counted nor checked
    n4 = nodes.copy(); n4["ref1"][0] = AR.REF_NONE
    assert AR.reachable(n4, 0) == [0, 1] and AR.containment_violations(n4, 0, verts) == []
    assert AR.sah_estimate(n4, 0) == 1.0 + 11.0 / 11.0


def test_estimate_rounds_each_term_in_float32_and_sums_in_float64():
    """Boxes whose half-areas are not exact in float32: the helper's value is the float32 terms' float64 sum over the float32 root area."""
    nodes, _ = _tree()
    nodes["q"][0][:6] = _box((0.1, 0.2, 0.3), (1.3, 2.7, 3.1))
    f = np.float32
    d = [f(1.3) - f(0.1), f(2.7) - f(0.2), f(3.1) - f(0.3)]
    t0 = f(f(d[0] * d[1]) + f(d[1] * d[2])) + f(d[2] * d[0])
    lo = np.minimum(nodes["q"][0][0:6:2], nodes["q"][0][6:12:2]); hi = np.maximum(nodes["q"][0][1:6:2], nodes["q"][0][7:12:2])
    e = hi - lo
    a0 = f(f(e[0] * e[1]) + f(e[1] * e[2])) + f(e[2] * e[0])
    assert t0.dtype == np.float32 and a0.dtype == np.float32
    assert AR.sah_estimate(nodes, 0) == 1.0 + (float(t0) + 5.0) / float(a0)
    assert AR.sah_estimate(nodes, 0) != 1.0 + (float(d[0]) * float(d[1]) + float(d[1]) * float(d[2]) + float(d[2]) * float(d[0]) + 5.0) / float(a0)
