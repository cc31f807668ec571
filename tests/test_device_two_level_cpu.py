"""The device build of the two-level layout without a GPU: the numpy reader of a two-level read-back (tests/accel2_reference.py) on a hand-built
tree with known numbers, the ABI surface of hpt_get_two_level_info and hpt_read_accel_two_level (declared, bound, exported, null-safe), and the
sort key's packing (lbvh_key.h) as a stand-alone program built with the sanitizers."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import accel_reference as AR
import accel2_reference as A2
from conftest import ROOT

SYMBOLS = ["hpt_get_two_level_info", "hpt_read_accel_two_level"]


# ---- 1. the reader on a tree with known numbers ---------------------------------------------------------------------------------------------------
def _box(lo, hi):
    return [lo[0], hi[0], lo[1], hi[1], lo[2], hi[2]]


def _tree():
    """Two meshes, three instances. Mesh 0: three triangles in [0,1] x [0,1] x [0,2] (half-area 1*1 + 1*2 + 2*1 = 5); its BLAS is node 1 over node 2
    (box [0,1] x [0,1] x [0,0], half-area 1; single-record leaves 0 and 1) and the leaf of record 2: depth 2, visits 1 + 1/5. Mesh 1 is empty.
    Instance 0: mesh 0, identity, box [0,1] x [0,1] x [0,2] (5). Instance 1: mesh 0, moving from x + 3 to x + 4, box [3,5] x [0,1] x [0,2]
    (2*1 + 1*2 + 2*2 = 8). Instance 2: the empty mesh, not in the TLAS. The TLAS is node 0 with the two instance leaves: depth 1, root box
    [0,5] x [0,1] x [0,2] (5*1 + 1*2 + 2*5 = 17), no inner child. Estimate: 1 + 5/17 * 1.2 + 8/17 * 1.2. Node 3 is unused."""
    nodes = np.zeros(4, AR.NODE_DTYPE)
    nodes[0] = (_box((0, 0, 0), (1, 1, 2)) + _box((3, 0, 0), (5, 1, 2)), AR.REF_LEAF | 0, AR.REF_LEAF | 1, 0, 0)
    nodes[1] = (_box((0, 0, 0), (1, 1, 0)) + _box((0, 0, 1), (1, 1, 2)), 2, AR.REF_LEAF | (1 << 28) | 2, 0, 0)
    nodes[2] = (_box((0, 0, 0), (1, 1, 0)) + _box((0, 0, 0), (1, 1, 0)), AR.REF_LEAF | (1 << 28) | 0, AR.REF_LEAF | (1 << 28) | 1, 0, 0)
    nodes[3] = ([9] * 12, 77, 78, 0, 0)
    mesh0 = np.array([[[0, 0, 0], [1, 0, 0], [0, 1, 0]], [[1, 1, 0], [1, 0, 0], [0, 1, 0]], [[0, 0, 1], [1, 0, 1], [0, 1, 2]]], np.float64)
    tris = np.zeros(3, AR.TRI_DTYPE)
    tris["primId"] = [1, 0, 2]                                                      # (leaf order need not be primitive order)
    insts = np.zeros(3, A2.INST_DTYPE)
    insts["root"] = [1, 1, AR.REF_NONE]
    insts["geomId"] = [0, 0, 1]
    insts["moving"] = [0, 1, 0]
    shift = lambda x: np.array([[1, 0, 0, x], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]], np.float64)
    return nodes, tris, insts, [mesh0, np.zeros((0, 3, 3))], [np.eye(4), shift(3.0), np.eye(4)], {1: shift(4.0)}


def test_reader_on_a_hand_built_two_level_tree():
    nodes, tris, insts, meshes, mats, mats1 = _tree()
    root = 0
    assert sorted(i for i, _, _ in A2.tlas_leaves(nodes, root)) == [0, 1]
    assert list(A2.instance_counts(nodes, root, 3)) == [1, 1, 0]
    assert A2.blas_roots(insts) == {0: 1, 1: AR.REF_NONE}
    cnt, owner = A2.blas_record_counts(nodes, insts, 3)
    assert list(cnt) == [1, 1, 1] and list(owner) == [0, 0, 0]
    assert A2.depth(nodes, root) == 1 and A2.depth(nodes, 1) == 2 and A2.depth(nodes, AR.REF_LEAF | 1) == 0 and A2.depth(nodes, AR.REF_NONE) == 0
    assert A2.blas_violations(nodes, tris, insts, meshes) == []
    assert A2.tlas_violations(nodes, root, insts, meshes, mats, mats1) == []
    bounds = {0: (np.float32([0, 0, 0]), np.float32([1, 1, 2]))}
    assert A2.blas_visits(nodes, 1, *bounds[0]) == 1.0 + 1.0 / 5.0
    assert A2.blas_visits(nodes, AR.REF_LEAF | (2 << 28), *bounds[0]) == 0.0
    bv = 1.0 + 1.0 / 5.0
    assert A2.estimate(nodes, insts, root, bounds) == (1.0 + 5.0 / 17.0 * bv) + 8.0 / 17.0 * bv
    # a TLAS root that is an instance leaf: that instance's BLAS visits
    assert A2.estimate(nodes, insts, AR.REF_LEAF | 1, bounds) == bv
    assert list(A2.instance_counts(nodes, AR.REF_LEAF | 1, 3)) == [0, 1, 0]
    assert A2.estimate(nodes, insts, AR.REF_NONE, bounds) == 0.0
    # the moving instance's leaf box must hold the second key too
    n2 = nodes.copy(); n2["q"][0][6 + 1] = 4.5
    bad = A2.tlas_violations(n2, root, insts, meshes, mats, mats1)
    assert len(bad) == 1 and "TLAS node 0 child 1" in bad[0]
    assert A2.tlas_violations(n2, root, insts, meshes, mats, {}) == []               # (with one key it would)
    # an object-space vertex outside its BLAS leaf
    m2 = [meshes[0].copy(), meshes[1]]; m2[0][2, 2, 2] = 2.5
    bad = A2.blas_violations(nodes, tris, insts, m2)
    assert len(bad) == 1 and bad[0].startswith("mesh 0: node 1 child 1")
    # records follow their primId, not their position
    t2 = tris.copy(); t2["primId"] = [2, 0, 1]
    assert A2.blas_violations(nodes, t2, insts, meshes) != []
    # an instance reached twice; a record never reached
    n3 = nodes.copy(); n3["ref1"][0] = AR.REF_LEAF | 0
    assert list(A2.instance_counts(n3, root, 3)) == [2, 0, 0]
    n4 = nodes.copy(); n4["ref1"][1] = AR.REF_LEAF | (1 << 28) | 1
    assert list(A2.blas_record_counts(n4, insts, 3)[0]) == [1, 2, 0]


# ---- 2. ABI -------------------------------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_two_level_symbols_and_the_front_end_binds_them():
    from hydracore3_amd import api
    hdr = open(os.path.join(ROOT, "include", "hydra_hip.h")).read()
    for name in SYMBOLS:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
        assert m, f"{name} is not declared in include/hydra_hip.h"
        assert name in api.ABI, f"{name} is not in api.ABI"
        assert len(api.ABI[name][1]) == len(m.group(1).split(",")), (name, m.group(1))
    assert len(api.ABI["hpt_get_two_level_info"][1]) == 2 and len(api.ABI["hpt_read_accel_two_level"][1]) == 6
    for meth in ("two_level_info", "read_accel_two_level"):
        assert hasattr(api.HipIntegrator, meth)
    assert '"device_build_two_level"' in hdr, "the option is not documented in include/hydra_hip.h"
    assert api.BVH_INST_DTYPE == A2.INST_DTYPE


def test_library_exports_the_two_level_symbols_and_null_handles_are_refused():
    from hydracore3_amd import api
    lib = api.load_library()
    nm = subprocess.run(["nm", "-D", "--defined-only", api.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (hpt_[a-z0-9_]+)", nm))
    assert set(SYMBOLS) <= exported
    buf = (C.c_float * 8)()
    nbytes, root = C.c_uint64(7), C.c_uint32(7)
    assert lib.hpt_get_two_level_info(None, buf) == 1                             # HPT_ERR_ARG, no device touched
    assert lib.hpt_read_accel_two_level(None, 0, None, 0, C.byref(nbytes), C.byref(root)) == 1
    assert lib.hpt_read_accel_two_level(None, 2, buf, 32, None, None) == 1
    assert nbytes.value == 7 and root.value == 7


# ---- 3. the sort key ------------------------------------------------------------------------------------------------------------------------------------
def test_key_packing_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "lbvh_key_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "cpp", "lbvh_key_test.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "all key checks passed" in r.stdout and "FAILED" not in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    bits = dict((int(a), int(b)) for a, b in re.findall(r"^slots=2\^(\d+) morton_bits=(\d+)$", r.stdout, re.M))
    assert bits[0] == 21 and bits[1] == 21 and bits[16] == 16 and bits[20] == 14      # (what lbvh_key.h says)
