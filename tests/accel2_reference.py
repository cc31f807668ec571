"""Pure-numpy reading of a two-level tree as HipIntegrator.read_accel_two_level() returns it (hpt_types.h: BvhNode, BvhTri, BvhInst), built on
accel_reference.py: which instances the TLAS root reaches and which records every BLAS root reaches, whether the boxes contain what lies below
them (float64: BLAS boxes the object-space vertices, TLAS boxes the world-space vertices at both keys of a moving instance), the depths, and the
two-level surface-area estimate - TLAS visits + the sum over the live instances of halfArea(instance box) / halfArea(TLAS root) x the BLAS visits
of its mesh; every half-area a float32 expression in the kernels' order, the sums in float64. No device, no library."""
import numpy as np

import accel_reference as AR

INST_DTYPE = np.dtype([("rows", np.float32, (3, 4)), ("root", np.uint32), ("geomId", np.uint32), ("moving", np.uint32), ("pad1", np.uint32)])


def is_instance_leaf(ref):
    return ref != AR.REF_NONE and bool(ref & AR.REF_LEAF) and ((int(ref) >> 28) & 7) == 0


def tlas_nodes(nodes, root):
    """Ids of the TLAS nodes, parents first (none when the root is an instance leaf or the scene is empty)."""
    return AR.reachable(nodes, root)


def tlas_leaves(nodes, root):
    """[(instance id, lo, hi)] of every instance leaf the root reaches, the box as stored in the leaf's parent (None for a root that is a leaf)."""
    if root == AR.REF_NONE:
        return []
    if is_instance_leaf(root):
        return [(int(root) & 0x0FFFFFFF, None, None)]
    out = []
    for i in tlas_nodes(nodes, root):
        q = nodes["q"][i]
        for c, ref in enumerate((int(nodes["ref0"][i]), int(nodes["ref1"][i]))):
            if ref == AR.REF_NONE or not (ref & AR.REF_LEAF):
                continue
            assert is_instance_leaf(ref), f"TLAS node {i} child {c}: a triangle leaf ({ref:#x}) in the top level"
            out.append((ref & 0x0FFFFFFF, q[6 * c:6 * c + 6:2].copy(), q[6 * c + 1:6 * c + 6:2].copy()))
    return out


def instance_counts(nodes, root, n_inst):
    """How often each instance is reached from the TLAS root (sound: 1 for an instance of a non-empty mesh, 0 for one of an empty mesh)."""
    cnt = np.zeros(n_inst, np.int64)
    for i, _, _ in tlas_leaves(nodes, root):
        assert i < n_inst, f"instance leaf {i} outside the {n_inst} instances"
        cnt[i] += 1
    return cnt


def depth(nodes, root):
    """Inner levels below (and with) the root: 0 for a leaf or no tree."""
    return AR.height(nodes, root) + 1


def blas_roots(insts):
    """{geomId: root reference} over the instance records; an instance of an empty mesh holds REF_NONE."""
    roots = {}
    for r in insts:
        g = int(r["geomId"])
        assert roots.setdefault(g, int(r["root"])) == int(r["root"]), f"mesh {g} has two roots"
    return roots


def blas_record_counts(nodes, insts, n_tris):
    """How often each triangle record is reached from the BLAS roots, every mesh counted once (sound: 1 everywhere), and the mesh of each record."""
    cnt, owner = np.zeros(n_tris, np.int64), np.full(n_tris, -1, np.int64)
    for g, root in sorted(blas_roots(insts).items()):
        if root == AR.REF_NONE:
            continue
        c = AR.record_counts(nodes, root, n_tris)
        cnt += c
        owner[c > 0] = g
    return cnt, owner


def blas_violations(nodes, tris, insts, mesh_verts):
    """Containment in object space: mesh_verts[g] is (nt, 3, 3) float64 by primitive. Strings, none for a sound tree."""
    bad = []
    cnt, owner = blas_record_counts(nodes, insts, tris.shape[0])
    verts = np.zeros((tris.shape[0], 3, 3))
    for k in np.flatnonzero(owner >= 0):
        verts[k] = mesh_verts[int(owner[k])][int(tris["primId"][k])]
    for g, root in sorted(blas_roots(insts).items()):
        if root != AR.REF_NONE:
            bad += [f"mesh {g}: {b}" for b in AR.containment_violations(nodes, root, verts)]
    return bad


def tlas_violations(nodes, root, insts, mesh_verts, matrices, matrices1=None):
    """Containment in world space: every TLAS child box contains, in float64, every vertex of every instance below it under the instance's
    row-major object -> world matrix (float32 values), and under matrices1[i] too for a moving instance i (dict)."""
    matrices1 = matrices1 or {}
    span = {}

    def inst_span(i):
        if i not in span:
            v = mesh_verts[int(insts["geomId"][i])].reshape(-1, 3)
            lo, hi = np.full(3, np.inf), np.full(3, -np.inf)
            for m in [matrices[i]] + ([matrices1[i]] if i in matrices1 else []):
                m = np.asarray(m, np.float32).astype(np.float64)
                w = v @ m[:3, :3].T + m[:3, 3]
                lo, hi = np.minimum(lo, w.min(axis=0)), np.maximum(hi, w.max(axis=0))
            span[i] = (lo, hi)
        return span[i]

    bad, lo_of, hi_of = [], {}, {}
    for i in reversed(tlas_nodes(nodes, root)):
        q = nodes["q"][i].astype(np.float64)
        nlo, nhi = np.full(3, np.inf), np.full(3, -np.inf)
        for c, ref in enumerate((int(nodes["ref0"][i]), int(nodes["ref1"][i]))):
            if ref == AR.REF_NONE:
                continue
            blo, bhi = q[6 * c:6 * c + 6:2], q[6 * c + 1:6 * c + 6:2]
            lo, hi = inst_span(ref & 0x0FFFFFFF) if ref & AR.REF_LEAF else (lo_of[ref], hi_of[ref])
            if not (np.all(blo <= lo) and np.all(hi <= bhi)):
                bad.append(f"TLAS node {i} child {c}: a vertex below it lies outside its box (box {blo} .. {bhi}, vertices {lo} .. {hi})")
            nlo, nhi = np.minimum(nlo, lo), np.maximum(nhi, hi)
        lo_of[i], hi_of[i] = nlo, nhi
    return bad


def _inner_area_sum(nodes, root):
    """Float64 sum of the float32 half-areas of the inner children below the root."""
    ids = np.asarray(AR.reachable(nodes, root))
    q = nodes["q"][ids]
    total = 0.0
    for c, name in enumerate(("ref0", "ref1")):
        ref = nodes[name][ids].astype(np.int64)
        lo, hi = q[:, 6 * c:6 * c + 6:2], q[:, 6 * c + 1:6 * c + 6:2]
        inner = (ref != AR.REF_NONE) & ((ref & AR.REF_LEAF) == 0) & (hi[:, 0] - lo[:, 0] >= 0)
        total += float(np.sum(AR._half_area32(lo, hi)[inner].astype(np.float64)))
    return total


def blas_visits(nodes, root, lo, hi):
    """Expected inner-node visits of a BLAS whose unpadded object-space bounds are lo .. hi (float32): 1 + the inner children's half-areas over
    the bounds' half-area; 0 when the root is no node or the bounds have no area."""
    if not AR.is_inner(root):
        return 0.0
    a0 = float(AR._half_area32(np.asarray(lo, np.float32), np.asarray(hi, np.float32)))
    return 1.0 + _inner_area_sum(nodes, root) / a0 if a0 > 0.0 else 0.0


def estimate(nodes, insts, root, mesh_bounds):
    """The two-level estimate. mesh_bounds[g] = (lo, hi), the float32 bounds of mesh g's vertices. The TLAS root's box is the union of the
    instance boxes stored in the leaves; a root that is an instance leaf has no box: the estimate is that instance's BLAS visits."""
    leaves = tlas_leaves(nodes, root)
    if not leaves:
        return 0.0
    visits = {g: blas_visits(nodes, r, *mesh_bounds[g]) for g, r in blas_roots(insts).items() if r != AR.REF_NONE}
    if is_instance_leaf(root):
        return visits[int(insts["geomId"][leaves[0][0]])]
    lo = np.min([l for _, l, _ in leaves], axis=0)
    hi = np.max([h for _, _, h in leaves], axis=0)
    a0 = float(AR._half_area32(lo, hi))
    if not a0 > 0.0:
        return 0.0
    v = 1.0 + _inner_area_sum(nodes, root) / a0
    for i, l, h in leaves:
        v += float(AR._half_area32(l, h)) / a0 * visits[int(insts["geomId"][i])]
    return v
