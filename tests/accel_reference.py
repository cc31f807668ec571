"""Pure-numpy reading of a single-level tree as HipIntegrator.read_accel() returns it (hpt_types.h: BvhNode, BvhTri): which records every
child reaches, whether every box contains what lies below it (float64), the tree's height, and the surface-area estimate hpt_get_refit_info
reports - per-term half-areas in float32 in the kernel's expression order, their sum in float64. No device, no library."""
import numpy as np

REF_LEAF = 0x80000000
REF_NONE = 0xFFFFFFFE

NODE_DTYPE = np.dtype([("q", np.float32, (12,)), ("ref0", np.uint32), ("ref1", np.uint32), ("pad0", np.uint32), ("pad1", np.uint32)])
TRI_DTYPE = np.dtype([("v0", np.float32, (3,)), ("primId", np.uint32), ("e1", np.float32, (3,)), ("instId", np.uint32), ("e2", np.float32, (3,)), ("pad1", np.uint32)])


def is_inner(ref):
    return ref != REF_NONE and not (ref & REF_LEAF)


def leaf_range(ref):
    """(first record, count) of a leaf reference."""
    return int(ref) & 0x0FFFFFFF, (int(ref) >> 28) & 7


def reachable(nodes, root):
    """Ids of the nodes the root reaches, parents before children. A node reached twice, or a reference past the array, raises."""
    if not is_inner(root):
        return []
    order, seen, stack = [], set(), [int(root)]
    while stack:
        i = stack.pop()
        assert 0 <= i < nodes.shape[0], f"node reference {i} outside the array of {nodes.shape[0]}"
        assert i not in seen, f"node {i} is reached twice"
        seen.add(i)
        order.append(i)
        for ref in (int(nodes["ref0"][i]), int(nodes["ref1"][i])):
            if is_inner(ref):
                stack.append(ref)
    return order


def record_counts(nodes, root, n_tris):
    """How often each triangle record is reached from the root (a sound tree: 1 everywhere)."""
    cnt = np.zeros(n_tris, np.int64)
    refs = [int(root)] if (root != REF_NONE and root & REF_LEAF) else []
    for i in reachable(nodes, root):
        refs += [int(nodes["ref0"][i]), int(nodes["ref1"][i])]
    for ref in refs:
        if ref != REF_NONE and ref & REF_LEAF:
            first, count = leaf_range(ref)
            assert first + count <= n_tris, f"leaf [{first}, {first + count}) outside the {n_tris} records"
            cnt[first:first + count] += 1
    return cnt


def height(nodes, root):
    """Height of the root among the inner nodes: 0 when both children are leaves, else 1 + the larger inner child's. -1: the root is no node."""
    order = reachable(nodes, root)
    if not order:
        return -1
    h = {}
    for i in reversed(order):
        h[i] = max([h[int(r)] + 1 for r in (nodes["ref0"][i], nodes["ref1"][i]) if is_inner(int(r))], default=0)
    return h[int(root)]


def record_world_vertices(tris, world_tris, ids):
    """(n, 3, 3) float64 world-space vertices in record order, from traversal_scenes.world_triangles' (vertices, (instId, primId)) of the scene."""
    where = {(int(i), int(p)): k for k, (i, p) in enumerate(ids)}
    return np.stack([world_tris[where[(int(t["instId"]), int(t["primId"]))]] for t in tris])


def containment_violations(nodes, root, verts):
    """The ways in which a box fails to contain what lies below it, as strings (a sound tree: none). verts: (n, 3, 3) float64 world-space vertices
    per triangle record. Checked: every child box contains, in float64, every vertex of every record below it; every inner child's box contains,
    compared exactly, both boxes stored in the node it references."""
    bad = []
    order = reachable(nodes, root)
    lo_of, hi_of = {}, {}                                     # per node: the float64 bounds of every vertex below it
    for i in reversed(order):
        q = nodes["q"][i].astype(np.float64)
        nlo, nhi = np.full(3, np.inf), np.full(3, -np.inf)
        for c, ref in enumerate((int(nodes["ref0"][i]), int(nodes["ref1"][i]))):
            if ref == REF_NONE:
                continue
            blo, bhi = q[6 * c:6 * c + 6:2], q[6 * c + 1:6 * c + 6:2]
            if ref & REF_LEAF:
                first, count = leaf_range(ref)
                v = verts[first:first + count].reshape(-1, 3)
                lo, hi = v.min(axis=0), v.max(axis=0)
            else:
                lo, hi = lo_of[ref], hi_of[ref]
                k = nodes["q"][ref].astype(np.float64)
                for cc, r2 in enumerate((int(nodes["ref0"][ref]), int(nodes["ref1"][ref]))):
                    if r2 == REF_NONE:
                        continue
                    if not (np.all(blo <= k[6 * cc:6 * cc + 6:2]) and np.all(k[6 * cc + 1:6 * cc + 6:2] <= bhi)):
                        bad.append(f"node {i} child {c}: its box does not contain box {cc} stored in node {ref}")
            if not (np.all(blo <= lo) and np.all(hi <= bhi)):
                bad.append(f"node {i} child {c}: a vertex below it lies outside its box (box {blo} .. {bhi}, vertices {lo} .. {hi})")
            nlo, nhi = np.minimum(nlo, lo), np.maximum(nhi, hi)
        lo_of[i], hi_of[i] = nlo, nhi
    return bad


def _half_area32(lo, hi):
    """dx * dy + dy * dz + dz * dx in float32, left to right (the kernels are compiled without contraction)."""
    d = (hi.astype(np.float32) - lo.astype(np.float32)).astype(np.float32)
    dx, dy, dz = d[..., 0], d[..., 1], d[..., 2]
    return ((dx * dy).astype(np.float32) + (dy * dz).astype(np.float32)).astype(np.float32) + (dz * dx).astype(np.float32)


def sah_estimate(nodes, root):
    """1 + sum over the inner children of half-area(child box) / half-area(root box): every term a float32 expression, the sum in float64; the
    root's box is the union of the two padded child boxes stored in the root. 0 when the root is no node or its box is empty."""
    order = reachable(nodes, root)
    if not order:
        return 0.0
    ids = np.asarray(order)
    q = nodes["q"][ids]
    total = 0.0
    for c, name in enumerate(("ref0", "ref1")):
        ref = nodes[name][ids].astype(np.int64)
        lo, hi = q[:, 6 * c:6 * c + 6:2], q[:, 6 * c + 1:6 * c + 6:2]
        inner = (ref != REF_NONE) & ((ref & REF_LEAF) == 0) & (hi[:, 0] - lo[:, 0] >= 0)
        total += float(np.sum(_half_area32(lo, hi)[inner].astype(np.float64)))
    r = nodes[int(root)]
    present = [c for c, ref in enumerate((int(r["ref0"]), int(r["ref1"]))) if ref != REF_NONE]
    lo = np.min([r["q"][6 * c:6 * c + 6:2] for c in present], axis=0)
    hi = np.max([r["q"][6 * c + 1:6 * c + 6:2] for c in present], axis=0)
    a0 = float(_half_area32(lo, hi))
    return 1.0 + total / a0 if a0 > 0.0 else 0.0
