"""Numpy restatement of the treelet optimiser (hydracore3_amd/csrc/treelet_opt.h): the subset recurrence in float32 with the header's
association and tie rule, the explicit enumeration of every binary topology over k leaves it is checked against, and the readers the GPU
tests use on a read-back tree. No device, no library.

  area(s) = half-area of the union box of the leaves in s       cost(one leaf) = 0
  cost(s) = area(s) + min over p of (cost(p) + cost(s ^ p))      part(s) = the lowest mask p attaining the minimum
"""
import numpy as np

LEAVES = 7
f32 = np.float32


def half_area32(lo, hi):
    """dx * dy + dy * dz + dz * dx in float32, left to right (no contraction)."""
    d = (np.asarray(hi, f32) - np.asarray(lo, f32)).astype(f32)
    return f32(f32(f32(d[0] * d[1]) + f32(d[1] * d[2])) + f32(d[2] * d[0]))


def subset_areas(boxes):
    """boxes: (k, 6) float32 rows {lo.xyz, hi.xyz}. area[s] for every mask s < 2^k (area[0] = 0)."""
    boxes = np.asarray(boxes, f32)
    k = boxes.shape[0]
    area = np.zeros(1 << k, f32)
    for s in range(1, 1 << k):
        sel = [j for j in range(k) if (s >> j) & 1]
        area[s] = half_area32(boxes[sel, :3].min(axis=0), boxes[sel, 3:].max(axis=0))
    return area


def splits(s):
    """The candidate partitions of s in ascending order: the non-empty subsets of s without its highest leaf."""
    rest = s ^ (1 << (s.bit_length() - 1))
    p = (-rest) & rest
    while p:
        yield p
        p = (p - rest) & rest


def optimize(boxes):
    """(area, cost, part) over the subsets of the k leaves, float32 / float32 / uint8, as treeletOptimize fills them."""
    area = subset_areas(boxes)
    k = np.asarray(boxes).shape[0]
    cost = np.zeros(1 << k, f32)
    part = np.zeros(1 << k, np.uint8)
    for size in range(2, k + 1):
        for s in range(1, 1 << k):
            if bin(s).count("1") != size:
                continue
            best, best_p = None, 0
            for p in splits(s):
                c = f32(cost[p] + cost[s ^ p])
                if best is None or c < best:
                    best, best_p = c, p
            cost[s] = f32(area[s] + best)
            part[s] = best_p
    return area, cost, part


def topology(part, s):
    """The chosen topology under s as nested tuples of leaf numbers."""
    if s & (s - 1) == 0:
        return s.bit_length() - 1
    p = int(part[s])
    return (topology(part, p), topology(part, s ^ p))


def topology_cost(area, topo):
    """(cost, mask) of a nested-tuple topology by the recurrence's formula: area + (cost(left) + cost(right)), float32."""
    if not isinstance(topo, tuple):
        return f32(0.0), 1 << topo
    (cl, ml), (cr, mr) = topology_cost(area, topo[0]), topology_cost(area, topo[1])
    return f32(area[ml | mr] + f32(cl + cr)), ml | mr


def all_topologies(leaves):
    """Every binary topology over the given leaf numbers, each once (children unordered): (2k - 3)!! of them."""
    leaves = list(leaves)
    if len(leaves) == 1:
        yield leaves[0]
        return
    head, rest = leaves[-1], leaves[:-1]
    for m in range(1, 1 << len(rest)):                                    # the side without the last leaf: any non-empty subset of the others
        a = [rest[j] for j in range(len(rest)) if (m >> j) & 1]
        b = [rest[j] for j in range(len(rest)) if not (m >> j) & 1] + [head]
        for ta in all_topologies(a):
            for tb in all_topologies(b):
                yield (ta, tb)


def topology_count(k):
    n = 1
    for j in range(3, 2 * k - 2, 2):
        n *= j
    return n


def enumerated_costs(area, k, s=None, memo=None):
    """The float32 cost of every topology over leaves 0 .. k-1, one entry per topology: per leaf set, for every split (the set's last leaf stays on
    the second side, so each unordered split comes once) every pairing of a topology of one side with a topology of the other, costed by the
    recurrence's formula area + (left + right)."""
    s = (1 << k) - 1 if s is None else s
    memo = {} if memo is None else memo
    if s not in memo:
        if s & (s - 1) == 0:
            memo[s] = np.zeros(1, f32)
        else:
            memo[s] = np.concatenate([(area[s] + (enumerated_costs(area, k, p, memo)[:, None] + enumerated_costs(area, k, s ^ p, memo)[None, :])).astype(f32).ravel()
                                      for p in splits(s)])
    return memo[s]


# ---- a read-back tree (accel_reference.NODE_DTYPE records) ------------------------------------------------------------------------------------
def tree_leaf_boxes(nodes, root, AR):
    """(k, 6) float32 {lo.xyz, hi.xyz}: the boxes of the leaf children the root reaches, as stored (padded) in their parents."""
    out = []
    for i in AR.reachable(nodes, root):
        for c, ref in enumerate((int(nodes["ref0"][i]), int(nodes["ref1"][i]))):
            if ref != AR.REF_NONE and ref & AR.REF_LEAF:
                q = nodes["q"][i][6 * c:6 * c + 6]
                out.append([q[0], q[2], q[4], q[1], q[3], q[5]])
    return np.asarray(out, f32)


def tree_half_area_sum(nodes, root, AR):
    """Sum over the inner nodes of the half-areas of their boxes, float64: the root's box is the union of the two boxes it stores, every other
    node's box is the one its parent stores for it."""
    order = AR.reachable(nodes, root)
    r = nodes["q"][int(root)].astype(np.float64)
    lo = np.minimum(r[0:6:2], r[6:12:2]); hi = np.maximum(r[1:6:2], r[7:12:2])
    d = hi - lo
    total = d[0] * d[1] + d[1] * d[2] + d[2] * d[0]
    for i in order:
        for c, ref in enumerate((int(nodes["ref0"][i]), int(nodes["ref1"][i]))):
            if AR.is_inner(ref):
                q = nodes["q"][i][6 * c:6 * c + 6].astype(np.float64)
                d = q[1::2] - q[0::2]
                total += d[0] * d[1] + d[1] * d[2] + d[2] * d[0]
    return float(total)
