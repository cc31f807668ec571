"""Seeded adversarial scenes and rays for the traversal tests (tests/test_traversal_edges.py), built in Python through hydracore3_amd.scene
(no golden files), and an independent float64 reference of the closest hit: every mesh taken to world space with the FORWARD instance
matrix in float64 and Moeller-Trumbore in float64 - not the float inverse rows the oracle and the kernels share."""
import numpy as np

from hydracore3_amd import scene as S

FLT_MAX = np.float32(3.402823466e+38)
NO_HIT = 0xFFFFFFFF


# ---- meshes (object space): (positions (n, 3) float64, indices (m, 3)) ------------------------------------------------------------------------
def quad():
    """Two coplanar triangles (the pair plane cull applies)."""
    return np.array([[-1, -1, 0], [1, -1, 0], [1, 1, 0], [-1, 1, 0]], float), np.array([[0, 1, 2], [0, 2, 3]])


def bent_quad():
    """A pair that is not coplanar: the plane cull never applies."""
    return np.array([[-1, -1, 0], [1, -1, 0.0], [1, 1, 0.35], [-1, 1, 0]], float), np.array([[0, 1, 2], [0, 2, 3]])


def lone_triangle():
    """One triangle: an odd mesh, paired with the padding record."""
    return np.array([[-1, -0.8, 0.1], [1.2, -0.5, -0.2], [0.1, 1.1, 0.05]], float), np.array([[0, 1, 2]])


def sliver():
    """Two triangles of aspect 1e-3."""
    return np.array([[-1, 0, 0], [1, 0, 0], [1, 2e-3, 0], [-1, 2e-3, 0]], float), np.array([[0, 1, 2], [0, 2, 3]])


def degenerate_and_duplicate():
    """A zero-area triangle (collinear vertices: det == 0), a triangle and the same triangle again (the primId tie rule)."""
    p = np.array([[-1, 0, 0], [0, 0, 0], [1, 0, 0], [-0.7, -0.9, 0.2], [0.9, -0.4, -0.1], [0.0, 1.0, 0.3]], float)
    return p, np.array([[0, 1, 2], [3, 4, 5], [3, 4, 5]])


def fan(n):
    """n triangles around a raised centre (no pair is coplanar)."""
    a = np.linspace(0.0, 2.0 * np.pi, n + 1)
    p = np.concatenate([[[0.0, 0.0, 0.4]], np.stack([np.cos(a), np.sin(a), np.zeros_like(a)], 1)])
    return p, np.array([[0, 1 + k, 2 + k] for k in range(n)])


def box():
    """A closed cube, 12 triangles."""
    p = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], float) * 0.5
    f = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    return p, np.array([t for a, b, c, d in f for t in ((a, b, c), (a, c, d))])


def strip(n, rng, flat=False):
    """A strip of n triangles over n + 2 vertices, crumpled unless flat (then every record pair is coplanar)."""
    k = np.arange(n + 2)
    p = np.stack([(k // 2) * 0.3, (k % 2) * 0.8, np.zeros(n + 2)], 1)
    if not flat:
        p[:, 2] = rng.uniform(-0.15, 0.15, n + 2)
    p[:, 0] -= p[:, 0].mean()
    return p, np.array([[j, j + 1, j + 2] if j % 2 == 0 else [j + 1, j, j + 2] for j in range(n)])


# ---- instance transforms (row-major 4x4, float64) ---------------------------------------------------------------------------------------------
def rotation(axis, ang):
    a = np.asarray(axis, float) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    m = np.eye(4)
    m[:3, :3] = np.eye(3) + np.sin(ang) * K + (1.0 - np.cos(ang)) * K @ K
    return m


def transform(kind, rng):
    """identity; rotation about an arbitrary axis; non-uniform scale with factors 1e-2 .. 1e2 apart; mirror (negative determinant); shear; far
    translation (1e3 .. 1e4). All but the identity and the far one sit within a few units of the origin, in view and overlapping."""
    t = S.translate(*rng.uniform(-3.0, 3.0, 3))
    rot = rotation(rng.normal(size=3), rng.uniform(0.0, 2.0 * np.pi))
    if kind == "identity":
        return np.eye(4)
    if kind == "rotate":
        return t @ rot
    if kind == "scale":
        s = 10.0 ** rng.uniform(-2.0, 2.0, 3)
        s *= rng.uniform(0.5, 2.0) / np.cbrt(np.prod(s))                  # the volume stays O(1): the instance stays in view
        return t @ rot @ S.scale(*s)
    if kind == "mirror":
        return t @ rot @ S.scale(-1.0, 1.0, 1.0)
    if kind == "shear":
        sh = np.eye(4)
        sh[0, 1], sh[1, 2], sh[0, 2] = rng.uniform(-1.5, 1.5, 3)
        return t @ sh @ rot
    if kind == "far":
        d = rng.normal(size=3)
        return S.translate(*(d / np.linalg.norm(d) * 10.0 ** rng.uniform(3.0, 4.0))) @ rot
    raise ValueError(kind)


def _add(sc, mesh, mat):
    p, idx = mesh
    n = p.shape[0]
    pos4 = np.concatenate([p, np.ones((n, 1))], 1).astype(np.float32)
    nrm = np.tile([0.0, 0.0, 1.0, 0.0], (n, 1)).astype(np.float32)
    tng = np.tile([1.0, 0.0, 0.0, 0.0], (n, 1)).astype(np.float32)
    uv = (p[:, :2] * 0.5 + 0.5).astype(np.float32)
    return sc.add_mesh(pos4, nrm, tng, uv, np.asarray(idx, np.uint32).reshape(-1), np.full(len(idx), mat, np.uint32))


def _base_scene(width, height, spectral, rng):
    """Camera, a rect light and four materials: lambert, textured lambert (texture 1, the one DR tests differentiate), glass, conductor."""
    sc = S.SceneData()
    sc.width, sc.height = width, height
    if spectral:
        sc.spectral_mode = 1
        sc.spec_offset_sz, sc.spec_values = [(0, 471)], np.ones(471, np.float32)
    sc.cam_pos, sc.cam_look_at, sc.cam_up = (0.5, 1.0, 9.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0)
    sc.fov, sc.trace_depth = 50.0, 5
    sc.env_color = (0.05, 0.06, 0.08, 0.0)
    img = rng.integers(0, 2 ** 32, (8, 8), dtype=np.uint64).astype(np.uint32) | np.uint32(0xFF000000)
    tex = sc.add_texture(S.Texture(img, S.TEX_RGBA8, True))
    M = sc.materials
    M.append(S.material_lambert((0.6, 0.55, 0.5)))
    M.append(S.material_lambert((0.8, 0.8, 0.8), tex))
    M.append(S.material_glass((1, 1, 1), (0.9, 0.95, 1.0), 1.5))
    M.append(S.material_conductor(0.2, 3.9, 0.1, 0.1))
    sc.lights.append(S.light_rect(S.translate(0.0, 4.0, 1.0), 1.2, 1.2, (1, 1, 1), 12.0))
    return sc


def sweep_scene(seed, width=48, height=32, spectral=False):
    """Automatic-sweep class: at most 32 instanced triangles in at most 8 instances (hpt_host.hip: SWEEP_MAX_TRIS, SWEEP_MAX_INSTS). Coplanar and
    bent quads, a lone triangle, slivers, a zero-area and a duplicated triangle, a fan (even seeds) or a box (odd seeds); each under one of
    the transform classes, and one small mesh a second time under the same matrix (the instId tie rule)."""
    rng = np.random.default_rng(seed)
    sc = _base_scene(width, height, spectral, rng)
    meshes = [quad(), bent_quad(), lone_triangle(), sliver(), degenerate_and_duplicate(), box() if seed % 2 else fan(int(rng.integers(3, 6)))]
    kinds = ["identity", "rotate", "scale", "mirror", "shear", "far"]
    # four meshes and four transforms per scene, rotating with the seed (three consecutive seeds cover all six of each), plus one of them a
    # second time: 5 instances, since from MANY_INSTANCES = 6 on the automatic choice takes the single-level tree instead of the sweep
    first = seed % 3 * 2
    pick = [(first + k) % 6 for k in range(4)]
    kind = [kinds[(first + 1 + k) % 6] for k in range(4)]
    geoms = [_add(sc, meshes[k], k % 4) for k in pick]
    mats = [transform(k, rng) for k in kind]
    for g, m in zip(geoms, mats):
        sc.add_instance(g, m)
    small = [j for j, k in enumerate(pick) if k != 5]                     # (twice the box would pass 32 triangles)
    twice = small[int(rng.integers(len(small)))]
    sc.add_instance(geoms[twice], mats[twice])
    return sc


FORCED_TRIS = (3, 4, 63, 64, 65, 66)       # 2, 2, 32, 32, 33, 33 record pairs: the per-lane pass' bounds and the wave-uniform loop past them


def forced_sweep_scene(seed, width=48, height=32):
    """Forced-sweep class (accel_layout=3): strips of 3, 4, 63, 64, 65 and 66 triangles under rotated, scaled and mirrored instances."""
    rng = np.random.default_rng(seed)
    sc = _base_scene(width, height, False, rng)
    for j, n in enumerate(FORCED_TRIS):
        g = _add(sc, strip(n, rng, flat=(j % 3 == 0)), j % 4)
        sc.add_instance(g, transform(("rotate", "scale", "mirror")[j % 3], rng))
    return sc


# ---- the float64 reference ----------------------------------------------------------------------------------------------------------------------
def world_triangles(sc):
    """(T, 3, 3) float64 world-space vertices and the (instId, primId) of each: float32 vertices and float32 matrices (what the scene holds),
    multiplied out in float64."""
    tris, ids = [], []
    for i, (g, m) in enumerate(zip(sc.inst_geom, sc.inst_matrices)):
        m32 = np.asarray(m, np.float32).astype(np.float64)
        to, vo = sc.mat_vert_offset[g]
        nt = sc.geom_tri_count[g]
        idx = sc.tri_indices[3 * to:3 * (to + nt)].reshape(nt, 3).astype(np.int64) + vo
        p = sc.vpos[:, :3].astype(np.float64)[idx]
        tris.append(p @ m32[:3, :3].T + m32[:3, 3])
        ids += [(i, k) for k in range(nt)]
    return np.concatenate(tris), np.asarray(ids, np.int64)


def reference_hits(tris, ids, inst_matrices, pos, dr, chunk=2048):
    """Closest hit of every ray in float64: (hit, t, instId, primId, robust). A ray is robust when every triangle is clear of its decision by a
    relative 1e-4 (barycentric margin; distance of t to tnear and tfar), the nearest and the runner-up t differ by more than 1e-4 relative,
    and every triangle it hits is met at |cos| > 1e-3 - the 1e-4 grown by the instance's condition number / 100 and by the magnitude of the
    coordinates / (100 x the triangle's smallest altitude), where the float ray's own object-space rounding outgrows it. A ray that comes near a sliver
    (altitude < 1e-2 of its longest edge) is never robust: on the sheared sliver of sweep_scene(12) the float pipeline's v differs from
    float64 by up to 0.25 on ~10 of 12 000 rays, more than the rounding bounds above explain (an open question, not held here). Equal t of identical triangles (duplicates) is a tie: the lower (instId, primId) wins,
    as in the kernels."""
    n = pos.shape[0]
    out_hit, out_t = np.zeros(n, bool), np.zeros(n)
    out_inst, out_prim, robust = np.full(n, -1), np.full(n, -1), np.zeros(n, bool)
    A, B, C = tris[:, 0], tris[:, 1], tris[:, 2]
    e1, e2 = B - A, C - A
    nrm = np.cross(e1, e2)
    area2 = np.linalg.norm(nrm, axis=1)
    live = area2 > 1e-9 * np.linalg.norm(e1, axis=1) * np.linalg.norm(e2, axis=1)
    size = area2 / np.maximum(np.maximum(np.linalg.norm(e1, axis=1), np.linalg.norm(e2, axis=1)), np.linalg.norm(C - B, axis=1))   # smallest altitude
    cond = np.array([np.linalg.cond(np.asarray(m, np.float64)[:3, :3]) for m in inst_matrices])[ids[:, 0]]
    sliver = size < 1e-2 * np.maximum(np.maximum(np.linalg.norm(e1, axis=1), np.linalg.norm(e2, axis=1)), np.linalg.norm(C - B, axis=1))
    order = np.lexsort((ids[:, 1], ids[:, 0]))
    for s in range(0, n, chunk):
        o = pos[s:s + chunk, None, :3].astype(np.float64)
        d = dr[s:s + chunk, None, :3].astype(np.float64)
        tn = pos[s:s + chunk, 3, None].astype(np.float64)
        tf = dr[s:s + chunk, 3, None].astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            pvec = np.cross(d, e2[None])
            det = np.sum(e1[None] * pvec, -1)
            inv = 1.0 / det
            tvec = o - A[None]
            u = np.sum(tvec * pvec, -1) * inv
            qvec = np.cross(tvec, e1[None])
            v = np.sum(d * qvec, -1) * inv
            t = np.sum(e2[None] * qvec, -1) * inv
            cos = np.abs(np.sum(nrm[None] * d, -1)) / (np.maximum(area2, 1e-300)[None] * np.linalg.norm(d, axis=-1))
            ok = live[None] & (det != 0.0) & np.isfinite(t)
            margin = np.minimum(np.minimum(u, v), 1.0 - u - v)
            hit = ok & (margin >= 0.0) & (t >= tn) & (t <= tf)
            mag = np.maximum(np.linalg.norm(tvec, axis=-1), np.linalg.norm(o, axis=-1) + np.linalg.norm(A, axis=-1)[None])
            # the float pipeline takes the ray to object space with rounded inverse rows: its error grows with the instance's condition
            # number and with the magnitude of the origin and of the triangle's coordinates (or their distance) in units of the triangle, and the
            # relative bound grows with both
            rel = 1e-4 * np.maximum(1.0, cond[None] * 1e-2) * np.maximum(1.0, mag / (1e2 * size[None]))
            scale = np.maximum(np.abs(t), 1.0)
            clear_t = (np.abs(t - tn) > rel * scale) & (np.abs(t - tf) > rel * scale)
            relg = rel * np.maximum(1.0, 1e-3 / np.maximum(cos, 1e-30))      # a grazing ray's barycentrics err by 1 / cos more, miss or hit
            rob_tri = ~live[None] | (ok & (margin < -relg)) | (ok & (margin > relg) & clear_t & (cos > 1e3 * rel))
            rob_tri &= ~(sliver[None] & ok & (margin > -0.5))                # (see the docstring)
            tt = np.where(hit, t, np.inf)
            k = order[np.argmin(tt[:, order], axis=1)]                     # argmin keeps the first of equal values: the lowest (instId, primId)
            best = tt[np.arange(tt.shape[0]), k]
            runner = np.where(tt == best[:, None], np.inf, tt).min(axis=1)
            sep = ~np.isfinite(runner) | (runner - best > 1e-4 * np.maximum(np.abs(best), 1.0))
        h = np.isfinite(best)
        sl = slice(s, s + tt.shape[0])
        out_hit[sl], out_t[sl] = h, np.where(h, best, 0.0)
        out_inst[sl], out_prim[sl] = np.where(h, ids[k, 0], -1), np.where(h, ids[k, 1], -1)
        robust[sl] = rob_tri.all(axis=1) & sep
    return out_hit, out_t, out_inst, out_prim, robust


def assert_hits_equal(h, ref, what):
    """Two hit arrays (RayQuery_NearestHit / ray_nearest records) equal bit for bit: ids, t, and the coordinates of the rays that hit."""
    for f in ("primId", "instId", "geomId"):
        bad = np.flatnonzero(h[f] != ref[f])
        assert bad.size == 0, f"{what}: {f} differs on {bad.size} rays, first {bad[:8]}: {h[f][bad[:4]]} vs {ref[f][bad[:4]]}"
    bad = np.flatnonzero(h["t"].view(np.uint32) != ref["t"].view(np.uint32))
    assert bad.size == 0, f"{what}: t differs on {bad.size} rays, first {bad[:8]}: {h['t'][bad[:4]]} vs {ref['t'][bad[:4]]}"
    hit = ref["geomId"] != NO_HIT
    assert np.array_equal(h["coords"][hit][:, :3].view(np.uint32), ref["coords"][hit][:, :3].view(np.uint32)), f"{what}: coords"


# ---- rays ---------------------------------------------------------------------------------------------------------------------------------------
FAMILIES = ("random", "aimed", "grazing", "offset", "axis", "far")
TNEARS = (0.0, None, -1.0, -1e2, -1e4, -float(FLT_MAX))                   # None: a random tnear > 0


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def make_rays(tris, n, seed, families=FAMILIES):
    """Ray families, built in float64 and rounded to float32, each towards a target on a random triangle: random rays around it; rays aimed at a
    vertex or an edge, the float direction nudged by -1, 0 or +1 ulp per component; grazing rays (1e-5 .. 1e-2 rad to the plane; a known limit,
    not fixed here: at 1e-7 rad the float test's t keeps no digit, and the trees' boxes - the oracle's too - miss some of its hits); rays leaving
    the surface from the renderer's offset (hpt_shade.h: hitPos + hitNorm * max(maxcomp(hitPos), 1) * 5e-6) to either side, into it or away;
    axis-parallel directions (one or two zero components); origins 1e3 .. 1e5 away. A third of the rays point away from their target (a hit
    behind the origin). tnear in {0, > 0, -1, -1e2, -1e4, -FLT_MAX}; tfar = FLT_MAX (with_tfar sets others). Returns pos (n, 4), dir (n, 4) float32
    and the family of each ray."""
    rng = np.random.default_rng(seed)
    fam = np.asarray([FAMILIES.index(f) for f in families])[rng.integers(0, len(families), n)]
    k = rng.integers(0, tris.shape[0], n)
    A, B, C = tris[k, 0], tris[k, 1], tris[k, 2]
    nrm = np.cross(B - A, C - A)
    nl = np.linalg.norm(nrm, axis=1, keepdims=True)
    nrm = np.where(nl > 0, nrm / np.where(nl > 0, nl, 1.0), np.array([0.0, 0.0, 1.0]))
    size = np.maximum(np.linalg.norm(np.stack([B - A, C - A, C - B], 1), axis=2).max(axis=1), 1e-3)
    bary = rng.dirichlet((1.0, 1.0, 1.0), n)
    tgt = bary[:, :1] * A + bary[:, 1:2] * B + bary[:, 2:] * C
    e = rng.integers(0, 3, n)
    P, Q = np.stack([A, B, C], 1)[np.arange(n), e], np.stack([B, C, A], 1)[np.arange(n), e]
    s = np.where(rng.uniform(size=n) < 0.33, 0.0, rng.uniform(size=n))     # a vertex, or a point on an edge
    tgt = np.where((fam == 1)[:, None], P + s[:, None] * (Q - P), tgt)
    d = _unit(rng.normal(size=(n, 3)))
    tang = _unit(d - np.sum(d * nrm, 1, keepdims=True) * nrm)
    ang = 10.0 ** rng.uniform(-5.0, -2.0, n) * np.where(rng.uniform(size=n) < 0.5, 1.0, -1.0)
    d = np.where((fam == 2)[:, None], np.cos(ang)[:, None] * tang + np.sin(ang)[:, None] * nrm, d)
    axd = np.zeros((n, 3))
    ax = rng.integers(0, 3, n)
    axd[np.arange(n), ax] = np.where(rng.uniform(size=n) < 0.5, 1.0, -1.0)
    two = rng.uniform(size=n) < 0.4
    axd[np.arange(n)[two], ((ax + 1) % 3)[two]] = rng.uniform(-1.0, 1.0, two.sum())
    axd = _unit(axd)
    d = np.where((fam == 4)[:, None], axd, d)
    dist = np.where(fam == 5, 10.0 ** rng.uniform(3.0, 5.0, n), size * 10.0 ** rng.uniform(-0.5, 1.0, n))
    org = tgt - d * dist[:, None]
    rnd = fam == 0
    org[rnd] = tgt[rnd] + rng.normal(size=(rnd.sum(), 3)) * size[rnd, None] * 2.0
    off = fam == 3
    hp = tgt[off].astype(np.float32)
    hn = (nrm[off] * np.where(rng.uniform(size=off.sum()) < 0.5, 1.0, -1.0)[:, None]).astype(np.float32)
    h = np.maximum(hp.max(axis=1), np.float32(1.0)) * np.float32(5e-6)
    org[off] = hp + hn * h[:, None]
    g = 10.0 ** rng.uniform(-7.0, 0.0, off.sum()) * np.where(rng.uniform(size=off.sum()) < 0.7, 1.0, -1.0)
    w = _unit(rng.normal(size=(off.sum(), 3)))
    d[off] = _unit(w - np.sum(w * hn, 1, keepdims=True) * hn + g[:, None] * hn)
    aim = (fam == 1) | (fam == 2) | (fam == 5)
    d[aim] = _unit(tgt[aim] - org[aim])
    back = rng.uniform(size=n) < 0.33
    d[back] = -d[back]
    pos, dr = np.zeros((n, 4), np.float32), np.zeros((n, 4), np.float32)
    pos[:, :3], dr[:, :3] = org, d
    nud = rng.integers(-1, 2, (n, 3))
    for c in range(3):
        sel = (fam == 1) & (nud[:, c] != 0)
        dr[sel, c] = np.nextafter(dr[sel, c], np.where(nud[sel, c] > 0, np.float32(np.inf), np.float32(-np.inf)))
    tk = rng.integers(0, len(TNEARS), n)
    tn = np.array([0.0 if TNEARS[j] is None else TNEARS[j] for j in tk])
    tn[tk == 1] = rng.uniform(0.0, 1.0, (tk == 1).sum()) * dist[tk == 1]
    pos[:, 3] = tn.astype(np.float32)
    dr[:, 3] = FLT_MAX
    return pos, dr, fam


def with_tfar(pos, dr, open_t, seed):
    """tfar per ray: FLT_MAX, random, exactly open_t (the brute-force t of the ray with tfar = FLT_MAX; random without a hit), or the float just
    below it."""
    rng = np.random.default_rng(seed)
    n = pos.shape[0]
    k = rng.integers(0, 4, n)
    rnd = (np.maximum(pos[:, 3], -1e4) + rng.uniform(0.0, 20.0, n)).astype(np.float32)
    exact = np.where(np.isfinite(open_t), open_t, rnd).astype(np.float32)
    below = np.where(np.isfinite(open_t), np.nextafter(exact, np.float32(-np.inf)), rnd).astype(np.float32)
    out = dr.copy()
    out[:, 3] = np.select([k == 0, k == 1, k == 2], [np.full(n, FLT_MAX), rnd, exact], below).astype(np.float32)
    return out


# ---- nested sheets: trees deeper than the LDS part of the traversal stacks ------------------------------------------------------------------------
NESTED_TRI_CAP = 32768                     # instanced triangles


def nested_sheets(n=8000, ratio=1.0015, a0=0.03, dz=3e-4, instances=1, width=96, height=64, spectral=False, emissive=False):
    """n right triangles in the planes z = i dz, triangle i larger than triangle i - 1 by `ratio` (legs 2 a0 ratio^i), every hypotenuse on the line
    x + y = 0 through the z axis and the boxes' centres (a_i / 2, -a_i / 2) moving away from it with the size: a ray along z at a distance
    below a0 / 2 from the axis lies in every triangle's box - hence in every node's - and meets every triangle (x + y < 0) or none (x + y > 0).
    The binned SAH build peels the few largest sheets off at every level, so the tree is far deeper than log2(n / 4): 8000 sheets at 1.0015 give
    a BVH2 of depth 18 and a 4-wide tree of depth 16 (stack bounds 19 and 49; the LDS part holds 16). instances > 1: the same mesh that many
    times, instance k scaled by 1.5^k in x and y and its stack of sheets put behind the one before. All materials gltf (the second one
    textured: texture 1, 8 x 8) or emissive; one large emissive sheet behind the camera lights the scene; the camera sits on the small end and
    looks along +z. emissive: every sheet an emitter of one of three colours instead, no light, trace depth 1 - a sample's colour is then the
    emission its primary ray meets (what the QMC pass can be held to the oracle on). Other sizes used by the tests (host build, BVH2 / 4-wide
    depth): 20 000 sheets at 1.0006: 19 / 17; 4 000 at 1.003 x 8 instances: 24 / 20. The parameters are returned in sc.nested."""
    assert n * instances + 2 <= NESTED_TRI_CAP
    sc = S.SceneData()
    sc.width, sc.height = width, height
    if spectral:
        sc.spectral_mode = 1
        sc.spec_offset_sz, sc.spec_values = [(0, 471)], np.ones(471, np.float32)
    sc.cam_pos, sc.cam_look_at, sc.cam_up = (0.0, 0.0, -0.3), (0.0, 0.0, 1.0), (0.0, 1.0, 0.0)
    sc.fov, sc.trace_depth = 20.0, 4
    sc.env_color = (0.05, 0.06, 0.08, 0.0)
    rng = np.random.default_rng(n)
    img = rng.integers(0, 2 ** 32, (8, 8), dtype=np.uint64).astype(np.uint32) | np.uint32(0xFF000000)
    tex = sc.add_texture(S.Texture(img, S.TEX_RGBA8, True))
    M = sc.materials
    M.append(S.material_gltf((0.7, 0.65, 0.6, 1.0), 0.0, 0.3))
    M.append(S.material_gltf((0.8, 0.8, 0.8, 1.0), 0.0, 0.5, 1.0, 1.5, tex))
    M.append(S.material_gltf((0.9, 0.9, 0.9, 1.0), 1.0, 0.9))
    emis = len(M)
    a = a0 * ratio ** np.arange(n)
    z = dz * np.arange(n)
    p = np.empty((n, 3, 3))
    p[:, 0] = np.stack([-a / 2, -3 * a / 2, z], 1)
    p[:, 1] = np.stack([3 * a / 2, -3 * a / 2, z], 1)
    p[:, 2] = np.stack([-a / 2, a / 2, z], 1)
    pos4 = np.concatenate([p.reshape(-1, 3), np.ones((3 * n, 1))], 1).astype(np.float32)
    nrm = np.tile([0.0, 0.0, -1.0, 0.0], (3 * n, 1)).astype(np.float32)
    tng = np.tile([1.0, 0.0, 0.0, 0.0], (3 * n, 1)).astype(np.float32)
    uv = np.tile([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0]], (n, 1)).astype(np.float32)
    g = sc.add_mesh(pos4, nrm, tng, uv, np.arange(3 * n, dtype=np.uint32), (np.arange(n) % 3).astype(np.uint32))
    depth = n * dz
    for k in range(instances):
        sc.add_instance(g, S.translate(0.0, 0.0, k * depth) @ S.scale(1.5 ** k, 1.5 ** k, 1.0))
    sc.nested = {"n": n, "ratio": ratio, "a0": a0, "dz": dz, "instances": instances, "z_end": instances * depth, "a_max": float(a[-1]) * 1.5 ** (instances - 1)}
    if emissive:
        sc.materials = [S.material_emissive(c, mult=m) for c, m in (((0.9, 0.2, 0.1), 1.0), ((0.1, 0.8, 0.3), 1.25), ((0.3, 0.4, 1.2), 1.5))]
        sc.trace_depth = 1
        sc.env_color = (0.125, 0.25, 0.5, 0.0)
        return sc
    lm = S.translate(0.0, 0.0, -2.0) @ S.rotate_x(-90.0)
    sc.lights.append(S.light_rect(lm, 3.0, 3.0, (1.0, 0.95, 0.9), 6.0))
    M.append(S.material_emissive((1.0, 0.95, 0.9), 6.0, 0))
    sc.lights[0]["matId"] = emis
    _add_emitter(sc, lm, emis)
    return sc


def _add_emitter(sc, lm, mat):
    p = np.array([[-3, 0, -3], [3, 0, -3], [3, 0, 3], [-3, 0, 3]], float)
    pos4 = np.concatenate([p, np.ones((4, 1))], 1).astype(np.float32)
    nrm = np.tile([0.0, -1.0, 0.0, 0.0], (4, 1)).astype(np.float32)
    tng = np.tile([1.0, 0.0, 0.0, 0.0], (4, 1)).astype(np.float32)
    uv = np.array([[0, 0], [1, 0], [1, 1], [0, 1]], np.float32)
    g = sc.add_mesh(pos4, nrm, tng, uv, np.array([0, 1, 2, 0, 2, 3], np.uint32), np.full(2, mat, np.uint32))
    sc.add_instance(g, lm, -1, 0)


NESTED_FAMILIES = ("covered", "empty", "covered tilted", "empty tilted", "outer covered", "outer empty")


def nested_rays(sc, n, seed, near=0.5):
    """Rays for nested_sheets, float32 pos (n, 4), dir (n, 4) and the family of each. Near the axis (distance a0 10^-2.5 .. a0 / 10: inside
    every box), through the covered half (x + y < 0: every sheet is hit, the closest-hit order matters) or the empty half of the boxes
    (x + y > 0: every node is visited, nothing is hit), along +z (most) or -z or tilted by 1e-4 .. 3e-2 rad about the point where they cross the
    middle of the stack; and, for the float64 reference, which cannot call a ray robust that passes a_max / 10^5 from an edge of the largest
    sheets, the same two kinds further out (a_max / 300 .. a_max / 4, along the axis only; the share 1 - near of all rays). Origins in front of the stack, behind it, or (a quarter to a sixth)
    inside it, where the negative tnear of TNEARS finds sheets behind the origin. tfar = FLT_MAX (with_tfar sets others)."""
    q = sc.nested
    rng = np.random.default_rng(seed)
    fam = rng.choice(len(NESTED_FAMILIES), n, p=[near / 4] * 4 + [(1.0 - near) / 2] * 2)
    outer = fam >= 4
    empty = (fam % 2) == 1
    r = np.where(outer, q["a_max"] * 10.0 ** rng.uniform(-2.5, -0.6, n), q["a0"] * 10.0 ** rng.uniform(-2.5, -1.0, n))
    # covered: a direction between -x and -y, where the triangle's own box ends furthest out; empty: between +x and the hypotenuse (y <= a / 2 there)
    phi = np.where(empty, rng.uniform(-0.6, 0.6, n), np.pi + np.pi / 4 + rng.uniform(-0.5, 0.5, n))
    x, y = r * np.cos(phi), r * np.sin(phi) * np.where(empty, 0.3, 1.0)
    sgn = np.where(rng.uniform(size=n) < np.where(outer, 0.5, 0.85), 1.0, -1.0)   # (from the small end the walk descends the whole unbalanced tree before its first leaf: the deepest stacks)
    d = np.zeros((n, 3)); d[:, 2] = sgn
    tilt = ((fam == 2) | (fam == 3))
    ang = 10.0 ** rng.uniform(-4.0, -1.5, n) * tilt
    psi = rng.uniform(0.0, 2.0 * np.pi, n)
    d[:, 0], d[:, 1] = np.tan(ang) * np.cos(psi), np.tan(ang) * np.sin(psi)
    d = _unit(d)
    zmid = 0.5 * q["z_end"]
    inside = rng.uniform(size=n) < np.where(outer, 0.25, 0.15)
    oz = np.where(inside, rng.uniform(0.0, q["z_end"], n), np.where(sgn > 0, -0.25, q["z_end"] + 0.25))
    s = (oz - zmid) / d[:, 2]                                             # the ray passes (x, y, zmid)
    org = np.stack([x + d[:, 0] * s, y + d[:, 1] * s, oz], 1)
    pos, dr = np.zeros((n, 4), np.float32), np.zeros((n, 4), np.float32)
    pos[:, :3], dr[:, :3] = org, d
    tk = rng.integers(0, len(TNEARS), n)
    tn = np.array([0.0 if TNEARS[j] is None else TNEARS[j] for j in tk])
    tn[tk == 1] = rng.uniform(0.0, 1.0, (tk == 1).sum()) * (q["z_end"] + 0.25)
    pos[:, 3] = tn.astype(np.float32)
    dr[:, 3] = FLT_MAX
    return pos, dr, fam
