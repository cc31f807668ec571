"""Scenes and the case table of the texture-adjoint tests (test_dr_textures_cpu.py, test_dr_textures_gpu.py).

Every DR test before these registered its parameter texture square, power of two, four channels, alone at offset 0, and fetched it with
uv in [0, 1) under wrap addressing. The cases here register it at the sizes and layouts where the index arithmetic of the differentiable
fetch (bilinearTaps / texFetchAD), of the record packing (drMakeRecord: tap 0's element, two signed steps) and of the staged scatter
(drReverseSweep) takes another path: sizes that are no power of two, w != h, one texel wide or high, one channel, a second texture behind
the first, clamp addressing. Everything is built in Python; no golden files."""
import functools

import numpy as np

from hydracore3_amd import scene as S
from hydracore3_amd.synth import _merge, _quad

WIDTH, HEIGHT = 33, 17            # 561 paths: 8 full waves and one of 49 lanes
DEPTH = 3
SEED = 3                          # scene seed of every case (see profiles/dr_textures.md for its history)
FLOOR_TEX, BOX_TEX = 1, 2         # texture ids the floor / the box material bind
PAD, PAD_VALUE = 8, 7.0           # a_data / a_dataGrad are passed PAD floats longer than registered, the tail filled with PAD_VALUE
SCHEDULES = [1, 2, 3]             # the parameter list of test_gpu_dr.test_c4_dr_test228_matches_oracle
W, C = S.ADDR_WRAP, S.ADDR_CLAMP


class Case:
    def __init__(self, name, floor, addr=(W, W), second=None):
        self.name, self.floor, self.addr, self.second = name, floor, addr, second

    def registrations(self):
        """[(texture id, w, h, channels)] in registration order."""
        r = [(FLOOR_TEX, *self.floor)]
        if self.second is not None:
            r.append((BOX_TEX, *self.second))
        return r

    def layout(self):
        """[(offset, w, h, channels)] of the registered textures in a_data."""
        out, off = [], 0
        for _, w, h, ch in self.registrations():
            out.append((off, w, h, ch))
            off += w * h * ch
        return out

    def size(self):
        return sum(w * h * ch for _, w, h, ch in self.registrations())

    def __repr__(self):
        return self.name


CASES = [
    Case("npot", (5, 3, 4)),                          # wrapi branch, w != h, both seams, negative steps
    Case("npot_t", (3, 5, 4)),                        # its transpose
    Case("pow2_rect", (8, 2, 4)),                     # mask branch with w != h
    Case("row", (7, 1, 4)),                           # dy == 0
    Case("column", (1, 7, 4)),                        # dx == 0
    Case("single", (1, 1, 4)),                        # all four taps on one element
    Case("mono_npot", (6, 5, 1)),                     # one-channel path
    Case("mono_pow2", (16, 8, 1)),                    # one-channel path, mask branch
    Case("clamp_u", (6, 4, 4), (C, W)),               # addr == 2 on one axis
    Case("clamp_uv", (5, 4, 1), (C, C)),              # addr == 2, one channel
    Case("two", (6, 2, 1), (W, W), (5, 3, 4)),        # 12 floats, then a four-channel texture at offset 12: both kinds in one path
    Case("sparse", (64, 24, 4)),                      # most texels get nothing: a misplaced tap is a non-zero where the oracle has 0
]
BY_NAME = {c.name: c for c in CASES}
OVERFLOW = Case("overflow", (5, 3, 4))                # the closed box below: more than 64 (lane, bounce) columns in one sweep


def _bound_image(rng, n=4):
    """A small RGBA32F image for a material to bind (the parameter fetch ignores its size and content). Square: its own fetch is not
    what these tests are about."""
    img = rng.uniform(0.2, 0.9, (n, n, 4)).astype(np.float32)
    img[..., 3] = 1.0
    return img


def _box_parts(mat):
    """Unit cube [0, 1]^3, outward normals, uv in [0, 1]^2 on every face."""
    faces = [((0, 1, 1), (1, 0, 0), (0, 0, -1)), ((0, 0, 0), (1, 0, 0), (0, 0, 1)), ((0, 0, 1), (1, 0, 0), (0, 1, 0)),
             ((1, 0, 0), (-1, 0, 0), (0, 1, 0)), ((1, 0, 1), (0, 0, -1), (0, 1, 0)), ((0, 0, 0), (0, 0, 1), (0, 1, 0))]
    return [(*_quad(*f), mat) for f in faces]


def _add_rect_light(sc, matrix, half, radiance):
    light_id, emis = len(sc.lights), len(sc.materials)
    sc.lights.append(S.light_rect(matrix, half, half, (1, 1, 1), radiance))
    sc.materials.append(S.material_emissive((1, 1, 1), radiance, light_id))
    sc.lights[light_id]["matId"] = emis
    lp, ln, lt, luv, lidx = _quad((-half, 0, -half), (2 * half, 0, 0), (0, 0, 2 * half))      # normal -y
    sc.add_instance(sc.add_mesh(lp, ln, lt, luv, lidx, [emis]), matrix, -1, light_id)


def floor_and_box_scene(addr=(W, W), seed=SEED):
    """A lambert floor and a gltf box (metalness 0.5, coat 1) on it under a rect light, 33 x 17, depth 3. The floor's texture matrix scales
    uv by about 2.5 and shifts it by about -0.7: the transformed coordinates cover negative values and several wrap periods in both axes.
    The box binds a second texture with the identity matrix. `addr`: the address modes of the floor's texture."""
    rng = np.random.RandomState(seed)
    sc = S.SceneData()
    sc.width, sc.height, sc.trace_depth, sc.fov = WIDTH, HEIGHT, DEPTH, 50.0
    sc.cam_pos = (0.3 + rng.uniform(-0.2, 0.2), 2.4 + rng.uniform(-0.2, 0.2), 4.2 + rng.uniform(-0.2, 0.2))
    sc.cam_look_at, sc.cam_up = (0.0, 0.3, 0.0), (0.0, 1.0, 0.0)
    sc.env_color = (0.05, 0.06, 0.08, 0.0)                                         # escaping paths carry a tail into the sweep
    assert sc.add_texture(S.Texture(_bound_image(rng), S.TEX_RGBA32F, False, addr[0], addr[1], S.FILTER_LINEAR)) == FLOOR_TEX
    assert sc.add_texture(S.Texture(_bound_image(rng), S.TEX_RGBA32F, False, W, W, S.FILTER_LINEAR)) == BOX_TEX
    floor = S.material_lambert((0.9, 0.85, 0.8), FLOOR_TEX)
    floor["row0"][0] = (2.5 + rng.uniform(-0.05, 0.05), 0.0, 0.0, -0.7 + rng.uniform(-0.02, 0.02))
    floor["row1"][0] = (0.0, 2.5 + rng.uniform(-0.05, 0.05), 0.0, -0.7 + rng.uniform(-0.02, 0.02))
    box = S.material_gltf((0.85, 0.8, 0.9, 1.0), 0.5, 0.6, 1.0, 1.5, BOX_TEX)
    sc.materials += [floor, box]
    sc.add_instance(sc.add_mesh(*_quad((-3, 0, 3), (6, 0, 0), (0, 0, -6), 4, 4), [0]), np.eye(4))
    m = S.translate(-0.5 + rng.uniform(-0.2, 0.2), 0.0, -0.2 + rng.uniform(-0.2, 0.2)) @ S.rotate_y(25.0 + rng.uniform(-10, 10)) @ \
        S.scale(1.3, 1.0, 1.3) @ S.translate(-0.5, 0.0, -0.5)
    sc.add_instance(sc.add_mesh(*_merge(_box_parts(1))), m)
    _add_rect_light(sc, S.translate(0.4, 3.5, 0.5), 0.8, 18.0)
    return sc


def closed_box_scene(seed=SEED):
    """A closed room seen from inside, every wall lambert with the parameter texture, a small light under the ceiling, 8 x 8, depth 8: almost
    every bounce of every path records a tap, so the sweep of a wave stages far more than 64 (lane, bounce) columns."""
    rng = np.random.RandomState(seed)
    sc = S.SceneData()
    sc.width, sc.height, sc.trace_depth, sc.fov = 8, 8, 8, 70.0
    sc.cam_pos = (0.1 + rng.uniform(-0.1, 0.1), 0.9 + rng.uniform(-0.1, 0.1), 0.8)
    sc.cam_look_at, sc.cam_up = (0.0, 0.7, -1.0), (0.0, 1.0, 0.0)
    assert sc.add_texture(S.Texture(_bound_image(rng), S.TEX_RGBA32F, False, W, W, S.FILTER_LINEAR)) == FLOOR_TEX
    wall = S.material_lambert((0.9, 0.9, 0.9), FLOOR_TEX)
    wall["row0"][0] = (2.5, 0.0, 0.0, -0.7)
    wall["row1"][0] = (0.0, 2.5, 0.0, -0.7)
    sc.materials.append(wall)
    X, Y, Z = 1.0, 2.0, 1.0
    parts = [(*_quad((-X, 0, Z), (2 * X, 0, 0), (0, 0, -2 * Z), 2, 2), 0), (*_quad((-X, Y, -Z), (2 * X, 0, 0), (0, 0, 2 * Z), 2, 2), 0),
             (*_quad((-X, 0, -Z), (2 * X, 0, 0), (0, Y, 0), 2, 2), 0), (*_quad((X, 0, Z), (-2 * X, 0, 0), (0, Y, 0), 2, 2), 0),
             (*_quad((-X, 0, Z), (0, 0, -2 * Z), (0, Y, 0), 2, 2), 0), (*_quad((X, 0, -Z), (0, 0, 2 * Z), (0, Y, 0), 2, 2), 0)]
    sc.add_instance(sc.add_mesh(*_merge(parts)), np.eye(4))
    _add_rect_light(sc, S.translate(0.0, Y - 0.01, 0.0), 0.25, 30.0)
    return sc


def scene_of(case):
    return closed_box_scene() if case is OVERFLOW else floor_and_box_scene(case.addr)


def inputs(case, sc, seed=5):
    """(data, ref): the parameters, PAD floats longer than registered with the tail set to PAD_VALUE, and the reference frame."""
    rng = np.random.default_rng(seed)
    data = np.full(case.size() + PAD, PAD_VALUE, np.float32)
    data[:case.size()] = rng.uniform(0.2, 0.9, case.size()).astype(np.float32)
    ref = rng.uniform(0.0, 0.5, (sc.height, sc.width, 4)).astype(np.float32)
    return data, ref


def register_cpu(cpu, case):
    out = []
    for tex, w, h, ch in case.registrations():
        rc, off, size = cpu.put_diff_tex2d(tex, w, h, ch)
        assert rc == 0
        out.append((off, size))
    assert out == [(off, w * h * ch) for off, w, h, ch in case.layout()]
    return out


def register_gpu(gpu, case):
    return [tuple(gpu.PutDiffTex2D(tex, w, h, ch)) for tex, w, h, ch in case.registrations()]


def oracle_dr(cpu, spp, ref, data, tid_begin=0, tid_count=None):
    """orc_path_trace_dr into a gradient buffer pre-filled with PAD_VALUE (OracleIntegrator.path_trace_dr hands over zeros): the reference
    memsets all of a_gradSize, and so does the oracle. Returns (loss, grad, frame)."""
    tid_count = cpu.N - tid_begin if tid_count is None else tid_count
    frame = np.zeros((cpu.H, cpu.W, 4), np.float32)
    grad = np.full(data.size, PAD_VALUE, np.float32)
    loss = cpu.L.orc_path_trace_dr(cpu.h, tid_begin, tid_count, 4, frame.ctypes.data, spp, ref.ctypes.data, data.ctypes.data, grad.ctypes.data, data.size)
    return float(loss), grad, frame


def where(case, j):
    """Element j of a_data as text: texture, texel coordinates, channel."""
    for k, (off, w, h, ch) in enumerate(case.layout()):
        if off <= j < off + w * h * ch:
            t = (j - off) // ch
            return f"texture {k} ({w}x{h}x{ch}) texel x={t % w} y={t // w} channel {(j - off) % ch}"
    return f"tail element {j - case.size()}"


def border_elements(case):
    """Every element of texel column 0 and w - 1 and of texel row 0 and h - 1, of every registered texture."""
    idx = []
    for off, w, h, ch in case.layout():
        y, x = np.mgrid[0:h, 0:w]
        edge = (x == 0) | (x == w - 1) | (y == 0) | (y == h - 1)
        t = np.flatnonzero(edge.reshape(-1))
        idx.append((off + t[:, None] * ch + np.arange(ch)[None, :]).reshape(-1))
    return np.concatenate(idx)


def alpha_elements(case):
    idx = [off + np.arange(w * h) * 4 + 3 for off, w, h, ch in case.layout() if ch == 4]
    return np.concatenate(idx) if idx else np.zeros(0, np.int64)


def as_four_channels(case, data):
    """The one-channel case registered with four channels, its data (d, d, d, 1): the same texture to the renderer."""
    assert case.second is None and case.floor[2] == 1
    four = Case(case.name + "_x4", (case.floor[0], case.floor[1], 4), case.addr)
    d4 = np.full(four.size() + PAD, PAD_VALUE, np.float32)
    q = d4[:four.size()].reshape(-1, 4)
    q[:, :3] = data[:case.size(), None]
    q[:, 3] = 1.0
    return four, d4


def reorder_noise(case, spp=4):
    """e_ord of a case: the oracle's gradient with one thread against sixteen (per-thread partial sums added in another order),
    max |c1 - c16| / max |c16|. The reference's own summation-order noise; the GPU tests take their absolute floor from it."""
    from oracle import orc
    sc = scene_of(case)
    data, ref = inputs(case, sc)
    grads = []
    try:
        for threads in (1, 16):
            cpu = orc.OracleIntegrator(sc, threads=threads)
            register_cpu(cpu, case)
            grads.append(oracle_dr(cpu, spp, ref, data)[1][:case.size()].astype(np.float64))
    finally:
        orc.lib().orc_set_threads(0)                                              # (the thread count is a setting of the library: back to automatic)
    return float(np.abs(grads[0] - grads[1]).max() / np.abs(grads[1]).max())


@functools.lru_cache(maxsize=None)
def max_reorder_noise(spp=4):
    return max(reorder_noise(c, spp) for c in CASES)


def element_atol(grad_c, spp=4):
    """The absolute floor of the per-element gradient bound: max(1e-5, 8 e_ord) max|c| - 1e-5 is test_gradient_matches_oracle's, e_ord the
    reference's own reorder noise, and 8 x covers the GPU's atomics being one more arbitrary order."""
    return max(1e-5, 8.0 * max_reorder_noise(spp)) * float(np.abs(grad_c).max())


def assert_elements(case, grad_g, grad_c, atol, what=""):
    """|g - c| <= 1e-3 |c| + atol for EVERY element (1e-3: the per-pixel image bar; a texel's gradient is a sum of 2 (C - ref) dC w over
    pixels held to it). Returns the worst error relative to max|c|."""
    g, c = grad_g.astype(np.float64), grad_c.astype(np.float64)
    err = np.abs(g - c)
    bad = np.flatnonzero(err > 1e-3 * np.abs(c) + atol)
    for j in bad[:8]:
        print(f"{what}{case.name}: element {j} = {where(case, j)}: gpu {grad_g[j]:.9g} oracle {grad_c[j]:.9g} (bound {1e-3 * abs(c[j]) + atol:.3g})")
    assert bad.size == 0, f"{what}{case.name}: {bad.size} gradient elements out of bound, first: {where(case, bad[0])} gpu {grad_g[bad[0]]:.9g} oracle {grad_c[bad[0]]:.9g}"
    return float(err.max() / np.abs(c).max())
