"""Scenes, gains and the bound of the light-colour gradient tests (test_light_grad_cpu.py, test_light_grad_gpu.py, light_grad_torch_child.py).

The colour of a sample is linear in the RGB gain of every light: C = C_0 + sum_l g_l C_l, and nothing about sampling reads an intensity. So
the frame F_l with light l at its own intensity and every other light at 0, and the frame F_0 with all of them at 0, trace the paths of the
frame under test, and d<a, F>/dg_l = <a, F_l - F_0> channel by channel: the reference of every gradient test here is made of forward frames.
Everything is built in Python; no golden files."""
import numpy as np

from hydracore3_amd import scene as S
from hydracore3_amd.synth import _merge, _quad, _sphere_mesh

WIDTH, HEIGHT, DEPTH = 24, 16, 5
BOX_TEX = 1                       # the 8 x 8 x 4 albedo texture of the box
TEX_W, TEX_H = 8, 8
SEED = 11                         # seed of the gains, adjoints and reference frames
BINS = 64                         # DR_LIGHT_BINS (hpt_shade.h): lights of the registration the workgroups' LDS bins hold
AREA_LIGHTS = (0, 1, 2)           # rect, disc, sphere: their meshes are in view
SCHEDULES = [1, 2]                # megakernel, wavefront


def _disc_mesh(segments=16):
    """Unit disc in the plane y = 0, normal -y (the side a rect / disc light emits from), as a triangle fan."""
    a = np.linspace(0.0, 2.0 * np.pi, segments, endpoint=False)
    pos = np.concatenate([[[0.0, 0.0, 0.0]], np.stack([np.cos(a), np.zeros(segments), np.sin(a)], 1)])
    n = pos.shape[0]
    pos4 = np.concatenate([pos, np.ones((n, 1))], 1).astype(np.float32)
    norm4 = np.tile(np.array([0.0, -1.0, 0.0, 0.0], np.float32), (n, 1))
    tang4 = np.tile(np.array([1.0, 0.0, 0.0, 0.0], np.float32), (n, 1))
    uv = (pos[:, [0, 2]] * 0.5 + 0.5).astype(np.float32)
    idx = []
    for i in range(segments):
        idx += [0, 1 + i, 1 + (i + 1) % segments]               # wound so that the geometric normal is -y as well
    return pos4, norm4, tang4, uv, np.asarray(idx, np.uint32)


def _bind_mesh(sc, light_id, mesh, matrix, color, mult):
    emis = len(sc.materials)
    sc.materials.append(S.material_emissive(color, mult, light_id))
    sc.lights[light_id]["matId"] = emis
    ntri = mesh[4].size // 3
    sc.add_instance(sc.add_mesh(mesh[0], mesh[1], mesh[2], mesh[3], mesh[4], np.full(ntri, emis, np.uint32)), matrix, -1, light_id)


def _base_scene():
    """A gltf floor and a gltf box with an 8 x 8 x 4 albedo texture, 24 x 16 pixels, trace depth 5, black environment."""
    rng = np.random.RandomState(SEED)
    sc = S.SceneData()
    sc.width, sc.height, sc.trace_depth, sc.fov = WIDTH, HEIGHT, DEPTH, 45.0
    sc.cam_pos, sc.cam_look_at, sc.cam_up = (0.0, 2.0, 5.5), (0.0, 1.0, 0.0), (0.0, 1.0, 0.0)
    sc.env_color = (0.0, 0.0, 0.0, 0.0)
    img = rng.uniform(0.2, 0.9, (TEX_H, TEX_W, 4)).astype(np.float32)
    img[..., 3] = 1.0
    assert sc.add_texture(S.Texture(img, S.TEX_RGBA32F, False, S.ADDR_WRAP, S.ADDR_WRAP, S.FILTER_LINEAR)) == BOX_TEX
    sc.materials += [S.material_gltf((0.8, 0.75, 0.7, 1.0), 0.0, 0.3, 0.0, 1.5), S.material_gltf((0.85, 0.8, 0.9, 1.0), 0.5, 0.6, 1.0, 1.5, BOX_TEX)]
    sc.add_instance(sc.add_mesh(*_quad((-4, 0, 4), (8, 0, 0), (0, 0, -8), 2, 2), [0]), np.eye(4))
    faces = [((0, 1, 1), (1, 0, 0), (0, 0, -1)), ((0, 0, 0), (1, 0, 0), (0, 0, 1)), ((0, 0, 1), (1, 0, 0), (0, 1, 0)),
             ((1, 0, 0), (-1, 0, 0), (0, 1, 0)), ((1, 0, 1), (0, 0, -1), (0, 1, 0)), ((0, 0, 0), (0, 0, 1), (0, 1, 0))]
    box = S.translate(-1.6, 0.0, 0.2) @ S.rotate_y(25.0) @ S.scale(1.1, 1.2, 1.1) @ S.translate(-0.5, 0.0, -0.5)
    sc.add_instance(sc.add_mesh(*_merge([(*_quad(*f), 1) for f in faces])), box)
    return sc


def scene_a():
    """Six lights, one of each kind: rect, disc, sphere (their meshes in view, tilted towards the camera and the floor), omni point, spot,
    directional. No environment colour and no emissive material without a light: every sample is homogeneous in the gains."""
    sc = _base_scene()
    L = sc.lights
    rect_m = S.translate(0.2, 2.3, -1.2) @ S.rotate_x(-50.0)
    L.append(S.light_rect(rect_m, 0.5, 0.35, (1.0, 0.9, 0.8), 9.0))
    lp, ln, lt, luv, lidx = _quad((-0.5, 0, -0.35), (1.0, 0, 0), (0, 0, 0.7))                      # normal -y
    _bind_mesh(sc, 0, (lp, ln, lt, luv, lidx), rect_m, (1.0, 0.9, 0.8), 9.0)
    disc_m = S.translate(1.9, 1.9, -0.6) @ S.rotate_x(-55.0)
    L.append(S.light_rect(disc_m, 0.0, 0.0, (0.6, 1.0, 0.7), 8.0, disk_radius=0.4))
    _bind_mesh(sc, 1, _disc_mesh(), disc_m @ S.scale(0.4, 1.0, 0.4), (0.6, 1.0, 0.7), 8.0)
    sph_m = S.translate(-0.3, 1.0, 1.2) @ S.scale(0.3, 0.3, 0.3)
    L.append(S.light_sphere(sph_m, 1.0, (0.7, 0.8, 1.0), 6.0))
    _bind_mesh(sc, 2, _sphere_mesh(1), sph_m, (0.7, 0.8, 1.0), 6.0)
    L.append(S.light_point(S.translate(1.2, 1.4, 1.8), (1.0, 0.6, 0.5), 5.0, "omni"))
    L.append(S.light_point(S.translate(-1.2, 3.2, 2.2), (0.9, 0.9, 1.0), 40.0, "spot",
                           float(np.cos(np.radians(25.0))), float(np.cos(np.radians(55.0)))))
    L.append(S.light_directional(S.rotate_x(20.0) @ S.rotate_y(40.0), (1.0, 0.95, 0.8), 0.6))
    return sc


def scene_b():
    """Scene A with what is part of C_0: a constant environment colour and an emissive quad that no light is bound to."""
    sc = scene_a()
    sc.env_color = (0.05, 0.07, 0.1, 0.0)
    emis = len(sc.materials)
    sc.materials.append(S.material_emissive((1.0, 0.5, 0.2), 2.0))
    m = S.translate(2.6, 0.6, 1.0) @ S.rotate_x(-90.0)
    sc.add_instance(sc.add_mesh(*_quad((-0.4, 0, -0.4), (0.8, 0, 0), (0, 0, 0.8)), [emis]), m)
    return sc


def many_lights_scene(count=BINS + 5):
    """`count` small omni point lights in a grid over the floor: more lights than the workgroups' bins hold."""
    sc = _base_scene()
    rng = np.random.RandomState(SEED + 1)
    side = int(np.ceil(np.sqrt(count)))
    for i in range(count):
        x, z = -3.0 + 6.0 * (i % side) / (side - 1), -2.5 + 5.0 * (i // side) / (side - 1)
        sc.lights.append(S.light_point(S.translate(x, 0.9 + 0.6 * rng.uniform(), z), tuple(rng.uniform(0.4, 1.0, 3)), 12.0, "omni"))
    return sc


def gains(n_lights, seed=SEED):
    """Random gains in [0, 2], one channel of light 1 exactly 0 and the last light all ones: float32 [n_lights, 4], the fourth float padding."""
    g = np.random.default_rng(seed).uniform(0.0, 2.0, (n_lights, 4)).astype(np.float32)
    g[:, 3] = 7.0                                                  # padding: never read
    g[1, 1] = 0.0
    g[n_lights - 1, :3] = 1.0
    return g


def scaled_lights(sc, g):
    """m_lights with intensity.rgb multiplied by g[l, :3] in float32 on the host."""
    lights = np.array(sc.lights).copy()
    for l in range(lights.size):
        lights[l]["intensity"][:3] = lights[l]["intensity"][:3] * np.asarray(g[l][:3], np.float32)
    return lights


def only_light(sc, l):
    """m_lights with every light but l scaled to 0 (l = None: all of them)."""
    g = np.zeros((len(sc.lights), 3), np.float32)
    if l is not None:
        g[l] = 1.0
    return scaled_lights(sc, g)


def adjoint(seed=SEED, shape=(HEIGHT, WIDTH)):
    """A mixed-sign image adjoint; its fourth float is not read."""
    a = np.random.default_rng(seed + 100).uniform(-1.0, 1.0, (*shape, 4)).astype(np.float32)
    a[..., 3] = -3.0
    return a


def pixel_mask(xy, tid_begin, tid_count, shape=(HEIGHT, WIDTH)):
    """[H, W] bool: the pixels threads [tid_begin, tid_begin + tid_count) render (xy: m_packedXY)."""
    m = np.zeros(shape, bool)
    sel = xy[tid_begin:tid_begin + tid_count]
    m[(sel >> 16).astype(np.int64), (sel & 0xFFFF).astype(np.int64)] = True
    return m


def expected_and_bound(a, f_l, f_0, mask, n):
    """(expected[3], bound[3]) of one light in float64: <a, F_l - F_0> and 2 (n + 8) 2^-24 sum |a| (F_l + F_0) over the pixels of `mask`.
    n = tid * spp * (traceDepth + 1): the f32 addends either side can have, the worst case of any summation order."""
    a64, fl, f0 = a[..., :3].astype(np.float64), f_l[..., :3].astype(np.float64), f_0[..., :3].astype(np.float64)
    w = mask[..., None].astype(np.float64)
    want = (a64 * (fl - f0) * w).sum(axis=(0, 1))
    bound = 2.0 * (n + 8) * 2.0 ** -24 * (np.abs(a64) * (fl + f0) * w).sum(axis=(0, 1))
    return want, bound


def lit_fraction(f_l, f_0):
    """Fraction of the pixels light l reaches: F_l - F_0 is positive in some channel."""
    return float(np.mean(np.any(f_l[..., :3] > f_0[..., :3], axis=-1)))


def emitter_pixels(f_l, light, spp):
    """Pixels that show light l's own mesh: every sample there returns the light's radiance, intensity * mult (area lights have no IES or spot term)."""
    rad = (np.asarray(light["intensity"][:3], np.float32) * np.float32(light["mult"])).astype(np.float64) * spp
    return int(np.count_nonzero(np.all(np.abs(f_l[..., :3] - rad) <= 1e-4 * rad, axis=-1)))
