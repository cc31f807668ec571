"""Scenes, maps and adjoints of the environment-map tests of the differentiable integrators (test_env_grad_cpu.py, test_env_grad_gpu.py,
env_grad_torch_child.py).

The colour of a sample is affine in the texels of the environment map: the paths, the pdf table in m_arrays1f and the MIS weights do not read
the texture. So with F_k the frame under the map "texel k, channel c = 1, everything else 0" and F_0 the frame under the black map, both
tracing the paths of the frame under test, d<a, F>/d texel[k, c] = <a, F_k - F_0>: the reference of the gradient tests is made of frames.
The pdf table is the one the loader built from the fixture's own map, whatever map is rendered (`with_map` swaps the image only).
Everything is built in Python, with fixed seeds; no golden files."""
import numpy as np

from hydracore3_amd import scene as S
from hydracore3_amd import synth
from hydracore3_amd.synth import _merge, _quad

WIDTH = HEIGHT = 32
N = WIDTH * HEIGHT
SEED = 23
SCHEDULES = [1, 2]                # megakernel, wavefront
MAPS = {"4x2": (4, 2), "8x4": (8, 4)}
ROW0, ROW1 = (1.0, 0.0, 0.0, 0.0625), (0.0, 1.0, 0.0, -0.125)   # the sampler matrix: u shifted by a sixteenth of a turn, v an eighth down
ENV_COLOR = (0.9, 1.0, 1.1, 0.0)
TEX, ENV_TEX = 1, 2               # the albedo texture of the plane / of the box, the environment map
PLANE_TEX_W = PLANE_TEX_H = 4
BOX_TEX_W = BOX_TEX_H = 8
BOX_DEPTH = 3
WINDOWS = {"whole": (0, N), "unaligned": (37, 300)}     # 300 threads from 37: no wave boundary at either end, a last wave of 44 lanes


def env_image(size, seed=SEED):
    """A random RGBA32F map of MAPS[size], rgb in [0.2, 2], alpha 1."""
    w, h = MAPS[size]
    img = np.random.default_rng(seed).uniform(0.2, 2.0, (h, w, 4)).astype(np.float32)
    img[..., 3] = 1.0
    return img


def basis_image(size, k=None, c=0):
    """The black map (alpha 1), with texel k's channel c set to 1."""
    w, h = MAPS[size]
    img = np.zeros((h, w, 4), np.float32)
    img[..., 3] = 1.0
    if k is not None:
        img[k // w, k % w, c] = 1.0
    return img


def with_map(sc, img):
    """The scene with another image behind the environment map: the pdf table in m_arrays1f stays the fixture's."""
    t = sc.textures[ENV_TEX]
    sc.textures[ENV_TEX] = S.Texture(np.asarray(img, np.float32), S.TEX_RGBA32F, False, t.addr_u, t.addr_v, t.filter)
    return sc


def _albedo(w, h, seed):
    img = np.random.RandomState(seed).uniform(0.3, 0.7, (h, w, 4)).astype(np.float32)
    img[..., 3] = 1.0
    return img


def _set_env(sc, size, sample, with_env=True):
    env = S.Texture(env_image(size), S.TEX_RGBA32F, False, S.ADDR_WRAP, S.ADDR_CLAMP, S.FILTER_LINEAR)    # wrap in U, clamp in V
    assert sc.add_texture(env) == ENV_TEX
    if with_env:
        sc.set_environment(ENV_COLOR, ENV_TEX, 1.0, ROW0, ROW1, sample=sample)
    else:
        sc.env_color = ENV_COLOR
    return sc


def plane_scene(size="4x2", sample=True, depth=1):
    """(P) synth.furnace_plane with a textured gltf Lambert material under the map: every path is camera -> plane -> sky. The plane's uv run
    200 times over its 100 units, so the 4 x 4 albedo texture repeats within the view."""
    sc = synth.furnace_plane(WIDTH, HEIGHT)
    sc.trace_depth = depth
    assert sc.add_texture(S.Texture(_albedo(PLANE_TEX_W, PLANE_TEX_H, SEED + 1), S.TEX_RGBA32F, False, S.ADDR_WRAP, S.ADDR_WRAP, S.FILTER_LINEAR)) == TEX
    sc.materials[0] = S.material_lambert((0.8, 0.7, 0.9), TEX)
    p, n, t, uv, idx = _quad((-50, 0, 50), (100, 0, 0), (0, 0, -100), uv_scale=200.0)
    return _set_env(_replace_geometry(sc, (p, n, t, uv, idx)), size, sample)


def _replace_geometry(sc, mesh):
    """furnace_plane's scene with `mesh` as its only mesh and instance (a fresh SceneData: the synth scene's own quad has other uv)."""
    out = S.SceneData()
    for k in ("width", "height", "cam_pos", "cam_look_at", "cam_up", "fov", "trace_depth"):
        setattr(out, k, getattr(sc, k))
    out.textures = list(sc.textures)
    out.materials = list(sc.materials)
    out.add_instance(out.add_mesh(*mesh, [0]), np.eye(4))
    return out


def _quad4(a, b, c, d):
    """The flat quadrilateral a b c d (any four coplanar corners, in order) as two triangles; uv (0,0) (1,0) (1,1) (0,1)."""
    pos = np.asarray([a, b, c, d], np.float64)
    n = np.cross(pos[1] - pos[0], pos[3] - pos[0])
    n /= np.linalg.norm(n)
    t = (pos[1] - pos[0]) / np.linalg.norm(pos[1] - pos[0])
    pos4 = np.concatenate([pos, np.ones((4, 1))], 1).astype(np.float32)
    norm4 = np.tile(np.append(n, 0.0), (4, 1)).astype(np.float32)
    tang4 = np.tile(np.append(t, 0.0), (4, 1)).astype(np.float32)
    uv = np.asarray([[0, 0], [1, 0], [1, 1], [0, 1]], np.float32)
    return pos4, norm4, tang4, uv, np.asarray([0, 1, 2, 0, 2, 3], np.uint32)


WALL_Z = -2.5                     # the back wall of (B)
BLOCK_SLANT = 30.0                # degrees between the block's side faces and its front face


def box_scene(size="4x2", sample=True, with_env=True):
    """(B) An open box: a floor that reaches far past the view (normal +y), a back wall (+z) and, against the wall, a textured block that
    occludes both - a top (+y), a front (+z) and two sides slanted towards the camera, normals (+-sin 30, 0, cos 30); one rect light without a
    mesh; trace depth 3. No path can reach a back face: the wall and the floor end where nothing lies behind them, and a ray that passes them
    never comes back. with_env False: the same scene with the map removed (a constant environment colour)."""
    sc = S.SceneData()
    sc.width, sc.height, sc.trace_depth, sc.fov = WIDTH, HEIGHT, BOX_DEPTH, 45.0
    sc.cam_pos, sc.cam_look_at, sc.cam_up = (0.0, 2.0, 5.5), (0.0, 1.0, 0.0), (0.0, 1.0, 0.0)
    assert sc.add_texture(S.Texture(_albedo(BOX_TEX_W, BOX_TEX_H, SEED + 2), S.TEX_RGBA32F, False, S.ADDR_WRAP, S.ADDR_WRAP, S.FILTER_LINEAR)) == TEX
    sc.materials += [S.material_gltf((0.8, 0.75, 0.7, 1.0), 0.0, 0.3, 0.0, 1.5), S.material_gltf((0.85, 0.8, 0.9, 1.0), 0.5, 0.6, 1.0, 1.5, TEX)]
    sc.add_instance(sc.add_mesh(*_quad((-20, 0, 20), (40, 0, 0), (0, 0, WALL_Z - 20), 2, 2), [0]), np.eye(4))   # the floor: it ends at the wall
    sc.add_instance(sc.add_mesh(*_quad((-20, 0, WALL_Z), (40, 0, 0), (0, 8, 0)), [0]), np.eye(4))             # the wall
    cx, wf, depth, hgt = -0.3, 0.7, 1.2, 1.3
    wb = wf + depth / np.tan(np.radians(BLOCK_SLANT))          # the sides run back to the wall at 30 degrees to the front face
    zf, zb = WALL_Z + depth, WALL_Z
    fl, fr, bl, br = (cx - wf, zf), (cx + wf, zf), (cx - wb, zb), (cx + wb, zb)
    P = lambda xz, y: (xz[0], y, xz[1])
    faces = [_quad4(P(fl, 0), P(fr, 0), P(fr, hgt), P(fl, hgt)),          # front
             _quad4(P(fr, 0), P(br, 0), P(br, hgt), P(fr, hgt)),          # right side
             _quad4(P(bl, 0), P(fl, 0), P(fl, hgt), P(bl, hgt)),          # left side
             _quad4(P(fl, hgt), P(fr, hgt), P(br, hgt), P(bl, hgt))]      # top
    sc.add_instance(sc.add_mesh(*_merge([(*f, 1) for f in faces])), np.eye(4))
    sc.lights.append(S.light_rect(S.translate(1.2, 3.0, 1.5), 0.5, 0.5, (1.0, 0.95, 0.9), 6.0))
    return _set_env(sc, size, sample, with_env)


def below_horizon_texels(size="8x4"):
    """Texels of the 8 x 4 map below the horizon of every point of (B) a path can visit (the tail at a path's end is evaluated along the last
    sampled direction whether or not that ray would leave the scene, so occlusion alone does not count: the direction must be below the
    surface). Every surface normal of (B) is +y, +z or (+-sin 30, 0, cos 30), so a direction d with d.y < 0, d.z < 0 and an azimuth within 60
    degrees of -z is below all of them; rays from the camera that leave the scene pass over the wall or the far edges of the floor, above
    -12 degrees. sphereMapTo2DTexCoord gives u = atan2(d.x, d.z) / 2 pi (-z: 1/2) and v = acos(-d.y) / pi (down: 0, the horizon: 1/2); ROW0
    adds 1/16 to u, ROW1 subtracts 1/8 from v. The sampler clamps below 0 only - past the last row it wraps to row 0, which is why v is
    shifted down: 4 v' - 1/2 then stays within [0, 3] and row 0 has a weight only for 4 v' - 1/2 < 1, v < 1/2: below the horizon. Texel
    (column 4, row 0) has a weight for 8 u' - 1/2 in (3, 5): within 45 degrees of -z, 15 inside the dark sector on either side."""
    w, h = MAPS[size]
    assert (w, h) == (8, 4) and ROW0 == (1.0, 0.0, 0.0, 0.0625) and ROW1 == (0.0, 1.0, 0.0, -0.125)
    return [4]


def adjoint(seed=SEED):
    """A mixed-sign image adjoint; its fourth float is not read."""
    a = np.random.default_rng(seed + 100).uniform(-1.0, 1.0, (HEIGHT, WIDTH, 4)).astype(np.float32)
    a[..., 3] = -3.0
    return a
