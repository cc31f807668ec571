"""The camera plug-in without a GPU: the numpy restatement of both cameras (tests/camrays_reference.py) against closed forms, and the ABI
surface of the hpt_cam_* entry points (declared, bound, exported, null-safe; the unit listed in UNITS)."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np

import camrays_reference as CR
from conftest import ROOT, scene_path

sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

SYMBOLS = ["hpt_cam_create", "hpt_cam_destroy", "hpt_cam_set_parameters", "hpt_cam_set_lens", "hpt_cam_set_batch_size", "hpt_cam_make_rays_block",
           "hpt_cam_make_rays_block_dev", "hpt_cam_add_samples_contribution_block", "hpt_cam_add_samples_contribution_block_dev", "hpt_cam_read_state",
           "hpt_cam_render_dev", "hpt_cam_get_execution_time"]


def _perspective_inv(fov_deg, aspect, near, far):
    """inverse of an OpenGL-style perspective matrix (symmetric frustum), column-major float32 [16]."""
    f = 1.0 / np.tan(np.radians(fov_deg) / 2.0)
    m = np.array([[f / aspect, 0, 0, 0], [0, f, 0, 0], [0, 0, (far + near) / (near - far), 2 * far * near / (near - far)], [0, 0, -1, 0]], np.float64)
    return np.linalg.inv(m).T.astype(np.float32).reshape(16)


def double_gauss(width, height):
    """The repository's own lens: the <optical_system> of tests/golden/scenes/env_map, as the loader hands it over (film side first)."""
    from hydracore3_amd.scene import load_hydra_xml
    sc = load_hydra_xml(scene_path("env_map"), width, height)
    lines = np.ascontiguousarray(sc.lens_lines, np.float32).reshape(-1, 4)
    assert lines.shape[0] == 11 and (lines[:, 0] == 0).sum() == 1
    return lines, (np.float32(sc.phys_size[0]), np.float32(sc.phys_size[1]))


# ---- 1. ABI ---------------------------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_camera_symbols_and_the_front_ends_bind_them():
    from hydracore3_amd import api
    hdr = open(os.path.join(ROOT, "include", "hydra_hip.h")).read()
    for name in SYMBOLS:
        m = re.search(r"\b(?:int|void)\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
        assert m, f"{name} is not declared in include/hydra_hip.h"
        assert name in api.ABI, f"{name} is not in api.ABI"
        assert len(api.ABI[name][1]) == len(m.group(1).split(",")), (name, m.group(1))
    for meth in ("SetParameters", "SetBatchSize", "MakeRaysBlock", "AddSamplesContributionBlock", "GetExecutionTime", "SetLens", "render_dev",
                 "make_rays_block_dev", "add_samples_contribution_block_dev", "read_state"):
        assert hasattr(api.CamRays, meth)
    assert '("camrays", "hpt_camrays.hip", [])' in open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert os.path.exists(os.path.join(ROOT, "hydracore3_amd", "csrc", "hpt_camrays.hip"))
    cpp = open(os.path.join(ROOT, "hydracore3_amd", "csrc", "cam_rays_hip.h")).read()
    for cls in ("class CamPinHoleHIP", "class CamTableLensHIP", "SetParameters", "SetBatchSize", "MakeRaysBlock", "AddSamplesContributionBlock", "CommitDeviceData", "GetExecutionTime"):
        assert cls in cpp
    assert os.path.exists(os.path.join(ROOT, "hydracore3_amd", "hydra_hip_camrays_gpu")), "build() makes the device-camera tool"


def test_library_exports_the_camera_symbols_and_null_handles_are_refused():
    from hydracore3_amd import api
    lib = api.load_library()
    nm = subprocess.run(["nm", "-D", "--defined-only", api.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (hpt_[a-z0-9_]+)", nm))
    assert set(SYMBOLS) <= exported
    buf = (C.c_float * 16)()
    cam = C.c_void_p()
    assert lib.hpt_cam_create(None, 0, C.byref(cam)) == 1 and not cam.value       # HPT_ERR_ARG, no device touched
    lib.hpt_cam_destroy(None)
    assert lib.hpt_cam_set_parameters(None, 4, 4, buf, 0) == 1
    assert lib.hpt_cam_set_lens(None, buf, 1, 1.0, 1.0) == 1
    assert lib.hpt_cam_set_batch_size(None, 16) == 1
    assert lib.hpt_cam_make_rays_block(None, buf, buf, 1, 0) == 1
    assert lib.hpt_cam_make_rays_block_dev(None, buf, buf, 1, 0, None) == 1
    assert lib.hpt_cam_add_samples_contribution_block(None, buf, buf, 1, 2, 2, 0) == 1
    assert lib.hpt_cam_add_samples_contribution_block_dev(None, buf, buf, 1, 2, 2, 0, None) == 1
    assert lib.hpt_cam_read_state(None, None, None, None, 0) == 1
    assert lib.hpt_cam_render_dev(None, None, buf, 1, None) == 1
    assert lib.hpt_cam_get_execution_time(None, b"MakeRaysBlock", buf) == 1


# ---- 2. the generator -----------------------------------------------------------------------------------------------------------------------------
def test_generators_agree_with_the_scalar_restatement_and_the_known_answers():
    import make_fixtures as MF
    kat = json.load(open(os.path.join(ROOT, "tests", "golden", "rng_kat.json")))
    gens = CR.gens_init(200000)
    for i in (0, 1, 7, 85, 4097, 173941, 173942, 173950, 199999):            # from 173 942 the reference's int seed overflows: 32-bit wrap-around
        seed = (i + 12345 * i) & 0xFFFFFFFF
        assert (seed >= 0x80000000) == (i >= 173942)
        s = [(seed * (seed * seed * 15731 + 74323) + 871483) & MF.M, (seed * (seed * seed * 13734 + 37828) + 234234) & MF.M]
        for _ in range(seed % 7 if seed < 0x80000000 else 0):                 # a negative int seed: a_seed % 7 <= 0, no warm-up step
            MF.next_state(s)
        assert list(gens[i]) == s, i
        if seed < 0x80000000:
            assert s == MF.gen_init(seed)
    # seed 12346 * 1 is not in the known answers, seed 0 is: lane 0
    st = gens[:1].copy()
    assert list(st[0]) == kat["0"]["init"]
    for bits in kat["0"]["float4_bits"]:
        assert [int(v.view(np.uint32)[0]) for v in CR.rnd_float4(st)] == bits
    assert list(st[0]) == kat["0"]["final"]
    st1, st4 = gens[5:6].copy(), gens[5:6].copy()                               # rndFloat1 is the first component of rndFloat4 and one state step
    assert CR.rnd_float1(st1)[0] == CR.rnd_float4(st4)[0][0] and np.array_equal(st1, st4)


# ---- 3. pinhole -----------------------------------------------------------------------------------------------------------------------------------
def test_pinhole_centre_of_an_odd_frame_looks_down_minus_z():
    pi = _perspective_inv(45.0, 1.0, 0.01, 100.0)
    cam = CR.Camera(CR.PINHOLE, 7, 5, pi, False, 35)
    before = cam.gens.copy()
    pos, dr = cam.make_rays(35, 0)
    centre = 2 * 7 + 3
    # (0, 0, -1): x and y exactly; z is (z / w) * (1 / length), two roundings of the same number: within one unit in the last place of 1
    assert dr[centre, 0] == 0 and dr[centre, 1] == 0 and dr[centre, 3] == 0 and abs(float(dr[centre, 2]) + 1.0) <= 2.0 ** -24
    assert not pos.any() and np.array_equal(cam.gens, before), "RGB: origin 0, wavelength 0, the generator is not touched"
    assert np.allclose(np.linalg.norm(dr[:, :3].astype(np.float64), axis=1), 1.0, atol=2e-7)
    assert np.array_equal(dr[:, 0], -dr[::-1, 0]) and np.all(dr[:, 2] < 0)      # a symmetric projection: mirrored pixels, mirrored directions
    # the corner pixel against the closed form tan(fov / 2) * (2 * (x + .5) / W - 1)
    t = np.tan(np.radians(22.5))
    want = np.array([t * (2 * 0.5 / 7 - 1), t * (2 * 0.5 / 5 - 1), -1.0])
    want /= np.linalg.norm(want)
    assert np.abs(dr[0, :3] - want).max() < 4e-7


def test_pinhole_tiles_split_the_frame_pitch_linear_and_the_short_last_tile_is_allowed():
    pi = _perspective_inv(45.0, 70 / 38, 0.01, 100.0)
    whole = CR.Camera(CR.PINHOLE, 70, 38, pi, False, 2660).make_rays(2660, 0)[1]
    cam = CR.Camera(CR.PINHOLE, 70, 38, pi, False, 350)
    parts = [cam.make_rays(min(350, 2660 - 350 * s), s)[1] for s in range(8)]
    assert parts[-1].shape[0] == 210 and np.array_equal(np.concatenate(parts), whole)


def test_sample_wavelengths_wraps_at_830():
    w = CR.sample_wavelengths(np.array([0.0, 0.5, 0.9], np.float32))
    assert np.array_equal(w[0], np.array([360.0, 477.5, 595.0, 712.5], np.float32))
    assert np.array_equal(w[1], np.array([595.0, 712.5, 830.0, 477.5], np.float32)), "830 itself is kept; the next one wraps to 360 + 117.5"
    assert w[2, 0] == np.float32(360.0) + np.float32(0.9) * np.float32(470.0) and w[2, 1] < w[2, 0] and np.all((w >= 360) & (w <= 830))
    cam = CR.Camera(CR.PINHOLE, 8, 8, _perspective_inv(45, 1, 0.01, 100), True, 64)
    g0 = cam.gens.copy()
    pos, _ = cam.make_rays(64, 0)
    assert np.array_equal(pos[:, 3], cam.waves) and np.all((pos[:, 3] >= 360) & (pos[:, 3] <= 830)) and np.unique(pos[:, 3]).size > 32
    assert not np.array_equal(cam.gens, g0)
    pos2, _ = cam.make_rays(64, 0)
    assert not np.array_equal(pos2[:, 3], pos[:, 3]), "the second call continues the generators"


# ---- 4. the lens stack ----------------------------------------------------------------------------------------------------------------------------
def test_one_spherical_surface_behind_a_stop_obeys_snell():
    """Film at z = 0, a stop 10 mm in front of it, a spherical surface (R = 50 mm, glass 1.5 on the film side, air outside) 10 mm further. A ray
    from the on-axis film point at a small angle: the refraction at the sphere against the vector form of Snell's law in float64."""
    lines = np.array([[0.0, 0.010, 0.0, 0.004], [0.050, 0.010, 1.5, 0.008]], np.float32)
    ang = np.linspace(-0.15, 0.15, 31)
    d64 = np.stack([np.sin(ang), 0.3 * np.sin(ang), -np.cos(ang)], axis=1)
    d64 /= np.linalg.norm(d64, axis=1)[:, None]
    # in camera space the film looks down +z towards the lens (LensRearZ > 0): TraceLensesFromFilm negates z on the way in
    pos = [np.zeros(31, np.float32) for _ in range(3)]
    dr = [d64[:, 0].astype(np.float32), d64[:, 1].astype(np.float32), (-d64[:, 2]).astype(np.float32)]
    ok, p, d = CR.trace_lenses_from_film(lines, pos, dr)
    assert ok.all()
    # float64: lens space (z negated), stop at z = -0.01 passes everything here, sphere centre at z = -0.02 + 0.05
    dl = np.stack([x.astype(np.float64) for x in (dr[0], dr[1], -dr[2])], axis=1)
    c = np.array([0.0, 0.0, 0.03])
    b = -2.0 * dl @ c
    cc = c @ c - 0.05 ** 2
    t = (-b - np.sqrt(b * b - 4 * cc)) / 2.0                                    # |d| = 1
    t_alt = (-b + np.sqrt(b * b - 4 * cc)) / 2.0
    t = np.where(dl[:, 2] > 0, np.minimum(t, t_alt), np.maximum(t, t_alt))       # useCloserT = (rayDir.z > 0) != (radius < 0)
    hit = t[:, None] * dl
    n = hit - c
    n /= np.linalg.norm(n, axis=1)[:, None]
    n = np.where((np.sum(n * -dl, axis=1) < 0)[:, None], -n, n)
    wi = -dl
    cos_i = np.sum(n * wi, axis=1)
    eta = 1.5
    cos_t = np.sqrt(1 - eta * eta * (1 - cos_i ** 2))
    wt = -eta * wi + (eta * cos_i - cos_t)[:, None] * n
    got = np.stack([d[0], d[1], -d[2]], axis=1).astype(np.float64)
    assert np.abs(got - wt).max() < 8 * 2.0 ** -24, np.abs(got - wt).max()
    assert np.allclose(np.stack([p[0], p[1], -p[2]], axis=1), hit, atol=1e-8)
    # Snell itself: n1 sin(i) = n2 sin(t) about the normal
    sin_i = np.linalg.norm(np.cross(n, wi), axis=1)
    sin_t = np.linalg.norm(np.cross(n, got / np.linalg.norm(got, axis=1)[:, None]), axis=1)
    assert np.abs(1.5 * sin_i - sin_t).max() < 1e-6


def test_a_ray_aimed_outside_an_aperture_is_the_sentinel():
    """A rear element of 8 mm semi-diameter in front of a 3 mm stop: rays are aimed all over the rear element, the stop lets the central ones through."""
    lines = np.array([[0.050, 0.010, 1.5, 0.008], [0.0, 0.010, 0.0, 0.003]], np.float32)
    cam = CR.Camera(CR.TABLE_LENS, 16, 16, _perspective_inv(45, 1, 0.01, 100), False, 256, lines=lines, phys_size=(0.004, 0.004))
    pos, dr = cam.make_rays(256, 0)
    blocked = ~cam.passed
    assert blocked.sum() > 64 and cam.passed.sum() >= 8
    assert np.all(pos[blocked, :3] == CR.SENTINEL_POS) and np.all(dr[blocked, :3] == CR.SENTINEL_DIR)
    # a ray that passed left through the stop: its origin is the negated point in the stop's plane, 20 mm from the film, inside the 3 mm hole
    out = pos[~blocked]
    assert np.all(np.hypot(out[:, 0], out[:, 1]) <= 0.003 * (1 + 1e-6)) and np.allclose(out[:, 2], -0.020, atol=1e-8)
    assert np.all((cam.cos4 > 0) & (cam.cos4 <= 1))


def test_double_gauss_passes_about_sixty_percent_and_the_flags_do_not_depend_on_the_last_bits_of_sin_and_cos():
    """The estimates quoted in profiles/camrays.md: 60 .. 62 % of the rays leave the stack; moving sin / cos by +-2 ulp changes no pass / blocked
    flag and moves unit directions by at most 4e-7."""
    pi = _perspective_inv(45.0, 64 / 48, 0.01, 100.0)
    for (w, h) in ((32, 32), (64, 48)):
        lines, phys = double_gauss(w, h)
        base = CR.Camera(CR.TABLE_LENS, w, h, pi, False, w * h, lines=lines, phys_size=phys)
        pos, dr = base.make_rays(w * h, 0)
        share = base.passed.mean()
        print(f"{w}x{h}: {100 * share:.2f} % of the rays pass the double-Gauss")
        assert 0.60 <= share <= 0.62
        assert np.allclose(np.linalg.norm(dr[:, :3].astype(np.float64), axis=1), 1.0, atol=3e-7)
    worst, flips = 0.0, 0
    for trial in range(1, 9):
        c = CR.Camera(CR.TABLE_LENS, w, h, pi, False, w * h, lines=lines, phys_size=phys, trig_ulps=2, trig_seed=trial)
        p2, d2 = c.make_rays(w * h, 0)
        flips += int((c.passed != base.passed).sum())
        both = c.passed & base.passed
        worst = max(worst, float(np.abs(d2[both, :3] - dr[both, :3]).max()))
    print(f"sin / cos moved by +-2 ulp, 8 trials: {flips} flags changed, directions moved by at most {worst:.3e}")
    assert flips == 0 and worst <= 4e-7
    rounded = CR.Camera(CR.TABLE_LENS, w, h, pi, False, w * h, lines=lines, phys_size=phys, rounded=True)
    p3, d3 = rounded.make_rays(w * h, 0)
    assert np.array_equal(rounded.passed, base.passed)


# ---- 5. contribution ------------------------------------------------------------------------------------------------------------------------------
def test_contribution_leaves_alpha_and_the_pixels_outside_the_tile_alone():
    pi = _perspective_inv(45.0, 1.0, 0.01, 100.0)
    rs = np.random.RandomState(11)
    for kind in (CR.PINHOLE, CR.TABLE_LENS):
        lines, phys = double_gauss(16, 12)
        cam = CR.Camera(kind, 16, 12, pi, False, 50, lines=lines, phys_size=phys)
        frame = rs.rand(12, 16, 4).astype(np.float32)
        before = frame.copy()
        colors = rs.rand(50, 4).astype(np.float32)
        cam.make_rays(50, 1)
        cam.contribute(frame, colors, 50, 1)
        flat, b = frame.reshape(-1, 4), before.reshape(-1, 4)
        assert np.array_equal(flat[:, 3], b[:, 3]), "alpha is untouched"
        assert np.array_equal(flat[:50], b[:50]) and np.array_equal(flat[100:], b[100:]), "only pixels 50 .. 99 belong to sub-pass 1"
        scale = cam.cos4[:50, None] if kind == CR.TABLE_LENS else np.float32(1.0)
        assert np.array_equal(flat[50:100, :3], (b[50:100, :3] + (colors[:, :3] * scale).astype(np.float32)).astype(np.float32))


def test_spectral_contribution_of_a_flat_spectrum_is_grey_of_the_cie_sums():
    from hydracore3_amd.scene import cie_xyz_fit
    cie = cie_xyz_fit()
    waves = np.arange(360, 831, dtype=np.float32)
    rgb = CR.spectrum_to_rgb(np.ones(471, np.float32), waves, cie).astype(np.float64)
    xyz = cie[:, :3].astype(np.float64) * 470.0 / 106.856895                      # value / pdf, the four equal samples averaged, / CIE_Y_integral
    m = np.array([[3.240479, -1.537150, -0.498535], [-0.969256, 1.875991, 0.041556], [0.055648, -0.204043, 1.057311]])
    assert np.abs(rgb - xyz @ m.T).max() < 1e-4 * np.abs(xyz).max()
    mean = rgb.mean(axis=0)                                                       # a flat spectrum, uniformly sampled: the equal-energy white
    assert np.abs(mean - np.array([1.205, 0.948, 0.909])).max() < 0.03              # illuminant E in linear sRGB primaries (D65 white): slightly pink
    # half a nanometre rounds to the next table entry; outside the table the observer is zero
    assert np.array_equal(CR.spectrum_to_rgb(np.ones(1, np.float32), np.array([500.5], np.float32), cie), CR.spectrum_to_rgb(np.ones(1, np.float32), np.array([501.0], np.float32), cie))
    assert not CR.spectrum_to_rgb(np.ones(1, np.float32), np.array([831.0], np.float32), cie).any()
