"""EvalGBuffer without a GPU: the numpy float32 restatement (tests/gbuffer_reference.py) pinned against things known independently of it -
the Hammersley points written out by hand, reductions of hand-built sample sets, a closed-form scene - and the record layout of the Python
front end against the C header."""
import os
import re

import numpy as np

import gbuffer_reference as R
from conftest import ROOT
from hydracore3_amd import scene as S
from hydracore3_amd import synth
from hydracore3_amd.api import GBUFFER_DTYPE


def test_hammersley_points_are_the_bit_reversal_values():
    u = [0, 1 / 2, 1 / 4, 3 / 4, 1 / 8, 5 / 8, 3 / 8, 7 / 8, 1 / 16, 9 / 16, 5 / 16, 13 / 16, 3 / 16, 11 / 16, 7 / 16, 15 / 16]
    h = R.plane_hammersley()
    assert h.dtype == np.float32 and h.shape == (16, 2)
    assert h[:, 0].tolist() == u                                         # dyadic rationals: exact in float32
    assert h[:, 1].tolist() == [(k + 0.5) / 16 for k in range(16)]


def _hit(depth, norm, obj, inst, mat, rgb):
    s = np.zeros((), GBUFFER_DTYPE)
    s["depth"], s["norm"], s["rgba"], s["coverage"] = depth, norm, (*rgb, 1.0), 1.0
    s["objId"], s["instId"], s["matId"] = obj, inst, mat
    return s


def _miss():
    s = np.zeros((), GBUFFER_DTYPE)
    s["norm"] = (0, 0, 1)
    s["objId"] = s["instId"] = s["matId"] = -1
    return s


def _reduce(samples):
    out, win = R.reduce_samples(np.array(samples, GBUFFER_DTYPE).reshape(1, 16), 64, 64)
    return out[0], int(win[0])


def test_reduction_of_sixteen_identical_hits():
    a = _hit(3.0, (0, 1, 0), 2, 5, 7, (0.25, 0.5, 0.75))
    out, win = _reduce([a] * 16)
    assert win == 0 and out["coverage"] == 1.0
    assert out["rgba"].tolist() == [0.25, 0.5, 0.75, 1.0] and out["depth"] == 3.0 and (out["objId"], out["instId"], out["matId"]) == (2, 5, 7)


def test_reduction_of_sixteen_misses():
    out, win = _reduce([_miss()] * 16)
    assert win == 0 and out["coverage"] == 1.0                           # thisDiff is 0 between two misses
    assert (out["objId"], out["instId"], out["matId"]) == (-1, -1, -1) and out["depth"] == 0.0 and out["rgba"].tolist() == [0, 0, 0, 0]


def test_reduction_majority_wins_with_its_coverage_and_the_mean_colour():
    a, b = _hit(3.0, (0, 1, 0), 1, 1, 1, (1.0, 0.0, 0.5)), _hit(3.0, (0, 1, 0), 2, 2, 2, (0.0, 1.0, 0.5))
    samples = [b, a, a, b, a, a, a, b, a, a, a, b, a, a, a, a]           # 12 of A, 4 of B, B first
    out, win = _reduce(samples)
    assert win == 1 and out["objId"] == 1                                # the first sample of A
    assert out["coverage"] == np.float32(12 / 16)
    assert out["rgba"].tolist() == [12 / 16, 4 / 16, 0.5, 1.0]           # the 16-term mean (dyadic: exact)


def test_reduction_tie_goes_to_the_first_group():
    a, b = _hit(3.0, (0, 1, 0), 1, 1, 1, (1.0, 0.0, 0.0)), _hit(3.0, (0, 1, 0), 2, 2, 2, (0.0, 1.0, 0.0))
    out, win = _reduce([b] * 8 + [a] * 8)
    assert win == 0 and out["objId"] == 2 and out["coverage"] == 0.5     # strict <: the later equal sum does not replace the first
    out, win = _reduce([a, b] * 8)
    assert win == 0 and out["objId"] == 1 and out["coverage"] == 0.5


def test_gbuff_diff_is_not_symmetric():
    """The pixel size comes from s1.depth: a near sample sees a far one as another surface before the far one does."""
    near, far = _hit(1.0, (0, 1, 0), 1, 1, 1, (0, 0, 0)), _hit(1.05, (0, 1, 0), 1, 1, 1, (0, 0, 0))
    n, f = np.array([near], GBUFFER_DTYPE), np.array([far], GBUFFER_DTYPE)
    assert R.gbuff_diff(n, f, 64, 64)[0] != R.gbuff_diff(f, n, 64, 64)[0]


def _facing_quad(width=40, height=24, d=2.0):
    """A quad in the plane y = 0, seen from (0, d, 0) straight down: it fills the view."""
    sc = S.SceneData()
    sc.width, sc.height = width, height
    sc.cam_pos, sc.cam_look_at, sc.cam_up = (0.0, d, 0.0), (0.0, 0.0, 0.0), (0.0, 0.0, -1.0)
    sc.fov, sc.trace_depth = 40.0, 1
    sc.materials.append(S.material_lambert((0.2, 0.5, 0.9)))
    p, n, t, uv, idx = synth._quad((-4, 0, 4), (8, 0, 0), (0, 0, -8))
    sc.add_instance(sc.add_mesh(p, n, t, uv, idx, [0]), np.eye(4))
    return sc


def test_closed_form_fronto_parallel_quad():
    """norm = the quad's normal, depth = d / cos(theta) of the winning sample's ray, coverage 1, constant ids.
    Bound on depth: the ray direction (two normalisations, two matrix products) and the triangle test's t (a dozen float32 operations on
    quantities within 2^3 of the result) each carry a few 2^-24 relative; 64 * 2^-24 = 3.8e-6 is taken."""
    from oracle.orc import OracleIntegrator
    d = 2.0
    sc = _facing_quad(d=d)
    cpu = OracleIntegrator(sc)
    frame, raw = R.eval_gbuffer(sc, cpu)
    red, win = R.reduce_samples(raw, sc.width, sc.height)
    assert frame.shape == (sc.height, sc.width)
    assert np.all(frame["coverage"] == 1.0)
    assert np.all(frame["objId"] == 0) and np.all(frame["instId"] == 0) and np.all(frame["matId"] == 0)
    assert np.all(frame["norm"] == np.array([0, 1, 0], np.float32))
    assert np.all(frame["rgba"][..., 3] == 1.0)
    assert np.allclose(frame["rgba"][..., :3], np.array([0.2, 0.5, 0.9], np.float32), rtol=1e-6, atol=0)
    xy = cpu.packed_xy()
    _, dr = R.eye_rays(cpu.params, xy)
    cos_theta = -dr[np.arange(xy.size), win, 1].astype(np.float64)       # the plane's normal is +y, the camera looks along -y
    assert np.all(cos_theta > 0.7)                                       # fov 40 degrees, aspect 5:3: the corner rays are 35 degrees off axis
    want = d / cos_theta
    got = red["depth"].astype(np.float64)
    rel = np.abs(got - want) / want
    print("closed form: worst relative depth error", rel.max())
    assert rel.max() < 64 * 2.0 ** -24


def test_record_layout_matches_the_header():
    assert GBUFFER_DTYPE.itemsize == 60
    hdr = open(os.path.join(ROOT, "include", "hydra_hip.h")).read()
    body = re.search(r"typedef\s+struct\s+hpt_gbuffer_pixel\s*\{(.*?)\}\s*hpt_gbuffer_pixel\s*;", hdr, re.S).group(1)
    offsets, off = {}, 0
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        ctype, names = decl.split(None, 1)
        assert ctype in ("float", "int32_t", "uint32_t"), ctype          # every member is one dword wide
        for name in (n.strip() for n in names.split(",")):
            m = re.fullmatch(r"(\w+)(?:\[(\d+)\])?", name)
            offsets[m.group(1)] = (off, ctype, int(m.group(2) or 1))
            off += 4 * int(m.group(2) or 1)
    assert off == 60
    assert set(offsets) == set(GBUFFER_DTYPE.names)
    for name, (o, ctype, count) in offsets.items():
        dt, fo = GBUFFER_DTYPE.fields[name][:2]
        assert fo == o, (name, fo, o)
        assert dt.base == (np.float32 if ctype == "float" else np.int32) and int(np.prod(dt.shape, dtype=int)) == count
    assert list(GBUFFER_DTYPE.names) == ["depth", "norm", "texc", "rgba", "shadow", "coverage", "matId", "objId", "instId"]


def test_python_front_end_declares_the_entry_points():
    from hydracore3_amd import api
    assert "hpt_eval_gbuffer" in api.ABI and "hpt_eval_gbuffer_dev" in api.ABI
    assert hasattr(api.HipIntegrator, "EvalGBuffer")
