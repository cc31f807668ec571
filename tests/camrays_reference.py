"""numpy float32 restatement of the camera plug-in's two cameras: kernel1D_MakeEyeRay and kernel1D_ContribSample of CamPinHole
(cam_plugin/CamPinHole.cpp:52-131) and CamTableLens (cam_plugin/CamTableLens.cpp:15-52, 128-319), with their per-lane state. Not a test.

Every product, sum, quotient and square root below is ONE float32 operation on float32 arrays in the order the reference's source gives them
(no fused multiply-add; numpy's '/' and sqrt are correctly rounded), vectorised over the lanes of a tile. float64 stands exactly where the
reference has double: the discriminant of Quadratic and its root. RandomGen is the integer arithmetic of include/crandom.h:17-75 on uint32
arrays (the scalar restatement tests/golden/make_fixtures.py pins the same numbers). Nothing here calls the HIP library or comes from it.

Definitions the reference leaves open:
 1. the seed of lane i is i + 12345 * i with 32-bit wrap-around, taken as the int RandomGenInit is given (the reference's int overflows from
    i = 173 942); a negative seed makes no warm-up step (its a_seed % 7 is <= 0);
 2. a tile may be shorter than the batch: lane tid serves pixel subPassId * batchSize + tid (the reference multiplies by in_blockSize and
    only ever passes the batch size);
 3. the table lens' SpectrumToXYZ call (CamTableLens.cpp:309, seven arguments, not declared anywhere) is the pinhole's six-argument call.

The only transcendental is MapSamplesToDisc's sin / cos (qmc_reference.map_samples_to_disc); `rounded` picks the correctly rounded pair instead of
numpy's float32 routines, `trig_ulps` moves r * sin and r * cos by up to that many units in the last place (the sensitivity estimate in profiles/camrays.md).
"""
import numpy as np

from gbuffer_reference import _a, _mul4x4, _normalize, f32
from qmc_reference import map_samples_to_disc

PINHOLE, TABLE_LENS = 0, 1
LAMBDA_MIN, LAMBDA_MAX = f32(360.0), f32(830.0)
SENTINEL_POS = np.array([0.0, -10000000.0, 0.0], np.float32)
SENTINEL_DIR = np.array([0.0, -1.0, 0.0], np.float32)
CIE_Y_INTEGRAL = f32(106.856895)
u32 = np.uint32


# ---- include/crandom.h ----------------------------------------------------------------------------------------------------------------------------
def next_state(state):
    """NextState on uint32 [n, 2] in place; returns x."""
    with np.errstate(over="ignore"):
        x = state[:, 0] * u32(17) + state[:, 1] * u32(13123)
        state[:, 0] = (x << u32(13)) ^ x
        state[:, 1] ^= (x << u32(7))
    return x


def gens_init(n):
    """m_randomGens[i] = RandomGenInit(i + 12345 * i) for i < n (definition 1): uint32 [n, 2]."""
    with np.errstate(over="ignore"):
        i = np.arange(n, dtype=np.uint32)
        seed = i + u32(12345) * i
        st = np.stack([seed * (seed * seed * u32(15731) + u32(74323)) + u32(871483),
                       seed * (seed * seed * u32(13734) + u32(37828)) + u32(234234)], axis=1).astype(np.uint32)
    s = seed.view(np.int32).astype(np.int64)
    warm = np.where(s > 0, s % 7, 0)                                      # C's % truncates: <= 0 for a negative seed, the loop does not run
    for k in range(6):
        sel = np.flatnonzero(warm > k)
        if sel.size:
            sub = st[sel]
            next_state(sub)
            st[sel] = sub
    return st


def _poly(x, a, b, c):
    with np.errstate(over="ignore"):
        return x * (x * x * u32(a) + u32(b)) + u32(c)


_SCALE = f32(1.0) / f32(4294967296.0)


def rnd_float4(state):
    x = next_state(state)
    return [_a(_poly(x, *abc).astype(np.float32) * _SCALE) for abc in ((15731, 74323, 871483), (13734, 37828, 234234), (11687, 26461, 137589), (15707, 789221, 1376312589))]


def rnd_float1(state):
    return _a(_poly(next_state(state), 15731, 74323, 871483).astype(np.float32) * _SCALE)


# ---- spectrum.h -----------------------------------------------------------------------------------------------------------------------------------
def sample_wavelengths(u, a=LAMBDA_MIN, b=LAMBDA_MAX):
    """SampleWavelengths (spectrum.h:58-75): float32 [n, 4]."""
    u = _a(np.atleast_1d(u))
    r = [_a(a + _a(u * f32(b - a)))]                                      # lerp(a, b, u) = a + u * (b - a)
    delta = f32(f32(b - a) / f32(4.0))
    for _ in range(3):
        nx = _a(r[-1] + delta)
        r.append(np.where(nx > b, _a(a + _a(nx - b)), nx).astype(np.float32))
    return np.stack(r, axis=1)


def spectrum_to_rgb(data, wave, cie):
    """SpectrumToXYZ(float4(data), float4(wave), 360, 830, cie, false) + XYZToRGB (spectrum.h:151-219): float32 [n, 3]."""
    cie = np.ascontiguousarray(cie, np.float32).reshape(-1, 4)
    pdf = f32(f32(1.0) / f32(LAMBDA_MAX - LAMBDA_MIN))
    s = _a(_a(data) / pdf)
    off = _a(np.floor(_a(_a(wave) + f32(0.5))) - LAMBDA_MIN).astype(np.int64)
    ok = (off >= 0) & (off < 471) & (off < cie.shape[0])
    c = np.where(ok[:, None], cie[np.clip(off, 0, cie.shape[0] - 1), :3], f32(0.0)).astype(np.float32)
    xyz = []
    for k in range(3):
        v = _a(c[:, k] * s)
        xyz.append(_a(_a(_a(_a(_a(v + v) + v) + v) / f32(4.0)) / CIE_Y_INTEGRAL))
    x, y, z = xyz
    r = _a(_a(_a(f32(3.240479) * x) - _a(f32(1.537150) * y)) - _a(f32(0.498535) * z))      # XYZToRGB, term by term from the left
    g = _a(_a(_a(f32(-0.969256) * x) + _a(f32(1.875991) * y)) + _a(f32(0.041556) * z))
    b = _a(_a(_a(f32(0.055648) * x) - _a(f32(0.204043) * y)) + _a(f32(1.057311) * z))
    return np.stack([r, g, b], axis=1)


# ---- CamTableLens.cpp:15-52, 128-215 --------------------------------------------------------------------------------------------------------------
def quadratic(A, B, C):
    """Quadratic: (ok, t0, t1). discrim and its root in double; the root rounded to float; q = -.5 * (B -+ root): the float difference times
    a double power of two, rounded to float."""
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        A64, B64, C64 = A.astype(np.float64), B.astype(np.float64), C.astype(np.float64)
        discrim = B64 * B64 - np.float64(4.0) * A64 * C64
        ok = ~(discrim < 0.0)
        root = np.sqrt(np.where(ok, discrim, 0.0)).astype(np.float32)
        q = np.where(B < 0, (np.float64(-0.5) * _a(B - root).astype(np.float64)).astype(np.float32),
                     (np.float64(-0.5) * _a(B + root).astype(np.float64)).astype(np.float32)).astype(np.float32)
        t0, t1 = _a(q / A), _a(C / q)
        swap = t0 > t1
        return ok, np.where(swap, t1, t0).astype(np.float32), np.where(swap, t0, t1).astype(np.float32)


def _dot(a, b):
    return _a(_a(a[0] * b[0] + a[1] * b[1]) + a[2] * b[2])


def trace_lenses_from_film(lines, pos, dr):
    """TraceLensesFromFilm for rays (pos, dr: lists of three float32 arrays, camera space): (passed, pos, dir)."""
    lines = np.ascontiguousarray(lines, np.float32).reshape(-1, 4)
    n = pos[0].shape[0]
    alive = np.ones(n, bool)
    p = [pos[0].copy(), pos[1].copy(), _a(-pos[2])]
    d = [dr[0].copy(), dr[1].copy(), _a(-dr[2])]
    element_z = f32(0.0)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for i in range(lines.shape[0]):
            radius, thickness, eta, aperture = (f32(v) for v in lines[i])
            element_z = f32(element_z - thickness)
            is_stop = radius == f32(0.0)
            nrm = [np.zeros(n, np.float32) for _ in range(3)]
            if is_stop:
                alive &= ~(d[2] >= f32(0.0))
                t = _a(_a(element_z - p[2]) / d[2])
            else:
                z_center = f32(element_z + radius)
                o = [p[0], p[1], _a(p[2] - z_center)]                     # rayPos - float3(0, 0, zCenter): x - 0 and y - 0 are exact
                A = _dot(d, d)
                B = _a(f32(2.0) * _dot(d, o))
                C = _a(_dot(o, o) - f32(radius * radius))
                ok, t0, t1 = quadratic(A, B, C)
                alive &= ok
                closer = (d[2] > f32(0.0)) != bool(radius < f32(0.0))
                lo = np.where(t1 < t0, t1, t0)                           # std::min(a, b) = b < a ? b : a
                hi = np.where(t0 < t1, t1, t0)                           # std::max(a, b) = a < b ? b : a
                t = np.where(closer, lo, hi).astype(np.float32)
                alive &= ~(t < f32(0.0))
                nrm = list(_normalize(_a(o[0] + t * d[0]), _a(o[1] + t * d[1]), _a(o[2] + t * d[2])))
                flip = _dot(nrm, [_a(f32(-1.0) * c) for c in d]) < f32(0.0)   # faceforward(n, -1.0f * rayDir)
                nrm = [np.where(flip, _a(f32(-1.0) * c), c).astype(np.float32) for c in nrm]
            hit = [_a(p[c] + t * d[c]) for c in range(3)]
            r2 = _a(hit[0] * hit[0] + hit[1] * hit[1])
            alive &= ~(r2 > f32(aperture * aperture))
            p = hit
            if not is_stop:
                eta_t = f32(1.0) if i == lines.shape[0] - 1 else f32(lines[i + 1, 2])
                if eta_t == f32(0.0):
                    eta_t = f32(1.0)
                e = f32(eta / eta_t)
                wi = list(_normalize(*[_a(f32(-1.0) * c) for c in d]))
                cos_i = _dot(nrm, wi)
                s2i = _a(f32(1.0) - _a(cos_i * cos_i))
                s2i = np.where(f32(0.0) < s2i, s2i, f32(0.0)).astype(np.float32)   # std::max(float(0), x)
                s2t = _a(f32(e * e) * s2i)
                alive &= ~(s2t >= f32(1.0))
                cos_t = np.sqrt(_a(f32(1.0) - s2t))
                k1 = f32(e * f32(-1.0))
                k2 = _a(_a(e * cos_i) - cos_t)
                d = [_a(_a(k1 * wi[c]) + _a(k2 * nrm[c])) for c in range(3)]
    return alive, [p[0], p[1], _a(-p[2])], [d[0], d[1], _a(-d[2])]


# ---- the cameras ----------------------------------------------------------------------------------------------------------------------------------
class Camera:
    """One ICamRaysAPI2 camera with its per-lane state: gens uint32 [batch, 2], waves / cos4 float32 [batch]."""

    def __init__(self, kind, width, height, proj_inv, spectral, batch, lines=None, phys_size=(0.0, 0.0), cie=None, rounded=False, trig_ulps=0, trig_seed=0):
        self.kind, self.width, self.height, self.spectral, self.batch = kind, int(width), int(height), bool(spectral), int(batch)
        self.proj_inv = np.asarray(list(proj_inv), np.float32).reshape(16)
        self.lines = None if lines is None else np.ascontiguousarray(lines, np.float32).reshape(-1, 4)
        self.phys_size = (f32(phys_size[0]), f32(phys_size[1]))
        self.cie = cie
        self.rounded, self.trig_ulps, self.trig_seed = rounded, int(trig_ulps), int(trig_seed)
        self.gens = gens_init(batch)
        self.waves = np.zeros(batch, np.float32)
        self.cos4 = np.zeros(batch, np.float32)
        self.film = None                                                  # the last tile's film points (table lens), for the tests' bookkeeping

    def pixels(self, n, sub_pass):
        assert n <= self.batch and sub_pass * self.batch + n <= self.width * self.height
        p = np.arange(n, dtype=np.int64) + sub_pass * self.batch
        return p % self.width, p // self.width, p

    def _film_coords(self, n, sub_pass):
        x, y, _ = self.pixels(n, sub_pass)
        xn = _a(_a(x.astype(np.float32) + f32(0.5)) / f32(self.width))
        yn = _a(_a(y.astype(np.float32) + f32(0.5)) / f32(self.height))
        return xn, yn

    def make_rays(self, n, sub_pass):
        """MakeRaysBlock: (RayPosAndW [n, 4], RayDirAndT [n, 4]); advances the state. Table lens: self.passed [n] says which rays left the stack."""
        xn, yn = self._film_coords(n, sub_pass)
        zero, one = np.zeros(n, np.float32), np.ones(n, np.float32)
        wave = zero.copy()
        if self.kind == PINHOLE:
            px, py, pz, pw = _mul4x4(self.proj_inv, _a(f32(2.0) * xn - f32(1.0)), _a(f32(2.0) * yn - f32(1.0)), zero, one)   # EyeRayDirNormalized
            dx, dy, dz = _normalize(_a(px / pw), _a(py / pw), _a(pz / pw))
            ox, oy, oz = zero, zero, zero
            if self.spectral:
                st = self.gens[:n].copy()
                wave = sample_wavelengths(rnd_float1(st))[:, 0]
                self.gens[:n] = st
            self.waves[:n] = wave
        else:
            st = self.gens[:n].copy()
            rx, ry, rz, _ = rnd_float4(st)
            self.gens[:n] = st
            if self.spectral:
                wave = sample_wavelengths(rz)[:, 0]
            fx = _a(f32(f32(0.25) * self.phys_size[0]) * _a(f32(2.0) * xn - f32(1.0)))
            fy = _a(f32(f32(0.25) * self.phys_size[1]) * _a(f32(2.0) * yn - f32(1.0)))
            self.film = (fx, fy)
            rear_z, rear_r = f32(self.lines[0, 1]), f32(self.lines[0, 3])
            sx, sy = map_samples_to_disc(_a(rx - f32(0.5)), _a(ry - f32(0.5)), self.rounded)
            if self.trig_ulps:                                            # sensitivity probe: sin / cos moved by a few units in the last place
                rs = np.random.RandomState(self.trig_seed)
                for arr in (sx, sy):
                    steps = rs.randint(-self.trig_ulps, self.trig_ulps + 1, size=n)
                    arr[...] = (arr.view(np.int32) + steps.astype(np.int32)).view(np.float32)
            k = f32(rear_r * f32(2.0))
            tx, ty = _a(k * sx), _a(k * sy)
            fdx, fdy, fdz = _normalize(_a(tx - fx), _a(ty - fy), _a(np.full(n, rear_z, np.float32) - zero))
            cos_theta = np.abs(fdz)
            ok, p, d = trace_lenses_from_film(self.lines, [fx, fy, zero], [fdx, fdy, fdz])
            nd = _normalize(*d)
            with np.errstate(invalid="ignore"):
                dx, dy, dz = [np.where(ok, _a(f32(-1.0) * c), s).astype(np.float32) for c, s in zip(nd, SENTINEL_DIR)]
                ox, oy, oz = [np.where(ok, _a(f32(-1.0) * c), s).astype(np.float32) for c, s in zip(p, SENTINEL_POS)]
            self.passed = ok
            self.waves[:n] = wave
            self.cos4[:n] = _a(_a(_a(cos_theta * cos_theta) * cos_theta) * cos_theta)
        pos = np.ascontiguousarray(np.stack([ox, oy, oz, wave], axis=1), np.float32)
        dr = np.ascontiguousarray(np.stack([dx, dy, dz, zero], axis=1), np.float32)
        return pos, dr

    def contribute(self, frame, colors, n, sub_pass):
        """AddSamplesContributionBlock: frame float32 [height, width, 4] changed in place; colors [n, 4], or [n] in spectral mode."""
        _, _, p = self.pixels(n, sub_pass)
        flat = frame.reshape(-1, 4)
        if self.spectral:
            data = _a(np.ascontiguousarray(colors, np.float32).reshape(-1)[:n])
            if self.kind == TABLE_LENS:
                data = _a(data * self.cos4[:n])
            rgb = spectrum_to_rgb(data, self.waves[:n], self.cie)
        else:
            rgb = _a(np.ascontiguousarray(colors, np.float32).reshape(-1, 4)[:n, :3])
            if self.kind == TABLE_LENS:
                rgb = _a(rgb * self.cos4[:n, None])
        flat[p, :3] = _a(flat[p, :3] + rgb)
        return frame
