"""numpy restatement of IntegratorKMLT's bookkeeping (mlt/integrator_kmlt.cpp) and of the pseudo generator it draws from (include/crandom.h).

Everything is vectorised over generators / chains; the steps of a chain run in order. float32 where the reference computes in float, float64
where it computes in double. Nothing here evaluates a path: F comes from the caller (a closed form in the CPU tests, the device's recorded
colours in the GPU tests).
"""
import numpy as np

F32 = np.float32
U32 = np.uint32
_SCALE = F32(1.0 / 4294967296.0)
BOUNCE_START, LGHT_ID, MATS_ID, BLND_ID, PER_BOUNCE = 6, 0, 4, 8, 10
PLARGE = F32(0.25)
MUTATE_COEFF_SCREEN, MUTATE_COEFF_BSDF = 128.0, 64.0


def _poly(x, a, b, c):
    """x * (x * x * a + b) + c in uint32 arithmetic (wraps at 2^32)."""
    with np.errstate(over="ignore"):
        return x * (x * x * U32(a) + U32(b)) + U32(c)


class Gens:
    """An array of RandomGen states (crandom.h:11-75). Every draw advances the generators `mask` selects (all by default)."""

    def __init__(self, sx, sy):
        self.sx, self.sy = np.array(sx, U32).reshape(-1), np.array(sy, U32).reshape(-1)

    @classmethod
    def from_states(cls, states):
        s = np.asarray(states, U32).reshape(-1, 2)
        return cls(s[:, 0], s[:, 1])

    @classmethod
    def init(cls, seeds):
        """RandomGenInit for seeds 0 .. 2^31 - 1 (a_seed % 7 warm-up steps)."""
        seeds = np.asarray(seeds, np.int64).reshape(-1)
        assert np.all((seeds >= 0) & (seeds < 2 ** 31))
        s = seeds.astype(U32)
        g = cls(_poly(s, 15731, 74323, 871483), _poly(s, 13734, 37828, 234234))
        warm = seeds % 7
        for i in range(6):
            g.next_state(warm > i)
        return g

    def next_state(self, mask=None):
        with np.errstate(over="ignore"):
            x = self.sx * U32(17) + self.sy * U32(13123)
            sx = (x << U32(13)) ^ x
            sy = self.sy ^ (x << U32(7))
        if mask is None:
            self.sx, self.sy = sx, sy
        else:
            self.sx, self.sy = np.where(mask, sx, self.sx), np.where(mask, sy, self.sy)
        return x

    def float1(self, mask=None):
        x = self.next_state(mask)
        return _poly(x, 15731, 74323, 871483).astype(F32) * _SCALE

    def float4(self, mask=None):
        x = self.next_state(mask)
        v = np.stack([_poly(x, 15731, 74323, 871483), _poly(x, 13734, 37828, 234234), _poly(x, 11687, 26461, 137589), _poly(x, 15707, 789221, 1376312589)], axis=-1)
        return v.astype(F32) * _SCALE

    def states(self):
        return np.stack([self.sx, self.sy], axis=-1)


def state_size(trace_depth):
    """AlignedSize(PER_BOUNCE * traceDepth + BOUNCE_START, 16)."""
    n = PER_BOUNCE * trace_depth + BOUNCE_START
    return n if n % 16 == 0 else n - n % 16 + 16


def chain_gens(chains):
    """gen1 = RandomGenInit(7 c + 1), gen2 = RandomGenInit(c), both advanced 10 + c % 17 states (:291-297)."""
    c = np.arange(chains, dtype=np.int64)
    g1, g2 = Gens.init(7 * c + 1), Gens.init(c)
    warm = 10 + c % 17
    for i in range(26):
        g1.next_state(warm > i)
        g2.next_state(warm > i)
    return g1, g2


def mutate_kelemen(value, rx, ry, p2, p1=1024.0):
    """MutateKelemen (:64-85) in float32."""
    value, rx, ry = np.asarray(value, F32), np.asarray(rx, F32), np.asarray(ry, F32)
    s1, s2 = F32(1.0) / F32(p1), F32(1.0) / F32(p2)
    power = -np.log(F32(s2 / s1))
    assert power.dtype == F32
    dv = np.maximum(s2 * (np.exp(power * np.sqrt(rx)) - np.exp(power)), F32(0.0)).astype(F32)
    up = value + dv
    up = np.where(up > F32(1.0), up - F32(1.0), up)
    dn = value - dv
    dn = np.where(dn < F32(0.0), dn + F32(1.0), dn)
    return np.where(ry < F32(0.5), up, dn).astype(F32)


def contrib_func(color):
    c = np.asarray(color, F32)
    return np.maximum(F32(0.333334) * ((c[..., 0] + c[..., 1]) + c[..., 2]), F32(0.0)).astype(F32)


def propose(x_vec, is_large, gen2):
    """The proposal of one step for every chain: x_vec [C, n] -> [C, n]; gen2 advances by n / 4 (large) or n / 2 (small) states."""
    C, n = x_vec.shape
    new = np.zeros_like(x_vec)
    small = ~is_large
    for i in range(0, n, 4):                                           # large steps: n / 4 float4 draws
        r = gen2.float4(is_large)
        new[:, i:i + 4] = np.where(is_large[:, None], r, new[:, i:i + 4])
    r1, r2 = gen2.float4(small), gen2.float4(small)
    cols = [mutate_kelemen(x_vec[:, 0], r1[:, 0], r1[:, 1], MUTATE_COEFF_SCREEN), mutate_kelemen(x_vec[:, 1], r1[:, 2], r1[:, 3], MUTATE_COEFF_SCREEN),
            mutate_kelemen(x_vec[:, 2], r2[:, 0], r2[:, 1], MUTATE_COEFF_BSDF), mutate_kelemen(x_vec[:, 3], r2[:, 2], r2[:, 3], MUTATE_COEFF_BSDF)]
    for i in range(4, n, 2):
        r = gen2.float4(small)
        cols.append(mutate_kelemen(x_vec[:, i], r[:, 0], r[:, 1], MUTATE_COEFF_BSDF))
        cols.append(mutate_kelemen(x_vec[:, i + 1], r[:, 2], r[:, 3], MUTATE_COEFF_BSDF))
    return np.where(small[:, None], np.stack(cols, axis=-1), new).astype(F32)


def run_chains(chains, steps, n, width_height, F=None, recorded=None):
    """The chains of IntegratorKMLT::PathTraceBlock (:286-444). F(x [C, n]) -> (colour [C, 3] float32, pixel [C]); or `recorded` = dict with
    initColor [C, >=3], initPixel [C], color [C, steps, >=3], pixel [C, steps]: the values of F taken from a run instead of evaluated.
    Returns the per-step records, the per-chain sums and the float64 scatter sum of the contributions with what its rounding bound needs."""
    w, h = width_height
    g1, g2 = chain_gens(chains)
    x_vec = np.stack([g2.float1() for _ in range(n)], axis=-1).astype(F32)
    out = {"init": x_vec.copy()}
    if recorded is None:
        y_color, pix = F(x_vec)
    else:
        y_color, pix = np.asarray(recorded["initColor"], F32)[:, :3], np.asarray(recorded["initPixel"])
    y_color, pix = np.asarray(y_color, F32).copy(), np.asarray(pix, np.int64).copy()
    y = contrib_func(y_color)
    out.update(initColor=y_color.copy(), initPixel=pix.copy())
    rec = {k: [] for k in ("isLarge", "accepted", "a", "color", "pixel", "oldPixel", "proposals", "contribAtX", "contribAtY", "addX", "addY")}
    accept, large = np.zeros(chains, np.int64), np.zeros(chains, np.int64)
    accum = np.zeros(chains, np.float64)
    frame = np.zeros((w * h, 3), np.float64)
    mag = np.zeros((w * h, 3), np.float64)                             # sum |x_i| per pixel and channel
    cnt = np.zeros(w * h, np.int64)                                    # additions per pixel
    for i in range(steps):
        is_large = g1.float1() < PLARGE
        x_new = propose(x_vec, is_large, g2)
        if recorded is None:
            new_color, new_pix = F(x_new)
        else:
            new_color, new_pix = np.asarray(recorded["color"], F32)[:, i, :3], np.asarray(recorded["pixel"])[:, i]
        new_color, new_pix = np.asarray(new_color, F32), np.asarray(new_pix, np.int64)
        y_new = contrib_func(new_color)
        y_old, old_color, old_pix = y, y_color, pix
        with np.errstate(divide="ignore", invalid="ignore"):
            a = np.where(y_old == F32(0.0), F32(1.0), np.minimum(F32(1.0), (y_new / y_old).astype(F32))).astype(F32)
        p = g1.float1()
        acc = p <= a
        x_vec = np.where(acc[:, None], x_new, x_vec)
        y, y_color, pix = np.where(acc, y_new, y), np.where(acc[:, None], new_color, y_color), np.where(acc, new_pix, pix)
        accept += acc
        large += is_large
        accum = np.where(is_large, accum + y_new.astype(np.float64), accum)
        k_y = (F32(1.0) / np.maximum(y_new, F32(1e-6))).astype(F32)
        k_x = (F32(1.0) / np.maximum(y_old, F32(1e-6))).astype(F32)
        at_y = ((new_color * k_y[:, None]).astype(F32) * a[:, None]).astype(F32)
        at_x = ((old_color * k_x[:, None]).astype(F32) * (F32(1.0) - a)[:, None]).astype(F32)
        dot = lambda v: ((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]).astype(F32) + v[:, 2] * v[:, 2]).astype(F32)
        add_x, add_y = dot(at_x) > F32(1e-12), dot(at_y) > F32(1e-12)
        for sel, where, val in ((add_x, old_pix, at_x), (add_y, new_pix, at_y)):
            np.add.at(frame, where[sel], val[sel].astype(np.float64))
            np.add.at(mag, where[sel], np.abs(val[sel]).astype(np.float64))
            np.add.at(cnt, where[sel], 1)
        for k, v in (("isLarge", is_large), ("accepted", acc), ("a", a), ("color", new_color), ("pixel", new_pix), ("oldPixel", old_pix),
                     ("proposals", x_new), ("contribAtX", at_x), ("contribAtY", at_y), ("addX", add_x), ("addY", add_y)):
            rec[k].append(v.copy())
    for k, v in rec.items():
        out[k] = np.stack(v, axis=1) if steps else np.zeros((chains, 0))
    out.update(accept=accept, largeSteps=large, accumBrightness=accum, frame=frame, mag=mag, count=cnt)
    return out


def normalisation(accum_brightness, large_steps, accept, frame_unnormalised, pixels_num, pass_num):
    """(:441-470) -> [avgBrightness, actualBrightness, acceptance rate, normConst]; chains without a large step are left out of the first mean;
    normConst is 1 when no chain made one or the frame is black."""
    has = large_steps > 0
    avg = float(np.mean(accum_brightness[has] / large_steps[has])) if has.any() else 0.0
    px = np.asarray(frame_unnormalised, F32).reshape(-1, 4)[:pixels_num]
    actual = float(np.sum(contrib_func(px[:, :3]).astype(np.float64)) / pixels_num)
    ok = has.any() and actual != 0.0
    norm = float(F32(pass_num) * F32(avg / actual)) if ok else 1.0
    return np.array([avg, actual, float(np.sum(accept)) / (float(pixels_num) * float(pass_num)), norm], np.float64)


def circular_distance(a, b):
    d = np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))
    return np.minimum(d, 1.0 - d)
