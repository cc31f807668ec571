"""PathTraceDR's texture adjoint on the GPU (texFetchAD / bilinearTaps, the record packing, the staged float-atomic scatter) against the
oracle's duals, at the texture sizes and layouts of dr_texture_cases.py and under every schedule; the oracle itself is pinned by finite
differences in test_dr_textures_cpu.py. Figures per case: profiles/dr_textures.md."""
import functools

import numpy as np
import pytest

import dr_texture_cases as T
from conftest import assert_pixel_parity
from dr_texture_cases import CASES, OVERFLOW, SCHEDULES

pytestmark = pytest.mark.gpu

SPP = 4


class Run:
    """What one PathTraceDR call left behind (gens: the generators afterwards; random_gens() makes it stand in for its integrator)."""

    def __init__(self, loss, grad, frame, gens, xy, offsets):
        self.loss, self.grad, self.frame, self.gens, self.xy, self.offsets = loss, grad, frame, gens, xy, offsets

    def random_gens(self):
        return self.gens

    def packed_xy(self):
        return self.xy


def _gpu(sc, schedule):
    from hydracore3_amd.api import HipIntegrator
    gpu = HipIntegrator(sc)
    if schedule == 2:
        gpu.set_schedule(2, 56, 0, 1)
    else:
        gpu.set_schedule(schedule)                                                 # 1: megakernel, 3: megakernel with block-local ray repacking
    return gpu


def _gpu_dr(case, schedule, data, ref, tid_begin=0, tid_count=None, sc=None, fill=T.PAD_VALUE):
    sc = T.scene_of(case) if sc is None else sc
    gpu = _gpu(sc, schedule)
    offsets = T.register_gpu(gpu, case)
    frame = np.zeros((sc.height, sc.width, 4), np.float32)
    grad = np.full(data.size, fill, np.float32)
    loss = gpu.PathTraceDR(gpu.N - tid_begin if tid_count is None else tid_count, 4, frame, SPP, ref, data, grad, tid_begin=tid_begin)
    assert gpu.last_schedule()[0] == schedule
    return Run(loss, grad, frame, gpu.random_gens(), gpu.packed_xy(), offsets)


@functools.lru_cache(maxsize=None)
def gpu_run(case, schedule):
    data, ref = T.inputs(case, T.scene_of(case))
    return _gpu_dr(case, schedule, data, ref)


@functools.lru_cache(maxsize=None)
def cpu_run(case, tid_begin=0, tid_count=None):
    """The oracle's result of a case, computed once and shared."""
    from oracle.orc import OracleIntegrator
    sc = T.scene_of(case)
    cpu = OracleIntegrator(sc)
    offsets = T.register_cpu(cpu, case)
    data, ref = T.inputs(case, sc)
    loss, grad, frame = T.oracle_dr(cpu, SPP, ref, data, tid_begin, tid_count)
    return Run(loss, grad, frame, cpu.random_gens(), cpu.packed_xy(), offsets)


def _against_oracle(case, g, c, what):
    """Loss, frame, gradient norm, every gradient element, alpha elements and the tail behind the registered textures."""
    n = case.size()
    assert abs(g.loss - c.loss) <= 1e-4 * abs(c.loss), (what, g.loss, c.loss)
    assert_pixel_parity(g.frame, c.frame, SPP, g, c, max_divergent=0, what=what)
    gg, gc = g.grad[:n], c.grad[:n]
    err = float(np.linalg.norm(gg.astype(np.float64) - gc) / np.linalg.norm(gc.astype(np.float64)))
    atol = T.element_atol(gc, SPP)
    worst = T.assert_elements(case, gg, gc, atol, what)
    print(f"{what}loss gpu={g.loss:.6f} cpu={c.loss:.6f}; gradient: norm error {err:.3e}, worst element error / max|c| = {worst:.3e} "
          f"(floor {atol / np.abs(gc).max():.1e}), non-zero elements {np.count_nonzero(gc)} of {n}")
    assert err < 1e-2
    assert np.all(g.grad[T.alpha_elements(case)] == 0)
    assert np.array_equal(g.grad[n:], c.grad[n:]), (what, g.grad[n:], c.grad[n:])   # the whole a_gradSize is memset (integrator_dr.cpp:1139)
    return err, worst


@pytest.mark.parametrize("schedule", SCHEDULES)
@pytest.mark.parametrize("case", CASES, ids=repr)
def test_case_matches_oracle(case, schedule):
    g, c = gpu_run(case, schedule), cpu_run(case)
    assert g.offsets == c.offsets == [(off, w * h * ch) for off, w, h, ch in case.layout()]
    _against_oracle(case, g, c, f"{case.name}, schedule {schedule}: ")
    assert np.count_nonzero(c.grad[:case.size()]) > 0


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_second_run_overwrites_the_gradient(case):
    """a_dataGrad is overwritten, not accumulated into: another integrator, the buffer pre-filled with another value, the same gradient
    (rtol 1e-4; the atomics land in another order: atol 1e-7 max|grad|, the project's floor for the same sums in another order). And
    a_data's tail is only read."""
    data, ref = T.inputs(case, T.scene_of(case))
    first = gpu_run(case, 1)
    again = _gpu_dr(case, 1, data, ref, fill=-3.0)
    assert np.allclose(again.grad, first.grad, rtol=1e-4, atol=1e-7 * np.abs(first.grad).max())
    assert np.array_equal(again.frame.view(np.uint32), first.frame.view(np.uint32))
    assert np.all(data[case.size():] == T.PAD_VALUE)


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_schedules_agree(case):
    """Frames and generators bit for bit among the schedules; gradients to 1e-5 of the norm (float atomics in another order)."""
    runs = [gpu_run(case, s) for s in SCHEDULES]
    for r in runs[1:]:
        assert np.array_equal(r.frame.view(np.uint32), runs[0].frame.view(np.uint32))
        assert np.array_equal(r.gens, runs[0].gens)
        assert np.linalg.norm(r.grad.astype(np.float64) - runs[0].grad) <= 1e-5 * np.linalg.norm(runs[0].grad.astype(np.float64))
        assert abs(r.loss - runs[0].loss) <= 1e-5 * abs(runs[0].loss)


@pytest.mark.parametrize("schedule", SCHEDULES)
@pytest.mark.parametrize("name", ["mono_npot", "mono_pow2"])
def test_one_channel_equals_four_channels(name, schedule):
    """test_dr_textures_cpu.test_one_channel_equals_four_channels on the GPU, with its tolerances."""
    case = T.BY_NAME[name]
    data, ref = T.inputs(case, T.scene_of(case))
    one = gpu_run(case, schedule)
    four, data4 = T.as_four_channels(case, data)
    r4 = _gpu_dr(four, schedule, data4, ref)
    assert np.array_equal(one.frame.view(np.uint32), r4.frame.view(np.uint32))
    assert np.array_equal(one.gens, r4.gens)
    g1, g4 = one.grad[:case.size()], r4.grad[:four.size()].reshape(-1, 4)
    assert np.count_nonzero(g1) > case.size() // 2
    assert np.allclose(g1, g4[:, 0] + g4[:, 1] + g4[:, 2], rtol=1e-5, atol=1e-7 * np.abs(g1).max())
    assert np.all(g4[:, 3] == 0)


def test_unaligned_four_channel_texture_is_refused():
    """A four-channel texture must start at a multiple of 4 floats (its taps are float4 loads): behind 5 x 3 x 1 = 15 floats it is refused with
    an error that says so, and the first registration still works - a DR call with it alone matches the oracle."""
    from hydracore3_amd.api import HydraHipError
    from oracle.orc import OracleIntegrator
    case = T.Case("mono_15", (5, 3, 1))
    sc = T.scene_of(case)
    gpu = _gpu(sc, 1)
    assert T.register_gpu(gpu, case) == [(0, 15)]
    with pytest.raises(HydraHipError, match="multiple of 4"):
        gpu.PutDiffTex2D(T.BOX_TEX, 5, 3, 4)
    data, ref = T.inputs(case, sc)
    frame, grad = np.zeros((sc.height, sc.width, 4), np.float32), np.full(data.size, T.PAD_VALUE, np.float32)
    loss = gpu.PathTraceDR(gpu.N, 4, frame, SPP, ref, data, grad)
    g = Run(loss, grad, frame, gpu.random_gens(), gpu.packed_xy(), None)
    cpu = OracleIntegrator(sc)
    T.register_cpu(cpu, case)
    loss_c, grad_c, frame_c = T.oracle_dr(cpu, SPP, ref, data)
    _against_oracle(case, g, Run(loss_c, grad_c, frame_c, cpu.random_gens(), cpu.packed_xy(), None), "after the refusal: ")


@pytest.mark.parametrize("schedule", SCHEDULES)
def test_unaligned_windows(schedule):
    """tid windows that are not wave-aligned, [0, 200) and [200, 561), on `npot`, each from a fresh integrator into buffers of its own: the
    gradients add up to the whole frame's (same sums, another order), the frames add up bit for bit, and each half matches the oracle's same
    window."""
    case = T.BY_NAME["npot"]
    sc = T.scene_of(case)
    data, ref = T.inputs(case, sc)
    whole = gpu_run(case, schedule)
    windows = [(0, 200), (200, 361)]
    halves = [_gpu_dr(case, schedule, data, ref, b, n) for b, n in windows]
    assert np.array_equal((halves[0].frame + halves[1].frame).view(np.uint32), whole.frame.view(np.uint32))
    assert np.count_nonzero(halves[0].frame[..., :3].sum(-1)) <= 200 and np.count_nonzero(halves[1].frame[..., :3].sum(-1)) <= 361
    assert np.array_equal(np.where((np.arange(whole.gens.shape[0]) < 200)[:, None], halves[0].gens, halves[1].gens), whole.gens)
    n = case.size()
    total = halves[0].grad[:n] + halves[1].grad[:n]
    assert np.allclose(total, whole.grad[:n], rtol=1e-5, atol=1e-7 * np.abs(whole.grad[:n]).max())
    for (b, cnt), g in zip(windows, halves):
        c = cpu_run(case, b, cnt)
        what = f"npot, schedule {schedule}, paths [{b}, {b + cnt}): "
        assert abs(g.loss - c.loss) <= 1e-4 * abs(c.loss), (what, g.loss, c.loss)
        T.assert_elements(case, g.grad[:n], c.grad[:n], T.element_atol(c.grad[:n], SPP), what)
        assert np.array_equal(g.grad[n:], c.grad[n:])


@pytest.mark.parametrize("schedule", SCHEDULES)
def test_staging_overflow(schedule):
    """The closed box at depth 8: a wave's sweep stages far more than 64 (lane, bounce) columns, so the staging area is flushed mid-sweep
    (schedules 1 and 3 defer the scatter to the end of the sweep; 2 scatters level by level). The oracle's side shows that the case does what
    it is for: every non-alpha element of the texture gets gradient."""
    g, c = gpu_run(OVERFLOW, schedule), cpu_run(OVERFLOW)
    n = OVERFLOW.size()
    assert g.offsets == c.offsets == [(0, n)]
    assert np.count_nonzero(c.grad[:n]) == n // 4 * 3
    _against_oracle(OVERFLOW, g, c, f"closed box, schedule {schedule}: ")
