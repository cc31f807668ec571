"""hpt_destroy / hpt_cam_destroy after ownership moved into destructors (hpt_host.hip: ~hpt_ctx, ~WfGroup, ~hpt_cam): contexts that have
allocated the wavefront groups with their streams, events and pinned progress word are made, rendered with and dropped in one process, with and
without a camera, and a later context must render the same bytes as the first, every call answering HPT_OK (the Python front end raises
otherwise). What this can catch is a teardown that disturbs the device or the next context (a free of something still in use, a destroy that
faults); a leak passes it unnoticed."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _render_and_drop(with_cam):
    from hydracore3_amd import synth
    from hydracore3_amd.api import CamRays, HipIntegrator
    integ = HipIntegrator(synth.furnace_plane(32, 32))
    integ.set_schedule(2)                                       # the wavefront schedule: allocates a group, its stream, nine events, the pinned word
    img = integ.render(1)
    assert integ.last_schedule()[0] == 2
    if with_cam:                                                # a camera with its tile buffers and the render loop's events, destroyed before its context
        cam = CamRays(integ, 0)
        cam.SetParameters(32, 32, np.asarray(list(integ.params.projInv), np.float32), 0)
        cam.SetBatchSize(256)
        integ.InitRandomGens(integ.N)
        frame = cam.render(1)
        assert np.isfinite(frame).all()
        img = np.concatenate([img.ravel(), frame.ravel()])
        del cam
    del integ                                                   # hpt_destroy
    return np.ascontiguousarray(img, np.float32).view(np.uint32)


@pytest.mark.parametrize("with_cam", [False, True])
def test_contexts_made_and_dropped_in_one_process_render_the_same_bytes(with_cam):
    first = _render_and_drop(with_cam)
    _render_and_drop(with_cam)
    third = _render_and_drop(with_cam)
    assert first.any() and np.array_equal(first, third)
