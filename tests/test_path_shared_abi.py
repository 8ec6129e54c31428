"""Host-side checks of the shared-preprocess knob of gsr_render_path (include/gsr.h,
GSR_TUNE_PATH_SHARED_PRE and the read-only launch counter): number, default, get / set,
range; and the path calls' argument errors, which return before any device work — so these
run without a GPU (the GPU behaviour is tests/test_gpu_path_shared.py)."""
import ctypes

import pytest

KNOB, LAUNCHES = 34, 35


def test_knob_number_default_and_range(gsr):
    r = gsr.Renderer()
    assert (gsr.TUNE_PATH_SHARED_PRE, gsr.TUNE_PATH_SHARED_LAUNCHES) == (KNOB, LAUNCHES)
    assert r.get_tuning(KNOB) == 1                # shared by default
    assert r.get_tuning(LAUNCHES) == 0            # nothing rendered yet
    for v in (0, 1, 0):
        r.set_tuning(KNOB, v)
        assert r.get_tuning(KNOB) == v
    for knob, v in ((KNOB, -1), (KNOB, 2), (LAUNCHES, 0), (LAUNCHES, 1)):
        with pytest.raises(gsr.GsrError):
            r.set_tuning(knob, v)
    assert r.get_tuning(KNOB) == 0                # a refused value changes nothing
    with pytest.raises(gsr.GsrError):
        r.get_tuning(36)
    r.close()


def test_knob_is_per_context_and_survives_lane_changes(gsr):
    a, b = gsr.Renderer(), gsr.Renderer()
    a.set_tuning(KNOB, 0)
    for F in (4, 1, 8):
        a.set_frames_in_flight(F)
        assert a.get_tuning(KNOB) == 0 and b.get_tuning(KNOB) == 1
    a.close()
    b.close()


def test_path_argument_errors_come_before_device_work(gsr):
    from gaussianrenderer_amd import _native
    L = _native.lib()
    r = gsr.Renderer()
    r.set_frames_in_flight(4)
    cams = (gsr.Camera * 2)()
    outs = (ctypes.c_void_p * 2)(None, None)
    args = lambda nframes, cams, outs, flags: (r.ctx, None, 0, 0, cams, None, nframes, 64, 64, 1, 1, 64, 64, 3.0, outs,
                                               None, None, None, ctypes.c_int(flags))
    assert L.gsr_render_path_ex(*args(0, None, None, 4)) == _native.GSR_E_ARG       # unknown flag
    assert L.gsr_render_path_ex(*args(-1, cams, outs, 0)) == _native.GSR_E_ARG      # negative frame count
    assert L.gsr_render_path_ex(*args(2, None, outs, 0)) == _native.GSR_E_ARG       # no cameras
    assert L.gsr_render_path_ex(*args(2, cams, None, 0)) == _native.GSR_E_ARG       # no outputs
    assert L.gsr_render_path_ex(*args(2, cams, outs, 0)) == _native.GSR_E_ARG       # a null output
    assert L.gsr_render_path_ex(*args(0, None, None, 0)) == _native.GSR_OK          # no frames: nothing to do
    assert r.get_tuning(LAUNCHES) == 0
    r.close()
