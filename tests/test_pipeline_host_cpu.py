"""CPU: the host rules of stereo_rcnn_amd/pipeline.py without a single library launch -- record -> objects (collect_3d on a
stub handle), the range-guard errors, the fp32 fallback (through detect_3d_batch on a fake model) and the numpy functions of
the scipy arrangement.  Expectations are written by record column from include/srcnn_hip.h (SRCNN_REC_COLS):
  0 score | 1-4 left box | 5-8 right box | 9-13 dim_orien (w,h,l,sin,cos) | 14-18 kpts | 19 roi index | 20 4-DoF status
  21-24 4-DoF x,y,z,theta | 25 dense-alignment status | 26 aligned disparity | 27-30 final x,y,z,theta | 31 alpha"""
import logging
import math
import os
import threading
import types

import numpy as np
import pytest
import torch

from oracle.dense_align import KITTI_DEMO_CALIB
from stereo_rcnn_amd import distributed, engine, pipeline
from stereo_rcnn_amd.model.utils import kitti_utils

N = 5                                   # rows of the record (rois per image)
UNSOLVED, INIT_ONLY, ALIGNED, UNSOLVED_2, BEYOND_COUNT = range(N)
IM_SHAPE = (375, 1242, 3)


class _Event(object):
    def synchronize(self):
        pass

    def query(self):
        return True


def _handle(rec, state, **fields):
    """What collect_3d reads of a launch_3d handle whose device work and host phases are over."""
    st = types.SimpleNamespace(worker=False, error=None, done=None, batch_head=None, phase=0, ctx=None, event=_Event(),
                               rec_host=torch.from_numpy(rec), state_host=torch.from_numpy(state))
    st.__dict__.update(fields)
    return st


def _fixture(k=4):
    """Five rows, the first k counted: unsolved, solved but not aligned, solved and aligned, unsolved, and a solved-looking row
    beyond the count.  Every value is a float32 number, so the way back (objects_to_record) is exact too."""
    rec = np.zeros((N + 1, pipeline.REC_COLS), np.float32)
    rec[0, 0] = k
    body = rec[1:]
    body[:, 0] = [0.95, 0.9, 0.75, 0.5, 0.25]
    body[:, 1:9] = np.arange(N * 8, dtype=np.float32).reshape(N, 8) * 0.5 + 10.0
    body[:, 9:12] = [[1.5, 1.25, 4.0], [1.625, 1.5, 3.75], [1.75, 1.375, 4.25], [1.5, 1.5, 4.0], [1.5, 1.5, 4.0]]
    body[:, 12], body[:, 13] = [0.6, -0.8, 0.28, 0.0, 1.0], [0.8, 0.6, -0.96, 1.0, 0.0]
    body[:, 14:19] = np.arange(N * 5, dtype=np.float32).reshape(N, 5) * 0.25 + 100.0
    body[:, 19] = [7, 3, 11, 0, 5]
    body[:, 20] = [0, 1, 1, 0, 1]
    body[:, 25] = [0, 0, 1, 0, 1]
    body[:, 26] = [0, 0, 17.5, 0, 3.0]
    state = np.zeros((2, N, 4), np.float64)
    state[0] = np.arange(N * 4).reshape(N, 4) * 0.25 + 1.0
    state[1] = np.arange(N * 4).reshape(N, 4) * -0.5 - 2.0
    return rec, state


def test_an_empty_record_gives_no_objects():
    rec, state = _fixture(k=0)
    assert pipeline.collect_3d(_handle(rec, state)) == []


def test_record_to_objects_exact():
    rec, state = _fixture()
    objs = pipeline.collect_3d(_handle(rec.copy(), state.copy()))
    assert [o['roi_index'] for o in objs] == [3, 11]                    # unsolved rows and rows beyond the count are skipped
    for o, i in zip(objs, (INIT_ONLY, ALIGNED)):
        row = rec[1 + i]
        assert o['score'] == float(row[0]) and isinstance(o['roi_index'], int) and o['roi_index'] == int(row[19])
        assert np.array_equal(o['box_left'], row[1:5]) and np.array_equal(o['box_right'], row[5:9])
        assert o['dim'].dtype == np.float64 and np.array_equal(o['dim'], row[9:12].astype(np.float64))
        assert o['alpha'] == math.atan2(float(row[12]), float(row[13]))
        assert np.array_equal(o['kpts'], row[14:19])
        assert np.array_equal(o['xyz_init'], state[0, i, 0:3]) and o['theta_init'] == float(state[0, i, 3])
    init, aligned = objs
    assert init['aligned'] is False and 'disparity' not in init
    assert np.array_equal(init['xyz'], state[0, INIT_ONLY, 0:3]) and init['theta'] == float(state[0, INIT_ONLY, 3])
    assert aligned['aligned'] is True and aligned['disparity'] == float(rec[1 + ALIGNED, 26])
    assert np.array_equal(aligned['xyz'], state[1, ALIGNED, 0:3]) and aligned['theta'] == float(state[1, ALIGNED, 3])


def test_a_not_aligned_object_has_its_own_xyz_array():
    """xyz and xyz_init are equal and distinct arrays: writing the final position must not move the 4-DoF one.  The one record
    test in this file that depends on _objects_from_record: before it, collect_3d gave a not-aligned object ONE array under
    both keys (the values were the same)."""
    rec, state = _fixture()
    init = pipeline.collect_3d(_handle(rec, state))[0]
    assert not init['aligned'] and init['xyz'] is not init['xyz_init'] and np.array_equal(init['xyz'], init['xyz_init'])


def test_objects_to_record_is_the_way_back():
    rec, state = _fixture()
    objs = pipeline.collect_3d(_handle(rec.copy(), state.copy()))
    back = distributed.objects_to_record(objs, N).numpy()
    assert back.shape == rec.shape and back[0, 0] == len(objs) == 2 and not back[3:].any()
    for r, i in zip(back[1:3], (INIT_ONLY, ALIGNED)):
        row = rec[1 + i]
        final = state[1 if row[25] > 0 else 0, i]
        for cols in (slice(0, 12), slice(14, 20), slice(25, 27)):
            assert np.array_equal(r[cols], row[cols]), cols
        assert r[20] == 1.0
        assert np.array_equal(r[21:25], state[0, i].astype(np.float32)) and np.array_equal(r[27:31], final.astype(np.float32))
        alpha = math.atan2(float(row[12]), float(row[13]))                # sin / cos / alpha come back through float64 libm calls
        assert np.array_equal(r[[12, 13, 31]], np.array([np.sin(alpha), np.cos(alpha), alpha], np.float32))


@pytest.mark.parametrize('own', [True, False])
def test_range_guard_flag_raises_with_the_layer_name(own):
    """Row 0, column 1 of the pair's own record -- or of the record of its batch's first image, which carries the flag of the
    forward the batch shares -- holds the tripped layer's tag + 1."""
    known = sorted(engine.TAG_NAMES)[0]
    unknown = max(engine.TAG_NAMES) + 1000
    for flag, text in ((known, engine.TAG_NAMES[known]), (unknown, 'layer tag %d' % (unknown - 1))):
        rec, state = _fixture()
        flagged = rec.copy()
        flagged[0, 1] = flag
        st = _handle(flagged, state) if own else _handle(rec, state, batch_head=_handle(flagged, state))
        with pytest.raises(engine.Split16RangeError) as e:
            pipeline.collect_3d(st)
        assert text in str(e.value) and ('shared forward' in str(e.value)) == (not own)


def test_lattice_overflow_of_a_solved_row_raises():
    rec, state = _fixture()
    rec[1 + ALIGNED, 25] = -1.0
    with pytest.raises(RuntimeError) as e:
        pipeline.collect_3d(_handle(rec, state))
    assert type(e.value) is RuntimeError and 'MAX_PIXELS' in str(e.value)      # dense_align.check_status
    rec, state = _fixture()
    rec[1 + UNSOLVED, 25] = -1.0                                               # an unsolved row is skipped before the check
    assert len(pipeline.collect_3d(_handle(rec, state))) == 2


def test_a_worker_error_is_raised_once_on_the_collecting_thread():
    rec, state = _fixture()
    done = threading.Event()
    done.set()
    st = _handle(rec, state, worker=True, done=done, error=ValueError('x'))
    with pytest.raises(ValueError, match='x'):
        pipeline.collect_3d(st)
    assert st.worker is False and st.error is None


# ------------------------------------------------------------------------------------------------ fp32 fallback
def _fake_batch(monkeypatch, collect):
    """detect_3d_batch on a fake model: launch_3d_batch returns a token, collect_3d_batch is `collect(precision)`."""
    model = types.SimpleNamespace(precision='f16x3', _weights=types.SimpleNamespace(guard_trips=0))
    seen = []

    def collect_3d_batch(handles):
        assert handles == 'handles'
        seen.append(model.precision)
        return collect(model.precision)

    monkeypatch.setattr(pipeline, 'launch_3d_batch', lambda *a, **k: 'handles')
    monkeypatch.setattr(pipeline, 'collect_3d_batch', collect_3d_batch)
    return model, seen, lambda: pipeline.detect_3d_batch(model, None, None, None, [None], [IM_SHAPE])


def _raise(err):
    raise err


def test_fallback_reruns_on_fp32_restores_the_precision_and_notes_the_trip(monkeypatch, caplog):
    model, seen, call = _fake_batch(monkeypatch, lambda p: 'marker' if p == 'f32' else _raise(engine.Split16RangeError('hot')))
    assert pipeline.RECALIBRATE_AFTER_TRIPS > 1                 # one trip stays below it: no plan is touched
    with caplog.at_level(logging.WARNING, logger='stereo_rcnn_amd'):
        assert call() == 'marker'
    assert seen == ['f16x3', 'f32'] and model.precision == 'f16x3' and model._weights.guard_trips == 1
    assert pipeline.guard_trips(model) == 1
    assert [r for r in caplog.records if r.name == 'stereo_rcnn_amd' and r.levelno == logging.WARNING
            and 'range guard tripped' in r.getMessage()]


def test_fallback_does_not_mask_or_count_a_failed_rerun(monkeypatch):
    model, seen, call = _fake_batch(monkeypatch,
                                    lambda p: _raise(RuntimeError('boom') if p == 'f32' else engine.Split16RangeError('hot')))
    with pytest.raises(RuntimeError, match='boom') as e:
        call()
    assert type(e.value) is RuntimeError
    assert seen == ['f16x3', 'f32'] and model.precision == 'f16x3' and model._weights.guard_trips == 0


def test_no_fallback_from_fp32(monkeypatch):
    model, seen, call = _fake_batch(monkeypatch, lambda p: _raise(engine.Split16RangeError('hot')))
    model.precision = 'f32'
    with pytest.raises(engine.Split16RangeError):
        call()
    assert seen == ['f32'] and model.precision == 'f32' and model._weights.guard_trips == 0


def test_a_second_trip_in_the_rerun_propagates(monkeypatch):
    model, seen, call = _fake_batch(monkeypatch, lambda p: _raise(engine.Split16RangeError('hot under ' + p)))
    with pytest.raises(engine.Split16RangeError, match='hot under f32'):
        call()
    assert seen == ['f16x3', 'f32'] and model.precision == 'f16x3' and model._weights.guard_trips == 0


# ------------------------------------------------------------------------------------------------ scipy arrangement
def _detections():
    """Three detections from the reference's solver cases: [0] as it is, [1] with a score below the threshold, [2] with
    regressed borders two pixels apart (narrower than half of any inferred pair)."""
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'reference_misc.npz'))
    c = g['solver_cases'][:3].astype(np.float32)            # alpha, dim 3, left box 4, right box 4, kpts 5
    score = np.array([[0.9], [0.02], [0.8]], np.float32)
    dim_orien = np.concatenate((c[:, 1:4], np.sin(c[:, 0:1]), np.cos(c[:, 0:1])), 1)
    kpts = c[:, 12:17].copy()
    kpts[2, 3:5] = [c[2, 4] + 10.0, c[2, 4] + 12.0]
    return (np.concatenate((c[:, 4:8], score), 1), np.concatenate((c[:, 8:12], score), 1), dim_orien, kpts)


def test_scipy_arrangement_4dof_tasks():
    dets = _detections()
    dl, dr, do, kpts = dets
    before = kpts.copy()
    inferred = kitti_utils.infer_boundary(IM_SHAPE, dl)
    narrow = [bool(before[i, 4] - before[i, 3] < 0.5 * (inferred[i, 1] - inferred[i, 0])) for i in range(3)]
    assert narrow == [False, False, True]                                        # the fixture is what its docstring says
    cand, alphas, tasks = pipeline._tasks_4dof(14, IM_SHAPE, KITTI_DEMO_CALIB, dets, 0.05)
    assert np.array_equal(kpts[:2], before[:2]) and np.array_equal(kpts[2, :3], before[2, :3])
    assert np.array_equal(kpts[2, 3:5], inferred[2]) and not np.array_equal(kpts[2, 3:5], before[2, 3:5])
    assert cand == [0, 2] and alphas == [math.atan2(do[i, 3], do[i, 4]) for i in cand]
    assert len(tasks) == 2
    for (kind, shape, p2, p3, args), i, a in zip(tasks, cand, alphas):
        assert kind == 14 and shape == IM_SHAPE and p2 is KITTI_DEMO_CALIB.p2 and p3 is KITTI_DEMO_CALIB.p3
        assert isinstance(args[0], float) and args[0] == a
        for got, want in zip(args[1:], (do[i, 0:3], dl[i, 0:4], dr[i, 0:4], kpts[i])):
            assert got.dtype == np.float32 and np.array_equal(got, want)


def test_scipy_arrangement_solved_objects_3dof_tasks_and_results():
    dets = _detections()
    dl, dr, do, kpts = dets
    cand, alphas, tasks = pipeline._tasks_4dof(14, IM_SHAPE, KITTI_DEMO_CALIB, dets, 0.05)
    res4 = [pipeline._solve_task(t) for t in tasks]
    assert all(status > 0 for status, _ in res4)
    assert pipeline._solved_objects(dets, cand, alphas, [(0, None), res4[1]])[0]['score'] == float(dl[2, 4])   # failed: dropped
    solved = pipeline._solved_objects(dets, cand, alphas, res4)
    assert len(solved) == 2
    for o, i, a, (_, state) in zip(solved, cand, alphas, res4):
        assert np.array_equal(o['box_left'], dl[i, 0:4]) and np.array_equal(o['box_right'], dr[i, 0:4])
        assert o['score'] == float(dl[i, 4]) and o['alpha'] == a and o['aligned'] is False and 'disparity' not in o
        assert o['dim'].dtype == np.float64 and np.array_equal(o['dim'], do[i, 0:3].astype(np.float64))
        assert np.array_equal(o['kpts'], kpts[i]) and o['kpts'] is not kpts[i]
        assert np.array_equal(o['xyz'], state[0:3]) and np.array_equal(o['xyz_init'], state[0:3]) and o['xyz'] is not o['xyz_init']
        assert o['theta'] == o['theta_init'] == float(state[3])
    boxes, kp, poses = pipeline._align_rows(solved)
    assert np.array_equal(boxes, dl[cand, 0:4]) and np.array_equal(kp, kpts[cand])
    assert np.array_equal(poses, [list(o['xyz']) + list(o['dim']) + [o['theta']] for o in solved])
    # disparity of the 4-DoF depth (focal length x baseline / z) as the float32 the alignment returns; only [1] "aligned"
    fb = KITTI_DEMO_CALIB.p2[0, 3] - KITTI_DEMO_CALIB.p3[0, 3]
    dis = np.array([fb / o['xyz'][2] for o in solved], np.float32)
    todo, tasks3 = pipeline._tasks_3dof(13, IM_SHAPE, KITTI_DEMO_CALIB, solved, np.array([0.0, 1.0], np.float32), dis)
    assert todo == [1] and len(tasks3) == 1
    kind, shape, p2, p3, (alpha, dim, box, d, kp1) = tasks3[0]
    o = solved[1]
    assert kind == 13 and shape == IM_SHAPE and p2 is KITTI_DEMO_CALIB.p2 and p3 is KITTI_DEMO_CALIB.p3
    assert isinstance(alpha, float) and alpha == float(np.float32(o['alpha']))                 # through float32, as poses_all
    assert dim is o['dim']
    assert box.dtype == np.float64 and np.array_equal(box, o['box_left'].astype(np.float64))
    assert kp1.dtype == np.float64 and np.array_equal(kp1, o['kpts'].astype(np.float64))
    assert type(d) is float and d == float(dis[1])
    res3 = [pipeline._solve_task(t) for t in tasks3]
    state, z = res3[0]
    init = o['xyz_init'].copy()
    pipeline._apply_3dof(solved, todo, res3, dis)
    assert solved[0]['aligned'] is False and 'disparity' not in solved[0]
    assert o['aligned'] is True and o['disparity'] == float(dis[1])
    assert o['xyz'].dtype == np.float64 and np.array_equal(o['xyz'], [state[0], state[1], z]) and o['xyz'][2] == z
    assert o['theta'] == float(state[2]) and np.array_equal(o['xyz_init'], init)
