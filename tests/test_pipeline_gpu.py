"""End-to-end flow (demo.py:137-326): HIP pipeline vs the CPU oracle pipeline on the same pair.
The 4-DoF scipy solve is chaotic in depth (see model/utils/box_estimator.py), so the comparison is per matched
object and statistical: same detections, same solver status, aligned disparities equal up to one fine depth
step, rectified 3-D boxes close for most objects."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def test_detect_3d_matches_oracle_pipeline(dev):
    from oracle import pipeline as opipe
    from oracle.dense_align import KITTI_DEMO_CALIB as calib
    from stereo_rcnn_amd import fixture, pipeline
    from stereo_rcnn_amd.model.stereo_rcnn.resnet import resnet
    torch.set_num_threads(min(torch.get_num_threads(), 16))
    sd = fixture.make_state_dict(3)
    m = resnet(('__background__', 'Car'), 101)
    m.create_architecture()
    m.load_state_dict(sd)
    m.cuda().eval()
    l, r, info = fixture.make_inputs(3, 200, 660, target_short=320)
    im_shape = (200, 660, 3)
    got = pipeline.detect_3d(m, l.to(dev), r.to(dev), info.to(dev), calib, im_shape, solver='scipy')
    ref = opipe.detect_3d(sd, l, r, info, calib, im_shape)
    assert len(ref) > 0 and abs(len(got) - len(ref)) <= max(2, len(ref) // 10)
    matched, same_init, ddis_same, ddis_other = 0, 0, [], []
    fb = calib.p2[0, 0] * (calib.p2[0, 3] - calib.p3[0, 3]) / calib.p2[0, 0]          # f * baseline
    for o in ref:
        best = min(got, key=lambda g: np.abs(g['box_left'] - o['box_left']).max())
        if np.abs(best['box_left'] - o['box_left']).max() > 0.05:
            continue
        matched += 1
        assert abs(best['score'] - o['score']) < 1e-4 and np.abs(best['dim'] - o['dim']).max() < 1e-3
        if not (best['aligned'] and o['aligned']):
            continue
        dd = abs(best['disparity'] - o['disparity'])
        # The dense alignment searches a depth grid centred on the 4-DoF solve (dense_align.py:186-215).  When scipy's
        # (chaotic, see box_estimator.py) end point is the same on both sides the grids coincide and the disparities
        # must agree; otherwise the grids are shifted against each other and only the coarse bracket is comparable.
        if np.abs(best['xyz_init'] - o['xyz_init']).max() < 1e-4:
            same_init += 1
            ddis_same.append(dd)
        else:
            ddis_other.append(dd * o['xyz_init'][2] ** 2 / fb)       # as a depth difference in metres
    assert matched >= 0.9 * len(ref)
    print('matched %d/%d, same 4-DoF end point %d: max |d disparity| %.3g px; shifted grids %d: median |dz| %.3g m'
          % (matched, len(ref), same_init, max(ddis_same, default=0.0), len(ddis_other),
             np.median(ddis_other) if ddis_other else 0.0))
    # (the images are noise, so the photometric cost has no structure: with shifted grids only the bracket is comparable;
    #  op-level parity on IDENTICAL inputs is asserted exactly in test_dense_align_gpu.py)
    if ddis_same:
        assert np.median(ddis_same) < 2e-3
    if ddis_other:
        assert np.median(ddis_other) < 1.0          # each side searches +-12.5 m around ITS solve: only typical agreement is checkable


def test_write_kitti_results(dev, tmp_path):
    from oracle.dense_align import KITTI_DEMO_CALIB as calib
    from stereo_rcnn_amd import pipeline
    from stereo_rcnn_amd.model.utils import kitti_utils
    c = kitti_utils.FrameCalibrationData()
    c.p2, c.p3 = calib.p2, calib.p3
    c.t_cam2_cam0 = np.array([0.06, 0, 0])
    objs = [{'box_left': np.array([1., 2, 3, 4]), 'xyz': np.array([1., 1.5, 20]), 'dim': np.array([1.6, 1.5, 4.0]),
             'theta': 0.2, 'score': 0.8}]
    pipeline.write_kitti_results(str(tmp_path), '000001', c, objs)
    assert (tmp_path / 'data' / '000001.txt').read_text().startswith('Car -1 -1 ')


def test_kitti_split_driver_writes_result_files(dev, tmp_path):
    """test_net.py's loop on a synthetic KITTI tree (image_2 / image_3 PNGs, calib files, split list): every frame of
    this rank's shard gets a result file whose lines parse as KITTI detections."""
    from PIL import Image
    from oracle.dense_align import KITTI_DEMO_CALIB as c            # calibration constants only
    from stereo_rcnn_amd import fixture, images, pipeline, test_net
    from stereo_rcnn_amd.distributed import shard_indices
    from stereo_rcnn_amd.model.stereo_rcnn.resnet import resnet
    root = tmp_path / 'training'
    for d in ('image_2', 'image_3', 'calib'):
        (root / d).mkdir(parents=True)
    ids = ['%06d' % i for i in range(3)]
    row = lambda name, mat: name + ': ' + ' '.join('%.12e' % v for v in np.ravel(mat))
    p0 = c.p2.copy(); p0[0, 3] = 0.0; p0[1, 3] = 0.0; p0[2, 3] = 0.0
    for k, frame in enumerate(ids):
        l, r = fixture.synthetic_pair(20 + k, 120, 400)
        Image.fromarray(l).save(str(root / 'image_2' / (frame + '.png')))
        Image.fromarray(r).save(str(root / 'image_3' / (frame + '.png')))
        (root / 'calib' / (frame + '.txt')).write_text('\n'.join([
            row('P0', p0), row('P1', p0), row('P2', c.p2), row('P3', c.p3), row('R0_rect', np.eye(3)),
            row('Tr_velo_to_cam', np.eye(3, 4)), row('Tr_imu_to_velo', np.eye(3, 4))]) + '\n')
    (tmp_path / 'val.txt').write_text('\n'.join(ids) + '\n')
    assert test_net.read_split(str(tmp_path / 'val.txt')) == ids
    m = resnet(('__background__', 'Car'), 101)
    m.create_architecture()
    m.load_state_dict(fixture.make_state_dict(3))
    m.cuda().eval()
    mine = [ids[i] for i in shard_indices(len(ids), 0, 2)]          # rank 0 of 2 -> frames 0 and 2
    frames, n_obj, _ = test_net.run_split(m, str(root), mine, str(tmp_path / 'result'), dev)
    assert frames == 2 and mine == ['000000', '000002']
    written = sorted(os.listdir(str(tmp_path / 'result' / 'data')))
    assert written == ['000000.txt', '000002.txt']
    lines = sum(((tmp_path / 'result' / 'data' / f).read_text().splitlines() for f in written), [])
    assert len(lines) == n_obj
    for ln in lines:
        parts = ln.split()
        assert parts[0] == 'Car' and len(parts) == 16 and all(np.isfinite(float(v)) for v in parts[1:])
    # a second run (three pairs in flight again) writes byte-identical files: the device 3-D stage is deterministic
    frames2, n_obj2, _ = test_net.run_split(m, str(root), ids, str(tmp_path / 'result2'), dev)
    assert frames2 == 3
    for f in written:
        assert (tmp_path / 'result2' / 'data' / f).read_text() == (tmp_path / 'result' / 'data' / f).read_text()
    # PNG decode on threads of this process (round 5's form) instead of the worker processes: the same pixels, the same files
    assert test_net.DECODE_PROCESSES and images._decode_workers
    test_net.DECODE_PROCESSES = False
    try:
        test_net.run_split(m, str(root), ids, str(tmp_path / 'result_threads'), dev)
    finally:
        test_net.DECODE_PROCESSES = True
    for f in sorted(os.listdir(str(tmp_path / 'result2' / 'data'))):
        assert (tmp_path / 'result_threads' / 'data' / f).read_text() == (tmp_path / 'result2' / 'data' / f).read_text()
    # the scipy comparison arrangement (host numpy + scipy in a process pool, staged) finds the same objects per frame
    with pipeline.SolverPool(2) as pool:
        frames3, n_obj3, _ = test_net.run_split(m, str(root), ids, str(tmp_path / 'result3'), dev, pool, solver='scipy')
    assert frames3 == 3
    same = total = 0
    for f in written:
        a = (tmp_path / 'result3' / 'data' / f).read_text().splitlines()
        b = (tmp_path / 'result' / 'data' / f).read_text().splitlines()
        boxes = lambda lines: {tuple(ln.split()[4:8]) for ln in lines}
        same += len(boxes(a) & boxes(b))
        total += max(len(a), len(b))
    assert total == 0 or same >= 0.6 * total      # objects at the z > 100 m / alignment-status edge differ (chaotic 4-DoF end point)


def test_demo_entry_point(dev, tmp_path, capsys):
    """python -m stereo_rcnn_amd.demo on PNG files + a calib file + a checkpoint in the reference's format."""
    from PIL import Image
    from oracle.dense_align import KITTI_DEMO_CALIB as c            # calibration constants only
    from stereo_rcnn_amd import demo, fixture
    l, r = fixture.synthetic_pair(31, 120, 400)
    Image.fromarray(l).save(str(tmp_path / 'left.png'))
    Image.fromarray(r).save(str(tmp_path / 'right.png'))
    row = lambda name, mat: name + ': ' + ' '.join('%.12e' % v for v in np.ravel(mat))
    p0 = c.p2.copy(); p0[:, 3] = 0.0
    (tmp_path / 'calib.txt').write_text('\n'.join([row('P0', p0), row('P1', p0), row('P2', c.p2), row('P3', c.p3),
                                                    row('R0_rect', np.eye(3)), row('Tr_velo_to_cam', np.eye(3, 4))]) + '\n')
    torch.save({'model': fixture.make_state_dict(3)}, str(tmp_path / 'ckpt.pth'))       # demo.py:81-82 loads checkpoint['model']
    demo.main(['--left', str(tmp_path / 'left.png'), '--right', str(tmp_path / 'right.png'), '--calib', str(tmp_path / 'calib.txt'),
               '--checkpoint', str(tmp_path / 'ckpt.pth')])
    out = capsys.readouterr().out
    assert 'objects (' in out
    for ln in out.splitlines():
        if ln.startswith('Car '):
            assert len(ln.split()) == 16


def test_streaming_pipeline_equals_serial(dev):
    """detect_3d_stream overlaps the GPU stages and the pooled scipy stages of consecutive pairs; per pair it must return
    exactly what detect_3d returns (same kernels on the same inputs, same deterministic solver calls)."""
    from oracle.dense_align import KITTI_DEMO_CALIB as calib       # calibration constants only
    from stereo_rcnn_amd import fixture, pipeline
    from stereo_rcnn_amd.model.stereo_rcnn.resnet import resnet
    m = resnet(('__background__', 'Car'), 101)
    m.create_architecture()
    m.load_state_dict(fixture.make_state_dict(3))
    m.cuda().eval()
    frames = []
    for seed in (3, 4, 5):
        l, r, info = fixture.make_inputs(seed, 200, 660, target_short=320)
        frames.append((l.to(dev), r.to(dev), info.to(dev), calib, (200, 660, 3), float(info[0, 2])))
    serial = [pipeline.detect_3d(m, *f[:5], solver='scipy') for f in frames]
    with pipeline.SolverPool(2) as pool:
        streamed = list(pipeline.detect_3d_stream(m, frames + frames, pool, solver='scipy'))
    assert len(streamed) == 6
    for want, got in zip(serial + serial, streamed):
        assert len(want) == len(got)
        for a, b in zip(want, got):
            assert np.array_equal(a['box_left'], b['box_left']) and a['aligned'] == b['aligned']
            assert np.array_equal(a['xyz'], b['xyz']) and a['theta'] == b['theta']


@pytest.mark.parametrize("solver", ['host', 'device'])
def test_three_in_flight_soak_is_bit_repeatable(dev, solver):
    """306 frames of the SAME full-size pair through the whole flow with three pairs in flight -- every
    3-D-stage kernel (class select / sort, pack, infer_boundary, solve4 / solve3 or the host solves, align_inputs, the dense
    alignment kernels) runs beside the MFMA kernels of the two other pairs' forwards, the co-residency under which the
    lane-quarter anomaly of DESIGN section 6 showed -- and every frame's objects must equal the lone run's bit for bit."""
    from oracle.dense_align import KITTI_DEMO_CALIB as calib
    from stereo_rcnn_amd import fixture, pipeline
    from stereo_rcnn_amd.model.stereo_rcnn.resnet import resnet
    m = resnet(('__background__', 'Car'), 101)
    m.create_architecture()
    m.load_state_dict(fixture.make_state_dict(3))
    m.cuda().eval()
    m.precision = 'f16x3'
    m.use_program = True
    l, r, info = [t.to(dev) for t in fixture.make_inputs(3, 375, 1242)]
    frame = (l, r, info, calib, (375, 1242, 3), float(info[0, 2]))
    # the streamed flow enters the serving regime (serving.enter: shipped throughput-tuned plans for this frame size); the lone
    # reference run must use the same conv plans -- another tile / split-K plan adds the K products in another order
    from stereo_rcnn_amd import serving
    serving.load_shipped_plans()
    lone = pipeline.detect_3d(m, *frame[:5], solver=solver)
    assert len(lone) >= 5 and any(o['aligned'] for o in lone)
    list(pipeline.detect_3d_stream(m, [frame] * 6, slots=3, solver=solver))          # first touch of every slot
    bad = []
    for k, objs in enumerate(pipeline.detect_3d_stream(m, [frame] * 306, slots=3, solver=solver)):
        same = len(objs) == len(lone)
        if same:
            for a, b in zip(lone, objs):
                for key, va in a.items():
                    vb = b[key]
                    if not (np.array_equal(va, vb) if isinstance(va, np.ndarray) else va == vb):
                        same = False
        if not same:
            bad.append(k)
    assert not bad, '%d of 306 frames differ from the lone run (first: %s)' % (len(bad), bad[:5])


def test_async_host_phases_give_the_same_objects(dev):
    """pipeline.ASYNC_HOST_PHASES (default; SRCNN_ASYNC_HOST=0 switches it off): a pair's host phases on a worker thread instead of on the loop
    thread -- the same calls on the same streams in the same order per pair: every frame's objects equal the default
    arrangement's bit for bit, also when a pair's slot is reused."""
    from oracle.dense_align import KITTI_DEMO_CALIB as calib
    from stereo_rcnn_amd import fixture, pipeline
    from stereo_rcnn_amd.model.stereo_rcnn.resnet import resnet
    m = resnet(('__background__', 'Car'), 101)
    m.create_architecture()
    m.load_state_dict(fixture.make_state_dict(3))
    m.cuda().eval()
    m.precision = 'f16x3'
    m.use_program = True
    frames = []
    for seed in (3, 4, 5):
        l, r, info = fixture.make_inputs(seed, 200, 660, target_short=320)
        frames.append((l.to(dev), r.to(dev), info.to(dev), calib, (200, 660, 3), float(info[0, 2])))
    saved = pipeline.ASYNC_HOST_PHASES
    try:
        pipeline.ASYNC_HOST_PHASES = False
        ref = list(pipeline.detect_3d_stream(m, frames * 4, slots=3, solver='host'))
        pipeline.ASYNC_HOST_PHASES = True
        got = list(pipeline.detect_3d_stream(m, frames * 4, slots=3, solver='host'))
    finally:
        pipeline.ASYNC_HOST_PHASES = saved
    assert len(ref) == len(got) == 12 and any(len(o) for o in ref)
    for a, b in zip(ref, got):
        assert len(a) == len(b)
        for x, y in zip(a, b):
            for key, va in x.items():
                vb = y[key]
                assert np.array_equal(va, vb) if isinstance(va, np.ndarray) else va == vb, key
