"""GPU: bench.py honours the driver's contract (one JSON line with the agreed keys) in both launch forms."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = {'metric', 'value', 'unit', 'n_gpus', 'steps', 'warmup', 'ms_per_step', 'higher_is_better', 'scaling', 'vs_baseline',
        'dtype', 'data', 'config', 'roofline'}


def _check(line, steps, warmup):
    d = json.loads(line)
    assert KEYS <= set(d), KEYS - set(d)
    assert d['steps'] == steps and d['warmup'] == warmup and d['n_gpus'] == 1
    assert d['unit'] == 'stereo pairs/s' and d['higher_is_better'] is True and d['scaling'] == 'weak' and d['data'] == 'synthetic'
    assert d['value'] > 20 and abs(d['value'] - 1e3 / d['ms_per_step']) < 0.05 * d['value']
    assert 'workload' in d['config'] and 'model' not in d['config']
    r = d['roofline']
    assert r['bound'] == 'mfma' and r['unit'] == 'TFLOP/s' and abs(r['frac'] - r['achieved'] / r['peak']) < 1e-3
    # each roofline is quoted next to the step time of ITS OWN execution (8.1 ms of conv in a 7.1 ms step)
    assert r['conv_ms_per_step'] <= r['step_ms_of_this_execution'] * 1.02
    h = r['headline']
    assert abs(h['step_ms_of_this_execution'] - d['ms_per_step']) < 1e-3 and 0 < h['frac'] < 1
    assert abs(h['achieved'] - r['algorithmic_gflop_per_step'] / d['ms_per_step']) < 0.01 * h['achieved']
    # traffic is either measured on these very kernel sources or withheld
    assert r['traffic'] is None or 'on these sources' in r['traffic_note']
    return d


def test_bench_single_process_line(dev):
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--steps', '4', '--warmup', '1', '--full'], cwd=ROOT,
                         capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    d = _check(out.stdout.strip().splitlines()[-1], 4, 1)
    # roofline.traffic is measured in this very run (child runs under rocprofv3 --pmc) wherever rocprofv3 exists
    import shutil
    if shutil.which('rocprofv3'):
        r = d['roofline']
        assert r['traffic'] and 'MEASURED IN THIS RUN' in r['traffic_note'], r['traffic_note']
        assert 0.9 < r['traffic_over_algorithmic'] < 2.0, r['traffic_over_algorithmic']
        # roofline.non_conv: every non-conv kernel family of the step, alone on the chip, bytes and GB/s
        nc = r['non_conv']
        fams = {row['family']: row for row in nc['rows']}
        for f in ('max_pool', 'fpn top-down add', 'rpn scores', 'roi_align', 'proposal: NMS mask', 'proposal: NMS greedy scan',
                  'proposal: top-6000 selection', 'decode + class NMS', 'head tails', 'stem_pack'):
            assert f in fams and fams[f]['us'] > 0 and fams[f]['launches'] >= 1, f
        assert 2000 < fams['max_pool']['gb_per_s'] < 8000 and fams['max_pool']['algorithmic_mb'] > 100
        assert not any('at::native' in k for row in nc['rows'] for k in row['kernels'])      # steady-state steps only, no torch op
    # `sustained` (item 4a): the same loop after a warm soak, >= 300 steps
    su = d['sustained']
    assert su['steps'] >= 300 and 0.85 * d['value'] < su['value'] < 1.1 * d['value'], (su, d['value'])
    # `parity` (item 4b): measured in the run against the reference goldens / oracle
    pa = d['parity']
    dp = pa['demo_pair']
    assert dp['proposals_matched'] == '300/300' and dp['max_abs_err_bbox_pred'] < 1e-4 and dp['max_abs_err_dim_orien_pred'] < 1e-4
    assert dp['class_nms_keep_list_equal'] is True and dp['scores_equal'] is True and dp['decoded_boxes_max_abs_err_px'] < 2.5e-4
    assert pa['dense_align']['argmin_index_flips'] == 0 and pa['dense_align']['status_equal'] is True
    wc = pa['box3d_well_conditioned']
    assert wc['host_solver_identical_detections_bit_identical'] is True and wc['host_solver_linf_on_well_conditioned']['median'] <= 2.5e-5
    assert pa['box3d_demo_pair']['alignment_status_equal'] is True and pa['box3d_demo_pair']['linf_final_3d_box']['n'] >= 12



def test_bench_under_torch_distributed_run(dev):
    """the driver's N > 1 launch form, at world size 1 on this box: RCCL init, batched detection gathers, barriers"""
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY='0')
    out = subprocess.run([sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '1', '--master-addr',
                          '127.0.0.1', '--master-port', '29533', os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '5',
                          '--warmup', '1', '--full', '--no-cpu-baseline', '--no-pmc'], cwd=ROOT, capture_output=True, text=True, timeout=900, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    d = _check([ln for ln in out.stdout.strip().splitlines() if ln.startswith('{')][-1], 5, 1)
    assert 'all_gather' in d['config']['parallelism']


@pytest.mark.parametrize("cfg,batch", [(2, 8), (4, 4)])
def test_bench_other_baseline_configs_are_driver_runnable(dev, cfg, batch):
    """BASELINE.json configs[2] (batch 8, full 3-D pipeline) and configs[4] (ResNet-50, 2x resolution, batch 4) through the same
    bench.py contract: one JSON line, `config.workload` names the BASELINE entry, value = pairs/s = batch / step time,
    roofline (with the per-layer table) included."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--config', str(cfg), '--steps', '2', '--warmup', '1',
                          '--full', '--no-cpu-baseline'], cwd=ROOT, capture_output=True, text=True, timeout=1200)
    assert out.returncode == 0, out.stderr[-2000:]
    d = json.loads(out.stdout.strip().splitlines()[-1])
    assert KEYS <= set(d) and d['steps'] == 2 and d['n_gpus'] == 1 and d['unit'] == 'stereo pairs/s'
    assert d['config']['baseline_config_index'] == cfg and d['config']['pairs_per_step'] == batch
    assert ('BASELINE configs[%d]' % cfg) in d['config']['workload'] and 'model' not in d['config']
    assert d['value'] > 5 and abs(d['value'] - batch * 1e3 / d['ms_per_step']) < 0.05 * d['value']
    r = d['roofline']
    assert r['bound'] == 'mfma' and 0 < r['frac'] < 1 and r['conv_ms_per_step'] <= r['step_ms_of_this_execution'] * 1.02
    assert len(r['layers']) == 15 and all(g['us'] > 0 and g['own_bound_us'] > 0 for g in r['layers'])
    assert r['layers'] == sorted(r['layers'], key=lambda g: -g['lost_us'])


def test_bench_config3_val_list_replay_is_driver_runnable(dev):
    """BASELINE.json configs[3]: frames of the 3769-id val list replayed from PNG files through test_net.run_split (decode, H2D,
    fused preprocessing, forward, full 3-D flow with the host solver, KITTI result files) and gathered -- one JSON line of the
    same contract, with the host-side split per pair and the rate at which one rank's host budget saturates."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--config', '3', '--steps', '32', '--warmup', '8',
                          '--full', '--no-cpu-baseline'], cwd=ROOT, capture_output=True, text=True, timeout=1200)
    assert out.returncode == 0, out.stderr[-2000:]
    d = json.loads([ln for ln in out.stdout.strip().splitlines() if ln.startswith('{')][-1])
    c = d['config']
    assert KEYS <= set(d) and d['steps'] == 32 and d['n_gpus'] == 1 and d['unit'] == 'stereo pairs/s' and 'dry_run' not in d
    assert c['baseline_config_index'] == 3 and 'BASELINE configs[3]' in c['workload'] and 'model' not in c
    assert c['network_input'] == [600, 1987] and c['records_gathered'] == [32, 301, 32] and c['result_files_rank0'] >= 32
    assert d['value'] > 20 and abs(d['value'] - 1e3 / d['ms_per_step']) < 0.05 * d['value']
    assert c['objects_written_rank0'] > 0                       # the 3-D flow solved and aligned objects on the synthetic frames
    hm = c['host_ms_per_pair']
    assert hm['png_decode_and_calib_parse'] > 1.0 and hm['newton_cg_solves_wall'] > 0 and hm['main_thread_busy'] > 0
    assert c['host_saturation']['pairs_per_s_at_which_the_host_saturates'] > 10
    r = d['roofline']
    assert r['bound'] == 'mfma' and 0 < r['frac'] < 1 and 1200 < r['algorithmic_gflop_per_step'] < 1960


def test_bench_plain_run_times_the_steps_and_dumps_the_last_step(dev, tmp_path):
    """A plain run (no --full) carries the headline only -- `value` over exactly --steps timed steps, `ms_per_step` -- and
    --dump-outputs writes the last timed step's forward outputs, decoded detections and class-NMS keep list."""
    import numpy as np
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--steps', '3', '--warmup', '1', '--dump-outputs',
                          str(tmp_path)], cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    d = json.loads(out.stdout.strip().splitlines()[-1])
    assert KEYS <= set(d) and d['steps'] == 3 and d['warmup'] == 1 and d['n_gpus'] == 1
    assert d['value'] > 20 and abs(d['value'] - 1e3 / d['ms_per_step']) < 0.05 * d['value']
    assert d['roofline'] is None and 'cpu_baseline' not in d and 'parity' not in d and 'sustained' not in d
    names = {f[:-4] for f in os.listdir(str(tmp_path))}
    assert {'rois_left', 'cls_prob', 'bbox_pred', 'boxes_left_0', 'scores_0', 'keep_idx_0', 'num_kept_0'} <= names, names
    got = {n: np.load(str(tmp_path / (n + '.npy'))) for n in names}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= 64 << 20
    assert got['rois_left'].shape == (1, 300, 5) and np.isfinite(got['bbox_pred']).all()
    k = int(got['num_kept_0'][0])
    assert 0 < k <= 300 and (got['keep_idx_0'][:k] >= 0).all() and (got['keep_idx_0'][k:] == -1).all()
