"""tools/benchlib.py without a GPU: the guarded runner against small stub tools, the alternating timer against a fake timer, and
that the nine measurement tools have handed both over to it."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, 'tools')
sys.path.insert(0, TOOLS)
import benchlib  # noqa: E402

NINE = ['loss_bench', 'targets_bench', 'conv_backward_bench', 'roi_align_backward_bench', 'optim_bench', 'loader_bench', 'overlay_bench',
        'train_step_bench', 'refresh_bench']

STUB = '''import os, sys, time
sys.path.insert(0, %r)
import benchlib


def child(reps, pairs, skip_step):
%s


benchlib.main(__file__, child, out=None, reps=9, timeout=20, header='# stub --reps %%(reps)d --pairs %%(pairs)d   (header)',
              extra=[('--pairs', dict(type=int, default=32)), ('--skip-step', dict(action='store_true'))])
'''


def run_stub(tmp_path, body, *args):
    tool = tmp_path / 'stub_bench.py'
    tool.write_text(STUB % (TOOLS, '\n'.join('    ' + ln for ln in body.splitlines())))
    out = tmp_path / 'made' / 'here' / 'profile.txt'                      # the runner creates the directory
    r = subprocess.run([sys.executable, str(tool), '--out', str(out)] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       universal_newlines=True, timeout=60)
    return r, out


def test_profile_is_header_plus_the_childs_stdout(tmp_path):
    r, out = run_stub(tmp_path, "print('first 1.5')\nprint('second %d' % reps)\nprint('not a result', file=sys.stderr)", '--reps', '7')
    assert r.returncode == 0, r.stderr
    assert r.stdout == 'first 1.5\nsecond 7\n'
    assert out.read_text() == '# stub --reps 7 --pairs 32   (header)\nfirst 1.5\nsecond 7\n'
    assert 'not a result' in r.stderr                                      # the child's stderr passes through, past the profile


def test_failing_child_stops_the_parent_and_leaves_no_profile(tmp_path):
    r, out = run_stub(tmp_path, "print('half a table')\nsys.exit(3)")
    assert r.returncode == 3
    assert r.stdout == 'half a table\n'
    assert not out.exists() and not out.parent.exists()


def test_child_past_its_time_limit_leaves_no_profile(tmp_path):
    r, out = run_stub(tmp_path, "print('started', flush=True)\ntime.sleep(30)", '--timeout', '1')
    assert r.returncode == 124                                             # timeout's status; the stub dies of its TERM, no KILL needed
    assert not out.exists()


def test_declared_arguments_reach_the_child_which_runs_at_the_root(tmp_path):
    body = "print(reps, pairs, skip_step, os.getcwd())"
    r, out = run_stub(tmp_path, body, '--pairs', '5', '--skip-step')
    assert r.returncode == 0, r.stderr
    assert r.stdout == '9 5 True %s\n' % ROOT
    assert out.read_text().startswith('# stub --reps 9 --pairs 5   (header)\n')
    r, _ = run_stub(tmp_path, body, '--reps', '4')
    assert r.stdout == '4 32 False %s\n' % ROOT


def test_alternating_order_warmup_before_and_own_timer():
    log = []
    fns = {'A': lambda: log.append('ran A'), 'B': lambda: log.append('ran B')}

    def fake(fn, inner, sync_before):
        log.append(('default', inner, sync_before))
        fn()
        log.append('end')
        return float(len(log))

    times = benchlib.alternating([('A', fns['A']), ('B', fns['B'])], reps=3, warmup=2, inner=4, sync_before=True,
                                 before=lambda name: log.append('before ' + name), timer=fake)
    one = lambda n: ['before ' + n, ('default', 4, True), 'ran ' + n, 'end']           # `before` outside the timed call, once per window
    assert log == (one('A') + one('B')) * 5                                               # A B A B ..., ten windows
    ends = [float(i + 1) for i, e in enumerate(log) if e == 'end']                        # what the fake timer returned, in order
    assert times == {'A': ends[4::2], 'B': ends[5::2]}                                    # the last three rounds only
    assert len(times['A']) == len(times['B']) == 3

    def own(fn, inner, sync_before):
        log.append('own')
        return -1.0
    del log[:]
    times = benchlib.alternating([('A', fns['A']), ('H', fns['B'], own)], reps=2, warmup=0, timer=fake)
    assert times['H'] == [-1.0, -1.0] and 'ran B' not in log and log.count('own') == 2    # timed by its own timer, not the default
    assert len(times['A']) == 2 and log.count(('default', 1, False)) == 2


def test_stats():
    assert benchlib.stats([3.0, 1.0, 2.0]) == (2.0, 1.0, 3.0)
    assert benchlib.stats([4.0, 1.0, 2.0, 3.0]) == (2.5, 1.0, 4.0)


def test_the_nine_tools_answer_help():
    procs = [subprocess.Popen([sys.executable, os.path.join(TOOLS, name + '.py'), '--help'], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                              universal_newlines=True) for name in NINE]
    for name, p in zip(NINE, procs):
        out, err = p.communicate(timeout=120)
        assert p.returncode == 0, (name, err)
        assert '--out' in out and '--reps' in out and '--timeout' in out, name


@pytest.mark.parametrize('name', NINE)
def test_runner_and_event_timing_live_in_benchlib_only(name):
    src = open(os.path.join(TOOLS, name + '.py')).read()
    for gone in ('--child', 'subprocess', "'timeout'", 'Event(', 'enable_timing', 'argparse'):
        assert gone not in src, (name, gone)
    assert 'benchlib.main(' in src
    lib = open(os.path.join(TOOLS, 'benchlib.py')).read()
    assert "'--child'" in lib and "subprocess.run(['timeout'" in lib and 'Event(enable_timing' in lib
