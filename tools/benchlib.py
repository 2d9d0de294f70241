"""What the measurement tools under tools/ share: the guarded runner, the device preamble, the alternating timer, the clocks.

The runner (`main`).  A tool's `main()` is one call of it.  The parent process touches no GPU: it runs the tool again as
`--child` under `timeout -k 10`, echoes the child's stdout (stderr passes through: only results go to the profile), and on a
non-zero exit leaves with that status and writes nothing -- on a shared machine nothing further may start after a fault, an abort
or a hang, and a profile is a file that a whole run stands behind.  Otherwise it writes the header line and the stdout to --out.

The timer (`alternating`, `window`).  The versions under comparison take turns inside every round, so that a drift of the clocks
or of the box falls on all of them alike; each window lies between two device events and ends in a wait for the second; the
first `warmup` rounds are thrown away.  The tool formats the lists it gets back (`stats`) in its own unit."""
import argparse
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(tool, child, out, reps, timeout, header, extra=()):
    """tool: the tool's __file__.  child(reps=..., <extra>=...): the measurement; what it prints is the profile.
    out, reps, timeout: the defaults of --out (a name under profiles/; None: no file unless asked), --reps, --timeout (seconds).
    header: the profile's first line, a %-format over the arguments' names (None: no such line).
    extra: [(flag, add_argument keywords)] of the tool's own arguments, forwarded to the child."""
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=out and os.path.join(ROOT, 'profiles', out))
    ap.add_argument('--reps', type=int, default=reps)
    ap.add_argument('--child', action='store_true')
    ap.add_argument('--timeout', type=int, default=timeout)
    flags = [('--reps', 'reps')] + [(flag, ap.add_argument(flag, **kw).dest) for flag, kw in extra]
    a = ap.parse_args()
    if a.child:
        return child(**{dest: getattr(a, dest) for _, dest in flags})
    forward = []
    for flag, dest in flags:
        value = getattr(a, dest)
        if isinstance(value, bool):             # a store_true switch
            forward += [flag] if value else []
        else:
            forward += [flag, str(value)]
    r = subprocess.run(['timeout', '-k', '10', str(a.timeout), sys.executable, os.path.abspath(tool), '--child'] + forward,
                       stdout=subprocess.PIPE, universal_newlines=True, cwd=ROOT)
    sys.stdout.write(r.stdout)
    if r.returncode != 0:
        sys.exit(r.returncode)                  # nothing further is started on the GPU, and no profile is written
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            if header:
                f.write(header % vars(a) + '\n')
            f.write(r.stdout)


def device():
    """Loads the library, refuses to go on without the GPU, returns cuda:0."""
    import torch
    from stereo_rcnn_amd import _lib
    _lib.lib()
    assert torch.cuda.is_available(), 'the measurement needs the GPU: no fallback'
    return torch.device('cuda:0')


def window(fn, inner=1, sync_before=False):
    """ms per call of `inner` back-to-back calls between two device events."""
    import torch
    if sync_before:
        torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / inner


def alternating(versions, reps, warmup, inner=1, before=None, sync_before=False, timer=window):
    """versions: [(name, fn)] or [(name, fn, a timer of its own)] -> {name: [reps times]}.  The versions take turns inside each
    round; before(name) runs untimed ahead of each window; the first `warmup` rounds are discarded."""
    times = {v[0]: [] for v in versions}
    for rep in range(warmup + reps):
        for name, fn, *own in versions:
            if before is not None:
                before(name)
            t = (own[0] if own else timer)(fn, inner, sync_before)
            if rep >= warmup:
                times[name].append(t)
    return times


def stats(times):
    return statistics.median(times), min(times), max(times)


def clocks():
    try:
        txt = subprocess.run(['rocm-smi', '--showclocks'], capture_output=True, text=True, timeout=20).stdout
        return ' | '.join(ln.strip() for ln in txt.splitlines() if 'sclk' in ln or 'mclk' in ln)[:400] or 'rocm-smi printed no clocks'
    except Exception as e:                                                        # the tool is optional
        return 'clocks not read (%s)' % type(e).__name__
