"""Validation inside the training loop (trainval_net --val-split): the model being trained runs a KITTI split through the
inference pipeline and kitti_eval, on ONE set of inference weights that lives as long as the training run.

The training model is an eval-mode _StereoRCNN: its inference forward keeps engine-side copies of the parameters (plan.Weights)
and per-size plans.  The first validation builds them; every later one calls Plan.refresh, which overwrites the prepared weights
from the live parameters on the device (srcnn_prep_weights, one host read) and keeps the buffers, the tuned conv plans and --
where no weight scale moved -- the recorded launch programs.  Nothing here draws a random number, and training's generators are
its own objects: a run with validation trains bit-identically to one without.
"""
import json
import os

import torch

from . import images, kitti_eval, test_net


class Validator(object):
    def __init__(self, model, kitti_path, split, label_dir, save_dir, precision='f16x3', device=None, log=print):
        self.model, self.label_dir, self.save_dir, self.precision, self.log = model, label_dir, save_dir, precision, log
        self.root = os.path.join(kitti_path, 'training')
        self.ids = images.read_split(split)
        self.device = device
        self.reports = []

    def refresh(self):
        """Brings the model's inference weights up to its parameters; returns Plan.refresh's report (None on first use: the first
        forward builds them)."""
        m = self.model
        if getattr(m, '_weights', None) is None or not m._plans:
            return None
        plan = next(reversed(list(m._plans.values())))
        return plan.refresh(m)              # the weights are shared: every other plan drops its programs at its next run if a scale moved

    def __call__(self, epoch):
        m = self.model
        rep = self.refresh()
        self.reports.append(rep)
        if rep is not None:
            self.log('validation: inference weights refreshed in place (%d layer scale(s) changed, programs %s)'
                     % (len(rep['scale_changed']), 'dropped' if rep['programs_dropped'] else 'kept'))
        prev = getattr(m, 'precision', 'f32')
        m.precision = self.precision
        result_dir = os.path.join(self.save_dir, 'val_epoch%d' % epoch)
        try:
            with torch.no_grad():
                test_net.run_split(m, self.root, self.ids, result_dir, self.device, solver='host', slots=1, prefetch=1)
        finally:
            m.precision = prev
        res = kitti_eval.evaluate_split(self.label_dir, result_dir, self.ids, self.device, log=lambda s: None)
        path = os.path.join(self.save_dir, 'ap_epoch%d.json' % epoch)
        with open(path, 'w') as fh:
            json.dump(res, fh, indent=1)
        self.log('[epoch %2d] validation on %d frames: %s -> %s' % (epoch, len(self.ids), car_moderate_line(res), path))
        return res


def car_moderate_line(res):
    """`Car Moderate AP_2d / AP_bev / AP_3d` (R40) at the first overlap set of the result."""
    car = res.get('Car') or {}
    if not car:
        return 'Car Moderate: no Car entries'
    key = next(iter(car))
    fmt = lambda v: 'n/a' if v is None else '%.2f' % v
    ap = lambda metric: fmt(car[key][metric]['moderate'].get('R40'))
    return 'Car Moderate AP@%s AP_2d %s / AP_bev %s / AP_3d %s' % (key, ap('bbox'), ap('bev'), ap('3d'))
