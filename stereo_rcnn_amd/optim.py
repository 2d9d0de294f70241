"""The optimiser step of Stereo R-CNN's training on the HIP kernels of csrc/optim.hip: the global gradient norm with the
reference's clip coefficient (srcnn_grad_norm) and SGD with momentum (srcnn_sgd_step), both over the whole parameter list.

Reference: clip_gradient (lib/model/utils/net_utils.py:37-49) + torch.optim.SGD.step() (trainval_net.py:158-168, 224-227).  There
the norm is read back to the host, every gradient is rewritten by the coefficient and the update is four more passes; here
`SGD.step(clip_norm=10.)` is one pass over the gradients for the norm and one pass that reads p, g, m and writes p, m, the
coefficient multiplied in on the way and never leaving the device.  The gradients are not modified.  No host read.

`SGD` has torch.optim.SGD's constructor arguments, param_groups and state key ('momentum_buffer'), so state_dict() /
load_state_dict() are interchangeable with it (the reference's checkpoints carry that dict).  Only what the reference uses is
implemented: dampening 0, no Nesterov, no maximize -- anything else is refused.
"""
import ctypes

import torch

from . import _lib


def _check_tensor(t, what):
    if not t.is_cuda:
        raise NotImplementedError("%s on %s: the optimiser kernels run on the GPU only" % (what, t.device))
    if t.dtype != torch.float32:
        raise TypeError("%s must be float32, got %s" % (what, t.dtype))
    if t.is_sparse or not t.is_contiguous():
        raise ValueError("%s must be dense and contiguous" % what)


def _pointers(tensors):
    return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def _numels(tensors):
    return (ctypes.c_longlong * len(tensors))(*[t.numel() for t in tensors])


def _norm(entry, grads, words, *scalars):
    """One norm entry over `grads`: its `words` float32 results as a device tensor."""
    grads = list(grads)
    if not grads:
        raise ValueError("%s: no gradients" % entry)
    for g in grads:
        _check_tensor(g, "gradient")
    L = _lib.lib()
    dev = grads[0].device
    numel = _numels(grads)
    nbytes = L.srcnn_grad_norm_workspace_bytes(len(grads), numel)
    ws = _lib.workspace(nbytes, dev, key="optim")
    out = torch.empty(words, dtype=torch.float32, device=dev)
    _lib.check(getattr(L, entry)(_pointers(grads), numel, len(grads), *scalars, out.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream()),
               entry)
    return out


def grad_norm(grads, clip_norm):
    """(2,) float32 device tensor {L2 norm over every element of `grads`, clip_norm / max(norm, clip_norm)}: clip_gradient's two
    numbers (net_utils.py:39-46), summed in the defined order of include/srcnn_hip.h and left on the device."""
    return _norm("srcnn_grad_norm", grads, 2, float(clip_norm))


def grad_norm_guarded(grads, clip_norm, grad_scale=1.0):
    """(3,) float32 device tensor {L2 norm of grad_scale * g over `grads`, clip_norm / max(norm, clip_norm), 1 where the norm is
    finite else 0} (include/srcnn_hip.h).  clip_norm float('inf'): the coefficient is 1."""
    return _norm("srcnn_grad_norm_guarded", grads, 3, float(clip_norm), float(grad_scale))


def scale_grads(grads, coef):
    """g *= coef for every tensor of `grads`, coef a one-element float32 device tensor (one launch per 64 tensors)."""
    grads = list(grads)
    for g in grads:
        _check_tensor(g, "gradient")
    _check_tensor(coef, "coefficient")
    _lib.check(_lib.lib().srcnn_grad_scale(_pointers(grads), _numels(grads), len(grads), coef.data_ptr(), _lib.stream()), "srcnn_grad_scale")


class SGD(torch.optim.Optimizer):
    """torch.optim.SGD (dampening 0, no Nesterov) as one fused launch per 64 tensors, with clip_gradient folded in.

    step(clip_norm=None, clip_params=None): with clip_norm, the global norm of the gradients of `clip_params` (default: every
    parameter of the optimiser) is taken first and those parameters' gradients enter the update multiplied by
    clip_norm / max(norm, clip_norm); the other parameters (the reference's `uncert`) use their gradient as it is.  The
    (norm, coefficient) pair stays on the device as `self.last_norm`.

    step(..., guard=True, grad_scale=s) (keywords; include/srcnn_hip.h, "skipped when not finite"): every gradient enters as g * s (s = 1 / N after N
    backward passes have summed into .grad), and the whole update -- the unclipped parameters' too -- runs only where the norm of
    the scaled gradients is finite: on an Inf, a NaN or an overflowing norm no parameter and no momentum buffer changes (a buffer
    created by that very step becomes zeros, which makes the next step the first one) and `self.skipped_steps`, a one-element
    int32 device tensor created at the first such call, goes up by one.  step never reads it, or anything else, from the device.
    `self.last_norm` is then (norm, coefficient, ok).  The word `ok` comes from the norm over `clip_params`; where nothing is
    clipped (clip_norm None, or no clip parameter has a gradient) it comes from a norm over EVERY gradient taken with a clip_norm
    of +infinity, whose coefficient is 1 and is not used.  Either keyword alone selects this path: a grad_scale other than 1 is
    always guarded.  With guard=False and grad_scale=1 the calls are exactly those of the plain step.  The counter is no part of
    state_dict()."""

    def __init__(self, params, lr=1e-3, momentum=0, dampening=0, weight_decay=0, nesterov=False, *, maximize=False):
        if lr < 0.0:
            raise ValueError("Invalid learning rate: {}".format(lr))
        if momentum < 0.0:
            raise ValueError("Invalid momentum value: {}".format(momentum))
        if weight_decay < 0.0:
            raise ValueError("Invalid weight_decay value: {}".format(weight_decay))
        if dampening != 0 or nesterov or maximize:
            raise ValueError("stereo_rcnn_amd.optim.SGD implements what the reference trains with: dampening 0, no Nesterov momentum, "
                             "no maximize")
        # the keys of torch.optim.SGD's groups, so that a state dict moves between the two classes
        defaults = dict(lr=lr, momentum=momentum, dampening=0, weight_decay=weight_decay, nesterov=False, maximize=False, foreach=None,
                        differentiable=False, fused=None)
        super().__init__(params, defaults)
        self.last_norm = None
        self.skipped_steps = None

    @torch.no_grad()
    def step(self, clip_norm=None, clip_params=None, closure=None, *, guard=False, grad_scale=1.0):
        grad_scale = float(grad_scale)
        if not 0.0 < grad_scale < float('inf'):
            raise ValueError("grad_scale must be > 0 and finite, got %r" % grad_scale)
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        # buckets of one srcnn_sgd_step call each: (momentum, buffers still to be created)
        buckets = {}
        every = []
        for group in self.param_groups:
            if group.get('dampening', 0) != 0 or group.get('nesterov', False) or group.get('maximize', False):
                raise ValueError("parameter group with dampening / nesterov / maximize: not implemented")
            momentum, lr, wd = float(group['momentum']), float(group['lr']), float(group['weight_decay'])
            for p in group['params']:
                if p.grad is None:
                    continue
                _check_tensor(p, "parameter")
                _check_tensor(p.grad, "gradient")
                if p.grad.shape != p.shape:
                    raise ValueError("gradient of shape %s for a parameter of shape %s" % (tuple(p.grad.shape), tuple(p.shape)))
                m, first = None, False
                if momentum != 0:
                    state = self.state[p]
                    m = state.get('momentum_buffer')
                    if m is None:
                        m = state['momentum_buffer'] = torch.empty_like(p, memory_format=torch.contiguous_format)
                        first = True
                    else:
                        _check_tensor(m, "momentum buffer")
                buckets.setdefault((momentum, first), []).append((p, m, lr, wd))
                every.append(p)
        if not every:
            return loss
        guarded = bool(guard) or grad_scale != 1.0
        coef, clip_ids = None, set()
        if clip_norm is not None:
            clipped = every if clip_params is None else [p for p in clip_params if p.grad is not None]
            clip_ids = set(id(p) for p in clipped)
            if clipped:
                grads = [p.grad for p in clipped]
                self.last_norm = grad_norm_guarded(grads, clip_norm, grad_scale) if guarded else grad_norm(grads, clip_norm)
                coef = self.last_norm[1:2].data_ptr()
        # what the guarded entry takes beyond the plain one's arguments: (grad_scale,) before coef, (ok, skipped) after it
        before, after = (), ()
        if guarded:
            if coef is None:
                self.last_norm = grad_norm_guarded([p.grad for p in every], float('inf'), grad_scale)
            if self.skipped_steps is None:
                self.skipped_steps = torch.zeros(1, dtype=torch.int32, device=every[0].device)
            before, after = (grad_scale,), (self.last_norm[2:].data_ptr(), self.skipped_steps.data_ptr())
        entry = "srcnn_sgd_step_guarded" if guarded else "srcnn_sgd_step"
        for (momentum, first), entries in buckets.items():
            ps = [e[0] for e in entries]
            n = len(ps)
            flags = (ctypes.c_int * n)(*[int(coef is not None and id(p) in clip_ids) for p in ps])
            lists = (_pointers(ps), _pointers([p.grad for p in ps]), _pointers([e[1] for e in entries]) if momentum != 0 else None,
                     _numels(ps), (ctypes.c_float * n)(*[e[2] for e in entries]), (ctypes.c_float * n)(*[e[3] for e in entries]), flags, n,
                     momentum, int(first))
            _lib.check(getattr(_lib.lib(), entry)(*lists, *before, coef, *after, _lib.stream()), entry)
            if guarded:
                after = (after[0], None)                                # the step's first call counts a skipped step, no other one
        return loss
