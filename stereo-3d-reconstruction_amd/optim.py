"""`SGD`, `Adam` and `AdamW` on the library's optimizer step (`s3r_optim_step`, include/s3r.h): torch.optim.Optimizer subclasses whose
`step()` is three kernel launches per parameter group of up to 64 tensors, in a defined fp32 rounding order, with the step count, the
running powers and the learning rate ON THE DEVICE — the same bits on every run, nothing read on the host at enqueue time, and a step that
replays from a captured graph (forward, loss, backward and `step()` in one `torch.cuda.graph`).

Per group there is one device state buffer (eight dwords), one scratch buffer and one cached ctypes tensor array.  The moments are
allocated and zeroed once, at construction or by `init_state()`: `step()` under stream capture with uninitialised state raises before
anything is enqueued (a zero fill captured into the graph would wipe the moments at every replay).  Outside capture `step()` writes a
changed `group["lr"]` into the device state; `set_lr` writes it at any time, and between two replays it is the only way to change it.
beta, eps, weight_decay, clip_grad_norm and the flags are baked into a captured step.

There is no fallback: parameters the kernels do not serve are refused with a ValueError that names the reason.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib

__all__ = ["SGD", "Adam", "AdamW"]

_M = {_lib.OPT_SGD: ("momentum_buffer", None), _lib.OPT_ADAM: ("exp_avg", "exp_avg_sq")}


def _chunks(n):
    return (n + 511) // 512


class _Group:
    """the device side of one parameter group"""

    def __init__(self):
        self.state = None        # (8,) fp32: s3r_optim_state_init's dwords
        self.scratch = None
        self.key = None          # what the cached tensor array was built from
        self.array = None
        self.lr = None           # the learning rate last written to the device, as a Python float


class _S3ROptimizer(torch.optim.Optimizer):
    _kind = None

    def __init__(self, params, defaults):
        self._dev = []
        super().__init__(params, defaults)
        self.init_state()

    # ---------------------------------------------------------------- refusals
    @staticmethod
    def _check_param(p):
        if not isinstance(p, torch.Tensor):
            raise TypeError("optimizer parameters must be tensors")
        if p.dtype != torch.float32:
            raise ValueError(f"s3r optimizers take fp32 parameters only (got {p.dtype}): the kernels have no bf16 / fp16 form")
        if p.device.type != "cuda":
            raise ValueError("s3r optimizers take parameters on the GPU only (got a CPU parameter): there is no CPU fallback")
        if not p.is_contiguous():
            raise ValueError("s3r optimizers take contiguous parameters only (got a non-contiguous parameter)")
        if p.numel() == 0:
            raise ValueError("s3r optimizers take non-empty parameters only")

    def add_param_group(self, param_group):
        if not isinstance(param_group["params"], torch.Tensor):
            param_group["params"] = list(param_group["params"])
        ps = param_group["params"]
        for p in ([ps] if isinstance(ps, torch.Tensor) else ps):
            self._check_param(p)
        super().add_param_group(param_group)
        group = self.param_groups[-1]
        if len({p.device for p in group["params"]}) > 1:
            raise ValueError("the parameters of one group must live on one device")
        self._check_group(group)
        self._dev.append(_Group())

    def _check_group(self, group):
        raise NotImplementedError

    @staticmethod
    def _check_common(group):
        if group.get("maximize"):
            raise ValueError("maximize=True is not supported")
        lr, wd, clip = group["lr"], group["weight_decay"], group["clip_grad_norm"]
        if not (isinstance(lr, (int, float)) and 0.0 <= lr < float("inf")):
            raise ValueError(f"invalid learning rate: {lr!r} (a finite Python number >= 0; a tensor lr is not supported)")
        if not 0.0 <= wd < float("inf"):
            raise ValueError(f"invalid weight_decay: {wd!r}")
        if clip is not None and not 0.0 <= clip < float("inf"):
            raise ValueError(f"invalid clip_grad_norm: {clip!r} (None, or a finite max_norm >= 0)")

    # ---------------------------------------------------------------- state
    def _slots(self, group):
        m, v = _M[self._kind]
        if self._kind == _lib.OPT_SGD and group["momentum"] == 0:
            m = None
        return m, v

    def _initialised(self, gi, group, params):
        d = self._dev[gi]
        m, v = self._slots(group)
        return d.state is not None and all((m is None or m in self.state[p]) and (v is None or v in self.state[p]) for p in params)

    @torch.no_grad()
    def init_state(self):
        """Allocate and zero what is missing: the moments of every parameter, and per group the device state (step 0, powers 1, lr) and
        the scratch of the gradient norm.  Not under stream capture."""
        if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("init_state() under stream capture: the zero fills would be replayed with the graph")
        lib = _lib.load()
        for gi, group in enumerate(self.param_groups):
            d, params = self._dev[gi], group["params"]
            m, v = self._slots(group)
            for p in params:
                st = self.state[p]
                for slot in (m, v):
                    if slot is not None and slot not in st:
                        st[slot] = torch.zeros_like(p, memory_format=torch.contiguous_format)
            if d.state is None:
                dev = params[0].device
                with torch.cuda.device(dev):
                    d.state = torch.empty(_lib.OPTIM_STATE_DWORDS, dtype=torch.float32, device=dev)
                    d.scratch = torch.empty(sum(_chunks(p.numel()) for p in params) + len(params), dtype=torch.float32, device=dev)
                    d.lr = float(group["lr"])
                    _lib.check(lib.s3r_optim_state_init(d.state.data_ptr(), d.lr, torch.cuda.current_stream(dev).cuda_stream),
                               "optim_state_init")

    def set_lr(self, value, group=None):
        """Write the learning rate into the device state of `group` (an index; None: every group), ordered on the current stream like
        a step, and into `param_groups[...]["lr"]`."""
        value = float(value)
        lib = _lib.load()
        for gi in (range(len(self.param_groups)) if group is None else [group]):
            d, g = self._dev[gi], self.param_groups[gi]
            if d.state is None:
                raise RuntimeError("set_lr before init_state()")
            dev = d.state.device
            with torch.cuda.device(dev):
                _lib.check(lib.s3r_optim_set_lr(d.state.data_ptr(), value, torch.cuda.current_stream(dev).cuda_stream), "optim_set_lr")
            d.lr = g["lr"] = value

    def device_state(self, group=0):
        """the group's eight state dwords as an int32 device tensor (a view: step, beta1_pow, beta2_pow, lr, grad_norm, clip_coef,
        skipped, reserved); nothing is synchronised"""
        return self._dev[group].state.view(torch.int32)

    def grad_norm(self, group=0):
        """the gradient norm of the group's last step with clip_grad_norm or skip_nonfinite: a device tensor, not synchronised"""
        return self._dev[group].state[4]

    def skipped(self, group=0):
        """how many steps of the group were skipped on a non-finite norm: an int32 device tensor, not synchronised"""
        return self._dev[group].state.view(torch.int32)[6]

    def state_dict(self):
        sd = super().state_dict()
        sd["s3r_device_state"] = [None if d.state is None else d.state.view(torch.int32).clone() for d in self._dev]
        return sd

    @torch.no_grad()
    def load_state_dict(self, state_dict):
        sd = dict(state_dict)
        dev_state = sd.pop("s3r_device_state", None)
        super().load_state_dict(sd)
        for st in self.state.values():          # torch keeps a loaded tensor of the right dtype and device AS IT IS: the moments would be
            for k, t in st.items():             # the saving optimizer's own, stepped by both
                if isinstance(t, torch.Tensor):
                    st[k] = t.clone(memory_format=torch.contiguous_format)
        for d in self._dev:
            d.key = d.array = None
        self.init_state()
        if dev_state is not None:
            if len(dev_state) != len(self._dev):
                raise ValueError("loaded state dict has a different number of parameter groups")
            for d, s, g in zip(self._dev, dev_state, self.param_groups):
                if s is not None:
                    d.state.view(torch.int32).copy_(s.to(d.state.device))
                    d.lr = float(g["lr"])

    # ---------------------------------------------------------------- the step
    def _desc(self, group):
        raise NotImplementedError

    def _flags(self, group):
        f = 0
        if group["clip_grad_norm"] is not None:
            f |= _lib.OPT_CLIP
        if group["skip_nonfinite"]:
            f |= _lib.OPT_SKIP_NONFINITE
        return f

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        lib = _lib.load()
        capturing = torch.cuda.is_current_stream_capturing()
        todo = []
        for gi, group in enumerate(self.param_groups):          # every refusal first: a refused step enqueues nothing
            self._check_group(group)
            params = [p for p in group["params"] if p.grad is not None]
            if not params:
                continue
            for p in params:
                g = p.grad
                if g.is_sparse:
                    raise ValueError("sparse gradients are not supported")
                if g.dtype != torch.float32 or g.device != p.device or not g.is_contiguous() or g.shape != p.shape:
                    raise ValueError("a gradient must be a contiguous fp32 tensor of its parameter's shape, on its device")
            if not self._initialised(gi, group, params):
                if capturing:
                    raise RuntimeError("step() under stream capture before init_state(): the moments are not allocated, and a zero "
                                       "fill captured into the graph would wipe them at every replay")
                self.init_state()
            todo.append((gi, group, params))
        for gi, group, params in todo:
            d = self._dev[gi]
            m, v = self._slots(group)
            key = tuple((p.data_ptr(), p.grad.data_ptr(), p.numel()) for p in params)
            if d.key != key:
                arr = (_lib.OptimTensor * len(params))()
                for i, p in enumerate(params):
                    st = self.state[p]
                    arr[i] = _lib.OptimTensor(p.data_ptr(), p.grad.data_ptr(), st[m].data_ptr() if m else None,
                                              st[v].data_ptr() if v else None, p.numel())
                d.key, d.array = key, arr
            dev = d.state.device
            with torch.cuda.device(dev):
                stream = torch.cuda.current_stream(dev).cuda_stream
                if not capturing and float(group["lr"]) != d.lr:
                    d.lr = float(group["lr"])
                    _lib.check(lib.s3r_optim_set_lr(d.state.data_ptr(), d.lr, stream), "optim_set_lr")
                desc = self._desc(group)
                _lib.check(lib.s3r_optim_step(C.byref(desc), d.array, len(params), d.state.data_ptr(), d.scratch.data_ptr(),
                                              d.scratch.numel(), stream), "optim_step")
            # packed weight images are keyed on `_version`: a raw-pointer update that did not bump it would train on stale ones
            torch.autograd.graph.increment_version(params)
        return loss


class SGD(_S3ROptimizer):
    """torch.optim.SGD's rule (momentum, Nesterov, L2 weight decay; the first step sets the momentum buffer to the gradient) on
    `s3r_optim_step`.  Extra keywords: `clip_grad_norm` (None or max_norm: the group's gradients are scaled by min(max_norm / (norm +
    1e-6), 1), their norm summed in a fixed order) and `skip_nonfinite` (skip the whole step, counted in `skipped()`, when that norm is
    NaN or infinite)."""
    _kind = _lib.OPT_SGD

    def __init__(self, params, lr=1e-3, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False, *, maximize=False,
                 clip_grad_norm=None, skip_nonfinite=False):
        super().__init__(params, dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov,
                                      maximize=maximize, clip_grad_norm=clip_grad_norm, skip_nonfinite=skip_nonfinite))

    def _check_group(self, group):
        self._check_common(group)
        if group["dampening"] != 0:
            raise ValueError("dampening != 0 is not supported")
        if not 0.0 <= group["momentum"] < 1.0:
            raise ValueError(f"invalid momentum: {group['momentum']!r} (must be in [0, 1))")
        if group["nesterov"] and group["momentum"] == 0:
            raise ValueError("nesterov momentum needs momentum > 0")

    def _desc(self, group):
        flags = self._flags(group) | (_lib.OPT_NESTEROV if group["nesterov"] else 0)
        return _lib.OptimDesc(_lib.OPT_SGD, flags, group["momentum"], 0.0, 0.0, group["weight_decay"], group["clip_grad_norm"] or 0.0)


class Adam(_S3ROptimizer):
    """torch.optim.Adam's rule with L2 weight decay (added to the gradient) on `s3r_optim_step`: m and v updated, both divided by their
    bias corrections 1 - beta^t (the running powers live on the device), p -= lr * mhat / (sqrt(vhat) + eps).  Extra keywords as `SGD`."""
    _kind = _lib.OPT_ADAM
    _decoupled = False

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, amsgrad=False, *, maximize=False,
                 clip_grad_norm=None, skip_nonfinite=False):
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, maximize=maximize,
                                      clip_grad_norm=clip_grad_norm, skip_nonfinite=skip_nonfinite))

    def _check_group(self, group):
        self._check_common(group)
        if group["amsgrad"]:
            raise ValueError("amsgrad=True is not supported")
        b1, b2 = group["betas"]
        if not (0.0 <= b1 < 1.0 and 0.0 <= b2 < 1.0):
            raise ValueError(f"invalid betas: {group['betas']!r} (each must be in [0, 1))")
        if not 0.0 <= group["eps"] < float("inf"):
            raise ValueError(f"invalid eps: {group['eps']!r}")

    def _desc(self, group):
        flags = self._flags(group) | (_lib.OPT_DECOUPLED_DECAY if self._decoupled else 0)
        return _lib.OptimDesc(_lib.OPT_ADAM, flags, group["betas"][0], group["betas"][1], group["eps"], group["weight_decay"],
                              group["clip_grad_norm"] or 0.0)


class AdamW(Adam):
    """torch.optim.AdamW: `Adam` with DECOUPLED weight decay, p -= (lr * weight_decay) * p in front of the Adam update."""
    _decoupled = True

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, *, maximize=False,
                 clip_grad_norm=None, skip_nonfinite=False):
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, maximize=maximize,
                         clip_grad_norm=clip_grad_norm, skip_nonfinite=skip_nonfinite)
