"""The optimiser of every device update: torch.optim.Adam (amsgrad off, weight decay 0), optionally behind clip_grad_norm_, as ONE class.

`DeviceAdam.step` on device parameters is one call of `hns_adam_clipped` per device (csrc/hns_adam.hip: one launch per 64 tensors and one bump of
the device-resident step counter that all tensors of a group share; no host value, so a step can be captured); on CPU parameters it is the
reference's torch statements.  Its state_dict is Adam's, both ways.  Every step bumps the parameters' version counters, so the env and
`policy.DevicePolicy` re-pack their operand images before the next forward pass.

`tp_train.TPAdam` (the predictor's: lr 1e-4, no clip, no norm) and `policy_train.ClippedAdam` (the actor's and the critic's: lr 5e-4,
clip_grad_norm_ first) are this class with other constructor arguments.  DESIGN.md §7.2."""
import ctypes as C
import math

import torch
import torch.nn as nn

from . import abi


class DeviceAdam(torch.optim.Optimizer):
    """torch.optim.Adam with its step on the device.  `max_grad_norm` None: plain Adam — `step()` takes no norm and steps the parameters of
    each device on their own.  A number (inf included): clip_grad_norm_(params, max_grad_norm) first — `step(grad_norm=...)` takes the total
    gradient norm as a one-element fp32 tensor on the parameters' device (required there unless max_grad_norm is inf; on the CPU the step
    computes it), a group's parameters live on one device, and `last_grad_norm` is the unclipped norm of the last step (what clip_grad_norm_
    returns).  state_dict() / load_state_dict() use Adam's format (per-parameter 'step' on the CPU, 'exp_avg', 'exp_avg_sq'; Adam's
    param_group keys)."""

    def __init__(self, params, lr, betas=(0.9, 0.999), eps=1e-8, max_grad_norm=None):
        defaults = dict(torch.optim.Adam([torch.zeros(1, requires_grad=True)], lr=lr, betas=betas, eps=eps).defaults)
        super().__init__(list(params), defaults)
        self.max_grad_norm = max_grad_norm
        self.last_grad_norm = None

    def _check_group(self, group):
        if group.get("weight_decay", 0) != 0 or group.get("amsgrad", False) or group.get("maximize", False):
            raise NotImplementedError(f"{type(self).__name__} implements Adam with weight_decay 0, amsgrad and maximize off")

    def _state(self, p, shared_step):
        st = self.state[p]
        if len(st) == 0:
            st["step"] = shared_step if shared_step is not None else torch.tensor(0.0, dtype=torch.float32)
            st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        return st

    @torch.no_grad()
    def step(self, closure=None, grad_norm=None):
        name, clips = type(self).__name__, self.max_grad_norm is not None
        if grad_norm is not None and not clips:
            raise TypeError(f"{name}.step takes no grad_norm: it does not clip")
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for group in self.param_groups:
            self._check_group(group)
            ps = [p for p in group["params"] if p.grad is not None]
            cpu, by_dev = [p for p in ps if not p.is_cuda], {}
            for p in ps:
                if p.is_cuda:
                    by_dev.setdefault(p.device, []).append(p)
            if cpu and clips:
                self.last_grad_norm = nn.utils.clip_grad_norm_(cpu, self.max_grad_norm)
            for p in cpu:
                self._cpu_step(p, self._state(p, None), group)
            if clips and len(by_dev) > 1:
                raise ValueError(f"{name}: the parameters of a group live on one device, not {set(by_dev)}")
            for dev, plist in by_dev.items():
                self._device_step(dev, plist, group, grad_norm)
        return loss

    @staticmethod
    def _cpu_step(param, st, group):
        """torch.optim.adam._single_tensor_adam's statements (capturable off)."""
        beta1, beta2 = group["betas"]
        lr, eps = group["lr"], group["eps"]
        grad, exp_avg, exp_avg_sq, step_t = param.grad, st["exp_avg"], st["exp_avg_sq"], st["step"]
        step_t += 1
        exp_avg.lerp_(grad, 1 - beta1)
        exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
        step = step_t.item()
        bias_correction1 = 1 - beta1 ** step
        bias_correction2 = 1 - beta2 ** step
        step_size = lr / bias_correction1
        bias_correction2_sqrt = bias_correction2 ** 0.5
        denom = (exp_avg_sq.sqrt() / bias_correction2_sqrt).add_(eps)
        param.addcdiv_(exp_avg, denom, value=-step_size)

    def _device_step(self, dev, ps, group, grad_norm):
        name, clips = type(self).__name__, self.max_grad_norm is not None
        clip = clips and math.isfinite(self.max_grad_norm)
        if clip:
            if grad_norm is None:
                raise ValueError(f"{name}.step on the device needs grad_norm= (value_loss_and_grad's) unless max_grad_norm is inf")
            if not torch.is_tensor(grad_norm) or grad_norm.device != dev or grad_norm.dtype != torch.float32 or grad_norm.numel() != 1:
                raise ValueError("grad_norm must be a one-element float32 tensor on the parameters' device")
        shared = next((self.state[p]["step"] for p in ps if len(self.state[p]) and self.state[p]["step"].device == dev), None)
        if shared is None:
            shared = torch.zeros((), dtype=torch.float32, device=dev)
        arr = (abi.HnsAdamTensor * len(ps))()
        for j, p in enumerate(ps):
            st = self._state(p, shared)
            if st["step"] is not shared:
                raise RuntimeError(f"{name}: the parameters of a group on one device step together (one step counter)")
            if p.dtype != torch.float32 or not p.is_contiguous() or not p.grad.is_contiguous() or p.grad.dtype != torch.float32:
                raise ValueError(f"{name} on the device takes contiguous float32 parameters and gradients")
            # (an empty tensor has no address; the entry wants a non-NULL one and reads nothing through it: the counter's)
            arr[j] = abi.HnsAdamTensor(*(t.data_ptr() or shared.data_ptr() for t in (p, p.grad, st["exp_avg"], st["exp_avg_sq"])), p.numel())
        beta1, beta2 = group["betas"]
        with torch.cuda.device(dev):
            rc = abi.load_library().hns_adam_clipped(arr, len(ps), shared.data_ptr(), grad_norm.data_ptr() if clip else None,
                                                     self.max_grad_norm if clips else math.inf, float(group["lr"]), float(beta1), float(beta2),
                                                     float(group["eps"]), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
        abi.check(rc, "hns_adam_clipped")
        if clips:
            self.last_grad_norm = grad_norm
        for p in ps:
            torch.autograd.graph.increment_version(p)

    def state_dict(self):
        sd = super().state_dict()
        sd["state"] = {k: {n: (v.detach().to("cpu", copy=True) if n == "step" else v) for n, v in s.items()} for k, s in sd["state"].items()}
        return sd

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        for group in self.param_groups:
            shared = {}
            for p in group["params"]:
                st = self.state.get(p)
                if not st or "step" not in st:
                    continue
                step = torch.as_tensor(st["step"], dtype=torch.float32).detach()
                if not p.is_cuda:
                    st["step"] = step.to("cpu", copy=True)
                    continue
                if p.device not in shared:
                    shared[p.device] = step.to(p.device, copy=True)
                elif float(shared[p.device]) != float(step):
                    raise ValueError(f"{type(self).__name__}: the parameters of a group on one device must share one step count")
                st["step"] = shared[p.device]


class TPAdam(DeviceAdam):
    """The predictor's optimiser (mappo.py:94): torch.optim.Adam(lr 1e-4), no clip."""

    def __init__(self, params, lr=1e-4, betas=(0.9, 0.999), eps=1e-8):
        super().__init__(params, lr, betas, eps)


class ClippedAdam(DeviceAdam):
    """clip_grad_norm_(params, max_grad_norm) followed by torch.optim.Adam's step, as update_critic and update_actor run them.
    max_grad_norm None or inf: the clip is off; the step still records `last_grad_norm`."""

    def __init__(self, params, lr=5e-4, betas=(0.9, 0.999), eps=1e-8, max_grad_norm=10.0, weight_decay=0.0):
        if weight_decay != 0:
            raise NotImplementedError("ClippedAdam implements Adam with weight_decay 0")
        super().__init__(params, lr, betas, eps, math.inf if max_grad_norm is None else float(max_grad_norm))
        if not self.max_grad_norm >= 0:
            raise ValueError("max_grad_norm must be >= 0")
