"""The trajectory predictor's training step: MAPPOPolicy.update_TP and its driver loop (learning/mappo.py:252-268, :405-441) on the device.

`loss_and_grad(tp, x, y, index)` is update_TP's first four statements (forward, nn.MSELoss, zero_grad, backward): device tensors go to ONE call
of `hns_tp_train_grad` (two launches: per-workgroup partial gradients on the matrix cores, then a fixed-order sum) that fills every parameter's
`.grad` in its PyTorch layout and returns the loss as a 0-dim device tensor — no autograd graph, no host synchronisation.  `index` reads a
minibatch of `make_dataset_naive` (mappo.py:493-513) in place.  A data-parallel caller can all_reduce the `.grad` tensors before the step.

`TPAdam` is torch.optim.Adam (amsgrad off, weight decay 0) with its step in ONE launch of `hns_tp_adam` over the six tensors and a
device-resident step counter; its state_dict is Adam's, both ways.  Every step bumps the parameters' version counters, so the env re-packs its
operand image before the next `hns_tp_observe` (env.HideAndSeek._tp_sync_weights).

`update_tp` is mappo.py:405-441 end to end.  CPU tensors run the reference's torch statements throughout (CPU tests, gloo runs — not the hot
path).  DESIGN.md §7.2."""
import ctypes as C

import torch
import torch.nn as nn

from . import abi

MAX_HISTORY, MAX_INPUT, MAX_FUTURE = 16, 80, 10


def _check(rc, what):
    if rc != abi.HNS_OK:
        raise RuntimeError(f"{what} failed ({rc}): {abi.load_library().hns_last_error().decode()}")


def parameters(tp):
    """TP_net's six parameters in hns_tp_params order (w_ih, w_hh, b_ih, b_hh, w_fc, b_fc)."""
    return [tp.lstm.weight_ih_l0, tp.lstm.weight_hh_l0, tp.lstm.bias_ih_l0, tp.lstm.bias_hh_l0, tp.fc.weight, tp.fc.bias]


def _as_blocks(x):
    """x as [E, S, T, I] (a [B, T, I] batch is [B, 1, T, I]) — a view, never a copy."""
    if x.dim() == 3:
        x = x.unsqueeze(1)
    if x.dim() != 4:
        raise ValueError(f"x must be [E, S, T, I] or [B, T, I], not {tuple(x.shape)}")
    return x


def _validate(params, x, y, index, check_index):
    """Every refusal of hns_tp_train_grad, raised here before anything is launched.  Returns (x4, y2, F)."""
    w_ih, w_hh, b_ih, b_hh, w_fc, b_fc = params
    H = abi.HNS_TP_HIDDEN
    for name, t in zip(abi.TP_WEIGHT_FIELDS, params):
        if t.dtype != torch.float32:
            raise TypeError(f"TP_net parameter {name} must be float32, not {t.dtype}")
        if not t.is_contiguous():
            raise ValueError(f"TP_net parameter {name} must be contiguous")
    if x.dtype != torch.float32 or y.dtype != torch.float32:
        raise TypeError(f"x and y must be float32, not {x.dtype} / {y.dtype}")
    x = _as_blocks(x)
    E, S, T, I = x.shape
    if tuple(w_hh.shape) != (4 * H, H) or tuple(b_ih.shape) != (4 * H,) or tuple(b_hh.shape) != (4 * H,) or w_ih.dim() != 2 or w_ih.shape[0] != 4 * H:
        raise ValueError("TP_net must be an LSTM with hidden size 64")
    if w_ih.shape[1] != I:
        raise ValueError(f"x frames have {I} values, the LSTM takes {w_ih.shape[1]}")
    if not 1 <= I <= MAX_INPUT:
        raise ValueError(f"frame width {I} outside [1, {MAX_INPUT}]")
    if not 1 <= T <= MAX_HISTORY:
        raise ValueError(f"history length {T} outside [1, {MAX_HISTORY}]")
    F3 = w_fc.shape[0]
    if w_fc.dim() != 2 or w_fc.shape[1] != H or F3 % 3 or tuple(b_fc.shape) != (F3,):
        raise ValueError(f"fc must be Linear(64 -> 3F), not {tuple(w_fc.shape)}")
    if not 1 <= F3 // 3 <= MAX_FUTURE:
        raise ValueError(f"future_step {F3 // 3} outside [1, {MAX_FUTURE}]")
    if E * S == 0:
        raise ValueError("x holds no sequence")
    if x.stride(3) != 1 or x.stride(2) != I:
        raise ValueError("each [T, I] block of x must be contiguous")
    if x.stride(1) < T * I or x.stride(0) < x.stride(1) * S:
        raise ValueError("x's leading strides overlap its [T, I] blocks")
    rows = E * S
    if y.numel() != rows * F3:
        raise ValueError(f"y must hold [E * S, 3F] = [{rows}, {F3}] values, not {tuple(y.shape)}")
    y = y.reshape(rows, F3)
    if index is not None:
        if index.dtype != torch.int64 or index.dim() != 1:
            raise TypeError("index must be a 1-d int64 tensor")
        if index.numel() < 1:
            raise ValueError("empty minibatch: the mean over zero sequences is NaN")
        if check_index and not (x.is_cuda and torch.cuda.is_current_stream_capturing()):
            lo, hi = int(index.min()), int(index.max())
            if lo < 0 or hi >= rows:
                raise IndexError(f"index values [{lo}, {hi}] outside the {rows} rows of x")
    devs = {t.device for t in (*params, x, y)} | ({index.device} if index is not None else set())
    if len(devs) != 1:
        raise ValueError(f"parameters, x, y and index must share one device, not {devs}")
    return x, y, F3 // 3


def _torch_loss_and_grad(tp, x, y, index):
    """update_TP's statements (mappo.py:256-266) on the gathered minibatch."""
    E, S, T, I = x.shape
    xb, yb = x.reshape(E * S, T, I), y
    if index is not None:
        xb, yb = xb[index], yb[index]
    out = tp(xb)
    loss = nn.MSELoss()(out, yb.reshape(xb.shape[0], -1))
    tp.zero_grad()
    loss.backward()
    return loss.detach()


def loss_and_grad(tp, x, y, index=None, check_index=True):
    """Loss of TP_net on a minibatch and every parameter's .grad (as zero_grad() + backward() leave them); returns the 0-dim loss.

    x: [E, S, T, I] fp32 with contiguous [T, I] blocks (`TP_input[:, :n_sel]` as it is) or [B, T, I]; y: [E * S, 3F] (or any shape of that many
    values, e.g. [E, S, F, 3]); index: int64 [B] rows of the flattened [E * S] (None: all E * S rows).  `check_index` range-checks the index
    (one host synchronisation; skipped inside a graph capture)."""
    params = parameters(tp)
    x, y, F = _validate(params, x, y, index, check_index)
    if not x.is_cuda:
        return _torch_loss_and_grad(tp, x, y, index)
    E, S, T, I = x.shape
    B = index.numel() if index is not None else E * S
    dev = x.device
    lib = abi.load_library()
    y = y.contiguous()
    for p in params:
        if p.grad is None:
            p.grad = torch.empty_like(p)
        elif p.grad.dtype != torch.float32 or not p.grad.is_contiguous() or p.grad.shape != p.shape:
            raise ValueError("existing .grad tensors must be contiguous float32 of the parameter's shape")
    nbytes = lib.hns_tp_train_workspace_bytes(B, I, F)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    loss = torch.empty((), dtype=torch.float32, device=dev)
    pw, gw = abi.HnsTpParams(), abi.HnsTpParams()
    for f, p in zip(abi.TP_WEIGHT_FIELDS, params):
        setattr(pw, f, p.data_ptr())
        setattr(gw, f, p.grad.data_ptr())
    with torch.cuda.device(dev):
        st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        rc = lib.hns_tp_train_grad(C.byref(pw), x.data_ptr(), E, S, x.stride(0), x.stride(1), T, I, y.data_ptr(),
                                   index.data_ptr() if index is not None else None, B, F, C.byref(gw), loss.data_ptr(), ws.data_ptr(), nbytes, st)
    _check(rc, "hns_tp_train_grad")
    return loss


class TPAdam(torch.optim.Optimizer):
    """torch.optim.Adam for TP_net's parameters: one launch of hns_tp_adam per step on the device (device-resident step counter, capturable),
    the reference's torch statements on the CPU.  state_dict() / load_state_dict() use Adam's format (per-parameter 'step' on the CPU,
    'exp_avg', 'exp_avg_sq'; Adam's param_group keys)."""

    def __init__(self, params, lr=1e-4, betas=(0.9, 0.999), eps=1e-8):
        params = list(params)
        defaults = dict(torch.optim.Adam([torch.zeros(1, requires_grad=True)], lr=lr, betas=betas, eps=eps).defaults)
        super().__init__(params, defaults)

    @staticmethod
    def _check_group(group):
        if group.get("weight_decay", 0) != 0 or group.get("amsgrad", False) or group.get("maximize", False):
            raise NotImplementedError("TPAdam implements Adam with weight_decay 0, amsgrad and maximize off")

    def _state(self, p, shared_step):
        st = self.state[p]
        if len(st) == 0:
            st["step"] = shared_step if shared_step is not None else torch.tensor(0.0, dtype=torch.float32)
            st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        return st

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for group in self.param_groups:
            self._check_group(group)
            ps = [p for p in group["params"] if p.grad is not None]
            dev = [p for p in ps if p.is_cuda]
            for p in ps:
                if not p.is_cuda:
                    self._cpu_step(p, self._state(p, None), group)
            if dev:
                self._device_step(dev, group)
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

    def _device_step(self, ps, group):
        by_dev = {}
        for p in ps:
            by_dev.setdefault(p.device, []).append(p)
        lib = abi.load_library()
        beta1, beta2 = group["betas"]
        for dev, plist in by_dev.items():
            shared = next((self.state[p]["step"] for p in plist if len(self.state[p]) and self.state[p]["step"].device == dev), None)
            if shared is None:
                shared = torch.zeros((), dtype=torch.float32, device=dev)
            for k in range(0, len(plist), 8):
                chunk = plist[k:k + 8]
                arr = (abi.HnsTpAdamTensor * len(chunk))()
                for j, p in enumerate(chunk):
                    st = self._state(p, shared)
                    if st["step"] is not shared:
                        raise RuntimeError("TPAdam: the parameters of a group on one device step together (one step counter)")
                    if p.dtype != torch.float32 or not p.is_contiguous() or not p.grad.is_contiguous() or p.grad.dtype != torch.float32:
                        raise ValueError("TPAdam on the device takes contiguous float32 parameters and gradients")
                    arr[j] = abi.HnsTpAdamTensor(p.data_ptr(), p.grad.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(), p.numel())
                if k > 0:
                    raise NotImplementedError("TPAdam: at most 8 parameters per group on one device")
                with torch.cuda.device(dev):
                    rc = lib.hns_tp_adam(arr, len(chunk), shared.data_ptr(), float(group["lr"]), float(beta1), float(beta2), float(group["eps"]),
                                         C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
                _check(rc, "hns_tp_adam")
            for p in plist:
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
                    raise ValueError("TPAdam: the parameters of a group on one device must share one step count")
                st["step"] = shared[p.device]


def select_windows(tp_input, tp_groundtruth, tp_done, future_step, window_step):
    """mappo.py:408-420: the windows of future ground truth the masks keep, as (x, y): x = TP_input[:, :n_sel] (a view), y [E * n_sel, 3F].
    One host synchronisation (masked_select's count), as in the reference."""
    windows = tp_groundtruth.unfold(dimension=1, size=future_step + 1, step=window_step).transpose(2, 3)[:, :, 1:]
    batch, _, fs, pos_dim = windows.shape
    mask = tp_done[:, :windows.shape[1]].squeeze(-1).unsqueeze(-1).unsqueeze(-1).expand_as(windows).bool()
    selected = torch.masked_select(windows, mask).view(batch, -1, fs, pos_dim)
    n_sel = selected.shape[1]
    return tp_input[:, :n_sel], selected.reshape(batch * n_sel, fs * pos_dim)


def minibatches(rows, num_minibatches, device, generator=None):
    """make_dataset_naive's permutation (mappo.py:506-513, seq_len 1): [num_minibatches, rows // num_minibatches] int64, same generator calls
    (`generator`: a torch.Generator on `device` instead of the global one)."""
    return torch.randperm((rows // num_minibatches) * num_minibatches, device=device, generator=generator).reshape(num_minibatches, -1)


def update_tp(tp, tp_input, tp_groundtruth, tp_done, future_step, window_step, num_minibatches, epochs, optimizer, generator=None):
    """MAPPOPolicy.train_op's predictor block (mappo.py:405-441) with update_TP (:252-268): tp_input [E, steps, T, I], tp_groundtruth
    [E, steps, 3], tp_done [E, steps, 1] (the rollout's ('next', 'agents', 'TP') entries).  Returns the mean minibatch loss as a 0-dim tensor.
    `generator`: the torch.Generator every epoch's permutation is drawn from (None: the global one)."""
    x, y = select_windows(tp_input, tp_groundtruth, tp_done, future_step, window_step)
    rows = x.shape[0] * x.shape[1]
    losses = []
    for _ in range(epochs):
        for idx in minibatches(rows, num_minibatches, x.device, generator):
            losses.append(loss_and_grad(tp, x, y, idx, check_index=False))
            optimizer.step()
    return torch.stack(losses).mean()
