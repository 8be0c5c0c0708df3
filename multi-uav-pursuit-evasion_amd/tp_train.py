"""The trajectory predictor's training step: MAPPOPolicy.update_TP and its driver loop (learning/mappo.py:252-268, :405-441) on the device.

`loss_and_grad(tp, x, y, index)` is update_TP's first four statements (forward, nn.MSELoss, zero_grad, backward): device tensors go to ONE call
of `hns_tp_train_grad` (two launches: per-workgroup partial gradients on the matrix cores, then a fixed-order sum) that fills every parameter's
`.grad` in its PyTorch layout and returns the loss as a 0-dim device tensor — no autograd graph, no host synchronisation.  `index` reads a
minibatch of `make_dataset_naive` (mappo.py:493-513) in place.  `update_tp(group=)` is the data-parallel caller: the ranks' gradients, weighted
by their minibatch sizes, are summed in one bucket before the step.

`TPAdam` (optim's, re-exported here) is torch.optim.Adam (amsgrad off, weight decay 0, lr 1e-4) with the device step every update shares.  Every
step bumps the parameters' version counters, so the env re-packs its operand image before the next `hns_tp_observe`
(env.HideAndSeek._tp_sync_weights).

`update_tp` is mappo.py:405-441 end to end.  CPU tensors run the reference's torch statements throughout (CPU tests, gloo runs — not the hot
path).  DESIGN.md §7.2."""
import ctypes as C

import torch
import torch.nn as nn

from . import abi
from .optim import TPAdam  # noqa: F401  (the predictor's optimiser, public here)

MAX_HISTORY, MAX_INPUT, MAX_FUTURE = 16, 80, 10


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
    abi.check(rc, "hns_tp_train_grad")
    return loss


def select_windows(tp_input, tp_groundtruth, tp_done, future_step, window_step):
    """mappo.py:408-420: the windows of future ground truth the masks keep, as (x, y): x = TP_input[:, :n_sel] (a view), y [E * n_sel, 3F].
    One host synchronisation (masked_select's count), as in the reference."""
    windows = tp_groundtruth.unfold(dimension=1, size=future_step + 1, step=window_step).transpose(2, 3)[:, :, 1:]
    batch, _, fs, pos_dim = windows.shape
    mask = tp_done[:, :windows.shape[1]].squeeze(-1).unsqueeze(-1).unsqueeze(-1).expand_as(windows).bool()
    selected = torch.masked_select(windows, mask)
    n_sel = selected.numel() // max(batch * fs * pos_dim, 1)     # (view(batch, -1, ..) cannot infer the count of an empty selection)
    selected = selected.view(batch, n_sel, fs, pos_dim)
    return tp_input[:, :n_sel], selected.reshape(batch * n_sel, fs * pos_dim)


def minibatches(rows, num_minibatches, device, generator=None):
    """make_dataset_naive's permutation (mappo.py:506-513, seq_len 1): [num_minibatches, rows // num_minibatches] int64, same generator calls
    (`generator`: a torch.Generator on `device` instead of the global one)."""
    return torch.randperm((rows // num_minibatches) * num_minibatches, device=device, generator=generator).reshape(num_minibatches, -1)


def update_tp(tp, tp_input, tp_groundtruth, tp_done, future_step, window_step, num_minibatches, epochs, optimizer, generator=None, group=None,
              bucket=None):
    """MAPPOPolicy.train_op's predictor block (mappo.py:405-441) with update_TP (:252-268): tp_input [E, steps, T, I], tp_groundtruth
    [E, steps, 3], tp_done [E, steps, 1] (the rollout's ('next', 'agents', 'TP') entries).  Returns the mean minibatch loss as a 0-dim tensor.
    `generator`: the torch.Generator every epoch's permutation is drawn from (None: the global one).

    `group` (a torch.distributed process group; None: the call above, untouched): every rank holds the windows its own TP_done selects, and
    the ranks step together on the union of their minibatches.  The selected-window counts are gathered ONCE; minibatch k of a rank has
    n_r = rows_r // num_minibatches windows, its gradient (a mean over n_r) is weighted by n_r / sum n before the SUM all-reduce of `bucket`
    (a policy_train.GradBucket over `parameters(tp)`; made here when None), and TP_loss is the same weighted mean (one all-reduce of the loss
    vector at the end).  A rank with n_r = 0 contributes zeros and still joins every collective; sum n = 0 skips the epochs on ALL ranks (the
    decision is the gathered counts', never a local one) and returns 0."""
    x, y = select_windows(tp_input, tp_groundtruth, tp_done, future_step, window_step)
    rows = x.shape[0] * x.shape[1]
    if group is not None:
        return _update_tp_group(tp, x, y, rows, num_minibatches, epochs, optimizer, generator, group, bucket)
    losses = []
    for _ in range(epochs):
        for idx in minibatches(rows, num_minibatches, x.device, generator):
            losses.append(loss_and_grad(tp, x, y, idx, check_index=False))
            optimizer.step()
    return torch.stack(losses).mean()


def _update_tp_group(tp, x, y, rows, num_minibatches, epochs, optimizer, generator, group, bucket):
    from . import policy_train as PT
    from . import sharding
    dev = x.device
    params = parameters(tp)
    if bucket is None:
        bucket = PT.GradBucket(params)
    elif len(bucket.params) != len(params) or any(a is not b for a, b in zip(bucket.params, params)):
        raise ValueError("bucket= must be the GradBucket of parameters(tp)")
    counts = sharding.all_gather_rows([rows // num_minibatches], group)[:, 0].tolist()       # the call's one gather: n_r of every rank
    n_mine, n_all = rows // num_minibatches, sum(counts)
    if n_all == 0:
        return torch.zeros((), dtype=torch.float32, device=dev)
    weight = n_mine / n_all
    losses = torch.zeros(epochs * num_minibatches, dtype=torch.float32, device=dev)
    k = 0
    for _ in range(epochs):
        batches = minibatches(rows, num_minibatches, dev, generator) if n_mine else [None] * num_minibatches
        for idx in batches:
            if idx is None:
                bucket.flat.zero_()
            else:
                loss = loss_and_grad(tp, x, y, idx, check_index=False)
                bucket.adopt()                                   # (the CPU backward replaces .grad; on the device the kernels wrote the views)
                bucket.flat.mul_(weight)
                losses[k] = loss * weight
            bucket.all_reduce(group)
            optimizer.step()
            k += 1
    return sharding.all_reduce_sum(losses, group).mean()
