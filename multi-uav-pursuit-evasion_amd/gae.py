"""The rollout boundary: GAE, the advantage normalisation and ValueNorm1's targets (learning/utils/gae.py:27-75, learning/mappo.py:370-402).

`compute_gae` / `compute_gae_` have the reference's signatures and return values and work as drop-ins
(`omni_drones.learning.mappo.compute_gae = hns_amd.gae.compute_gae`): device tensors go to ONE launch of `hns_gae` instead of the reference's
Python loop over T (~8 elementwise launches per step), bit for bit the reference's fp32 statements; CPU tensors run a torch restatement of the
reference's statement order (CPU tests, gloo runs — not the hot path).

`rollout_targets` is mappo.py:370-402 in data-parallel form: denormalise + GAE + this rank's moment row (one `hns_gae` call: two launches), the path's
single collective (`sharding.allgather_moments`), `sharding.valuenorm1_update`, and the in-place normalisation of advantages and returns (one launch of
`hns_rollout_normalise`).  No host synchronisation anywhere: the success rate comes back as a 0-dim device tensor.  DESIGN.md §7.1."""
import ctypes as C

import torch

from . import abi, sharding


def _check(rc, what):
    if rc != abi.HNS_OK:
        raise RuntimeError(f"{what} failed ({rc}): {abi.load_library().hns_last_error().decode()}")


def _split(reward, done, value, next_value, time_major):
    """(N, T, K, Kd) of the reference's shapes: reward / value [N, T, *k] ([T, N, *k] time-major), done the same rank with trailing size 1 or k,
    next_value [N, *k]."""
    if reward.shape != value.shape:
        raise ValueError(f"reward {tuple(reward.shape)} and value {tuple(value.shape)} differ")
    if reward.dim() < 3:
        raise ValueError("reward / value need at least three dims: [N, T, k] (or [T, N, k])")
    T, N = (reward.shape[0], reward.shape[1]) if time_major else (reward.shape[1], reward.shape[0])
    K = reward[0, 0].numel()
    if done.dim() != reward.dim() or done.shape[:2] != reward.shape[:2]:
        raise ValueError(f"done {tuple(done.shape)} must have reward's rank and leading dims {tuple(reward.shape[:2])}")
    Kd = done[0, 0].numel()
    if Kd != 1 and done.shape[2:] != reward.shape[2:]:
        raise ValueError(f"done's trailing dims {tuple(done.shape[2:])} must be all 1 or reward's {tuple(reward.shape[2:])}")
    if next_value.numel() != N * K or next_value.shape[0] != N:
        raise ValueError(f"next_value {tuple(next_value.shape)} must be [N, *k] with N = {N}, prod(k) = {K}")
    return N, T, K, Kd


def _done_arg(done):
    if done.dtype == torch.bool or done.dtype == torch.uint8:
        return done.contiguous(), abi.HNS_GAE_DONE_U8
    if done.dtype == torch.float32:
        return done.contiguous(), abi.HNS_GAE_DONE_F32
    raise TypeError(f"hns_gae takes bool / uint8 / float32 dones, not {done.dtype}")


def _f32_dev(name, t, device):
    if t.dtype != torch.float32:
        raise TypeError(f"hns_gae takes float32 {name}, not {t.dtype}")
    if t.device != device:
        raise ValueError(f"{name} is on {t.device}, reward on {device}")
    return t.contiguous()


def _launch_gae(reward, done, value, next_value, gamma, lmbda, time_major, scale=None, shift=None, success=None, moments=False):
    """advantages, returns (reward's layout) and, with `moments`, this rank's [MOMENT_DIM] fp64 row — one call of hns_gae."""
    N, T, K, Kd = _split(reward, done, value, next_value, time_major)
    dev = reward.device
    reward, value, next_value = (_f32_dev(n, t, dev) for n, t in (("reward", reward), ("value", value), ("next_value", next_value)))
    done, dkind = _done_arg(done)
    if done.device != dev:
        raise ValueError(f"done is on {done.device}, reward on {dev}")
    if (scale is None) != (shift is None):
        raise ValueError("scale and shift go together")
    if scale is not None:
        scale, shift = _f32_dev("scale", scale, dev), _f32_dev("shift", shift, dev)
        if scale.numel() != 1 or shift.numel() != 1:
            raise ValueError("scale / shift are one value each (ValueNorm1 with input_shape (1,))")
    if success is not None:
        success = _f32_dev("success", success.float() if success.dtype == torch.bool else success, dev)
    adv, ret = torch.empty_like(reward), torch.empty_like(reward)
    row = ws = None
    if moments:
        row = torch.empty(sharding.MOMENT_DIM, dtype=torch.float64, device=dev)
        ws = torch.empty(abi.HNS_GAE_WORKSPACE_DOUBLES, dtype=torch.float64, device=dev)
    lib = abi.load_library()
    ptr = lambda t: t.data_ptr() if t is not None else None          # noqa: E731
    with torch.cuda.device(dev):
        st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        rc = lib.hns_gae(reward.data_ptr(), value.data_ptr(), done.data_ptr(), next_value.data_ptr(), N, T, K, Kd,
                         abi.HNS_GAE_TIME_MAJOR if time_major else abi.HNS_GAE_BATCH_MAJOR, dkind, float(gamma), float(lmbda),
                         ptr(scale), ptr(shift), ptr(success), success.numel() if success is not None else 0,
                         adv.data_ptr(), ret.data_ptr(), ptr(row), ptr(ws), st)
    _check(rc, "hns_gae")
    return adv, ret, row


def _torch_gae(reward, done, value, next_value, gamma, lmbda, time_major):
    """The reference's statements in its order (CPU path): index t along dim 1 (batch-major) or dim 0 (time-major)."""
    assert reward.shape == value.shape
    not_done = 1.0 - done.float()
    num_steps = not_done.shape[0] if time_major else not_done.shape[1]
    gae = 0
    advantages = torch.zeros_like(reward)
    for step in reversed(range(num_steps)):
        sl = (step,) if time_major else (slice(None), step)
        delta = reward[sl] + gamma * next_value * not_done[sl] - value[sl]
        advantages[sl] = gae = delta + (gamma * lmbda * not_done[sl] * gae)
        next_value = value[sl]
    returns = advantages + value
    return advantages, returns


def compute_gae(reward, done, value, next_value, gamma=0.99, lmbda=0.95):
    """reward / value [N, T, k], done [N, T, 1 or k], next_value [N, k] -> (advantages, returns) — learning/utils/gae.py:27-52."""
    if reward.is_cuda:
        adv, ret, _ = _launch_gae(reward, done, value, next_value, gamma, lmbda, time_major=False)
        return adv, ret
    return _torch_gae(reward, done, value, next_value, gamma, lmbda, time_major=False)


def compute_gae_(reward, done, value, next_value, gamma=0.99, lmbda=0.95):
    """reward / value [T, N, k], done [T, N, 1 or k], next_value [N, k] -> (advantages, returns) — learning/utils/gae.py:55-75."""
    if reward.is_cuda:
        adv, ret, _ = _launch_gae(reward, done, value, next_value, gamma, lmbda, time_major=True)
        return adv, ret
    return _torch_gae(reward, done, value, next_value, gamma, lmbda, time_major=True)


def rollout_normalise(advantages, returns, adv_mean=None, adv_den=None, ret_mean=None, ret_scale=None):
    """In place: advantages = (advantages - adv_mean) / adv_den, returns = (returns - ret_mean) / ret_scale, one launch of hns_rollout_normalise
    (device fp32 scalars; either pair may be None).  CPU tensors: the same two torch expressions."""
    pairs = [(advantages, adv_mean, adv_den), (returns, ret_mean, ret_scale)]
    if not advantages.is_cuda:
        for x, m, d in pairs:
            if m is not None:
                x.copy_((x - m) / d)
        return advantages, returns
    args = []
    for name, (x, m, d) in zip(("advantages", "returns"), pairs):
        if m is None:
            args += [None, 0, None, None]
            continue
        if x.dtype != torch.float32 or not x.is_contiguous():
            raise TypeError(f"hns_rollout_normalise works in place on contiguous float32 {name}")
        m, d = (_f32_dev(n, s.reshape(1), x.device) for n, s in (("mean", m), ("scale", d)))
        args += [x.data_ptr(), x.numel(), m.data_ptr(), d.data_ptr()]
    lib = abi.load_library()
    with torch.cuda.device(advantages.device):
        rc = lib.hns_rollout_normalise(*args, C.c_void_p(torch.cuda.current_stream(advantages.device).cuda_stream))
    _check(rc, "hns_rollout_normalise")
    return advantages, returns


def rollout_targets(reward, done, value, next_value, gamma, lmbda, value_normalizer=None, success=None, normalize_advantages=True, eps=1e-8,
                    time_major=False, return_moments=False):
    """MAPPOPolicy.train_op's targets (learning/mappo.py:370-402) for this rank's share of a data-parallel rollout.

    reward [N, T, *k, r] (summed over its last dim when r != 1, mappo.py:370-371), value [N, T, *k, 1] (critic output, normalised when a
    `value_normalizer` — the reference's ValueNorm1 — is given), done [N, T, ...] of the same rank (1 or k trailing), next_value [N, *k, 1];
    [T, N, ...] with `time_major`.  Returns (advantages, returns, success_rate): the normalised targets in reward's layout and the global success
    rate as a 0-dim device tensor (None without `success`).  `value_normalizer` is updated in place with the global batch moments of the returns.
    With `return_moments` a fourth value follows: (advantages_mean, advantages_std) of the advantages BEFORE the normalisation (mappo.py:391-392,
    train_info's entries; torch.std: unbiased) as 0-dim fp32 tensors, from the same gathered table."""
    if reward.shape[-1] != 1:
        reward = reward.sum(-1, keepdim=True)
    scale = shift = None
    if value_normalizer is not None:
        mean, var = value_normalizer.running_mean_var()
        scale, shift = torch.sqrt(var), mean
    if reward.is_cuda:
        adv, ret, row = _launch_gae(reward, done, value, next_value, gamma, lmbda, time_major, scale, shift, success, moments=True)
    else:
        if scale is not None:
            value, next_value = value * scale + shift, next_value * scale + shift
        adv, ret = _torch_gae(reward, done, value, next_value, gamma, lmbda, time_major)
        row = sharding.local_moments(adv, None if success is None else success.float(), ret)
    table = sharding.allgather_moments(row)
    if value_normalizer is not None:
        sharding.valuenorm1_update(value_normalizer, table)
    adv_mean = adv_den = ret_mean = ret_scale = moments = None
    if normalize_advantages or return_moments:
        mean, std = sharding.global_mean_std(table)
        moments = (mean.to(adv.dtype), std.to(adv.dtype))
    if normalize_advantages:
        adv_mean, adv_den = moments[0], moments[1] + eps
    if value_normalizer is not None:
        mean, var = value_normalizer.running_mean_var()
        ret_mean, ret_scale = mean, torch.sqrt(var)
    if adv_mean is not None or ret_mean is not None:
        rollout_normalise(adv, ret, adv_mean, adv_den, ret_mean, ret_scale)
    rate = None
    if success is not None:
        tot = table.sum(0)
        rate = tot[3] / tot[4]
    if return_moments:
        return adv, ret, rate, moments
    return adv, ret, rate
