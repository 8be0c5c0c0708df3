"""clip_grad_norm_'s scaling and torch.optim.Adam's single-tensor statements (amsgrad off, weight decay 0) restated in numpy fp32: what the
device optimiser step (csrc/hns_adam.hip behind hns_adam_clipped and hns_tp_adam; hns_amd.optim) is held to, bit for bit.  The restatement is
itself held to torch.optim.Adam(foreach=False) on the CPU by tests/test_tp_train.py and tests/test_critic_train.py.

Who bumps the counter: the caller.  `adam_np` takes the step count of THIS step (the counter after its bump), as the kernel forms it once for
all tensors of a step; `bump` is that one statement and `clip_adam_np` a whole step over lists of arrays."""
import numpy as np


def _fma32(a, b, c):
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def bump(step):
    """step + 1 in fp32, as the device counter holds it."""
    return np.float32(np.float32(step) + np.float32(1.0))


def clip_np(grads, total_norm, max_norm):
    """clip_grad_norm_'s scaling in fp32: coef = min((1 / (norm + 1e-6)) * max_norm, 1) (torch forms max_norm / x as reciprocal(x) * max_norm),
    every gradient times coef — always, also when coef is 1."""
    f32 = np.float32
    coef = f32(f32(f32(1.0) / f32(f32(total_norm) + f32(1e-6))) * f32(max_norm))
    coef = f32(min(coef, f32(1.0)))
    return [(g * coef).astype(f32) for g in grads], coef


def adam_np(p, g, m, v, step, lr, betas=(0.9, 0.999), eps=1e-8, sqrt=np.sqrt):
    """The statement order of torch's single-tensor Adam on its CPU kernels, in numpy fp32, with `step` already bumped: returns p, m, v.
    `sqrt`: IEEE (the kernel's); torch's CPU sqrt is not correctly rounded (about 0.6 % of values 1 ulp off), so a CPU self-check passes torch's in."""
    b1, b2 = betas
    f32 = np.float32
    m = _fma32(f32(1 - b1), (g - m).astype(f32), m)                      # lerp_(g, 1 - b1): fused on both the vector body and the tail
    v = _fma32((f32(1 - b2) * g).astype(f32), g, (v * f32(b2)).astype(f32))   # mul_(b2).addcmul_(g, g, value=1 - b2)
    bc1 = 1 - b1 ** float(step)
    bc2 = 1 - b2 ** float(step)
    den = (sqrt(v) / f32(bc2 ** 0.5)).astype(f32) + f32(eps)
    p = (p + (f32(-(lr / bc1)) * m).astype(f32) / den).astype(f32)
    return p, m, v


def clip_adam_np(params, grads, ms, vs, step, total_norm, max_norm, lr=5e-4, **kw):
    """One optimiser step over lists of arrays: (params, clipped grads, ms, vs, step + 1).  max_norm None or inf: no clip (total_norm unused)."""
    if max_norm is not None and np.isfinite(max_norm):
        grads, _ = clip_np(grads, total_norm, max_norm)
    step = bump(step)
    out = [adam_np(p, g, m, v, step, lr, **kw) for p, g, m, v in zip(params, grads, ms, vs)]
    return [o[0] for o in out], grads, [o[1] for o in out], [o[2] for o in out], step
