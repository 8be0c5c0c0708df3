#!/usr/bin/env python3
"""Generate tests/golden/g_tp_train.npz by EXECUTING the reference's predictor training (authoring container only: needs the reference checkout;
never run on the GPU box, never from tests).  Reuses make_golden.py's loaders without changing that file.

The reference's own TP_net class (learning/mappo.py:572-589), its update_TP (:252-268), make_dataset_naive (:493-513) and the use_TP_net
statement of train_op (:405-441) run on CPU, with torch.optim.Adam(lr=1e-4) and nn.MSELoss as MAPPOPolicy.__init__ makes them (:92-95), from
the golden predictor weights (g_tp_obs.npz).  The rollout: 64 envs x 64 steps, three pursuers (I = 16), T = 10, F = 5, window_step 1,
16 minibatches, one epoch (cfg/algo/mappo.yaml).  Progress runs 760 .. 800 and restarts at 1: TP_done masks the five windows of steps 36-40.
Stored: the inputs (the frame sequence the windows are cut from, values on a 2^-6 grid, ground truth on a 2^-10 grid, so the file stays
small), every minibatch's indices and loss, the gradients of the first minibatch and a SHA-256 digest of every minibatch's gradients (the six
fp32 arrays in state_dict order), the weights and Adam moments after the update.  The initial weights are g_tp_obs.npz's.
"""
import hashlib
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as M  # noqa: E402

MAPPO = "omni_drones/learning/mappo.py"
E, STEPS, A, T, F, NMB, EPOCHS, MAX_LEN = 64, 64, 3, 10, 5, 16, 1, 800
KEYS = ["lstm.weight_ih_l0", "lstm.weight_hh_l0", "lstm.bias_ih_l0", "lstm.bias_hh_l0", "fc.weight", "fc.bias"]


class MiniTD:
    """The few TensorDict operations the block uses: construction with batch dims, key lookup, reshape(-1), integer-tensor indexing."""

    def __init__(self, d, batch_size):
        self.d, self.batch_size = dict(d), torch.Size(batch_size)

    def __getitem__(self, k):
        if isinstance(k, str):
            return self.d[k]
        return MiniTD({n: v[k] for n, v in self.d.items()}, k.shape)

    @property
    def shape(self):
        return self.batch_size

    @property
    def device(self):
        return next(iter(self.d.values())).device

    def reshape(self, *shape):
        assert shape == (-1,)
        n = self.batch_size.numel()
        return MiniTD({k: v.reshape(n, *v.shape[len(self.batch_size):]) for k, v in self.d.items()}, (n,))


def windows(frames):
    """TP_input [E, steps, T, I] from the frame sequence [E, steps + T, I]: step s sees frames s + 1 .. s + T (tests/test_tp_train.py does the same)."""
    return torch.stack([frames[:, s + 1:s + 1 + T] for s in range(frames.shape[1] - T)], dim=1).contiguous()


def grad_digest(grads):
    return hashlib.sha256(b"".join(np.ascontiguousarray(g.detach().numpy(), dtype=np.float32).tobytes() for g in grads)).hexdigest()


def rollout(g):
    """TP_input / TP_groundtruth / TP_done of a 64-step rollout as the env's ('next', 'agents', 'TP') entries stack them."""
    progress = torch.tensor([760 + s if 760 + s <= MAX_LEN else s - 40 for s in range(1, STEPS + 1)], dtype=torch.float32)
    I = 7 + 3 * A
    frames = torch.round(torch.randn(E, STEPS + T, I, generator=g) * 0.4 * 64) / 64
    frames[..., 0] = torch.cat([torch.arange(760 - T, 760, dtype=torch.float32), progress])[None, :]
    gt = torch.round((torch.rand(E, STEPS, 3, generator=g) * 2 - 1) * 0.9 * 1024) / 1024
    done = (progress <= MAX_LEN - F)[None, :, None].expand(E, STEPS, 1).clone()
    return frames, gt, done


def main():
    torch.set_num_threads(1)
    tp_cls = M._tp_class()
    w0 = dict(np.load(os.path.join(M.OUT, "g_tp_obs.npz")))
    net = tp_cls(input_dim=7 + 3 * A, output_dim=3 * F, future_predcition_step=F, window_step=1)
    with torch.no_grad():
        for k in KEYS:
            getattr(net, "lstm" if k.startswith("lstm") else "fc").__getattr__(k.split(".")[1]).copy_(torch.from_numpy(w0["w_" + k.replace(".", "_")]))
    init = {k: v.detach().clone() for k, v in net.state_dict().items()}
    g = torch.Generator().manual_seed(20261017)
    frames, tp_gt, tp_done = rollout(g)
    tp_input = windows(frames)

    fns = M.exec_functions(M.extract_source(MAPPO, ["update_TP"], "MAPPOPolicy"), {"torch": torch, "TensorDict": MiniTD, "Dict": dict, "Any": object})
    mdn = M.exec_functions(M.extract_source(MAPPO, ["make_dataset_naive"]), {"torch": torch, "TensorDict": MiniTD})["make_dataset_naive"]
    stmts = M._stmt_sources(MAPPO, "MAPPOPolicy", "train_op", lambda s: s.startswith("if self.use_TP_net:") and "make_dataset_naive" in s)
    assert len(stmts) == 1 and "make_dataset_naive" in stmts[0]
    self = types.SimpleNamespace(use_TP_net=1, TP_net=net, TP_optimizer=torch.optim.Adam(net.parameters(), lr=0.0001), TP_criterion=nn.MSELoss(),
                                 TP_epoch=EPOCHS, cfg=types.SimpleNamespace(num_minibatches=NMB))
    rec = {"idx": [], "loss": [], "digest": [], **{f"grad_{i}": [] for i in range(6)}}
    upd = fns["update_TP"]

    def update_TP(batch):
        info = upd(self, batch)
        rec["loss"].append(info["TP_loss"])
        params = dict(net.named_parameters())
        rec["digest"].append(grad_digest([params[k].grad for k in KEYS]))
        for i, k in enumerate(KEYS):
            rec[f"grad_{i}"].append(params[k].grad.detach().clone())
        return info
    self.update_TP = update_TP
    randperm = torch.randperm

    def recording_randperm(*a, **k):
        p = randperm(*a, **k)
        rec["idx"].append(p.clone())
        return p
    tensordict = {"next": {"agents": {"TP": {"TP_input": tp_input, "TP_groundtruth": tp_gt, "TP_done": tp_done}}}}
    ns = {"self": self, "tensordict": tensordict, "torch": torch, "TensorDict": MiniTD, "make_dataset_naive": mdn, "TP_info": []}
    torch.manual_seed(7)
    torch.randperm = recording_randperm
    try:
        exec(stmts[0], ns)
    finally:
        torch.randperm = randperm
    assert len(rec["loss"]) == NMB * EPOCHS and len(rec["idx"]) == EPOCHS
    out = {"frames": frames, "tp_groundtruth": tp_gt, "tp_done": tp_done, "n_sel": np.int64(ns["select_seq_len"]),
           "meta": np.array([E, STEPS, A, T, F, NMB, EPOCHS, 1], dtype=np.int64), "seed": np.int64(7),
           "perm": torch.stack(rec["idx"]).reshape(EPOCHS * NMB, -1), "loss": np.array(rec["loss"], dtype=np.float32),
           "grad_digest": np.array(rec["digest"])}
    for i, k in enumerate(KEYS):
        assert torch.equal(init[k], torch.from_numpy(w0["w_" + k.replace(".", "_")]))
        out["grad0_" + k] = rec[f"grad_{i}"][0]
        p = dict(net.named_parameters())[k]
        st = self.TP_optimizer.state[p]
        out["final_" + k], out["exp_avg_" + k], out["exp_avg_sq_" + k] = p.detach(), st["exp_avg"], st["exp_avg_sq"]
        out["step"] = st["step"]
    M.save("g_tp_train", **out)


if __name__ == "__main__":
    main()
