#!/usr/bin/env python3
"""Every output bit of the encoder's three users on a fixed list of cases, for a before / after comparison of a change that must not move any:
hns_policy_forward (policy.DevicePolicy), the critic's update (critic_train.value_loss_and_grad) and the actor's (actor_train.policy_loss_and_grad);
and of the four policy classes through all eight policy entries, with their packed images (policy_section).

    python tools/encoder_bits.py OUT.npz                 # on an MI355X: runs every case, writes every output array
    python tools/encoder_bits.py --cpu OUT.npz           # anywhere: the policy section alone on CPU tensors (the classes' restatements)
    python tools/encoder_bits.py --compare A.npz B.npz   # anywhere: the first array that differs (np.array_equal on the uint32 views); exit 1 if any

Run it once in a tree of the commit before the change (with that tree's own build of the library) and once in the tree after it, on the same
card.  The cases are the small shapes at which the tile code can go wrong (a partial tile, one row past a tile, no state_others, the widest
self embedding, the longest token loops) and reuse the case builders of tests/: nothing here needs more than a few seconds."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
TAGS = ("a3k5d35", "a3k8d20", "a1k5d20", "a6k16d24")
TRAIN_LIMITS = [(1, 5, 20, 40), (7, 5, 20, 9), (3, 1, 20, 33), (3, 16, 20, 33), (3, 5, 1, 33), (3, 5, 96, 33), (3, 5, 35, 1), (3, 5, 35, 11)]   # (A, K, D, batch): the tests' list
# (E, A, K) of the policy section: no state_others and one live row; 33 rows (the shared grid's second tile has one live row, the agent-major
# tile is partial); agent-major: two tiles per agent, the second with one live env; both maxima
POLICY_SHAPES = [(1, 1, 1), (11, 3, 5), (33, 3, 2), (5, 7, 16)]


def compare(a, b):
    za, zb = np.load(a), np.load(b)
    if sorted(za.files) != sorted(zb.files):
        print(f"the dumps hold different arrays: only in {a}: {sorted(set(za.files) - set(zb.files))}; only in {b}: {sorted(set(zb.files) - set(za.files))}")
        return 1
    bad = []
    for k in za.files:
        x, y = za[k], zb[k]
        if x.shape != y.shape or not np.array_equal(x.view(np.uint32), y.view(np.uint32)):
            bad.append(k)
    if bad:
        k = bad[0]
        n = int((za[k].view(np.uint32) != zb[k].view(np.uint32)).sum()) if za[k].shape == zb[k].shape else -1
        print(f"{len(bad)} of {len(za.files)} arrays differ; the first: {k} ({n} of {za[k].size} values)")
        return 1
    print(f"all {len(za.files)} arrays are bit-identical ({sum(za[k].size for k in za.files)} values)")
    return 0


def policy_section(put, torch, P, device="cuda"):
    """Every output array of the four policy classes through all their entries (hns_policy_forward / _act and their _rnn, _agents and
    _rnn_agents forms) and the packed images themselves.  policy.py and abi.py decide nothing about the bits, so HNS_LIBRARY=<another
    build> python tools/encoder_bits.py OUT.npz is the other arm in the same tree.  No NaN goes in: operand order may move a NaN's payload."""
    dev, D = torch.device(device), 35                            # (on "cpu" the classes run their restatements: a rehearsal of this loop)
    cuda = dev.type == "cuda"                                    # the packed images and the call counter exist on the device only
    put_out = lambda tag, o: [put(f"{tag}:{n}", getattr(o, n)) for n in o._fields if getattr(o, n) is not None]      # noqa: E731
    for E, A, K in POLICY_SHAPES:
        g = torch.Generator().manual_seed(9000 + 100 * E + 10 * A + K)
        r = lambda *s: torch.randn(*s, generator=g).to(dev)                                                         # noqa: E731
        xs, xo, xc, eps = r(E, A, D), (r(E, A, A - 1, 3) if A > 1 else None), r(E, A, K, 5), r(E, A, 4)
        h0 = (r(E, A, 128), r(E, A, 128))
        mixed = (torch.arange(E) % 2 == 0).to(dev)
        on = lambda d: {k: v.to(dev) for k, v in d.items()}                                                         # noqa: E731
        sa, sc = P.random_parameters(D, A, 3)
        pa, pc = P.random_parameters_per_agent(D, A, 4)
        ra, rc = {**sa, **P.random_rnn_parameters(5)}, {**sc, **P.random_rnn_parameters(6)}
        qa, qc = {**pa, **P.random_rnn_parameters_per_agent(A, 7)}, {**pc, **P.random_rnn_parameters(8)}
        seed = 2 ** 40 + 12345
        modes = {"eps": dict(eps=eps), "philox": {}, "det": dict(deterministic=True), "vo": dict(value_only=True)}
        for cls, (a, c) in {"DevicePolicy": (sa, sc), "PerAgentDevicePolicy": (pa, pc)}.items():
            pol, tag = getattr(P, cls)(on(a), on(c), seed=seed), f"pol:{cls}:e{E}a{A}k{K}"
            if cuda:
                pol.refresh()
                put(f"{tag}:packed", pol.packed.view(torch.float32))
            for mode, kw in modes.items():
                if cuda:
                    pol.counter.fill_(7)
                put_out(f"{tag}:{mode}", pol.forward(xs, xo, xc, **kw))
                if cuda:
                    put(f"{tag}:{mode}:counter", pol.counter)
            put(f"{tag}:act", pol.act(xs, xo, xc))
        for cls, (a, c) in {"RecurrentDevicePolicy": (ra, rc), "PerAgentRecurrentDevicePolicy": (qa, qc)}.items():
            pol, tag = getattr(P, cls)(on(a), on(c), seed=seed), f"pol:{cls}:e{E}a{A}k{K}"
            if cuda:
                pol.refresh()
                put(f"{tag}:packed", pol.packed.view(torch.float32))
                put(f"{tag}:rnn_packed", pol.rnn_packed.view(torch.float32))
            for st in ("absent", "given", "inplace"):
                for fl, is_init in (("noflags", None), ("mixed", mixed)):
                    t = f"{tag}:{st}:{fl}"
                    for mode, kw in modes.items():
                        ha, hc = (None, None) if st == "absent" else (h0[0].clone(), h0[1].clone())
                        if cuda:
                            pol.counter.fill_(7)
                        o = pol.forward(xs, xo, xc, actor_state=ha, critic_state=hc, is_init=is_init, out_states=(ha, hc) if st == "inplace" else None, **kw)
                        put_out(f"{t}:{mode}", o)
                        if cuda:
                            put(f"{t}:{mode}:counter", pol.counter)
                        if st == "inplace":                       # what value_only must leave alone included
                            put(f"{t}:{mode}:actor_buffer", ha)
                    h = None if st == "absent" else h0[0].clone()
                    action, new = pol.act_step(xs, xo, xc, state=h, is_init=is_init, out_state=h if st == "inplace" else None)
                    put(f"{t}:act_step:action", action)
                    put(f"{t}:act_step:state", new)


def flat(t):
    return np.ascontiguousarray(t.detach().cpu().numpy().astype(np.float32, copy=False)).reshape(-1)


def save(path, out):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    np.savez(path, **out)
    print(f"{len(out)} arrays, {sum(v.size for v in out.values())} values -> {path}")


def dump_cpu(path):
    import torch
    sys.path.insert(0, ROOT)
    import hns_amd  # noqa: F401
    from hns_amd import policy as P
    out = {}
    policy_section(lambda name, t: out.__setitem__(name, flat(t)), torch, P, device="cpu")
    save(path, out)


def dump(path):
    import torch
    for p in (ROOT, os.path.join(ROOT, "tests")):
        sys.path.insert(0, p)
    import hns_amd  # noqa: F401
    from hns_amd import policy as P
    from hns_amd import critic_train as CT
    from hns_amd import actor_train as AT
    import policy_reference as R
    import critic_update_reference as UC
    import actor_update_reference as UA
    import test_hip_critic_train as TC
    import test_hip_actor_train as TA

    out = {}

    def put(name, t):
        out[name] = flat(t)

    dev = lambda d: {k: torch.as_tensor(np.asarray(v)).cuda() for k, v in d.items()}

    # ---- the forward pass: sampled (stored eps), deterministic, and value_only both ways
    def forward_case(tag, actor, critic, obs, eps, seed=0, counter=None):
        pol = P.DevicePolicy(dev(actor), dev(critic), seed=seed)
        x = (torch.as_tensor(obs["state_self"]).cuda(), torch.as_tensor(obs["state_others"]).cuda() if "state_others" in obs else None,
             torch.as_tensor(obs["cylinders"]).cuda())
        e = torch.as_tensor(eps).cuda() if eps is not None else None
        for det in (False, True):
            for vo in (False, True):
                if counter is not None:
                    pol.counter.fill_(counter)
                o = pol.forward(*x, eps=e, deterministic=det, value_only=vo)
                for n in ("action", "log_prob", "value", "loc"):
                    if getattr(o, n) is not None:
                        put(f"fwd:{tag}:det{int(det)}:vo{int(vo)}:{n}", getattr(o, n))

    gp = np.load(os.path.join(GOLDEN, "g_policy.npz"))
    for tag in TAGS:
        forward_case("golden-" + tag, *R.golden_case(gp, tag)[:4])
    for shape in R.LIMIT_SHAPES:
        forward_case(R.limit_tag(shape), *R.limit_case(shape))
    for mode in R.EDGES:
        forward_case(mode, *R.edge_case(mode))
    actor, critic = R.random_net(35, 3, 61)
    obs, _ = R.random_obs(5, 3, 5, 35, 62)                     # 15 rows: a partial tile
    forward_case("philox", actor, critic, obs, None, seed=2 ** 40 + 12345, counter=7)
    policy_section(put, torch, P)

    # ---- the updates: every scalar, values / log_probs, every parameter's .grad
    def critic_case(tag, critic, obs, bv, ret, index, shape=None, **kw):
        c, o = TC._dev_call(critic, obs, bv, ret, index, shape, **kw)
        for n in ("value_loss", "explained_var", "grad_norm", "values"):
            put(f"critic:{tag}:{n}", getattr(o, n))
        for k, v in c.items():
            put(f"critic:{tag}:grad:{k}", v.grad)

    def actor_case(tag, actor, obs, action, lpo, adv, index, shape=None, **kw):
        c, o = TA._dev_call(actor, obs, action, lpo, adv, index, shape, **kw)
        for n in ("policy_loss", "entropy", "ess", "grad_norm", "log_probs"):
            put(f"actor:{tag}:{n}", getattr(o, n))
        for k, v in c.items():
            put(f"actor:{tag}:grad:{k}", v.grad)

    zc, za = np.load(os.path.join(GOLDEN, "g_critic_update.npz")), np.load(os.path.join(GOLDEN, "g_actor_update.npz"))
    for tag in TAGS:
        critic, obs, bv, ret, index, _, _ = UC.golden_case(zc, gp, tag)
        for loss in ("huber", "mse"):
            critic_case(f"golden-{tag}-{loss}", critic, obs, bv, ret, index, loss=loss)
        actor, obs, action, lpo, adv, index, ent_coef, _ = UA.golden_case(za, gp, tag)
        actor_case(f"golden-{tag}", actor, obs, action, lpo, adv, index, entropy_coef=ent_coef)
    for A, K, D, B in TRAIN_LIMITS:
        seed = 500 + A + K + D + B
        critic_case(f"limit-a{A}k{K}d{D}b{B}", *TC._case(48, A, K, D, seed, B=B, shift=-0.3 if B % 2 else 0.3))
        actor_case(f"limit-a{A}k{K}d{D}b{B}", *TA._case(48, A, K, D, seed, B=B))
    edges = {"flat_tokens": dict(embed_scale=1e-4, flat_bias=True), "saturated_softmax": dict(weight_scale=40.0), "large_obs": dict(obs_scale=300.0)}
    for i, (mode, kw) in enumerate(edges.items()):
        critic_case(mode, *TC._case(1024, 3, 8, 20, 21 + i, B=700, **kw))
        actor_case(mode, *TA._case(1024, 3, 8, 20, 21 + i, B=700, **kw))

    # an indexed minibatch (11 env-steps x 3 agents = 33 rows) of a strided [N, T, A, ..] rollout: the last dimension cut from twice its width
    N, T = 4, 6

    def strided(x):
        t = torch.as_tensor(np.concatenate([x, np.zeros_like(x)], axis=-1)).cuda()
        return t.reshape(N, T, *t.shape[1:])[..., :x.shape[-1]]

    lay = lambda x: torch.as_tensor(x).cuda().reshape(N, T, *x.shape[1:])
    critic, obs, bv, ret, index = TC._case(N * T, 3, 5, 35, 711, B=11)
    c, idx = dev(critic), torch.as_tensor(index).cuda()
    xs, xo, xc = (strided(obs[k]) for k in ("state_self", "state_others", "cylinders"))
    assert not xs.is_contiguous()
    o = CT.value_loss_and_grad(c, xs, xo, xc, lay(bv), lay(ret), idx)
    for n in ("value_loss", "explained_var", "grad_norm", "values"):
        put(f"critic:strided:{n}", getattr(o, n))
    for k, v in c.items():
        put(f"critic:strided:grad:{k}", v.grad)
    actor, obs, action, lpo, adv, index = TA._case(N * T, 3, 5, 35, 712, B=11)
    c, idx = dev(actor), torch.as_tensor(index).cuda()
    xs, xo, xc = (strided(obs[k]) for k in ("state_self", "state_others", "cylinders"))
    o = AT.policy_loss_and_grad(c, xs, xo, xc, lay(action), lay(lpo), lay(adv), idx)
    for n in ("policy_loss", "entropy", "ess", "grad_norm", "log_probs"):
        put(f"actor:strided:{n}", getattr(o, n))
    for k, v in c.items():
        put(f"actor:strided:grad:{k}", v.grad)

    torch.cuda.synchronize()
    save(path, out)


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    if len(sys.argv) == 3 and sys.argv[1] == "--cpu":
        sys.exit(dump_cpu(sys.argv[2]))
    if len(sys.argv) != 2 or sys.argv[1].startswith("-"):
        sys.exit(__doc__)
    dump(sys.argv[1])
