"""bench.py's output contract on the GPU box: ONE JSON line with the driver's keys, the roofline object of the
dominant kernel and the cpu_baseline object (small sizes; the numbers themselves are not asserted)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_bench_prints_one_json_line_with_the_contract_keys():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "64", "--warmup", "8", "--envs", "4096",
                          "--cpu-steps", "3", "--tp-steps", "8", "--stream-groups", "2", "--group-steps", "16", "--abi-steps", "16",
                          "--config-steps", "16", "--envgen-episodes", "4", "--envgen-episode-length", "8"],
                         capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, out.stdout
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
              "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 64 and d["warmup"] == 8 and d["higher_is_better"] is True
    assert d["unit"] == "agent-steps/s" and d["scaling"] == "weak" and d["vs_baseline"] is None and d["data"] == "synthetic"
    assert d["dtype"] == "f32" and "workload" in d["config"] and "model" not in d["config"]
    assert abs(d["value"] - 4096 * 3 * 64 / (d["ms_per_step"] * 1e-3 * 64)) / d["value"] < 1e-3
    r = d["roofline"]
    assert r["bound"] == "hbm" and r["unit"] == "GB/s" and r["peak"] == 8000.0 and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-3
    # two durations under their own names: `frac` = `frac_kernel` prices the kernel's average launch duration (events around blocks of
    # consecutive launches after the region), `frac_step_rate` the timed region per step, which can never claim more than the wall clock of the same
    # region allows; isolated event-bracketed dispatches are a third, separately named field
    assert r["frac"] == r["frac_kernel"] and r["kernel_us"] > 0 and "blocks of consecutive plain launches" in r["kernel_us_source"]
    assert r["kernel_samples"] == 512 and len(r["kernel_us_blocks"]) == 8 and abs(sum(r["kernel_us_blocks"]) / 8 - r["kernel_us"]) < 0.02
    assert "hipEvent pair" in r["step_us_source"] and r["region_ms"] <= r["region_wall_ms"] * 1.001
    assert abs(r["step_us"] - max(r["region_ms"], r["region_wall_ms"]) * 1e3 / d["steps"]) < 0.02
    assert abs(r["frac_step_rate"] - r["bytes_per_launch"] / (r["step_us"] * 1e-6) / 1e9 / 8000.0) < 2e-4
    wall_rate = r["bytes_per_launch"] / (d["ms_per_step"] * 1e-3) / 1e9
    assert wall_rate / 1.03 <= r["frac_step_rate"] * 8000.0 <= wall_rate * 1.001                   # bounded by the wall clock of the same region, both ways
    assert r["isolated_dispatch_samples"] == 16 and r["kernel_us_isolated_dispatch_events"] > 0 and "dispatch_event_samples_in_region" not in r
    assert r["device_copy_GBs"] > 0 and "hns_copy_f4" in r["device_copy_kernel"]
    c = d["cpu_baseline"]
    assert c["kind"] == "port" and c["cores"] >= 1 and c["value"] > 0 and c["unit"] == "agent-steps/s" and "sample" in c
    assert c["cfg2"]["value"] >= c["cfg2"]["one_core_value"] > 0 and "4 096 envs" in c["cfg2"]["sample"]
    assert d["tp_mode"]["value"] > 0 and d["stream_shards"]["groups"] == 2
    tr = d["tp_mode"]["roofline"]                                                          # the predictor against the matrix-core peak
    assert tr["bound"] == "mfma" and tr["unit"] == "TFLOP/s" and tr["peak"] == 2500.0 and 0 < tr["frac"] < 1 and d["tp_mode"]["observe_us"] > 0
    rd = d["tp_mode"]["reference_default_batch"]                                           # ... and at the reference's own default batch (one-tile workgroups)
    assert "2 048 envs" in rd["workload"] and rd["value"] > 0 and 0 < rd["observe_us"] < d["tp_mode"]["observe_us"]
    assert "env.step" in d["config"]["workload"] and d["abi_rate"]["value"] > 0        # headline through the Python class, bare ABI beside it
    # PMC traffic: measured in the run itself (two rocprofv3 passes of a short inner run, the default) or, failing that, the labelled look-up
    assert r["traffic"] is None or "rocprofv3" in r["traffic_source"] or "look-up" in r["traffic_source"]
    if "rocprofv3 --kernel-trace --pmc" in r.get("traffic_source", ""):
        assert 0.9 < r["traffic"] / r["bytes_per_launch"] < 1.3 and r["traffic_detail"]["FETCH_SIZE_dispatches"] >= 60
    cf = d["configs"]                                                                      # every other BASELINE configuration
    assert set(cf) == {"cfg2", "cfg4", "cfg4_baseline_R", "cfg5_shard", "ext_3v2"} and "R_min 0.5 / R_max 0.9" in cf["cfg4_baseline_R"]["workload"]
    assert cf["ext_3v2"]["value"] > 0 and cf["ext_3v2"]["roofline"]["bytes_per_launch"] > 0          # the two-evader extension at the reference's pursuer count (round 6)
    assert cf["cfg2"]["roofline"]["bytes_per_env"] == 1497 and cf["cfg5_shard"]["roofline"]["frac"] > 0
    for leg in ("cfg2", "cfg5_shard"):                                                     # the legs carry both figures too
        rl = cf[leg]["roofline"]
        assert rl["frac"] == rl["frac_kernel"] and rl["frac_step_rate"] > 0 and rl["kernel_samples"] == 256 and rl["step_us"] > 0
    assert len(cf["cfg4"]["generator_ms_per_episode"]) == 4 and cf["cfg4"]["value_incl_generator"] > 0


@pytest.mark.gpu
def test_bench_two_ranks_on_one_gpu_over_gloo():
    """The N > 1 path end to end as the driver launches it (torch.distributed.run, one rank per 'GPU'): on a 1-GPU
    box both ranks share cuda:0 and the collective runs over gloo (HNS_DIST_BACKEND) instead of RCCL."""
    env = dict(os.environ, HNS_DIST_BACKEND="gloo", MASTER_ADDR="127.0.0.1")
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                          "--master-port", "29533", os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "192", "--warmup", "16", "--envs", "4096"],
                         capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout            # rank 0 only
    d = json.loads(lines[0])
    # n_gpus counts DEVICES (both ranks share cuda:0 here); the rank count is reported beside it
    assert d["n_gpus"] == 1 and d["config"]["ranks"] == 2 and d["config"]["sharding"].endswith("x2") and "all-gather" in d["config"]["collective"]
    assert abs(d["value"] - 2 * 4096 * 3 / (d["ms_per_step"] * 1e-3)) / d["value"] < 1e-3      # whole-job aggregate
    assert d["cpu_baseline"] is None              # rank 0 at N = 1 only
    # a rank's clock stops when ITS steps are complete on its device; the closing barrier's own latency is reported beside the line, not inside ms_per_step
    assert d["closing_barrier_us"] is not None and d["closing_barrier_us"] >= 0.0


@pytest.mark.gpu
def test_bench_launches_its_own_ranks():
    """`python bench.py --gpus 2` with no launcher around it starts two ranks itself and reports the rank count it
    OBSERVED (an all-reduce of ones), with the per-rank kernel times (gloo on a 1-GPU box)."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env["HNS_DIST_BACKEND"] = "gloo"
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "128", "--warmup", "8", "--envs", "4096"],
                         capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout
    d = json.loads(lines[0])
    assert d["n_gpus"] == 1 and d["config"]["ranks"] == 2 and d["config"]["world_size_launched"] == 2
    k = d["roofline"]["kernel_us_by_rank"]
    assert len(k["all"]) == 2 and 0 < k["min"] <= k["max"]
    cu = d["collective_us"]                                  # the all-gather per rollout is timed (two rollouts of 64 steps here)
    assert cu["rollouts"] == 2 and 0 < cu["per_rollout_us_mean"] <= cu["per_rollout_us_max"]
    assert abs(d["value"] - 2 * 4096 * 3 / (d["ms_per_step"] * 1e-3)) / d["value"] < 1e-3


@pytest.mark.gpu
def test_bench_refuses_to_fold_rccl_ranks_onto_one_gpu():
    """With the RCCL backend two ranks need two devices: on a 1-GPU box the launch fails loudly instead of reporting n_gpus 2."""
    import torch
    if torch.cuda.device_count() != 1:
        pytest.skip("needs a box with exactly one GPU")
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "HNS_DIST_BACKEND")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "16", "--warmup", "2", "--envs", "4096"],
                         capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    assert out.returncode != 0 and "refuse to fold" in (out.stderr + out.stdout)


@pytest.mark.gpu
def test_bench_loop_with_two_hip_shards_reproduces_the_whole_batch():
    """The multi-GPU plumbing end to end THROUGH bench.py's own loop (steps, episode-boundary resets, the per-rollout collective), with the
    shards stepped by the HIP kernels: two ranks (gloo, both on cuda:0) over env slices [0, 4096) and [4096, 8192) leave exactly the state one
    rank leaves for the whole 8192-env batch — slice by slice, sha256 of every buffer.  What the first real 8-GPU run adds is RCCL, not logic."""
    common = ["--steps", "96", "--warmup", "8", "--episode", "40", "--no-cpu-baseline", "--tp-steps", "0", "--config-steps", "0", "--abi-steps", "0", "--no-traffic-live"]
    one = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--envs", "8192", "--state-digest", "4", *common],
                         capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert one.returncode == 0, one.stderr[-2000:]
    env = dict(os.environ, HNS_DIST_BACKEND="gloo", MASTER_ADDR="127.0.0.1")
    two = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                          "--master-port", "29541", os.path.join(ROOT, "bench.py"), "--gpus", "2", "--envs", "4096", "--state-digest", "4", *common],
                         capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    assert two.returncode == 0, two.stderr[-2000:]
    d1 = json.loads([ln for ln in one.stdout.splitlines() if ln.startswith("{")][0])
    d2 = json.loads([ln for ln in two.stdout.splitlines() if ln.startswith("{")][0])
    assert len(d1["state_digest"]) == 4 and d1["state_digest"] == d2["state_digest"]
    assert len(set(d1["state_digest"])) == 4                        # four different slices, not four times the same bytes
    assert d2["config"]["ranks"] == 2 and d2["collective_us"]["rollouts"] == 1


@pytest.mark.gpu
def test_bench_dumps_the_outputs_of_its_last_timed_step(tmp_path):
    """`--dump-outputs DIR`: what the last step of the timed region handed its caller, one float32 / float64 .npy per leaf of the stepped tensordict,
    the same bytes from run to run.  Episodes of 20 steps: after 8 warm-up + 12 timed steps every env is done — those are the step's outputs, copied
    before the boundary's reset rewrites them — and after 8 + 11 none is, so --steps sets the step that is dumped.  At 65 536 envs the whole tree
    exceeds the 64 MB cap and a fixed sample of envs is written."""
    import numpy as np
    common = ["--gpus", "1", "--envs", "65536", "--warmup", "8", "--episode", "20", "--settle-steps", "100", "--no-cpu-baseline", "--tp-steps", "0",
              "--config-steps", "0", "--abi-steps", "0", "--no-traffic-live"]
    dumps = {}
    for tag, steps in (("a", 12), ("b", 12), ("c", 11)):
        d = tmp_path / tag
        out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", str(steps), "--dump-outputs", str(d), *common],
                             capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert out.returncode == 0, out.stderr[-2000:]
        assert json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][0])["steps"] == steps
        assert sum(f.stat().st_size for f in d.iterdir()) <= 64e6
        dumps[tag] = {f.name[:-4]: np.load(f) for f in d.iterdir()}
    a, b, c = dumps["a"], dumps["b"], dumps["c"]
    assert set(a) == set(b) == set(c) and {"next.agents.observation.state_self", "next.agents.reward", "next.done", "env_index"} <= set(a)
    for k in a:
        assert a[k].dtype in (np.float32, np.float64) and np.array_equal(a[k], b[k], equal_nan=True), k
    idx = a["env_index"]
    assert 0 < len(idx) < 65536 and np.all(np.diff(idx) > 0) and idx[-1] < 65536 and all(v.shape[0] == len(idx) for v in a.values())
    assert np.all(a["next.done"] == 1) and np.all(c["next.done"] == 0)
    assert not np.array_equal(a["next.agents.observation.state_self"], c["next.agents.observation.state_self"])


@pytest.mark.gpu
def test_bench_under_torchrun_with_one_rccl_rank():
    """Multi-GPU day one: the driver launches `python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N`.  With ONE rank
    torchrun still sets WORLD_SIZE / RANK / MASTER_*, so bench.py runs its launched-by-torchrun branch; HNS_BENCH_FORCE_DIST=1 makes it initialise the
    process group with the RCCL backend ("nccl") and take the distributed branch of its loop even at world size 1 — the RCCL all-gather of the
    rollout moments, the events around it, the per-rank kernel times and the device count execute on hardware before an 8-GPU node ever sees them."""
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = dict(os.environ, HNS_BENCH_FORCE_DIST="1", HNS_DIST_BACKEND="nccl", HSA_ENABLE_IPC_MODE_LEGACY="0", MASTER_ADDR="127.0.0.1")
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1",
                          "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "128", "--warmup", "8", "--envs", "4096",
                          "--no-cpu-baseline", "--tp-steps", "0", "--config-steps", "0", "--abi-steps", "0", "--no-traffic-live"],
                         capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    assert out.returncode == 0, out.stdout[-1000:] + out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout
    d = json.loads(lines[0])
    assert d["n_gpus"] == 1 and d["config"]["ranks"] == 1 and d["config"]["world_size_launched"] == 1 and d["config"]["dist_backend"] == "nccl"
    cu = d["collective_us"]
    assert cu["rollouts"] == 2 and "RCCL" in cu["what"] and 0 < cu["per_rollout_us_mean"] <= cu["per_rollout_us_max"] < 50_000
    k = d["roofline"]["kernel_us_by_rank"]
    assert len(k["all"]) == 1 and k["min"] == k["max"] > 0
    assert abs(d["value"] - 4096 * 3 / (d["ms_per_step"] * 1e-3)) / d["value"] < 1e-3


def _profile_header(path):
    """(avg us, frac) of the first `# kernel ...` line of a profiles/*.txt composed by tools/make_profile_txt.py."""
    import re
    for ln in open(path):
        m = re.match(r"# kernel `[^`]+`: (\d+) launches, avg ([0-9.]+) us .* = ([0-9.]+) of (8 TB/s|the 2.5 PF)", ln)
        if m:
            return int(m.group(1)), float(m.group(2)), float(m.group(3))
    raise AssertionError(f"{path}: no kernel line in the header")


def test_committed_bench_line_agrees_with_the_committed_profiles():
    """the round's committed bench line (profiles/r06_bench_final.json) and the rocprofv3 summaries of the same build
    (profiles/r06_*.txt, headers computed from their tables) must tell the same story: |line.frac - profile.frac| <= 5 % of the profile's
    (and <= 0.03 absolute) for the 3v1 step kernel, the 6v2 shard and the predictor.  Skipped until the round's files exist."""
    prof = os.path.join(ROOT, "profiles")
    line_path = os.path.join(prof, "r06_bench_final.json")
    if not os.path.exists(line_path):
        pytest.skip("profiles/r06_bench_final.json not committed yet")
    d = json.loads([ln for ln in open(line_path) if ln.startswith("{")][-1])
    pairs = [("r06_v4_step_kernel.txt", d["roofline"]["frac"], d["roofline"]["kernel_us"]),
             ("r06_step_kernel_a6t2.txt", d["configs"]["cfg5_shard"]["roofline"]["frac"], d["configs"]["cfg5_shard"]["roofline"]["kernel_us"]),
             ("r06_tp_observe.txt", d["tp_mode"]["roofline"]["frac"], d["tp_mode"]["observe_us"])]
    for name, frac, us in pairs:
        path = os.path.join(prof, name)
        assert os.path.exists(path), f"{name} is missing beside r06_bench_final.json"
        n, avg_us, pfrac = _profile_header(path)
        assert n >= 50, f"{name}: only {n} launches profiled"
        assert abs(frac - pfrac) <= max(0.05 * pfrac, 1e-4) and abs(frac - pfrac) <= 0.03, f"{name}: line frac {frac} ({us} us) vs profile {pfrac} ({avg_us} us)"
