"""
bench.py as the driver invokes it: `python bench.py --gpus N` must start N ranks itself (the reference has no
distributed entry point at all, train_cgcn.sh:5 picks one GPU).  CPU tests cover the refusals that need no GPU; the `gpu` test
runs the real self-launch with two ranks sharing the one GPU of the box over gloo (GCNPT_BENCH_ONE_DEVICE=1).  --dump-outputs: its size
cap and row sample on the CPU, its arrays against the CPU oracle on the GPU.  A plain run against --full: which fields each prints.
"""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
FAST = ["--no-cpu-baseline", "--no-kernel-breakdown", "--no-pooled-only", "--no-secondary", "--no-secondary-shapes"]


def _run(args, env=None, timeout=600):
    e = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    e.update(env or {})
    return subprocess.run([sys.executable, BENCH] + args, env=e, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout)


def test_gpus_must_agree_with_world_size():
    """Under a launcher (WORLD_SIZE set) a different --gpus is refused before anything touches a GPU."""
    r = _run(["--gpus", "2"], env={"WORLD_SIZE": "3", "RANK": "0", "LOCAL_RANK": "0"})
    assert r.returncode == 2 and b"must agree" in r.stderr, r.stderr[-500:]


def test_self_launch_refuses_more_ranks_than_gpus():
    """No GPU here: --gpus 2 must not silently run one rank (round 1 did: it printed n_gpus 1 and exited 0)."""
    import torch
    if torch.cuda.device_count() >= 2:
        pytest.skip("two GPUs visible")
    env = {k: "" for k in ()}
    r = _run(["--gpus", "2"] + FAST, env=env)
    assert r.returncode != 0 and r.stdout.strip() == b"" and b"GPU(s) visible" in r.stderr, (r.returncode, r.stderr[-500:])


@pytest.mark.gpu
def test_self_launch_two_ranks_one_device():
    """The real entry: the parent starts 2 fresh ranks (before any GPU call of its own), they share GPU 0 and exchange the flat
    gradient bucket over gloo.  Same shard on both ranks, so the reduced bucket must be 2 x the one-rank bucket."""
    common = ["--steps", "40", "--warmup", "5", "--launch", "native"] + FAST
    one = _run(["--gpus", "1"] + common, env={"GCNPT_BENCH_SAME_SHARD": "1"})
    assert one.returncode == 0, one.stderr[-2000:]
    l1 = [ln for ln in one.stdout.decode().splitlines() if ln.startswith("{")]
    assert len(l1) == 1
    d1 = json.loads(l1[0])
    assert d1["n_gpus"] == 1
    two = _run(["--gpus", "2", "--dist-backend", "gloo", "--full"] + common,                # --full: async_upper_bound beside the headline
               env={"GCNPT_BENCH_ONE_DEVICE": "1", "GCNPT_BENCH_SAME_SHARD": "1"})
    assert two.returncode == 0, two.stderr[-3000:]
    l2 = [ln for ln in two.stdout.decode().splitlines() if ln.startswith("{")]
    assert len(l2) == 1, two.stdout[-2000:]                              # ONE JSON line, from rank 0
    d2 = json.loads(l2[0])
    assert d2["n_gpus"] == 2 and d2["config"]["world_size"] == 2 and d2["config"]["global_batch"] == 2 * d1["config"]["global_batch"]
    assert d2["config"]["ranks_started_by"].startswith("bench.py itself")
    assert len(d2["config"]["ms_per_step_by_rank"]) == 2
    assert d2["scaling"] == "weak" and d2["value"] > 0
    g1, g2 = d1["config"]["grad_bucket_abs_sum"], d2["config"]["grad_bucket_abs_sum"]
    assert g1 > 0 and abs(g2 - 2 * g1) <= 2e-3 * g2, (g1, g2)            # float atomics reorder the sums: not bit-exact
    # the N > 1 headline is SYNCHRONOUS SGD: every step's all-reduce feeds a device-side update the next step's pack reads
    assert d2["config"]["dp_mode"].startswith("synchronous SGD") and d2["config"]["weight_abs_drift_after_timed_steps"] > 0
    assert "async_upper_bound" in d2 and "NOT synchronous" in d2["async_upper_bound"]["note"]
    assert d1["config"]["dp_mode"] == "none (1 GPU)"


@pytest.mark.gpu
def test_plain_run_is_the_headline_alone_and_full_adds_the_rest():
    """A plain run prints the headline and nothing that needs runs of its own; --full adds the repeats, the secondary steps and
    shapes, the per-kernel breakdown with its roofline and launch floor, and the CPU baseline (kept short here)."""
    extra = ("ms_per_step_repeats", "with_prune", "with_cached_trees", "fp32", "with_pooling", "pooled_only_rows", "roofline", "kernels",
             "step_roofline", "launch_floor_us", "secondary_shapes", "cpu_baseline")
    lines = {}
    for name, flags in (("plain", []), ("full", ["--full", "--repeats", "2", "--cpu-seconds", "0.2"])):
        r = _run(["--gpus", "1", "--steps", "20", "--warmup", "5"] + flags)
        assert r.returncode == 0, (name, r.stderr[-2000:])
        ln = [x for x in r.stdout.decode().splitlines() if x.startswith("{")]
        assert len(ln) == 1, (name, r.stdout[-2000:])
        lines[name] = json.loads(ln[0])
    for d in lines.values():
        assert d["metric"] == "GCN-layer fwd+bwd sentences/sec at batch=50 seq=100 h=200" and d["unit"] == "sentences/s"
        assert d["higher_is_better"] is True and d["dtype"] == "bf16" and d["steps"] == 20 and d["warmup"] == 5
        assert d["value"] > 0 and abs(d["value"] - 50 / (d["ms_per_step"] * 1e-3)) <= 1e-6 * d["value"]
    plain, full = lines["plain"], lines["full"]
    assert [k for k in extra if plain.get(k) is not None] == [] and plain["ms_per_step_median"] is None, sorted(plain)
    assert [k for k in extra if full.get(k) is None] == [] and full["ms_per_step_repeats"]["n"] == 2, sorted(full)


def test_dump_outputs_stays_under_cap_with_a_fixed_sample(tmp_path):
    """--dump-outputs writes float32 .npy files, at most 64 MB in all: above that, every 2-D array keeps the same seeded rows (the same
    ones in every run, and in every array with that row count); 1-D arrays stay whole."""
    import numpy as np
    import torch

    import bench
    n = 40000
    h = torch.randn(n, 300)
    dx = torch.randn(n, 600)
    dx[:, 0] = torch.arange(n, dtype=torch.float32)                    # row ids, to find which rows were kept
    arrays = {"h": h.to(torch.bfloat16), "dx": dx, "db": torch.randn(300)}
    assert 4 * sum(a.numel() for a in arrays.values()) > bench.DUMP_BYTES
    got = []
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), arrays)
        assert sum(f.stat().st_size for f in (tmp_path / d).iterdir()) <= bench.DUMP_BYTES
        got.append({f.stem: np.load(f) for f in (tmp_path / d).iterdir()})
    a, b = got
    assert sorted(a) == ["db", "dx", "h"] and all(v.dtype == np.float32 for v in a.values())
    assert all(np.array_equal(a[k], b[k]) for k in a)
    assert np.array_equal(a["db"], arrays["db"].numpy())
    rows = a["dx"][:, 0].astype(np.int64)
    assert 0 < len(rows) < n and np.all(np.diff(rows) > 0)
    assert np.array_equal(a["dx"], dx.numpy()[rows]) and np.array_equal(a["h"], arrays["h"].float().numpy()[rows])


@pytest.mark.gpu
def test_dump_outputs_are_what_the_timed_step_computed(tmp_path):
    """--dump-outputs at fp32 without dropout: the arrays of the last timed step match the CPU oracle on the same seeded inputs
    (rank 0's shard seed 1234), whatever the number of steps and the launch mode."""
    import numpy as np

    from gcn_over_pruned_trees_amd.utils import synthetic
    from helpers import FWD_RTOL, GRAD_RTOL, max_rel
    from oracle import gcn_ref, prune_ref
    B, T, Din, H = 4, 20, 200, 200
    tb = synthetic.random_tree_batch(1234, B, T, "full")
    Ws, bs = synthetic.layer_params(1235, [Din, H, H])
    x, gy = synthetic.normal(1236, (B, T, Din)), synthetic.normal(1237, (B, T, H))
    adj = prune_ref.batch_adj(tb["head"], tb["subj_pos"], tb["obj_pos"], tb["deprel"], tb["lens"], 1)["adj"]
    h1, _ = gcn_ref.gcn_forward(adj, x, Ws[:1], bs[:1])
    h2, _ = gcn_ref.gcn_forward(adj, x, Ws, bs)
    dx, dWs, dbs = gcn_ref.gcn_backward(adj, x, Ws, bs, gy)
    want = dict(h1=h1, h2=h2, dx=dx, dW0=dWs[0], db0=dbs[0], dW1=dWs[1], db1=dbs[1])
    shape = ["--batch", str(B), "--seq", str(T), "--din", str(Din), "--hidden", str(H), "--dtype", "fp32", "--drop", "0", "--repeats", "1"]
    for steps, launch in (("3", "native"), ("7", "graph")):
        out = tmp_path / launch
        r = _run(["--gpus", "1", "--steps", steps, "--warmup", "1", "--launch", launch, "--dump-outputs", str(out)] + shape + FAST)
        assert r.returncode == 0, r.stderr[-2000:]
        got = {f.stem: np.load(f) for f in out.iterdir()}
        assert sorted(got) == sorted(want) and all(v.dtype == np.float32 for v in got.values())
        for k, v in want.items():
            v = v.reshape(-1, v.shape[-1]) if v.ndim == 3 else v                # [B, T, *] activations are dumped as [rows, *]
            assert got[k].shape == v.shape, (k, got[k].shape, v.shape)
            err = max_rel(got[k], v)
            assert err <= (FWD_RTOL if k in ("h1", "h2") else GRAD_RTOL), (launch, k, err)
