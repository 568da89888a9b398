#!/usr/bin/env python3
"""
The output head alone, forward + backward, torch against opt['gcn_native_head']'s ops, A/B in ONE process: out_mlp (600 -> 200 -> 200, ReLU),
classifier (200 -> 42), CrossEntropyLoss + 0.003 * (pooled[:, :200] ** 2).sum(1).mean() on a [50, 600] pooled vector -- the bench shape
(tools/model_step.py).  Eager launches; a step ends without a sync, a round of --steps steps (default 500) ends in one.  --repeats rounds
(default 5) per arm, alternating torch, native, torch, native, ...  Prints one JSON object: every round's microseconds per step, the median
and the spread (max - min) per arm, and how far the two arms' losses and gradients are apart.
--arm torch|native: that arm only, one round -- for `rocprofv3 --kernel-trace --stats -- python tools/head_step.py --arm native`, whose
summary then holds the head's launches and nothing else (divide the call counts by steps + 10 warm-up steps).
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gcn_over_pruned_trees_amd.model import gcn  # noqa: E402

B, H, C, L2 = 50, 200, 42, 0.003


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--arm", default="")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(1234)
    layers = nn.ModuleList([nn.Linear(3 * H, H), nn.Linear(H, H), nn.Linear(H, C)]).to(dev)
    pooled = torch.randn(B, 3 * H, device=dev, requires_grad=True)      # it gets a gradient in the model: dX of the first layer is paid for
    labels = torch.from_numpy(np.random.RandomState(7).randint(0, C, size=(B,)).astype(np.int64)).to(dev)

    def step_torch():
        layers.zero_grad(set_to_none=True)
        pooled.grad = None
        x = F.relu(layers[1](F.relu(layers[0](pooled))))
        loss = F.cross_entropy(layers[2](x), labels) + L2 * (pooled[:, :H] ** 2).sum(1).mean()
        loss.backward()
        return loss.detach()

    def step_native():
        layers.zero_grad(set_to_none=True)
        pooled.grad = None
        x = gcn.linear_act(pooled, layers[0].weight, layers[0].bias, relu=True)
        x = gcn.linear_act(x, layers[1].weight, layers[1].bias, relu=True)
        loss = gcn.head_loss(gcn.linear_act(x, layers[2].weight, layers[2].bias), labels, pooled[:, :H], L2)
        loss.backward()
        return loss.detach()

    arms = {"torch": step_torch, "native": step_native}

    def timed(step):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            step()
        torch.cuda.synchronize()
        return round((time.perf_counter() - t0) / args.steps * 1e6, 2)

    if args.arm:
        for _ in range(10):
            arms[args.arm]()
        print(json.dumps({args.arm: dict(us_per_step=timed(arms[args.arm]), steps=args.steps, warmup=10)}))
        return
    out, grads = {}, {}
    for name, step in arms.items():
        for _ in range(10):
            loss = step()
        grads[name] = [float(loss)] + [p.grad.clone() for p in list(layers.parameters()) + [pooled]]
    rel = lambda a, b: float((a - b).abs().max() / b.abs().max())  # noqa: E731
    out["native_vs_torch"] = dict(loss=abs(grads["native"][0] - grads["torch"][0]) / abs(grads["torch"][0]),
                                  max_grad_rel=max(rel(a, b) for a, b in zip(grads["native"][1:], grads["torch"][1:])))
    runs = {name: [] for name in arms}
    for _ in range(args.repeats):
        for name, step in arms.items():
            runs[name].append(timed(step))
    for name, r in runs.items():
        out[name] = dict(us_per_step=r, median=float(np.median(r)), spread=round(max(r) - min(r), 2))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
