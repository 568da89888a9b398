#!/usr/bin/env python3
"""
The GCN stack of the BERT no-RNN model (reference train.py:105,143-144: emb_dim = 1024; model/gcn.py:136,235-236: BERT-large vectors
+ POS + NER straight into the GCN), B = 50, T = 100, 1084 -> 200 -> 200, one fwd+bwd per step through gcn_layers: in fp32 the first
layer takes the wide form (csrc/wide_kernels.hip).  --din / --hidden set other widths: e.g. --din 360 --hidden 768 (word ids + POS + NER
into a GCN as wide as a BERT-base vector) or --din 1084 --hidden 1024, where fp32 backward-data takes its wide form in both layers
(csrc/wide_bwd_kernels.hip).  As the yardstick, the same forward (and fwd+bwd) written the reference's way in
torch on the same GPU: dense adj.bmm + nn.Linear per layer (gcn.py:269-271, 390-392).  Prints one JSON object; run it under
`rocprofv3 --kernel-trace --stats -- python tools/bert_step.py` for the per-kernel times.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gcn_over_pruned_trees_amd.model import gcn, tree  # noqa: E402
from gcn_over_pruned_trees_amd.utils import synthetic  # noqa: E402


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(steps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return 1000.0 * t0.elapsed_time(t1) / steps          # us per step


def main(steps=50, warmup=10, din=1084, hidden=200):
    dev = torch.device("cuda:0")
    B, T, dims, K = 50, 100, [din, hidden, hidden], 1
    tb = synthetic.random_tree_batch(1236, B, T, "tacred")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    trees = tree.prune_to_csr(t(tb["head"]), t(tb["subj_pos"]), t(tb["obj_pos"]), t(tb["deprel"]), K, masks=t(tb["masks"]))
    adj = (trees.to_dense() != 0).float()
    Wn, bn = synthetic.layer_params(5, dims)
    x = t(synthetic.normal(6, (B, T, dims[0]))).requires_grad_()
    gy = t(synthetic.normal(7, (B, T, dims[-1])))
    Ws = [t(w).requires_grad_() for w in Wn]
    bs = [t(b).requires_grad_() for b in bn]
    res = dict(shape=dict(B=B, T=T, dims=dims, prune_k=K), steps=steps)
    for name, cd in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
        def fwd():
            with torch.no_grad():
                gcn.gcn_layers(x, Ws, bs, trees, compute_dtype=cd)

        def step():
            h = gcn.gcn_layers(x, Ws, bs, trees, compute_dtype=cd)
            h.backward(gy)
        res[name] = dict(fwd_us=round(timed(fwd, steps, warmup), 1), fwd_bwd_us=round(timed(step, steps, warmup), 1))

    lins = [torch.nn.Linear(dims[l], dims[l + 1]).to(dev) for l in range(2)]
    for lin, w, b in zip(lins, Wn, bn):
        lin.weight.data.copy_(t(w))
        lin.bias.data.copy_(t(b))
    denom = adj.sum(2).unsqueeze(2) + 1                     # gcn.py:261

    def torch_fwd():
        h = x
        for lin in lins:                                    # gcn.py:269-271, 390-392 (dropout 0)
            Ax = adj.bmm(h)
            AxW = lin(Ax) + lin(h)
            h = torch.relu(AxW / denom)
        return h

    def torch_nograd():
        with torch.no_grad():
            torch_fwd()

    def torch_step():
        torch_fwd().backward(gy)
    res["torch_reference_fp32"] = dict(fwd_us=round(timed(torch_nograd, steps, warmup), 1), fwd_bwd_us=round(timed(torch_step, steps, warmup), 1))
    print(json.dumps(res))


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.strip().splitlines()[0])
    ap.add_argument("--din", type=int, default=1084, help="input columns of the first layer")
    ap.add_argument("--hidden", type=int, default=200, help="hidden width of both layers")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    a = ap.parse_args()
    main(a.steps, a.warmup, a.din, a.hidden)
