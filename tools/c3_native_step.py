#!/usr/bin/env python3
"""
`--steps` (default 1) eager fwd+bwd steps of the C-GCN classifier (C3: BiLSTM 200 + 2-layer GCN, B=50 T=100, tools/model_step.py's
batch) with the BiLSTM on the native recurrence (opt['gcn_native_rnn']), nothing else: the program to trace with
`rocprofv3 --kernel-trace --stats -- python3 tools/c3_native_step.py` for a per-kernel summary of one step.  `--torch-rnn`: the same
step on MIOpen's LSTM.
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gcn_over_pruned_trees_amd.model import gcn  # noqa: E402
from gcn_over_pruned_trees_amd.utils import synthetic  # noqa: E402
from model_step import opt_for  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=1)
    ap.add_argument("--dtype", choices=["fp32", "bf16"], default="fp32")
    ap.add_argument("--torch-rnn", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    B, T = 50, 100
    tb = synthetic.random_tree_batch(1236, B, T, "tacred")
    rng = np.random.RandomState(7)
    t = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dev)  # noqa: E731
    words = rng.randint(2, 5000, size=(B, T)).astype(np.int64)
    words[tb["masks"]] = 0
    inputs = (t(words), t(tb["masks"]), t(rng.randint(0, 47, size=(B, T)).astype(np.int64)), t(rng.randint(0, 15, size=(B, T)).astype(np.int64)),
              t(tb["deprel"]), t(tb["head"]), t(tb["subj_pos"]), t(tb["obj_pos"]))
    labels = t(rng.randint(0, 42, size=(B,)).astype(np.int64))
    torch.manual_seed(1234)
    model = gcn.GCNClassifier(opt_for(True, a.dtype, native_rnn=not a.torch_rnn)).to(dev).train()
    for _ in range(a.steps):
        model.zero_grad(set_to_none=True)
        logits, pooled = model(inputs)
        loss = torch.nn.functional.cross_entropy(logits, labels) + 0.003 * (pooled ** 2).sum(1).mean()
        loss.backward()
    torch.cuda.synchronize()
    print("loss %.6f after %d step(s)" % (float(loss), a.steps))


if __name__ == "__main__":
    main()
