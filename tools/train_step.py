#!/usr/bin/env python3
"""
The C2 module step of tools/model_step.py (GCNClassifier, 2-layer GCN, no LSTM, B=50 T=100 hidden=200, native embedding front end and
native head, fp32, trees pruned in the step) PLUS the update, reference train.py:225-227, as an A/B in ONE process:
  A  dense word-table gradient + torch.nn.utils.clip_grad_norm_ + torch.optim.SGD.step() + zero_grad()       (the existing behaviour)
  B  opt['gcn_sparse_emb_grad'] + gcn_over_pruned_trees_amd.optim.get_optimizer('sgd' | 'adagrad').step()    (csrc/optim_kernels.hip)
for vocab_size 5 000 and 50 000, launched eagerly and as one torch.cuda.graph per arm.  Both models are built first; then R rounds
(default 5) of N steps (default 100) alternate A, B, A, B, ...  Prints one JSON object: every round's ms per step with the median and
the spread (max - min) per arm and cell.
  --optim sgd|adagrad   arm A's Adagrad is torch.optim.Adagrad(initial_accumulator_value=0.1) (dense only; the reference's MyAdagrad is Python)
  --arm A|B --vocab V --steps N [--graph]   only that arm, N steps after 10 warm-up steps: the form to put under a kernel trace
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gcn_over_pruned_trees_amd import optim  # noqa: E402
from gcn_over_pruned_trees_amd.model import gcn  # noqa: E402
from gcn_over_pruned_trees_amd.utils import synthetic  # noqa: E402

B, T, MAX_GRAD_NORM, LR = 50, 100, 5.0, 1.0


def opt_for(vocab, sparse):
    return dict(vocab_size=vocab, emb_dim=300, pos_dim=30, ner_dim=30, hidden_dim=200, num_layers=2, input_dropout=0.5, gcn_dropout=0.5,
                word_dropout=0.04, emb_dropout=0.0, topn=1e10, prune_k=1, pooling="max", pooling_l2=0.003, mlp_layers=2, no_adj=False,
                rnn=False, rnn_hidden=200, rnn_layers=1, rnn_dropout=0.5, cuda=True, dataset="tacred", num_class=42, adj_type="regular",
                gcn_dtype="fp32", gcn_check_trees=False, gcn_graph_rng=True, gcn_native_embed=True, gcn_native_head=True,
                gcn_sparse_emb_grad=sparse)


def make_step(arm, vocab, kind, dev):
    tb = synthetic.random_tree_batch(1236, B, T, "tacred")
    rng = np.random.RandomState(7)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    words = rng.randint(2, vocab, size=(B, T)).astype(np.int64)
    words[tb["masks"]] = 0
    inputs = (t(words), t(tb["masks"]), t(rng.randint(0, 47, size=(B, T)).astype(np.int64)), t(rng.randint(0, 15, size=(B, T)).astype(np.int64)),
              t(tb["deprel"]), t(tb["head"]), t(tb["subj_pos"]), t(tb["obj_pos"]))
    labels = t(rng.randint(0, 42, size=(B,)).astype(np.int64))
    torch.manual_seed(1234)
    model = gcn.GCNClassifier(opt_for(vocab, arm == "B")).to(dev).train()
    params = [p for p in model.parameters() if p.requires_grad]
    if arm == "B":
        opt = optim.get_optimizer(kind, params, LR, MAX_GRAD_NORM)
    elif kind == "sgd":
        opt = torch.optim.SGD(params, lr=LR)
    else:
        opt = torch.optim.Adagrad(params, lr=LR, initial_accumulator_value=0.1)

    def step():
        logits, pooled = model(inputs)
        loss = model.loss(logits, pooled, labels)
        loss.backward()
        if arm == "A":
            torch.nn.utils.clip_grad_norm_(model.parameters(), MAX_GRAD_NORM)
        opt.step()
        if arm == "A":
            opt.zero_grad()
        return loss.detach()
    return step


def captured(step):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    return graph.replay


def timed(run, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        run()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--optim", default="sgd", choices=["sgd", "adagrad"])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--vocabs", default="5000,50000")
    ap.add_argument("--arm", default="", choices=["", "A", "B"])
    ap.add_argument("--vocab", type=int, default=50000)
    ap.add_argument("--graph", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    out = {}
    if args.arm:
        run = make_step(args.arm, args.vocab, args.optim, dev)
        if args.graph:
            run = captured(run)
        for _ in range(10):
            run()
        out["%s_V%d_%s" % (args.arm, args.vocab, "graph" if args.graph else "eager")] = dict(ms_per_step=round(timed(run, args.steps) * 1e3, 4))
        print(json.dumps(out))
        return
    for vocab in (int(v) for v in args.vocabs.split(",")):
        for mode in ("eager", "graph"):
            runs = {arm: make_step(arm, vocab, args.optim, dev) for arm in ("A", "B")}
            if mode == "graph":
                runs = {arm: captured(s) for arm, s in runs.items()}
            for r in runs.values():
                for _ in range(10):
                    r()
            ms = {"A": [], "B": []}
            for _ in range(args.repeats):
                for arm in ("A", "B"):
                    ms[arm].append(round(timed(runs[arm], args.steps) * 1e3, 4))
            for arm in ("A", "B"):
                out["%s_V%d_%s" % (arm, vocab, mode)] = dict(ms_per_step=ms[arm], median=float(np.median(ms[arm])),
                                                            spread=round(max(ms[arm]) - min(ms[arm]), 4))
            del runs
            torch.cuda.synchronize()
    out["note"] = "C2 cell of tools/model_step.py (native embed + head, fp32, trees pruned in the step) plus the update; optim=%s, lr %g, " \
                  "max_grad_norm %g, B=%d T=%d; A = dense gradients + clip_grad_norm_ + torch optimizer + zero_grad, B = sparse word " \
                  "gradient + native step" % (args.optim, LR, MAX_GRAD_NORM, B, T)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
