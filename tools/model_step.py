#!/usr/bin/env python3
"""
Full-model step times through the drop-in modules ("plus full-model step numbers for C3"), and the measured
device copy bandwidth (the denominator SURVEY asks for beside the nominal 8 TB/s).  Synthetic TACRED-shaped batch, random
weights; eager launches (ctypes + torch), one optimizer-free fwd+bwd per step.  Prints one JSON object.
  C2: GCNClassifier, 2-layer GCN, no LSTM, B=50 T=100 hidden=200 (emb 300 + pos 30 + ner 30)
  C3: the same with the BiLSTM in front (rnn_hidden 200), i.e. C-GCN; C3_cgcn_native_rnn: its BiLSTM on the native recurrence
      (opt['gcn_native_rnn'], model/rnn.py) instead of MIOpen's
  *_native_embed: the same cell with opt['gcn_native_embed'] (lookups, cat, dropouts, cast as one launch; csrc/embed_kernels.hip).
      Every cell has emb_dropout = 0, so neither front end runs its word-type dropout here: input_dropout = 0.5 is what both pay for
  *_native_head: the same cell with opt['gcn_native_head'] (out_mlp, classifier and the loss on csrc/head_kernels.hip).  Every cell's loss
      goes through model.loss, so each arm pays for its own loss: torch's cross_entropy + penalty chain, or head_loss
--cells A,B: only the named cells (C2_gcn, C2_gcn_native_embed, C3_cgcn, ...); --no-copy: skip the copy bandwidth measurement
--ab A,B [--repeats R]: A/B of two cells in ONE process: both models are built first, then R rounds (default 5) of 100 steps each,
      alternating A, B, A, B, ...; prints every round's ms per step with the median and the spread (max - min) per arm
--adj-type full_deprel|diagonal_deprel [--repeats R]: the relation-aware model (no LSTM, hidden 200, deprel_emb_dim 50; full_deprel: a 200-wide
      input, since its one shared weight serves every layer) in three arms built in ONE process -- `padded` (the default: gcn_check_trees
      on, in-tree compaction with its host sync), `padded_nocheck` (gcn_check_trees=False: all B*T rows, no sync), `packed` (gcn_packed:
      sum(len) rows, no sync; cached trees come from TreeCache.batch_packed with the host's row count) -- R rounds of 50 steps each,
      alternating the arms; per arm the forward alone and the whole step (forward + backward), median and spread over the rounds
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gcn_over_pruned_trees_amd.model import gcn, tree  # noqa: E402
from gcn_over_pruned_trees_amd.utils import synthetic  # noqa: E402


def opt_for(rnn, dtype, native_rnn=False, native_embed=False, native_head=False):
    return dict(vocab_size=5000, emb_dim=300, pos_dim=30, ner_dim=30, hidden_dim=200, num_layers=2, input_dropout=0.5, gcn_dropout=0.5,
                word_dropout=0.04, emb_dropout=0.0, topn=1e10, prune_k=1, pooling="max", pooling_l2=0.003, mlp_layers=2, no_adj=False,
                rnn=rnn, rnn_hidden=200, rnn_layers=1, rnn_dropout=0.5, cuda=True, dataset="tacred", num_class=42, adj_type="regular",
                gcn_dtype=dtype, gcn_check_trees=False, gcn_native_rnn=native_rnn, gcn_native_embed=native_embed, gcn_native_head=native_head)


def deprel_arms(args, dev, inputs, labels, B, T):
    """--adj-type: the three arms of a relation-aware model, alternating (see the module docstring)."""
    full = args.adj_type == "full_deprel"
    arms = (("padded", dict(gcn_check_trees=True)), ("padded_nocheck", dict()), ("packed", dict(gcn_packed=True)))
    n_rows = int((inputs[1] == 0).sum().item())
    idx = torch.arange(B, device=dev)
    cache = tree.TreeCache.build(inputs[5], inputs[6], inputs[7], inputs[4], 1, masks=inputs[1], want_label=True)
    out = dict(adj_type=args.adj_type, B=B, T=T, hidden=200, deprel_emb_dim=50, tokens=n_rows, steps_per_round=50, rounds=args.repeats)
    for dtype in ("fp32", "bf16"):
        models = {}
        for name, kw in arms:
            torch.manual_seed(1234)
            opt = dict(opt_for(False, dtype), adj_type=args.adj_type, deprel_emb_dim=50, emb_dim=140 if full else 300, **kw)
            models[name] = gcn.GCNClassifier(opt).to(dev).train()

        def run(name, cached, backward):
            model = models[name]
            model.zero_grad(set_to_none=True)
            trees = None
            if cached:
                trees = cache.batch_packed(idx, T, n_rows=n_rows) if name == "packed" else cache.batch(idx, T)
            logits, pooled = model(inputs, trees=trees)
            loss = model.loss(logits, pooled, labels)
            if backward:
                loss.backward()
            return loss.detach()

        def timed(name, cached, backward, n=50):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n):
                run(name, cached, backward)
            torch.cuda.synchronize()
            return round((time.perf_counter() - t0) / n * 1e3, 3)

        for cached in (False, True):
            for name, _ in arms:
                for _ in range(10):
                    run(name, cached, True)
            runs = {(name, part): [] for name, _ in arms for part in ("forward", "step")}
            for _ in range(args.repeats):
                for name, _ in arms:
                    runs[(name, "forward")].append(timed(name, cached, False))
                    runs[(name, "step")].append(timed(name, cached, True))
            for (name, part), v in runs.items():
                out["%s_%s_%s_%s" % (name, dtype, "cached_trees" if cached else "pruned_in_step", part)] = dict(
                    ms=v, median=float(np.median(v)), spread=round(max(v) - min(v), 3))
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--adj-type", default="regular", choices=("regular", "full_deprel", "diagonal_deprel"))
    ap.add_argument("--cells", default="")
    ap.add_argument("--no-copy", action="store_true")
    ap.add_argument("--ab", default="")
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    only = [c for c in args.cells.split(",") if c]
    dev = torch.device("cuda:0")
    B, T = 50, 100
    tb = synthetic.random_tree_batch(1236, B, T, "tacred")
    rng = np.random.RandomState(7)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    words = rng.randint(2, 5000, size=(B, T)).astype(np.int64)
    words[tb["masks"]] = 0
    inputs = (t(words), t(tb["masks"]), t(rng.randint(0, 47, size=(B, T)).astype(np.int64)), t(rng.randint(0, 15, size=(B, T)).astype(np.int64)),
              t(tb["deprel"]), t(tb["head"]), t(tb["subj_pos"]), t(tb["obj_pos"]))
    labels = t(rng.randint(0, 42, size=(B,)).astype(np.int64))
    if args.adj_type != "regular":
        deprel_arms(args, dev, inputs, labels, B, T)
        return
    out = {}
    cells = (("C2_gcn", False, False, False, False), ("C2_gcn_native_embed", False, False, True, False), ("C2_gcn_native_head", False, False, False, True),
             ("C2_gcn_native_embed_native_head", False, False, True, True), ("C3_cgcn", True, False, False, False),
             ("C3_cgcn_native_rnn", True, True, False, False), ("C3_cgcn_native_rnn_native_embed", True, True, True, False),
             ("C3_cgcn_native_rnn_native_embed_native_head", True, True, True, True))
    idx = torch.arange(B, device=dev)

    def make_step(name, dtype):
        _, rnn, native, embed, head = next(c for c in cells if c[0] == name)
        torch.manual_seed(1234)
        model = gcn.GCNClassifier(opt_for(rnn, dtype, native, embed, head)).to(dev).train()
        cache = tree.TreeCache.build(inputs[5], inputs[6], inputs[7], inputs[4], 1, masks=inputs[1], want_label=False)

        def step(cached):
            model.zero_grad(set_to_none=True)
            logits, pooled = model(inputs, trees=cache.batch(idx, T) if cached else None)
            loss = model.loss(logits, pooled, labels)      # trainer.py:94-100; opt['pooling_l2'] = 0.003, no conv_l2
            loss.backward()
            return loss.detach()        # no reference to the autograd graph survives the step (its AccumulateGrad nodes would pin a stream)
        return step

    def timed(step, cached, n=100):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            loss = step(cached)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n, loss

    if args.ab:
        a, b = args.ab.split(",")
        for dtype in ("fp32", "bf16"):
            steps = {a: make_step(a, dtype), b: make_step(b, dtype)}
            for cached in (False, True):
                for s in steps.values():
                    for _ in range(10):
                        s(cached)
                runs = {a: [], b: []}
                for _ in range(args.repeats):
                    for name in (a, b):
                        runs[name].append(round(timed(steps[name], cached)[0] * 1e3, 3))
                for name in (a, b):
                    out["%s_%s_%s" % (name, dtype, "cached_trees" if cached else "pruned_in_step")] = dict(
                        ms_per_step=runs[name], median=float(np.median(runs[name])), spread=round(max(runs[name]) - min(runs[name]), 3))
        print(json.dumps(out))
        return
    for name, _, _, _, _ in cells:
        if only and name not in only:
            continue
        for dtype in ("fp32", "bf16"):
            step = make_step(name, dtype)
            for cached in (False, True):
                for _ in range(10):
                    step(cached)
                dt, loss = timed(step, cached)
                out["%s_%s_%s" % (name, dtype, "cached_trees" if cached else "pruned_in_step")] = dict(
                    ms_per_step=round(dt * 1e3, 3), sentences_per_s=round(B / dt), loss=float(loss))
    if args.no_copy:
        print(json.dumps(out))
        return
    # device copy bandwidth: 1 GiB read + 1 GiB write per copy
    a = torch.empty((1 << 28,), dtype=torch.float32, device=dev)
    b = torch.empty_like(a)
    for _ in range(3):
        b.copy_(a)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(20):
        b.copy_(a)
    e1.record()
    torch.cuda.synchronize()
    out["copy_bandwidth_GBps"] = round(20 * 2 * a.numel() * 4 / (e0.elapsed_time(e1) * 1e-3) / 1e9, 1)
    out["note"] = "eager launches through the modules (no hipGraph): embeddings, optional BiLSTM (MIOpen, or the native recurrence in C3_cgcn_native_rnn), pruner or cached trees, GCN layers, " \
                  "fused pooling, MLP, loss, backward; B=50 T=100"
    print(json.dumps(out))


if __name__ == "__main__":
    main()
