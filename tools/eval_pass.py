#!/usr/bin/env python3
"""
One evaluation pass over a split (reference train.py:245-285), timed three ways in ONE process on the C2 model of tools/epoch_step.py
(GCNClassifier, 2-layer GCN, no LSTM, hidden 200, native embedding front end and head, fp32, trees from a TreeCache) over a synthetic split
of N batches of 50 TACRED-shaped sentences of mixed lengths (default N = 40: 2 000 sentences), the same weights and the same batch plan
(staging.length_buckets, each batch padded to its longest sentence) in every arm:
  A  the reference's way: per batch DeviceDataset.batch, forward, model.loss and its .item(), model.predict, .cpu().numpy().tolist() of the
     probabilities and the predictions, the sorted(zip(...)) unsort (trainer.py:117-124); then id -> label strings and a Python scorer
     loop over them (utils/scorer.py:20-96, restated)
  B  evaluate.Evaluator, eager: the same launches plus ONE scoring launch per batch, one finishing launch, one read at the end
  C  evaluate.Evaluator(graph=True): one captured graph per padded width (rounded up to 8), replayed after a copy of the sentence numbers
R rounds (default 5) of K passes (default 10) alternate A, B, C, A, ...; every pass ends with its result on the host.  Prints one JSON
object: every round's ms per pass with the median and the spread (max - min) per arm, and whether the three arms agree on the predictions
and on precision / recall / F1.
  --arm A|B|C --passes K    only that arm, K passes after 2 warm-up passes: the form to put under a kernel trace
"""
import argparse
import json
import os
import sys
import time
from collections import Counter

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from epoch_step import B, FIELDS, make_dataset, opt_for  # noqa: E402
from gcn_over_pruned_trees_amd import dataset, evaluate  # noqa: E402
from gcn_over_pruned_trees_amd.model import gcn  # noqa: E402
from gcn_over_pruned_trees_amd.utils import staging  # noqa: E402

NO_RELATION = "no_relation"


def score_strings(gold, guess):
    """Micro-averaged precision, recall and F1 over label strings, NO_RELATION counting neither as a guess nor as a gold relation."""
    correct, guessed, wanted = Counter(), Counter(), Counter()
    for g, p in zip(gold, guess):
        if p != NO_RELATION:
            guessed[p] += 1
        if g != NO_RELATION:
            wanted[g] += 1
            if g == p:
                correct[p] += 1
    c, n_guess, n_gold = sum(correct.values()), sum(guessed.values()), sum(wanted.values())
    prec = float(c) / float(n_guess) if n_guess > 0 else 1.0
    rec = float(c) / float(n_gold) if n_gold > 0 else 0.0
    f1 = 2.0 * prec * rec / (prec + rec) if prec + rec > 0.0 else 0.0
    return prec, rec, f1


def make_arm(arm, model, host, dev_ds, cache):
    """A callable that runs one pass and returns (predictions in the dataset's order as a list, (P, R, F1), loss figure)."""
    if arm == "A":
        batches = staging.length_buckets(host["lens"], B)
        names = [NO_RELATION] + ["rel_%d" % k for k in range(1, 42)]
        gold = [names[int(y)] for y in host["labels"]]

        def run():
            model.eval()
            preds, order, total = [], [], 0.0
            with torch.no_grad():
                for idx in batches:
                    batch = dev_ds.batch(idx)
                    logits, pooled = model(batch.inputs, trees=cache.batch(batch.idx, batch.T))
                    loss = model.loss(logits, pooled, batch.labels)
                    probs, pred = model.predict(logits)
                    probs = probs.cpu().numpy().tolist()
                    pred = pred.cpu().numpy().tolist()
                    _, pred, probs = [list(t) for t in zip(*sorted(zip(idx.tolist(), pred, probs)))]
                    preds += pred
                    order += sorted(idx.tolist())
                    total += loss.item()
            by_sentence = [0] * len(gold)
            for s, p in zip(order, preds):
                by_sentence[s] = p
            return by_sentence, score_strings(gold, [names[p] for p in by_sentence]), total / len(gold) * B
        return run
    ev = evaluate.Evaluator(model, dev_ds, B, cache=cache, graph=(arm == "C"))

    def run():
        res = ev.run()
        r = res.read()
        return res, (r["precision"], r["recall"], r["f1"]), r["loss"]
    return run


def timed(run, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        run()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--batches", type=int, default=40)
    ap.add_argument("--passes", type=int, default=10)
    ap.add_argument("--arm", default="", choices=["", "A", "B", "C"])
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    host, _ = make_dataset(args.batches)
    dev_ds = dataset.DeviceDataset.build(*(host[k] for k in FIELDS), host["lens"], host["labels"], dev)
    cache = dev_ds.tree_cache(1, want_label=False)
    torch.manual_seed(1234)
    model = gcn.GCNClassifier(opt_for()).to(dev).eval()
    arms = [args.arm] if args.arm else ["A", "B", "C"]
    runs = {a: make_arm(a, model, host, dev_ds, cache) for a in arms}
    first = {}
    for a in arms:
        for _ in range(2):
            first[a] = runs[a]()
    out = {}
    if not args.arm:
        pa = first["A"][0]
        agree = all(first[a][0].pred.cpu().numpy().tolist() == pa and first[a][1] == first["A"][1] for a in ("B", "C"))
        out["arms_agree"] = bool(agree)
        out["f1"] = first["A"][1][2]
    ms = {a: [] for a in arms}
    for _ in range(1 if args.arm else args.repeats):
        for a in arms:
            ms[a].append(round(timed(runs[a], args.passes) * 1e3, 3))
    for a in arms:
        out[a] = dict(ms_per_pass=ms[a], median=float(np.median(ms[a])), spread=round(max(ms[a]) - min(ms[a]), 3))
    out["note"] = "one evaluation pass, C2 model (native embed + head, fp32, cached trees), %d sentences in %d batches of %d, %d passes " \
                  "per round; A = per-batch read-backs + Python unsort + Python scorer, B = Evaluator eager, C = Evaluator(graph=True)" \
                  % (len(host["lens"]), args.batches, B, args.passes)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
