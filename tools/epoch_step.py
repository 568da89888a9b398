#!/usr/bin/env python3
"""
Where a batch comes from, timed on the whole C2 training step of tools/train_step.py (GCNClassifier, 2-layer GCN, no LSTM, B=50 T=100
hidden=200, native embedding front end, native head, row-sparse word gradient, native SGD step, fp32, trees from a TreeCache), three arms
in ONE process over the same synthetic dataset (N batches of 50 TACRED-shaped sentences, each batch holding a 100-token sentence so that
every arm pads to T = 100):
  A  the host assembles the batch: vectorised NumPy word dropout on the batch's rows (loader.py:96-98), utils/staging.py
     PinnedStager.upload (fancy indexing, pad fills, seven pinned copies and a mask), the labels and the sentence numbers uploaded; eager
  B  DeviceDataset.batch from token arrays that stay in HBM (one launch, word dropout included; the sentence numbers uploaded); eager
  C  ONE captured hipGraph -- batch gather, TreeCache.batch, forward, loss, backward, optimizer step, and the add_ that advances the word
     dropout's device counter -- replayed per batch after a 400-byte copy of the sentence numbers into the captured idx tensor
Each arm has its own model (same initial weights) and optimizer.  R rounds (default 5) of K steps (default 100) that cycle
through the N batches (default 20) alternate A, B, C, A, ...; prints one JSON object: every round's ms per step with the median and the spread (max - min) per arm.
  --arm A|B|C --steps N    only that arm, N steps after 10 warm-up steps: the form to put under a kernel trace
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gcn_over_pruned_trees_amd import dataset, optim  # noqa: E402
from gcn_over_pruned_trees_amd.model import gcn  # noqa: E402
from gcn_over_pruned_trees_amd.utils import constant, staging, synthetic  # noqa: E402

B, T, VOCAB, P_WORD, MAX_GRAD_NORM, LR = 50, 100, 5000, 0.04, 5.0, 1.0
FIELDS = ("words", "pos", "ner", "deprel", "head", "subj_pos", "obj_pos")


def opt_for():
    return dict(vocab_size=VOCAB, emb_dim=300, pos_dim=30, ner_dim=30, hidden_dim=200, num_layers=2, input_dropout=0.5, gcn_dropout=0.5,
                word_dropout=P_WORD, emb_dropout=0.0, topn=1e10, prune_k=1, pooling="max", pooling_l2=0.003, mlp_layers=2, no_adj=False,
                rnn=False, rnn_hidden=200, rnn_layers=1, rnn_dropout=0.5, cuda=True, dataset="tacred", num_class=42, adj_type="regular",
                gcn_dtype="fp32", gcn_check_trees=False, gcn_graph_rng=True, gcn_native_embed=True, gcn_native_head=True,
                gcn_sparse_emb_grad=True)


def make_dataset(n_batches):
    """n_batches * B sentences padded to T; sentences j*B .. j*B + B - 1 form batch j, longest first, the first of them T tokens long."""
    rng = np.random.RandomState(7)
    parts = [synthetic.random_tree_batch(1236 + j, B, T, "tacred") for j in range(n_batches)]
    ds = {k: np.concatenate([p[k] for p in parts]) for k in ("deprel", "head", "subj_pos", "obj_pos", "lens")}
    live = ~np.concatenate([p["masks"] for p in parts])
    S = n_batches * B
    ds["words"] = rng.randint(2, VOCAB, size=(S, T)).astype(np.int64) * live
    ds["pos"] = rng.randint(1, constant.N_POS, size=(S, T)).astype(np.int64) * live
    ds["ner"] = rng.randint(1, constant.N_NER, size=(S, T)).astype(np.int64) * live
    ds["labels"] = rng.randint(0, 42, size=(S,)).astype(np.int64)
    return ds, [np.arange(j * B, (j + 1) * B, dtype=np.int64) for j in range(n_batches)]


def make_arm(arm, host, dev_ds, cache, dev):
    torch.manual_seed(1234)
    model = gcn.GCNClassifier(opt_for()).to(dev).train()
    opt = optim.get_optimizer("sgd", [p for p in model.parameters() if p.requires_grad], LR, MAX_GRAD_NORM)

    def train(inputs, labels, idx_dev):
        logits, pooled = model(inputs, trees=cache.batch(idx_dev, T))
        loss = model.loss(logits, pooled, labels)
        loss.backward()
        opt.step()
        return loss.detach()

    if arm == "A":
        stager = staging.PinnedStager({k: (torch.int64, 150 if k.endswith("_pos") else 0) for k in FIELDS}, B, T, dev)
        rng = np.random.RandomState(11)
        dropped = dict(host, words=host["words"].copy())

        def run(idx):
            w = host["words"][idx]
            drop = (rng.random_sample(w.shape) < P_WORD) & (w != constant.UNK_ID) & (w != constant.PAD_ID)
            dropped["words"][idx] = np.where(drop, constant.UNK_ID, w)
            out, masks, ev = stager.upload(dropped, idx)
            labels = torch.from_numpy(host["labels"][idx]).to(dev, non_blocking=True)
            idx_dev = torch.from_numpy(idx).to(dev, non_blocking=True)
            stager.ready(ev)
            return train((out["words"], masks) + tuple(out[k] for k in FIELDS[1:]), labels, idx_dev)
        return run
    if arm == "B":
        def run(idx):
            batch = dev_ds.batch(idx, T, word_dropout=P_WORD)
            return train(batch.inputs, batch.labels, batch.idx)
        return run
    idx_buf = torch.zeros((B,), dtype=torch.int64, device=dev)
    pinned = {}                                                       # one pinned copy per batch, written once: no buffer is reused while a copy may be in flight
    counter = torch.zeros((1,), dtype=torch.int64, device=dev)

    def step():
        counter.add_(1)
        batch = dev_ds.batch(idx_buf, T, word_dropout=P_WORD, seed=99, seed_dev=counter)
        return train(batch.inputs, batch.labels, idx_buf)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss = step()

    def run(idx):
        key = int(idx[0])
        if key not in pinned:
            pinned[key] = torch.from_numpy(idx).pin_memory()
        idx_buf.copy_(pinned[key], non_blocking=True)                 # 400 bytes, ordered on the stream between two replays
        graph.replay()
        return loss
    return run


def timed(run, batches, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(n):
        run(batches[i % len(batches)])
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--batches", type=int, default=20)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--arm", default="", choices=["", "A", "B", "C"])
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    host, batches = make_dataset(args.batches)
    dev_ds = dataset.DeviceDataset.build(*(host[k] for k in FIELDS), host["lens"], host["labels"], dev)
    cache = dev_ds.tree_cache(1, want_label=False)
    out = {}
    arms = [args.arm] if args.arm else ["A", "B", "C"]
    runs = {a: make_arm(a, host, dev_ds, cache, dev) for a in arms}
    for r in runs.values():
        for i in range(10):
            r(batches[i % len(batches)])
    ms = {a: [] for a in arms}
    for _ in range(1 if args.arm else args.repeats):
        for a in arms:
            ms[a].append(round(timed(runs[a], batches, args.steps) * 1e3, 4))
    for a in arms:
        out[a] = dict(ms_per_step=ms[a], median=float(np.median(ms[a])), spread=round(max(ms[a]) - min(ms[a]), 4))
    out["note"] = "C2 training step (native embed + head + SGD step, fp32, cached trees), B=%d T=%d, %d batches, %d steps per round; " \
                  "A = host assembly + PinnedStager.upload, B = DeviceDataset.batch eager, C = one captured graph per step replayed " \
                  "after a %d-byte idx copy" % (B, T, args.batches, args.steps, B * 8)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
