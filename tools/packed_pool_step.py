#!/usr/bin/env python3
"""
A/B of the pooling on token-packed rows, in one process, A and B alternating: A = the layer stack's output unpacked to [B,T,H], pool3 on the
padded tensor, gcnpt_layers_bwd (what opt['gcn_pool_handover']=False keeps); B = the poolings on the packed rows with the dZ hand-over
(gcnpt_pool3_fwd_packed, gcnpt_pool3_bwd_dz_packed + gcnpt_layers_bwd_dz).  Op level (gcn_layers + pooling, forward and backward, bf16
and fp32) and model level (GCNClassifier with gcn_packed, trees from TreeCache.batch_packed, gcn_check_trees=False) at the C5 per-GPU
shard (B=16, T=300, 600 -> 300 -> 300, K=2) and at C2 (B=50, T=100, 360 -> 200 -> 200, K=1), TACRED-shaped lengths.  Each figure: a host
clock around 200 steps that end in a synchronise, after warm-up, five repeats; median, min and max in microseconds per step.  Prints one
JSON object and writes nothing else.
"""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gcn_over_pruned_trees_amd.model import gcn, tree  # noqa: E402
from gcn_over_pruned_trees_amd.utils import synthetic  # noqa: E402

STEPS, WARMUP, REPEATS = 200, 30, 5
SHAPES = {"C5_shard": dict(B=16, T=300, din=600, hid=300, K=2), "C2": dict(B=50, T=100, din=360, hid=200, K=1)}


def ab(step_a, step_b):
    """us per step of A and B: REPEATS timed regions each, alternating."""
    for f in (step_a, step_b):
        for _ in range(WARMUP):
            f()
    torch.cuda.synchronize()
    us = {"A": [], "B": []}
    for _ in range(REPEATS):
        for name, f in (("A", step_a), ("B", step_b)):
            t0 = time.perf_counter()
            for _ in range(STEPS):
                f()
            torch.cuda.synchronize()
            us[name].append((time.perf_counter() - t0) / STEPS * 1e6)
    out = {k: dict(median_us=round(float(np.median(v)), 2), min_us=round(min(v), 2), max_us=round(max(v), 2)) for k, v in us.items()}
    out["B_minus_A_us"] = round(out["B"]["median_us"] - out["A"]["median_us"], 2)
    return out


def op_level(dev, s, dtype):
    B, T, din, hid, K = s["B"], s["T"], s["din"], s["hid"], s["K"]
    tb = synthetic.random_tree_batch(1236, B, T, "tacred")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    subj, obj = t(tb["subj_pos"]), t(tb["obj_pos"])
    trees = tree.prune_to_csr(t(tb["head"]), subj, obj, t(tb["deprel"]), K, masks=t(tb["masks"]), want_label=False)
    packed = trees.pack(tb["lens"].tolist()).check()
    Wn, bn = synthetic.layer_params(5, [din, hid, hid])
    Ws = [t(w).requires_grad_() for w in Wn]
    bs = [t(b).requires_grad_() for b in bn]
    xp = t(synthetic.normal(6, (B, T, din))[~tb["masks"]]).to(dtype).requires_grad_()
    gp = t(synthetic.normal(7, (B, 3 * hid)))
    kw = dict(drop_p=[0.5, 0.0], seeds=[11, 0], compute_dtype=dtype, out_dtype=torch.float32)

    def run(handover):
        for p in Ws + bs + [xp]:
            p.grad = None
        if handover:
            pooled = gcn.gcn_layers(xp, Ws, bs, packed, pool=(subj, obj, "max"), **kw)
        else:
            pooled = gcn.pool3(packed.unpack_rows(gcn.gcn_layers(xp, Ws, bs, packed, **kw)), trees.pool_mask, subj, obj, "max")
        pooled.backward(gp)
    r = ab(lambda: run(False), lambda: run(True))
    r["rows"] = dict(packed=packed.N, padded=B * T)
    return r


def model_level(dev, s, dtype):
    B, T, K = s["B"], s["T"], s["K"]
    tb = synthetic.random_tree_batch(1236, B, T, "tacred")
    rng = np.random.RandomState(7)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    words = rng.randint(2, 5000, size=(B, T)).astype(np.int64)
    words[tb["masks"]] = 0
    inputs = (t(words), t(tb["masks"]), t(rng.randint(0, 47, size=(B, T)).astype(np.int64)), t(rng.randint(0, 15, size=(B, T)).astype(np.int64)),
              t(tb["deprel"]), t(tb["head"]), t(tb["subj_pos"]), t(tb["obj_pos"]))
    labels = t(rng.randint(0, 42, size=(B,)).astype(np.int64))
    emb = s["din"] - 60
    opt = dict(vocab_size=5000, emb_dim=emb, pos_dim=30, ner_dim=30, hidden_dim=s["hid"], num_layers=2, input_dropout=0.5, gcn_dropout=0.5,
               word_dropout=0.04, emb_dropout=0.0, topn=1e10, prune_k=K, pooling="max", pooling_l2=0.003, mlp_layers=2, no_adj=False, rnn=False,
               cuda=True, dataset="tacred", num_class=42, adj_type="regular", gcn_dtype=dtype, gcn_check_trees=False, gcn_packed=True)
    cache = tree.TreeCache.build(inputs[5], inputs[6], inputs[7], inputs[4], K, masks=inputs[1], want_label=False)
    idx = torch.arange(B, device=dev)
    N = int(tb["lens"].sum())
    models = {}
    for handover in (False, True):
        torch.manual_seed(1234)
        models[handover] = gcn.GCNClassifier(dict(opt, gcn_pool_handover=handover)).to(dev).train()

    def run(handover):
        model = models[handover]
        model.zero_grad(set_to_none=True)
        logits, pooled = model(inputs, trees=cache.batch_packed(idx, T, n_rows=N))
        loss = torch.nn.functional.cross_entropy(logits, labels) + 0.003 * (pooled ** 2).sum(1).mean()
        loss.backward()
    return ab(lambda: run(False), lambda: run(True))


def main():
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda:0")
    out = {"steps": STEPS, "warmup": WARMUP, "repeats": REPEATS,
           "A": "unpack_rows + pool3 + gcnpt_layers_bwd (gcn_pool_handover=False)", "B": "poolings on packed rows + dZ hand-over"}
    for name, s in SHAPES.items():
        for dtype, tag in ((torch.bfloat16, "bf16"), (torch.float32, "fp32")):
            out["op_%s_%s" % (name, tag)] = op_level(dev, s, dtype)
            out["model_%s_%s" % (name, tag)] = model_level(dev, s, tag)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
