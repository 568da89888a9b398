#!/usr/bin/env python3
"""
Generates tests/golden/e2e_wide_hidden.npz by IMPORTING the reference (read-only, /root/reference) and recording its outputs:
GCNClassifier with rnn = False and hidden_dim = 768, a GCN as wide as a BERT-base vector, on word ids (emb 300 + POS 30 + NER 30 =
360 input columns, model/gcn.py:136), 2 layers, max pooling, 2 MLP layers, prune_k = 1, every dropout 0.  Both GCN layers then
contract over 768 columns in their backward-data, wider than the row-tile kernel holds in fp32.

Only data is written.  The inputs and every parameter are regenerated from seeds by the test (utils/synthetic.py); the file keeps
the seeds, the checksums of what they give, and the reference's outputs: logits, pooled output, and the gradients of
L = sum(logits * g_logits) + sum(pooled * g_pooled) with respect to the word / POS / NER tables, both GCN biases and both GCN
weights (each weight gradient kept as every 16th column and a seeded projection onto 8 columns, to stay small).
Re-run:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_wide_hidden.py
"""
import json
import os
import sys

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("GCNPT_REFERENCE", "/root/reference")
sys.path.insert(0, ROOT)
sys.path.insert(0, REF)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from model.gcn import GCNClassifier  # noqa: E402  (reference)

from gcn_over_pruned_trees_amd.utils import synthetic  # noqa: E402  (this repo)

META = json.dumps(dict(torch=torch.__version__, numpy=np.__version__, python=sys.version.split()[0],
                       reference="gstoica27/gcn-over-pruned-trees"))
SEED = 3031
B, T, VOCAB, HIDDEN = 6, 36, 12, 768
LENS = np.array([36, 31, 27, 22, 15, 9], np.int32)


def opt():
    return dict(vocab_size=VOCAB, emb_dim=300, pos_dim=30, ner_dim=30, hidden_dim=HIDDEN, num_layers=2, input_dropout=0.0, gcn_dropout=0.0,
                emb_dropout=0.0, word_dropout=0.0, topn=10 ** 10, deprel_emb_dim=200, adj_type="regular", prune_k=1, pooling="max",
                mlp_layers=2, pooling_l2=0.003, conv_l2=0.0, rnn=False, rnn_hidden=200, rnn_layers=1, rnn_dropout=0.0, cuda=False,
                dataset="tacred", num_class=42, no_adj=False)


def inputs(seed=SEED):
    """The batch (shared with the test): trees, word / POS / NER ids (0 = PAD on padding)."""
    tb = synthetic.random_tree_batch(seed, B, T, LENS)
    rng = np.random.RandomState(seed + 1)
    words = rng.randint(2, VOCAB, size=(B, T)).astype(np.int64)
    pos = rng.randint(2, 47, size=(B, T)).astype(np.int64)
    ner = rng.randint(2, 15, size=(B, T)).astype(np.int64)
    for a in (words, pos, ner):
        a[tb["masks"]] = 0
    return tb, words, pos, ner


def params(shapes, seed=SEED):
    """Every parameter of the state dict, in sorted key order, from its own seed: N(0, 1) / sqrt(fan_in) for matrices, 0.1 N(0, 1)
    for vectors; row 0 of the embedding tables (their padding row) zero."""
    out = {}
    for i, k in enumerate(sorted(shapes)):
        shape = tuple(shapes[k])
        a = synthetic.normal(seed + 100 + i, shape)
        a = a / np.float32(np.sqrt(shape[-1])) if len(shape) > 1 else a * np.float32(0.1)
        if k.endswith("emb.weight"):
            a[0] = 0.0
        out[k] = a.astype(np.float32)
    return out


def main():
    torch.manual_seed(0)
    model = GCNClassifier(opt())
    shapes = {k: list(v.shape) for k, v in model.state_dict().items()}
    p = params(shapes)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in p.items()}, strict=True)
    model.train()                                     # every dropout is 0: the training forward is the eval forward
    tb, words, pos, ner = inputs()
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731
    batch = (t(words), t(tb["masks"]), t(pos), t(ner), t(tb["deprel"]), t(tb["head"]), t(tb["subj_pos"]), t(tb["obj_pos"]))
    logits, pooled = model(batch)
    g_logits, g_pooled = synthetic.normal(SEED + 3, tuple(logits.shape)), synthetic.normal(SEED + 4, tuple(pooled.shape))
    ((logits * t(g_logits)).sum() + (pooled * t(g_pooled)).sum()).backward()
    rel = model.gcn_model
    out = dict(meta=np.array(META), opt=np.array(json.dumps(opt())), seed=np.int64(SEED), B=np.int64(B), T=np.int64(T), lens=LENS,
               shapes=np.array(json.dumps(shapes)),
               words_sum=np.int64(words.sum()), pos_sum=np.int64(pos.sum()), ner_sum=np.int64(ner.sum()), head_sum=np.int64(tb["head"].sum()),
               logits=logits.detach().numpy(), pooling_output=pooled.detach().numpy(),
               d_emb=rel.emb.weight.grad.numpy(), d_pos_emb=rel.pos_emb.weight.grad.numpy(), d_ner_emb=rel.ner_emb.weight.grad.numpy())
    for l in range(2):
        dW = rel.gcn.W[l].weight.grad.numpy()
        proj = synthetic.normal(SEED + 5 + l, (dW.shape[1], 8))
        out["dW%d_cols16" % l] = dW[:, ::16].copy()
        out["dW%d_proj" % l] = (dW.astype(np.float64) @ proj).astype(np.float64)
        out["db%d" % l] = rel.gcn.W[l].bias.grad.numpy()
    for k, v in p.items():
        out["sum:" + k] = np.float64(v.astype(np.float64).sum())
    path = os.path.join(HERE, "e2e_wide_hidden.npz")
    np.savez_compressed(path, **out)
    print("%-28s %8.1f KB" % (os.path.basename(path), os.path.getsize(path) / 1024))


if __name__ == "__main__":
    torch.set_num_threads(4)
    main()
