"""GPU tests of the native embedding front end (csrc/embed_kernels.hip, model.gcn.embed_inputs, opt['gcn_native_embed']).  The torch
expressions it replaces -- three lookups, cat, EmbeddingDropout, nn.Dropout, .to(bfloat16), pack_rows -- are written out here as the
reference.  The fp32 forward is exact by construction (a gather and two multiplications), so the forward checks are bit for bit."""
import json

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden
from helpers import GRAD_RTOL, cuda_dev, gcn_api, max_rel, prune, to_dev
from gcn_over_pruned_trees_amd.utils import synthetic

pytestmark = pytest.mark.gpu

V0, V1, V2 = 1000, 47, 15
P_EMB, P_IN = 0.3, 0.5
SEEDS = (20240607, 977)
S_EMB = float(np.float32(1.0) / (np.float32(1.0) - np.float32(P_EMB)))
S_IN = float(np.float32(1.0) / (np.float32(1.0) - np.float32(P_IN)))


@pytest.fixture(scope="module")
def dev():
    return cuda_dev()


@pytest.fixture(scope="module")
def api():
    return gcn_api()


def _batch(api, dev, seed, B, T, E, vocab=V0, lengths="tacred"):
    """ids as the loader pads them (0 past each sentence's end), tables whose only zero row is the word table's padding row, and the
    batch's PackedTrees."""
    _, tree = api
    tb = synthetic.random_tree_batch(seed, B, T, lengths)
    rng = np.random.RandomState(seed + 1)
    words = rng.randint(2, vocab, size=(B, T)).astype(np.int64)
    pos = rng.randint(0, V1, size=(B, T)).astype(np.int64)
    ner = rng.randint(0, V2, size=(B, T)).astype(np.int64)
    for a in (words, pos, ner):
        a[tb["masks"]] = 0
    W0 = synthetic.normal(seed + 2, (V0, E[0]))
    W0[0] = 0.0
    W1 = synthetic.normal(seed + 3, (V1, E[1])) if E[1] else None
    W2 = synthetic.normal(seed + 4, (V2, E[2])) if E[2] else None
    d = lambda a: None if a is None else to_dev(a, dev)  # noqa: E731
    packed = prune(tree, tb, 1, dev).pack([int(n) for n in tb["lens"]])
    return dict(words=d(words), pos=d(pos), ner=d(ner), W0=d(W0), W1=d(W1), W2=d(W2), packed=packed, tb=tb, E=E)


def _cat(words, pos, ner, W0, W1, W2):
    """The torch path: model/gcn.py:235-239 without dropout.  A float `words` is the dense word source."""
    parts = [words if words.dim() > 2 else F.embedding(words, W0, padding_idx=0)]
    if W1 is not None:
        parts.append(F.embedding(pos, W1))
    if W2 is not None:
        parts.append(F.embedding(ner, W2))
    return torch.cat(parts, 2)


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and bool((_bits(a) == _bits(b)).all())


def _run(api, c, words=None, **kw):
    gcn, _ = api
    return gcn.embed_inputs(c["words"] if words is None else words, c["pos"], c["ner"], c["W0"], c["W1"], c["W2"], **kw)


SHAPES = {"c2": (50, 100, (300, 30, 30)), "odd_7_3_0": (5, 17, (7, 3, 0)), "odd_33_5_1": (6, 23, (33, 5, 1)), "t300": (4, 300, (300, 30, 30)),
          "semeval_no_ner": (50, 100, (300, 30, 0))}


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_forward_without_dropout_is_the_cat_bit_for_bit(api, dev, shape):
    B, T, E = SHAPES[shape]
    c = _batch(api, dev, 11, B, T, E)
    y0 = _cat(c["words"], c["pos"], c["ner"], c["W0"], c["W1"], c["W2"])
    out = _run(api, c)
    assert out.shape == (B, T, sum(E)) and _same_bits(out, y0)
    assert _same_bits(_run(api, c, out_dtype=torch.bfloat16), y0.to(torch.bfloat16))
    trees = c["packed"]
    pk = _run(api, c, trees=trees)
    N = int(c["tb"]["lens"].sum())
    assert pk.shape == (trees.N, sum(E)) and _same_bits(pk[:N], trees.pack_rows(y0)[:N])
    assert _same_bits(_run(api, c, trees=trees, out_dtype=torch.bfloat16)[:N], trees.pack_rows(y0.to(torch.bfloat16))[:N])
    # the dense word source (float `words`, gcn.py:235-236): same rows without the lookup
    dense = F.embedding(c["words"], c["W0"])
    assert _same_bits(_run(api, c, words=dense), y0)
    assert _same_bits(_run(api, c, words=dense, trees=trees, out_dtype=torch.bfloat16)[:N], trees.pack_rows(y0.to(torch.bfloat16))[:N])
    # pure gather whatever the seeds are
    assert _same_bits(_run(api, c, seeds=(5, 6), seed_dev=torch.full((1,), 9, dtype=torch.int64, device=dev)), y0)


def test_forward_dropout_values_layouts_and_fractions(api, dev):
    """Observed on the MI355X with SEEDS on the C2 shape: element dropout keeps 0.49926 of the 300 000 POS / NER elements (p = 0.5, 5 sigma =
    0.0046), word-type dropout keeps 0.71193 of the 1 576 (sentence, word) types (p = 0.3, 5 sigma = 0.0577)."""
    B, T, E = SHAPES["c2"]
    c = _batch(api, dev, 12, B, T, E)
    E0 = E[0]
    y0 = _cat(c["words"], c["pos"], c["ner"], c["W0"], c["W1"], c["W2"])
    kw = dict(p_emb=P_EMB, p_in=P_IN, seeds=SEEDS)
    out = _run(api, c, **kw)
    want = torch.cat([(y0[..., :E0] * S_EMB) * S_IN, y0[..., E0:] * S_IN], 2)
    ob = _bits(out)
    assert bool(((ob == 0) | (ob == _bits(want))).all())             # +0.0 or exactly (y0 * s_emb) * s_in
    assert _same_bits(_run(api, c, **kw), out)                        # same seeds, same mask
    other = _run(api, c, p_emb=P_EMB, p_in=P_IN, seeds=(SEEDS[0] + 1, SEEDS[1] + 1))
    assert not _same_bits(other, out) and bool(((_bits(other) == 0) | (_bits(other) == _bits(want))).all())
    shifted = _run(api, c, seed_dev=torch.full((1,), 3, dtype=torch.int64, device=dev), p_emb=P_EMB, p_in=P_IN, seeds=(SEEDS[0] - 3, SEEDS[1] - 3))
    assert _same_bits(shifted, out)                                   # the device word is added to both seeds
    trees = c["packed"]
    N = int(c["tb"]["lens"].sum())
    assert _same_bits(_run(api, c, trees=trees, **kw)[:N], trees.pack_rows(out)[:N])
    b16 = _run(api, c, out_dtype=torch.bfloat16, **kw)
    assert _same_bits(b16, out.to(torch.bfloat16))
    assert _same_bits(_run(api, c, trees=trees, out_dtype=torch.bfloat16, **kw)[:N], trees.pack_rows(b16)[:N])
    # word-type dropout alone: POS / NER untouched, the word segment of a token entirely kept or entirely dropped
    we = _run(api, c, p_emb=P_EMB, seeds=SEEDS)
    assert _same_bits(we[..., E0:], y0[..., E0:])
    wb, tb = _bits(we[..., :E0]), _bits(y0[..., :E0] * S_EMB)
    tok_kept, tok_dropped = (wb == tb).all(-1), (wb == 0).all(-1)
    real = c["words"] != 0
    assert bool((tok_kept | tok_dropped)[real].all())
    # ... and it is the word-type decision of the combined run
    type_kept_combined = (out[..., :E0] != 0).any(-1)
    assert bool((type_kept_combined == tok_kept)[real].all())
    # the dense word source ignores p_emb
    dn = _run(api, c, words=F.embedding(c["words"], c["W0"]), p_emb=P_EMB, seeds=SEEDS)
    assert _same_bits(dn, y0)
    # kept fractions, 5 binomial standard deviations
    el = _run(api, c, p_in=P_IN, seeds=SEEDS)
    n_el = (y0[..., E0:] != 0).sum().item()
    f_el = (el[..., E0:] != 0).sum().item() / n_el
    keys = (torch.arange(B, device=dev).unsqueeze(1) * V0 + c["words"])[real]
    uniq, first = np.unique(keys.cpu().numpy(), return_index=True)
    f_ty = float(tok_kept[real].cpu().numpy()[first].mean())
    print("element dropout keeps %.5f of %d, word-type dropout keeps %.5f of %d types" % (f_el, n_el, f_ty, len(uniq)))
    assert abs(f_el - (1 - P_IN)) <= 5 * np.sqrt(P_IN * (1 - P_IN) / n_el)
    assert abs(f_ty - (1 - P_EMB)) <= 5 * np.sqrt(P_EMB * (1 - P_EMB) / len(uniq))


def test_word_type_dropout_is_shared_by_all_occurrences_in_a_sentence(api, dev):
    B, T, E = 50, 100, (300, 30, 30)
    c = _batch(api, dev, 13, B, T, E, vocab=22, lengths="full")     # 100 tokens drawn from 20 word ids: every word repeats
    out = _run(api, c, p_emb=P_EMB, p_in=P_IN, seeds=SEEDS)
    kept = (out[..., :E[0]] != 0).any(-1).cpu().numpy()
    words = c["words"].cpu().numpy()
    table = np.full((B, 22), -1)
    repeated = 0
    for b in range(B):
        for i in np.unique(words[b]):
            flags = kept[b][words[b] == i]
            assert (flags == flags[0]).all(), (b, i)
            repeated += len(flags) > 1
            table[b, i] = flags[0]
    assert repeated > 900                                             # of 50 x 20 (sentence, word) pairs
    live = table[:, 2:]
    assert (live == 0).any() and (live == 1).any()
    assert ((live == 0).any(0) & (live == 1).any(0)).any()            # the decision is per sentence: a word kept here, dropped there


def _grad_case(api, dev, c, layout, g_dtype, sparse=False, topn=None, dense=False, bump_seed=False):
    """Gradients of embed_inputs against torch autograd of cat(...) * M * scales with the mask M recovered from the forward."""
    gcn, _ = api
    B, T = c["words"].shape
    E0 = c["E"][0]
    trees = c["packed"] if layout == "packed" else None
    N = int(c["tb"]["lens"].sum())
    leaves = [None if w is None else w.clone().requires_grad_() for w in (c["W0"], c["W1"], c["W2"])]
    src = to_dev(synthetic.normal(97, (B, T, E0)), dev).requires_grad_() if dense else None      # (no zeros: M is read off the output)
    seed_dev = torch.full((1,), 5, dtype=torch.int64, device=dev) if bump_seed else None
    kw = dict(p_emb=P_EMB, p_in=P_IN, seeds=SEEDS, seed_dev=seed_dev, out_dtype=g_dtype, sparse=sparse, topn=topn)
    emb = torch.nn.Embedding(V0, E0, padding_idx=0).to(dev)
    emb.weight = torch.nn.Parameter(leaves[0])
    out = gcn.embed_inputs(src if dense else c["words"], c["pos"], c["ner"], None if dense else emb, leaves[1], leaves[2], trees=trees, **kw)
    g = to_dev(synthetic.normal(99, tuple(out.shape)), dev).to(g_dtype)
    if trees is not None:
        g[N:] = 0
    if bump_seed:
        seed_dev.add_(7)                                              # the backward still sees the forward's word
    out.backward(g)
    got = [emb.weight.grad if not dense else src.grad, None if leaves[1] is None else leaves[1].grad, None if leaves[2] is None else leaves[2].grad]
    # reference
    padded = gcn.embed_inputs(src.detach() if dense else c["words"], c["pos"], c["ner"], None if dense else c["W0"], c["W1"], c["W2"],
                              p_emb=P_EMB, p_in=P_IN, seeds=SEEDS, seed_dev=torch.full((1,), 5, dtype=torch.int64, device=dev) if bump_seed else None)
    M = (padded != 0).float()
    scales = torch.full((padded.shape[-1],), S_IN, device=dev)
    if not dense:
        scales[:E0] = S_EMB * S_IN
    ref_leaves = [None if w is None else w.clone().requires_grad_() for w in (c["W0"], c["W1"], c["W2"])]
    ref_src = src.detach().clone().requires_grad_() if dense else None
    if dense:
        word_part = ref_src
    elif sparse:
        word_part = gcn._EmbedFn.apply(ref_leaves[0], c["words"], 0, True, topn)
    else:
        word_part = F.embedding(c["words"], ref_leaves[0], padding_idx=0)
    parts = [word_part] + [F.embedding(i, w) for i, w in ((c["pos"], ref_leaves[1]), (c["ner"], ref_leaves[2])) if w is not None]
    ref = torch.cat(parts, 2) * (M * scales)
    if trees is not None:
        ref = trees.pack_rows(ref)
    ref.backward(g.float())
    want = [ref_src.grad if dense else ref_leaves[0].grad, None if ref_leaves[1] is None else ref_leaves[1].grad,
            None if ref_leaves[2] is None else ref_leaves[2].grad]
    if topn is not None and not sparse and not dense:
        want[0] = want[0].clone()
        want[0][topn:] = 0
    return got, want


@pytest.mark.parametrize("layout,g_dtype", [("padded", torch.float32), ("padded", torch.bfloat16), ("packed", torch.float32),
                                            ("packed", torch.bfloat16)])
@pytest.mark.parametrize("shape", ["c2", "odd_33_5_1", "semeval_no_ner"])
def test_backward_matches_autograd_of_the_masked_cat(api, dev, shape, layout, g_dtype):
    B, T, E = SHAPES[shape]
    c = _batch(api, dev, 14, B, T, E)
    for case in (dict(), dict(topn=400), dict(dense=True), dict(bump_seed=True)):
        got, want = _grad_case(api, dev, c, layout, g_dtype, **case)
        for k, (a, b) in enumerate(zip(got, want)):
            assert (a is None) == (b is None), (case, k)
            if a is not None:
                err = max_rel(a.cpu().numpy(), b.cpu().numpy())
                print(shape, layout, g_dtype, case, "table %d" % k, "%.2e" % err)
                assert err <= GRAD_RTOL, (case, k, err)
        if not case.get("dense"):
            assert bool((got[0][0] == 0).all())                      # padding_idx row
            if case.get("topn"):
                assert bool((got[0][400:] == 0).all())


@pytest.mark.parametrize("layout", ["padded", "packed"])
@pytest.mark.parametrize("topn", [None, 400])
@pytest.mark.parametrize("g_dtype", [torch.float32, torch.bfloat16], ids=["g_fp32", "g_bf16"])
def test_backward_sparse_form_equals_embedfn_sparse(api, dev, layout, topn, g_dtype):
    B, T, E = SHAPES["c2"]
    c = _batch(api, dev, 15, B, T, E)
    got, want = _grad_case(api, dev, c, layout, g_dtype, sparse=True, topn=topn)
    a, b = got[0], want[0]
    assert a.is_sparse and b.is_sparse and tuple(a.shape) == tuple(b.shape)
    assert torch.equal(a._indices(), b._indices())
    assert max_rel(a._values().cpu().numpy(), b._values().cpu().numpy()) <= GRAD_RTOL
    flat = c["words"].reshape(-1)
    dead = (flat == 0) | (flat >= (topn or V0))
    assert bool((a._values()[dead] == 0).all())
    for k in (1, 2):
        assert max_rel(got[k].cpu().numpy(), want[k].cpu().numpy()) <= GRAD_RTOL


def test_ids_outside_their_table(api, dev):
    gcn, _ = api
    B, T, E = 6, 23, (33, 6, 4)
    c = _batch(api, dev, 16, B, T, E, lengths="full")
    E0 = E[0]
    words = c["words"].clone()
    words[1, 3], words[2, 4] = V0 + 5, -1
    status = torch.full((1,), 77, dtype=torch.int32, device=dev)
    leaves = [w.clone().requires_grad_() for w in (c["W0"], c["W1"], c["W2"])]
    out = gcn.embed_inputs(words, c["pos"], c["ner"], leaves[0], leaves[1], leaves[2], status=status)
    assert int(status.item()) == 1                                    # bit 0: the word table
    safe = words.clone()
    safe[1, 3], safe[2, 4] = 0, 0                                     # the zero padding row stands in for "nothing read"
    ref_leaves = [w.clone().requires_grad_() for w in (c["W0"], c["W1"], c["W2"])]
    ref = _cat(safe, c["pos"], c["ner"], *ref_leaves)
    assert _same_bits(out.detach(), ref.detach())                     # zero word segments there, every other element unchanged
    assert bool((out[1, 3, :E0] == 0).all() and (out[2, 4, :E0] == 0).all())
    g = to_dev(synthetic.normal(98, tuple(out.shape)), dev)
    out.backward(g)
    ref.backward(g)
    for a, b in zip(leaves, ref_leaves):
        assert torch.isfinite(a.grad).all() and max_rel(a.grad.cpu().numpy(), b.grad.cpu().numpy()) <= GRAD_RTOL
    # the row-sparse form holds zero rows for them; a clean batch leaves the status word clear; POS / NER raise their own bits
    lw = c["W0"].clone().requires_grad_()
    gcn.embed_inputs(words, c["pos"], c["ner"], lw, c["W1"], c["W2"], sparse=True).backward(g)
    vals = lw.grad._values().view(B, T, E0)
    assert bool((vals[1, 3] == 0).all() and (vals[2, 4] == 0).all()) and float(vals.abs().sum()) > 0
    gcn.embed_inputs(c["words"], c["pos"], c["ner"], c["W0"], c["W1"], c["W2"], status=status)
    assert int(status.item()) == 0
    pos, ner = c["pos"].clone(), c["ner"].clone()
    pos[0, 0], ner[5, 22] = V1, -2
    leaves = [w.clone().requires_grad_() for w in (c["W0"], c["W1"], c["W2"])]
    out = gcn.embed_inputs(c["words"], pos, ner, leaves[0], leaves[1], leaves[2], status=status, trees=None)
    assert int(status.item()) == 6
    assert bool((out[0, 0, E0:E0 + E[1]] == 0).all() and (out[5, 22, E0 + E[1]:] == 0).all())
    # ... and their backward: the clean ids' gradients with those two tokens' POS / NER contributions removed
    out.backward(g)
    hole = torch.ones_like(g)
    hole[0, 0, E0:E0 + E[1]] = 0
    hole[5, 22, E0 + E[1]:] = 0
    ref_leaves = [w.clone().requires_grad_() for w in (c["W0"], c["W1"], c["W2"])]
    (_cat(c["words"], c["pos"], c["ner"], *ref_leaves) * hole).backward(g)
    for a, b in zip(leaves, ref_leaves):
        assert torch.isfinite(a.grad).all() and max_rel(a.grad.cpu().numpy(), b.grad.cpu().numpy()) <= GRAD_RTOL


def _model(gcn, g, dev, sd=None, **kw):
    opt = dict(json.loads(str(g["opt"])), cuda=True, **kw)
    m = gcn.GCNClassifier(opt)
    m.load_state_dict(sd if sd is not None else {k[3:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("sd:")}, strict=True)
    return m.to(dev)


def _inputs(g, dev, opt):
    keys = ("words", "masks", "pos", "ner", "deprel", "head", "subj_pos", "obj_pos")
    if opt["dataset"] != "tacred":
        keys = keys[:3] + keys[4:]
    return tuple(to_dev(g[k], dev) for k in keys)


@pytest.mark.parametrize("kw", [dict(), dict(gcn_packed=True), dict(gcn_pooled_only=True)], ids=["padded", "packed", "pooled_only"])
def test_module_eval_equals_the_torch_front_end_bit_for_bit(api, dev, kw):
    gcn, _ = api
    g = load_golden("e2e_gcn.npz")
    inputs = _inputs(g, dev, json.loads(str(g["opt"])))
    with torch.no_grad():
        want, wp = _model(gcn, g, dev, **kw).eval()(inputs)
        got, gp = _model(gcn, g, dev, gcn_native_embed=True, **kw).eval()(inputs)
    assert _same_bits(got, want) and _same_bits(gp, wp)


@pytest.mark.parametrize("tag", ["gcn", "semeval", "cgcn", "diag", "full"])
def test_module_reproduces_the_golden_logits(api, dev, tag):
    gcn, tree = api
    g = load_golden("e2e_%s.npz" % tag)
    opt = json.loads(str(g["opt"]))
    inputs = _inputs(g, dev, opt)
    with torch.no_grad():
        logits, pooled = _model(gcn, g, dev, gcn_native_embed=True).eval()(inputs)
        assert max_rel(logits.cpu().numpy(), g["logits"]) <= 1e-4
        assert max_rel(pooled.cpu().numpy(), g["pooling_output"]) <= 1e-4
        m16 = _model(gcn, g, dev, gcn_native_embed=True, gcn_dtype="bf16").eval()
        l16, _ = m16(inputs)
        assert max_rel(l16.cpu().numpy(), g["logits"]) <= 3e-2
        if tag in ("gcn", "semeval"):
            # the bf16 module hands the stack bf16 rows directly: gcn_layers on the torch-path embeddings .to(bfloat16), bit for bit
            rel, net = m16.gcn_model, m16.gcn_model.gcn
            head, subj, obj, deprel, masks = inputs[-3], inputs[-2], inputs[-1], inputs[-4], inputs[1]
            trees = tree.prune_to_csr(head, subj, obj, deprel, opt["prune_k"], masks=masks)
            x = _cat(inputs[0], inputs[2], inputs[3] if opt["dataset"] == "tacred" else None, rel.emb.weight, rel.pos_emb.weight,
                     rel.ner_emb.weight if opt["dataset"] == "tacred" else None).to(torch.bfloat16)
            want = gcn.gcn_layers(x, [lin.weight for lin in net.W], [lin.bias for lin in net.W], trees, compute_dtype=torch.bfloat16,
                                  out_dtype=torch.float32)
            h, _ = net(trees, inputs)
            assert _same_bits(h, want)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_module_bert_no_rnn_golden(api, dev, dtype):
    from test_gpu_wide_layers import _golden_batch
    gcn, _ = api
    g = load_golden("e2e_bert_norrn.npz")
    _, batch, sd = _golden_batch(g)
    inputs = tuple(to_dev(a, dev) for a in batch)
    m = _model(gcn, g, dev, sd={k: torch.from_numpy(v) for k, v in sd.items()}, gcn_native_embed=True, gcn_dtype=dtype).eval()
    with torch.no_grad():
        logits, pooled = m(inputs)
    assert max_rel(logits.cpu().numpy(), g["logits"]) <= (1e-4 if dtype == "fp32" else 3e-2)
    if dtype == "fp32":
        assert max_rel(pooled.cpu().numpy(), g["pooling_output"]) <= 1e-4


@pytest.mark.parametrize("variant", ["gcn", "gcn_packed", "gcn_pooled_only", "gcn_sparse", "cgcn", "cgcn_native_rnn", "semeval", "diag"])
def test_module_training_step_same_gradients(api, dev, variant):
    gcn, _ = api
    tag = variant.split("_")[0]
    g = load_golden("e2e_%s.npz" % tag)
    kw = dict(input_dropout=0.0, emb_dropout=0.0, word_dropout=0.0, gcn_dropout=0.0, rnn_dropout=0.0)
    kw.update({"gcn_packed": dict(gcn_packed=True), "gcn_pooled_only": dict(gcn_pooled_only=True), "gcn_sparse": dict(gcn_sparse_emb_grad=True),
               "cgcn_native_rnn": dict(gcn_native_rnn=True)}.get(variant, {}))
    inputs = _inputs(g, dev, json.loads(str(g["opt"])))
    grads = []
    for native in (False, True):
        m = _model(gcn, g, dev, gcn_native_embed=native, **kw).train()
        logits, pooled = m(inputs)
        labels = torch.arange(logits.shape[0], device=dev) % logits.shape[1]
        (F.cross_entropy(logits, labels) + 0.003 * (pooled ** 2).sum(1).mean()).backward()
        grads.append({n: p.grad for n, p in m.named_parameters()})
    assert grads[0].keys() == grads[1].keys()
    seen = 0
    for n in grads[0]:
        a, b = grads[1][n], grads[0][n]
        assert (a is None) == (b is None), n
        if a is None:
            continue
        if a.is_sparse:
            a, b = a.to_dense(), b.to_dense()
        seen += 1
        assert max_rel(a.cpu().numpy(), b.cpu().numpy()) <= GRAD_RTOL, n
    assert seen >= 8 and grads[1]["gcn_model.emb.weight"] is not None


def test_module_raises_on_bad_ids_only_when_checking(api, dev):
    gcn, _ = api
    g = load_golden("e2e_gcn.npz")
    inputs = list(_inputs(g, dev, json.loads(str(g["opt"]))))
    inputs[0] = inputs[0].clone()
    inputs[0][0, 0] = 10 ** 6
    with torch.no_grad():
        with pytest.raises(IndexError, match="words"):
            _model(gcn, g, dev, gcn_native_embed=True).eval()(tuple(inputs))
        logits, _ = _model(gcn, g, dev, gcn_native_embed=True, gcn_check_trees=False).eval()(tuple(inputs))
    assert torch.isfinite(logits).all()


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_training_step_graph_capture_with_native_front_end(api, dev, dtype):
    """The whole training step with the native front end as ONE hipGraph: the input masks advance from the device counter on every
    replay, and the backward recomputes the forward's masks although the counter moves on between the two."""
    gcn, _ = api
    e = load_golden("e2e_gcn.npz")
    model = _model(gcn, e, dev, gcn_dtype=dtype, gcn_graph_rng=True, gcn_check_trees=False, gcn_native_embed=True, input_dropout=0.5,
                   emb_dropout=0.3, word_dropout=0.0, gcn_dropout=0.0).train()
    inputs = _inputs(e, dev, json.loads(str(e["opt"])))
    labels = torch.arange(inputs[0].shape[0], device=dev) % 42

    def step():
        model.zero_grad(set_to_none=True)
        logits, pooled = model(inputs)
        loss = F.cross_entropy(logits, labels) + 0.003 * (pooled ** 2).sum(1).mean()
        loss.backward()
        return loss

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            step()
    torch.cuda.current_stream().wait_stream(side)
    counter = model.gcn_model.gcn._rng_step
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        loss = step()
    E = model.gcn_model.emb.weight
    counter.fill_(100)
    graph.replay()
    l1, g1 = float(loss), E.grad.clone()
    graph.replay()
    l2 = float(loss)
    assert int(counter) == 102 and l1 != l2                          # identical inputs, another input mask
    counter.fill_(100)
    graph.replay()
    assert float(loss) == l1
    assert torch.isfinite(E.grad).all() and max_rel(E.grad.cpu().numpy(), g1.cpu().numpy()) <= 1e-5
    counter.fill_(100)
    le = step()                                                       # the replayed step is the eager step
    assert abs(float(le) - l1) <= 1e-6 * abs(l1)
    assert max_rel(E.grad.cpu().numpy(), g1.cpu().numpy()) <= 1e-5
