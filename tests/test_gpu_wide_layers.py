"""The wide form of the layer forward (csrc/wide_kernels.hip) on the MI355X: GCN layers whose input is too wide for the row-tile
kernel's LDS -- the no-RNN model on BERT-large vectors (1024 + POS + NER = 1084 columns, reference train.py:105,143-144 and
model/gcn.py:136,235-236) -- against the float64 oracle, against the row-tile form where both run, through the module and in a
captured training step.  Every test here fails on the code without the wide form (the layers are refused for their LDS, or the
option does not exist)."""
import ctypes

import numpy as np
import pytest
import torch

from helpers import FWD_RTOL, GRAD_RTOL, cuda_dev, gcn_api, max_rel, options, prune, to_dev

pytestmark = pytest.mark.gpu

BF16_GRAD = 2e-2


@pytest.fixture(scope="module")
def dev():
    return cuda_dev()


@pytest.fixture(scope="module")
def api():
    return gcn_api()


# (B, T, Din, H, K): BERT-large + POS + NER; a 300-wide hidden layer; K = 0 trees; 4096 columns; a second output-column slice
# pass of the row tile's width (520); an odd width (element loads) with a row count that is not a multiple of 32
SHAPES = [(4, 40, 1084, 200, 1), (3, 57, 1324, 300, 2), (2, 50, 2048, 200, 0), (5, 17, 4096, 40, 1), (1, 200, 1100, 520, 2),
          (3, 41, 1085, 200, 1)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("layout", ["padded", "packed"])
@pytest.mark.parametrize("compute", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_wide_layers_vs_oracle(api, dev, shape, layout, compute):
    """A two-layer stack Din -> H -> H whose first layer takes the wide form (in fp32 at every shape; in bf16 where even bf16 does
    not fit), forward and gradients (dx, dW, db) against oracle/gcn_ref.py.  The gradients are the oracle's differentiated through the
    device's own activations (relu' is a step function), as the full-size tests of test_gpu_parity.py take them."""
    from oracle import gcn_ref, prune_ref
    from gcn_over_pruned_trees_amd.utils import synthetic
    gcn, tree = api
    B, T, din, hid, K = shape
    tb = synthetic.random_tree_batch(400 + B + T, B, T, "tacred")
    adj = prune_ref.batch_adj(tb["head"], tb["subj_pos"], tb["obj_pos"], tb["deprel"], tb["lens"], K)["adj"]
    Wn, bn = synthetic.layer_params(11, [din, hid, hid])
    xn, gyn = synthetic.normal(12, (B, T, din)), synthetic.normal(13, (B, T, hid))
    trees = prune(tree, tb, K, dev)
    x0, g0 = to_dev(xn, dev), to_dev(gyn, dev)
    keep = ~to_dev(np.arange(T)[None, :] >= tb["lens"][:, None], dev)
    if layout == "packed":
        trees = trees.pack(tb["lens"].tolist())
        x0, g0 = x0[keep].contiguous(), g0[keep].contiguous()
    x = x0.clone().requires_grad_()
    Ws = [to_dev(w, dev).requires_grad_() for w in Wn]
    bs = [to_dev(b, dev).requires_grad_() for b in bn]
    h, acts = gcn.gcn_layers_with_acts(x, Ws, bs, trees, compute_dtype=compute)
    h.backward(g0)
    torch.cuda.synchronize()

    def padded(a):                      # device rows in the oracle's [B, T, *] layout (packed: zero rows past a sentence's end)
        a = a.detach().float()
        if layout == "packed":
            full = torch.zeros((B, T) + tuple(a.shape[1:]), dtype=a.dtype, device=a.device)
            full[keep] = a
            a = full
        return a.cpu().numpy()

    href, _ = gcn_ref.gcn_forward(adj, xn, Wn, bn)
    real = np.arange(T)[None, :] < tb["lens"][:, None]
    outs = [padded(a) for a in acts]
    if layout == "packed":              # padding rows: the oracle's relu(W pad-row + 2b) is not produced (every consumer masks it)
        _, _, (_, _, saved) = gcn_ref.gcn_forward(adj, xn, Wn, bn, return_saved=True)
        for l in range(2):
            outs[l][~real] = saved[l][2][~real]
    assert max_rel(padded(h)[real], href[real]) <= (FWD_RTOL if compute == torch.float32 else 3e-2)
    gy_full = gyn if layout == "padded" else np.where(real[..., None], gyn, 0.0).astype(np.float32)
    dx, dWs, dbs = gcn_ref.gcn_backward(adj, xn, Wn, bn, gy_full, acts=outs)
    tol = GRAD_RTOL if compute == torch.float32 else BF16_GRAD
    assert max_rel(padded(x.grad)[real], dx[real]) <= tol
    for l in range(2):
        assert max_rel(Ws[l].grad.cpu().numpy(), dWs[l]) <= tol and max_rel(bs[l].grad.cpu().numpy(), dbs[l]) <= tol


def _stack_fwd(lib, L, x, Wf, b32, trees, dims, compute, drop, seeds, seed_dev, out_dtype):
    """gcnpt_layers_fwd with an S image for every layer: the outputs and the images."""
    dev = x.device
    rows, T = (trees.N, 0) if getattr(trees, "packed", False) else (x.shape[0] * x.shape[1], x.shape[1])
    B = rows if T == 0 else x.shape[0]
    lead = tuple(x.shape[:-1])
    mid = torch.float32 if compute == lib.F32 else torch.bfloat16
    outs = [torch.empty(lead + (H,), dtype=out_dtype if l == L - 1 else mid, device=dev) for l, (H, _) in enumerate(dims)]
    sf = [torch.zeros((lib.lib().gcnpt_frag_bytes(rows, K, compute),), dtype=torch.uint8, device=dev) for _, K in dims]
    ints = lambda v: (ctypes.c_int * L)(*v)  # noqa: E731
    lib.check(lib.lib().gcnpt_layers_fwd(
        lib.stream(), L, lib.ptr(x), lib.dtype_code(x.dtype), lib.ptr_array(Wf), lib.ptr_array(b32), lib.ptr(trees.row_ptr),
        lib.ptr(trees.col_idx), lib.ptr(trees.ell), lib.ptr(trees.ell), B, T, ints([k for _, k in dims]), ints([h for h, _ in dims]),
        lib.ptr_array(outs), ints([lib.dtype_code(o.dtype) for o in outs]), compute, (ctypes.c_float * L)(*drop),
        (ctypes.c_uint64 * L)(*seeds), lib.ptr_array(sf), lib.ptr(seed_dev)))
    torch.cuda.synchronize()
    return outs, sf


@pytest.mark.parametrize("case", [(50, 100, 360, "tacred"), (50, 100, 416, "tacred"), (300, 100, 360, "tacred")],
                         ids=["c2", "13_ksteps", "4_waves"])
@pytest.mark.parametrize("layout", ["padded", "packed"])
@pytest.mark.parametrize("compute", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_forced_wide_form_matches_row_tile(api, dev, case, layout, compute):
    """GCNPT_OPT_WIDE_FORM = 1 sends every forward launch through the wide form.  At shapes the row tile also runs (C2: 360 -> 200
    -> 200; 416 = 13 bf16 k-steps; B = 300, where the row tile takes its 4-wave form) with dropout 0.3 on layer 0 and a device seed
    counter: every layer's output and S fragment image are bit-identical to the row tile's; through the module op the input gradient
    is too, and the weight gradients agree to the float-atomic bound of the other form tests."""
    from gcn_over_pruned_trees_amd import _lib
    from gcn_over_pruned_trees_amd.model.gcn import WeightPack
    from gcn_over_pruned_trees_amd.utils import synthetic
    gcn, tree = api
    B, T, din, lengths = case
    hid, K = 200, 1
    tb = synthetic.random_tree_batch(77 + B, B, T, lengths)
    trees = prune(tree, tb, K, dev)
    Wn, bn = synthetic.layer_params(78, [din, hid, hid])
    xn, gyn = synthetic.normal(79, (B, T, din)), synthetic.normal(80, (B, T, hid))
    x0, g0 = to_dev(xn, dev), to_dev(gyn, dev)
    if layout == "packed":
        keep = ~to_dev(tb["masks"], dev)
        trees = trees.pack(tb["lens"].tolist())
        x0, g0 = x0[keep].contiguous(), g0[keep].contiguous()
    if compute == torch.bfloat16:
        x0 = x0.to(torch.bfloat16)
    cd = _lib.dtype_code(compute)
    Wt = [to_dev(w, dev) for w in Wn]
    bt = [to_dev(b, dev) for b in bn]
    pk = WeightPack(Wt, cd, dev)
    _lib.check(_lib.lib().gcnpt_pack_weights_multi(_lib.stream(), *pk.c_args()))
    seed_dev = torch.tensor([12345], dtype=torch.int64, device=dev)
    dims = [(hid, din), (hid, hid)]
    res, grads = [], []
    for form in (0, 1):
        with options(WIDE_FORM=form):
            res.append(_stack_fwd(_lib, 2, x0, pk.wf, bt, trees, dims, cd, [0.3, 0.0], [5, 0], seed_dev, torch.float32))
            x = x0.clone().float().requires_grad_() if compute == torch.float32 else x0.clone().requires_grad_()
            Ws = [w.clone().requires_grad_() for w in Wt]
            bs = [b.clone().requires_grad_() for b in bt]
            h = gcn.gcn_layers(x, Ws, bs, trees, [0.3, 0.0], [5, 0], compute_dtype=compute, seed_dev=seed_dev)
            h.backward(g0)
            torch.cuda.synchronize()
            grads.append((h.detach(), x.grad, [w.grad for w in Ws], [b.grad for b in bs]))
    (oa, sa), (ob, sb) = res
    assert float(oa[-1].abs().max()) > 0 and (oa[0] == 0).float().mean() > 0.3          # the dropout mask is there
    for l in range(2):
        assert torch.equal(oa[l], ob[l]), "layer %d output" % l
        assert torch.equal(sa[l], sb[l]), "layer %d S image" % l
    a, b = grads
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    for l in range(2):
        assert max_rel(b[2][l].cpu().numpy(), a[2][l].cpu().numpy()) <= 1e-5
        assert max_rel(b[3][l].cpu().numpy(), a[3][l].cpu().numpy()) <= 1e-5


def test_option_zero_brings_the_refusal_back(api, dev):
    """GCNPT_OPT_WIDE_FORM = 0: a 1084-wide fp32 layer is refused for its LDS as before; the default takes it."""
    from gcn_over_pruned_trees_amd import _lib
    from gcn_over_pruned_trees_amd.utils import synthetic
    gcn, tree = api
    B, T = 2, 30
    tb = synthetic.random_tree_batch(5, B, T, "tacred")
    trees = prune(tree, tb, 1, dev)
    Wn, bn = synthetic.layer_params(6, [1084, 200])
    x = to_dev(synthetic.normal(7, (B, T, 1084)), dev)
    Ws, bs = [to_dev(w, dev) for w in Wn], [to_dev(b, dev) for b in bn]
    with options(WIDE_FORM=0):
        with pytest.raises(_lib.GcnptError) as e:
            gcn.gcn_layers(x, Ws, bs, trees)
        assert e.value.code == _lib.E_UNSUPPORTED and b"LDS" in str(e.value).encode()
    with torch.no_grad():
        h = gcn.gcn_layers(x, Ws, bs, trees)
    torch.cuda.synchronize()
    assert torch.isfinite(h).all() and float(h.abs().max()) > 0


def _bert_opt(**kw):
    opt = dict(vocab_size=100, emb_dim=1024, pos_dim=30, ner_dim=30, hidden_dim=200, num_layers=2, input_dropout=0.0, gcn_dropout=0.0,
               word_dropout=0.0, emb_dropout=0.0, topn=1e10, prune_k=1, pooling="max", pooling_l2=0.003, mlp_layers=2, no_adj=False,
               rnn=False, cuda=True, dataset="tacred", num_class=42, adj_type="regular", gcn_dtype="fp32")
    opt.update(kw)
    return opt


def _bert_inputs(dev, B, T, seed):
    from gcn_over_pruned_trees_amd.utils import synthetic
    tb = synthetic.random_tree_batch(seed, B, T, "tacred")
    rng = np.random.RandomState(seed)
    words = rng.standard_normal((B, T, 1024)).astype(np.float32)          # BERT-large vectors (data/bert_embeddings.py's output)
    words[tb["masks"]] = 0.0
    return (to_dev(words, dev), to_dev(tb["masks"], dev), to_dev(rng.randint(0, 47, size=(B, T)).astype(np.int64), dev),
            to_dev(rng.randint(0, 15, size=(B, T)).astype(np.int64), dev), to_dev(tb["deprel"], dev), to_dev(tb["head"], dev),
            to_dev(tb["subj_pos"], dev), to_dev(tb["obj_pos"], dev)), tb


def _golden_batch(g):
    """The fixture's batch and parameters, regenerated from its seeds exactly as tests/golden/make_golden_wide.py draws them, and
    checked against its checksums."""
    import json
    from gcn_over_pruned_trees_amd.utils import synthetic
    seed, B, T = int(g["seed"]), int(g["B"]), int(g["T"])
    tb = synthetic.random_tree_batch(seed, B, T, g["lens"])
    rng = np.random.RandomState(seed + 1)
    words = synthetic.normal(seed + 2, (B, T, 1024))
    words[tb["masks"]] = 0.0
    pos = rng.randint(2, 47, size=(B, T)).astype(np.int64)
    ner = rng.randint(2, 15, size=(B, T)).astype(np.int64)
    pos[tb["masks"]] = 0
    ner[tb["masks"]] = 0
    assert abs(float(words.astype(np.float64).sum()) - float(g["words_sum"])) < 1e-6
    assert int(pos.sum()) == int(g["pos_sum"]) and int(ner.sum()) == int(g["ner_sum"]) and int(tb["head"].sum()) == int(g["head_sum"])
    shapes = json.loads(str(g["shapes"]))
    sd = {}
    for i, k in enumerate(sorted(shapes)):
        shape = tuple(shapes[k])
        a = synthetic.normal(seed + 100 + i, shape)
        a = a / np.float32(np.sqrt(shape[-1])) if len(shape) > 1 else a * np.float32(0.1)
        if k.endswith("emb.weight"):
            a[0] = 0.0
        sd[k] = a.astype(np.float32)
        assert abs(float(sd[k].astype(np.float64).sum()) - float(g["sum:" + k])) < 1e-6, k
    return tb, (words, tb["masks"], pos, ner, tb["deprel"], tb["head"], tb["subj_pos"], tb["obj_pos"]), sd


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_bert_no_rnn_classifier_golden(api, dev, dtype):
    """GCNClassifier(rnn=False) on float word vectors [B, T, 1024] + POS + NER -- the first GCN layer reads 1084 columns, the wide
    form in fp32 -- against the reference's own GCNClassifier on the same batch and parameters (tests/golden/e2e_bert_norrn.npz, made by
    tests/golden/make_golden_wide.py): fp32 logits, pooled output and the gradients of the POS / NER tables and GCN.W[0] within 1e-4,
    bf16 logits within 3e-2.  gcn_packed and gcn_pooled_only give the padded path's logits; an eval() / no_grad forward gives the
    training forward's (every dropout is 0)."""
    import json
    from conftest import load_golden
    gcn, _ = api
    g = load_golden("e2e_bert_norrn.npz")
    _, batch, sd = _golden_batch(g)
    opt = dict(json.loads(str(g["opt"])), cuda=True, gcn_dtype=dtype)
    inputs = tuple(to_dev(a, dev) for a in batch)

    def build(**kw):
        m = gcn.GCNClassifier(dict(opt, **kw))
        m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)   # the reference's checkpoint layout
        return m.to(dev).train()

    model = build()
    logits, pooled = model(inputs)
    g_logits = to_dev(synthetic_normal(int(g["seed"]) + 3, tuple(logits.shape)), dev)
    g_pooled = to_dev(synthetic_normal(int(g["seed"]) + 4, tuple(pooled.shape)), dev)
    ((logits * g_logits).sum() + (pooled * g_pooled).sum()).backward()
    torch.cuda.synchronize()
    lg = logits.detach().cpu().numpy()
    if dtype == "bf16":
        assert max_rel(lg, g["logits"]) <= 3e-2
    else:
        assert max_rel(lg, g["logits"]) <= 1e-4
        assert max_rel(pooled.detach().cpu().numpy(), g["pooling_output"]) <= 1e-4
        rel = model.gcn_model
        assert max_rel(rel.pos_emb.weight.grad.cpu().numpy(), g["d_pos_emb"]) <= GRAD_RTOL
        assert max_rel(rel.ner_emb.weight.grad.cpu().numpy(), g["d_ner_emb"]) <= GRAD_RTOL
        dW0 = rel.gcn.W[0].weight.grad.cpu().numpy()
        proj = synthetic_normal(int(g["seed"]) + 5, (dW0.shape[1], 8))
        assert max_rel(dW0[:, ::8], g["dW0_cols8"]) <= GRAD_RTOL and max_rel(dW0[:, 1024:], g["dW0_posner"]) <= GRAD_RTOL
        assert max_rel(dW0.astype(np.float64) @ proj, g["dW0_proj"]) <= GRAD_RTOL
        assert max_rel(rel.gcn.W[0].bias.grad.cpu().numpy(), g["db0"]) <= GRAD_RTOL
    tol = 1e-5 if dtype == "fp32" else 3e-2
    with torch.no_grad():
        for kw in (dict(gcn_packed=True), dict(gcn_pooled_only=True)):
            lo, _ = build(**kw)(inputs)
            assert max_rel(lo.cpu().numpy(), lg) <= tol, kw
        model.eval()
        le, _ = model(inputs)
    assert max_rel(le.cpu().numpy(), lg) <= 1e-6


def synthetic_normal(seed, shape):
    from gcn_over_pruned_trees_amd.utils import synthetic
    return synthetic.normal(seed, shape)


def test_bert_no_rnn_training_step_capture(api, dev):
    """A whole BERT no-RNN training step (1084-wide first layer in fp32, layer dropout drawn from the device counter) captured with
    torch.cuda.graph replays to the eager step; trees from a TreeCache inside the step."""
    gcn, tree = api
    B, T = 20, 60
    inputs, _ = _bert_inputs(dev, B, T, 123)
    labels = to_dev(np.random.RandomState(4).randint(0, 42, size=(B,)).astype(np.int64), dev)
    torch.manual_seed(1234)
    model = gcn.GCNClassifier(_bert_opt(gcn_dropout=0.5, gcn_check_trees=False, gcn_graph_rng=True)).to(dev).train()
    cache = tree.TreeCache.build(inputs[5], inputs[6], inputs[7], inputs[4], 1, masks=inputs[1], want_label=False, compact=True)
    idx = torch.arange(B, device=dev)

    def step():
        model.zero_grad(set_to_none=True)
        logits, pooled = model(inputs, trees=cache.batch(idx, T))
        loss = torch.nn.functional.cross_entropy(logits, labels) + 0.003 * (pooled ** 2).sum(1).mean()
        loss.backward()
        return loss.detach()

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    counter = model.gcn_model.gcn._rng_step
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss = step()
    W0 = model.gcn_model.gcn.W[0].weight
    counter.fill_(7)
    graph.replay()
    torch.cuda.synchronize()
    l1, g1 = float(loss), W0.grad.clone()
    graph.replay()
    torch.cuda.synchronize()
    assert float(loss) != l1 and int(counter) == 9
    counter.fill_(7)
    le = float(step())                                   # eager, same counter value: same masks, same loss
    torch.cuda.synchronize()
    assert abs(le - l1) <= 1e-5 * abs(l1)
    assert torch.isfinite(g1).all() and float(g1.abs().max()) > 0
    assert max_rel(W0.grad.cpu().numpy(), g1.cpu().numpy()) <= 1e-4
