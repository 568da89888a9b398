"""The wide form of the layer backward-data (csrc/wide_kernels.hip, wide_bwd_kernel) on the MI355X: GCN layers whose hidden width H is
too wide for the row-tile backward's two H-wide tiles in LDS (fp32: H > 608, bf16: H > 1216) -- a GCN as wide as a BERT vector, hidden_dim
768 or 1024 -- against the float64 oracle, bit for bit against the row-tile form where both run, through the module against the reference's
own GCNClassifier, and in a captured training step.  Every test here fails on the code without the wide backward (the first backward at
these widths is refused for its LDS, or the option does not exist)."""
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


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. against the oracle
# (B, T, Din, H, K): hidden 640 (the first width past the fp32 row tile in steps of 16), BERT-base / -large hidden widths, an odd width
# (element loads, H not a multiple of 16)
FP32_SHAPES = [(4, 40, 360, 640, 1), (3, 45, 360, 768, 1), (2, 50, 1084, 1024, 2), (3, 41, 361, 650, 1)]
BF16_SHAPES = [(4, 40, 360, 1280, 1)]


def _oracle_case(api, dev, shape, layout, compute, drop=0.0, no_adj=False):
    from oracle import gcn_ref
    from gcn_over_pruned_trees_amd.utils import synthetic
    gcn, tree = api
    B, T, din, hid, K = shape
    tb = synthetic.random_tree_batch(500 + B + T + hid, B, T, "tacred")
    Wn, bn = synthetic.layer_params(21 + hid, [din, hid, hid])
    xn, gyn = synthetic.normal(22, (B, T, din)), synthetic.normal(23, (B, T, hid))
    trees = prune(tree, tb, K, dev)
    x0, g0 = to_dev(xn, dev), to_dev(gyn, dev)
    real = np.arange(T)[None, :] < tb["lens"][:, None]
    if layout == "compact":             # the kept tokens only: a [B, Tc] batch of its own, checked against the oracle on that batch
        ct = trees.compact()
        trees = ct.trees
        x0, g0 = ct.take(x0, fill=0.0).contiguous(), ct.take(g0, fill=0.0).contiguous()
        xn, gyn = x0.cpu().numpy(), g0.cpu().numpy()
        real = ct.valid.cpu().numpy()
    adj = trees.to_dense().cpu().numpy().astype(np.float32)
    keep = to_dev(real, dev)
    if layout == "packed":
        trees = trees.pack(tb["lens"].tolist())
        x0, g0 = x0[keep].contiguous(), g0[keep].contiguous()
    x = x0.clone().requires_grad_()
    Ws = [to_dev(w, dev).requires_grad_() for w in Wn]
    bs = [to_dev(b, dev).requires_grad_() for b in bn]
    h, acts = gcn.gcn_layers_with_acts(x, Ws, bs, trees, drop_p=[drop, 0.0], seeds=[9, 0], compute_dtype=compute, no_adj=no_adj)
    h.backward(g0)
    torch.cuda.synchronize()

    def padded(a):                      # device rows in the oracle's [B, T, *] layout (packed: zero rows past a sentence's end)
        a = a.detach().float()
        if layout == "packed":
            full = torch.zeros(real.shape + tuple(a.shape[1:]), dtype=a.dtype, device=a.device)
            full[keep] = a
            a = full
        return a.cpu().numpy()

    outs = [padded(a) for a in acts]
    masks = [outs[0] > 0] if drop > 0 else None
    if layout == "packed":              # padding rows: the oracle's relu(W pad-row + 2b) is not produced (every consumer masks it)
        _, _, (_, _, saved) = gcn_ref.gcn_forward(adj, xn, Wn, bn, no_adj=no_adj, return_saved=True)
        for l in range(2):
            outs[l][~real] = saved[l][2][~real]
    if drop == 0:
        href, _ = gcn_ref.gcn_forward(adj, xn, Wn, bn, no_adj=no_adj)
        assert max_rel(padded(h)[real], href[real]) <= (FWD_RTOL if compute == torch.float32 else 3e-2)
    gy_full = gyn if layout != "packed" else np.where(real[..., None], gyn, 0.0).astype(np.float32)
    dx, dWs, dbs = gcn_ref.gcn_backward(adj, xn, Wn, bn, gy_full, drop_masks=masks, drop_p=drop, no_adj=no_adj, acts=outs)
    tol = GRAD_RTOL if compute == torch.float32 else BF16_GRAD
    assert max_rel(padded(x.grad)[real], dx[real]) <= tol
    for l in range(2):
        assert max_rel(Ws[l].grad.cpu().numpy(), dWs[l]) <= tol, "dW%d" % l
        assert max_rel(bs[l].grad.cpu().numpy(), dbs[l]) <= tol, "db%d" % l


@pytest.mark.parametrize("shape", FP32_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("layout", ["padded", "packed", "compact"])
def test_wide_bwd_vs_oracle_fp32(api, dev, shape, layout):
    """A two-layer stack Din -> H -> H in fp32 whose backward-data takes the wide form in both layers (H > 608), fwd + bwd through
    gcn_layers against oracle/gcn_ref.py driven by the device's stored activations: dx, dW_l, db_l within GRAD_RTOL."""
    _oracle_case(api, dev, shape, layout, torch.float32)


@pytest.mark.parametrize("shape", BF16_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("layout", ["padded", "packed", "compact"])
def test_wide_bwd_vs_oracle_bf16(api, dev, shape, layout):
    """bf16 operands at H = 1280 (> 1216, past the bf16 row tile): the gradients within the bf16 bar of the other layer tests."""
    _oracle_case(api, dev, shape, layout, torch.bfloat16)


@pytest.mark.parametrize("case", ["no_adj", "dropout"])
def test_wide_bwd_vs_oracle_no_adj_and_dropout(api, dev, case):
    """no_adj (empty ELL for the gather, degrees from the forward pattern) and dropout 0.4 between the layers (the hand-over's
    next_scale), 360 -> 768 -> 768 in fp32."""
    if case == "no_adj":
        _oracle_case(api, dev, (3, 45, 360, 768, 1), "padded", torch.float32, no_adj=True)
    else:
        _oracle_case(api, dev, (3, 45, 360, 768, 1), "padded", torch.float32, drop=0.4)


# ---------------------------------------------------------------------------------------------------------------------------------
# 2.-4. the C-ABI sweep, forced wide form against the row tile
class _Stack:
    """A two-layer stack at the C-ABI: weights packed, the forward with S images (gcnpt_layers_fwd), and the backward sweep
    (gcnpt_layers_bwd / _bwd_dz / _bwd_range) into dh buffers and dZ images pre-filled with NaN."""

    def __init__(self, dev, trees, B, T, x, Ws, bs, compute, mid, out_dtype, drop):
        from gcn_over_pruned_trees_amd import _lib
        from gcn_over_pruned_trees_amd.model.gcn import WeightPack
        self.lib, self.L = _lib, 2
        self.dev, self.trees, self.B, self.T, self.x = dev, trees, B, T, x
        self.cd = _lib.dtype_code(compute)
        self.dims = [tuple(w.shape) for w in Ws]
        self.rows = B * T
        pk = WeightPack(Ws, self.cd, dev)
        _lib.check(_lib.lib().gcnpt_pack_weights_multi(_lib.stream(), *pk.c_args()))
        self.pk, self.bs = pk, bs
        self.drop = drop
        lead = tuple(x.shape[:-1])
        self.outs = [torch.empty(lead + (H,), dtype=out_dtype if l == 1 else mid, device=dev) for l, (H, _) in enumerate(self.dims)]
        self.sf = [torch.zeros((_lib.lib().gcnpt_frag_bytes(self.rows, K, self.cd),), dtype=torch.uint8, device=dev) for _, K in self.dims]
        ints = self._ints
        _lib.check(_lib.lib().gcnpt_layers_fwd(
            _lib.stream(), 2, _lib.ptr(x), _lib.dtype_code(x.dtype), _lib.ptr_array(pk.wf), _lib.ptr_array(bs), _lib.ptr(trees.row_ptr),
            _lib.ptr(trees.col_idx), _lib.ptr(trees.ell), _lib.ptr(trees.ell), B, T, ints([k for _, k in self.dims]),
            ints([h for h, _ in self.dims]), _lib.ptr_array(self.outs), ints([_lib.dtype_code(o.dtype) for o in self.outs]), self.cd,
            (ctypes.c_float * 2)(drop, 0.0), (ctypes.c_uint64 * 2)(17, 0), _lib.ptr_array(self.sf), None))
        torch.cuda.synchronize()

    def _ints(self, v):
        return (ctypes.c_int * self.L)(*v)

    def bwd(self, g, gy_is_dz, pieces=None):
        """The sweep (pieces: run it one launch at a time through gcnpt_layers_bwd_range).  Returns (dh[0], dh[1], z images, dW, db)."""
        lib, t = self.lib, self.trees
        in_dtypes = [self.x.dtype, self.outs[0].dtype]
        dh = [torch.full(tuple(self.x.shape[:-1]) + (K,), float("nan"), dtype=in_dtypes[l], device=self.dev) for l, (_, K) in enumerate(self.dims)]
        zf = [torch.full((lib.lib().gcnpt_frag_bytes(self.rows, H, self.cd),), 0xFF, dtype=torch.uint8, device=self.dev) for H, _ in self.dims]
        dW = [torch.full((H, K), float("nan"), device=self.dev) for H, K in self.dims]
        db = [torch.full((H,), float("nan"), device=self.dev) for H, _ in self.dims]
        scales = (ctypes.c_float * 2)(1.0 / (1.0 - self.drop) if self.drop > 0 else 1.0, 1.0)
        args = (lib.stream(), 2, lib.ptr(g), lib.ptr_array(self.outs), self._ints([lib.dtype_code(o.dtype) for o in self.outs]),
                lib.ptr_array(self.pk.wb), lib.ptr(t.ell), lib.ptr(t.rowT_ptr), lib.ptr(t.colT_idx), lib.ptr(t.ellT), self.B, self.T,
                self._ints([k for _, k in self.dims]), self._ints([h for h, _ in self.dims]), lib.ptr_array(dh),
                self._ints([lib.dtype_code(d) for d in in_dtypes]), self.cd, scales, lib.ptr_array(zf), lib.ptr_array(self.sf),
                lib.ptr_array(dW), lib.ptr_array(db))
        L = lib.lib()
        if pieces is None:
            lib.check((L.gcnpt_layers_bwd_dz if gy_is_dz else L.gcnpt_layers_bwd)(*args))
        else:
            for k in range(pieces):
                lib.check(L.gcnpt_layers_bwd_range(*args, 1 if gy_is_dz else 0, k, 1))
                torch.cuda.synchronize()
        torch.cuda.synchronize()
        return dh, zf, dW, db


def _img_nan(z, compute):
    from gcn_over_pruned_trees_amd import _lib
    return bool(torch.isnan(z.view(torch.float32 if compute == _lib.F32 else torch.bfloat16)).any())


def _stack_case(api, dev, B, T, din, hid, compute, x_dtype, mid, out_dtype, seed):
    from gcn_over_pruned_trees_amd.utils import synthetic
    _, tree = api
    tb = synthetic.random_tree_batch(seed, B, T, "tacred")
    trees = prune(tree, tb, 1, dev)
    Wn, bn = synthetic.layer_params(seed + 1, [din, hid, hid])
    x = to_dev(synthetic.normal(seed + 2, (B, T, din)), dev).to(x_dtype)
    st = _Stack(dev, trees, B, T, x, [to_dev(w, dev) for w in Wn], [to_dev(b, dev) for b in bn], compute, mid, out_dtype, 0.3)
    gy = to_dev(synthetic.normal(seed + 3, (B, T, hid)), dev).to(out_dtype)
    # a ready-made top dZ (what gcnpt_pool3_bwd_dz leaves): zero where the top layer's output is, like the real one
    dz = torch.where(st.outs[1] > 0, gy.float() * 0.25, torch.zeros_like(gy.float())).to(out_dtype)
    return st, gy, dz


# (compute, input x, mid activations, top output): exact fp32; bf16 operands with every (in, out) activation pair of the backward
# launches: f32/f32; layer 1 f32 -> bf16 and layer 0 bf16 -> f32; bf16/bf16
PRECISIONS = [(torch.float32,) * 4, (torch.bfloat16, torch.float32, torch.float32, torch.float32),
              (torch.bfloat16, torch.float32, torch.bfloat16, torch.float32), (torch.bfloat16,) * 4]
# (B, T): 15 row tiles (where the row tile's launch carries the layer above's weight gradient) and a C5-sized batch, 128 x 300
# (1200 row tiles: the row tile's 4-wave form, no rider)
BATCHES = [(12, 40), (128, 300)]


def _forced_cases():
    out = []
    for pr in PRECISIONS:
        for hid in ((200, 304, 600) if pr[0] == torch.float32 else (200, 1200)):
            for bt in BATCHES:
                out.append((pr, hid, bt))
    return out


@pytest.mark.parametrize("entry", ["dy", "dz"])
@pytest.mark.parametrize("case", _forced_cases(), ids=lambda c: "%s-h%d-b%d" % ("-".join(str(d)[6:] for d in c[0]), c[1], c[2][0]))
def test_forced_wide_bwd_matches_row_tile(api, dev, case, entry):
    """GCNPT_OPT_WIDE_BWD = 1 sends every backward-data launch through the wide form.  At widths the row tile also runs, with dropout
    0.3 between the layers (the hand-over's next_scale) and GCNPT_OPT_DETERMINISTIC = 1: the handed-down dZ, dx and both dZ fragment
    images are bit-identical to the row tile's, from a derived top dZ (gcnpt_layers_bwd) and from a ready-made one (gcnpt_layers_bwd_dz,
    the pooling's hand-over).  Every element of dh and of the images is written (they start as NaN).  dW / db come from identical
    images: bit-identical for the big batch, where both sweeps leave every weight gradient to the launch at the end of the sweep.  In
    the small batch the row tile's launch of layer 0 carries layer 1's gradient, so the two sweeps group the weight-gradient launches
    differently, and a deterministic launch's waves per workgroup (hence its summation order) depend on how many layers it holds:
    there they agree to 1e-6."""
    (compute, x_dtype, mid, out_dtype), hid, (B, T) = case
    st, gy, dz = _stack_case(api, dev, B, T, 360, hid, compute, x_dtype, mid, out_dtype, 600 + hid + B)
    g = dz if entry == "dz" else gy
    res = []
    for form in (0, 1):
        with options(WIDE_BWD=form, DETERMINISTIC=1):
            res.append(st.bwd(g, entry == "dz"))
    (dha, zfa, dWa, dba), (dhb, zfb, dWb, dbb) = res
    cd = st.cd
    for l in range(2):
        assert not torch.isnan(dhb[l].float()).any(), "dh[%d]: an element was not written" % l
        assert not _img_nan(zfb[l], cd), "z image %d: an element was not written" % l
        assert torch.equal(dha[l], dhb[l]), "dh[%d]" % l
        assert torch.equal(zfa[l], zfb[l]), "z image %d" % l
        if B * T > 192 * 32:
            assert torch.equal(dWa[l], dWb[l]) and torch.equal(dba[l], dbb[l]), "dW / db %d" % l
        else:
            assert max_rel(dWb[l].cpu().numpy(), dWa[l].cpu().numpy()) <= 1e-6, "dW %d" % l
            assert max_rel(dbb[l].cpu().numpy(), dba[l].cpu().numpy()) <= 1e-6, "db %d" % l
    assert float(dhb[0].float().abs().max()) > 0 and float(dWb[1].abs().max()) > 0


@pytest.mark.parametrize("wide", [1, -1], ids=["forced", "hidden768"])
@pytest.mark.parametrize("entry", ["dy", "dz"])
def test_sweep_in_pieces(api, dev, wide, entry):
    """gcnpt_layers_bwd_range one launch at a time gives the whole sweep's dh, dW and db (deterministic weight gradients): the sweep's
    bookkeeping of launches it does not issue (would_carry) knows that a wide launch carries no weight gradient, so the launch at the
    end of the sweep computes layer 1's.  Small batches (15 row tiles), where a row-tile launch would have carried it: forced at H = 200,
    and by itself at H = 768."""
    hid = 200 if wide == 1 else 768
    st, gy, dz = _stack_case(api, dev, 12, 40, 360, hid, *(torch.float32,) * 4, 700 + hid)
    g = dz if entry == "dz" else gy
    with options(WIDE_BWD=wide, DETERMINISTIC=1):
        whole = st.bwd(g, entry == "dz")
        parts = st.bwd(g, entry == "dz", pieces=4)
    for l in range(2):
        assert torch.equal(whole[0][l], parts[0][l]), "dh[%d]" % l
        assert torch.equal(whole[2][l], parts[2][l]) and torch.equal(whole[3][l], parts[3][l]), "dW / db %d" % l
    assert float(parts[2][1].abs().max()) > 0


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. the option
def test_option_zero_brings_the_refusal_back(api, dev):
    """GCNPT_OPT_WIDE_BWD = 0: the first backward of a 768-wide fp32 stack is refused for its LDS, as before; the default trains it."""
    from gcn_over_pruned_trees_amd import _lib
    from gcn_over_pruned_trees_amd.utils import synthetic
    gcn, tree = api
    B, T = 2, 30
    tb = synthetic.random_tree_batch(5, B, T, "tacred")
    trees = prune(tree, tb, 1, dev)
    Wn, bn = synthetic.layer_params(6, [360, 768, 768])
    x = to_dev(synthetic.normal(7, (B, T, 360)), dev)

    def run():
        Ws = [to_dev(w, dev).requires_grad_() for w in Wn]
        bs = [to_dev(b, dev).requires_grad_() for b in bn]
        gcn.gcn_layers(x, Ws, bs, trees).sum().backward()
        return Ws

    with options(WIDE_BWD=0):
        with pytest.raises(_lib.GcnptError) as e:
            run()
        assert e.value.code == _lib.E_UNSUPPORTED and b"LDS" in str(e.value).encode()
    Ws = run()
    torch.cuda.synchronize()
    assert all(torch.isfinite(w.grad).all() and float(w.grad.abs().max()) > 0 for w in Ws)


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. the module against the reference
def _golden_batch(g):
    """The fixture's batch and parameters, regenerated from its seeds exactly as tests/golden/make_golden_wide_hidden.py draws them,
    and checked against its checksums."""
    import json
    from gcn_over_pruned_trees_amd.utils import synthetic
    seed, B, T = int(g["seed"]), int(g["B"]), int(g["T"])
    vocab = json.loads(str(g["opt"]))["vocab_size"]
    tb = synthetic.random_tree_batch(seed, B, T, g["lens"])
    rng = np.random.RandomState(seed + 1)
    words = rng.randint(2, vocab, size=(B, T)).astype(np.int64)
    pos = rng.randint(2, 47, size=(B, T)).astype(np.int64)
    ner = rng.randint(2, 15, size=(B, T)).astype(np.int64)
    for a in (words, pos, ner):
        a[tb["masks"]] = 0
    assert int(words.sum()) == int(g["words_sum"]) and int(pos.sum()) == int(g["pos_sum"]) and int(ner.sum()) == int(g["ner_sum"])
    assert int(tb["head"].sum()) == int(g["head_sum"])
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
    return (words, tb["masks"], pos, ner, tb["deprel"], tb["head"], tb["subj_pos"], tb["obj_pos"]), sd


@pytest.mark.parametrize("packed", [False, True], ids=["padded", "gcn_packed"])
def test_wide_hidden_classifier_golden(api, dev, packed):
    """GCNClassifier(rnn=False, hidden_dim=768) in fp32 against the reference's own GCNClassifier on the same batch and parameters
    (tests/golden/e2e_wide_hidden.npz, made by tests/golden/make_golden_wide_hidden.py): logits and pooled output within 1e-4, the
    gradients of both GCN weights, both biases and the word / POS / NER tables within GRAD_RTOL."""
    import json
    from conftest import load_golden
    from gcn_over_pruned_trees_amd.utils import synthetic
    gcn, _ = api
    g = load_golden("e2e_wide_hidden.npz")
    batch, sd = _golden_batch(g)
    opt = dict(json.loads(str(g["opt"])), cuda=True, gcn_dtype="fp32", gcn_packed=packed)
    model = gcn.GCNClassifier(opt)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    model = model.to(dev).train()
    logits, pooled = model(tuple(to_dev(a, dev) for a in batch))
    seed = int(g["seed"])
    g_logits = to_dev(synthetic.normal(seed + 3, tuple(logits.shape)), dev)
    g_pooled = to_dev(synthetic.normal(seed + 4, tuple(pooled.shape)), dev)
    ((logits * g_logits).sum() + (pooled * g_pooled).sum()).backward()
    torch.cuda.synchronize()
    assert max_rel(logits.detach().cpu().numpy(), g["logits"]) <= 1e-4
    assert max_rel(pooled.detach().cpu().numpy(), g["pooling_output"]) <= 1e-4
    rel = model.gcn_model
    assert max_rel(rel.emb.weight.grad.cpu().numpy(), g["d_emb"]) <= GRAD_RTOL
    assert max_rel(rel.pos_emb.weight.grad.cpu().numpy(), g["d_pos_emb"]) <= GRAD_RTOL
    assert max_rel(rel.ner_emb.weight.grad.cpu().numpy(), g["d_ner_emb"]) <= GRAD_RTOL
    for l in range(2):
        dW = rel.gcn.W[l].weight.grad.cpu().numpy()
        proj = synthetic.normal(seed + 5 + l, (dW.shape[1], 8))
        assert max_rel(dW[:, ::16], g["dW%d_cols16" % l]) <= GRAD_RTOL, "dW%d" % l
        assert max_rel(dW.astype(np.float64) @ proj, g["dW%d_proj" % l]) <= GRAD_RTOL, "dW%d" % l
        assert max_rel(rel.gcn.W[l].bias.grad.cpu().numpy(), g["db%d" % l]) <= GRAD_RTOL, "db%d" % l


# ---------------------------------------------------------------------------------------------------------------------------------
# 7. capture
def test_wide_hidden_training_step_capture(api, dev):
    """A whole no-RNN training step at hidden_dim = 768 in fp32 (both layers' backward-data in the wide form, the top one from the
    pooling's dZ hand-over), trees from a TreeCache inside the step, captured with torch.cuda.graph: with GCNPT_OPT_DETERMINISTIC = 1
    the replay gives the eager step's loss and the GCN layers' gradients bit for bit (the torch-side gradients of the other
    parameters to 1e-6)."""
    from gcn_over_pruned_trees_amd.utils import synthetic
    gcn, tree = api
    B, T = 16, 50
    tb = synthetic.random_tree_batch(321, B, T, "tacred")
    rng = np.random.RandomState(5)
    words = rng.randint(2, 40, size=(B, T)).astype(np.int64)
    pos = rng.randint(2, 47, size=(B, T)).astype(np.int64)
    ner = rng.randint(2, 15, size=(B, T)).astype(np.int64)
    for a in (words, pos, ner):
        a[tb["masks"]] = 0
    inputs = tuple(to_dev(a, dev) for a in (words, tb["masks"], pos, ner, tb["deprel"], tb["head"], tb["subj_pos"], tb["obj_pos"]))
    labels = to_dev(rng.randint(0, 42, size=(B,)).astype(np.int64), dev)
    opt = dict(vocab_size=40, emb_dim=300, pos_dim=30, ner_dim=30, hidden_dim=768, num_layers=2, input_dropout=0.0, gcn_dropout=0.0,
               word_dropout=0.0, emb_dropout=0.0, topn=1e10, prune_k=1, pooling="max", pooling_l2=0.003, mlp_layers=2, no_adj=False,
               rnn=False, cuda=True, dataset="tacred", num_class=42, adj_type="regular", gcn_dtype="fp32", gcn_check_trees=False)
    torch.manual_seed(99)
    model = gcn.GCNClassifier(opt).to(dev).train()
    cache = tree.TreeCache.build(inputs[5], inputs[6], inputs[7], inputs[4], 1, masks=inputs[1], want_label=False)
    idx = torch.arange(B, device=dev)

    def step():
        model.zero_grad(set_to_none=False)
        logits, pooled = model(inputs, trees=cache.batch(idx, T))
        loss = torch.nn.functional.cross_entropy(logits, labels) + 0.003 * (pooled ** 2).sum(1).mean()
        loss.backward()
        return loss.detach()

    with options(DETERMINISTIC=1):
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(3):
                step()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        params = [p for p in model.parameters() if p.grad is not None]      # (the deprel table of a regular GCN takes no gradient)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            loss = step()
        graph.replay()
        torch.cuda.synchronize()
        l1, g1 = loss.clone(), [p.grad.clone() for p in params]
        le = step()                                      # eager
        torch.cuda.synchronize()
    assert torch.equal(le, l1)
    gcn_params = {id(p) for p in model.gcn_model.gcn.W.parameters()}
    assert len(gcn_params) == 4
    for p, g in zip(params, g1):
        if id(p) in gcn_params:
            assert torch.equal(p.grad, g)
        else:
            assert max_rel(p.grad.cpu().numpy(), g.cpu().numpy()) <= 1e-6
    W1 = model.gcn_model.gcn.W[1].weight
    assert torch.isfinite(W1.grad).all() and float(W1.grad.abs().max()) > 0
