"""
The three masked poolings (model/gcn.py:116-121) on token-packed rows, forward and backward, with the dZ hand-over to the top layer:
gcnpt_pool3_fwd_packed / gcnpt_pool3_bwd_packed / gcnpt_pool3_bwd_dz_packed, model.gcn.pool3_packed, gcn_layers(pool=...) with a
PackedTrees, and GCNClassifier with opt['gcn_packed'] (whose layer-stack output is then never unpacked).

The packed kernels map token i of a sentence to the same stream and round as the padded ones, and a pad slot contributes +0.0 to a sum
and -1e12 to a max there, so packed == padded BIT FOR BIT (the loader's pad positions are non-zero); against the CPU the sums run in
another order (FWD_RTOL).
"""
import json

import numpy as np
import pytest
import torch

from conftest import load_golden
from helpers import FWD_RTOL, GRAD_RTOL, max_rel
from gcn_over_pruned_trees_amd.utils import synthetic

pytestmark = pytest.mark.gpu

KINDS = ["max", "avg", "sum"]
LONG_LENS = np.array([300, 257, 200, 129, 128, 127, 65, 64, 33, 32, 31, 9])


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu-marked tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def api():
    from gcn_over_pruned_trees_amd import _lib
    from gcn_over_pruned_trees_amd.model import gcn, tree
    _lib.lib()
    return gcn, tree


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _batch(tree, dev, seed, B, T, lengths, K, n_rows=None):
    """(tb, padded trees, packed trees, subj, obj) of a synthetic batch."""
    tb = synthetic.random_tree_batch(seed, B, T, lengths)
    head, subj, obj, deprel, masks = (_t(tb[k], dev) for k in ("head", "subj_pos", "obj_pos", "deprel", "masks"))
    trees = tree.prune_to_csr(head, subj, obj, deprel, K, masks=masks).check(expect_maxlen=T)
    packed = trees.pack(tb["lens"].tolist(), n_rows=n_rows)
    if n_rows is None:
        packed.check()
    return tb, trees, packed, subj, obj


def _both_pools(gcn, trees, packed, subj, obj, h, gp, kind):
    """(packed out, packed grad of hp, padded out, padded grad packed with pack_rows) for h [B,T,H]."""
    hp = packed.pack_rows(h).detach().requires_grad_()
    out_p = gcn.pool3_packed(hp, packed, subj, obj, kind)
    out_p.backward(gp)
    hq = packed.pack_rows(h).detach().requires_grad_()
    hu = packed.unpack_rows(hq)
    hu.retain_grad()
    out_u = gcn.pool3(hu, trees.pool_mask, subj, obj, kind)
    out_u.backward(gp)
    return out_p.detach(), hp.grad, out_u.detach(), packed.pack_rows(hu.grad)


SHAPES = {"h72": (301, 23, 61, "tacred", 1, 72), "h75": (301, 23, 61, "tacred", 1, 75), "t300": (306, 12, 300, LONG_LENS, 2, 300)}


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_packed_pool_equals_padded_pool(api, dev, shape, kind, dtype):
    """pool3_packed on packed rows == pool3 on the unpacked tensor, output and gradient, bit for bit (H=75: element loads; t300: five
    sentences on either side of the kernels' 128-token regime)."""
    gcn, tree = api
    seed, B, T, lengths, K, H = SHAPES[shape]
    tb, trees, packed, subj, obj = _batch(tree, dev, seed, B, T, lengths, K)
    if shape != "t300":
        assert packed.N == 879 and B * T == 1403
    h = _t(synthetic.normal(seed + 1, (B, T, H)), dev).to(dtype)
    gp = _t(synthetic.normal(seed + 2, (B, 3 * H)), dev)
    out_p, g_p, out_u, g_u = _both_pools(gcn, trees, packed, subj, obj, h, gp, kind)
    assert tuple(out_p.shape) == (B, 3 * H) and tuple(g_p.shape) == (packed.N, H) and g_p.dtype == dtype
    assert torch.isfinite(out_p).all()
    assert torch.equal(out_p, out_u)
    assert torch.equal(g_p, g_u)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("kind", KINDS)
def test_pools_match_reference_pool_t300(api, dev, kind, dtype):
    """Both forms against the reference's pool() (model/gcn.py:473-483) run by torch on the CPU, at T = 300."""
    gcn, tree = api
    B, T, H = 12, 300, 300
    tb, trees, packed, subj, obj = _batch(tree, dev, 306, B, T, LONG_LENS, 2)
    h = _t(synthetic.normal(307, (B, T, H)), dev).to(dtype)
    hc = h.float().cpu()
    masks = [trees.pool_mask.cpu(), (subj != 0).cpu().unsqueeze(2), (obj != 0).cpu().unsqueeze(2)]
    ref = torch.cat([gcn.pool(hc, m, kind) for m in masks], dim=1).numpy()
    got_p = gcn.pool3_packed(packed.pack_rows(h), packed, subj, obj, kind).cpu().numpy()
    got_u = gcn.pool3(h, trees.pool_mask, subj, obj, kind).cpu().numpy()
    assert np.isfinite(ref).all()
    for got in (got_p, got_u):
        print("pool %s %s: max_rel %.3e" % (kind, dtype, max_rel(got, ref)))
        if kind == "max":
            assert np.array_equal(got, ref)
        else:
            assert max_rel(got, ref) <= FWD_RTOL


@pytest.mark.parametrize("kind", KINDS)
def test_packed_pool_edge_sentences(api, dev, kind):
    """One-token sentences have no tree token at all: -1e12 (max), 0 (sum) and NaN (avg) in the same places as the padded form."""
    gcn, tree = api
    B, T, H = 6, 40, 24
    tb, trees, packed, subj, obj = _batch(tree, dev, 307, B, T, np.array([40, 17, 3, 2, 1, 1]), 1)
    h = _t(synthetic.normal(308, (B, T, H)), dev)
    gp = _t(synthetic.normal(309, (B, 3 * H)), dev)
    out_p, g_p, out_u, g_u = _both_pools(gcn, trees, packed, subj, obj, h, gp, kind)
    a, b = out_p.cpu().numpy(), out_u.cpu().numpy()
    assert np.array_equal(a, b, equal_nan=True)
    tree_part = a[4:, :H]
    if kind == "max":
        assert (tree_part == np.float32(-1e12)).all()
    elif kind == "sum":
        assert (tree_part == 0).all()
    else:
        assert np.isnan(tree_part).all()
    assert np.array_equal(g_p.cpu().numpy(), g_u.cpu().numpy(), equal_nan=True)


@pytest.mark.parametrize("kind", KINDS)
def test_packed_pool_backward_zeroes_surplus_rows(api, dev, kind):
    """n_rows = sum(len) + 37: both backward forms write dh completely -- the rows past sum(len) are zero, not what the buffer held."""
    from gcn_over_pruned_trees_amd import _lib
    gcn, tree = api
    seed, B, T, lengths, K, H = SHAPES["h72"]
    tb, trees, exact, subj, obj = _batch(tree, dev, seed, B, T, lengths, K)
    N = exact.N
    tb, trees, packed, subj, obj = _batch(tree, dev, seed, B, T, lengths, K, n_rows=N + 37)
    torch.cuda.synchronize()
    assert int(packed.status[0]) == 0 and int(packed.status[1]) == N and packed.N == N + 37
    h = _t(synthetic.normal(seed + 1, (B, T, H)), dev)
    gp = _t(synthetic.normal(seed + 2, (B, 3 * H)), dev)
    _, want, _, _ = _both_pools(gcn, trees, exact, subj, obj, h, gp, kind)
    hp = torch.zeros((N + 37, H), device=dev)
    hp[:N] = exact.pack_rows(h)
    L, st, P = _lib.lib(), _lib.stream(), _lib.ptr
    code = KINDS.index(kind)
    out = torch.empty((B, 3 * H), device=dev)
    amax = torch.empty((B, 3, H), dtype=torch.int32, device=dev)
    pm = packed.pool_mask.contiguous()
    _lib.check(L.gcnpt_pool3_fwd_packed(st, P(hp), _lib.F32, P(pm), P(subj), P(obj), P(packed.cu_seqlens), B, T, N + 37, H, code, P(out), P(amax)))
    assert torch.equal(out, gcn.pool3_packed(exact.pack_rows(h), exact, subj, obj, kind))
    dh = torch.full((N + 37, H), float("nan"), device=dev)
    _lib.check(L.gcnpt_pool3_bwd_packed(st, P(gp), P(amax), P(pm), P(subj), P(obj), P(packed.cu_seqlens), B, T, N + 37, H, code, P(dh), _lib.F32))
    assert (dh[N:] == 0).all() and torch.equal(dh[:N], want)
    # the dZ form with y = 1 and scale 1: dz = dh / (deg + 1)
    dz = torch.full((N + 37, H), float("nan"), device=dev)
    y = torch.ones((N + 37, H), device=dev)
    _lib.check(L.gcnpt_pool3_bwd_dz_packed(st, P(gp), P(amax), P(pm), P(subj), P(obj), P(packed.cu_seqlens), B, T, N + 37, H, code, P(y), P(packed.ell),
                                           1.0, P(dz), _lib.F32))
    deg = packed.ell.view(-1, 8)[:N, 0].float().unsqueeze(1)
    assert (dz[N:] == 0).all() and torch.equal(dz[:N], want * (1.0 / (deg + 1.0)))


@pytest.mark.parametrize("compute", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("kind", KINDS)
def test_pool_handover_op_on_packed_rows(api, dev, compute, kind):
    """tests/test_gpu_parity.py::test_pool_handover_op_matches_two_ops on packed rows: gcn_layers(pool=...) with a PackedTrees against
    pool3(unpack_rows(gcn_layers(...))), dropout on both layers; bounds of that test (fp32: same arithmetic, only the order of the weight
    gradient's atomics moves).  The forward also equals the padded op's bit for bit when dropout is off (dropout hashes the row number)."""
    gcn, tree = api
    B, T, din, hid = 23, 61, 88, 72
    tb, trees, packed, subj, obj = _batch(tree, dev, 77, B, T, "tacred", 1)
    Wn, bn = synthetic.layer_params(5, [din, hid, hid])
    x0 = _t(synthetic.normal(6, (B, T, din)), dev)
    gp = _t(synthetic.normal(7, (B, 3 * hid)), dev)
    res = []
    for handover in (False, True):
        Ws = [_t(w, dev).requires_grad_() for w in Wn]
        bs = [_t(b, dev).requires_grad_() for b in bn]
        xp = packed.pack_rows(x0).detach().requires_grad_()
        kw = dict(drop_p=[0.3, 0.4], seeds=[11, 12], compute_dtype=compute, out_dtype=torch.float32)
        if handover:
            pooled = gcn.gcn_layers(xp, Ws, bs, packed, pool=(subj, obj, kind), **kw)
        else:
            pooled = gcn.pool3(packed.unpack_rows(gcn.gcn_layers(xp, Ws, bs, packed, **kw)), trees.pool_mask, subj, obj, type=kind)
        pooled.backward(gp)
        res.append([pooled.detach()] + [t.grad for t in [xp] + Ws + bs])
    tol = 2e-5 if compute == torch.float32 else 2e-2
    for a, b in zip(*res):
        assert torch.isfinite(b).all()
        err = max_rel(b.float().cpu().numpy(), a.float().cpu().numpy())
        print("handover packed %s %s: %.3e" % (kind, compute, err))
        assert err <= tol
    assert torch.equal(res[0][0], res[1][0])
    Ws, bs = [_t(w, dev) for w in Wn], [_t(b, dev) for b in bn]
    kw = dict(compute_dtype=compute, out_dtype=torch.float32)
    with torch.no_grad():
        assert torch.equal(gcn.gcn_layers(packed.pack_rows(x0), Ws, bs, packed, pool=(subj, obj, kind), **kw),
                           gcn.gcn_layers(x0, Ws, bs, trees, pool=(subj, obj, kind), **kw))


@pytest.mark.parametrize("kind", ["max", "avg"])
def test_packed_handover_vs_oracle(api, dev, kind):
    """B=50, T=100, 360 -> 200 -> 200, fp32, no dropout: the pooled output and dx / dW / db against the CPU oracle (gcn_forward + pool,
    gcn_backward fed with the pooling's gradient computed in NumPy)."""
    from oracle import gcn_ref, prune_ref
    gcn, tree = api
    B, T, din, hid, K = 50, 100, 360, 200, 1
    tb, trees, packed, subj, obj = _batch(tree, dev, 303, B, T, "tacred", K)
    Ws, bs = synthetic.layer_params(304, [din, hid, hid])
    x, gp = synthetic.normal(305, (B, T, din)), synthetic.normal(306, (B, 3 * hid))
    keep = ~tb["masks"]
    adj = prune_ref.batch_adj(tb["head"], tb["subj_pos"], tb["obj_pos"], tb["deprel"], tb["lens"], K)["adj"]
    href, mask = gcn_ref.gcn_forward(adj, x, Ws, bs)
    ms = [mask, (tb["subj_pos"] != 0)[..., None], (tb["obj_pos"] != 0)[..., None]]
    assert all((~m).any(1).all() for m in ms)                         # every sentence pools at least one token, three times
    pref = np.concatenate([gcn_ref.pool(href, m, kind) for m in ms], axis=1)
    gy = np.zeros_like(href)
    for k, m in enumerate(ms):                                        # d pool / d h (gcn.py:473-483)
        g = gp[:, k * hid:(k + 1) * hid]
        if kind == "max":
            am = np.where(m, np.float32(-1e12), href).argmax(1)       # [B,H], first maximum
            np.add.at(gy, (np.arange(B)[:, None], am, np.arange(hid)[None, :]), g)
        else:
            cnt = (T - m.astype(np.float32).sum(1))                   # [B,1]
            gy += np.where(m, np.float32(0), (g / cnt)[:, None, :])
    dx, dWs, dbs = gcn_ref.gcn_backward(adj, x, Ws, bs, gy.astype(np.float32))
    xp = _t(x[keep], dev).requires_grad_()
    Wt = [_t(w, dev).requires_grad_() for w in Ws]
    bt = [_t(b, dev).requires_grad_() for b in bs]
    pooled = gcn.gcn_layers(xp, Wt, bt, packed, pool=(subj, obj, kind), compute_dtype=torch.float32, out_dtype=torch.float32)
    pooled.backward(_t(gp, dev))
    errs = [max_rel(pooled.detach().cpu().numpy(), pref), max_rel(xp.grad.cpu().numpy(), dx[keep])]
    errs += [max_rel(Wt[l].grad.cpu().numpy(), dWs[l]) for l in range(2)] + [max_rel(bt[l].grad.cpu().numpy(), dbs[l]) for l in range(2)]
    print("packed handover vs oracle %s: %s" % (kind, ["%.2e" % e for e in errs]))
    assert errs[0] <= FWD_RTOL
    assert max(errs[1:]) <= GRAD_RTOL


@pytest.mark.parametrize("fixture", ["e2e_gcn.npz", "e2e_avgpool.npz", "e2e_cgcn.npz"])
def test_packed_classifier_pools_packed_rows(api, dev, fixture, monkeypatch):
    """GCNClassifier with gcn_packed: hand-over on (default) and off give the same eval logits bit for bit (the golden ones to 1e-4) and
    the same parameter gradients to 1e-4 -- and with the hand-over the stack's output is never unpacked."""
    gcn, tree = api
    e = load_golden(fixture)
    opt = json.loads(str(e["opt"]))
    opt["cuda"] = True
    keys = ("words", "masks", "pos", "ner", "deprel", "head", "subj_pos", "obj_pos") if opt["dataset"] == "tacred" else \
        ("words", "masks", "pos", "deprel", "head", "subj_pos", "obj_pos")
    inputs = tuple(_t(e[k], dev) for k in keys)
    sd = {k[3:]: torch.from_numpy(v) for k, v in e.items() if k.startswith("sd:")}
    out = []
    for handover in (False, True):
        model = gcn.GCNClassifier(dict(opt, gcn_packed=True, gcn_pool_handover=handover))
        model.load_state_dict(sd, strict=True)
        model.to(dev).eval()
        if handover:
            def no_unpack(self, t):
                raise AssertionError("PackedTrees.unpack_rows reached on the hand-over path")
            monkeypatch.setattr(tree.PackedTrees, "unpack_rows", no_unpack)
            seen = []
            model.gcn_model.gcn.register_forward_hook(lambda m, i, o: seen.append(o[0]))
        with torch.no_grad():
            le, pe = model(inputs)
        assert max_rel(le.cpu().numpy(), e["logits"]) <= 1e-4
        model.train()
        torch.manual_seed(99)
        logits, pooled = model(inputs)
        (logits.logsumexp(1).mean() + 0.003 * (pooled ** 2).sum(1).mean() + 1e-3 * model.conv_l2()).backward()
        torch.cuda.synchronize()
        if handover:
            assert seen and all(isinstance(o, gcn._Pooled) for o in seen)          # the marker, not h [B,T,H]
            monkeypatch.undo()
        out.append((le, pe, {n: p.grad for n, p in model.named_parameters() if p.grad is not None}))
    (la, pa, ga), (lb, pb, gb) = out
    assert torch.equal(la, lb) and torch.equal(pa, pb)
    assert set(ga) == set(gb) and len(ga) > 4
    for n in ga:
        assert max_rel(gb[n].cpu().numpy(), ga[n].cpu().numpy()) <= 1e-4, n


def test_packed_handover_graph_capture(api, dev):
    """Trees from TreeCache.batch_packed; gcn_layers(pool=...) on packed rows, forward and backward, captured once and replayed twice:
    pooled output and dx equal the eager ones bit for bit, dW / db to 1e-6 (their float atomics)."""
    gcn, tree = api
    B, T, din, hid = 50, 100, 360, 200
    tb = synthetic.random_tree_batch(1234, B, T, "tacred")
    head, subj, obj, deprel, masks = (_t(tb[k], dev) for k in ("head", "subj_pos", "obj_pos", "deprel", "masks"))
    cache = tree.TreeCache.build(head, subj, obj, deprel, 1, masks=masks, want_label=False)
    ids = torch.arange(B, device=dev)
    N = int(tb["lens"].sum())
    Wn, bn = synthetic.layer_params(2, [din, hid, hid])
    Ws = [_t(w, dev).requires_grad_() for w in Wn]
    bs = [_t(b, dev).requires_grad_() for b in bn]
    xp = _t(synthetic.normal(3, (B, T, din))[~tb["masks"]], dev).requires_grad_()
    gp = _t(synthetic.normal(4, (B, 3 * hid)), dev)

    def step():
        for t in Ws + bs + [xp]:
            t.grad = None
        packed = cache.batch_packed(ids, T, n_rows=N)
        pooled = gcn.gcn_layers(xp, Ws, bs, packed, [0.5, 0.0], [11, 0], torch.bfloat16, torch.float32, pool=(subj, obj, "max"))
        pooled.backward(gp)
        return pooled.detach()

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            want = step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    want = want.clone()
    want_g = [t.grad.clone() for t in [xp] + Ws + bs]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = step()
    for _ in range(2):
        graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(got, want)
    assert torch.equal(xp.grad, want_g[0])
    for t, w in zip(Ws + bs, want_g[1:]):
        assert max_rel(t.grad.cpu().numpy(), w.cpu().numpy()) <= 1e-6
