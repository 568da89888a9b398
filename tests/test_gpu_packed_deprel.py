"""
The relation-aware adjacency types on token-packed trees (opt['gcn_packed'] with adj_type 'full_deprel' / 'diagonal_deprel'):

  * PackedTrees.pack_ids (gcnpt_pack_ids): the loader's int64 ids in packed order, `fill` in the rows past sum(len)
  * gcnpt_full_agg_*_packed / gcnpt_diag_layer_*_packed against the padded entry points on the same operands: a real token's row is
    BIT-IDENTICAL, the rows past sum(len) (n_rows = sum(len) + 5 throughout) are zero
  * GCN.forward(PackedTrees, inputs) against the values recorded from the reference, trees from prune_to_csr_packed and from
    TreeCache.batch_packed, and GCNClassifier(gcn_packed=True) against its recorded logits
  * one full_deprel training step on packed trees captured with torch.cuda.graph

What "against the recorded values" means on packed rows.  The fixtures' x and gy are non-zero in the pad slots, and the reference computes
them: a pad token has no adjacency entry, so its row is a chain of self-loop terms that no real token reads, and its gy flows into dW / db /
dE / dx of its own slot only.  Packed rows hold no pad slot (unpack_rows leaves zeros there, include/gcnpt.h).  A backward is linear in gy
and the pad rows are isolated, so what the packed path must give is
    h        = recorded h on the real slots, exactly 0 on the pad slots
    gradient = recorded gradient - oracle backward of (gy restricted to the pad slots)      (oracle/gcn_ref.py, the fp32 restatement)
and the bars of test_full_deprel_golden / test_diag_deprel_golden apply to that unchanged.  The correction is zero on every real slot of dx.
"""
import functools
import json

import numpy as np
import pytest
import torch

from conftest import dense_from_coo, load_golden
from helpers import FWD_RTOL, GRAD_RTOL, cuda_dev, fro_rel, gcn_api, max_rel, to_dev
from gcn_over_pruned_trees_amd.utils import synthetic

pytestmark = pytest.mark.gpu

FA_FWD, FA_REV = 42, 84              # utils/constant.py:14,16
SUM_TOL = 1e-6                       # a float64 host sum of <= 4 fp32 terms against the device's fp32 one: a few ulps of max|.|
BF16_FRO = 1e-1                      # tests/test_gpu_parity.py


@pytest.fixture(scope="module")
def dev():
    return cuda_dev()


@pytest.fixture(scope="module")
def api():
    return gcn_api()


# ---------------------------------------------------------------------------------------------------
# the batches
# ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _edge_batch():
    """trees_edge_cases.npz (sentences of length T = 12, one of 9, failed parses with empty rows) plus a length-1 sentence."""
    g = load_golden("trees_edge_cases.npz")
    T = g["head"].shape[1]
    one = lambda first, rest: np.array([[first] + [rest] * (T - 1)], np.int64)  # noqa: E731
    return dict(head=np.concatenate([g["head"], one(0, 0)]), deprel=np.concatenate([g["deprel"], one(5, 0)]),
                subj_pos=np.concatenate([g["subj_pos"], np.arange(T, dtype=np.int64)[None]]),
                obj_pos=np.concatenate([g["obj_pos"], np.arange(T, dtype=np.int64)[None]]),
                lens=np.concatenate([g["lens"].astype(np.int64), [1]]))


def _labelled_pair(tree, dev, tb, K=1, extra=5, plant=True):
    """(padded PrunedTrees with labels, the same batch .pack()ed into sum(len) + extra rows).  plant: three entries of the first sentence
    that has them get the labels 0, 42 and 84 -- the values that fall in neither range (gcn.py:308-311, 340-344)."""
    lens = tb["lens"].astype(np.int64)
    padded = tree.prune_to_csr(*(to_dev(tb[k], dev) for k in ("head", "subj_pos", "obj_pos", "deprel")), K,
                               lens=to_dev(lens.astype(np.int32), dev), want_label=True)
    if plant:
        rp = padded.row_ptr.view(padded.B, padded.T + 1).cpu().numpy()
        b0 = int(np.flatnonzero(rp[:, -1] - rp[:, 0] >= 3)[0])
        padded.label[int(rp[b0, 0]):int(rp[b0, 0]) + 3] = torch.tensor([0, FA_FWD, FA_REV], dtype=torch.int32, device=dev)
    pk = padded.pack(lens.tolist(), n_rows=int(lens.sum()) + extra)
    torch.cuda.synchronize()
    assert int(pk.status[0]) == 0 and int(pk.cu_seqlens[-1]) == int(lens.sum())
    return padded, pk


def _host_csr(pk):
    n = int(pk.cu_seqlens[-1])
    rp = pk.row_ptr[:n + 1].cpu().numpy()
    nnz = int(rp[n])
    return n, rp, pk.col_idx[:nnz].cpu().numpy(), pk.label[:nnz].cpu().numpy()


def _slot_map(padded, pk):
    """padded CSR slot of every packed CSR slot (the packer keeps a sentence's entries in order, offsets contiguous)."""
    cu = pk.cu_seqlens.cpu().numpy()
    rp_pk = pk.row_ptr.cpu().numpy()
    rp_pad = padded.row_ptr.view(padded.B, padded.T + 1).cpu().numpy()
    idx = np.zeros(int(rp_pk[cu[-1]]), np.int64)
    for b in range(padded.B):
        lo, hi = int(rp_pk[cu[b]]), int(rp_pk[cu[b + 1]])
        idx[lo:hi] = rp_pad[b, 0] + np.arange(hi - lo)
        assert hi - lo == rp_pad[b, min(int(cu[b + 1] - cu[b]), padded.T)] - rp_pad[b, 0]
    return idx


def _real_slots(tb, T):
    return np.arange(T)[None, :] < tb["lens"][:, None]


# ---------------------------------------------------------------------------------------------------
# 1. pack_ids
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["edge_cases", "random_12x70"])
def test_pack_ids(api, dev, case):
    gcn, tree = api
    tb = _edge_batch() if case == "edge_cases" else synthetic.random_tree_batch(93, 12, 70, "tacred")
    lens = tb["lens"].astype(np.int64)
    B, T = tb["head"].shape
    _, pk = _labelled_pair(tree, dev, tb, plant=False)
    assert pk.N == int(lens.sum()) + 5
    want = np.concatenate([tb["deprel"][b, :lens[b]] for b in range(B)])
    deprel = to_dev(tb["deprel"], dev)
    for fill in (0, 77, -1):
        got = pk.pack_ids(deprel, fill=fill) if fill else pk.pack_ids(deprel)
        assert got.dtype == torch.int64 and tuple(got.shape) == (pk.N,)
        got = got.cpu().numpy()
        np.testing.assert_array_equal(got[:len(want)], want)
        np.testing.assert_array_equal(got[len(want):], np.full(5, fill, np.int64))
    big = deprel + (1 << 40)                                            # all 64 bits travel
    np.testing.assert_array_equal(pk.pack_ids(big).cpu().numpy()[:len(want)], want + (1 << 40))
    with pytest.raises(TypeError, match="pack_ids"):
        pk.pack_rows(deprel)
    with pytest.raises(TypeError):
        pk.pack_ids(deprel.to(torch.int32))


# ---------------------------------------------------------------------------------------------------
# 2. full_agg, op level
# ---------------------------------------------------------------------------------------------------
def _host_full_agg(n, rp, ci, lab, yf, yr, st, kf, kr):
    """float64 relu(agg / (deg + 1)) of the live rows, and the (row, column, direction) of every entry that contributes."""
    z = np.zeros((n, yf.shape[1])) if st is None else st[:n].astype(np.float64).copy()
    used = []
    for r in range(n):
        for e in range(rp[r], rp[r + 1]):
            fw, rv = 0 < lab[e] < FA_FWD, FA_FWD < lab[e] < FA_REV
            if not (fw or (rv and yr is not None)):
                continue
            keep = kf if fw else kr
            if keep is not None and not keep[e]:
                continue
            z[r] += (yf if fw else yr)[ci[e]].astype(np.float64)
            used.append((r, int(ci[e]), fw))
        z[r] /= rp[r + 1] - rp[r] + 1
    return np.maximum(z, 0.0), used


@pytest.mark.parametrize("variant", ["plain", "edge_keep", "directed", "dropout"])
@pytest.mark.parametrize("H", [200, 6], ids=["H200_vec", "H6_scalar"])
def test_full_agg_packed_vs_padded(api, dev, H, variant):
    gcn, tree = api
    tb = _edge_batch()
    padded, pk = _labelled_pair(tree, dev, tb)
    B, T, N = padded.B, padded.T, pk.N
    n, rp, ci, lab = _host_csr(pk)
    assert N == n + 5 and N % 4 != 0 and 1 in tb["lens"] and T in tb["lens"]
    assert {0, FA_FWD, FA_REV} <= set(lab.tolist()) and ((lab > 0) & (lab < FA_FWD)).any() and ((lab > FA_FWD) & (lab < FA_REV)).any()
    rng = np.random.RandomState(H + len(variant))
    mk = lambda *s: to_dev(rng.standard_normal(s).astype(np.float32), dev)  # noqa: E731
    yf, st, g = mk(N, H), mk(N, H), mk(N, H)
    yr = None if variant == "directed" else mk(N, H)
    kf = kr = None
    if variant != "plain":
        kf = to_dev((rng.rand(pk.nnz_cap) < 0.6).astype(np.uint8), dev)
        kr = None if variant == "directed" else to_dev((rng.rand(pk.nnz_cap) < 0.6).astype(np.uint8), dev)
    p, seed = (0.4, 20240607) if variant == "dropout" else (0.0, 0)
    real = to_dev(_real_slots(tb, T), dev)

    def run(trees, yf_, yr_, st_, pos, kf_, kr_, M, g_):
        leaves = [None if t is None else t.clone().requires_grad_() for t in (yf_, yr_, st_)]
        out = gcn._FullAggFn.apply(leaves[0], leaves[1], leaves[2], trees, pos, kf_, kr_, M, p, seed, None)
        out.backward(g_)
        return [out.detach()] + [None if t is None else t.grad for t in leaves]

    out, dyf, dyr, dagg = run(pk, yf, yr, st, None, kf, kr, N, g)
    torch.cuda.synchronize()
    assert tuple(out.shape) == (N, H) and not out[n:].any() and not dagg[n:].any()          # dead rows: exactly zero
    # the padded run on the same operands: rows unpacked, identity pos, the keep flags moved to the padded slots
    slot = torch.from_numpy(_slot_map(padded, pk)).to(dev)

    def pad_keep(k):
        if k is None:
            return None
        out_k = torch.zeros((B * padded.cap,), dtype=torch.uint8, device=dev)
        out_k[slot] = k[:slot.numel()]
        return out_k
    un = lambda t: None if t is None else pk.unpack_rows(t).reshape(B * T, H)  # noqa: E731
    ident = torch.arange(B * T, dtype=torch.int32, device=dev)
    out_p, dyf_p, dyr_p, dagg_p = run(padded, un(yf), un(yr), un(st), ident, pad_keep(kf), pad_keep(kr), B * T, un(g))
    pick = lambda t: t.view(B, T, H)[real]  # noqa: E731
    if p == 0.0:
        assert torch.equal(out[:n], pick(out_p)), "forward rows differ between the layouts"
        assert torch.equal(dagg[:n], pick(dagg_p)), "dagg rows differ between the layouts"
    else:
        # The dropout hash is keyed on the row number, which one seed cannot make agree between the layouts once a sentence is
        # shorter than T.  Up to the end of the first short sentence the packed row number IS the padded one: bit-equal there, same
        # seed.  Everywhere: a float64 host computation with the keep bits read off the output's zero pattern.
        same = int(np.cumsum(tb["lens"])[int(np.flatnonzero(tb["lens"] < T)[0])])
        assert same >= T and torch.equal(out[:same], pick(out_p)[:same]) and torch.equal(dagg[:same], pick(dagg_p)[:same])
    f = lambda t: None if t is None else t.cpu().numpy()  # noqa: E731
    z, used = _host_full_agg(n, rp, ci, lab, f(yf), f(yr), f(st), f(kf), f(kr))
    scale = float(np.float32(1.0 / (1.0 - p))) if p > 0 else 1.0
    o = f(out)[:n].astype(np.float64)
    kept = (o != 0) | (z <= 0)
    err = np.abs(o - np.where(kept, z * scale, 0.0)).max() / np.abs(z * scale).max()
    print("full_agg fwd vs float64: %.2e" % err)
    assert err <= SUM_TOL
    if p > 0 and H == 200:                      # ~9 000 positive elements: 0.03 is six standard deviations of the kept fraction
        assert abs((o != 0)[z > 1e-3].mean() - (1 - p)) < 0.03
    deg1 = (rp[1:n + 1] - rp[:n] + 1)[:, None]
    dz = np.where(o > 0, f(g)[:n].astype(np.float64) * scale / deg1, 0.0)
    err = np.abs(f(dagg)[:n] - dz).max() / np.abs(dz).max()
    print("full_agg dagg vs float64: %.2e" % err)
    assert err <= SUM_TOL
    # dyf / dyr: a float64 scatter of the device's own dagg along the entries (at most three fp32 atomic adds per traversed row)
    src = f(dagg).astype(np.float64)
    want_f, want_r = np.zeros((N, H)), np.zeros((N, H))
    for r, c, fw in used:
        (want_f if fw else want_r)[c] += src[r]
    for got, want, name in ((dyf, want_f, "dyf"), (dyr, want_r, "dyr")):
        if got is None:
            assert name == "dyr" and variant == "directed"
            continue
        err = np.abs(f(got) - want).max() / max(np.abs(want).max(), 1e-30)
        print("full_agg %s vs float64 scatter: %.2e" % (name, err))
        assert np.abs(want).max() > 0 and err <= SUM_TOL, name


# ---------------------------------------------------------------------------------------------------
# 3. diag layer, op level
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("H", [200, 6], ids=["H200_vec", "H6_scalar"])
def test_diag_layer_packed_vs_padded(api, dev, H, dtype):
    gcn, tree = api
    tb = _edge_batch()
    padded, pk = _labelled_pair(tree, dev, tb)
    B, T, N = padded.B, padded.T, pk.N
    n = int(pk.cu_seqlens[-1])
    rng = np.random.RandomState(H)
    mk = lambda *s: to_dev(rng.standard_normal(s).astype(np.float32), dev)  # noqa: E731
    h, g = mk(N, H).to(dtype), mk(N, H).to(dtype)
    E = to_dev(rng.uniform(-1, 1, size=(85, H)).astype(np.float32), dev)
    deprel = to_dev(tb["deprel"], dev)
    real = to_dev(_real_slots(tb, T), dev)

    def run(trees, h_, dep, g_):
        hl, El = h_.clone().requires_grad_(), E.clone().requires_grad_()
        out = gcn.diag_layer(hl, El, dep, trees)
        out.backward(g_)
        return out.detach(), hl.grad, El.grad

    out, dh, dE = run(pk, h, pk.pack_ids(deprel), g)
    out_p, dh_p, dE_p = run(padded, pk.unpack_rows(h), deprel, pk.unpack_rows(g))
    torch.cuda.synchronize()
    assert tuple(out.shape) == (N, H) and out.dtype == dtype
    assert not out[n:].any() and not dh[n:].any()                                           # dead rows: exactly zero
    assert torch.equal(out[:n], out_p[real]), "forward rows differ between the layouts"
    assert torch.equal(dh[:n], dh_p[real]), "dh rows differ between the layouts"
    assert out[:n].abs().sum() > 0 and dh[:n].abs().sum() > 0
    a, b = dE.float().cpu().numpy(), dE_p.float().cpu().numpy()
    err = max_rel(a, b) if dtype == torch.float32 else fro_rel(a, b)
    print("diag dE packed vs padded (%s): %.2e" % (dtype, err))
    assert np.abs(b).max() > 0 and err <= (GRAD_RTOL if dtype == torch.float32 else 3e-2)   # test_diag_deprel_vs_oracle's bars for dE


# ---------------------------------------------------------------------------------------------------
# 4. / 5. GCN.forward(PackedTrees, inputs) against the recorded values
# ---------------------------------------------------------------------------------------------------
def _packed_trees(tree, dev, g, source, lens, K, extra=0):
    head, subj, obj, dep = (to_dev(g[k], dev) for k in ("head", "subj_pos", "obj_pos", "deprel"))
    n_rows = int(np.sum(lens)) + extra
    if source == "pruner":
        return tree.prune_to_csr_packed(head, subj, obj, dep, K, [int(v) for v in lens], want_label=True, n_rows=n_rows)
    cache = tree.TreeCache.build(head, subj, obj, dep, K, lens=to_dev(np.asarray(lens, np.int32), dev), want_label=True)
    return cache.batch_packed(torch.arange(head.shape[0], device=dev), head.shape[1], n_rows=n_rows)


def _deprel_gcn(api, dev, adj_type, din, hidden, layers, table, **kw):
    gcn, _ = api
    opt = dict(emb_dim=din, pos_dim=0, ner_dim=0, input_dropout=0.0, gcn_dropout=0.0, emb_dropout=0.0, rnn=False, cuda=True, dataset="tacred",
               prune_k=1, hidden_dim=hidden, num_layers=layers, adj_type=adj_type, gcn_packed=True, **kw)
    demb = torch.nn.Embedding(85, table.shape[1], padding_idx=0)
    with torch.no_grad():
        demb.weight.copy_(torch.from_numpy(table))
    net = gcn.GCN(opt, (None, None, None, demb), hidden, layers)
    return net, demb


def _run_packed(net, demb, dev, g, trees):
    """h, mask and every gradient of GCN.forward(PackedTrees, inputs) with x as the (dense) word input."""
    net.to(dev).eval()
    demb.to(dev)
    T = g["head"].shape[1]
    x = to_dev(g["x"], dev).requires_grad_()
    masks = np.arange(T)[None, :] >= g["lens"][:, None]
    inputs = (x, to_dev(masks, dev), None, None, to_dev(g["deprel"], dev), to_dev(g["head"], dev), to_dev(g["subj_pos"], dev),
              to_dev(g["obj_pos"], dev))
    h, mask = net(trees, inputs)
    h.backward(to_dev(g["gy"], dev))
    f = lambda t: t.detach().float().cpu().numpy()  # noqa: E731
    dE = f(demb.weight.grad).copy() if demb.weight.grad is not None else np.zeros(tuple(demb.weight.shape), np.float32)
    dE[0] = 0                                   # nn.Embedding(padding_idx=0): the model's hook does this (checked end to end below)
    lin = net.W if hasattr(net, "W") else net.preprocessor
    return dict(h=f(h), mask=mask.cpu().numpy(), dx=f(x.grad), dW=f(lin.weight.grad), db=f(lin.bias.grad), dE=dE)


@functools.lru_cache(maxsize=None)
def _full_golden():
    from oracle import gcn_ref
    g = dict(load_golden("layers_full_deprel.npz"))
    B, T = int(g["B"]), int(g["T"])
    g["adj"] = dense_from_coo(g["coo"], B, T)
    g["cases"] = json.loads(str(g["cases"]))
    pad = np.arange(T)[None, :] >= g["lens"][:, None]
    assert pad.any() and np.abs(g["gy"][pad]).max() > 0
    g["pad"] = pad
    for ci, c in enumerate(g["cases"]):                     # what the pad slots' gy put into the recorded gradients (module docstring)
        g["fix%d" % ci] = gcn_ref.full_backward(g["adj"], g["x"], g["deprel"], g["W"], g["b"], g["E"], c["layers"], g["gy"] * pad[..., None],
                                                max_depth=c["deprel_max_depth"], directed=c["deprel_directed"], self_loop=c["deprel_self_loop"])
    return g


@pytest.mark.parametrize("source", ["pruner", "cache"])
@pytest.mark.parametrize("ci", [0, 1, 2, 3])
def test_full_deprel_golden_on_packed_trees(api, dev, ci, source):
    """layers_full_deprel.npz's four option sets at test_full_deprel_golden's bars (h 1e-4, gradients 2e-4 * max(1, |ref|max))."""
    gcn, tree = api
    g = _full_golden()
    c = g["cases"][ci]
    net, demb = _deprel_gcn(api, dev, "full_deprel", int(g["hidden"]), int(g["hidden"]), c["layers"], g["E"], deprel_emb_dim=int(g["D"]),
                            deprel_max_depth=c["deprel_max_depth"], deprel_directed=c["deprel_directed"], deprel_self_loop=c["deprel_self_loop"])
    with torch.no_grad():
        net.W.weight.copy_(torch.from_numpy(g["W"]))
        net.W.bias.copy_(torch.from_numpy(g["b"]))
    trees = _packed_trees(tree, dev, g, source, g["lens"], int(g["prune_k"]), extra=3 if source == "cache" else 0)
    r = _run_packed(net, demb, dev, g, trees)
    pad = g["pad"]
    np.testing.assert_array_equal(r["mask"], g["mask%d" % ci])
    assert not r["h"][pad].any() and not r["dx"][pad].any()
    err = max_rel(r["h"][~pad], g["h%d" % ci][~pad])
    print("full_deprel packed case %d (%s): h %.2e" % (ci, source, err))
    assert err <= 1e-4, (ci, source)
    for key, fix in zip(("dx", "dW", "db", "dE"), g["fix%d" % ci]):
        ref = g["%s%d" % (key, ci)] - fix
        err = np.abs(r[key] - ref).max()
        print("   %s %.2e (bar %.2e)" % (key, err, 2e-4 * max(1.0, np.abs(ref).max())))
        assert err <= 2e-4 * max(1.0, np.abs(ref).max()), (key, ci, source)


def test_full_deprel_bf16_on_packed_trees_vs_oracle(api, dev):
    """gcn_dtype='bf16' on packed trees at test_full_deprel_bf16_backward_vs_oracle's bars (its batch and parameters): forward 3e-2,
    gradients normwise 1e-1 against the fp32 oracle, whose gy is zero in the pad slots here."""
    from oracle import gcn_ref, prune_ref
    gcn, tree = api
    B, T, hidden, D, K, L = 12, 70, 64, 16, 1, 2
    tb = synthetic.random_tree_batch(93, B, T, "tacred")
    adj = prune_ref.batch_adj(tb["head"], tb["subj_pos"], tb["obj_pos"], tb["deprel"], tb["lens"], K)["adj"]
    rng = np.random.RandomState(7)
    pad = ~_real_slots(tb, T)
    g = dict(tb, x=synthetic.normal(8, (B, T, hidden)), gy=synthetic.normal(9, (B, T, hidden)) * ~pad[..., None],
             E=rng.uniform(-1, 1, size=(85, D)).astype(np.float32),
             W=(rng.uniform(-1, 1, size=(D * hidden, hidden)) / np.sqrt(hidden * D)).astype(np.float32),
             b=(rng.uniform(-1, 1, size=(D * hidden,)) / np.sqrt(hidden)).astype(np.float32))
    net, demb = _deprel_gcn(api, dev, "full_deprel", hidden, hidden, L, g["E"], deprel_emb_dim=D, deprel_max_depth=2, deprel_directed=False,
                            deprel_self_loop=True, gcn_dtype="bf16")
    with torch.no_grad():
        net.W.weight.copy_(torch.from_numpy(g["W"]))
        net.W.bias.copy_(torch.from_numpy(g["b"]))
    r = _run_packed(net, demb, dev, g, _packed_trees(tree, dev, g, "pruner", tb["lens"], K))
    kw = dict(max_depth=2, directed=False, self_loop=True)
    href, _ = gcn_ref.full_forward(adj, g["x"], g["deprel"], g["W"], g["b"], g["E"], L, **kw)
    want = gcn_ref.full_backward(adj, g["x"], g["deprel"], g["W"], g["b"], g["E"], L, g["gy"], **kw)
    assert not r["h"][pad].any() and max_rel(r["h"][~pad], href[~pad]) <= 3e-2
    dx = want[0] * ~pad[..., None]              # (the oracle's pad rows pass their -- zero -- dz on; dx of a pad slot is zero either way)
    for key, ref in zip(("dx", "dW", "db", "dE"), (dx,) + tuple(want[1:])):
        err = fro_rel(r[key], ref)
        print("full_deprel packed bf16 %s fro %.2e" % (key, err))
        assert err <= BF16_FRO, key


@pytest.mark.parametrize("source", ["pruner", "cache"])
def test_diag_deprel_golden_on_packed_trees(api, dev, source):
    """layers_diag_deprel.npz at test_diag_deprel_golden's bars: forward 1e-5, gradients 1e-4 (normwise)."""
    from oracle import gcn_ref
    gcn, tree = api
    g = dict(load_golden("layers_diag_deprel.npz"))
    B, T, L = int(g["B"]), int(g["T"]), int(g["layers"])
    net, demb = _deprel_gcn(api, dev, "diagonal_deprel", int(g["din"]), int(g["hidden"]), L, g["E"])
    with torch.no_grad():
        net.preprocessor.weight.copy_(torch.from_numpy(g["Wp"]))
        net.preprocessor.bias.copy_(torch.from_numpy(g["bp"]))
    trees = _packed_trees(tree, dev, g, source, g["lens"], int(g["prune_k"]), extra=3 if source == "cache" else 0)
    r = _run_packed(net, demb, dev, g, trees)
    pad = np.arange(T)[None, :] >= g["lens"][:, None]
    assert pad.any() and np.abs(g["gy"][pad]).max() > 0
    fix = gcn_ref.diag_backward(dense_from_coo(g["coo"], B, T), g["x"], g["deprel"], g["Wp"], g["bp"], g["E"], L, g["gy"] * pad[..., None])
    np.testing.assert_array_equal(r["mask"], g["mask"])
    assert not r["h"][pad].any() and not r["dx"][pad].any()
    err = max_rel(r["h"][~pad], g["h"][~pad])
    print("diagonal_deprel packed (%s): h %.2e" % (source, err))
    assert err <= FWD_RTOL
    for key, rec, f in zip(("dx", "dW", "db", "dE"), ("dx", "dWp", "dbp", "dE"), fix):
        err = max_rel(r[key], g[rec] - f)
        print("   %s %.2e" % (rec, err))
        assert err <= GRAD_RTOL, rec


def test_packed_deprel_forward_says_what_the_trees_lack(api, dev):
    gcn, tree = api
    g = _full_golden()
    for adj_type, kw in (("full_deprel", dict(want_label=False)), ("diagonal_deprel", dict(want_label=False)),
                         ("diagonal_deprel", dict(want_label=True, want_transpose=False))):
        net, demb = _deprel_gcn(api, dev, adj_type, int(g["hidden"]), int(g["hidden"]), 1, np.zeros((85, int(g["hidden"])), np.float32),
                                deprel_emb_dim=int(g["D"]))
        trees = tree.prune_to_csr_packed(*(to_dev(g[k], dev) for k in ("head", "subj_pos", "obj_pos", "deprel")), 1,
                                         [int(v) for v in g["lens"]], **kw)
        with pytest.raises(ValueError, match="want_label=True" if not kw["want_label"] else "want_transpose=True"):
            _run_packed(net, demb, dev, g, trees)


# ---------------------------------------------------------------------------------------------------
# 6. end to end
# ---------------------------------------------------------------------------------------------------
def _classifier(gcn, g, dev, **kw):
    opt = dict(json.loads(str(g["opt"])), cuda=True, **kw)
    m = gcn.GCNClassifier(opt)
    m.load_state_dict({k[3:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("sd:")}, strict=True)
    return m.to(dev)


@pytest.mark.parametrize("tag", ["full", "diag"])
def test_classifier_packed_deprel_matches_golden_logits(api, dev, tag):
    gcn, tree = api
    g = load_golden("e2e_%s.npz" % tag)
    inputs = tuple(to_dev(g[k], dev) for k in ("words", "masks", "pos", "ner", "deprel", "head", "subj_pos", "obj_pos"))
    model = _classifier(gcn, g, dev, gcn_packed=True).eval()
    head, subj, obj, dep, masks = (inputs[k] for k in (5, 6, 7, 4, 1))
    lens = (~masks.bool()).sum(1).to(torch.int32)
    cache = tree.TreeCache.build(head, subj, obj, dep, model.opt["prune_k"], lens=lens, want_label=True)
    ids = torch.arange(head.shape[0], device=dev)
    batch = lambda: cache.batch_packed(ids, head.shape[1], n_rows=int(lens.sum()))  # noqa: E731
    with torch.no_grad():
        logits, pooled = model(inputs)                                   # the model prunes straight into the packed layout
        logits_c, pooled_c = model(inputs, trees=batch())                # the loader-side form: a ValueError without the feature
        native, _ = _classifier(gcn, g, dev, gcn_packed=True, gcn_native_embed=True).eval()(inputs, trees=batch())
    for lg, pl in ((logits, pooled), (logits_c, pooled_c)):
        assert max_rel(lg.cpu().numpy(), g["logits"]) <= 1e-4
        assert max_rel(pl.cpu().numpy(), g["pooling_output"]) <= 1e-4
    # the native front end hands the layers the same packed rows bit for bit (tests/test_gpu_embed.py's bar for eval)
    assert torch.equal(native, logits_c)
    model.train()
    lg, pl = model(inputs, trees=batch())
    (lg.logsumexp(1).mean() + 0.003 * (pl ** 2).sum(1).mean()).backward()
    table = model.get_deprel_emb()
    assert torch.isfinite(table.grad).all() and table.grad.abs().sum() > 0 and (table.grad[0] == 0).all()
    assert all(torch.isfinite(q.grad).all() for q in model.parameters() if q.grad is not None)
    # gcn_pooled_only keeps precedence over gcn_packed, as on the regular path
    with torch.no_grad():
        lp, _ = _classifier(gcn, g, dev, gcn_packed=True, gcn_pooled_only=True).eval()(inputs)
    assert max_rel(lp.cpu().numpy(), g["logits"]) <= 1e-4


# ---------------------------------------------------------------------------------------------------
# 7. no host sync: one full_deprel training step on packed trees is a hipGraph
# ---------------------------------------------------------------------------------------------------
def test_full_deprel_packed_step_graph_capture(api, dev):
    """gcn_packed + gcn_check_trees=False + trees from batch_packed(n_rows=<host sum>): nothing in a full_deprel forward and backward
    reads the device, so torch.cuda.graph captures it (a host sync inside a capture is an error); the replay gives the eager step's
    numbers at the golden tolerances, with the layer dropout on the graph-safe counter."""
    gcn, tree = api
    g = load_golden("e2e_full.npz")
    model = _classifier(gcn, g, dev, gcn_packed=True, gcn_check_trees=False, gcn_graph_rng=True, input_dropout=0.0, emb_dropout=0.0,
                        word_dropout=0.0, gcn_dropout=0.5).train()
    inputs = tuple(to_dev(g[k], dev) for k in ("words", "masks", "pos", "ner", "deprel", "head", "subj_pos", "obj_pos"))
    head, subj, obj, dep, masks = (inputs[k] for k in (5, 6, 7, 4, 1))
    B, T = head.shape
    n_rows = int((g["masks"] == 0).sum())                                # the loader knows it: no device read
    cache = tree.TreeCache.build(head, subj, obj, dep, model.opt["prune_k"], lens=(~masks.bool()).sum(1).to(torch.int32), want_label=True)
    ids = torch.arange(B, device=dev)
    labels = torch.arange(B, device=dev) % 42

    def step():
        model.zero_grad(set_to_none=True)
        logits, pooled = model(inputs, trees=cache.batch_packed(ids, T, n_rows=n_rows))
        loss = torch.nn.functional.cross_entropy(logits, labels) + 0.003 * (pooled ** 2).sum(1).mean()
        loss.backward()
        return loss.detach(), logits.detach()

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
        loss, logits = step()
    W, table = model.gcn_model.gcn.W.weight, model.get_deprel_emb()
    counter.fill_(100)
    graph.replay()
    l1, lg1, gW, gE = float(loss), logits.clone(), W.grad.clone(), table.grad.clone()
    graph.replay()
    assert int(counter) == 102 and float(loss) != l1                     # the dropout mask moved on
    counter.fill_(100)
    le, lge = step()                                                     # eager, same counter value: same masks
    assert abs(float(le) - l1) <= 1e-4 * abs(l1)
    assert max_rel(lg1.cpu().numpy(), lge.cpu().numpy()) <= 1e-4
    for a, b in ((gW, W.grad), (gE, table.grad)):
        a, b = a.cpu().numpy(), b.cpu().numpy()
        assert np.isfinite(a).all() and np.abs(a).max() > 0 and np.abs(a - b).max() <= 2e-4 * max(1.0, np.abs(b).max())
