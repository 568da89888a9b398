"""GPU tests of the native output head (csrc/head_kernels.hip, model.gcn.linear_act / head_loss / head_predict, opt['gcn_native_head']).
Reference: the same computation in torch float64 on the CPU from the same float32 inputs; where ReLU is on, the reference gradient uses the
device's own Y for the mask.  Tolerances are the project's (helpers.FWD_RTOL / GRAD_RTOL, max_rel): a plain float32 torch
implementation stays below 5e-7 forward and 1e-6 on gradients against float64 at these shapes."""
import json

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden
from helpers import FWD_RTOL, GRAD_RTOL, cuda_dev, gcn_api, max_rel, options, to_dev
from gcn_over_pruned_trees_amd import _lib
from gcn_over_pruned_trees_amd.utils import synthetic

pytestmark = pytest.mark.gpu

POISON = -7.25e4                     # never produced by the cases below
PAD = 64                             # floats of poisoned guard band before and after every output


@pytest.fixture(scope="module")
def dev():
    return cuda_dev()


@pytest.fixture(scope="module")
def api():
    return gcn_api()


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and bool((a.contiguous().view(torch.int32) == b.contiguous().view(torch.int32)).all())


# ---- the linear kernels -------------------------------------------------------------------------------------------------------------
LINEAR_SHAPES = [(1, 4, 1), (15, 37, 17), (16, 600, 200), (17, 200, 42), (50, 600, 200), (130, 1084, 300)]


def _linear_case(M, K, N, seed=0):
    x = synthetic.normal(100 + seed, (M, K))
    w = (synthetic.normal(101 + seed, (N, K)) / np.sqrt(K)).astype(np.float32)
    b = synthetic.normal(102 + seed, (N,))
    gy = synthetic.normal(103 + seed, (M, N))
    return x, w, b, gy


def _linear_ref(x, w, b, gy, relu, y_dev):
    """float64 forward and gradients; the ReLU mask is the device's own Y > 0."""
    x, w, b, gy = (a.astype(np.float64) for a in (x, w, b, gy))
    y = x @ w.T + b
    if relu:
        y = np.maximum(y, 0.0)
    dz = gy * (y_dev > 0) if relu else gy
    return y, dz @ w, dz.T @ x, dz.sum(0)


@pytest.mark.parametrize("relu", [False, True], ids=["identity", "relu"])
@pytest.mark.parametrize("shape", LINEAR_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_linear_act_matches_float64(api, dev, shape, relu):
    gcn, _ = api
    M, K, N = shape
    x, w, b, gy = _linear_case(M, K, N)
    xt, wt, bt = (to_dev(a, dev).requires_grad_() for a in (x, w, b))
    y = gcn.linear_act(xt, wt, bt, relu=relu)
    assert y.shape == (M, N) and y.dtype == torch.float32 and y.is_contiguous()
    y.backward(to_dev(gy, dev))
    y_dev = y.detach().cpu().numpy()
    want = _linear_ref(x, w, b, gy, relu, y_dev)
    errs = [max_rel(y_dev, want[0])] + [max_rel(g.grad.cpu().numpy(), r) for g, r in zip((xt, wt, bt), want[1:])]
    print(shape, relu, "fwd %.2e dx %.2e dW %.2e db %.2e" % tuple(errs))
    assert errs[0] <= FWD_RTOL and max(errs[1:]) <= GRAD_RTOL, errs
    if relu:
        assert float(y.min()) >= 0.0


def test_linear_act_reads_a_column_slice_in_place_and_skips_dx(api, dev):
    gcn, _ = api
    M, K, N = 50, 200, 200
    x, w, b, gy = _linear_case(M, K, N, seed=10)
    wide = synthetic.normal(7, (M, 3 * K))
    wide[:, K:2 * K] = x                                          # the middle third: ldx = 3K, base not at the buffer's start
    leaf = to_dev(wide, dev).requires_grad_()
    wt, bt = (to_dev(a, dev).requires_grad_() for a in (w, b))
    view = leaf[:, K:2 * K]
    assert not view.is_contiguous()
    y = gcn.linear_act(view, wt, bt, relu=True)
    y.backward(to_dev(gy, dev))
    y_dev = y.detach().cpu().numpy()
    want = _linear_ref(x, w, b, gy, True, y_dev)
    g = leaf.grad.cpu().numpy()
    assert max_rel(y_dev, want[0]) <= FWD_RTOL
    assert max_rel(g[:, K:2 * K], want[1]) <= GRAD_RTOL and not g[:, :K].any() and not g[:, 2 * K:].any()
    assert max_rel(wt.grad.cpu().numpy(), want[2]) <= GRAD_RTOL and max_rel(bt.grad.cpu().numpy(), want[3]) <= GRAD_RTOL
    # x without a gradient: dW and db alone (the dX tiles are not launched), same values
    w2, b2 = (to_dev(a, dev).requires_grad_() for a in (w, b))
    y2 = gcn.linear_act(to_dev(x, dev), w2, b2, relu=True)
    y2.backward(to_dev(gy, dev))
    assert _same_bits(y2.detach(), y.detach()) and _same_bits(w2.grad, wt.grad) and _same_bits(b2.grad, bt.grad)


def _guarded(dev, n):
    """(buffer, pointer of its payload): n floats between two poisoned guard bands."""
    buf = torch.full((n + 2 * PAD,), POISON, dtype=torch.float32, device=dev)
    return buf, buf.data_ptr() + 4 * PAD


def _guards_intact(buf, n):
    return bool((buf[:PAD] == POISON).all()) and bool((buf[PAD + n:] == POISON).all())


@pytest.mark.parametrize("shape", [(1, 4, 1), (15, 37, 17), (17, 200, 42), (50, 600, 200)], ids=lambda s: "x".join(map(str, s)))
def test_linear_kernels_write_nothing_outside_their_outputs_and_repeat_bit_for_bit(dev, shape):
    L, st = _lib.lib(), _lib.stream()
    M, K, N = shape
    x, w, b, gy = _linear_case(M, K, N, seed=20)
    xt, wt, bt, gt = (to_dev(a, dev) for a in (x, w, b, gy))
    ybuf, yp = _guarded(dev, M * N)
    _lib.check(L.gcnpt_head_linear_fwd(st, xt.data_ptr(), K, wt.data_ptr(), bt.data_ptr(), yp, M, K, N, 1))
    y = ybuf[PAD:PAD + M * N].view(M, N)
    assert _guards_intact(ybuf, M * N) and not bool((y == POISON).any())
    ld = K + 5                                                    # dX rows with a gap the launch must leave alone
    outs = []
    for _ in range(2):
        dxbuf, dxp = _guarded(dev, M * ld)
        dwbuf, dwp = _guarded(dev, N * K)
        dbbuf, dbp = _guarded(dev, N)
        _lib.check(L.gcnpt_head_linear_bwd(st, gt.data_ptr(), yp, xt.data_ptr(), K, wt.data_ptr(), dxp, ld, dwp, dbp, M, K, N, 1))
        dx = dxbuf[PAD:PAD + M * ld].view(M, ld)
        assert _guards_intact(dxbuf, M * ld) and _guards_intact(dwbuf, N * K) and _guards_intact(dbbuf, N)
        assert bool((dx[:, K:] == POISON).all()) and not bool((dx[:, :K] == POISON).any())
        assert not bool((dwbuf[PAD:PAD + N * K] == POISON).any()) and not bool((dbbuf[PAD:PAD + N] == POISON).any())
        outs.append((dx[:, :K].clone(), dwbuf[PAD:PAD + N * K].clone(), dbbuf[PAD:PAD + N].clone()))
    for a, c in zip(*outs):
        assert _same_bits(a, c)                                   # no atomics: the same bits run to run
    want = _linear_ref(x, w, b, gy, True, y.cpu().numpy())
    assert max_rel(outs[0][0].cpu().numpy(), want[1]) <= GRAD_RTOL
    assert max_rel(outs[0][1].view(N, K).cpu().numpy(), want[2]) <= GRAD_RTOL


# ---- the loss kernels ---------------------------------------------------------------------------------------------------------------
# (300, 42, 200): more rows than the forward's 16 waves take in one pass; (9, 130, 70): C and H above one 64-lane pass
LOSS_SHAPES = [(1, 42, 200), (17, 5, 8), (50, 42, 200), (64, 19, 16), (300, 42, 200), (9, 130, 70)]


def _loss_case(M, C, H, seed=0):
    z = synthetic.normal(200 + seed, (M, C)) * np.float32(3.0)
    z[M // 2] += np.float32(1e4)                                  # a naive softmax overflows on this row
    pooled = synthetic.normal(201 + seed, (M, 3 * H))
    labels = (np.arange(M) * 7 + 3) % C
    return z.astype(np.float32), pooled, labels.astype(np.int64)


def _loss_ref(z, pooled, labels, H, l2, scale):
    z64 = torch.from_numpy(z.astype(np.float64)).requires_grad_()
    p64 = torch.from_numpy(pooled.astype(np.float64)).requires_grad_()
    loss = F.cross_entropy(z64, torch.from_numpy(labels))
    if l2 > 0:
        loss = loss + l2 * (p64[:, :H] ** 2).sum(1).mean()
    (scale * loss).backward()
    return float(loss), z64.grad.numpy(), (p64.grad.numpy() if p64.grad is not None else np.zeros_like(pooled, dtype=np.float64))


@pytest.mark.parametrize("l2", [0.0, 0.003], ids=["ce_only", "with_l2"])
@pytest.mark.parametrize("shape", LOSS_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_head_loss_matches_float64(api, dev, shape, l2):
    gcn, _ = api
    M, C, H = shape
    z, pooled, labels = _loss_case(M, C, H)
    zt, pt = to_dev(z, dev).requires_grad_(), to_dev(pooled, dev).requires_grad_()
    view = pt[:, :H]                                              # the strided view the model returns
    assert view.is_contiguous() == (M == 1)
    status = torch.full((1,), 77, dtype=torch.int32, device=dev)
    loss = gcn.head_loss(zt, to_dev(labels, dev), view, l2, status=status)
    assert loss.dim() == 0 and loss.dtype == torch.float32 and int(status.item()) == 0
    (3 * loss).backward()                                         # dloss = 3, read from the device
    want = _loss_ref(z, pooled, labels, H, l2, 3.0)
    e_loss = abs(float(loss) - want[0]) / abs(want[0])
    e_dz = max_rel(zt.grad.cpu().numpy(), want[1])
    print(shape, l2, "loss %.2e dlogits %.2e" % (e_loss, e_dz))
    assert e_loss <= FWD_RTOL and e_dz <= GRAD_RTOL
    if l2 > 0:
        e_dp = max_rel(pt.grad.cpu().numpy(), want[2])
        print("dpooled %.2e" % e_dp)
        assert e_dp <= GRAD_RTOL and not bool(pt.grad[:, H:].any())
    else:
        assert pt.grad is None or not bool(pt.grad.any())
    # the same bits run to run (fixed summation order)
    z2 = to_dev(z, dev).requires_grad_()
    loss2 = gcn.head_loss(z2, to_dev(labels, dev), to_dev(pooled, dev)[:, :H], l2)
    (3 * loss2).backward()
    assert _same_bits(loss2.detach(), loss.detach()) and _same_bits(z2.grad, zt.grad)


@pytest.mark.parametrize("shape", LOSS_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_head_predict_probs_and_argmax(api, dev, shape):
    gcn, _ = api
    M, C, H = shape
    z, _, _ = _loss_case(M, C, H, seed=5)
    if C > 8:                                                     # exact ties: the maximum twice in a row, and again past lane 63
        z[0, 3] = z[0, 7] = z[0].max() + 1
        if C > 70:
            z[1, 5] = z[1, 70] = z[1].max() + 1
    zt = to_dev(z, dev)
    probs, pred = gcn.head_predict(zt)
    assert probs.shape == (M, C) and pred.shape == (M,) and pred.dtype == torch.int64
    want = torch.softmax(torch.from_numpy(z.astype(np.float64)), 1).numpy()
    assert max_rel(probs.cpu().numpy(), want) <= FWD_RTOL
    assert np.array_equal(pred.cpu().numpy(), np.argmax(zt.cpu().numpy(), axis=1))
    if C > 8:
        assert int(pred[0]) == 3
        if C > 70:
            assert int(pred[1]) == 5


SMALL_OPT = dict(vocab_size=50, emb_dim=8, pos_dim=2, ner_dim=2, hidden_dim=16, num_layers=2, input_dropout=0.0, gcn_dropout=0.0,
                 prune_k=1, pooling="max", mlp_layers=2, rnn=False, dataset="tacred", num_class=5, topn=1e10, cuda=True, pooling_l2=0.003)


@pytest.mark.parametrize("bad", [5, -1], ids=["label_C", "label_minus_1"])
def test_label_outside_the_classes(api, dev, bad):
    gcn, _ = api
    M, C, H = 17, 5, 16
    z, pooled, labels = _loss_case(M, C, H, seed=9)
    labels[4] = bad
    lt = to_dev(labels, dev)
    status = torch.zeros((1,), dtype=torch.int32, device=dev)
    loss = gcn.head_loss(to_dev(z, dev), lt, to_dev(pooled, dev)[:, :H], 0.003, status=status)
    assert int(status.item()) & 1 and bool(torch.isfinite(loss))
    checking = gcn.GCNClassifier(dict(SMALL_OPT, gcn_native_head=True)).to(dev)
    with pytest.raises(IndexError):
        checking.loss(to_dev(z, dev), to_dev(pooled, dev)[:, :H], lt)
    quiet = gcn.GCNClassifier(dict(SMALL_OPT, gcn_native_head=True, gcn_check_trees=False)).to(dev)
    zt, pt = to_dev(z, dev).requires_grad_(), to_dev(pooled, dev).requires_grad_()
    loss = quiet.loss(zt, pt[:, :H], lt)
    loss.backward()
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(zt.grad).all())
    assert not bool(zt.grad[4].any()) and bool(zt.grad[3].any())
    # the bad row contributes nothing; the mean is still over M rows
    keep = np.arange(M) != 4
    ref = _loss_ref(z[keep], pooled[keep], labels[keep], H, 0.0, 1.0)
    want = ref[0] * (M - 1) / M + 0.003 * float((pooled[:, :H].astype(np.float64) ** 2).sum(1).mean())
    assert abs(float(loss) - want) <= FWD_RTOL * abs(want)
    assert max_rel(zt.grad.cpu().numpy()[keep], ref[1] * (M - 1) / M) <= GRAD_RTOL


# ---- the modules --------------------------------------------------------------------------------------------------------------------
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


@pytest.mark.parametrize("tag", ["gcn", "semeval", "cgcn", "diag", "full"])
def test_module_reproduces_the_golden_logits(api, dev, tag):
    gcn, _ = api
    g = load_golden("e2e_%s.npz" % tag)
    inputs = _inputs(g, dev, json.loads(str(g["opt"])))
    with torch.no_grad():
        m = _model(gcn, g, dev, gcn_native_head=True).eval()
        logits, pooled = m(inputs)
        assert max_rel(logits.cpu().numpy(), g["logits"]) <= 1e-4
        assert max_rel(pooled.cpu().numpy(), g["pooling_output"]) <= 1e-4
        probs, pred = m.predict(logits)
    assert np.array_equal(pred.cpu().numpy(), np.argmax(logits.cpu().numpy(), axis=1))
    assert max_rel(probs.cpu().numpy(), torch.softmax(logits.double().cpu(), 1).numpy()) <= FWD_RTOL


def _step_grads(m, inputs, dev):
    logits, pooled = m(inputs)
    labels = torch.arange(logits.shape[0], device=dev) % logits.shape[1]
    loss = m.loss(logits, pooled, labels)
    loss.backward()
    return loss.detach(), {n: p.grad for n, p in m.named_parameters()}


def _assert_same_grads(got, want):
    assert got.keys() == want.keys()
    seen = 0
    for n in want:
        a, b = got[n], want[n]
        assert (a is None) == (b is None), n
        if a is None:
            continue
        seen += 1
        assert max_rel(a.cpu().numpy(), b.cpu().numpy()) <= GRAD_RTOL, n
    return seen


@pytest.mark.parametrize("variant", ["gcn", "gcn_packed", "gcn_pooled_only", "cgcn"])
def test_module_training_step_same_gradients(api, dev, variant):
    gcn, _ = api
    g = load_golden("e2e_%s.npz" % variant.split("_")[0])
    kw = dict(input_dropout=0.0, emb_dropout=0.0, word_dropout=0.0, gcn_dropout=0.0, rnn_dropout=0.0, pooling_l2=0.003)
    kw.update({"gcn_packed": dict(gcn_packed=True), "gcn_pooled_only": dict(gcn_pooled_only=True)}.get(variant, {}))
    inputs = _inputs(g, dev, json.loads(str(g["opt"])))
    l0, g0 = _step_grads(_model(gcn, g, dev, gcn_native_head=False, **kw).train(), inputs, dev)
    l1, g1 = _step_grads(_model(gcn, g, dev, gcn_native_head=True, **kw).train(), inputs, dev)
    assert abs(float(l1) - float(l0)) <= FWD_RTOL * abs(float(l0))
    assert _assert_same_grads(g1, g0) >= 8
    for n in ("classifier.weight", "classifier.bias", "gcn_model.out_mlp.0.weight", "gcn_model.out_mlp.0.bias"):
        assert g1[n] is not None and bool(g1[n].any()), n


@pytest.mark.parametrize("mlp_layers", [1, 3])
def test_module_mlp_depths_on_a_small_random_model(api, dev, mlp_layers):
    gcn, _ = api
    g = load_golden("e2e_gcn.npz")
    base = json.loads(str(g["opt"]))
    inputs = _inputs(g, dev, base)
    kw = dict(cuda=True, hidden_dim=24, mlp_layers=mlp_layers, input_dropout=0.0, emb_dropout=0.0, word_dropout=0.0, gcn_dropout=0.0,
              pooling_l2=0.003, conv_l2=0.01)
    torch.manual_seed(77)
    plain = gcn.GCNClassifier(dict(base, **kw)).to(dev).train()
    native = gcn.GCNClassifier(dict(base, gcn_native_head=True, **kw)).to(dev).train()
    native.load_state_dict(plain.state_dict(), strict=True)
    assert len([k for k in native.state_dict() if "out_mlp" in k]) == 2 * mlp_layers
    l0, g0 = _step_grads(plain, inputs, dev)
    l1, g1 = _step_grads(native, inputs, dev)
    assert abs(float(l1) - float(l0)) <= FWD_RTOL * abs(float(l0))
    assert _assert_same_grads(g1, g0) >= 6 + 2 * mlp_layers


# ---- graph capture ------------------------------------------------------------------------------------------------------------------
ATOMIC_SUMS = ("gcn_model.emb.weight", "gcn_model.pos_emb.weight", "gcn_model.ner_emb.weight", "gcn_model.deprel_emb.weight")


def test_training_step_graph_capture_with_native_head(api, dev):
    """The whole no-LSTM training step, loss included (model.loss: no host sync with gcn_check_trees=False), as ONE hipGraph.  Three
    replays give the eager step's loss and gradients bit for bit.  The embedding tables' gradients are the exception: torch's index_add_
    sums them with float atomics, whose order differs between two runs of the eager step itself (EXPERIMENTS.md, "Same bits"), so they are
    held to the 1e-5 the existing capture tests use; the layer weights are summed in the library's ordered form (OPT_DETERMINISTIC)."""
    gcn, _ = api
    e = load_golden("e2e_gcn.npz")
    model = _model(gcn, e, dev, gcn_native_head=True, gcn_check_trees=False, gcn_graph_rng=True, input_dropout=0.0, emb_dropout=0.0,
                   word_dropout=0.0, gcn_dropout=0.0, pooling_l2=0.003).train()
    inputs = _inputs(e, dev, json.loads(str(e["opt"])))
    labels = torch.arange(inputs[0].shape[0], device=dev) % 42

    def step():
        model.zero_grad(set_to_none=True)
        logits, pooled = model(inputs)
        loss = model.loss(logits, pooled, labels)
        loss.backward()
        return loss

    with options(DETERMINISTIC=1):
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(3):
                step()                                            # (results dropped: a kept autograd graph would pin its stream)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, capture_error_mode="thread_local"):
            loss = step()
        params = dict(model.named_parameters())
        replays = []
        for _ in range(3):
            graph.replay()
            torch.cuda.synchronize()
            replays.append((loss.detach().clone(), {n: p.grad.clone() for n, p in params.items() if p.grad is not None}))
        eager_loss = step().detach().clone()                      # the same step, launched eagerly
        eager = {n: p.grad.clone() for n, p in params.items() if p.grad is not None}
        assert len(eager) >= 10
        for got_loss, got in replays:
            assert _same_bits(got_loss, eager_loss)
            assert got.keys() == eager.keys()
            for n, want in eager.items():
                if n in ATOMIC_SUMS:
                    assert max_rel(got[n].cpu().numpy(), want.cpu().numpy()) <= 1e-5, n
                else:
                    assert _same_bits(got[n], want), n
