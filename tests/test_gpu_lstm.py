"""The native BiLSTM recurrence on the MI355X (csrc/lstm_kernels.hip through model/rnn.py and opt['gcn_native_rnn']):
against torch.nn.LSTM over pack_padded_sequence on the CPU, against the reference's recorded C-GCN outputs, as part of a captured
hipGraph training step, and without a host sync."""
import copy
import json

import numpy as np
import pytest
import torch

from conftest import load_golden
from helpers import max_rel

pytestmark = pytest.mark.gpu

E2E_KEYS = ("words", "masks", "pos", "ner", "deprel", "head", "subj_pos", "obj_pos")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu-marked tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def mods():
    from gcn_over_pruned_trees_amd import _lib
    from gcn_over_pruned_trees_amd.model import gcn, rnn
    _lib.lib()          # fails loudly when libgcnpt.so was not built
    return _lib, gcn, rnn


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _ragged_lens(B, T, seed):
    rng = np.random.RandomState(seed)
    lens = rng.randint(1, T + 1, size=B)
    lens[0], lens[-1] = T, 1
    if B > 2:
        lens[1] = max(1, T // 2)
    return lens


def _torch_bilstm(m, x, lens, dy):
    """The reference's encode_with_rnn on the CPU: pack, zero state, LSTM, pad back to T."""
    x = x.clone().requires_grad_()
    packed = torch.nn.utils.rnn.pack_padded_sequence(x, torch.as_tensor(lens), batch_first=True, enforce_sorted=False)
    out, _ = m(packed)
    out, _ = torch.nn.utils.rnn.pad_packed_sequence(out, batch_first=True, total_length=x.shape[1])
    out.backward(dy)
    return out.detach(), x.grad, {n: p.grad.clone() for n, p in m.named_parameters()}


@pytest.mark.parametrize("B,T,Din,H,layers", [(3, 7, 5, 1, 1), (10, 60, 24, 16, 1), (50, 100, 360, 200, 1), (10, 60, 24, 16, 2),
                                              (5, 9, 7, 19, 2)])
def test_bilstm_matches_torch_cpu(mods, dev, B, T, Din, H, layers):
    _lib, _, rnn = mods
    torch.manual_seed(1000 + B + H)
    m = torch.nn.LSTM(Din, H, layers, batch_first=True, bidirectional=True, dropout=0.0)
    lens = _ragged_lens(B, T, B * T + H)
    x = torch.randn(B, T, Din)
    dy = torch.randn(B, T, 2 * H)
    want_y, want_dx, want_g = _torch_bilstm(m, x, lens, dy)

    md = copy.deepcopy(m).to(dev)
    xd = x.to(dev).requires_grad_()
    y = rnn.bilstm(xd, _t(lens.astype(np.int32), dev), md, True)
    y.backward(dy.to(dev))
    torch.cuda.synchronize()
    y = y.detach().cpu()
    assert y.shape == (B, T, 2 * H)
    assert max_rel(y.numpy(), want_y.numpy()) <= 2e-5
    pad = torch.arange(T)[None, :] >= torch.as_tensor(lens)[:, None]
    assert pad.any() and torch.count_nonzero(y[pad]) == 0                  # padding rows are exactly 0, both directions
    assert max_rel(xd.grad.cpu().numpy(), want_dx.numpy()) <= 1e-4
    got_g = {n: p.grad.cpu() for n, p in md.named_parameters()}
    assert set(got_g) == set(want_g) and len(got_g) == 8 * layers
    for n in want_g:
        assert max_rel(got_g[n].numpy(), want_g[n].numpy()) <= 1e-4, n


def _golden_model(gcn, g, dev, **extra):
    opt = dict(json.loads(str(g["opt"])), cuda=True, **extra)
    model = gcn.GCNClassifier(opt)
    model.load_state_dict({k[3:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("sd:")}, strict=True)
    return model.to(dev)


def _forbid_torch_lstm(model):
    def hook(*_):
        raise AssertionError("nn.LSTM.forward ran: the native recurrence was not used")
    return model.gcn_model.gcn.rnn.register_forward_pre_hook(hook)


def test_cgcn_golden_native_rnn(mods, dev):
    """GCNClassifier with opt['gcn_native_rnn'] gives the reference's recorded C-GCN logits, and in training mode the gradients of the
    option-off model (whose BiLSTM is torch's) for every parameter."""
    _, gcn, _ = mods
    g = load_golden("e2e_cgcn.npz")
    inputs = tuple(_t(g[k], dev) for k in E2E_KEYS)
    model = _golden_model(gcn, g, dev, gcn_native_rnn=True).eval()
    handle = _forbid_torch_lstm(model)
    logits, pooled = model(inputs)
    assert max_rel(logits.detach().cpu().numpy(), g["logits"]) <= 1e-4
    assert max_rel(pooled.detach().cpu().numpy(), g["pooling_output"]) <= 1e-4

    quiet = dict(input_dropout=0.0, gcn_dropout=0.0, rnn_dropout=0.0, emb_dropout=0.0)
    loss = lambda lo, po: lo.logsumexp(1).mean() + 0.003 * (po ** 2).sum(1).mean()      # noqa: E731
    grads = []
    for native in (True, False):
        torch.manual_seed(5)
        m = _golden_model(gcn, g, dev, gcn_native_rnn=native, **quiet).train()
        h = _forbid_torch_lstm(m) if native else None
        lo, po = m(inputs)
        loss(lo, po).backward()
        grads.append({n: p.grad.detach().cpu().numpy() for n, p in m.named_parameters() if p.grad is not None})
        if h is not None:
            h.remove()
    got, want = grads
    assert set(got) == set(want) and sum("rnn." in n for n in want) == 8
    for n in want:
        assert max_rel(got[n], want[n]) <= 1e-4, n
    handle.remove()


def test_cgcn_training_step_graph_capture(mods, dev):
    """The whole C-GCN training step (tree build, BiLSTM, layers, pooling, MLP, loss, backward) captured as ONE hipGraph replays to the
    eager step bit for bit.  The torch path cannot be captured (pack_padded_sequence wants the lengths on the host)."""
    _lib, gcn, _ = mods
    g = load_golden("e2e_cgcn.npz")
    inputs = tuple(_t(g[k], dev) for k in E2E_KEYS)
    labels = torch.arange(inputs[0].shape[0], device=dev) % 42
    model = _golden_model(gcn, g, dev, gcn_native_rnn=True, gcn_check_trees=False, gcn_graph_rng=True, input_dropout=0.0,
                          gcn_dropout=0.0, rnn_dropout=0.0, emb_dropout=0.0, word_dropout=0.0).train()
    _forbid_torch_lstm(model)
    # one summation order for the GCN weight gradients; the embedding tables' gradients are float-atomic index_add_ sums (any order)
    old = _lib.set_option(_lib.OPT_DETERMINISTIC, 1)
    try:
        def step():
            model.zero_grad(set_to_none=False)
            logits, pooled = model(inputs)
            loss = torch.nn.functional.cross_entropy(logits, labels) + 0.003 * (pooled ** 2).sum(1).mean()
            loss.backward()
            return logits.detach()

        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(3):
                step()
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, capture_error_mode="thread_local"):
            static_logits = step()
        graph.replay()
        torch.cuda.synchronize()
        got_logits = static_logits.clone()
        got = {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}
        eager_logits = step()
        torch.cuda.synchronize()
    finally:
        _lib.set_option(_lib.OPT_DETERMINISTIC, old)
    assert torch.equal(got_logits, eager_logits)
    emb = ("gcn_model.emb.weight", "gcn_model.pos_emb.weight", "gcn_model.ner_emb.weight")
    assert set(got) == {n for n, p in model.named_parameters() if p.grad is not None}
    assert sum(".rnn." in n for n in got) == 8 and all(n in got for n in emb)
    for n, p in model.named_parameters():
        if n not in got:
            continue
        assert torch.isfinite(got[n]).all(), n
        if n in emb:
            assert max_rel(got[n].cpu().numpy(), p.grad.cpu().numpy()) <= 1e-6, n
        else:
            assert torch.equal(got[n], p.grad), n


def test_native_rnn_forward_has_no_host_sync(mods, dev):
    """encode_with_rnn with the option issues no device-to-host copy or sync (forward and backward); the torch path does."""
    _, gcn, _ = mods
    g = load_golden("e2e_cgcn.npz")
    masks = _t(g["masks"], dev)
    B, T = masks.shape
    native = _golden_model(gcn, g, dev, gcn_native_rnn=True).train().gcn_model.gcn
    plain = _golden_model(gcn, g, dev).train().gcn_model.gcn
    x = torch.randn(B, T, native.rnn.input_size, device=dev, requires_grad=True)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = native.encode_with_rnn(x, masks, B)
        out.backward(torch.ones_like(out))
        with pytest.raises(RuntimeError):
            plain.encode_with_rnn(x, masks, B)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert out.shape == (B, T, 2 * native.rnn.hidden_size) and torch.isfinite(x.grad).all()
