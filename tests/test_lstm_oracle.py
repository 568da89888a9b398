"""oracle/lstm_ref.py (the float64 checker of the native BiLSTM recurrence) against torch.nn.LSTM in double on the CPU over
pack_padded_sequence: outputs, dx, every parameter gradient and dL/dc0.  This is what makes the oracle trustworthy; the GPU tests in
tests/test_gpu_lstm_edges.py then measure the kernels against it."""
import numpy as np
import pytest
import torch

from oracle import lstm_ref


def _torch_double(m, x, lens, dy):
    """nn.LSTM in double over pack_padded_sequence from an explicit zero (h0, c0) that requires a gradient."""
    B, T, _ = x.shape
    H, L = m.hidden_size, m.num_layers
    x = x.clone().requires_grad_()
    h0 = torch.zeros(2 * L, B, H, dtype=torch.float64, requires_grad=True)
    c0 = torch.zeros(2 * L, B, H, dtype=torch.float64, requires_grad=True)
    packed = torch.nn.utils.rnn.pack_padded_sequence(x, torch.as_tensor(lens), batch_first=True, enforce_sorted=False)
    out, _ = m(packed, (h0, c0))
    out, _ = torch.nn.utils.rnn.pad_packed_sequence(out, batch_first=True, total_length=T)
    out.backward(dy)
    return out.detach().numpy(), x.grad.numpy(), {n: p.grad.numpy() for n, p in m.named_parameters()}, c0.grad.numpy()


def _rel(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


@pytest.mark.parametrize("B,T,Din,H,layers,bias,lens", [
    (1, 1, 3, 1, 1, True, [1]),
    (4, 9, 5, 7, 1, True, [3, 9, 1, 6]),
    (6, 12, 4, 17, 2, True, [12, 2, 7, 1, 12, 5]),
    (5, 8, 6, 9, 1, False, [8, 1, 4, 8, 3]),
    (3, 11, 4, 5, 2, False, [6, 11, 2]),
])
def test_lstm_oracle_matches_torch_double(B, T, Din, H, layers, bias, lens):
    torch.manual_seed(7 * B + H)
    m = torch.nn.LSTM(Din, H, layers, bias=bias, batch_first=True, bidirectional=True).double()
    with torch.no_grad():
        for p in m.parameters():
            p.uniform_(-0.6, 0.6)
    x = torch.randn(B, T, Din, dtype=torch.float64)
    dy = torch.randn(B, T, 2 * H, dtype=torch.float64)
    lens = np.asarray(lens)
    want_y, want_dx, want_g, want_dc0 = _torch_double(m, x, lens, dy)

    got = lstm_ref.bilstm_stack_ref(x.numpy(), lens, [lstm_ref.params_of(m, l) for l in range(layers)], dy.numpy())
    assert got["y"].dtype == np.float64
    assert _rel(got["y"], want_y.reshape(B * T, 2 * H)) <= 1e-12
    assert _rel(got["dx"], want_dx.reshape(B * T, Din)) <= 1e-12
    for l in range(layers):
        for d, sfx in enumerate(("", "_reverse")):
            assert _rel(got["dw_ih"][l][d], want_g["weight_ih_l%d%s" % (l, sfx)]) <= 1e-12, (l, d)
            assert _rel(got["dw_hh"][l][d], want_g["weight_hh_l%d%s" % (l, sfx)]) <= 1e-12, (l, d)
            if bias:
                assert _rel(got["db"][l][d], want_g["bias_ih_l%d%s" % (l, sfx)]) <= 1e-12, (l, d)
                assert _rel(got["db"][l][d], want_g["bias_hh_l%d%s" % (l, sfx)]) <= 1e-12, (l, d)
            # c0.grad rows are ordered layer-major, direction-minor (nn.LSTM's h0/c0 layout), in the caller's batch order
            assert _rel(got["dc0"][l][d], want_dc0[2 * l + d]) <= 1e-12, (l, d)
    assert sum(1 for _ in want_g) == (8 if bias else 4) * layers


def test_lstm_oracle_single_layer_layouts():
    """bilstm_ref exposes c, gates, h_prev and dgates in include/gcnpt.h's layouts: checked against the equations at a hand-picked
    row of each direction, padding rows and a sentence of length 0 (all zeros), and the float32 run stays float32."""
    rng = np.random.RandomState(3)
    B, T, Din, H = 3, 5, 4, 6
    params = tuple(tuple(rng.uniform(-0.5, 0.5, s) for s in ((4 * H, Din), (4 * H, H), (4 * H,), (4 * H,))) for _ in range(2))
    x, dy = rng.randn(B, T, Din), rng.randn(B, T, 2 * H)
    lens = np.array([5, 0, 3])
    r = lstm_ref.bilstm_ref(x, lens, params, dy)
    for k in ("y", "c", "h_prev", "dgates", "gates"):
        a = r[k].reshape(B, T, -1)
        assert not a[1].any(), k                                              # length 0: all zeros
        assert not a[2, 3:].any(), k                                          # padding rows of the sentence of length 3
    assert not r["dc0"][:, 1].any()
    sig = lambda v: 1 / (1 + np.exp(-v))                                      # noqa: E731
    # forward direction at t = 0 of sentence 0 (zero state), reverse direction at its first step t = len-1 = 2 of sentence 2
    for b, t, d in ((0, 0, 0), (2, 2, 1)):
        w_ih, _, b_ih, b_hh = params[d]
        pre = w_ih @ x[b, t] + b_ih + b_hh
        i, f, g, o = sig(pre[:H]), sig(pre[H:2 * H]), np.tanh(pre[2 * H:3 * H]), sig(pre[3 * H:])
        row = b * T + t
        assert np.allclose(r["gates"][row, d * 4 * H:(d + 1) * 4 * H], np.concatenate((i, f, g, o)), rtol=0, atol=1e-14)
        assert np.allclose(r["c"][row, d * H:(d + 1) * H], i * g, rtol=0, atol=1e-14)
        assert np.allclose(r["y"][row, d * H:(d + 1) * H], o * np.tanh(i * g), rtol=0, atol=1e-14)
        assert not r["h_prev"][row, d * H:(d + 1) * H].any()
    r32 = lstm_ref.bilstm_ref(x, lens, params, dy, dtype=np.float32)
    assert all(r32[k].dtype == np.float32 for k in ("y", "c", "gates", "h_prev", "dgates", "dx", "dw_ih", "dw_hh", "db", "dc0"))
    assert _rel(r32["y"], r["y"]) < 1e-5 and _rel(r32["dx"], r["dx"]) < 1e-4
