"""The native BiLSTM recurrence (csrc/lstm_kernels.hip: gcnpt_lstm_fwd / gcnpt_lstm_bwd, and model/rnn.py's bilstm around them) against
the float64 oracle of oracle/lstm_ref.py, at the shapes and edges tests/test_gpu_lstm.py does not reach: hidden sizes past one operand-load
trip (H > 256 forward, 4H > 1024 backward), sentences of length 0, B and H at the 16-wide tile boundaries, T = 1 and T = 300, saturated
gates, the inference branch, module variants, and a hipGraph capture.  The direct C-ABI tests fill every output with NaN first, so a row
the kernels do not write shows up whatever the allocator hands back, and they check c, the gates, h_prev, dG and dc0 directly.

Tolerance rule (assert_fp32_close): the kernels compute in fp32, so they are measured against the float64 oracle with the same oracle run
in float32 as the yardstick of honest fp32 rounding.  A result passes when its error against float64 is at most FP32_FACTOR times the
float32 oracle's own error plus a floor, and also within the absolute bars of test_gpu_lstm.py (2e-5 forward, 1e-4 gradients).  The floor is
FLOOR for what the kernels write (y, c, gates, h_prev, dG, dc) and GEMM_FLOOR for what model/rnn.py's library GEMMs reduce from dG
(dx over 8H columns; dW_ih, dW_hh and db over B*T rows): their summation order is not numpy's, and a long fp32 sum's rounding depends
on the order.  At B=50, T=300, H=200, numpy's blocked sgemm gives dW_hh to 3.9e-7 against float64 and a plain sequential fp32 sum of
the same 15000 products to 3.1e-6; GEMM_FLOOR covers the latter."""
import numpy as np
import pytest
import torch

from helpers import max_rel
from oracle import lstm_ref

pytestmark = pytest.mark.gpu

FP32_FACTOR = 4.0           # the kernels may be this many times as far from float64 as the float32 oracle is
FLOOR = 1e-6                # normwise, a few fp32 ulps: covers cases where the float32 oracle happens to round very well
GEMM_FLOOR = 4e-6           # the library-GEMM reductions (see the module docstring)
FWD_BAR, GRAD_BAR = 2e-5, 1e-4


def assert_fp32_close(name, got, ref64, ref32, bar, floor=FLOOR):
    """The tolerance rule of this file: max_rel(got, ref64) <= min(bar, FP32_FACTOR * max_rel(ref32, ref64) + floor)."""
    err, base = max_rel(got, ref64), max_rel(ref32, ref64)
    print("%-18s err %.2e  fp32 oracle %.2e  (%.1fx)" % (name, err, base, err / max(base, 1e-30)))
    assert err <= bar and err <= FP32_FACTOR * base + floor, "%s: error %.3e against float64; the float32 oracle's is %.3e, bar %.0e" % (
        name, err, base, bar)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu-marked tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def mods():
    from gcn_over_pruned_trees_amd import _lib
    from gcn_over_pruned_trees_amd.model import rnn
    _lib.lib()          # fails loudly when libgcnpt.so was not built
    return _lib, rnn


def _lens(B, T, seed):
    """Ragged, unsorted lengths in [0, T]; with B >= 3 they include 0, 1 and T at random positions."""
    rng = np.random.RandomState(seed)
    lens = rng.randint(0, T + 1, size=B)
    if B >= 3:
        lens[rng.permutation(B)[:3]] = (0, 1, T)
    elif B == 2:
        lens[:] = (1, T)
    else:
        lens[:] = T
    return lens


def _case(B, T, Din, H, seed, layers=1, bias=True, dropout=0.0, xscale=1.0):
    torch.manual_seed(seed)
    m = torch.nn.LSTM(Din, H, layers, bias=bias, batch_first=True, bidirectional=True, dropout=dropout)
    rng = np.random.RandomState(seed + 1)
    x = (xscale * rng.randn(B, T, Din)).astype(np.float32)
    dy = rng.randn(B, T, 2 * H).astype(np.float32)
    return m, x, dy


def _oracle(m, x, lens, dy):
    """(float64, float32) runs of the oracle on the module's fp32 parameters."""
    params = [lstm_ref.params_of(m, l) for l in range(m.num_layers)]
    return tuple(lstm_ref.bilstm_stack_ref(x, lens, params, dy, dt) for dt in (np.float64, np.float32))


def _run_bilstm(rnn, dev, m, x, lens, dy, lens_dtype=torch.int32, training=True):
    """rnn.bilstm on the GPU, forward and backward: (y [B*T,2H], dx [B*T,Din], {name: grad}) as numpy."""
    B, T, Din = x.shape
    md = m.to(dev)
    md.zero_grad(set_to_none=True)
    xd = torch.from_numpy(x).to(dev).requires_grad_()
    y = rnn.bilstm(xd, torch.from_numpy(np.asarray(lens)).to(device=dev, dtype=lens_dtype), md, training)
    y.backward(torch.from_numpy(dy).to(dev))
    torch.cuda.synchronize()
    grads = {n: p.grad.cpu().numpy() for n, p in md.named_parameters()}
    return y.detach().reshape(B * T, -1).cpu().numpy(), xd.grad.reshape(B * T, Din).cpu().numpy(), grads


def _check_bilstm(got, ref64, ref32, m, lens, T):
    y, dx, grads = got
    assert_fp32_close("y", y, ref64["y"], ref32["y"], FWD_BAR)
    pad = (np.arange(T)[None, :] >= np.asarray(lens)[:, None]).reshape(-1)
    assert not y[pad].any(), "padding rows of y are not exactly 0"
    assert_fp32_close("dx", dx, ref64["dx"], ref32["dx"], GRAD_BAR, GEMM_FLOOR)
    assert len(grads) == (8 if m.bias else 4) * m.num_layers
    for l in range(m.num_layers):
        for d, sfx in enumerate(("", "_reverse")):
            for name, key in (("weight_ih", "dw_ih"), ("weight_hh", "dw_hh"), ("bias_ih", "db"), ("bias_hh", "db")):
                n = "%s_l%d%s" % (name, l, sfx)
                if n in grads:
                    assert_fp32_close(n, grads[n], ref64[key][l][d], ref32[key][l][d], GRAD_BAR, GEMM_FLOOR)


def _params_dev(dev, params):
    """The direct calls' operands of one layer: w_ih [8H,Din] and bias [8H] (both directions), w_hh_f, w_hh_r."""
    f = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)      # noqa: E731
    (wf, hf, bif, bhf), (wr, hr, bir, bhr) = params
    bias = None if bif is None else f(np.concatenate((bif + bhf, bir + bhr)))
    return f(np.concatenate((wf, wr))), bias, f(hf), f(hr)


def _direct(_lib, dev, x, lens, params, dy, save=True, fill=float("nan")):
    """gcnpt_lstm_fwd (+ gcnpt_lstm_bwd when save) on buffers filled with `fill`; numpy dict of every output."""
    B, T, Din = x.shape
    w_ih, bias, whh_f, whh_r = _params_dev(dev, params)
    H = whh_f.shape[1]
    x2 = torch.from_numpy(x.reshape(B * T, Din)).to(dev)
    gx = torch.addmm(bias, x2, w_ih.t()) if bias is not None else torch.mm(x2, w_ih.t())
    ld = torch.from_numpy(np.asarray(lens, dtype=np.int32)).to(dev)
    full = lambda *shape: torch.full(shape, fill, dtype=torch.float32, device=dev)          # noqa: E731
    y, c = full(B * T, 2 * H), full(B * T, 2 * H)
    gates, h_prev = (full(B * T, 8 * H), full(B * T, 2 * H)) if save else (None, None)
    P, L = _lib.ptr, _lib.lib()
    _lib.check(L.gcnpt_lstm_fwd(_lib.stream(), P(gx), 8 * H, P(whh_f), P(whh_r), P(ld), B, T, H, P(y), P(c), P(gates), P(h_prev)))
    out = dict(y=y, c=c)
    if save:
        dg, dc = full(B * T, 8 * H), full(2 * B * H)
        dyd = torch.from_numpy(dy.reshape(B * T, 2 * H)).to(dev)
        _lib.check(L.gcnpt_lstm_bwd(_lib.stream(), P(dyd), P(whh_f), P(whh_r), P(ld), B, T, H, P(c), P(gates), 8 * H, P(dg), P(dc)))
        out.update(gates=gates, h_prev=h_prev, dgates=dg, dc=dc)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _check_direct(out, lens, T, H, ref64, ref32):
    """Every row written, padding exactly 0, h_prev 0 at each sentence's first step, and every output against the oracle."""
    lens = np.asarray(lens)
    B = lens.shape[0]
    for k, v in out.items():
        assert not np.isnan(v).any(), "%s: %d entries never written" % (k, int(np.isnan(v).sum()))
    pad = (np.arange(T)[None, :] >= lens[:, None]).reshape(-1)
    for k in ("y", "c", "h_prev", "gates", "dgates"):
        assert not out[k][pad].any(), "padding rows of %s are not exactly 0" % k
    hp = out["h_prev"].reshape(B, T, 2 * H)
    for b in np.nonzero(lens > 0)[0]:
        assert not hp[b, 0, :H].any() and not hp[b, lens[b] - 1, H:].any(), "h_prev of sentence %d's first step is not 0" % b
    for k in ("y", "c", "gates", "h_prev"):
        assert_fp32_close(k, out[k], ref64[k], ref32[k], FWD_BAR)
    assert_fp32_close("dgates", out["dgates"], ref64["dgates"], ref32["dgates"], GRAD_BAR)
    assert_fp32_close("dc", out["dc"], ref64["dc0"].reshape(-1), ref32["dc0"].reshape(-1), GRAD_BAR)


# (B, T, Din, H): every H in {1, 15, 16, 17, 64, 200, 256, 257, 300, 512}, every B in {1, 16, 17, 33, 50}, every T in {1, 2, 37, 100},
# T = 300 at H = 200; every H > 256 with ragged lengths (B >= 3: the lengths include 0, 1 and T)
SWEEP = [(1, 1, 3, 1), (17, 100, 5, 1), (1, 37, 8, 15), (33, 2, 9, 15), (16, 2, 6, 16), (50, 100, 12, 16), (17, 37, 7, 17),
         (1, 100, 10, 64), (33, 100, 20, 64), (50, 37, 24, 200), (50, 300, 16, 200), (16, 100, 24, 256), (17, 37, 11, 257),
         (33, 2, 9, 257), (1, 100, 8, 257), (33, 100, 16, 300), (16, 37, 13, 300), (33, 1, 6, 300), (50, 37, 16, 512),
         (16, 2, 5, 512), (17, 100, 8, 512)]
SWEEP_IDS = ["B%d-T%d-H%d" % (B, T, H) for B, T, _, H in SWEEP]


@pytest.mark.parametrize("B,T,Din,H", SWEEP, ids=SWEEP_IDS)
def test_bilstm_sweep_matches_float64(mods, dev, B, T, Din, H):
    _, rnn = mods
    m, x, dy = _case(B, T, Din, H, seed=B * 1000 + T * 10 + H)
    lens = _lens(B, T, B + T + H)
    ref64, ref32 = _oracle(m, x, lens, dy)
    _check_bilstm(_run_bilstm(rnn, dev, m, x, lens, dy), ref64, ref32, m, lens, T)


@pytest.mark.parametrize("B,T,Din,H", SWEEP, ids=SWEEP_IDS)
def test_direct_sweep_every_row_written(mods, dev, B, T, Din, H):
    _lib, _ = mods
    m, x, dy = _case(B, T, Din, H, seed=B * 1000 + T * 10 + H + 1)
    lens = _lens(B, T, B + T + H + 1)
    params = lstm_ref.params_of(m)
    ref64, ref32 = (lstm_ref.bilstm_ref(x, lens, params, dy, dt) for dt in (np.float64, np.float32))
    _check_direct(_direct(_lib, dev, x, lens, params, dy), lens, T, H, ref64, ref32)


LENGTH_EDGES = {"all0": lambda B, T: np.zeros(B, np.int64), "all1": lambda B, T: np.ones(B, np.int64),
                "allT": lambda B, T: np.full(B, T, np.int64), "mix0": lambda B, T: np.arange(B) % 3 * (T // 2)}


@pytest.mark.parametrize("kind", sorted(LENGTH_EDGES))
@pytest.mark.parametrize("H", [17, 300])
def test_length_edges(mods, dev, kind, H):
    _lib, rnn = mods
    B, T, Din = 17, 37, 9
    lens = LENGTH_EDGES[kind](B, T)
    assert kind != "mix0" or (lens == 0).any()
    m, x, dy = _case(B, T, Din, H, seed=H + len(kind))
    ref64, ref32 = _oracle(m, x, lens, dy)
    got = _run_bilstm(rnn, dev, m, x, lens, dy)
    params = lstm_ref.params_of(m)
    out = _direct(_lib, dev, x, lens, params, dy)
    if kind == "all0":
        y, dx, grads = got
        assert not y.any() and not dx.any(), "a batch of empty sentences gives a nonzero output or dx"
        for n, g in grads.items():
            assert not g.any(), n
        for k, v in out.items():
            assert not np.isnan(v).any() and not v.any(), k
        return
    _check_bilstm(got, ref64, ref32, m, lens, T)
    r64, r32 = (lstm_ref.bilstm_ref(x, lens, params, dy, dt) for dt in (np.float64, np.float32))
    _check_direct(out, lens, T, H, r64, r32)


def test_inference_branch_bit_identical(mods, dev):
    """gates = h_prev = NULL (nothing saved) gives the training call's y and c bit for bit; so does bilstm under no_grad with frozen
    parameters, which takes that branch."""
    _lib, rnn = mods
    B, T, Din, H = 33, 37, 10, 300
    m, x, dy = _case(B, T, Din, H, seed=11)
    lens = _lens(B, T, 12)
    params = lstm_ref.params_of(m)
    train = _direct(_lib, dev, x, lens, params, dy, save=True)
    infer = _direct(_lib, dev, x, lens, params, dy, save=False)
    assert set(infer) == {"y", "c"}
    assert np.array_equal(train["y"], infer["y"]) and np.array_equal(train["c"], infer["c"])

    y_train = _run_bilstm(rnn, dev, m, x, lens, dy)[0]
    md = m.to(dev).requires_grad_(False)
    with torch.no_grad():
        y = rnn.bilstm(torch.from_numpy(x).to(dev), torch.from_numpy(lens).to(dev), md, False)
    assert y.grad_fn is None
    assert np.array_equal(y.reshape(B * T, 2 * H).cpu().numpy(), y_train)


def test_deterministic(mods, dev):
    """Two calls give bit-identical outputs (the waves' partial sums meet in a fixed order)."""
    _lib, _ = mods
    B, T, Din, H = 50, 37, 16, 257
    m, x, dy = _case(B, T, Din, H, seed=21)
    lens = _lens(B, T, 22)
    params = lstm_ref.params_of(m)
    a = _direct(_lib, dev, x, lens, params, dy)
    b = _direct(_lib, dev, x, lens, params, dy, fill=0.0)
    for k in ("y", "c", "gates", "h_prev", "dgates", "dc"):
        assert np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("H", [64, 300])
def test_saturated_gates(mods, dev, H):
    """x scaled by 30: most gate pre-activations are far into the sigmoid's and tanh's flat tails.  Finite, and as close to float64 as
    an fp32 computation gets."""
    _lib, rnn = mods
    B, T, Din = 17, 37, 12
    m, x, dy = _case(B, T, Din, H, seed=31 + H, xscale=30.0)
    lens = _lens(B, T, 32)
    ref64, ref32 = _oracle(m, x, lens, dy)
    got = _run_bilstm(rnn, dev, m, x, lens, dy)
    assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all() and all(np.isfinite(v).all() for v in got[2].values())
    _check_bilstm(got, ref64, ref32, m, lens, T)
    params = lstm_ref.params_of(m)
    r64, r32 = (lstm_ref.bilstm_ref(x, lens, params, dy, dt) for dt in (np.float64, np.float32))
    live = (np.arange(T)[None, :] < lens[:, None]).reshape(-1)
    assert r64["gates"][live, :H].min() < 1e-6 and r64["gates"][live, :H].max() > 1 - 1e-6     # input gates shut and wide open
    _check_direct(_direct(_lib, dev, x, lens, params, dy), lens, T, H, r64, r32)


def test_bilstm_bias_false(mods, dev):
    _, rnn = mods
    B, T, Din, H = 17, 37, 11, 257
    m, x, dy = _case(B, T, Din, H, seed=41, bias=False)
    lens = _lens(B, T, 42)
    ref64, ref32 = _oracle(m, x, lens, dy)
    got = _run_bilstm(rnn, dev, m, x, lens, dy)
    assert set(got[2]) == {"weight_ih_l0", "weight_hh_l0", "weight_ih_l0_reverse", "weight_hh_l0_reverse"}
    _check_bilstm(got, ref64, ref32, m, lens, T)


def test_bilstm_three_layers(mods, dev):
    _, rnn = mods
    B, T, Din, H = 16, 37, 24, 40
    m, x, dy = _case(B, T, Din, H, seed=51, layers=3)
    lens = _lens(B, T, 52)
    ref64, ref32 = _oracle(m, x, lens, dy)
    _check_bilstm(_run_bilstm(rnn, dev, m, x, lens, dy), ref64, ref32, m, lens, T)


def test_bilstm_dropout_ignored_in_eval(mods, dev):
    """nn.LSTM(dropout=0.5) called with training=False: no dropout between the layers (the oracle has none), and the output and
    gradients are bit-identical to the same module with dropout=0."""
    _, rnn = mods
    B, T, Din, H = 17, 37, 9, 33
    m, x, dy = _case(B, T, Din, H, seed=61, layers=2, dropout=0.5)
    lens = _lens(B, T, 62)
    ref64, ref32 = _oracle(m, x, lens, dy)
    got = _run_bilstm(rnn, dev, m, x, lens, dy, training=False)
    _check_bilstm(got, ref64, ref32, m, lens, T)
    m0, _, _ = _case(B, T, Din, H, seed=61, layers=2, dropout=0.0)
    ref = _run_bilstm(rnn, dev, m0, x, lens, dy, training=False)
    assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])
    assert all(np.array_equal(got[2][n], ref[2][n]) for n in ref[2])


def test_bilstm_lens_int64_and_int32_agree(mods, dev):
    _, rnn = mods
    B, T, Din, H = 33, 37, 8, 300
    m, x, dy = _case(B, T, Din, H, seed=71)
    lens = _lens(B, T, 72)
    a = _run_bilstm(rnn, dev, m, x, lens, dy, lens_dtype=torch.int32)
    b = _run_bilstm(rnn, dev, m, x, lens, dy, lens_dtype=torch.int64)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert set(a[2]) == set(b[2]) and all(np.array_equal(a[2][n], b[2][n]) for n in a[2])


def test_bilstm_only_weight_hh_l0_reverse_needs_grad(mods, dev):
    """Two layers, x and every parameter but weight_hh_l0_reverse frozen: that gradient is the oracle's, every other one is None (the
    needs_input_grad branches of _BiLSTMLayerFn.backward; layer 1 still passes dx down)."""
    _, rnn = mods
    B, T, Din, H = 17, 37, 10, 257
    m, x, dy = _case(B, T, Din, H, seed=81, layers=2)
    lens = _lens(B, T, 82)
    ref64, ref32 = _oracle(m, x, lens, dy)
    md = m.to(dev)
    for n, p in md.named_parameters():
        p.requires_grad_(n == "weight_hh_l0_reverse")
    xd = torch.from_numpy(x).to(dev)
    y = rnn.bilstm(xd, torch.from_numpy(lens).to(dev), md, True)
    y.backward(torch.from_numpy(dy).to(dev))
    torch.cuda.synchronize()
    assert xd.grad is None
    assert [n for n, p in md.named_parameters() if p.grad is not None] == ["weight_hh_l0_reverse"]
    assert_fp32_close("weight_hh_l0_reverse", md.weight_hh_l0_reverse.grad.cpu().numpy(), ref64["dw_hh"][0][1], ref32["dw_hh"][0][1],
                      GRAD_BAR, GEMM_FLOOR)


def test_bilstm_graph_capture_h300_zero_length(mods, dev):
    """bilstm forward and backward at H = 300 (the second load trip) with a sentence of length 0, captured as one hipGraph on one stream,
    replays to the eager results bit for bit."""
    _, rnn = mods
    B, T, Din, H = 17, 37, 12, 300
    m, x, dy = _case(B, T, Din, H, seed=91)
    lens = _lens(B, T, 92)
    assert (lens == 0).any()
    md = m.to(dev)
    xd = torch.from_numpy(x).to(dev).requires_grad_()
    ld = torch.from_numpy(lens.astype(np.int32)).to(dev)
    dyd = torch.from_numpy(dy).to(dev)

    def step():
        md.zero_grad(set_to_none=False)
        if xd.grad is not None:
            xd.grad.zero_()
        y = rnn.bilstm(xd, ld, md, True)
        y.backward(dyd)
        return y.detach()

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        static_y = step()
    graph.replay()
    torch.cuda.synchronize()
    got_y, got_dx = static_y.clone(), xd.grad.clone()
    got = {n: p.grad.clone() for n, p in md.named_parameters()}
    eager_y = step()
    torch.cuda.synchronize()
    assert torch.equal(got_y, eager_y) and torch.equal(got_dx, xd.grad)
    assert len(got) == 8 and all(torch.equal(got[n], p.grad) for n, p in md.named_parameters())
    ref64, ref32 = _oracle(m.cpu(), x, lens, dy)
    assert_fp32_close("captured y", got_y.reshape(B * T, 2 * H).cpu().numpy(), ref64["y"], ref32["y"], FWD_BAR)
