"""CPU-side checks of the native BiLSTM recurrence (include/gcnpt.h gcnpt_lstm_fwd / gcnpt_lstm_bwd, model/rnn.py): the symbols are
exported, argument validation returns the documented codes without a GPU, and opt['gcn_native_rnn'] leaves the module's parameters and
state_dict names as they are.  No compute is launched here."""
import ctypes

import pytest

from gcn_over_pruned_trees_amd import _lib


def test_lstm_symbols_exported():
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("gcnpt_lstm_fwd", "gcnpt_lstm_bwd"):
        assert hasattr(handle, name), name
        assert name in _lib.SIGNATURES


def test_lstm_argument_validation_needs_no_gpu():
    L = _lib.lib()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    B, T, H = 2, 3, 4
    # fwd(stream, gx, gx_cols, w_hh_f, w_hh_r, lens, B, T, H, y, c, gates, h_prev); every call here fails its checks before a launch
    assert L.gcnpt_lstm_fwd(None, None, 8 * H, p, p, p, B, T, H, p, p, None, None) == _lib.E_INVALID
    assert b"null" in L.gcnpt_last_error()
    assert L.gcnpt_lstm_fwd(None, p, 8 * H, p, None, p, B, T, H, p, p, None, None) == _lib.E_INVALID
    assert L.gcnpt_lstm_fwd(None, p, 8 * H, p, p, None, B, T, H, p, p, None, None) == _lib.E_INVALID
    assert L.gcnpt_lstm_fwd(None, p, 8 * H, p, p, p, B, T, H, p, None, None, None) == _lib.E_INVALID
    assert L.gcnpt_lstm_fwd(None, p, 0, p, p, p, B, T, 0, p, p, None, None) == _lib.E_INVALID
    assert b"hidden size" in L.gcnpt_last_error()
    assert L.gcnpt_lstm_fwd(None, p, 8 * H, p, p, p, 0, T, H, p, p, None, None) == _lib.E_INVALID
    assert L.gcnpt_lstm_fwd(None, p, 8 * H, p, p, p, B, -1, H, p, p, None, None) == _lib.E_INVALID
    # the gate rows must be the two directions' 4 gates of H units: x W_ih^T of a mismatched input width / hidden size is refused
    assert L.gcnpt_lstm_fwd(None, p, 4 * H, p, p, p, B, T, H, p, p, None, None) == _lib.E_INVALID
    assert b"columns" in L.gcnpt_last_error()
    # B*T*8H beyond the kernels' 32-bit indexing
    assert L.gcnpt_lstm_fwd(None, p, 8 * 200, p, p, p, 50000, 1000, 200, p, p, None, None) == _lib.E_UNSUPPORTED
    assert L.gcnpt_lstm_fwd(None, p, 8, p, p, p, 1 << 30, 1 << 30, 1, p, p, None, None) == _lib.E_UNSUPPORTED
    # bwd(stream, dy, w_hh_f, w_hh_r, lens, B, T, H, c, gates, gates_cols, dgates, dc)
    assert L.gcnpt_lstm_bwd(None, None, p, p, p, B, T, H, p, p, 8 * H, p, p) == _lib.E_INVALID
    assert L.gcnpt_lstm_bwd(None, p, p, p, p, B, T, H, p, p, 8 * H, p, None) == _lib.E_INVALID
    assert L.gcnpt_lstm_bwd(None, p, p, p, p, B, T, H, p, None, 8 * H, p, p) == _lib.E_INVALID
    assert L.gcnpt_lstm_bwd(None, p, p, p, p, B, T, 0, p, p, 0, p, p) == _lib.E_INVALID
    assert L.gcnpt_lstm_bwd(None, p, p, p, p, B, T, H, p, p, 8 * H + 1, p, p) == _lib.E_INVALID
    assert L.gcnpt_lstm_bwd(None, p, p, p, p, 50000, 1000, 200, p, p, 8 * 200, p, p) == _lib.E_UNSUPPORTED


def test_native_rnn_option_keeps_state_dict():
    import torch
    from gcn_over_pruned_trees_amd.model import gcn, rnn
    opt = dict(vocab_size=50, emb_dim=8, pos_dim=2, ner_dim=2, hidden_dim=16, num_layers=2, input_dropout=0.0, gcn_dropout=0.5,
               prune_k=1, pooling="max", mlp_layers=2, rnn=True, rnn_hidden=5, rnn_layers=2, rnn_dropout=0.0, dataset="tacred",
               num_class=42, topn=10, cuda=False)
    plain = gcn.GCNClassifier(opt)
    native = gcn.GCNClassifier(dict(opt, gcn_native_rnn=True))
    a, b = plain.state_dict(), native.state_dict()
    assert list(a) == list(b)
    assert all(a[k].shape == b[k].shape for k in a)
    assert isinstance(native.gcn_model.gcn.rnn, torch.nn.LSTM)
    assert "gcn_model.gcn.rnn.weight_hh_l1_reverse" in b
    native.load_state_dict(a, strict=True)                      # checkpoints of either form load into the other
    # the native path has no CPU fallback: a CPU tensor is refused, never run through torch
    x = torch.zeros(1, 3, native.gcn_model.gcn.rnn.input_size)
    with pytest.raises(RuntimeError, match="GPU only"):
        rnn.bilstm(x, torch.tensor([3]), native.gcn_model.gcn.rnn, False)
