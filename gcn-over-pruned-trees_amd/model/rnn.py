"""
The C-GCN model's BiLSTM encoder on the native recurrence (csrc/lstm_kernels.hip, gcnpt_lstm_fwd / gcnpt_lstm_bwd).

`bilstm(x, lens, lstm, training)` computes what the reference's GCN.encode_with_rnn does (model/gcn.py: nn.LSTM(bidirectional=True,
batch_first=True) over pack_padded_sequence(x, lens, enforce_sorted=False) from a zero state, then pad_packed_sequence), with the
lengths on the device: no host sync, so a whole C-GCN training step captures into a hipGraph.  It reads the parameters of the given
nn.LSTM on every call (state_dict names, checkpoints, `p.data` updates, flatten_parameters() and .to() are unaffected).

Per layer: the step-to-step recurrence is the library's (T launches per direction sweep, both directions in each); the time-parallel
products are library GEMMs here:  Gx = x W_ih^T + b_ih + b_hh (both directions in one GEMM), dx = dG W_ih, dW_ih = dG^T x,
dW_hh = dG^T h_prev (h_prev saved by the forward kernel), db_ih = db_hh = sum dG.

Differences from the torch path: the output is always [B, T, 2H] (pad_packed_sequence returns max(len) columns; the reference's loader
pads every batch to its longest sentence, so the two agree there), a sentence of length 0 gives zeros (pack_padded_sequence raises), and
between stacked layers the dropout masks come from F.dropout, not from the fused RNN's RNG stream.  Everything is fp32.
"""
import torch
import torch.nn.functional as F

from .. import _lib


class _BiLSTMLayerFn(torch.autograd.Function):
    """One bidirectional LSTM layer: x [B,T,Din] -> y [B,T,2H]; parameters in nn.LSTM's layout (gate order i, f, g, o)."""

    @staticmethod
    def forward(ctx, x, lens, w_ih_f, w_hh_f, b_ih_f, b_hh_f, w_ih_r, w_hh_r, b_ih_r, b_hh_r):
        B, T, Din = x.shape
        H = w_hh_f.shape[1]
        if w_ih_f.shape != (4 * H, Din) or w_ih_r.shape != (4 * H, Din) or w_hh_r.shape != (4 * H, H):
            raise RuntimeError("bilstm: input width %d does not match weights %s / %s" % (Din, tuple(w_ih_f.shape), tuple(w_hh_f.shape)))
        dev = x.device
        x2 = x.reshape(B * T, Din).to(torch.float32).contiguous()
        w_ih = torch.cat((w_ih_f, w_ih_r)).to(torch.float32)                                       # [8H, Din]
        bias = None
        if b_ih_f is not None:
            bias = torch.cat((b_ih_f + b_hh_f, b_ih_r + b_hh_r)).to(torch.float32)
            gx = torch.addmm(bias, x2, w_ih.t())
        else:
            gx = torch.mm(x2, w_ih.t())
        whh_f = w_hh_f.detach().to(torch.float32).contiguous()
        whh_r = w_hh_r.detach().to(torch.float32).contiguous()
        lens = lens.to(device=dev, dtype=torch.int32).contiguous()
        y = torch.empty((B * T, 2 * H), dtype=torch.float32, device=dev)
        c = torch.empty_like(y)
        want_bwd = any(ctx.needs_input_grad)
        gates = torch.empty((B * T, 8 * H), dtype=torch.float32, device=dev) if want_bwd else None
        h_prev = torch.empty_like(y) if want_bwd else None
        P = _lib.ptr
        _lib.check(_lib.lib().gcnpt_lstm_fwd(_lib.stream(), P(gx), 8 * H, P(whh_f), P(whh_r), P(lens), B, T, H,
                                             P(y), P(c), P(gates), P(h_prev)))
        if want_bwd:
            ctx.save_for_backward(x2, lens, w_ih, whh_f, whh_r, c, gates, h_prev)
        ctx.dims = (B, T, Din, H)
        ctx.x_dtype, ctx.has_bias = x.dtype, bias is not None
        return y.view(B, T, 2 * H)

    @staticmethod
    def backward(ctx, dy):
        x2, lens, w_ih, whh_f, whh_r, c, gates, h_prev = ctx.saved_tensors
        B, T, Din, H = ctx.dims
        dev = dy.device
        dy = dy.to(torch.float32).reshape(B * T, 2 * H).contiguous()
        dg = torch.empty((B * T, 8 * H), dtype=torch.float32, device=dev)
        dc = torch.empty((2 * B * H,), dtype=torch.float32, device=dev)
        P = _lib.ptr
        _lib.check(_lib.lib().gcnpt_lstm_bwd(_lib.stream(), P(dy), P(whh_f), P(whh_r), P(lens), B, T, H,
                                             P(c), P(gates), 8 * H, P(dg), P(dc)))
        n = ctx.needs_input_grad
        dx = torch.mm(dg, w_ih).view(B, T, Din).to(ctx.x_dtype) if n[0] else None
        dw_ih = torch.mm(dg.t(), x2) if (n[2] or n[6]) else None                                  # [8H, Din]
        dw_hh_f = torch.mm(dg[:, :4 * H].t(), h_prev[:, :H]) if n[3] else None
        dw_hh_r = torch.mm(dg[:, 4 * H:].t(), h_prev[:, H:]) if n[7] else None
        db = dg.sum(0) if ctx.has_bias else None
        dbf, dbr = (db[:4 * H], db[4 * H:]) if db is not None else (None, None)
        return (dx, None, dw_ih[:4 * H] if n[2] else None, dw_hh_f, dbf if n[4] else None, dbf if n[5] else None,
                dw_ih[4 * H:] if n[6] else None, dw_hh_r, dbr if n[8] else None, dbr if n[9] else None)


def bilstm(x, lens, lstm, training):
    """The reference's encode_with_rnn output [B, T, 2H] of `lstm` (an nn.LSTM with bidirectional=True, batch_first=True) over x [B,T,Din]
    with per-sentence lengths `lens` (a device tensor, any integer dtype), on the native recurrence.  Between stacked layers, dropout
    lstm.dropout is applied in training mode, where nn.LSTM applies it."""
    if not (lstm.bidirectional and lstm.batch_first):
        raise ValueError("bilstm: the module must be nn.LSTM(bidirectional=True, batch_first=True), as the reference builds it")
    if getattr(lstm, "proj_size", 0):
        raise ValueError("bilstm: nn.LSTM with proj_size is not supported")
    _lib.require_gpu(x)
    out = x
    for layer in range(lstm.num_layers):
        if layer > 0 and training and lstm.dropout > 0:
            out = F.dropout(out, p=lstm.dropout, training=True)
        args = []
        for sfx in ("", "_reverse"):
            args += [getattr(lstm, "weight_ih_l%d%s" % (layer, sfx)), getattr(lstm, "weight_hh_l%d%s" % (layer, sfx))]
            args += [getattr(lstm, "bias_ih_l%d%s" % (layer, sfx), None), getattr(lstm, "bias_hh_l%d%s" % (layer, sfx), None)] \
                if lstm.bias else [None, None]
        out = _BiLSTMLayerFn.apply(out, lens, *args)
    return out
