"""
The output head of GCNClassifier over csrc/head_kernels.hip: `linear_act` (out_mlp's Linear + ReLU layers and the classifier, reference
model/gcn.py:31-36, 66-72, 122-125), `head_loss` (the trainer's CrossEntropyLoss + pooling_l2 penalty, model/trainer.py:94-100) and
`head_predict` (its softmax + argmax, trainer.py:119-120).  Everything float32, one launch per op and direction, no host sync.
"""
import torch

from .. import _lib


def _gpu_only(what, *tensors):
    for t in tensors:
        if t is not None and not (torch.is_tensor(t) and t.is_cuda):
            raise TypeError("%s runs on the GPU only (got %s); there is no CPU path" % (what, t.device if torch.is_tensor(t) else type(t)))


def _rows(x):
    """x as float32 [M, K] rows the kernels can read in place: unit column stride, row stride >= K (a column slice of a wider tensor
    qualifies; anything else is copied).  Returns (tensor, row stride in elements)."""
    x = x.detach()
    if x.dtype != torch.float32:
        x = x.float()
    M, K = x.shape
    if (K > 1 and x.stride(1) != 1) or (M > 1 and x.stride(0) < K):
        x = x.contiguous()
    return x, (x.stride(0) if M > 1 else K)


class _LinearActFn(torch.autograd.Function):
    """y = act(x W^T + b) as ONE autograd node over gcnpt_head_linear_fwd / gcnpt_head_linear_bwd: the backward's dx, dW and db come from
    one launch (dx skipped when x needs no gradient), dW / db as fresh tensors that autograd accumulates."""

    @staticmethod
    def forward(ctx, x, weight, bias, relu):
        lib, st, P = _lib.lib(), _lib.stream(), _lib.ptr
        xs, ldx = _rows(x)
        w = weight.detach().to(torch.float32).contiguous()
        b = bias.detach().to(torch.float32).contiguous()
        (M, K), N = xs.shape, w.shape[0]
        y = torch.empty((M, N), dtype=torch.float32, device=xs.device)
        _lib.check(lib.gcnpt_head_linear_fwd(st, xs.data_ptr(), ldx, P(w), P(b), P(y), M, K, N, int(relu)))
        ctx.save_for_backward(xs, w, y if relu else None)
        ctx.ldx, ctx.relu, ctx.dtypes = ldx, bool(relu), (x.dtype, weight.dtype, bias.dtype)
        return y

    @staticmethod
    def backward(ctx, g):
        xs, w, y = ctx.saved_tensors
        lib, st, P = _lib.lib(), _lib.stream(), _lib.ptr
        (M, K), N = xs.shape, w.shape[0]
        g = g.to(torch.float32).contiguous()
        f32 = dict(dtype=torch.float32, device=g.device)
        dx = torch.empty((M, K), **f32) if ctx.needs_input_grad[0] else None
        dw, db = torch.empty((N, K), **f32), torch.empty((N,), **f32)
        _lib.check(lib.gcnpt_head_linear_bwd(st, P(g), P(y), xs.data_ptr(), ctx.ldx, P(w), P(dx), K, P(dw), P(db), M, K, N, int(ctx.relu)))
        tx, tw, tb = ctx.dtypes
        return (dx.to(tx) if dx is not None else None, dw.to(tw) if ctx.needs_input_grad[1] else None,
                db.to(tb) if ctx.needs_input_grad[2] else None, None)


def linear_act(x, weight, bias, relu=False):
    """relu(x @ weight.T + bias) (relu=True) or x @ weight.T + bias, float32, exact fp32 MFMA, one launch forward and one backward.
    x: 2-D CUDA tensor [M, K] with any row stride (pooled[:, :H] of a wider tensor is read in place); weight [N, K] and bias [N] as
    nn.Linear holds them.  Returns a contiguous [M, N] tensor."""
    _gpu_only("linear_act", x, weight, bias)
    if x.dim() != 2 or weight.dim() != 2 or bias.dim() != 1 or weight.shape[1] != x.shape[1] or bias.shape[0] != weight.shape[0]:
        raise ValueError("linear_act: x [M,K], weight [N,K], bias [N] expected, got %s, %s, %s" % (tuple(x.shape), tuple(weight.shape), tuple(bias.shape)))
    return _LinearActFn.apply(x, weight, bias, bool(relu))


class _HeadLossFn(torch.autograd.Function):
    """cross entropy (mean) + l2 * mean_m sum_j pooled[m,j]^2 as ONE autograd node over gcnpt_head_loss_fwd / gcnpt_head_loss_bwd.  The
    backward recomputes the softmax from the logits and reads the incoming gradient from the device."""

    @staticmethod
    def forward(ctx, logits, labels, pooled, l2, status):
        lib, st, P = _lib.lib(), _lib.stream(), _lib.ptr
        z = logits.detach().to(torch.float32).contiguous()
        y = labels.contiguous()
        M, C = z.shape
        ps, ldp, H = None, 0, 0
        if pooled is not None and l2 > 0:
            ps, ldp = _rows(pooled)
            H = ps.shape[1]
        loss = torch.empty((), dtype=torch.float32, device=z.device)
        _lib.check(lib.gcnpt_head_loss_fwd(st, P(z), P(y), ps.data_ptr() if ps is not None else None, ldp, H, l2, M, C, P(loss), None, None,
                                           P(status)))
        ctx.save_for_backward(z, y, ps)
        ctx.lay = (ldp, H, l2, M, C)
        ctx.dtypes = (logits.dtype, pooled.dtype if pooled is not None else None)
        return loss

    @staticmethod
    def backward(ctx, g):
        z, y, ps = ctx.saved_tensors
        lib, st, P = _lib.lib(), _lib.stream(), _lib.ptr
        ldp, H, l2, M, C = ctx.lay
        g = g.to(torch.float32).contiguous()
        f32 = dict(dtype=torch.float32, device=z.device)
        dz = torch.empty((M, C), **f32) if ctx.needs_input_grad[0] else None
        dp = torch.empty((M, H), **f32) if (ps is not None and ctx.needs_input_grad[2]) else None
        if dz is not None or dp is not None:
            _lib.check(lib.gcnpt_head_loss_bwd(st, P(g), P(z), P(y), ps.data_ptr() if ps is not None else None, ldp, H, l2, M, C, P(dz), P(dp)))
        return (dz.to(ctx.dtypes[0]) if dz is not None else None, None, dp.to(ctx.dtypes[1]) if dp is not None else None, None, None)


def head_loss(logits, labels, pooling_output=None, pooling_l2=0.0, status=None):
    """CrossEntropyLoss()(logits, labels) + pooling_l2 * (pooling_output ** 2).sum(1).mean() (model/trainer.py:94-100) as a 0-dim float32
    tensor, one launch forward and one backward.  logits [M, C] float, labels int64 [M]; pooling_output [M, H] may be the strided
    pooled[:, :H] view the model returns (read in place).  A label outside [0, C) contributes nothing, gets a zero gradient row and sets bit
    0 of `status` (optional int32 [1] CUDA tensor, written by the launch) -- an error for the caller to raise, not ignore_index."""
    _gpu_only("head_loss", logits, labels, pooling_output, status)
    if logits.dim() != 2 or labels.dim() != 1 or labels.dtype != torch.int64 or labels.shape[0] != logits.shape[0]:
        raise TypeError("head_loss: logits [M,C] and int64 labels [M] expected, got %s and %s %s" % (tuple(logits.shape), labels.dtype, tuple(labels.shape)))
    if pooling_output is not None and (pooling_output.dim() != 2 or pooling_output.shape[0] != logits.shape[0]):
        raise TypeError("head_loss: pooling_output must be [M,H], got %s" % (tuple(pooling_output.shape),))
    if status is not None and (status.dtype != torch.int32 or status.numel() != 1):
        raise TypeError("head_loss: status must be an int32 [1] tensor")
    return _HeadLossFn.apply(logits, labels, pooling_output, float(pooling_l2), status)


def head_predict(logits):
    """(F.softmax(logits, 1), argmax(logits, 1)) -- the trainer's predict (model/trainer.py:119-120) -- from one launch; ties resolve to the
    lowest index, as np.argmax does.  No gradient flows through it."""
    _gpu_only("head_predict", logits)
    if logits.dim() != 2:
        raise TypeError("head_predict: logits [M,C] expected, got %s" % (tuple(logits.shape),))
    z = logits.detach().to(torch.float32).contiguous()
    M, C = z.shape
    probs = torch.empty((M, C), dtype=torch.float32, device=z.device)
    pred = torch.empty((M,), dtype=torch.int64, device=z.device)
    _lib.check(_lib.lib().gcnpt_head_loss_fwd(_lib.stream(), _lib.ptr(z), None, None, 0, 0, 0.0, M, C, None, _lib.ptr(probs), _lib.ptr(pred), None))
    return probs, pred
