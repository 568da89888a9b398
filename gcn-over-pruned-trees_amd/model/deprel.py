"""
The ops of the relation-aware adjacency types: `full_deprel`'s fused aggregation and bilinear traversal (reference model/gcn.py:296-388,
400-434; csrc/full_kernels.hip, csrc/bilinear_kernels.hip) and the `diagonal_deprel` layer (gcn.py:272-294; csrc/diag_kernels.hip).
"""
import torch

from .. import _lib
from ..utils import constant


class _FullAggFn(torch.autograd.Function):
    """Aggregation + self loop + /(deg+1) + ReLU + dropout of a full_deprel layer in one kernel (csrc/full_kernels.hip); reference
    model/gcn.py:308-311, 331, 340-344, 362, 385, 390-393.  `trees`: a PrunedTrees (rows [B*T, H]) or a PackedTrees (rows [N, H], pos
    may be None = every packed row was traversed, keep flags per packed CSR slot; rows past sum(len) come out zero)."""

    @staticmethod
    def forward(ctx, yf, yr, self_term, trees, pos, keep_f, keep_r, M, drop_p, seed, seed_dev):
        H = yf.shape[1]
        P = _lib.ptr
        yf = yf.to(torch.float32).contiguous()
        yr = yr.to(torch.float32).contiguous() if yr is not None else None
        st = self_term.to(torch.float32).contiguous() if self_term is not None else None
        N = trees.N if trees.packed else trees.B * trees.T
        if st is not None and tuple(st.shape) != (N, H):
            raise ValueError("full_agg: self_term %s does not fit %d rows of width %d" % (tuple(st.shape), N, H))
        out = torch.empty((N, H), dtype=torch.float32, device=yf.device)
        if trees.packed:
            _lib.check(_lib.lib().gcnpt_full_agg_fwd_packed(_lib.stream(), P(yf), P(yr), P(st), P(pos), P(trees.row_ptr), P(trees.col_idx),
                                                            P(trees.label), P(keep_f), P(keep_r), trees.n_live_ptr(), trees.N, trees.nnz_cap, H,
                                                            int(M), P(out), float(drop_p), int(seed), P(seed_dev)))
        else:
            _lib.check(_lib.lib().gcnpt_full_agg_fwd(_lib.stream(), P(yf), P(yr), P(st), P(pos), P(trees.row_ptr), P(trees.col_idx), P(trees.label),
                                                     P(keep_f), P(keep_r), trees.B, trees.T, H, int(M), P(out), float(drop_p), int(seed),
                                                     P(seed_dev)))
        ctx.save_for_backward(out, pos, keep_f, keep_r)
        ctx.trees, ctx.M, ctx.rows = trees, int(M), (yf.shape[0], yr is not None, st is not None)
        ctx.scale = 1.0 / (1.0 - drop_p) if drop_p > 0 else 1.0
        return out

    @staticmethod
    def backward(ctx, g):
        out, pos, keep_f, keep_r = ctx.saved_tensors
        trees = ctx.trees
        H = out.shape[1]
        rows, has_r, has_self = ctx.rows
        P = _lib.ptr
        g = g.to(torch.float32).contiguous()
        dagg = torch.empty_like(out)
        dyf = torch.zeros((rows, H), dtype=torch.float32, device=out.device)
        dyr = torch.zeros((rows, H), dtype=torch.float32, device=out.device) if has_r else None
        if trees.packed:
            _lib.check(_lib.lib().gcnpt_full_agg_bwd_packed(_lib.stream(), P(g), P(out), P(pos), P(trees.row_ptr), P(trees.col_idx), P(trees.label),
                                                            P(keep_f), P(keep_r), trees.n_live_ptr(), trees.N, trees.nnz_cap, H, ctx.M, ctx.scale,
                                                            P(dagg), P(dyf), P(dyr)))
        else:
            _lib.check(_lib.lib().gcnpt_full_agg_bwd(_lib.stream(), P(g), P(out), P(pos), P(trees.row_ptr), P(trees.col_idx), P(trees.label),
                                                     P(keep_f), P(keep_r), trees.B, trees.T, H, ctx.M, ctx.scale, P(dagg), P(dyf), P(dyr)))
        return dyf, dyr, (dagg if has_self else None), None, None, None, None, None, None, None, None


def operand_format(compute):
    """(k-step width, torch dtype) of the traversal kernels' operands in precision `compute` (csrc/bilinear_kernels.hip: KSTEP, op_t)."""
    return (32, torch.bfloat16) if compute == _lib.BF16 else (16, torch.float32)


def padded_cols(src, k, dtype):
    """Zero-padded [M, ceil(W/k)*k] copy of src [M, W] in `dtype`."""
    M, W = src.shape
    out = torch.zeros((M, (W + k - 1) // k * k), dtype=dtype, device=src.device)
    out[:, :W] = src
    return out


def image_buffer(n_bytes, dev):
    """Uninitialised buffer for a fragment image of n_bytes bytes."""
    return torch.empty((n_bytes,), dtype=torch.uint8, device=dev)


class _BilinearFn(torch.autograd.Function):
    """y = sum_d e[:,d] * (x @ W3[d]) + e @ b3 (reference traverse_deprel, model/gcn.py:400-415) with the contraction on
    csrc/bilinear_kernels.hip in either precision: exact fp32 MFMA (the module's default) or bf16 operands with fp32 accumulation.
    The outer product e (x) x the reference materialises never exists.  The op is linear in each argument: dx is the same kernel on
    the transposed weight image, de the same per-relation products dotted with the upstream gradient, dW the token contraction
    of row-contraction fragment images with the gy fragments scaled by e in registers (gcnpt_bilinear_bwd_w)."""

    @staticmethod
    def forward(ctx, xt, e, weight, bias, compute):
        M, Tin = xt.shape
        D = e.shape[1]
        H = weight.shape[0] // D
        lib, st, dev = _lib.lib(), _lib.stream(), xt.device
        k, op_dtype = operand_format(compute)
        w32 = weight.detach().to(torch.float32).contiguous()
        img = image_buffer(lib.gcnpt_bilinear_packed_bytes(D, Tin, H, compute), dev)
        _lib.check(lib.gcnpt_bilinear_pack(st, _lib.ptr(w32), D, Tin, H, _lib.ptr(img), 0, compute))
        xb = padded_cols(xt.detach(), k, op_dtype)
        e32 = e.detach().to(torch.float32).contiguous()
        planes = torch.empty((lib.gcnpt_bilinear_planes(M, D, Tin, H, compute), M, H), dtype=torch.float32, device=dev)
        _lib.check(lib.gcnpt_bilinear_fwd(st, _lib.ptr(xb), _lib.ptr(e32), _lib.ptr(img), M, D, Tin, H, _lib.ptr(planes), compute))
        y = torch.addmm(planes.sum(0), e32, bias.detach().to(torch.float32).reshape(D, H))      # + e @ b3, gcn.py:413
        ctx.save_for_backward(xt, e, weight, bias, xb, img)
        ctx.compute = compute
        return y

    @staticmethod
    def backward(ctx, gy):
        xt, e, weight, bias, xb, img = ctx.saved_tensors
        compute = ctx.compute
        M, Tin = xt.shape
        D = e.shape[1]
        H = weight.shape[0] // D
        lib, st, dev = _lib.lib(), _lib.stream(), xt.device
        k, op_dtype = operand_format(compute)
        gy = gy.to(torch.float32).contiguous()
        x32, e32 = xt.to(torch.float32), e.to(torch.float32).contiguous()
        w32 = weight.detach().to(torch.float32).contiguous()
        b3 = bias.to(torch.float32).reshape(D, H)
        dx = de = dW = db = None
        on_kernel = bool(lib.gcnpt_bilinear_supported(D, H, Tin, compute))         # the transposed problem contracts over H
        if ctx.needs_input_grad[0]:
            if on_kernel:       # dx = sum_d e_d (gy @ W3[d]^T): the forward kernel on the transposed weight image
                imgT = image_buffer(lib.gcnpt_bilinear_packed_bytes(D, H, Tin, compute), dev)
                _lib.check(lib.gcnpt_bilinear_pack(st, _lib.ptr(w32), D, Tin, H, _lib.ptr(imgT), 1, compute))
                gyb = padded_cols(gy, k, op_dtype)
                planes = torch.empty((lib.gcnpt_bilinear_planes(M, D, H, Tin, compute), M, Tin), dtype=torch.float32, device=dev)
                _lib.check(lib.gcnpt_bilinear_fwd(st, _lib.ptr(gyb), _lib.ptr(e32), _lib.ptr(imgT), M, D, H, Tin, _lib.ptr(planes), compute))
                dx = planes.sum(0)
            else:
                dx = (torch.mm(gy, w32.reshape(D * Tin, H).t()).view(M, D, Tin) * e32.unsqueeze(2)).sum(1)
        if ctx.needs_input_grad[1]:
            # de[m,d] = (x[m] @ W3[d]) . gy[m] + gy[m] . b3[d]: the forward's per-relation products, dotted instead of summed
            planes = torch.empty((lib.gcnpt_bilinear_de_planes(M, D, Tin, H, compute), M, D), dtype=torch.float32, device=dev)
            _lib.check(lib.gcnpt_bilinear_bwd_e(st, _lib.ptr(xb), _lib.ptr(gy), _lib.ptr(img), M, D, Tin, H, _lib.ptr(planes), compute))
            de = torch.addmm(planes.sum(0), gy, b3.t())
        if ctx.needs_input_grad[2]:                                       # dW3[d] = (e_d * x)^T gy without the [M, D*Tin] outer product
            xI = image_buffer(lib.gcnpt_rows_image_bytes(M, Tin, compute), dev)
            gI = image_buffer(lib.gcnpt_rows_image_bytes(M, H, compute), dev)
            x32c = x32.contiguous()
            _lib.check(lib.gcnpt_rows_pack(st, _lib.ptr(x32c), M, Tin, _lib.ptr(xI), compute))
            _lib.check(lib.gcnpt_rows_pack(st, _lib.ptr(gy), M, H, _lib.ptr(gI), compute))
            eT = padded_cols(e32.t(), k, torch.float32)
            dW32 = torch.empty(weight.shape, dtype=torch.float32, device=dev)
            _lib.check(lib.gcnpt_bilinear_bwd_w(st, _lib.ptr(xI), _lib.ptr(gI), _lib.ptr(eT), M, D, Tin, H, _lib.ptr(dW32), compute))
            dW = dW32.to(weight.dtype)
        if ctx.needs_input_grad[3]:
            db = torch.mm(e32.t(), gy).reshape(-1).to(bias.dtype)
        return dx, de, dW, db, None


def bilinear_traverse(xt, e, weight, bias, compute_dtype=torch.bfloat16):
    """traverse_deprel of the reference for M compacted token rows: xt [M,Tin], e [M,D] relation vectors, weight [D*H,Tin] and
    bias [D*H] of the shared nn.Linear (read as W3 [D,Tin,H] / b3 [D,H], gcn.py:301-303).  float32 [M,H].  compute_dtype: float32 =
    exact fp32 MFMA, bfloat16 = bf16 operands with fp32 accumulation."""
    for t in (xt, e, weight, bias):
        _lib.require_gpu(t)
    return _BilinearFn.apply(xt, e, weight, bias, _lib.dtype_code(compute_dtype))


def bilinear_supported(D, Tin, H, compute_dtype=torch.bfloat16):
    return bool(_lib.lib().gcnpt_bilinear_supported(int(D), int(Tin), int(H), _lib.dtype_code(compute_dtype)))


def _zero_pad_row(grad):
    grad = grad.clone()
    grad[0].zero_()
    return grad


class _DiagLayerFn(torch.autograd.Function):
    """One diagonal_deprel layer (csrc/diag_kernels.hip): reference model/gcn.py:272-294 + 390-393.  `trees`: a PrunedTrees (h [B,T,H],
    deprel [B,T]) or a PackedTrees (h [N,H], deprel the packed [N] ids of PackedTrees.pack_ids; rows past sum(len) come out zero)."""

    @staticmethod
    def forward(ctx, h, emb, deprel, trees, drop_p, seed, seed_dev=None):
        for t in (h, emb, deprel):
            _lib.require_gpu(t)
        if trees.label is None:
            raise ValueError("diagonal_deprel needs the adjacency values: build the trees with want_label=True")
        B, T = trees.B, trees.T
        H = h.shape[-1]
        N = trees.N if trees.packed else B * T
        if h.numel() != N * H or emb.shape != (constant.N_DEPREL, H) or deprel.numel() != N:
            raise ValueError("diag layer: h %s, table %s, deprel %s do not fit the trees' %d rows" %
                             (tuple(h.shape), tuple(emb.shape), tuple(deprel.shape), N))
        if trees.packed and trees.rowT_ptr is None and any(ctx.needs_input_grad[:2]):
            raise ValueError("diagonal_deprel's backward needs the transposed pattern: build the packed trees with want_transpose=True")
        h = h.contiguous()
        E = emb.detach().float().contiguous()
        deprel = deprel.contiguous()
        out = torch.empty_like(h)
        if trees.packed:
            _lib.check(_lib.lib().gcnpt_diag_layer_fwd_packed(_lib.stream(), _lib.ptr(h), _lib.dtype_code(h.dtype), _lib.ptr(E), _lib.ptr(deprel),
                                                              _lib.ptr(trees.row_ptr), _lib.ptr(trees.col_idx), _lib.ptr(trees.label),
                                                              trees.n_live_ptr(), trees.N, trees.nnz_cap, H, _lib.ptr(out), float(drop_p),
                                                              int(seed), _lib.ptr(seed_dev)))
        else:
            _lib.check(_lib.lib().gcnpt_diag_layer_fwd(_lib.stream(), _lib.ptr(h), _lib.dtype_code(h.dtype), _lib.ptr(E), _lib.ptr(deprel),
                                                       _lib.ptr(trees.row_ptr), _lib.ptr(trees.col_idx), _lib.ptr(trees.label), B, T, H,
                                                       _lib.ptr(out), float(drop_p), int(seed), _lib.ptr(seed_dev)))
        ctx.trees, ctx.scale = trees, (1.0 / (1.0 - drop_p) if drop_p > 0 else 1.0)
        ctx.save_for_backward(h, out, E, deprel)
        return out

    @staticmethod
    def backward(ctx, gout):
        h, out, E, deprel = ctx.saved_tensors
        trees = ctx.trees
        B, T, H = trees.B, trees.T, h.shape[-1]
        gout = gout.to(h.dtype).contiguous()
        dh = torch.empty_like(h)
        dE = torch.zeros_like(E)
        args = (_lib.stream(), _lib.ptr(gout), _lib.ptr(out), _lib.ptr(h), _lib.dtype_code(h.dtype), _lib.ptr(E), _lib.ptr(deprel),
                _lib.ptr(trees.row_ptr), _lib.ptr(trees.col_idx), _lib.ptr(trees.label), _lib.ptr(trees.rowT_ptr), _lib.ptr(trees.colT_idx))
        if trees.packed:
            _lib.check(_lib.lib().gcnpt_diag_layer_bwd_packed(*args, trees.n_live_ptr(), trees.N, trees.nnz_cap, H, _lib.ptr(dh), _lib.ptr(dE),
                                                              ctx.scale))
        else:
            _lib.check(_lib.lib().gcnpt_diag_layer_bwd(*args, B, T, H, _lib.ptr(dh), _lib.ptr(dE), ctx.scale))
        return dh, dE, None, None, None, None, None


def diag_layer(h, deprel_table, deprel, trees, drop_p=0.0, seed=0, seed_dev=None):
    """dropout(relu(((F (E[deprel] * h)) + (R (E[deprel+42] * h)) + E[84] * h) / (deg + 1))) for h [B,T,H] (fp32 or bf16), or -- `trees` a
    PackedTrees -- token-packed h [N,H] with packed `deprel` [N]."""
    return _DiagLayerFn.apply(h, deprel_table, deprel, trees, drop_p, seed, seed_dev)
