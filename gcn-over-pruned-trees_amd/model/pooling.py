"""
The masked poolings of GCNRelationModel.forward (reference model/gcn.py:116-121, 473-483) over csrc/pool_kernels.hip: one pair of launch
helpers for padded [B,T,H] and token-packed [N,H] rows, which the pooling op here and the layer-stack op (model/layers.py) share.
"""
import torch

from .. import _lib
from ..utils import constant
from .tree import PackedTrees


def pool_kind(type):
    """The kernels' code of a pooling type; anything but 'max' / 'avg' is the sum, as in the reference's pool()."""
    return {'max': 0, 'avg': 1}.get(type, 2)


def _row_layout(trees, shape):
    """(token-packed?, sentences, the entry points' layout arguments) of rows of `shape`: [B,T,H] when `trees` is None or padded, else
    the [N,H] rows of a PackedTrees (sentence b pools rows cu_seqlens[b] .. cu_seqlens[b+1]-1)."""
    if trees is not None and trees.packed:
        N, H = shape
        return True, trees.B, (_lib.ptr(trees.cu_seqlens), trees.B, trees.T, N, H)
    B, T, H = shape
    return False, B, (B, T, H)


def pool3_forward(h, trees, pm, sp, op, kind):
    """One pass over contiguous rows h: (float32 [B, 3H] = [pool(h, pm) | pool(h, sp != 0) | pool(h, op != 0)], int32 [B,3,H] argmax
    for 'max', else None)."""
    lib, P = _lib.lib(), _lib.ptr
    packed, nb, layout = _row_layout(trees, h.shape)
    H = h.shape[-1]
    out = torch.empty((nb, 3 * H), dtype=torch.float32, device=h.device)
    argmax = torch.empty((nb, 3, H), dtype=torch.int32, device=h.device) if kind == 0 else None
    fn = lib.gcnpt_pool3_fwd_packed if packed else lib.gcnpt_pool3_fwd
    _lib.check(fn(_lib.stream(), P(h), _lib.dtype_code(h.dtype), P(pm), P(sp), P(op), *layout, kind, P(out), P(argmax)))
    return out, argmax


def pool3_backward(g, trees, shape, dtype, pm, sp, op, argmax, kind, y=None, ell=None, scale=1.0):
    """The gradient of pool3_forward's rows (`shape`, `dtype`) from g [B, 3H].  With y -- the stored output of the GCN layer that
    produced the rows -- the trees' ELL heads and that layer's dropout scale, the result is the layer's dZ instead of dh."""
    lib, P = _lib.lib(), _lib.ptr
    packed, _, layout = _row_layout(trees, shape)
    dh = torch.empty(shape, dtype=dtype, device=g.device)
    g = g.to(torch.float32).contiguous()
    if y is None:
        fn, through = (lib.gcnpt_pool3_bwd_packed if packed else lib.gcnpt_pool3_bwd), ()
    else:
        fn, through = (lib.gcnpt_pool3_bwd_dz_packed if packed else lib.gcnpt_pool3_bwd_dz), (P(y), P(ell), scale)
    _lib.check(fn(_lib.stream(), P(g), P(argmax), P(pm), P(sp), P(op), *layout, kind, *through, P(dh), _lib.dtype_code(dtype)))
    return dh


class _Pool3Fn(torch.autograd.Function):
    """[pool(h, pool_mask) | pool(h, subj_pos != 0) | pool(h, obj_pos != 0)] in one pass (csrc/pool_kernels.hip); trees: the
    PackedTrees of token-packed rows, None for padded ones."""

    @staticmethod
    def forward(ctx, h, trees, pool_mask, subj_pos, obj_pos, kind):
        h = h.contiguous()
        pm = pool_mask.contiguous()
        sp, op = subj_pos.contiguous(), obj_pos.contiguous()
        out, argmax = pool3_forward(h, trees, pm, sp, op, kind)
        ctx.save_for_backward(pm, sp, op, argmax)
        ctx.kind, ctx.shape, ctx.h_dtype, ctx.trees = kind, tuple(h.shape), h.dtype, trees
        return out

    @staticmethod
    def backward(ctx, g):
        pm, sp, op, argmax = ctx.saved_tensors
        return pool3_backward(g, ctx.trees, ctx.shape, ctx.h_dtype, pm, sp, op, argmax, ctx.kind), None, None, None, None, None


def pool3(h, pool_mask, subj_pos, obj_pos, type='max'):
    """
    The three poolings of GCNRelationModel.forward (model/gcn.py:116-121) fused: returns float32 [B, 3H] =
    cat([pool(h, pool_mask), pool(h, subj_pos != 0), pool(h, obj_pos != 0)], dim=1) with pool() of model/gcn.py:473-483.
    h [B,T,H] float32/bfloat16 CUDA, pool_mask bool [B,T,1] (True = excluded), subj_pos / obj_pos int64 [B,T].
    """
    _lib.require_gpu(h)
    if pool_mask.dtype not in (torch.bool, torch.uint8) or subj_pos.dtype != torch.int64 or obj_pos.dtype != torch.int64:
        raise TypeError("pool3: pool_mask must be bool/uint8, subj_pos / obj_pos int64")
    return _Pool3Fn.apply(h, None, pool_mask, subj_pos, obj_pos, pool_kind(type))


def _check_positions(what, subj_pos, obj_pos, trees):
    """The position tensors of a pooling over `trees`' batch: the loader's padded int64 [B,T], whatever layout the rows have."""
    for name, t in (("subj_pos", subj_pos), ("obj_pos", obj_pos)):
        if t.dtype != torch.int64 or tuple(t.shape) != (trees.B, trees.T):
            raise TypeError("%s: %s must be int64 [%d,%d], got %s %s" % (what, name, trees.B, trees.T, t.dtype, tuple(t.shape)))


def pool3_packed(h, trees, subj_pos, obj_pos, type='max'):
    """
    pool3 on token-packed rows: h [N,H] float32/bfloat16 CUDA (N = trees.N rows, sentence b's token i at row cu_seqlens[b] + i), trees a
    PackedTrees (its pool_mask [N,1] is the tree mask), subj_pos / obj_pos the loader's padded int64 [B,T].  Returns float32 [B, 3H];
    differentiable (the gradient of h is written completely, rows past sum(len) as zeros).
    Equal to pool3(trees.unpack_rows(h), <padded pool mask>, subj_pos, obj_pos) bit for bit when every pad slot of the positions is
    non-zero, which is what the loader writes (150, data/loader.py:120-121): a pad slot with position 0 is a subject / object token of
    value zero in the padded form and does not exist in the packed form.
    """
    if not isinstance(trees, PackedTrees):
        raise TypeError("pool3_packed: trees must be a PackedTrees (PrunedTrees.pack, prune_to_csr_packed, TreeCache.batch_packed)")
    _lib.require_gpu(h)
    if h.dim() != 2 or h.shape[0] != trees.N:
        raise RuntimeError("pool3_packed: packed trees hold %d rows but h is %s" % (trees.N, tuple(h.shape)))
    _check_positions("pool3_packed", subj_pos, obj_pos, trees)
    return _Pool3Fn.apply(h, trees, trees.pool_mask, subj_pos, obj_pos, pool_kind(type))


def pool(h, mask, type='max'):
    """Reference model/gcn.py:473-483 (mask True = excluded)."""
    if type == 'max':
        return h.masked_fill(mask, -constant.INFINITY_NUMBER).max(1)[0]
    h = h.masked_fill(mask, 0)
    if type == 'avg':
        return h.sum(1) / (mask.size(1) - mask.float().sum(1))
    return h.sum(1)
