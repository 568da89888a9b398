"""
The reference's layer loop (model/gcn.py:266-393) as one autograd op over the per-layer kernels of include/gcnpt.h: `gcn_layers` (and its
one-layer form `gcn_layer`), with the packed weight images (`WeightPack`) and, on request, the three masked poolings fused onto the stack.
"""
import ctypes

import torch

from .. import _lib
from .pooling import _check_positions, pool3_backward, pool3_forward, pool_kind
from .tree import PackedTrees, PrunedTrees


def _row_dims(h, trees, what):
    """(B, T) as the C-ABI wants them, rows, leading shape.  Padded: h is [B,T,W] and the trees are for [B,T].  Token-packed
    (PackedTrees): h is [N,W]; the entry points then take B = N, T = 0 (include/gcnpt.h, gcnpt_pack_trees)."""
    if trees.packed:
        if h.dim() != 2 or h.shape[0] != trees.N:
            raise RuntimeError("%s: packed trees hold %d rows but the inputs are %s" % (what, trees.N, tuple(h.shape)))
        return trees.N, 0, trees.N, (trees.N,)
    if h.dim() != 3 or (h.shape[0], h.shape[1]) != (trees.B, trees.T):
        raise RuntimeError("%s: inputs are %s but the adjacency is for [%d,%d]" % (what, tuple(h.shape), trees.B, trees.T))
    return trees.B, trees.T, trees.B * trees.T, (trees.B, trees.T)


def gcn_layer(h, weight, bias, trees, drop_p=0.0, seed=0, compute_dtype=torch.float32, out_dtype=None, no_adj=False, seed_dev=None):
    """
    Functional form of one iteration of the reference's layer loop: out = dropout(relu((((A+I) h) W^T + 2 b) / (deg + 1)))
    (model/gcn.py:269-271, 390-393), as a one-layer gcn_layers.  h [B,T,Din] (float32 or bfloat16, CUDA), weight [H,Din],
    bias [H] (nn.Linear layout), trees: PrunedTrees.  compute_dtype float32 = exact fp32 MFMA, bfloat16 = bf16 operands with
    fp32 accumulation; out_dtype (default: h's) is float32 whenever compute_dtype is.  seed_dev: optional int64 [1] CUDA tensor
    added to `seed` on the device (advance it between replays of a captured graph to get fresh dropout masks).
    """
    return gcn_layers(h, [weight], [bias], trees, [drop_p], [seed], compute_dtype, out_dtype or h.dtype, no_adj, seed_dev)


class WeightPack(object):
    """The layer weights' MFMA-order images (gcnpt_pack_weights_multi) as a request that another launch can carry as a side job:
    `prune_to_csr(..., pack=wp)` / `TreeCache.batch(..., pack=wp)` build the trees and fill wp.wf / wp.wb in ONE launch
    (include/gcnpt.h, gcnpt_prune_to_csr_pack); the layer op then takes the images from the request when they still belong to the
    current weights (same storage, same version counters), and packs as usual otherwise."""

    def __init__(self, Ws, compute, dev):
        lib = _lib.lib()
        self.key = WeightPack.key_of(Ws, compute, dev)
        self.compute = compute
        self.dims = [tuple(w.shape) for w in Ws]
        self.w32 = [w.detach().to(torch.float32).contiguous() for w in Ws]
        u8 = dict(dtype=torch.uint8, device=dev)
        self.wf = [torch.empty((lib.gcnpt_packed_bytes(h, k, compute),), **u8) for h, k in self.dims]
        self.wb = [torch.empty((lib.gcnpt_packed_bytes(k, h, compute),), **u8) for h, k in self.dims]
        self.launched = False                      # set by the launch that carried the request

    @staticmethod
    def key_of(Ws, compute, dev):
        return (compute, str(dev)) + tuple((w.data_ptr(), w._version, tuple(w.shape)) for w in Ws)

    def c_args(self):
        """The trailing arguments of gcnpt_pack_weights_multi / gcnpt_*_pack."""
        ints = _lib.int_array
        return (len(self.dims), _lib.ptr_array(self.w32), ints([h for h, _ in self.dims]), ints([k for _, k in self.dims]), self.compute,
                _lib.ptr_array(self.wf), _lib.ptr_array(self.wb))


class _GCNLayersFn(torch.autograd.Function):
    """The reference's layer loop (model/gcn.py:266-393) as ONE autograd op over the per-layer kernels: one launch packs
    every layer's weights, one launch per layer and direction does the layer, one launch at the end of the backward sweep
    computes every layer's weight gradient (2L + 2 launches instead of 4L)."""

    @staticmethod
    def forward(ctx, x, trees, cfg, *params):
        Ws, bs = params[0::2], params[1::2]
        L = len(Ws)
        B, T, rows, lead = _row_dims(x, trees, "GCN layers")
        Din = x.shape[-1]
        dims = [tuple(w.shape) for w in Ws]                           # (H_l, Din_l)
        for l, (h, k) in enumerate(dims):
            if k != (Din if l == 0 else dims[l - 1][0]):
                raise RuntimeError("GCN layer %d: weight %s does not fit an input of width %d" % (l, (h, k), Din if l == 0 else dims[l - 1][0]))
        lib, st, dev, compute = _lib.lib(), _lib.stream(), x.device, cfg["compute"]
        x = x.contiguous()
        b32 = [b.detach().to(torch.float32).contiguous() for b in bs]
        u8 = dict(dtype=torch.uint8, device=dev)
        ints = _lib.int_array
        # the fragment-order images only change when an optimizer step (or a load_state_dict) rewrites a weight in place, which bumps
        # the tensor's version counter: a module passes its cache and eval() / gradient-accumulation forwards skip the pack launch;
        # a training step that builds its trees in the same forward gets them from that launch's side job (WeightPack)
        cache = None if torch.cuda.is_current_stream_capturing() else cfg.get("wcache")     # (a captured step must contain its pack;
        # the module passes its cache only where reuse is safe, see GCN._cache_usable)
        key = WeightPack.key_of(Ws, compute, dev)
        pre = cfg.get("prepacked")
        if pre is not None and pre.key == key and pre.launched:
            wf, wb = pre.wf, pre.wb
            if cache is not None:
                cache.update(key=key, wf=wf, wb=wb)
        elif cache is not None and cache.get("key") == key:
            wf, wb = cache["wf"], cache["wb"]
        else:
            pk = WeightPack(Ws, compute, dev)
            _lib.check(lib.gcnpt_pack_weights_multi(st, *pk.c_args()))
            wf, wb = pk.wf, pk.wb
            if cache is not None:
                cache.update(key=key, wf=wf, wb=wb)
        need_w = any(p.requires_grad for p in params)
        g_ell = trees.empty_ell() if cfg["no_adj"] else trees.ell
        outs = [torch.empty(lead + (H,), dtype=cfg["out_dtype"] if l == L - 1 else cfg["mid_dtype"], device=dev) for l, (H, _) in enumerate(dims)]
        # the S images: for the weight gradients, and for every layer that takes the wide form (staged through its image even in
        # a no-grad forward; gcnpt_layer_fwd_needs_s_frag answers on the host)
        s_frag = [torch.empty((lib.gcnpt_frag_bytes(rows, K, compute),), **u8)
                  if need_w or lib.gcnpt_layer_fwd_needs_s_frag(rows, K, H, compute) == 1 else None for H, K in dims]
        # every layer's launch from ONE native call (gcnpt_layers_fwd): no interpreter time between the launches
        _lib.check(lib.gcnpt_layers_fwd(
            st, L, _lib.ptr(x), _lib.dtype_code(x.dtype), _lib.ptr_array(wf), _lib.ptr_array(b32), _lib.ptr(trees.row_ptr),
            _lib.ptr(trees.col_idx), _lib.ptr(g_ell), _lib.ptr(trees.ell), B, T, ints([k for _, k in dims]), ints([h for h, _ in dims]),
            _lib.ptr_array(outs), ints([_lib.dtype_code(o.dtype) for o in outs]), compute, (ctypes.c_float * L)(*cfg["drop_p"]),
            (ctypes.c_uint64 * L)(*cfg["seed"]), _lib.ptr_array(s_frag), _lib.ptr(cfg.get("seed_dev"))))
        if cfg.get("acts") is not None:
            cfg["acts"].extend(outs)          # every layer's stored output (what the backward reads): tests drive the oracle's backward with them
        ctx.trees, ctx.cfg, ctx.dims, ctx.shape, ctx.need_w = trees, cfg, dims, (B, T, Din, L), need_w
        ctx.rows, ctx.lead = rows, lead
        ctx.x_dtype = x.dtype
        ctx.param_dtypes = [p.dtype for p in params]
        ctx.save_for_backward(*outs, *wb, *(s_frag if need_w else []))
        pool = cfg.get("pool")
        if pool is None:
            return outs[-1]
        # the consumer of the stack, fused into the op (gcn.py:114-121): the three masked poolings in one pass over h_L -- packed rows
        # where they lie (no unpack_rows, no [B,T,H] tensor).  Its backward then hands the top layer dZ instead of dh, and that layer
        # gathers one row per neighbour, not three
        sp, op, kind = pool
        pm = trees.pool_mask.contiguous()
        pooled, argmax = pool3_forward(outs[-1], trees, pm, sp, op, kind)
        ctx.pool = (pm, sp, op, argmax, kind)
        return pooled

    @staticmethod
    def backward(ctx, gout):
        B, T, Din, L = ctx.shape
        saved = ctx.saved_tensors
        outs, wb, s_frag = saved[:L], saved[L:2 * L], saved[2 * L:]
        trees, cfg, dims = ctx.trees, ctx.cfg, ctx.dims
        lib, st, dev, compute = _lib.lib(), _lib.stream(), gout.device, cfg["compute"]
        want_w = ctx.need_w and any(ctx.needs_input_grad[3:])
        g_ellT = trees.empty_ell() if cfg["no_adj"] else trees.ellT
        u8 = dict(dtype=torch.uint8, device=dev)
        z_frag, dWs, dbs = [None] * L, [None] * L, [None] * L
        scales = [1.0 / (1.0 - p) if p > 0 else 1.0 for p in cfg["drop_p"]]
        pool = getattr(ctx, "pool", None) if cfg.get("pool") is not None else None
        if pool is None:
            g = gout.to(outs[-1].dtype).contiguous()
        else:
            pm, sp, op, argmax, kind = pool
            # dZ of the top layer, straight from the pooling's backward
            g = pool3_backward(gout, trees, outs[-1].shape, outs[-1].dtype, pm, sp, op, argmax, kind, y=outs[-1], ell=trees.ell, scale=scales[-1])
        in_dtypes = [ctx.x_dtype if l == 0 else outs[l - 1].dtype for l in range(L)]
        dhs = [torch.empty(ctx.lead + (K,), dtype=in_dtypes[l], device=dev) if (l > 0 or ctx.needs_input_grad[0]) else None
               for l, (_, K) in enumerate(dims)]
        if want_w:
            z_frag = [torch.empty((lib.gcnpt_frag_bytes(ctx.rows, H, compute),), **u8) for H, _ in dims]
            dWs = [torch.empty((H, K), dtype=torch.float32, device=dev) for H, K in dims]       # cleared by the sweep's launches
            dbs = [torch.empty((H,), dtype=torch.float32, device=dev) for H, _ in dims]
        ints = _lib.int_array
        # the backward sweep and all weight gradients from ONE native call (gcnpt_layers_bwd; _bwd_dz: its first tensor already is dZ)
        _lib.check((lib.gcnpt_layers_bwd if pool is None else lib.gcnpt_layers_bwd_dz)(
            st, L, _lib.ptr(g), _lib.ptr_array(list(outs)), ints([_lib.dtype_code(o.dtype) for o in outs]), _lib.ptr_array(list(wb)),
            _lib.ptr(trees.ell), _lib.ptr(trees.rowT_ptr), _lib.ptr(trees.colT_idx), _lib.ptr(g_ellT), B, T, ints([k for _, k in dims]),
            ints([h for h, _ in dims]), _lib.ptr_array(dhs), ints([_lib.dtype_code(t) for t in in_dtypes]), compute,
            (ctypes.c_float * L)(*scales), _lib.ptr_array(z_frag) if want_w else None, _lib.ptr_array(list(s_frag)) if want_w else None,
            _lib.ptr_array(dWs) if want_w else None, _lib.ptr_array(dbs) if want_w else None))
        g = dhs[0]
        grads = [None] * (2 * L)
        if want_w:
            for l in range(L):
                grads[2 * l] = dWs[l].to(ctx.param_dtypes[2 * l])
                grads[2 * l + 1] = dbs[l].to(ctx.param_dtypes[2 * l + 1])
        return (g if ctx.needs_input_grad[0] else None, None, None) + tuple(grads)


def gcn_layers(x, weights, biases, trees, drop_p=None, seeds=None, compute_dtype=torch.float32, out_dtype=torch.float32, no_adj=False,
               seed_dev=None, wcache=None, pool=None, prepacked=None, acts=None):
    """
    The reference's whole layer loop (model/gcn.py:266-393) over the per-layer kernels.  x [B,T,Din] float32/bfloat16 CUDA, or
    token-packed rows [N,Din] with a PackedTrees; weights / biases: lists of the nn.Linear parameters (any widths that chain); drop_p[l]: dropout applied to the output of
    layer l (0 for the last); acts: None or a list that receives every layer's stored output; wcache: an empty dict the caller keeps -- the packed weight images are reused while the weights'
    version counters stand still; pool: see below.  compute_dtype float32 = exact fp32 MFMA (activations stay float32), bfloat16 = bf16 operands
    and bf16 activations between the layers, fp32 accumulation; the last layer's output has out_dtype.
    """
    if not isinstance(trees, (PrunedTrees, PackedTrees)):
        raise TypeError("trees must be a PrunedTrees (see model.tree.prune_to_csr / adj_to_csr) or a PackedTrees (PrunedTrees.pack)")
    _lib.require_gpu(x)
    L = len(weights)
    compute = _lib.dtype_code(compute_dtype)
    if compute == _lib.F32:
        x, out_dtype = (x.float() if x.dtype != torch.float32 else x), torch.float32
    cfg = dict(drop_p=[float(p) for p in (drop_p or [0.0] * L)], seed=[int(s) for s in (seeds or [0] * L)], compute=compute,
               mid_dtype=torch.float32 if compute == _lib.F32 else torch.bfloat16, out_dtype=out_dtype, no_adj=bool(no_adj),
               seed_dev=seed_dev, wcache=wcache, pool=None, prepacked=prepacked, acts=acts)
    if pool is not None:
        # pool = (subj_pos, obj_pos, 'max' | 'avg' | 'sum'): the op returns float32 [B, 3H] = pool3(h_L, trees.pool_mask, subj_pos, obj_pos)
        # instead of h_L; with a PackedTrees = pool3_packed(h_L, trees, subj_pos, obj_pos), the positions being the padded [B,T] tensors
        sp, op, kind = pool
        _check_positions("gcn_layers(pool=...)", sp, op, trees)
        cfg["pool"] = (sp.contiguous(), op.contiguous(), pool_kind(kind))
    params = [t for wb in zip(weights, biases) for t in wb]
    return _GCNLayersFn.apply(x, trees, cfg, *params)


def gcn_layers_with_acts(x, weights, biases, trees, **kw):
    """gcn_layers plus the list of every layer's stored output (detached; the last one is the op's result before any pooling)."""
    acts = []
    out = gcn_layers(x, weights, biases, trees, acts=acts, **kw)
    return out, [a.detach() for a in acts]
