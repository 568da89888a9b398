"""
The two embedding front ends of GCN.forward (reference model/gcn.py:235-241): `_embed`, an nn.Embedding lookup with a one-launch backward,
and `embed_inputs`, the whole front end -- lookups, cat, both dropouts, the bf16 cast and pack_rows -- over csrc/embed_kernels.hip.
"""
import torch
import torch.nn as nn

from .. import _lib
from .tree import PackedTrees


class _EmbedFn(torch.autograd.Function):
    """nn.Embedding lookup (model/gcn.py:235-239) whose backward is ONE index_add_ of float atomics.  PyTorch-ROCm 2.10's own
    embedding backward takes ~140 us per table at the 1.5-5 k indices of a batch (embedding_backward_feature_kernel: three
    tables = half of the no-LSTM training step) and above 3072 indices a rocPRIM sort path that faults when replayed in a
    hipGraph; same sums, same zero row for padding_idx.
    sparse = True: the gradient is a ROW-SPARSE tensor instead (indices = the batch's token ids, values = their gradient rows; rows
    >= topn and the padding row zeroed, gcn.py:84-88): a data-parallel loop then exchanges (row ids, rows) with
    shard.SparseRowExchange instead of all-reducing the dense [V, E] table."""

    @staticmethod
    def forward(ctx, weight, idx, padding_idx, sparse=False, topn=None):
        ctx.save_for_backward(idx)
        ctx.table, ctx.pad, ctx.sparse, ctx.topn = tuple(weight.shape), padding_idx, sparse, topn
        return torch.nn.functional.embedding(idx, weight)

    @staticmethod
    def backward(ctx, g):
        (idx,) = ctx.saved_tensors
        flat, rows = idx.reshape(-1), g.reshape(-1, g.shape[-1])
        if ctx.sparse:
            keep = torch.ones_like(flat, dtype=torch.bool)
            if ctx.pad is not None:
                keep &= flat != ctx.pad
            if ctx.topn is not None:
                keep &= flat < ctx.topn
            rows = rows * keep.unsqueeze(1).to(rows.dtype)
            return torch.sparse_coo_tensor(flat.unsqueeze(0), rows, size=ctx.table), None, None, None, None
        gw = torch.zeros(ctx.table, dtype=g.dtype, device=g.device)
        gw.index_add_(0, flat, rows)
        if ctx.pad is not None:
            gw[ctx.pad].zero_()
        return gw, None, None, None, None


def _embed(table, idx, sparse=False, topn=None):
    """table: nn.Embedding.  Same result as table(idx)."""
    if idx.is_cuda and table.weight.requires_grad and torch.is_grad_enabled():
        return _EmbedFn.apply(table.weight, idx, table.padding_idx, sparse, topn)
    return table(idx)


class _EmbedInputsFn(torch.autograd.Function):
    """The front end of GCN.forward (model/gcn.py:235-241) as ONE autograd node over gcnpt_embed_fwd / gcnpt_embed_bwd
    (csrc/embed_kernels.hip): lookups, cat, word-type and element dropout, the bf16 cast and pack_rows in one launch; the backward
    recomputes the dropout decisions from the seeds and scatters g into the tables in one launch."""

    @staticmethod
    def forward(ctx, words, pos, ner, W0, W1, W2, cfg):
        lib, st, P = _lib.lib(), _lib.stream(), _lib.ptr
        dense = words.dim() > 2
        B, T = words.shape[0], words.shape[1]
        dev = words.device
        words = (words.detach().to(torch.float32) if dense else words).contiguous()
        pos = pos.contiguous() if W1 is not None else None
        ner = ner.contiguous() if W2 is not None else None
        t0 = None if dense else W0.detach().to(torch.float32).contiguous()
        t1 = W1.detach().to(torch.float32).contiguous() if W1 is not None else None
        t2 = W2.detach().to(torch.float32).contiguous() if W2 is not None else None
        dims = (0 if dense else t0.shape[0], t1.shape[0] if t1 is not None else 0, t2.shape[0] if t2 is not None else 0,
                words.shape[2] if dense else t0.shape[1], t1.shape[1] if t1 is not None else 0, t2.shape[1] if t2 is not None else 0)
        Din = sum(dims[3:])
        trees = cfg["trees"]
        cu, n_rows = (trees.cu_seqlens, trees.N) if trees is not None else (None, 0)
        out = torch.empty((n_rows, Din) if trees is not None else (B, T, Din), dtype=cfg["out_dtype"], device=dev)
        seed_dev = cfg["seed_dev"]
        lay = (*dims, P(cu), B, T, n_rows)
        rng = (cfg["p_emb"], cfg["p_in"], cfg["seeds"][0], cfg["seeds"][1], P(seed_dev))
        _lib.check(lib.gcnpt_embed_fwd(st, None if dense else P(words), P(words) if dense else None, P(pos), P(ner), P(t0), P(t1), P(t2),
                                       *lay, P(out), _lib.dtype_code(out.dtype), *rng, P(cfg["status"])))
        ctx.save_for_backward(None if dense else words, pos, ner)
        ctx.keep = (cu, seed_dev)                # (tensors the launch arguments point at)
        ctx.lay, ctx.rng, ctx.cfg, ctx.dense = lay, rng, cfg, dense
        ctx.dtypes = [w.dtype if w is not None else None for w in (W0, W1, W2)]
        ctx.src_dtype = cfg["src_dtype"]
        return out

    @staticmethod
    def backward(ctx, g):
        words, pos, ner = ctx.saved_tensors
        lib, st, P = _lib.lib(), _lib.stream(), _lib.ptr
        V0, V1, V2, E0, E1, E2 = ctx.lay[:6]
        B, T = ctx.lay[7], ctx.lay[8]
        cfg = ctx.cfg
        if g.dtype not in (torch.float32, torch.bfloat16):
            g = g.float()
        g = g.contiguous()
        f32 = dict(dtype=torch.float32, device=g.device)
        need = ctx.needs_input_grad
        d_dense = torch.empty((B, T, E0), **f32) if (ctx.dense and need[0]) else None
        sparse = bool(cfg["sparse"]) and not ctx.dense and need[3]
        d0 = torch.empty((V0, E0), **f32) if (not ctx.dense and need[3] and not sparse) else None      # cleared by the call
        rows = torch.empty((B * T, E0), **f32) if sparse else None
        d1 = torch.empty((V1, E1), **f32) if (E1 > 0 and need[4]) else None
        d2 = torch.empty((V2, E2), **f32) if (E2 > 0 and need[5]) else None
        if any(t is not None for t in (d_dense, d0, rows, d1, d2)):
            pad, topn = cfg["padding_idx"], cfg["topn"]
            _lib.check(lib.gcnpt_embed_bwd(st, P(g), _lib.dtype_code(g.dtype), P(words), P(pos), P(ner), *ctx.lay, *ctx.rng,
                                           -1 if pad is None else int(pad), 0 if topn is None else min(int(topn), 2 ** 31 - 1), P(d0), P(rows), P(d_dense),
                                           P(d1), P(d2)))
        if sparse:
            d0 = torch.sparse_coo_tensor(words.reshape(1, -1), rows.to(ctx.dtypes[0]), size=(V0, E0))
        elif d0 is not None:
            d0 = d0.to(ctx.dtypes[0])
        return (d_dense.to(ctx.src_dtype) if d_dense is not None else None, None, None, d0, d1.to(ctx.dtypes[1]) if d1 is not None else None,
                d2.to(ctx.dtypes[2]) if d2 is not None else None, None)


def embed_inputs(words, pos, ner, emb, pos_emb, ner_emb, trees=None, p_emb=0., p_in=0., seeds=(0, 0), seed_dev=None,
                 out_dtype=torch.float32, sparse=False, topn=None, status=None):
    """
    dropout([emb_dropout(emb[words]) | pos_emb[pos] | ner_emb[ner]]) -- the input of the layer stack (model/gcn.py:235-241) -- as one
    launch forward and one backward.  words / pos / ner: the loader's int64 [B,T] id tensors (CUDA); a float `words` [B,T,E0] is a dense
    word source that skips the lookup (gcn.py:235-236; no word-type dropout then).  emb / pos_emb / ner_emb: nn.Embedding modules or
    their float weight tensors (a module's padding_idx row gets no gradient); pos_emb / ner_emb may be None (no such segment).
    Returns [B,T,Din], or token-packed rows [N,Din] when `trees` is a PackedTrees: PackedTrees.pack_rows of the padded result bit for
    bit, under dropout too.  p_emb: word-TYPE dropout (one decision per sentence and word id, model/dropouts.py:23-39); p_in: element
    dropout; seeds = (seed_emb, seed_in), plus the optional device word seed_dev (int64 [1]) for captured graphs.  The result is
    (v / (1-p_emb)) / (1-p_in) or +0.0, exactly.  out_dtype float32 or bfloat16.  sparse / topn: the word table's gradient as a
    row-sparse tensor / limited to rows < topn (_EmbedFn).  status: optional int32 [1] CUDA tensor that receives a bit per table
    (1 word, 2 POS, 4 NER) when an id lies outside it -- such a segment is zero and gets no gradient.
    """
    tables = [(t.weight, t.padding_idx) if isinstance(t, nn.Embedding) else (t, None) for t in (emb, pos_emb, ner_emb)]
    W0, W1, W2 = (w for w, _ in tables)
    dense = torch.is_tensor(words) and words.dim() > 2
    if dense:
        W0 = None
    elif W0 is None:
        raise TypeError("embed_inputs: word ids need the word table")
    for t in (words, pos if W1 is not None else None, ner if W2 is not None else None, W0, W1, W2, seed_dev, status):
        if t is not None and not (torch.is_tensor(t) and t.is_cuda):
            raise TypeError("embed_inputs runs on the GPU only (got %s); there is no CPU path" % (t.device if torch.is_tensor(t) else type(t)))
    if trees is not None and not isinstance(trees, PackedTrees):
        raise TypeError("embed_inputs: trees must be None (padded rows) or a PackedTrees (token-packed rows)")
    if words.dim() not in (2, 3) or (not dense and words.dtype != torch.int64) or (dense and not words.is_floating_point()):
        raise TypeError("embed_inputs: words must be int64 [B,T] or a float [B,T,E0] source, got %s %s" % (words.dtype, tuple(words.shape)))
    for name, ids, w in (("pos", pos, W1), ("ner", ner, W2)):
        if w is not None and (ids is None or ids.dtype != torch.int64 or tuple(ids.shape) != tuple(words.shape[:2])):
            raise TypeError("embed_inputs: %s must be int64 %s" % (name, tuple(words.shape[:2])))
    if trees is not None and (trees.B, trees.T) != tuple(words.shape[:2]):
        raise RuntimeError("embed_inputs: packed trees are for a [%d,%d] batch, the ids are %s" % (trees.B, trees.T, tuple(words.shape)))
    _lib.dtype_code(out_dtype)
    if seed_dev is not None and (p_emb > 0 or p_in > 0) and torch.is_grad_enabled():
        seed_dev = seed_dev.clone()            # the backward must see the word this forward saw, whatever advances it in between
    cfg = dict(trees=trees, p_emb=float(p_emb), p_in=float(p_in), seeds=(int(seeds[0]), int(seeds[1])), seed_dev=seed_dev, out_dtype=out_dtype,
               sparse=bool(sparse), topn=topn, padding_idx=tables[0][1], status=status,
               src_dtype=words.dtype)
    return _EmbedInputsFn.apply(words, pos if W1 is not None else None, ner if W2 is not None else None, W0, W1, W2, cfg)
