"""
Host-side mirror of the reference's model/gcn.py for the `regular` GCN path, running on MI355X kernels.

Same class names, constructor arguments, `opt` keys, parameter / state_dict names and forward()
signatures as the reference, so `from model.gcn import GCNClassifier` can be swapped for
`from gcn_over_pruned_trees_amd.model.gcn import GCNClassifier` in its trainer (model/trainer.py:82):

  GCNClassifier(opt, emb_matrix=None).forward(inputs) -> (logits [B,C], pooling_output [B,H])   gcn.py:15-36
  GCNRelationModel(opt, emb_matrix=None).forward(inputs) -> (outputs [B,H], h_out [B,H])        gcn.py:38-126
  GCN(opt, embeddings, mem_dim, num_layers).forward(adj, inputs) -> (h [B,T,H], mask [B,T,1])   gcn.py:128-395
  pool(h, mask, type)                                                                            gcn.py:473-483

What is different underneath: the tree pruning + adjacency build (gcn.py:96-110) is one device kernel
(model/tree.py here) and every iteration of the layer loop (gcn.py:266-393) is one fused HIP kernel per
direction, reached through the C-ABI of include/gcnpt.h.  Embeddings and the output MLP / classifier stay ordinary
PyTorch-ROCm modules, as in the reference, unless opt['gcn_native_embed'] / opt['gcn_native_head'] is set; so does the optional
BiLSTM unless opt['gcn_native_rnn'] is set.

New optional `opt` keys (defaults reproduce the reference): `gcn_dtype` = 'fp32' | 'bf16' (MFMA operand /
activation storage type inside the layer stack), `gcn_check_trees` = True (synchronise once per forward to
raise on malformed trees the way the reference does; False keeps the step free of host syncs), `gcn_packed` = False (True: the
layer loop runs on token-packed rows, sum(len) instead of B*T, padding only at the module boundary -- every adj_type: the relation-aware
variants then take any labelled PackedTrees, TreeCache.batch_packed's included, traverse every packed row and never synchronise),
`gcn_graph_rng` = False
(True: dropout seeds that survive hipGraph capture), `gcn_pool_handover` = True (layer stack + poolings as one op whose backward
hands the top layer its dZ), `gcn_pack_with_trees` = True (the tree launch also packs the weights in a training step),
`gcn_sparse_emb_grad` = False (True: the word-embedding table's gradient is a row-sparse tensor of the batch's token rows, for
shard.SparseRowExchange in a data-parallel loop), `gcn_reuse_packed_weights` = False (True: a forward may reuse the packed weight images of the previous one while the weights'
version counters stand still -- gradient accumulation, a frozen model; off by default because `p.data` updates do not bump them, in eval() either),
`gcn_native_rnn` = False (True: the C-GCN model's BiLSTM runs on the native recurrence of model/rnn.py with the lengths on the device, output
[B, T, 2H]) -- with `gcn_check_trees=False` a whole training step can be captured with torch.cuda.graph and replayed: the no-LSTM model as
it is (tests/test_gpu_parity.py::test_training_step_graph_capture), the C-GCN model with `gcn_native_rnn=True` (tests/test_gpu_lstm.py).
`gcn_native_embed` = False (True: the embedding front end of GCN.forward -- the three lookups, the cat, word-type and input dropout, the bf16
cast and, on PackedTrees, pack_rows -- is one launch forward and one backward, `embed_inputs` over csrc/embed_kernels.hip; the nn.Embedding
modules keep the tables).
`gcn_native_head` = False (True: out_mlp's Linear + ReLU layers and the classifier run as `linear_act`, and the new methods
GCNClassifier.loss / GCNClassifier.predict -- the trainer's CrossEntropyLoss + pooling_l2 penalty and its softmax + argmax, reference
model/trainer.py:94-100, 119-120 -- as `head_loss` / `head_predict`, one launch per op and direction over csrc/head_kernels.hip; the
nn.Linear modules keep the parameters.  With `gcn_check_trees` the loss reads one status word back and raises IndexError on a label
outside [0, num_class)).
"""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import _lib
from ..utils import constant
from .deprel import _DiagLayerFn, _FullAggFn, _zero_pad_row, bilinear_supported, bilinear_traverse, diag_layer  # noqa: F401
from .embed import _embed, _EmbedFn, embed_inputs  # noqa: F401
from .head import head_loss, head_predict, linear_act  # noqa: F401
from .layers import WeightPack, gcn_layer, gcn_layers, gcn_layers_with_acts  # noqa: F401
from .pooling import pool, pool3, pool3_packed  # noqa: F401
from .rnn import bilstm
from .tree import CompactTrees, PackedTrees, PrunedTrees, adj_to_csr, prune_to_csr, prune_to_csr_packed


def _draw_seed():
    """One dropout seed from the CPU generator (torch.manual_seed fixes it): no GPU sync."""
    return int(torch.randint(0, 2 ** 62, (1,)).item())


# ------------------------------------------------------------------------------------------------------
# modules with the reference's names and state_dict layout
# ------------------------------------------------------------------------------------------------------
class GCNClassifier(nn.Module):
    """Reference model/gcn.py:15-36."""

    def __init__(self, opt, emb_matrix=None):
        super().__init__()
        self.gcn_model = GCNRelationModel(opt, emb_matrix=emb_matrix)
        self.classifier = nn.Linear(opt['hidden_dim'], opt['num_class'])
        self.opt = opt

    def conv_l2(self):
        return self.gcn_model.gcn.conv_l2()

    def forward(self, inputs, trees=None):
        outputs, pooling_output = self.gcn_model(inputs, trees)
        if self.opt.get('gcn_native_head', False):
            return linear_act(outputs, self.classifier.weight, self.classifier.bias, relu=False), pooling_output
        return self.classifier(outputs), pooling_output

    def loss(self, logits, pooling_output, labels):
        """The training loss of the reference's trainer (model/trainer.py:94-100) from forward()'s two results: CrossEntropyLoss, the
        conv_l2 decay (opt['conv_l2'] > 0) and the pooling_l2 penalty (opt['pooling_l2'] > 0).  With opt['gcn_native_head'] the cross
        entropy and the penalty are one launch each way (head_loss)."""
        l2 = float(self.opt.get('pooling_l2', 0) or 0)
        if self.opt.get('gcn_native_head', False):
            check = bool(self.opt.get('gcn_check_trees', True))
            status = torch.empty((1,), dtype=torch.int32, device=logits.device) if check else None
            loss = head_loss(logits, labels, pooling_output if l2 > 0 else None, l2, status=status)
            if check and int(status.item()) & 1:                      # a host sync of its own, only with gcn_check_trees
                raise IndexError("labels out of range: the classifier has %d classes" % logits.shape[1])
        else:
            loss = F.cross_entropy(logits, labels)
            if l2 > 0:
                loss = loss + l2 * (pooling_output ** 2).sum(1).mean()
        if self.opt.get('conv_l2', 0) > 0:
            loss = loss + self.conv_l2() * self.opt['conv_l2']
        return loss

    def predict(self, logits):
        """(class probabilities [B,C], predicted class int64 [B]) as the reference's trainer derives them (model/trainer.py:119-120)."""
        if self.opt.get('gcn_native_head', False):
            return head_predict(logits)
        return F.softmax(logits.detach(), 1), logits.detach().argmax(1)

    def get_deprel_emb(self):
        return self.gcn_model.get_deprel_embedding()

    def get_gcn_parameters(self):
        return self.gcn_model.get_gcn_parameters()


class GCNRelationModel(nn.Module):
    """Reference model/gcn.py:38-126; the tree build of lines 96-112 runs on the device."""

    def __init__(self, opt, emb_matrix=None):
        super().__init__()
        self.opt = opt
        self.emb_matrix = emb_matrix
        self.adj_type = opt.get('adj_type', 'regular')
        if self.adj_type not in ('regular', 'diagonal_deprel', 'full_deprel'):
            raise ValueError('Adjacency aggregation type not supported.')            # gcn.py:388 (concat_deprel is dead code there)
        self.emb = nn.Embedding(opt['vocab_size'], opt['emb_dim'], padding_idx=constant.PAD_ID)
        self.pos_emb = nn.Embedding(constant.N_POS, opt['pos_dim']) if opt['pos_dim'] > 0 else None
        self.ner_emb = nn.Embedding(constant.N_NER, opt['ner_dim']) if opt['ner_dim'] > 0 else None
        # gcn.py:48-56: the reference keeps a 1-wide dummy table on the regular path (kept for checkpoints);
        # diagonal_deprel scales hidden vectors element-wise, so its table is hidden_dim wide; full_deprel mixes deprel_emb_dim matrices
        width = {'regular': 1, 'diagonal_deprel': opt['hidden_dim']}.get(self.adj_type) or opt['deprel_emb_dim']
        self.deprel_emb = nn.Embedding(constant.N_DEPREL, width, padding_idx=0)
        self.init_embeddings()
        self.gcn = GCN(opt, (self.emb, self.pos_emb, self.ner_emb, self.deprel_emb), opt['hidden_dim'], opt['num_layers'])
        mlp = [nn.Linear(opt['hidden_dim'] * 3, opt['hidden_dim']), nn.ReLU()]
        for _ in range(opt['mlp_layers'] - 1):
            mlp += [nn.Linear(opt['hidden_dim'], opt['hidden_dim']), nn.ReLU()]
        self.out_mlp = nn.Sequential(*mlp)

    def _mlp(self, pooled):
        """out_mlp (gcn.py:66-72, 122); with opt['gcn_native_head'] each Linear + ReLU pair is one linear_act over the module's parameters."""
        if not self.opt.get('gcn_native_head', False):
            return self.out_mlp(pooled)
        x = pooled
        for lin in self.out_mlp:
            if isinstance(lin, nn.Linear):
                x = linear_act(x, lin.weight, lin.bias, relu=True)
        return x

    def get_deprel_embedding(self):
        return self.deprel_emb.weight

    def get_gcn_parameters(self):
        return self.gcn.get_gcn_parameters()

    def init_embeddings(self):
        """gcn.py:73-88: uniform(-1,1) or the given matrix; topn decides which rows are fine-tuned."""
        with torch.no_grad():
            if self.emb_matrix is None:
                self.emb.weight[1:, :].uniform_(-1.0, 1.0)
            else:
                m = self.emb_matrix
                self.emb.weight.copy_(torch.from_numpy(m) if isinstance(m, np.ndarray) else m)
        topn = self.opt.get('topn', self.opt['vocab_size'])
        if topn <= 0:
            self.emb.weight.requires_grad = False
        elif topn < self.opt['vocab_size'] and not self.opt.get('gcn_sparse_emb_grad', False):
            def keep_top(grad, n=topn):
                grad = grad.clone()
                grad[n:].zero_()
                return grad
            self.emb.weight.register_hook(keep_top)

    def forward(self, inputs, trees=None):
        """`trees`: optional PrunedTrees of this batch from a TreeCache (model.tree, loader-side pre-pruning); by default
        the batch is pruned here."""
        if self.opt['dataset'] == 'tacred':
            words, masks, pos, ner, deprel, head, subj_pos, obj_pos = inputs
        else:
            words, masks, pos, deprel, head, subj_pos, obj_pos = inputs
        pack = None
        if trees is None:
            # lengths, head_to_tree, tree_to_adj and the upload (gcn.py:96-112) in one launch, no host round trip; in a training step the
            # same launch packs the layer weights on the CUs the tree build leaves idle (one launch boundary less)
            pack = self.gcn.weight_pack(head.shape[0], head.shape[1]) if self.opt.get('gcn_pack_with_trees', True) else None
            if self.opt.get('gcn_packed', False) and not self.opt.get('gcn_pooled_only', False):
                # token-packed rows: the layers run on sum(len) rows instead of B*T (one host sync for sum(len), where the reference syncs
                # for the lengths anyway, gcn.py:96); the SAME launch writes the packed layout (and packs the weights); the relation-aware
                # variants read the adjacency values from it
                trees = prune_to_csr_packed(head, subj_pos, obj_pos, deprel, self.opt['prune_k'], masks.eq(0).sum(1), masks=masks,
                                            want_label=self.adj_type != 'regular', pack=pack)
                if self.opt.get('gcn_check_trees', True):
                    trees.padded.check(expect_maxlen=head.shape[1])
                    trees.check()
            else:
                trees = prune_to_csr(head, subj_pos, obj_pos, deprel, self.opt['prune_k'], masks=masks,
                                     want_label=self.adj_type != 'regular', pack=pack)
                if self.opt.get('gcn_check_trees', True):
                    trees.check(expect_maxlen=head.shape[1])
                if self.opt.get('gcn_pooled_only', False):
                    # one host sync for the width (a TreeCache avoids it); entity tokens are kept even when the tree does not hold them
                    trees = trees.compact(also_keep=(subj_pos == 0) | (obj_pos == 0))
        else:
            if (trees.B, trees.T) != tuple(head.shape):
                raise ValueError("trees are for a [%d,%d] batch, the inputs are %s" % (trees.B, trees.T, tuple(head.shape)))
            if self.opt.get('gcn_check_trees', True):
                trees.check() if isinstance(trees, PackedTrees) else trees.check(expect_maxlen=head.shape[1])
        return self._forward_trees(inputs, trees, pack, subj_pos, obj_pos)

    def _forward_trees(self, inputs, trees, pack, subj_pos, obj_pos):
        # regular adjacency, padded or token-packed rows: the GCN returns the three pooled vectors itself (stack + pooling as ONE autograd op, so
        # the pooling's backward hands the top layer its dZ; packed rows are pooled where they lie, never unpacked); opt['gcn_pool_handover'] =
        # False keeps the two ops apart (packed: unpack_rows, then pool3 on [B,T,H])
        handover = (self.adj_type == 'regular' and isinstance(trees, (PrunedTrees, CompactTrees, PackedTrees))
                    and self.opt.get('gcn_pool_handover', True))
        if isinstance(trees, CompactTrees):
            # only the tokens of the pruned trees and the entity tokens are computed ([B,Tc,H]); the three poolings never look at
            # any other (gcn.py:116-119), so the pooled vectors are the full batch's
            subj_pos, obj_pos = trees.take(subj_pos, fill=150), trees.take(obj_pos, fill=150)      # 150: the loader's pad value (loader.py:120-121)
        self.gcn._pool_req = (subj_pos, obj_pos, self.opt['pooling']) if handover else None
        if pack is not None:
            self.gcn.use_weight_pack(pack)
        try:
            h, pool_mask = self.gcn(trees, inputs)
        finally:
            self.gcn._take_request()              # (a forward that raised before it got there leaves nothing behind)
        if isinstance(h, _Pooled):
            pooled = h.value
            return self._mlp(pooled), pooled[:, :self.opt['hidden_dim']]
        # gcn.py:116-121: three masked poolings and the concat, one pass over h (masks straight from the position tensors)
        pooled = pool3(h, pool_mask, subj_pos, obj_pos, type=self.opt['pooling'])
        h_out = pooled[:, :self.opt['hidden_dim']]
        return self._mlp(pooled), h_out


class _Pooled(object):
    """Marker: GCN.forward was asked (by GCNRelationModel) for pool3(h_L, ...) and returns it in place of h_L."""

    def __init__(self, value):
        self.value = value


class GCN(nn.Module):
    """Reference model/gcn.py:128-395, `regular` and `diagonal_deprel` adjacency types.  `adj` may be a dense
    float32 [B,T,T] tensor (as the reference passes) or a PrunedTrees from model.tree."""

    def __init__(self, opt, embeddings, mem_dim, num_layers):
        super().__init__()
        self.opt = opt
        self.layers = num_layers
        self.use_cuda = opt.get('cuda', True)
        self.mem_dim = mem_dim
        tacred = opt['dataset'] == 'tacred'
        self.in_dim = opt['emb_dim'] + opt['pos_dim'] + (opt['ner_dim'] if tacred else 0)
        self.emb, self.pos_emb, self.ner_emb, self.deprel_emb = embeddings
        self.adj_type = opt.get('adj_type', 'regular')
        if self.adj_type not in ('regular', 'diagonal_deprel', 'full_deprel'):
            raise ValueError('Adjacency aggregation type not supported.')            # gcn.py:388
        if opt.get('rnn', False):
            self.rnn = nn.LSTM(self.in_dim, opt['rnn_hidden'], opt['rnn_layers'], batch_first=True,
                               dropout=opt['rnn_dropout'], bidirectional=True)
            self.in_dim = opt['rnn_hidden'] * 2
            self.rnn_drop = nn.Dropout(opt['rnn_dropout'])
        self.in_drop = nn.Dropout(opt['input_dropout'])
        self.gcn_drop = nn.Dropout(opt['gcn_dropout'])
        self.emb_dropout = opt.get('emb_dropout', 0.0)
        if self.adj_type == 'diagonal_deprel':                  # gcn.py:153-155: no per-layer weights in this variant
            self.preprocessor = nn.Linear(self.in_dim, mem_dim)
            self.in_dim = mem_dim
        elif self.adj_type == 'full_deprel':                    # gcn.py:156-167: ONE Linear, reshaped to [D, in_dim, H], for every layer
            self.W = nn.Linear(self.in_dim, opt['deprel_emb_dim'] * mem_dim, bias=True)
        else:
            self.W = nn.ModuleList(nn.Linear(self.in_dim if l == 0 else mem_dim, mem_dim) for l in range(num_layers))
        kind = opt.get('gcn_dtype', 'fp32')
        if kind not in ('fp32', 'bf16'):
            raise ValueError("gcn_dtype must be 'fp32' or 'bf16'")
        self.compute_dtype = torch.float32 if kind == 'fp32' else torch.bfloat16
        self._wcache = {}             # packed weight images, valid while the weights' version counters stand still
        # what the next forward was asked for behind its fixed (adj, inputs) signature, see _take_request: the pooled vectors
        # (subj_pos, obj_pos, pooling type; set by GCNRelationModel) and a filled WeightPack (use_weight_pack)
        self._pool_req = self._prepacked = None
        # graph-safe dropout: a by-value seed is frozen into a captured hipGraph, so with opt['gcn_graph_rng'] the per-layer
        # seeds are fixed at construction and a device counter (advanced by one captured op per forward) is added in the kernel
        self.graph_rng = bool(opt.get('gcn_graph_rng', False))
        if self.graph_rng:
            self.register_buffer('_rng_step', torch.zeros(1, dtype=torch.int64), persistent=False)
            self._base_seeds = [_draw_seed() for _ in range(num_layers)]
            if opt.get('gcn_native_embed', False):                   # (seed_emb, seed_in) of the native front end
                self._embed_seeds = tuple(_draw_seed() for _ in range(2))

    def conv_l2(self):
        # the reference's diagonal_deprel model has no W list, so its conv_l2() / get_gcn_parameters() raise AttributeError
        # (gcn.py:180-184, 397-398), and full_deprel's single nn.Linear is not iterable (TypeError); the same happens here
        return sum(p.pow(2).sum() for lin in self.W for p in (lin.weight, lin.bias))

    def get_gcn_parameters(self):
        return self.W

    def _word_grad_form(self):
        """(sparse, topn) of the word table's gradient.  opt['gcn_sparse_emb_grad']: the gradient as (token ids, rows) -- what a
        data-parallel loop exchanges with shard.SparseRowExchange instead of the dense [V, 300] all-reduce; topn (None: every row is
        fine-tuned) is then applied to the rows by the op, not by the hook of init_embeddings."""
        topn = self.opt.get('topn', self.opt['vocab_size'])
        return bool(self.opt.get('gcn_sparse_emb_grad', False)), topn if 0 < topn < self.opt['vocab_size'] else None

    def _word_embeddings(self, words):
        """EmbeddingDropout of the reference (model/dropouts.py:23-39): in training, every word TYPE of a
        sentence is dropped with probability emb_dropout and the rest is scaled by 1/(1-p)."""
        embs = _embed(self.emb, words, *self._word_grad_form())       # (a dense gradient ignores topn: the hook applies it)
        p = self.emb_dropout
        if not self.training or p <= 0.0:
            return embs
        keep = torch.empty((words.shape[0], self.emb.num_embeddings), device=words.device).bernoulli_(1 - p)
        return embs * torch.gather(keep, 1, words).unsqueeze(-1) / (1 - p)

    def _native_inputs(self, adj, words, pos, ner, use_rnn):
        """opt['gcn_native_embed']: what the lookups, the cat, _word_embeddings' dropout, in_drop and (PackedTrees, no LSTM) pack_rows
        compute, from embed_inputs.  Returns (rows, whether they are token-packed: PackedTrees without an LSTM in front, on the regular path
        or -- opt['gcn_packed'] -- a relation-aware one).  float32, except that a bf16 module whose layer stack reads them directly (no LSTM,
        regular adjacency) gets bfloat16.  Seeds as _dropout_plan's: the CPU generator per forward, or with
        opt['gcn_graph_rng'] fixed base seeds plus the _rng_step device counter.  In eval() / without dropout the op is a pure gather."""
        direct = self.adj_type == 'regular' and not use_rnn
        to_packed = not use_rnn and isinstance(adj, PackedTrees) and (direct or self._packed_deprel(adj))
        p_emb = self.emb_dropout if (self.training and words.dim() == 2) else 0.0
        p_in = self.in_drop.p if self.training else 0.0
        seeds, seed_dev = (0, 0), None
        if p_emb > 0 or p_in > 0:
            if self.graph_rng:
                self._rng_step.add_(1)                                # on the stream: part of a captured graph
                seeds, seed_dev = self._embed_seeds, self._rng_step
            else:
                seeds = tuple(_draw_seed() for _ in range(2))
        check = bool(self.opt.get('gcn_check_trees', True))
        status = torch.empty((1,), dtype=torch.int32, device=words.device) if check else None
        sparse, topn = self._word_grad_form()
        rows = embed_inputs(words, pos, ner, self.emb, self.pos_emb if self.opt['pos_dim'] > 0 else None,
                            self.ner_emb if (self.opt['ner_dim'] > 0 and ner is not None) else None, trees=adj if to_packed else None,
                            p_emb=p_emb, p_in=p_in, seeds=seeds, seed_dev=seed_dev,
                            out_dtype=torch.bfloat16 if (direct and self.compute_dtype == torch.bfloat16) else torch.float32,
                            sparse=sparse, topn=topn, status=status)
        if check:
            bits = int(status.item())                                 # a host sync of its own, only with gcn_check_trees
            if bits:
                raise IndexError("embedding ids out of range in: %s" % ", ".join(n for k, n in enumerate(("words", "pos", "ner")) if bits >> k & 1))
        return rows, to_packed

    def encode_with_rnn(self, rnn_inputs, masks, batch_size):
        if self.opt.get('gcn_native_rnn', False):
            # the native recurrence (model/rnn.py): lengths stay on the device, the output is [B, T, 2H] (zeros past each sentence)
            return bilstm(rnn_inputs.float(), masks.eq(0).sum(1).int(), self.rnn, self.training)
        lens = masks.eq(0).long().sum(1).cpu()
        shape = (self.opt['rnn_layers'] * 2, batch_size, self.opt['rnn_hidden'])
        h0 = rnn_inputs.new_zeros(shape)
        packed = nn.utils.rnn.pack_padded_sequence(rnn_inputs, lens, batch_first=True, enforce_sorted=False)
        out, _ = self.rnn(packed, (h0, h0.clone()))
        out, _ = nn.utils.rnn.pad_packed_sequence(out, batch_first=True)
        return out

    def weight_pack(self, B=None, T=None):
        """A WeightPack for the launch that builds this step's trees (`prune_to_csr(..., pack=)`, `TreeCache.batch(..., pack=)`), or None
        when the next forward would not use one: only the `regular` per-layer kernels pack this way, and only when the cached images do
        not already belong to the current weights (eval(), gradient accumulation).  Hand the request back with `use_weight_pack`."""
        if self.adj_type != 'regular':
            return None
        dev = self.W[0].weight.device
        if dev.type != 'cuda':
            return None
        Ws = [lin.weight for lin in self.W]
        compute = _lib.dtype_code(self.compute_dtype)
        if self._cache_usable() and self._wcache.get("key") == WeightPack.key_of(Ws, compute, dev):
            return None
        return WeightPack(Ws, compute, dev)

    def use_weight_pack(self, pack):
        """The next forward takes the weight images from `pack` (a WeightPack a tree launch has filled); None clears it."""
        self._prepacked = pack

    def _take_request(self):
        """(pooling request, WeightPack) for this forward, cleared: a request serves ONE forward."""
        req, pre = self._pool_req, self._prepacked
        self._pool_req = self._prepacked = None
        return req, pre

    def _cache_usable(self):
        """Whether this forward may reuse the packed weight images of an earlier one.  The cache is keyed on the weights' storage and
        version counters, and an in-place update through `p.data` (the reference's own MyAdagrad does that, utils/torch_utils.py:84-88;
        so do EMA swaps and hand-written clipping) changes the values WITHOUT bumping the counter -- in train() and in eval() alike
        (`eval -> p.data.copy_(ema) -> eval` is the usual evaluation of an averaged model).  So every forward re-packs -- one 4 us launch,
        none at all when the tree launch of the same forward carries it (gcn_pack_with_trees) -- unless opt['gcn_reuse_packed_weights']
        says the caller knows its weights stand still between forwards (gradient accumulation, a frozen model serving requests); such a
        caller calls invalidate_weight_cache() after writing to `p.data` by hand."""
        if torch.cuda.is_current_stream_capturing():
            return False                                                  # a captured step must contain its pack
        ok = bool(self.opt.get('gcn_reuse_packed_weights', False))
        if not ok:
            self._wcache.clear()
        return ok

    def invalidate_weight_cache(self):
        self._wcache.clear()

    def _dropout_plan(self):
        """(p per layer, seed per layer, device seed word or None) for this forward -- gcn.py:393: every layer but the last."""
        ps = [self.gcn_drop.p if (self.training and l < self.layers - 1) else 0.0 for l in range(self.layers)]
        if self.graph_rng:
            if any(p > 0 for p in ps):
                self._rng_step.add_(1)                                # on the stream: part of a captured graph
            return ps, [s if p > 0 else 0 for s, p in zip(self._base_seeds, ps)], self._rng_step
        return ps, [_draw_seed() if p > 0 else 0 for p in ps], None

    def _packed_deprel(self, trees):
        """Whether a relation-aware forward on these PackedTrees runs on the token-packed rows: opt['gcn_packed'] says so (without it the
        variants keep to the padded adjacency a .pack()ed batch carries along).  Raises for packed trees that lack what the variant reads."""
        if self.adj_type == 'regular' or not self.opt.get('gcn_packed', False):
            return False
        if trees.label is None:
            raise ValueError("adj_type %r needs the adjacency values: build the packed trees with want_label=True" % self.adj_type)
        if self.adj_type == 'diagonal_deprel' and trees.rowT_ptr is None and torch.is_grad_enabled():
            raise ValueError("adj_type 'diagonal_deprel' needs the transposed pattern for its backward: build the packed trees with "
                             "want_transpose=True")
        return True

    @staticmethod
    def _packed_rows(trees, gcn_inputs, rows_packed):
        """float32 [N, width] rows of a relation-aware forward on PackedTrees, the rows past sum(len) zero (the GEMMs around the kernels
        run over all N rows, and what an allocation happens to hold must not reach a weight gradient): the padded inputs packed once, or
        the rows embed_inputs packed already."""
        if not rows_packed:
            return trees.pack_rows(gcn_inputs.to(torch.float32), zero_tail=True)
        x = gcn_inputs.to(torch.float32)
        return torch.where(trees.live_rows().unsqueeze(1), x, x.new_zeros(()))

    def _forward_diagonal(self, adj, gcn_inputs, deprel, rows_packed=False):
        """gcn.py:255-257, 272-294: Linear preprocessor (host BLAS), then the element-wise relation-scaled layers.
        no_adj has no effect on this variant in the reference either (it only zeroes the matrix the regular path uses).
        On a PackedTrees (opt['gcn_packed']) the preprocessor and every layer see the N packed rows; the output is unpacked once."""
        pk = adj if isinstance(adj, PackedTrees) else None
        trees = adj if isinstance(adj, (PrunedTrees, PackedTrees)) else adj_to_csr(adj, want_label=True)
        if pk is not None:
            gcn_inputs, deprel = self._packed_rows(pk, gcn_inputs, rows_packed), pk.pack_ids(deprel)
        x = self.preprocessor(gcn_inputs).to(self.compute_dtype)
        table = self.deprel_emb.weight            # padding_idx=0: nn.Embedding's backward would zero row 0, the hook below does
        if table.requires_grad and not getattr(self, '_pad_hooked', False):
            table.register_hook(_zero_pad_row)
            self._pad_hooked = True
        ps, seeds, seed_dev = self._dropout_plan()
        for l in range(self.layers):
            x = diag_layer(x, table, deprel, trees, ps[l], seeds[l], seed_dev)
        if pk is not None:
            return pk.unpack_rows(x.float()), pk.padded.pool_mask
        return x.float(), trees.pool_mask

    def _forward_full(self, adj, gcn_inputs, deprel, all_tokens=False, rows_packed=False):
        """adj_type='full_deprel', gcn.py:296-388 + traverse_deprel / traverse_self_loop 400-434; the traversal's contraction runs on
        csrc/bilinear_kernels.hip in the module's precision: exact fp32 MFMA (default) or, with opt['gcn_dtype']='bf16', bf16 operands.
        trav(x, e)[n] = sum_d e[n,d] (x[n] W3[d] + b3[d]) is only needed for tokens that sit in a pruned tree, so those are
        compacted (their number is read back together with the tree check's status word; with opt['gcn_check_trees']=False or
        CompactTrees, whose rows are those tokens already, every row is traversed and there is no host sync at all).  The
        contraction runs on the hand-written kernels in both precisions (a library GEMM only when Tin > 256).  Everything around it -- aggregation of the traversed rows over the forward / reverse entries of the
        device pruner's CSR (picked by label range), edge dropout, the self-loop term, /(deg+1), ReLU, dropout -- is ONE kernel
        (csrc/full_kernels.hip, gcnpt_full_agg_fwd / _bwd).  The reference materialises [B,T,D,Tin] for all tokens and multiplies
        dense [B,T,T] matrices instead.
        On a PackedTrees (opt['gcn_packed']) the rows are the N token-packed ones: all of them are traversed (no compaction, no host sync,
        whatever gcn_check_trees says -- fewer rows than B*T, more than the in-tree count), the self-loop GEMM sees N rows, the edge keep
        flags are drawn per packed CSR slot, and the output is unpacked once, at the end."""
        opt = self.opt
        pk = adj if isinstance(adj, PackedTrees) else None
        trees = adj if isinstance(adj, (PrunedTrees, PackedTrees)) else adj_to_csr(adj, want_label=True)
        if trees.label is None:
            raise ValueError("full_deprel needs the adjacency values: build the trees with want_label=True")
        B, T = trees.B, trees.T
        N, n_slots = (pk.N, pk.nnz_cap) if pk is not None else (B * T, B * trees.cap)
        D, H = opt['deprel_emb_dim'], self.mem_dim
        dev = trees.device
        max_depth = opt.get('deprel_max_depth', 2)
        directed, self_loop = bool(opt.get('deprel_directed', False)), bool(opt.get('deprel_self_loop', True))
        if pk is not None:
            tok = pos = None                                             # identity: packed row r is row r of the traversal
            gcn_inputs = self._packed_rows(pk, gcn_inputs, rows_packed)
        elif all_tokens or not opt.get('gcn_check_trees', True):
            # no compaction, no sync: every row is traversed (CompactTrees: the rows ARE the tokens of the pruned trees)
            tok = torch.arange(N, device=dev)
            pos = tok.to(torch.int32)
        else:
            tok = torch.nonzero(~trees.pool_mask.view(-1)).squeeze(1)                            # tokens of the pruned trees
            pos = torch.full((N,), -1, dtype=torch.int32, device=dev)
            pos[tok] = torch.arange(tok.numel(), device=dev, dtype=torch.int32)
        M = int(tok.numel()) if tok is not None else N
        deprel_tok = deprel.reshape(-1)[tok] if tok is not None else pk.pack_ids(deprel)
        b3 = self.W.bias.reshape(D, H)                                                            # gcn.py:303
        x = gcn_inputs.to(torch.float32)
        ps, seeds, seed_dev = self._dropout_plan()
        for l in range(self.layers):
            Tin = x.shape[-1]
            if self.W.weight.shape[1] != Tin:       # the reference's einsum fails the same way when in_dim != mem_dim (layer 1)
                raise RuntimeError("full_deprel: layer %d input has %d features but the shared weight is [D, %d, H] (gcn.py:167, 301)"
                                   % (l, Tin, self.W.weight.shape[1]))
            Wk = self.W.weight.reshape(D * Tin, H)                                                # W3[d,t,h] flattened over (d,t), gcn.py:301
            xf = x.reshape(N, Tin)
            xt = xf[tok] if tok is not None else xf
            plain = l >= max_depth                                                                # gcn.py:323-324, 355-356, 371-374
            ys, keeps = [None, None], [None, None]
            for k, (shift, on) in enumerate(((0, True), (constant.DEPREL_FORWARD_BOUND, not directed))):
                if not on or M == 0:
                    continue
                e = _embed(self.deprel_emb, deprel_tok + shift)
                keep_prop = opt.get('deprel_keep_prop', 1.0)
                if self.training and keep_prop < 1.0:                                             # maybe_forget_deprels, gcn.py:451-470
                    kept = torch.empty((M, 1), device=dev).bernoulli_(keep_prop) == 1
                    e = torch.where(kept, e, torch.ones_like(e))
                if plain:
                    e = torch.ones_like(e)
                if bilinear_supported(D, Tin, H, self.compute_dtype):
                    # hand-written MFMA contraction in the module's precision (exact fp32 MFMA by default): e (x) x never exists
                    ys[k] = bilinear_traverse(xt, e, self.W.weight, self.W.bias, self.compute_dtype)
                else:                                                                             # Tin > 256: one library GEMM, gcn.py:408-414
                    ys[k] = torch.mm((e.unsqueeze(2) * xt.unsqueeze(1)).reshape(-1, D * Tin), Wk) + torch.mm(e, b3)
                edge_keep = opt.get('edge_keep_prob', 1.0)
                if self.training and edge_keep < 1.0:                                             # maybe_drop_edges, gcn.py:436-449
                    keeps[k] = torch.empty((n_slots,), device=dev).bernoulli_(edge_keep).to(torch.uint8)
            self_term = None
            if self_loop:                                                                         # gcn.py:366-385, 417-434 (plain GEMMs)
                se = torch.ones((D,), device=dev) if plain else self.deprel_emb.weight[constant.SELF_LOOP_INDEX]
                self_term = torch.mm(xf, torch.mm(se.unsqueeze(0), self.W.weight.reshape(D, Tin * H)).reshape(Tin, H)) + torch.mv(b3.t(), se)
            if ys[0] is None:
                ys[0] = torch.zeros((1, H), dtype=torch.float32, device=dev)                      # no token sits in a tree
            x = _FullAggFn.apply(ys[0], ys[1], self_term, trees, pos, keeps[0], keeps[1], M if M > 0 else 0, ps[l], seeds[l], seed_dev)
            x = x.view(B, T, H) if pk is None else x
        if pk is not None:
            return pk.unpack_rows(x), pk.padded.pool_mask
        return x, trees.pool_mask

    def forward(self, adj, inputs):
        if self.opt['dataset'] == 'tacred':
            words, masks, pos, ner, deprel, head, subj_pos, obj_pos = inputs
        else:
            words, masks, pos, deprel, head, subj_pos, obj_pos = inputs
            ner = None
        ct = adj if isinstance(adj, CompactTrees) else None
        use_rnn = bool(self.opt.get('rnn', False))
        if ct is not None:
            # "pooled-only" rows: the layers run on the kept tokens.  Without an LSTM in front the lookups themselves are
            # done for those tokens only; with one, its outputs are gathered
            adj, deprel = ct.trees, ct.take(deprel)
            if not use_rnn:
                words, pos = ct.take(words), ct.take(pos)
                ner = ct.take(ner) if ner is not None else None
        rows_packed = False
        if self.opt.get('gcn_native_embed', False):
            # lookups, cat, both dropouts, the bf16 cast and pack_rows as one launch (embed_inputs)
            embs, rows_packed = self._native_inputs(adj, words, pos, ner, use_rnn)
        else:
            parts = [words if words.dim() > 2 else self._word_embeddings(words)]    # gcn.py:235-239
            if self.opt['pos_dim'] > 0:
                parts.append(_embed(self.pos_emb, pos))
            if self.opt['ner_dim'] > 0 and ner is not None:
                parts.append(_embed(self.ner_emb, ner))
            embs = self.in_drop(torch.cat(parts, dim=2))
        if use_rnn:
            gcn_inputs = self.rnn_drop(self.encode_with_rnn(embs, masks, words.size(0)))
            if ct is not None:
                gcn_inputs = ct.take(gcn_inputs)
        else:
            gcn_inputs = embs

        packed = adj if isinstance(adj, PackedTrees) else None
        if packed is not None and self.adj_type != 'regular' and not self._packed_deprel(packed):
            if not isinstance(packed.padded, PrunedTrees):
                raise ValueError("adj_type %r runs on the padded adjacency, which trees pruned straight into the packed layout "
                                 "(prune_to_csr_packed, TreeCache.batch_packed) do not keep: use prune_to_csr(...).pack(...)" % self.adj_type)
            adj = packed.padded                                  # the deprel variants run on the padded layout
        if self.adj_type == 'diagonal_deprel':
            return self._forward_diagonal(adj, gcn_inputs, deprel, rows_packed)
        if self.adj_type == 'full_deprel':
            return self._forward_full(adj, gcn_inputs, deprel, all_tokens=ct is not None, rows_packed=rows_packed)
        trees = adj if isinstance(adj, (PrunedTrees, PackedTrees)) else adj_to_csr(adj, want_label=False)   # gcn.py:260-262
        return self._forward_regular(trees, gcn_inputs, rows_packed)

    def _forward_regular(self, trees, gcn_inputs, rows_packed):
        """gcn.py:264-271, 390-395 on a PrunedTrees or a PackedTrees: the layer stack as one op.  Token-packed rows are padded / unpadded
        only here, at the module boundary: the layer loop sees [sum(len), width] rows (rows_packed: the inputs are such rows already),
        the caller [B,T,H]."""
        no_adj = bool(self.opt.get('no_adj', False))                                           # gcn.py:264-265
        ps, seeds, seed_dev = self._dropout_plan()
        Ws, bs = [lin.weight for lin in self.W], [lin.bias for lin in self.W]
        x = gcn_inputs
        if trees.packed and not rows_packed:
            x = trees.pack_rows(x if x.dtype in (torch.float32, torch.bfloat16) else x.float())
        req, pre = self._take_request()
        wcache = self._wcache if self._cache_usable() else None
        # req: GCNRelationModel asked for the pooled vectors directly (it would pool h next, gcn.py:116-121): stack + pooling as one op,
        # packed rows pooled where they lie
        h = gcn_layers(x, Ws, bs, trees, ps, seeds, self.compute_dtype, torch.float32, no_adj, seed_dev, wcache, pool=req, prepacked=pre)
        pool_mask = trees.padded.pool_mask if trees.packed else trees.pool_mask
        if req is not None:
            return _Pooled(h), pool_mask
        return (trees.unpack_rows(h) if trees.packed else h), pool_mask
