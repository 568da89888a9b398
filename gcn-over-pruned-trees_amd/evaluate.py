"""
Device-side evaluation of a split (reference model/trainer.py:112-124, train.py:245-285, utils/scorer.py:20-96).

The reference reads every batch's softmax and logits back, unsorts them in Python and scores strings in a loop.  Here one launch per
batch (gcnpt_eval_batch, csrc/eval_kernels.hip) writes predictions, per-sentence loss and confusion counts where the DATASET's order wants
them, one finishing launch (gcnpt_eval_finish) makes loss, precision, recall and F1 of them, and the host reads one small result:

    ev = Evaluator(model, ds, 50, cache=ds.tree_cache(prune_k), graph=True)
    res = ev.run()                       # nothing here reads from the device
    m = res.read()                       # the single transfer: loss, precision, recall, f1, n_scored, n_sentences, n_unseen, bad_label
    dev_loss = res.dev_loss(50)          # train.py:269's own figure, for log lines that match the reference

A caller who keeps the reference's loader uses the accumulators alone, in place of trainer.py:118-124 plus the scorer:

    st = EvalState(len(gold), num_class, device)
    for batch in loader:
        logits, _ = model(inputs)
        st.add(logits, labels, orig_idx)
    m = st.finish().read()

No CPU path exists: a device that is not a GPU, or a CPU tensor, raises.
"""
import numpy as np
import torch

from . import _lib
from .utils import staging

MAX_CLASSES = 1024         # include/gcnpt.h: the confusion matrix is C*C int32


def _gpu_only(what, *tensors):
    for t in tensors:
        if t is not None and not (torch.is_tensor(t) and t.is_cuda):
            raise TypeError("%s runs on the GPU only (got %s); there is no CPU path" % (what, t.device if torch.is_tensor(t) else type(t)))


class EvalResult(object):
    """What a finished evaluation left on the device: pred int64 [S] (-1: never scored), probs float32 [S,C] or None, row_loss float32 [S],
    confusion int32 [C,C] (gold x predicted), by_relation int32 [3,C] (correct, guessed, gold), totals int32 [6], metrics float64 [4],
    status int32 [1]; `batches`: the batch plan (host index arrays) when an Evaluator made it."""

    def __init__(self, pred, probs, row_loss, confusion, by_relation, totals, metrics, status, seen, batches=None):
        self.pred, self.probs, self.row_loss, self.confusion = pred, probs, row_loss, confusion
        self.by_relation, self.totals, self.metrics, self.status, self.seen, self.batches = by_relation, totals, metrics, status, seen, batches

    def read(self, predictions=False):
        """The single host transfer.  predictions=True adds `pred` (NumPy int64 [S]); they stay on the device otherwise."""
        small = torch.cat([self.metrics, self.totals.to(torch.float64), self.status.to(torch.float64)]).cpu().numpy()
        loss, p, r, f = (float(v) for v in small[:4])
        totals = [int(v) for v in small[4:10]]                        # (int32 counts are exact in float64)
        out = dict(loss=loss, precision=p, recall=r, f1=f, n_scored=totals[0], n_sentences=totals[1], n_unseen=totals[5],
                   bad_label=bool(int(small[10]) & 1))
        if predictions:
            out["pred"] = self.pred.cpu().numpy()
        return out

    def dev_loss(self, batch_size, batches=None):
        """The reference's own figure (train.py:269): sum over the batches of each batch's mean loss, / S * batch_size -- on the host, from
        row_loss and the batch plan (host index arrays; default: the Evaluator's).  `read()['loss']` is the exact mean."""
        batches = self.batches if batches is None else batches
        if batches is None:
            raise ValueError("EvalResult.dev_loss: no batch plan (pass batches=, the index arrays the split was evaluated in)")
        row = self.row_loss.cpu().numpy().astype(np.float64)
        S = row.shape[0]
        total = 0.0
        for b in batches:
            b = np.asarray(b)
            b = b[(b >= 0) & (b < S)]
            if b.size:
                total += float(row[b].mean())
        return total / S * batch_size


class EvalState(object):
    """The accumulators of one evaluation over S sentences and C classes; `no_relation`: the class the scorer excludes (-1: none)."""

    def __init__(self, S, C, device, no_relation=0, want_probs=False):
        device = torch.device(device)
        if device.type != "cuda":
            raise TypeError("EvalState runs on the GPU only (got %s); there is no CPU path" % device)
        S, C, no_relation = int(S), int(C), int(no_relation)
        if S < 1 or C < 1 or C > MAX_CLASSES:
            raise ValueError("EvalState: S >= 1 and 1 <= C <= %d expected (S=%d C=%d)" % (MAX_CLASSES, S, C))
        if not -1 <= no_relation < C:
            raise ValueError("EvalState: no_relation = %d is outside [-1, C = %d)" % (no_relation, C))
        _lib.lib()
        self.S, self.C, self.no_relation, self.device = S, C, no_relation, device
        i32 = dict(dtype=torch.int32, device=device)
        self.pred = torch.empty((S,), dtype=torch.int64, device=device)
        self.probs = torch.empty((S, C), dtype=torch.float32, device=device) if want_probs else None
        self.row_loss = torch.empty((S,), dtype=torch.float32, device=device)
        self.seen, self.confusion, self.status = torch.empty((S,), **i32), torch.empty((C, C), **i32), torch.empty((1,), **i32)
        self.by_relation, self.totals = torch.empty((3, C), **i32), torch.empty((6,), **i32)
        self.metrics = torch.empty((4,), dtype=torch.float64, device=device)
        self.reset()

    def reset(self):
        """The initial state, with fills on the current stream (in place: a captured `add` keeps pointing at these buffers)."""
        self.pred.fill_(-1)
        self.row_loss.zero_()
        if self.probs is not None:
            self.probs.zero_()
        for t in (self.seen, self.confusion, self.status, self.by_relation, self.totals, self.metrics):
            t.zero_()

    def add(self, logits, labels, idx, slot_status=None):
        """Scores the rows of one batch in ONE launch: logits float32 [M,C], labels int64 [M], idx int64 [M] (the sentence number of each
        row), slot_status int32 [M] or None (DeviceBatch.status; a non-zero slot is skipped, as is an idx outside [0,S))."""
        _gpu_only("EvalState.add", logits, labels, idx, slot_status)
        if logits.dim() != 2 or logits.shape[1] != self.C:
            raise TypeError("EvalState.add: logits [M,%d] expected, got %s" % (self.C, tuple(logits.shape)))
        M = int(logits.shape[0])
        if labels.numel() != M or idx.numel() != M or (slot_status is not None and slot_status.numel() != M):
            raise ValueError("EvalState.add: labels, idx and slot_status must hold one entry per row of logits (M=%d)" % M)
        z = logits.detach().to(torch.float32).contiguous()
        y, s = labels.to(torch.int64).contiguous(), idx.to(torch.int64).contiguous()
        st = None if slot_status is None else slot_status.to(torch.int32).contiguous()
        P = _lib.ptr
        _lib.check(_lib.lib().gcnpt_eval_batch(_lib.stream(), P(z), P(y), P(s), P(st), M, self.C, self.S, self.no_relation, P(self.pred),
                                               P(self.probs), P(self.row_loss), P(self.seen), P(self.confusion), P(self.status)))

    def finish(self, batches=None):
        """ONE launch: by_relation, totals and metrics from the accumulators; returns an EvalResult of device tensors (views of this
        state's buffers: read or clone them before the next reset())."""
        P = _lib.ptr
        _lib.check(_lib.lib().gcnpt_eval_finish(_lib.stream(), P(self.confusion), P(self.seen), P(self.row_loss), self.C, self.S,
                                                self.no_relation, P(self.by_relation), P(self.totals), P(self.metrics)))
        return EvalResult(self.pred, self.probs, self.row_loss, self.confusion, self.by_relation, self.totals, self.metrics, self.status,
                          self.seen, batches)


class Evaluator(object):
    """
    A model, a DeviceDataset and a batch plan: `run()` evaluates the whole split and returns an EvalResult without reading from the device.

    The batches are planned once from the host copy of the lengths (staging.length_buckets, no shuffle) and every batch's sentence numbers
    are uploaded once, as one int64 [n_batches, batch_size] tensor whose last row is padded with -1: gcnpt_gather_batch gives such a slot a
    non-zero status and an empty masked row, and the scoring launch skips it.  cache: the dataset's TreeCache (None: the model prunes each
    batch itself).  graph=True: one torch.cuda.graph per distinct padded width -- gather, trees, forward and the scoring launch -- captured
    on first use (which synchronises, once) and replayed after a copy of the batch's sentence numbers into the captured idx buffer.
    T_round (default 8 with graph=True, else 1) rounds a batch's width up, capped at dataset.Ts: it bounds the number of graphs.
    """

    def __init__(self, model, dataset, batch_size, cache=None, no_relation=0, graph=False, T_round=None, want_probs=False):
        device = torch.device(dataset.device)
        if device.type != "cuda":
            raise TypeError("Evaluator runs on the GPU only (got %s); there is no CPU path" % device)
        if graph and model.opt.get('gcn_check_trees', True):
            raise ValueError("Evaluator(graph=True): opt['gcn_check_trees'] is on -- its forward synchronises and cannot be captured; "
                             "set opt['gcn_check_trees'] = False")
        self.model, self.dataset, self.cache, self.graph = model, dataset, cache, bool(graph)
        self.batch_size = B = int(batch_size)
        if B < 1:
            raise ValueError("Evaluator: batch_size must be positive (got %d)" % B)
        self.T_round = int(T_round) if T_round is not None else (8 if graph else 1)
        if self.T_round < 1:
            raise ValueError("Evaluator: T_round must be positive (got %d)" % self.T_round)
        lens = np.asarray(dataset.lens_host)
        self.batches = staging.length_buckets(lens, B)
        plan = np.full((len(self.batches), B), -1, dtype=np.int64)
        for j, b in enumerate(self.batches):
            plan[j, :len(b)] = b
        self.idx = torch.from_numpy(plan).to(device)
        r = self.T_round
        self.widths = [min(-(-max(int(lens[b].max()), 1) // r) * r, dataset.Ts) for b in self.batches]
        self.state = EvalState(dataset.S, int(model.opt['num_class']), device, no_relation, want_probs)
        self.graphs = {}                                             # padded width -> (CUDAGraph, captured idx buffer)

    def _step(self, idx, T):
        batch = self.dataset.batch(idx, T)
        if self.cache is not None:
            logits, _ = self.model(batch.inputs, trees=self.cache.batch(batch.idx, T))
        else:
            logits, _ = self.model(batch.inputs)
        self.state.add(logits, batch.labels, batch.idx, batch.status)

    def _capture(self, T):
        """The graph of width T over an idx buffer of its own.  The warm-up and the capture run on empty slots (idx = -1), which the
        scoring launch skips: neither touches the accumulators."""
        buf = torch.full((self.batch_size,), -1, dtype=torch.int64, device=self.state.device)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            self._step(buf, T)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, capture_error_mode="thread_local"):
            self._step(buf, T)
        self.graphs[T] = (graph, buf)
        return self.graphs[T]

    def run(self):
        was_training = self.model.training
        self.model.eval()
        try:
            with torch.no_grad():
                self.state.reset()
                for j, T in enumerate(self.widths):
                    if not self.graph:
                        self._step(self.idx[j], T)
                        continue
                    graph, buf = self.graphs.get(T) or self._capture(T)
                    buf.copy_(self.idx[j])
                    graph.replay()
                return self.state.finish(self.batches)
        finally:
            self.model.train(was_training)
