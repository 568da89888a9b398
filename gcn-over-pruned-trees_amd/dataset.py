"""
Device-resident dataset (the loader's half; reference data/loader.py:81-141, model/trainer.py:52-73).

The reference pads every batch on the host, applies word dropout in Python and uploads eight tensors per step.  Here the token arrays of
the WHOLE dataset stay in HBM as int32 [S,Ts] (TACRED's training set is under 200 MB), and `DeviceDataset.batch(idx)` writes the loader
tensors of a batch from them in ONE launch (gcnpt_gather_batch, csrc/batch_kernels.hip), word dropout included.  Together with
`TreeCache.batch` over the same sentence numbers, a training step reads nothing from the host but `idx`: it can be captured in a hipGraph
once and replayed per batch after a copy into the captured `idx` tensor.

    ds = DeviceDataset.build(words, pos, ner, deprel, head, subj_pos, obj_pos, lens, labels, device)
    cache = ds.tree_cache(prune_k)
    for idx in staging.length_buckets(lens, 50):
        batch = ds.batch(idx, word_dropout=0.04)
        logits, pooled = model(batch.inputs, trees=cache.batch(batch.idx, batch.T))
        loss = model.loss(logits, pooled, batch.labels)

No CPU path exists: `build` raises when the device is not a GPU or libgcnpt.so is missing.
"""
import numpy as np
import torch

from . import _lib
from .model.tree import TreeCache, TreeError

FIELDS = ("words", "pos", "ner", "deprel", "head", "subj_pos", "obj_pos")
POS_FILL = 150             # data/loader.py:120-121


class BatchError(TreeError):
    """A slot of the batch holds no sentence; `.sentence` (the slot) and `.code` (E_INVALID: index outside the dataset, E_LENGTH: the
    sentence is longer than the batch is padded to)."""


def _draw_seed():
    """One dropout seed from the CPU generator (torch.manual_seed fixes it): no GPU sync."""
    return int(torch.randint(0, 2 ** 62, (1,)).item())


def _int32(a, name, device, shape=None):
    """An integer array (NumPy or torch, any integer dtype) as a contiguous int32 tensor on `device`; refuses what does not fit."""
    if isinstance(a, np.ndarray):
        a = np.ascontiguousarray(a) if a.flags.writeable else a.copy()             # (torch wraps writable arrays only)
    t = torch.from_numpy(a) if isinstance(a, np.ndarray) else a
    if not torch.is_tensor(t):
        t = torch.as_tensor(np.asarray(a))
    if t.dtype.is_floating_point or t.dtype.is_complex or t.dtype == torch.bool:
        raise TypeError("DeviceDataset: %s must be an integer array, got %s" % (name, t.dtype))
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError("DeviceDataset: %s has shape %s, expected %s" % (name, tuple(t.shape), tuple(shape)))
    if t.numel() and t.dtype not in (torch.int32, torch.int16, torch.int8, torch.uint8):
        lo, hi = int(t.min()), int(t.max())
        if lo < -2 ** 31 or hi > 2 ** 31 - 1:
            raise ValueError("DeviceDataset: %s holds ids outside int32 (%d .. %d)" % (name, lo, hi))
    return t.to(device=device, dtype=torch.int32).contiguous()


class DeviceBatch(object):
    """
    One batch as the reference's loader hands it to the model (data/loader.py:140-141), in HBM.

    inputs  (words, masks, pos, ner, deprel, head, subj_pos, obj_pos), or the seven-field form without ner: int64 [B,T], masks bool
    labels  int64 [B]      lens  int32 [B]      status  int32 [B] (0 or a GCNPT_E_* code per slot)      idx  int64 [B] as used
    """

    def __init__(self, inputs, labels, lens, status, idx, T):
        self.inputs, self.labels, self.lens, self.status, self.idx, self.T = inputs, labels, lens, status, idx, T

    def check(self):
        """One host sync; raises BatchError for the first slot that holds no sentence."""
        st = self.status.cpu()
        bad = torch.nonzero(st != 0)
        if bad.numel():
            b = int(bad[0])
            raise BatchError(b, int(st[b]))
        return self


class DeviceDataset(object):
    """The dataset's token arrays in HBM: int32 [S,Ts] per field (ner: None for SemEval), lens / labels int32 [S], lens also on the host."""

    def __init__(self, arrays, lens, labels, lens_host):
        self.arrays, self.lens, self.labels, self.lens_host = arrays, lens, labels, lens_host
        self.S, self.Ts = (int(n) for n in arrays["words"].shape)

    def __len__(self):
        return self.S

    @property
    def device(self):
        return self.lens.device

    @classmethod
    def build(cls, words, pos, ner, deprel, head, subj_pos, obj_pos, lens, labels, device=None):
        """The integer arrays the reference's loader produces, NumPy or torch, any integer dtype: per-token arrays [S,Ts] padded to the
        dataset's longest sentence (what lies behind a sentence's end is never read), ner=None for SemEval; lens, labels [S]."""
        if device is None:
            device = words.device if torch.is_tensor(words) else "cpu"
        device = torch.device(device)
        if device.type != "cuda":
            raise TypeError("DeviceDataset runs on the GPU only (got %s); there is no CPU path" % device)
        _lib.lib()
        if getattr(words, "ndim", 0) != 2:
            raise ValueError("DeviceDataset: words must be [S,Ts] ids (BERT inputs, a 3-D words, are not supported)")
        shape = tuple(int(n) for n in words.shape)
        if shape[0] < 1 or shape[1] < 1:
            raise ValueError("DeviceDataset: empty dataset %s" % (shape,))
        given = dict(words=words, pos=pos, ner=ner, deprel=deprel, head=head, subj_pos=subj_pos, obj_pos=obj_pos)
        arrays = {k: None if (k == "ner" and v is None) else _int32(v, k, device, shape) for k, v in given.items()}
        lens_dev = _int32(lens, "lens", device, (shape[0],))
        return cls(arrays, lens_dev, _int32(labels, "labels", device, (shape[0],)), lens_dev.cpu().numpy())

    def batch(self, idx, T=None, word_dropout=0.0, seed=None, seed_dev=None, pos_fill=POS_FILL):
        """
        The loader tensors of the sentences idx (repeats allowed) in one launch; returns a DeviceBatch.
        idx: CUDA int64 tensor [B] (nothing synchronises; T is then required), or a host sequence, which is uploaded.
        T: the width the batch is padded to; None = the longest sentence of the batch, from the host copy of the lengths.
        word_dropout: loader.py:182-186 per batch slot, counter based on seed (None: drawn from the CPU generator) plus the device word
        seed_dev (int64 [1], optional: a captured step advances it between replays).
        """
        on_dev = torch.is_tensor(idx) and idx.is_cuda
        if on_dev:
            if T is None:
                raise ValueError("DeviceDataset.batch: T is required when idx lives on the device (the lengths would need a host sync)")
            idx_dev = idx.to(torch.int64).contiguous().view(-1)
        else:
            host = np.asarray(idx.cpu() if torch.is_tensor(idx) else idx).astype(np.int64).reshape(-1)
            if T is None:
                ok = host[(host >= 0) & (host < self.S)]
                T = max(int(self.lens_host[ok].max()) if ok.size else 1, 1)
            idx_dev = torch.from_numpy(host).to(self.device)
        B, T = int(idx_dev.numel()), int(T)
        p = float(word_dropout)
        if seed is None:
            seed = _draw_seed() if p > 0 else 0
        dev = self.device
        out = {k: torch.empty((B, T), dtype=torch.int64, device=dev) for k in FIELDS if self.arrays[k] is not None}
        masks = torch.empty((B, T), dtype=torch.bool, device=dev)
        labels = torch.empty((B,), dtype=torch.int64, device=dev)
        lens = torch.empty((B,), dtype=torch.int32, device=dev)
        status = torch.empty((B,), dtype=torch.int32, device=dev)
        P = _lib.ptr
        a = self.arrays
        _lib.check(_lib.lib().gcnpt_gather_batch(
            _lib.stream(), P(a["words"]), P(a["pos"]), P(a["ner"]), P(a["deprel"]), P(a["head"]), P(a["subj_pos"]), P(a["obj_pos"]),
            P(self.lens), P(self.labels), self.S, self.Ts, P(idx_dev), B, T, P(out["words"]), P(masks), P(out["pos"]), P(out.get("ner")),
            P(out["deprel"]), P(out["head"]), P(out["subj_pos"]), P(out["obj_pos"]), P(labels), P(lens), P(status), int(pos_fill), p,
            int(seed), P(seed_dev)))
        inputs = (out["words"], masks) + tuple(out[k] for k in FIELDS[1:] if k in out)
        return DeviceBatch(inputs, labels, lens, status, idx_dev, T)

    def tree_cache(self, prune_k, **kw):
        """TreeCache.build over the dataset's own parse arrays (through a transient int64 copy: the pruner reads int64)."""
        a = self.arrays
        return TreeCache.build(a["head"].long(), a["subj_pos"].long(), a["obj_pos"].long(), a["deprel"].long(), prune_k, lens=self.lens, **kw)
