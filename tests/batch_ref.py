"""NumPy restatement of what DeviceDataset.batch (gcnpt_gather_batch) must produce: the reference loader's batch assembly
(data/loader.py:93-141: get_long_tensor's pad fills -- PAD_ID for words / pos / ner / deprel / head, 150 for the two position fields --,
masks, labels) and its word dropout (loader.py:96-98, 182-186: a token whose id is not UNK_ID becomes UNK_ID when dropped), with the
Bernoulli draw replaced by the project's counter-based decision, which is part of the contract: drop_hash / drop_keep of
csrc/layer_common.h in uint32 arithmetic, keyed on (seed + seed_dev, b*T + t, column pair 0), low half, 16-bit threshold of float32 p.
Nothing of the reference is executed."""
import numpy as np

PAD_ID, UNK_ID, POS_FILL = 0, 1, 150
E_INVALID, E_LENGTH = -1, -11
ID_FIELDS = ("words", "pos", "ner", "deprel", "head", "subj_pos", "obj_pos")
M32 = np.uint64(0xFFFFFFFF)


def drop_hash(seed, row, col_pair):
    """csrc/layer_common.h drop_hash: seed a Python int (taken mod 2^64), row / col_pair uint32 arrays or ints -> uint32 array."""
    seed = int(seed) % (1 << 64)
    lo, hi = np.uint64(seed & 0xFFFFFFFF), np.uint64(seed >> 32)
    row, col_pair = np.asarray(row, dtype=np.uint64) & M32, np.asarray(col_pair, dtype=np.uint64) & M32
    x = (row * np.uint64(0x9E3779B1) + col_pair * np.uint64(0x85EBCA77) + lo) & M32
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x2C1B3C6D)) & M32
    x = (x + hi) & M32
    x ^= x >> np.uint64(12)
    x = (x * np.uint64(0x297A2D39)) & M32
    x ^= x >> np.uint64(15)
    return x.astype(np.uint32)


def thresh16(p):
    """The 16-bit drop threshold of a float32 probability: (unsigned)((double)p * 65536.0)."""
    return int(np.float64(np.float32(p)) * 65536.0)


def drop_keep(h, col, th):
    h = np.asarray(h, dtype=np.uint32)
    half = (h >> np.uint32(16)) if (col & 1) else (h & np.uint32(0xFFFF))
    return half >= np.uint32(th)


def word_drop_decisions(B, T, p, seed, seed_dev=0):
    """bool [B,T]: slot (b, t) is dropped (whether or not a droppable token sits there)."""
    key = np.arange(B * T, dtype=np.uint64).reshape(B, T)
    return ~drop_keep(drop_hash(int(seed) + int(seed_dev), key, 0), 0, thresh16(p))


def batch_ref(ds, idx, T, p=0.0, seed=0, seed_dev=0, pos_fill=POS_FILL):
    """ds: {field: int array [S,Ts] (ner may be None), 'lens': [S], 'labels': [S]}; idx: sentence numbers [B].  Returns a dict with the
    seven id fields (int64 [B,T]; no 'ner' when the dataset has none), masks (bool), labels (int64 [B]), lens and status (int32 [B])."""
    idx = np.asarray(idx, dtype=np.int64)
    S, Ts = ds["words"].shape
    B = len(idx)
    fields = [k for k in ID_FIELDS if ds.get(k) is not None]
    out = {k: np.full((B, T), pos_fill if k in ("subj_pos", "obj_pos") else PAD_ID, dtype=np.int64) for k in fields}
    out.update(masks=np.ones((B, T), dtype=bool), labels=np.zeros((B,), np.int64), lens=np.zeros((B,), np.int32),
               status=np.zeros((B,), np.int32))
    for b, s in enumerate(idx):
        if s < 0 or s >= S:
            out["status"][b] = E_INVALID
            continue
        n = int(ds["lens"][s])
        if n > T or n > Ts:
            out["status"][b] = E_LENGTH
            continue
        for k in fields:
            out[k][b, :n] = ds[k][s, :n]
        out["masks"][b, :n] = False
        out["labels"][b] = ds["labels"][s]
        out["lens"][b] = n
    if thresh16(p) > 0:
        drop = word_drop_decisions(B, T, p, seed, seed_dev) & ~out["masks"] & (out["words"] != UNK_ID)
        out["words"][drop] = UNK_ID
    return out
