"""CPU-side checks of the device-resident dataset's entry point (include/gcnpt.h gcnpt_gather_batch) and of tests/batch_ref.py, the NumPy
restatement the GPU tests compare against: the symbol is exported and bound, argument validation returns GCNPT_E_INVALID with a text that
names the entry point before anything is launched, the Python surface refuses a CPU device, and the restatement reproduces the loader's
position fields and pad fills.  No compute is launched here."""
import ctypes

import numpy as np
import pytest

import batch_ref
from gcn_over_pruned_trees_amd import _lib
from gcn_over_pruned_trees_amd.utils import synthetic


def test_gather_batch_symbol_exported_and_bound():
    handle = ctypes.CDLL(_lib.LIB_PATH)
    assert "gcnpt_gather_batch" in _lib.SIGNATURES
    assert hasattr(handle, "gcnpt_gather_batch")
    assert len(_lib.SIGNATURES["gcnpt_gather_batch"][1]) == 30
    assert _lib.lib().gcnpt_abi_version() == 7                      # additive: nothing existing changed


def _call(p, **kw):
    a = dict(src_words=p, src_pos=p, src_ner=p, src_deprel=p, src_head=p, src_subj_pos=p, src_obj_pos=p, src_len=p, src_label=p, S=3, Ts=5,
             idx=p, B=2, T=5, words=p, masks=p, pos=p, ner=p, deprel=p, head=p, subj_pos=p, obj_pos=p, labels=p, lens=p, status=p,
             pos_fill=150, p_word=0.0)
    a.update(kw)
    return _lib.lib().gcnpt_gather_batch(None, a["src_words"], a["src_pos"], a["src_ner"], a["src_deprel"], a["src_head"], a["src_subj_pos"],
                                         a["src_obj_pos"], a["src_len"], a["src_label"], a["S"], a["Ts"], a["idx"], a["B"], a["T"],
                                         a["words"], a["masks"], a["pos"], a["ner"], a["deprel"], a["head"], a["subj_pos"], a["obj_pos"],
                                         a["labels"], a["lens"], a["status"], a["pos_fill"], a["p_word"], 1, None)


REQUIRED = ("src_words", "src_pos", "src_deprel", "src_head", "src_subj_pos", "src_obj_pos", "src_len", "src_label", "idx", "words", "masks",
            "pos", "deprel", "head", "subj_pos", "obj_pos", "labels")
BAD = ([{k: None} for k in REQUIRED] + [dict(src_ner=None), dict(ner=None)] +
       [{k: v} for k in ("S", "Ts", "B", "T") for v in (0, -2)] +
       [dict(p_word=1.0), dict(p_word=1.5), dict(p_word=-0.1), dict(p_word=float("nan"))])


@pytest.mark.parametrize("bad", BAD, ids=lambda d: ",".join("%s=%s" % kv for kv in d.items()))
def test_gather_batch_refusals_need_no_gpu(bad):
    L = _lib.lib()
    buf = ctypes.create_string_buffer(256)
    assert _call(ctypes.addressof(buf), **bad) == _lib.E_INVALID, bad
    assert L.gcnpt_last_error().startswith(b"gcnpt_gather_batch:"), L.gcnpt_last_error()


def test_gather_batch_refusal_texts():
    L = _lib.lib()
    buf = ctypes.create_string_buffer(256)
    p = ctypes.addressof(buf)
    assert _call(p, B=0) == _lib.E_INVALID and b"positive" in L.gcnpt_last_error()
    assert _call(p, ner=None) == _lib.E_INVALID and b"go together" in L.gcnpt_last_error()
    assert _call(p, p_word=1.0) == _lib.E_INVALID and b"[0, 1)" in L.gcnpt_last_error()
    assert _call(p, idx=None) == _lib.E_INVALID and b"null" in L.gcnpt_last_error()


def test_device_dataset_refuses_cpu():
    import torch
    from gcn_over_pruned_trees_amd import dataset
    ids = torch.zeros((3, 5), dtype=torch.int64)
    one = torch.ones((3,), dtype=torch.int64)
    with pytest.raises(TypeError, match="GPU only"):
        dataset.DeviceDataset.build(ids, ids, ids, ids, ids, ids, ids, one, one)             # the tensors' own device
    with pytest.raises(TypeError, match="GPU only"):
        dataset.DeviceDataset.build(ids.numpy(), ids.numpy(), None, ids.numpy(), ids.numpy(), ids.numpy(), ids.numpy(), one.numpy(),
                                    one.numpy(), device="cpu")


def test_batch_ref_hash_is_the_kernels():
    """drop_hash / thresh16 by hand for a few keys (csrc/layer_common.h, in Python integers)."""
    def by_hand(seed, row, cp):
        m = 0xFFFFFFFF
        x = (row * 0x9E3779B1 + cp * 0x85EBCA77 + (seed & m)) & m
        x ^= x >> 15
        x = (x * 0x2C1B3C6D) & m
        x = (x + (seed >> 32)) & m
        x ^= x >> 12
        x = (x * 0x297A2D39) & m
        x ^= x >> 15
        return x
    for seed in (0, 1, 0x123456789ABCDEF, 2 ** 64 - 1):
        rows = np.array([0, 1, 44, 1664, 2 ** 31 - 1, 2 ** 32 - 1], dtype=np.uint64)
        got = batch_ref.drop_hash(seed, rows, 0)
        assert got.dtype == np.uint32 and [int(v) for v in got] == [by_hand(seed, int(r), 0) for r in rows]
    assert int(batch_ref.drop_hash(2 ** 64 + 5, 7, 0)) == int(batch_ref.drop_hash(5, 7, 0))            # seed + seed_dev wraps mod 2^64
    assert batch_ref.thresh16(0.25) == 16384 and batch_ref.thresh16(0.0) == 0 and batch_ref.thresh16(0.04) == 2621
    assert batch_ref.thresh16(0.9999999) == 65535


def test_batch_ref_reproduces_position_fields():
    """get_positions-style rows (data/loader.py:162-165 through utils/synthetic.positions) come back for the real tokens, 150 behind them."""
    spans = [(0, 0, 7), (2, 4, 9), (5, 5, 6), (0, 2, 3), (8, 8, 9)]
    S, Ts = len(spans), 9
    ds = {k: np.zeros((S, Ts), np.int64) for k in batch_ref.ID_FIELDS}
    ds["lens"] = np.array([n for _, _, n in spans], np.int32)
    ds["labels"] = np.arange(S, dtype=np.int64) + 3
    for s, (a, e, n) in enumerate(spans):
        ds["subj_pos"][s, :n] = synthetic.positions(a, e, n)
        ds["obj_pos"][s, :n] = synthetic.positions(n - 1 - e, n - 1 - a, n)
        ds["subj_pos"][s, n:] = -99                                  # what lies behind a sentence's end is never taken over
        ds["words"][s, :n] = 10 + np.arange(n)
    idx = [4, 1, 1, 0, 3, 2]
    got = batch_ref.batch_ref(ds, idx, 9)
    for b, s in enumerate(idx):
        a, e, n = spans[s]
        assert got["subj_pos"][b].tolist() == synthetic.positions(a, e, n) + [150] * (9 - n)
        assert got["obj_pos"][b].tolist() == synthetic.positions(n - 1 - e, n - 1 - a, n) + [150] * (9 - n)
        assert (got["subj_pos"][b, :n] == 0).sum() == e - a + 1
    assert got["labels"].tolist() == [7, 4, 4, 3, 6, 5] and got["lens"].tolist() == [9, 9, 9, 7, 3, 6] and not got["status"].any()
    assert np.array_equal(got["masks"], got["words"] == 0)          # the reference's derivation (loader.py:110) agrees with the lengths


def test_batch_ref_pad_fills_by_hand():
    ds = dict(words=np.array([[5, 1, 7, 9], [8, 0, 0, 0], [4, 6, 1, 0]]), pos=np.array([[3, 4, 5, 6], [2, 9, 9, 9], [7, 7, 7, 9]]), ner=None,
              deprel=np.array([[11, 12, 13, 14], [15, 0, 0, 0], [16, 17, 18, 0]]), head=np.array([[2, 0, 2, 3], [0, 0, 0, 0], [0, 1, 1, 0]]),
              subj_pos=np.array([[0, 1, 2, 3], [0, 150, 150, 150], [-1, 0, 1, 150]]), obj_pos=np.array([[-3, -2, -1, 0], [0, 150, 150, 150], [0, 1, 2, 150]]),
              lens=np.array([4, 1, 3]), labels=np.array([9, 8, 7]))
    got = batch_ref.batch_ref(ds, [2, 0, 1, 3, -1], 5)
    assert "ner" not in got
    assert got["words"].tolist() == [[4, 6, 1, 0, 0], [5, 1, 7, 9, 0], [8, 0, 0, 0, 0], [0] * 5, [0] * 5]
    assert got["pos"].tolist() == [[7, 7, 7, 0, 0], [3, 4, 5, 6, 0], [2, 0, 0, 0, 0], [0] * 5, [0] * 5]
    assert got["head"].tolist() == [[0, 1, 1, 0, 0], [2, 0, 2, 3, 0], [0] * 5, [0] * 5, [0] * 5]
    assert got["subj_pos"].tolist() == [[-1, 0, 1, 150, 150], [0, 1, 2, 3, 150], [0, 150, 150, 150, 150], [150] * 5, [150] * 5]
    assert got["obj_pos"].tolist() == [[0, 1, 2, 150, 150], [-3, -2, -1, 0, 150], [0, 150, 150, 150, 150], [150] * 5, [150] * 5]
    assert got["masks"].tolist() == [[False] * 3 + [True] * 2, [False] * 4 + [True], [False] + [True] * 4, [True] * 5, [True] * 5]
    assert got["labels"].tolist() == [7, 9, 8, 0, 0] and got["lens"].tolist() == [3, 4, 1, 0, 0]
    assert got["status"].tolist() == [0, 0, 0, batch_ref.E_INVALID, batch_ref.E_INVALID]
    short = batch_ref.batch_ref(ds, [0, 2], 3)                      # T below a sentence's length: an empty row, E_LENGTH
    assert short["status"].tolist() == [batch_ref.E_LENGTH, 0] and short["words"].tolist() == [[0, 0, 0], [4, 6, 1]]
    assert short["subj_pos"].tolist() == [[150] * 3, [-1, 0, 1]] and short["masks"].tolist() == [[True] * 3, [False] * 3]
    # word dropout: only real tokens that are not UNK_ID change, and only to UNK_ID
    full = batch_ref.batch_ref(ds, [0, 0, 2, 1], 4)
    dropped = batch_ref.batch_ref(ds, [0, 0, 2, 1], 4, p=0.5, seed=11)
    changed = dropped["words"] != full["words"]
    assert changed.any() and (dropped["words"][changed] == 1).all() and (full["words"][changed] > 1).all() and not full["masks"][changed].any()
    assert all(np.array_equal(dropped[k], full[k]) for k in full if k != "words")
