"""CPU-side checks of the device-side evaluation's entry points (include/gcnpt.h gcnpt_eval_batch / gcnpt_eval_finish) and of
tests/eval_ref.py, the NumPy restatement the GPU tests compare against: the symbols are declared, exported and bound, argument validation
answers before anything is launched with a text that starts with the entry point's name, the Python surface refuses a CPU device, and the
restatement reproduces the reference scorer's precision / recall / F1 (equal as float64) and confusion counts on the recorded cases of
tests/golden/scorer_cases.npz (tests/golden/make_golden_scorer.py).  No compute is launched here."""
import ctypes
import os
import re

import numpy as np
import pytest

import eval_ref
from conftest import ROOT, load_golden
from gcn_over_pruned_trees_amd import _lib

NAMES = ("gcnpt_eval_batch", "gcnpt_eval_finish")


def test_eval_symbols_declared_exported_and_bound():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gcnpt.h")).read(), flags=re.S)
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _lib.SIGNATURES and hasattr(handle, name), name
    assert len(_lib.SIGNATURES["gcnpt_eval_batch"][1]) == 15 and len(_lib.SIGNATURES["gcnpt_eval_finish"][1]) == 10
    assert _lib.lib().gcnpt_abi_version() == _lib.ABI_VERSION == 7       # additive: nothing existing changed


def _batch(p, **kw):
    a = dict(logits=p, labels=p, idx=p, slot_status=p, M=3, C=5, S=4, no_relation=0, pred=p, probs=p, row_loss=p, seen=p, confusion=p, status=p)
    a.update(kw)
    return _lib.lib().gcnpt_eval_batch(None, a["logits"], a["labels"], a["idx"], a["slot_status"], a["M"], a["C"], a["S"], a["no_relation"],
                                       a["pred"], a["probs"], a["row_loss"], a["seen"], a["confusion"], a["status"])


def _finish(p, **kw):
    a = dict(confusion=p, seen=p, row_loss=p, C=5, S=4, no_relation=0, by_relation=p, totals=p, metrics=p)
    a.update(kw)
    return _lib.lib().gcnpt_eval_finish(None, a["confusion"], a["seen"], a["row_loss"], a["C"], a["S"], a["no_relation"], a["by_relation"],
                                        a["totals"], a["metrics"])


BAD_BATCH = ([{k: None} for k in ("logits", "labels", "idx", "pred", "row_loss", "seen", "confusion")] +
             [dict(M=0), dict(M=-1), dict(C=0), dict(S=0), dict(no_relation=5), dict(no_relation=-2)])
BAD_FINISH = ([{k: None} for k in ("confusion", "seen", "row_loss", "by_relation", "totals", "metrics")] +
              [dict(C=0), dict(S=0), dict(S=-3), dict(no_relation=5), dict(no_relation=-2)])
_ids = lambda d: ",".join("%s=%s" % kv for kv in d.items())  # noqa: E731


@pytest.mark.parametrize("bad", BAD_BATCH, ids=_ids)
def test_eval_batch_refusals_need_no_gpu(bad):
    buf = ctypes.create_string_buffer(256)
    assert _batch(ctypes.addressof(buf), **bad) == _lib.E_INVALID, bad
    assert _lib.lib().gcnpt_last_error().startswith(b"gcnpt_eval_batch:"), _lib.lib().gcnpt_last_error()


@pytest.mark.parametrize("bad", BAD_FINISH, ids=_ids)
def test_eval_finish_refusals_need_no_gpu(bad):
    buf = ctypes.create_string_buffer(256)
    assert _finish(ctypes.addressof(buf), **bad) == _lib.E_INVALID, bad
    assert _lib.lib().gcnpt_last_error().startswith(b"gcnpt_eval_finish:"), _lib.lib().gcnpt_last_error()


def test_eval_class_limit_and_validation_order():
    """C = 1025 is E_UNSUPPORTED from both calls; no_relation = -1 (no class excluded) passes validation, shown without a launch by the
    call going on to the next refusal: it reports the class limit, not no_relation."""
    L = _lib.lib()
    buf = ctypes.create_string_buffer(256)
    p = ctypes.addressof(buf)
    for call, name in ((_batch, b"gcnpt_eval_batch:"), (_finish, b"gcnpt_eval_finish:")):
        assert call(p, C=1025) == _lib.E_UNSUPPORTED
        assert L.gcnpt_last_error().startswith(name) and b"1024" in L.gcnpt_last_error()
        assert call(p, C=1025, no_relation=-1) == _lib.E_UNSUPPORTED and b"no_relation" not in L.gcnpt_last_error()
        assert call(p, C=1025, no_relation=1024) == _lib.E_UNSUPPORTED
        assert call(p, C=1025, no_relation=1025) == _lib.E_INVALID and b"no_relation" in L.gcnpt_last_error()
        assert call(p, C=1024, no_relation=-2) == _lib.E_INVALID and b"no_relation" in L.gcnpt_last_error()
    assert _batch(p, logits=None) == _lib.E_INVALID and b"null" in L.gcnpt_last_error()
    assert _batch(p, M=0) == _lib.E_INVALID and b"positive" in L.gcnpt_last_error()


def test_evaluate_refuses_cpu():
    import torch
    from gcn_over_pruned_trees_amd import evaluate
    with pytest.raises(TypeError, match="GPU only"):
        evaluate.EvalState(4, 5, "cpu")
    with pytest.raises(TypeError, match="GPU only"):
        evaluate.EvalState(4, 5, torch.device("cpu"), no_relation=-1, want_probs=True)

    class CpuDataset(object):
        device, S, Ts, lens_host = torch.device("cpu"), 3, 5, np.array([5, 2, 3])

    class Model(object):
        opt = dict(num_class=5, gcn_check_trees=False)

    with pytest.raises(TypeError, match="GPU only"):
        evaluate.Evaluator(Model(), CpuDataset(), 2)
    # a state cannot exist without a GPU, so add()'s refusal of CPU tensors is reached through an instance that skipped the constructor
    st = object.__new__(evaluate.EvalState)
    st.S, st.C, st.no_relation = 4, 5, 0
    z, y = torch.zeros((2, 5)), torch.zeros((2,), dtype=torch.int64)
    with pytest.raises(TypeError, match="GPU only"):
        st.add(z, y, y)


def test_evaluator_refuses_a_checking_model_under_graph():
    """Refused before the device is looked at twice: the option's name is in the message."""
    import torch
    from gcn_over_pruned_trees_amd import evaluate

    class Dataset(object):
        device, S, Ts, lens_host = torch.device("cuda:0"), 3, 5, np.array([5, 2, 3])

    class Model(object):
        opt = dict(num_class=5, gcn_check_trees=True)

    with pytest.raises(ValueError, match="gcn_check_trees"):
        evaluate.Evaluator(Model(), Dataset(), 2, graph=True)


# ---- eval_ref against the reference scorer's recorded results ----
def _cases():
    g = load_golden("scorer_cases.npz")
    return [(str(g["names"][k]), int(g["C"][k]), g["gold_%02d" % k], g["pred_%02d" % k], g["conf_%02d" % k], g["prf"][k]) for k in range(len(g["C"]))]


def test_scorer_fixture_holds_the_cases_it_should():
    cases = _cases()
    names = [c[0] for c in cases]
    assert len(cases) >= 35 and len(set(names)) == len(names)
    for part in ("random_C42", "random_C10", "all_pred_no_relation", "all_gold_no_relation", "both_all_no_relation", "single_", "perfect"):
        assert any(n.startswith(part) for n in names), part
    for name, C, gold, pred, conf, prf in cases:
        assert gold.dtype == pred.dtype == conf.dtype == np.int32 and prf.dtype == np.float64
        assert gold.shape == pred.shape and conf.shape == (C, C) and 0 <= gold.min() and gold.max() < C and 0 <= pred.min() and pred.max() < C
    by_name = {c[0]: c for c in cases}
    assert by_name["both_all_no_relation_C42"][5].tolist() == [1.0, 0.0, 0.0]           # no guess: P = 1; no gold: R = 0
    assert by_name["perfect_C10"][5].tolist() == [1.0, 1.0, 1.0]
    assert by_name["all_pred_no_relation_C10"][5].tolist() == [1.0, 0.0, 0.0]
    assert by_name["all_gold_no_relation_C10"][5].tolist() == [0.0, 0.0, 0.0]


def test_eval_ref_equals_the_reference_scorer():
    """P, R and F1 equal as float64 (not close: equal), the confusion matrix equal to compute_confusion_matrices' counts -- through
    score_ref, and through the two restated launches fed one-hot logits in three batches of shuffled rows."""
    rng = np.random.RandomState(3)
    for name, C, gold, pred, conf, prf in _cases():
        got_conf, got_prf = eval_ref.score_ref(gold, pred, C, no_relation=0)
        assert np.array_equal(got_conf, conf), name
        assert got_prf == tuple(prf.tolist()), (name, got_prf, prf.tolist())
        if len(gold) > 300:
            continue
        S = len(gold)
        logits = np.zeros((S, C), np.float32)
        logits[np.arange(S), pred] = 1.0
        st = eval_ref.new_state(S, C)
        order = rng.permutation(S)
        for part in np.array_split(order, 3):
            if len(part):
                eval_ref.eval_batch_ref(st, logits[part], gold[part], part)
        by, totals, metrics = eval_ref.eval_finish_ref(st["confusion"], st["seen"], st["row_loss"], 0)
        assert np.array_equal(st["pred"], pred) and np.array_equal(st["confusion"], conf) and (st["seen"] == 1).all(), name
        assert tuple(metrics[1:].tolist()) == tuple(prf.tolist()), name
        assert totals.tolist()[:2] == [S, S] and totals[5] == 0 and not st["status"][0]
        keep = np.arange(C) != 0
        assert np.array_equal(by[2], conf.sum(1) * keep) and np.array_equal(by[1], conf.sum(0) * keep) and np.array_equal(by[0], np.diag(conf) * keep)
        assert totals.tolist()[2:5] == [int(v) for v in by.sum(1)]


def test_eval_ref_edges_by_hand():
    """Skipped slots, a bad label, a sentence scored twice, ties, an all-NaN row and no_relation = -1, on numbers small enough to check."""
    C, S = 3, 5
    logits = np.array([[0.0, 2.0, 2.0], [1.0, 1.0, 1.0], [np.nan] * 3, [5.0, 0.0, -5.0], [0.0, 0.0, 9.0], [0.0, 9.0, 0.0]], np.float32)
    labels = np.array([1, 0, 0, 7, 2, 2])
    idx = np.array([3, 0, 1, 2, 3, -1])
    st = eval_ref.eval_batch_ref(eval_ref.new_state(S, C), logits, labels, idx, slot_status=np.array([0, 0, 0, 0, 0, 0]))
    assert st["pred"].tolist() == [0, 0, 0, 2, -1] and st["seen"].tolist() == [1, 1, 0, 2, 0] and st["status"][0] == 1
    assert st["confusion"].tolist() == [[2, 0, 0], [0, 1, 0], [0, 0, 1]] and st["row_loss"][2] == 0.0
    assert abs(st["row_loss"][0] - np.log(3.0)) < 1e-12 and abs(st["probs"][2].sum() - 1.0) < 1e-12
    by, totals, metrics = eval_ref.eval_finish_ref(st["confusion"], st["seen"], st["row_loss"], 0)
    assert by.tolist() == [[0, 1, 1], [0, 1, 1], [0, 1, 1]] and totals.tolist() == [4, 3, 2, 2, 2, 2]
    assert metrics[1:].tolist() == [1.0, 1.0, 1.0]
    by, totals, _ = eval_ref.eval_finish_ref(st["confusion"], st["seen"], st["row_loss"], -1)
    assert by.tolist() == [[2, 1, 1], [2, 1, 1], [2, 1, 1]] and totals.tolist() == [4, 3, 4, 4, 4, 2]
    skipped = eval_ref.eval_batch_ref(eval_ref.new_state(S, C), logits, labels, idx, slot_status=np.array([0, -1, 0, -11, 0, 0]))
    assert skipped["pred"].tolist() == [-1, 0, -1, 2, -1] and skipped["status"][0] == 0 and skipped["seen"].tolist() == [0, 1, 0, 2, 0]
    # the fixed-order loss is the plain mean up to rounding, over seen sentences only
    rng = np.random.RandomState(5)
    row, seen = rng.random_sample(2500).astype(np.float32), (rng.random_sample(2500) < 0.7).astype(np.int32)
    assert abs(eval_ref.loss_fixed_order(row, seen) - row[seen > 0].astype(np.float64).mean()) < 1e-12
    assert eval_ref.loss_fixed_order(row, np.zeros_like(seen)) == 0.0
