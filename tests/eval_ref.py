"""NumPy restatement of the two evaluation launches (include/gcnpt.h gcnpt_eval_batch / gcnpt_eval_finish; reference model/trainer.py:118-124
and utils/scorer.py:20-96 in confusion-matrix form): what the accumulators must hold after a batch and what the finishing launch makes of
them.  Counts are integers and exact; the per-row loss is float64 (the kernels' float32 is compared within a tolerance); precision, recall
and F1 are Python-float arithmetic in scorer.py:84-92's own order, which tests/golden/scorer_cases.npz holds to the reference's scorer.
Nothing of the reference is executed."""
import numpy as np

FINISH_THREADS, FINISH_GROUP = 1024, 32        # csrc/eval_kernels.hip: the fixed order of the loss sum


def new_state(S, C, want_probs=True):
    """The caller's buffers at their required initial values."""
    return dict(pred=np.full((S,), -1, np.int64), probs=np.zeros((S, C), np.float64) if want_probs else None, row_loss=np.zeros((S,), np.float64),
                seen=np.zeros((S,), np.int32), confusion=np.zeros((C, C), np.int32), status=np.zeros((1,), np.int32))


def eval_batch_ref(st, logits, labels, idx, slot_status=None):
    """One gcnpt_eval_batch on the state `st`, in place.  logits float32 [M,C]; the loss and the softmax are computed in float64."""
    logits = np.asarray(logits, dtype=np.float32)
    M, C = logits.shape
    S = st["pred"].shape[0]
    for m in range(M):
        s = int(idx[m])
        if (slot_status is not None and int(slot_status[m]) != 0) or s < 0 or s >= S:
            continue
        z = logits[m].astype(np.float64)
        p = int(np.argmax(logits[m]))                                 # the lowest index on ties; 0 for an all-NaN row
        with np.errstate(invalid="ignore", over="ignore"):
            mx = np.max(z)
            e = np.exp(z - mx)
            den = e.sum()
        st["pred"][s] = p
        if st["probs"] is not None:
            st["probs"][s] = e / den
        y = int(labels[m])
        if 0 <= y < C:
            st["row_loss"][s] = (mx - z[y]) + np.log(den)
            st["seen"][s] += 1
            st["confusion"][y, p] += 1
        else:
            st["row_loss"][s] = 0.0
            st["status"][0] |= 1
    return st


def prf(correct, guessed, gold):
    """scorer.py:84-92, literally, in Python floats."""
    prec_micro = 1.0
    if guessed > 0:
        prec_micro = float(correct) / float(guessed)
    recall_micro = 0.0
    if gold > 0:
        recall_micro = float(correct) / float(gold)
    f1_micro = 0.0
    if prec_micro + recall_micro > 0.0:
        f1_micro = 2.0 * prec_micro * recall_micro / (prec_micro + recall_micro)
    return prec_micro, recall_micro, f1_micro


def loss_fixed_order(row_loss, seen):
    """The finishing launch's sum, in its order, in float64: thread t of 1024 adds sentences t, t + 1024, ... in order; the partials are
    added 32 at a time in thread order, then the 32 sums in order; divided by the number of sentences with seen > 0 (0.0 when none)."""
    row = np.asarray(row_loss).astype(np.float64)
    live = np.asarray(seen) > 0
    part = [0.0] * FINISH_THREADS
    for t in range(min(FINISH_THREADS, len(row))):
        acc = 0.0
        for s in range(t, len(row), FINISH_THREADS):
            if live[s]:
                acc += float(row[s])
        part[t] = acc
    total = 0.0
    for g in range(FINISH_THREADS // FINISH_GROUP):
        sub = 0.0
        for q in range(FINISH_GROUP):
            sub += part[g * FINISH_GROUP + q]
        total += sub
    n = int(live.sum())
    return total / float(n) if n > 0 else 0.0


def eval_finish_ref(confusion, seen, row_loss, no_relation):
    """gcnpt_eval_finish: (by_relation int32 [3,C], totals int32 [6], metrics float64 [4])."""
    confusion = np.asarray(confusion).astype(np.int64)
    by = np.stack([np.diag(confusion), confusion.sum(0), confusion.sum(1)])
    if no_relation >= 0:
        by[:, no_relation] = 0
    n_seen = int((np.asarray(seen) > 0).sum())
    correct, guessed, gold = (int(v) for v in by.sum(1))
    totals = np.array([int(confusion.sum()), n_seen, correct, guessed, gold, len(seen) - n_seen], np.int32)
    metrics = np.array((loss_fixed_order(row_loss, seen),) + prf(correct, guessed, gold), np.float64)
    return by.astype(np.int32), totals, metrics


def confusion_of(gold, pred, C):
    """Dense [C,C] counts, gold x predicted (scorer.py:98-106 as an array)."""
    conf = np.zeros((C, C), np.int32)
    np.add.at(conf, (np.asarray(gold, np.int64), np.asarray(pred, np.int64)), 1)
    return conf


def score_ref(gold, pred, C, no_relation=0):
    """(confusion, (P, R, F1)) of class-id sequences: what scorer.score gives on the ids' names, through the confusion matrix."""
    conf = confusion_of(gold, pred, C)
    by, _, metrics = eval_finish_ref(conf, np.ones((1,), np.int32), np.zeros((1,), np.float32), no_relation)
    return conf, tuple(float(v) for v in metrics[1:])
