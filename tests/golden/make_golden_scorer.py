#!/usr/bin/env python3
"""
Generates tests/golden/scorer_cases.npz by IMPORTING the reference's utils/scorer.py (read-only; its checkout is named by the environment
variable GCNPT_REFERENCE) and recording what `score` and `compute_confusion_matrices` return on fixed class-id sequences.  Only data is
written -- int arrays `gold_NN` / `pred_NN`, the class count `C`, float64 `prf` = (P, R, F1) per case, the confusion counts as a dense
[C,C] array `conf_NN` and the cases' names -- never reference source.  Class id 0 stands for the scorer's NO_RELATION, id k > 0 for
"rel_k".  Re-run:  GCNPT_REFERENCE=<reference checkout> PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_scorer.py
"""
import contextlib
import io
import json
import os
import sys

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("GCNPT_REFERENCE")
if not REF or not os.path.isdir(REF):
    sys.exit("set GCNPT_REFERENCE to a checkout of gstoica27/gcn-over-pruned-trees")
sys.path.insert(0, REF)

import numpy as np  # noqa: E402

from utils import scorer  # noqa: E402  (reference)

META = json.dumps(dict(numpy=np.__version__, python=sys.version.split()[0], reference="gstoica27/gcn-over-pruned-trees utils/scorer.py"))


def name_of(k):
    return scorer.NO_RELATION if k == 0 else "rel_%d" % k


def cases():
    rng = np.random.RandomState(2024)
    out = []
    for C, sizes in ((42, (1, 2, 7, 50, 300, 1000, 3000)), (10, (1, 3, 23, 200, 1500))):
        for n in sizes:
            for p_none in (0.8, 0.2):                                 # TACRED is ~80 % no_relation; and the other way round
                def draw():
                    ids = rng.randint(1, max(C, 2), size=n)
                    return np.where(rng.random_sample(n) < p_none, 0, ids)
                gold = draw()
                agree = rng.random_sample(n) < 0.6
                out.append(("random_C%d_n%d_none%.1f" % (C, n, p_none), C, gold, np.where(agree, gold, draw())))
    for C in (42, 10):
        n = 64
        some = rng.randint(0, C, size=n)
        some[:3] = (1, C - 1, 0)
        zeros = np.zeros(n, np.int64)
        out.append(("all_pred_no_relation_C%d" % C, C, some, zeros))
        out.append(("all_gold_no_relation_C%d" % C, C, zeros, some))
        out.append(("both_all_no_relation_C%d" % C, C, zeros, zeros))
        out.append(("perfect_C%d" % C, C, some, some.copy()))
        out.append(("never_right_C%d" % C, C, some, (some + 1) % C))
    out.append(("single_right", 42, np.array([5]), np.array([5])))
    out.append(("single_wrong", 42, np.array([5]), np.array([6])))
    out.append(("single_no_relation", 42, np.array([0]), np.array([0])))
    out.append(("single_missed", 10, np.array([3]), np.array([0])))
    out.append(("single_spurious", 10, np.array([0]), np.array([3])))
    return out


def main():
    data = dict(meta=np.array(META))
    names, Cs, prf = [], [], []
    for k, (name, C, gold, pred) in enumerate(cases()):
        key = [name_of(int(g)) for g in gold]
        guess = [name_of(int(p)) for p in pred]
        with contextlib.redirect_stdout(io.StringIO()):
            p, r, f = scorer.score(key, guess)
        conf = np.zeros((C, C), np.int32)
        index = {name_of(c): c for c in range(C)}
        for g, row in scorer.compute_confusion_matrices(key, guess).items():
            for q, count in row.items():
                conf[index[g], index[q]] = count
        names.append(name)
        Cs.append(C)
        prf.append((p, r, f))
        data["gold_%02d" % k] = gold.astype(np.int32)
        data["pred_%02d" % k] = pred.astype(np.int32)
        data["conf_%02d" % k] = conf
    data.update(names=np.array(names), C=np.array(Cs, np.int32), prf=np.array(prf, np.float64))
    path = os.path.join(HERE, "scorer_cases.npz")
    np.savez_compressed(path, **data)
    print("%s: %d cases, %d bytes" % (path, len(names), os.path.getsize(path)))


if __name__ == "__main__":
    main()
