"""GPU tests of the device-side evaluation (csrc/eval_kernels.hip gcnpt_eval_batch / gcnpt_eval_finish, gcn_over_pruned_trees_amd.evaluate):
predictions in the dataset's order, per-sentence loss and confusion counts from one launch per batch, loss and micro-averaged scores from
one finishing launch.  The reference is tests/eval_ref.py, which tests/test_eval_capi.py holds to the reference's scorer.  Counts,
predictions, precision, recall and F1 are compared for equality; the float32 per-sentence loss and the mean loss against float64 within
helpers.FWD_RTOL (normwise); probs, pred and the per-row loss bit for bit against gcnpt_head_loss_fwd on the same logits."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import eval_ref
from helpers import FWD_RTOL, cuda_dev, gcn_api, max_rel
from gcn_over_pruned_trees_amd import _lib
from gcn_over_pruned_trees_amd.utils import staging, synthetic

pytestmark = pytest.mark.gpu

GUARD = 16                 # elements in front of and behind every raw output
SENTINEL = -777


@pytest.fixture(scope="module")
def dev():
    return cuda_dev()


@pytest.fixture(scope="module")
def api():
    return gcn_api()


class RawState(object):
    """The caller's buffers of the two entry points, each between two guard bands of SENTINEL; bodies at the header's initial values
    (probs and row_loss, which need none, at SENTINEL: an element nobody wrote shows)."""
    SPEC = (("pred", torch.int64, -1), ("probs", torch.float32, SENTINEL), ("row_loss", torch.float32, SENTINEL), ("seen", torch.int32, 0),
            ("confusion", torch.int32, 0), ("status", torch.int32, 0), ("by_relation", torch.int32, SENTINEL), ("totals", torch.int32, SENTINEL),
            ("metrics", torch.float64, SENTINEL))

    def __init__(self, S, C, dev, no_relation=0, want_probs=True):
        self.S, self.C, self.no_relation, self.dev = S, C, no_relation, dev
        sizes = dict(pred=S, probs=S * C, row_loss=S, seen=S, confusion=C * C, status=1, by_relation=3 * C, totals=6, metrics=4)
        self.bufs = {}
        for name, dtype, init in self.SPEC:
            if name == "probs" and not want_probs:
                continue
            t = torch.full((sizes[name] + 2 * GUARD,), SENTINEL, dtype=dtype, device=dev)
            t[GUARD:-GUARD] = init
            self.bufs[name] = t

    def P(self, name):
        t = self.bufs.get(name)
        return None if t is None else t.data_ptr() + GUARD * t.element_size()

    def add(self, logits, labels, idx, slot_status=None, with_status=True):
        z = torch.as_tensor(np.ascontiguousarray(logits, np.float32), device=self.dev)
        y = torch.as_tensor(np.asarray(labels, np.int64), device=self.dev)
        s = torch.as_tensor(np.asarray(idx, np.int64), device=self.dev)
        st = None if slot_status is None else torch.as_tensor(np.asarray(slot_status, np.int32), device=self.dev)
        P = self.P
        _lib.check(_lib.lib().gcnpt_eval_batch(_lib.stream(), _lib.ptr(z), _lib.ptr(y), _lib.ptr(s), _lib.ptr(st), z.shape[0], self.C, self.S,
                                               self.no_relation, P("pred"), P("probs"), P("row_loss"), P("seen"), P("confusion"),
                                               P("status") if with_status else None))
        torch.cuda.synchronize()

    def finish(self, no_relation=None):
        P = self.P
        nr = self.no_relation if no_relation is None else no_relation
        _lib.check(_lib.lib().gcnpt_eval_finish(_lib.stream(), P("confusion"), P("seen"), P("row_loss"), self.C, self.S, nr, P("by_relation"),
                                                P("totals"), P("metrics")))
        torch.cuda.synchronize()
        return self.host()

    def host(self):
        """Every buffer's body as NumPy, after asserting that no guard band was touched."""
        out = {}
        for name, t in self.bufs.items():
            h = t.cpu().numpy()
            assert (h[:GUARD] == SENTINEL).all() and (h[-GUARD:] == SENTINEL).all(), "%s: written outside the array" % name
            out[name] = h[GUARD:-GUARD].copy()
        if "probs" in out:
            out["probs"] = out["probs"].reshape(self.S, self.C)
        out["confusion"] = out["confusion"].reshape(self.C, self.C)
        out["by_relation"] = out["by_relation"].reshape(3, self.C)
        return out


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def assert_counts_equal(got, st, by, totals, metrics, what):
    assert np.array_equal(got["pred"], st["pred"]), (what, "pred")
    assert np.array_equal(got["seen"], st["seen"]), (what, "seen")
    assert np.array_equal(got["confusion"], st["confusion"]), (what, "confusion")
    assert int(got["status"][0]) == int(st["status"][0]), (what, "status")
    assert np.array_equal(got["by_relation"], by), (what, "by_relation")
    assert got["totals"].tolist() == totals.tolist(), (what, got["totals"].tolist(), totals.tolist())
    assert got["metrics"][1:].tolist() == metrics[1:].tolist(), (what, got["metrics"].tolist(), metrics.tolist())      # P, R, F1: equal


def head_loss_fwd(logits_dev, labels_dev=None, rows=None):
    """gcnpt_head_loss_fwd on the same logits: (probs, pred) over all rows, or with `rows` the loss of each of those rows alone (M = 1)."""
    M, C = logits_dev.shape
    if rows is None:
        probs = torch.empty((M, C), dtype=torch.float32, device=logits_dev.device)
        pred = torch.empty((M,), dtype=torch.int64, device=logits_dev.device)
        _lib.check(_lib.lib().gcnpt_head_loss_fwd(_lib.stream(), _lib.ptr(logits_dev), None, None, 0, 0, 0.0, M, C, None, _lib.ptr(probs),
                                                  _lib.ptr(pred), None))
        return probs.cpu().numpy(), pred.cpu().numpy()
    out = []
    loss = torch.empty((1,), dtype=torch.float32, device=logits_dev.device)
    for r in rows:
        _lib.check(_lib.lib().gcnpt_head_loss_fwd(_lib.stream(), logits_dev.data_ptr() + r * C * 4, labels_dev.data_ptr() + r * 8, None, 0, 0, 0.0,
                                                  1, C, _lib.ptr(loss), None, None, None))
        out.append(loss.cpu().numpy()[0])
    return np.array(out, np.float32)


SHAPES = [(1, 1), (7, 19), (50, 42), (5, 64), (5, 65), (300, 42), (3, 1024)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "M%d_C%d" % s)
def test_kernels_against_eval_ref(dev, shape):
    """The shapes cross the wave width in C (64 / 65, 1024) and the workgroup's four rows in M (5, 7, 50, 300).  Sentences: a shuffled
    subset of S = M + 3, so three are never seen; a quarter of the labels is class 0 (no_relation)."""
    M, C = shape
    S = M + 3
    rng = np.random.RandomState(1000 * M + C)
    logits = (rng.standard_normal((M, C)) * 3.0).astype(np.float32)
    labels = np.where(rng.random_sample(M) < 0.25, 0, rng.randint(0, C, size=M))
    idx = rng.permutation(S)[:M]
    want = eval_ref.eval_batch_ref(eval_ref.new_state(S, C), logits, labels, idx)
    raw = RawState(S, C, dev)
    raw.add(logits, labels, idx)
    for nr in (0, -1):
        got = raw.finish(nr)
        by, totals, metrics = eval_ref.eval_finish_ref(want["confusion"], want["seen"], want["row_loss"], nr)
        assert_counts_equal(got, want, by, totals, metrics, (shape, nr))
        assert totals.tolist()[:2] == [M, M] and totals[5] == 3
        print("eval %s no_relation=%d: loss %.9g (float64 %.9g), P R F1 %s" % (shape, nr, got["metrics"][0], metrics[0], got["metrics"][1:].tolist()))
        assert max_rel(got["metrics"][0], metrics[0]) <= FWD_RTOL
        # the fixed order, restated on the device's own float32 losses: the same double, bit for bit
        assert got["metrics"][0] == eval_ref.loss_fixed_order(got["row_loss"], got["seen"])
    live = want["seen"] > 0
    err = max_rel(got["row_loss"][live], want["row_loss"][live])
    print("eval %s: row_loss max-rel error %.3e" % (shape, err))
    assert err <= FWD_RTOL
    assert (got["row_loss"][~live] == SENTINEL).all() and (got["probs"][~live] == SENTINEL).all() and (got["pred"][~live] == -1).all()
    assert max_rel(got["probs"][live], want["probs"][live]) <= FWD_RTOL
    # bit-identity with the output head's launch on the same logits
    z_dev = torch.as_tensor(logits, device=dev)
    y_dev = torch.as_tensor(np.asarray(labels, np.int64), device=dev)
    h_probs, h_pred = head_loss_fwd(z_dev)
    assert np.array_equal(got["pred"][idx], h_pred) and same_bits(got["probs"][idx], h_probs)
    rows = sorted({0, M // 2, M - 1})
    assert same_bits(got["row_loss"][idx[rows]], head_loss_fwd(z_dev, y_dev, rows))
    # probs is optional
    lean = RawState(S, C, dev, want_probs=False)
    lean.add(logits, labels, idx)
    got2 = lean.finish(0)
    assert "probs" not in got2 and same_bits(got2["row_loss"], got["row_loss"]) and np.array_equal(got2["confusion"], got["confusion"])


def test_edge_rows(dev):
    """Exact ties take the lowest index; logits of +-1e4 give a finite loss; an all-NaN row predicts 0; a label of -1 or C sets the status
    bit, is not counted and touches no guard band; idx = -1, idx = S and a non-zero slot_status skip the row (pred stays -1); a sentence
    scored twice shows in totals[0] - totals[1]; an unseen sentence in totals[5]."""
    C, S = 67, 12
    z = np.zeros((11, C), np.float32)
    z[0, [3, 40, 66]] = 2.5                     # ties across lanes and across the two 64-column passes
    z[1, :] = 1.0                               # every class ties
    z[2, 5], z[2, 6] = 1e4, -1e4
    z[3, :] = np.nan
    z[4, 9] = 4.0                               # label -1
    z[5, 10] = 4.0                              # label C
    z[6, 11] = 4.0                              # idx -1
    z[7, 12] = 4.0                              # idx S
    z[8, 13] = 4.0                              # slot_status != 0
    z[9, 65] = 3.0                              # sentence 9 ...
    z[10, 64] = 3.0                             # ... scored twice
    labels = np.array([40, 2, 6, 0, -1, C, 1, 1, 1, 65, 65])
    idx = np.array([0, 1, 2, 3, 4, 5, -1, S, 8, 9, 9])
    slot = np.array([0, 0, 0, 0, 0, 0, 0, 0, _lib.E_LENGTH, 0, 0], np.int32)
    raw = RawState(S, C, dev)
    raw.add(z, labels, idx, slot)
    got = raw.finish(0)
    assert got["pred"][[0, 1, 2, 3, 4, 5]].tolist() == [3, 0, 5, 0, 9, 10]
    assert got["pred"][[6, 7, 8, 10, 11]].tolist() == [-1] * 5 and got["pred"][9] in (65, 64)
    assert got["row_loss"][2] == np.float32(2e4) and np.isfinite(got["row_loss"][[0, 1, 2]]).all()
    assert np.isnan(got["row_loss"][3]) and np.isnan(got["probs"][3]).all()
    assert got["status"][0] == 1 and got["row_loss"][4] == 0.0 and got["row_loss"][5] == 0.0
    assert abs(float(got["probs"][4].sum()) - 1.0) < 1e-5 and abs(float(got["probs"][5].sum()) - 1.0) < 1e-5      # still written
    assert got["seen"].tolist() == [1, 1, 1, 1, 0, 0, 0, 0, 0, 2, 0, 0]
    assert (got["row_loss"][[6, 7, 8, 10, 11]] == SENTINEL).all() and (got["probs"][[6, 7, 8, 10, 11]] == SENTINEL).all()
    conf = np.zeros((C, C), np.int32)
    for y, p in ((40, 3), (2, 0), (6, 5), (0, 0), (65, 65), (65, 64)):
        conf[y, p] += 1
    assert np.array_equal(got["confusion"], conf)
    totals = got["totals"].tolist()
    assert totals[0] == 6 and totals[1] == 5 and totals[0] - totals[1] == 1 and totals[5] == S - 5
    assert totals[2:5] == [1, 4, 5]             # correct: (65, 65); guessed: 3, 5, 65, 64; gold: 40, 2, 6, 65, 65
    assert got["metrics"][1:].tolist() == list(eval_ref.prf(1, 4, 5))
    # status is optional: the same rows without it
    quiet = RawState(S, C, dev)
    quiet.add(z, labels, idx, slot, with_status=False)
    got2 = quiet.finish(0)
    assert got2["status"][0] == 0 and np.array_equal(got2["confusion"], conf) and np.array_equal(got2["seen"], got["seen"])
    # against the restatement (the twice-scored sentence keeps either of its two rows: compare the others)
    want = eval_ref.eval_batch_ref(eval_ref.new_state(S, C), z, labels, idx, slot)
    keep = np.arange(S) != 9
    assert np.array_equal(got["pred"][keep], want["pred"][keep]) and np.array_equal(got["seen"], want["seen"])
    assert np.array_equal(got["confusion"], want["confusion"])


def test_several_adds_equal_one_and_reset_restores(dev):
    """EvalState: three add() calls and one finish() give exactly what one big add() gives; reset() brings back the initial state."""
    from gcn_over_pruned_trees_amd import evaluate
    M, C, S = 130, 42, 140
    rng = np.random.RandomState(8)
    logits = torch.as_tensor((rng.standard_normal((M, C)) * 2.0).astype(np.float32), device=dev)
    labels = torch.as_tensor(np.where(rng.random_sample(M) < 0.5, 0, rng.randint(0, C, size=M)), device=dev)
    idx = torch.as_tensor(rng.permutation(S)[:M], device=dev)
    one = evaluate.EvalState(S, C, dev, want_probs=True)
    one.add(logits, labels, idx)
    a = one.finish()
    parts = evaluate.EvalState(S, C, dev, want_probs=True)
    for lo, hi in ((0, 50), (50, 51), (51, M)):
        parts.add(logits[lo:hi], labels[lo:hi], idx[lo:hi])
    b = parts.finish()
    for name in ("pred", "probs", "row_loss", "confusion", "by_relation", "totals", "metrics", "status", "seen"):
        assert same_bits(getattr(a, name).cpu().numpy(), getattr(b, name).cpu().numpy()), name
    want = eval_ref.eval_batch_ref(eval_ref.new_state(S, C), logits.cpu().numpy(), labels.cpu().numpy(), idx.cpu().numpy())
    by, totals, metrics = eval_ref.eval_finish_ref(want["confusion"], want["seen"], want["row_loss"], 0)
    read = b.read(predictions=True)
    assert np.array_equal(read["pred"], want["pred"]) and np.array_equal(b.confusion.cpu().numpy(), want["confusion"])
    assert (read["precision"], read["recall"], read["f1"]) == tuple(metrics[1:].tolist())
    assert (read["n_scored"], read["n_sentences"], read["n_unseen"], read["bad_label"]) == (M, M, S - M, False)
    assert max_rel(read["loss"], metrics[0]) <= FWD_RTOL and "pred" not in b.read()
    parts.reset()
    torch.cuda.synchronize()
    assert (parts.pred == -1).all() and not parts.seen.any() and not parts.confusion.any() and not parts.status.any()
    parts.add(logits, labels, idx)
    c = parts.finish()
    for name in ("pred", "probs", "row_loss", "confusion", "by_relation", "totals", "metrics", "status"):
        assert same_bits(getattr(a, name).cpu().numpy(), getattr(c, name).cpu().numpy()), name
    # a label outside [0, C) is reported by read()
    parts.reset()
    bad = labels.clone()
    bad[3] = C
    parts.add(logits, bad, idx)
    r = parts.finish().read()
    assert r["bad_label"] and r["n_scored"] == M - 1 and r["n_unseen"] == S - M + 1
    with pytest.raises(TypeError, match="GPU only"):
        parts.add(logits.cpu(), labels, idx)


# ---- Evaluator end to end: S = 23 sentences of 3 .. 20 tokens, B = 5 (the last batch holds 3 sentences and two empty slots) ----
S_E2E, TS_E2E, B_E2E = 23, 20, 5


@functools.lru_cache(maxsize=None)
def e2e_host(C):
    """Shared between the tests: read only."""
    rng = np.random.RandomState(40 + C)
    lens = rng.randint(3, TS_E2E + 1, size=S_E2E).astype(np.int32)
    lens[[0, 1]] = (TS_E2E, 3)
    tb = synthetic.random_tree_batch(41, S_E2E, TS_E2E, lengths=lens)
    live = ~tb["masks"]
    h = dict(words=rng.randint(2, 500, size=(S_E2E, TS_E2E)) * live, pos=rng.randint(1, 47, size=(S_E2E, TS_E2E)) * live,
             ner=rng.randint(1, 15, size=(S_E2E, TS_E2E)) * live, deprel=tb["deprel"], head=tb["head"], subj_pos=tb["subj_pos"],
             obj_pos=tb["obj_pos"], lens=lens, labels=np.where(rng.random_sample(S_E2E) < 0.3, 0, rng.randint(0, C, size=S_E2E)).astype(np.int64))
    for a in h.values():
        a.setflags(write=False)
    return h


@functools.lru_cache(maxsize=None)
def e2e_dataset(with_ner):
    from gcn_over_pruned_trees_amd import dataset
    h = e2e_host(5 if with_ner else 10)
    ds = dataset.DeviceDataset.build(h["words"], h["pos"], h["ner"] if with_ner else None, h["deprel"], h["head"], h["subj_pos"], h["obj_pos"],
                                     h["lens"], h["labels"], cuda_dev())
    return ds, ds.tree_cache(1, want_label=False), h


def e2e_model(gcn, dev, with_ner=True, **kw):
    opt = dict(vocab_size=500, emb_dim=8, pos_dim=2, ner_dim=2 if with_ner else 0, hidden_dim=16, num_layers=2, input_dropout=0.5,
               gcn_dropout=0.5, emb_dropout=0.0, word_dropout=0.0, prune_k=1, pooling="max", pooling_l2=0.003, mlp_layers=2, rnn=False,
               dataset="tacred" if with_ner else "semeval", num_class=5 if with_ner else 10, topn=1e10, cuda=True, adj_type="regular",
               gcn_check_trees=False, gcn_native_head=True)
    opt.update(kw)
    torch.manual_seed(77)
    model = gcn.GCNClassifier(opt).to(dev)
    with torch.no_grad():                                             # freshly initialised weights give every sentence the same class: spread the logits
        for name, p in model.named_parameters():
            if p.dim() == 2 and "emb" not in name:
                p.mul_(4.0)
        model.classifier.bias.zero_()
    return model


def reference_loop(model, ds, cache, h, B):
    """trainer.predict per batch (trainer.py:116-120) + the unsort, on the host: (pred [S], loss [S] float64, sum of the batch means)."""
    S = len(h["lens"])
    pred, loss, means = np.full((S,), -1, np.int64), np.zeros((S,), np.float64), 0.0
    model.eval()
    with torch.no_grad():
        for idx in staging.length_buckets(h["lens"], B):
            batch = ds.batch(idx)
            logits, _ = model(batch.inputs, trees=cache.batch(batch.idx, batch.T))
            _, p = model.predict(logits)
            ce = F.cross_entropy(logits.double(), batch.labels, reduction="none")
            pred[idx], loss[idx] = p.cpu().numpy(), ce.cpu().numpy()
            means += float(F.cross_entropy(logits.double(), batch.labels))
    return pred, loss, means


@pytest.mark.parametrize("with_ner", [True, False], ids=["tacred", "semeval"])
def test_evaluator_end_to_end(api, dev, with_ner):
    from gcn_over_pruned_trees_amd import evaluate
    gcn, _ = api
    ds, cache, h = e2e_dataset(with_ner)
    C = 5 if with_ner else 10
    model = e2e_model(gcn, dev, with_ner).train()
    ev = evaluate.Evaluator(model, ds, B_E2E, cache=cache)
    assert len(ev.batches) == 5 and ev.idx.shape == (5, B_E2E) and ev.idx[-1].tolist()[3:] == [-1, -1] and len(ev.batches[-1]) == 3
    res = ev.run()
    assert model.training                                             # the training flag is restored ...
    r = res.read(predictions=True)
    model.eval()
    ev.run()
    assert not model.training                                         # ... whichever it was
    want_pred, want_loss, means = reference_loop(model, ds, cache, h, B_E2E)
    print("evaluator: predicted classes %s" % np.bincount(want_pred, minlength=C).tolist())
    assert np.array_equal(r["pred"], want_pred) and len(set(np.round(want_loss, 6).tolist())) > S_E2E // 2      # (the sentences differ ...
    assert len(set(want_pred.tolist())) > 1                                                                         # ... and so do the predictions)
    err = max_rel(res.row_loss.cpu().numpy(), want_loss)
    print("evaluator %s: row_loss max-rel error %.3e, loss %.9g" % ("tacred" if with_ner else "semeval", err, r["loss"]))
    assert err <= FWD_RTOL and max_rel(r["loss"], want_loss.mean()) <= FWD_RTOL
    conf, prf = eval_ref.score_ref(h["labels"], want_pred, C, 0)
    assert (r["precision"], r["recall"], r["f1"]) == prf and np.array_equal(res.confusion.cpu().numpy(), conf)
    assert (r["n_scored"], r["n_sentences"], r["n_unseen"], r["bad_label"]) == (S_E2E, S_E2E, 0, False)
    assert max_rel(res.dev_loss(B_E2E), means / S_E2E * B_E2E) <= FWD_RTOL
    assert (res.seen == 1).all() and res.probs is None
    # without a cache the model prunes each batch itself: the same predictions
    r2 = evaluate.Evaluator(model, ds, B_E2E, want_probs=True).run()
    assert np.array_equal(r2.pred.cpu().numpy(), want_pred) and abs(float(r2.probs.sum()) - S_E2E) < 1e-3


def _snapshot(res):
    return {k: getattr(res, k).clone() for k in ("pred", "confusion", "row_loss", "metrics", "by_relation", "totals")}


def test_graph_evaluator_equals_eager_and_follows_the_weights(api, dev):
    """graph=True, T_round=8 against graph=False, T_round=8: pred, confusion, row_loss and metrics bit-identical; a second run() replays
    only (the graph cache does not grow); after the weights change in place the next run() gives the eager result for the new weights."""
    from gcn_over_pruned_trees_amd import evaluate
    gcn, _ = api
    ds, cache, h = e2e_dataset(True)
    model = e2e_model(gcn, dev).eval()
    eager = evaluate.Evaluator(model, ds, B_E2E, cache=cache, graph=False, T_round=8)
    graphed = evaluate.Evaluator(model, ds, B_E2E, cache=cache, graph=True)
    assert graphed.T_round == 8 and graphed.widths == eager.widths and set(eager.widths) == {8, 16, 20}
    assert evaluate.Evaluator(model, ds, B_E2E, cache=cache).T_round == 1

    def compare(what):
        want = _snapshot(eager.run())
        got = _snapshot(graphed.run())
        torch.cuda.synchronize()
        for k in want:
            assert same_bits(got[k].cpu().numpy(), want[k].cpu().numpy()), (what, k)
        return want

    first = compare("first run (captures)")
    assert sorted(graphed.graphs) == [8, 16, 20]
    graphs = {T: id(g) for T, (g, _) in graphed.graphs.items()}
    compare("second run (replays)")
    assert {T: id(g) for T, (g, _) in graphed.graphs.items()} == graphs and len(graphed.graphs) == 3
    assert int(first["totals"][0]) == S_E2E and int(first["totals"][5]) == 0
    with torch.no_grad():
        for p in model.parameters():
            p.data.add_(torch.randn_like(p) * 0.3)
    third = compare("after the weights moved")
    assert {T: id(g) for T, (g, _) in graphed.graphs.items()} == graphs
    assert not same_bits(third["row_loss"].cpu().numpy(), first["row_loss"].cpu().numpy())


def test_graph_evaluator_refuses_a_checking_model(api, dev):
    from gcn_over_pruned_trees_amd import evaluate
    gcn, _ = api
    ds, cache, _ = e2e_dataset(True)
    model = e2e_model(gcn, dev, gcn_check_trees=True)
    with pytest.raises(ValueError, match="gcn_check_trees"):
        evaluate.Evaluator(model, ds, B_E2E, cache=cache, graph=True)
    assert evaluate.Evaluator(model, ds, B_E2E, cache=cache, graph=False).graphs == {}
