"""GPU tests of the native optimizer step (csrc/optim_kernels.hip gcnpt_optim_step, gcn_over_pruned_trees_amd.optim): clip_grad_norm_ +
SGD / MyAdagrad + zero_grad as one call over dense tensors and row-sparse tables.  Reference: tests/optim_ref.py, the float64 restatement
that tests/test_optim_capi.py pins to the reference's own recorded loop; the module tests run against that recording itself
(tests/golden/train_trajectory.npz).  Bounds: norm and coef 1e-6 relative, weights 2e-6 * max(max|want|, lr) -- an Adagrad step is at most lr
in size -- Adagrad sums 2e-6 relative (the bounds of test_sgd_clip_update_kernel_matches_clip_grad_norm, widened by lr); a row that k tokens
share adds k * 2^-24 * sum|rows| for the order of its fp32 sum.
Argument-block capacity of one launch: 64 dense tensors and 8 tables (_lib.OPTIM_TENSORS_PER_LAUNCH / OPTIM_TABLES_PER_LAUNCH); the dense
case below passes 80 tensors and the many-tables case 9 tables, so both take a second launch per phase."""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

import optim_ref
from conftest import GOLDEN, load_golden
from helpers import cuda_dev, gcn_api, to_dev
from gcn_over_pruned_trees_amd import _lib
from gcn_over_pruned_trees_amd.utils import synthetic

pytestmark = pytest.mark.gpu

POISON = -7.25e4                     # never produced by the cases below
KINDS = {"sgd": _lib.OPTIM_SGD, "adagrad": _lib.OPTIM_ADAGRAD}
LR = 0.5


@pytest.fixture(scope="module")
def dev():
    return cuda_dev()


@pytest.fixture(scope="module")
def api():
    return gcn_api()


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and bool((a.contiguous().view(torch.int32) == b.contiguous().view(torch.int32)).all())


def _capi_step(kind, dense, tables, lr, max_norm, dev, lr_dev=None, clear=1):
    """gcnpt_optim_step on device tensors.  dense: [(w, g, state or None)], tables: [(w, state or None, ids, rows, owner, scratch)].
    Returns (norm, coef) as the call left them."""
    L, P = _lib.lib(), (lambda t: None if t is None else t.data_ptr())
    partials = torch.full((int(L.gcnpt_optim_partials_floats(len(dense), len(tables))),), POISON, dtype=torch.float32, device=dev)
    ct = (_lib.OptimTensor * max(len(dense), 1))(*[(P(w), P(g), P(st), w.numel()) for w, g, st in dense])
    cb = (_lib.OptimTable * max(len(tables), 1))(*[(P(w), P(st), P(ids), P(rows), P(owner), P(scr), w.shape[0], w.shape[1], ids.shape[0], 0)
                                                   for w, st, ids, rows, owner, scr in tables])
    _lib.check(L.gcnpt_optim_step(_lib.stream(), kind, ct, len(dense), cb, len(tables), max_norm, lr, P(lr_dev), clear, P(partials)))
    torch.cuda.synchronize()
    return float(partials[_lib.OPTIM_NORM]), float(partials[_lib.OPTIM_COEF])


def _check_weights(got, want, lr, extra=0.0, what=""):
    want = want.double()
    err = (got.double().cpu() - want).abs()
    tol = 2e-6 * max(float(want.abs().max()), lr) + extra
    assert bool((err <= tol).all()), (what, float(err.max()), float(torch.as_tensor(tol).max()))


def _check_sums(got, want, extra=0.0, what=""):
    err = (got.double().cpu() - want.double()).abs()
    tol = 2e-6 * float(want.abs().max()) + extra
    assert bool((err <= tol).all()), (what, float(err.max()))


# ---- dense tensors ------------------------------------------------------------------------------------------------------------------
DENSE_LENGTHS = [1, 3, 4, 5, 255, 256, 257, 1027]
MISALIGNED = [5, 1030]               # views that start one float past a 16-byte boundary: the scalar path
N_SINGLE = 70                        # one-element tensors: 80 tensors in all, more than one 64-tensor argument block


def _carve(lengths, shifts, fill, dev):
    """Tensors of the given lengths as views of one pool, each starting `shift` floats past a 16-byte boundary, with poisoned gaps of
    at least 4 floats around them.  fill(i, n) -> numpy float32 [n].  Returns (pool, [views], gap mask)."""
    offs, at = [], 4
    for n, sh in zip(lengths, shifts):
        offs.append(at + sh)
        at = (at + sh + n + 4 + 3) // 4 * 4
    host = np.full(at + 4, POISON, np.float32)
    gap = np.ones(at + 4, bool)
    for i, (o, n) in enumerate(zip(offs, lengths)):
        host[o:o + n] = fill(i, n)
        gap[o:o + n] = False
    pool = to_dev(host, dev)
    views = [pool[o:o + n] for o, n in zip(offs, lengths)]
    assert all(v.data_ptr() % 16 == 4 * sh for v, sh in zip(views, shifts))
    return pool, views, torch.from_numpy(gap)


@pytest.mark.parametrize("clip", ["bites", "loose", "off"])
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_dense_tensors_match_the_restatement(dev, kind, clip):
    lengths = DENSE_LENGTHS + MISALIGNED + [1] * N_SINGLE
    shifts = [0] * len(DENSE_LENGTHS) + [1] * len(MISALIGNED) + [0] * N_SINGLE
    assert len(lengths) > _lib.OPTIM_TENSORS_PER_LAUNCH
    wp, ws, wgap = _carve(lengths, shifts, lambda i, n: synthetic.normal(500 + i, (n,)), dev)
    gp, gs, ggap = _carve(lengths, shifts, lambda i, n: 0.05 * synthetic.normal(700 + i, (n,)), dev)
    sp, ss, sgap = _carve(lengths, shifts, lambda i, n: 0.1 + np.abs(synthetic.normal(900 + i, (n,))), dev)
    ada = kind == "adagrad"
    dense = [(w, g, s if ada else None) for w, g, s in zip(ws, gs, ss)]
    before = [(w.cpu().clone(), g.cpu().clone(), s.cpu().clone() if ada else None) for w, g, s in dense]
    true_norm = optim_ref.grad_norm([g for _, g, _ in before])
    max_norm = {"bites": 0.5 * true_norm, "loose": 2.0 * true_norm, "off": 0.0}[clip]
    want = optim_ref.step(KINDS[kind], before, [], LR, max_norm)
    assert (want["coef"] < 1.0) == (clip == "bites")
    s0 = sp.cpu().clone()
    norm, coef = _capi_step(KINDS[kind], dense, [], LR, max_norm, dev)
    assert abs(norm - want["norm"]) <= 1e-6 * want["norm"] and abs(coef - want["coef"]) <= 1e-6 * want["coef"]
    for i, ((w, g, s), (w_want, s_want)) in enumerate(zip(dense, want["dense"])):
        _check_weights(w, w_want, LR, what="w%d" % i)
        if ada:
            _check_sums(s, s_want, what="sum%d" % i)
        assert float(g.abs().max()) == 0.0, i                      # zero_grad rode on the update
    for pool, gap in ((wp, wgap), (gp, ggap), (sp, sgap)):
        assert bool((pool.cpu()[gap] == POISON).all())             # nothing written between the tensors
    if not ada:
        assert torch.equal(sp.cpu(), s0)                           # SGD never touches a state buffer


def test_dense_clear_grads_off_keeps_the_gradients(dev):
    w, g = to_dev(synthetic.normal(1, (300,)), dev), to_dev(synthetic.normal(2, (300,)), dev)
    g0 = g.clone()
    _capi_step(_lib.OPTIM_SGD, [(w, g, None)], [], LR, 0.0, dev, clear=0)
    assert torch.equal(g, g0)


# ---- row-sparse tables --------------------------------------------------------------------------------------------------------------
V, TOPN = 97, 60


def _table_ids(n_rows, seed):
    """(ids, fold): one id once, one twice, one `fold` times (130 of 200 rows), ids -1 and V (ignored), ids >= TOPN (their rows are zero),
    and otherwise random ids below TOPN."""
    rng = np.random.RandomState(seed)
    if n_rows == 1:
        return np.array([7], np.int64), 1
    fold = 130 if n_rows >= 200 else n_rows // 2
    ids = [5, 9, 9, -1, V, 70, 96, 70] + [11] * fold
    ids += list(rng.choice(np.setdiff1d(np.arange(12, TOPN), [5, 9, 11]), size=n_rows - len(ids)))
    ids = np.array(ids, np.int64)
    rng.shuffle(ids)
    assert len(ids) == n_rows and (ids == 5).sum() == 1 and (ids == 9).sum() == 2 and (ids == 11).sum() == fold
    return ids, fold


def _table_case(E, n_rows, seed, dev, ada, ids=None):
    """One table with a guard row before and after w / state (a write through id -1 or V would land there)."""
    fold = None
    if ids is None:
        ids, fold = _table_ids(n_rows, seed)
    rows = 0.01 * synthetic.normal(seed + 1, (n_rows, E))
    rows[ids >= TOPN] = 0.0                                         # what the embedding backward leaves under topn
    w_full = np.full((V + 2, E), POISON, np.float32)
    w_full[1:V + 1] = synthetic.normal(seed + 2, (V, E))
    s_full = np.full((V + 2, E), POISON, np.float32)
    s_full[1:V + 1] = 0.5 + np.abs(synthetic.normal(seed + 3, (V, E))).clip(0, 1)        # sums in [0.5, 1.5]
    w_full, s_full = to_dev(w_full, dev), to_dev(s_full, dev)
    t = dict(w_full=w_full, s_full=s_full, w=w_full[1:V + 1], state=s_full[1:V + 1] if ada else None, ids=to_dev(ids, dev),
             rows=to_dev(rows, dev), owner=torch.full((V,), -1, dtype=torch.int32, device=dev),
             scratch=torch.full((n_rows,), 12345, dtype=torch.int32, device=dev), fold=fold, ids_host=ids, rows_host=rows)
    return t


def _arg(t):
    return (t["w"], t["state"], t["ids"], t["rows"], t["owner"], t["scratch"])


@pytest.mark.parametrize("kind", sorted(KINDS))
@pytest.mark.parametrize("n_rows", [1, 63, 64, 65, 200])
@pytest.mark.parametrize("E", [300, 50, 7])
def test_tables_match_the_restatement(dev, E, n_rows, kind):
    ada = kind == "adagrad"
    t = _table_case(E, n_rows, 40 + E + n_rows, dev, ada)
    dw, dg = to_dev(synthetic.normal(3, (37,)), dev), to_dev(0.02 * synthetic.normal(4, (37,)), dev)
    ds = to_dev(0.5 + np.abs(synthetic.normal(5, (37,))), dev) if ada else None
    w0, s0 = t["w_full"].cpu().clone(), t["s_full"].cpu().clone()
    before_dense = [(dw.cpu().clone(), dg.cpu().clone(), ds.cpu().clone() if ada else None)]
    before_tables = [(w0[1:V + 1], s0[1:V + 1] if ada else None, torch.from_numpy(t["ids_host"]), torch.from_numpy(t["rows_host"]))]
    G = optim_ref.coalesce(t["ids_host"], t["rows_host"], V)
    true_norm = optim_ref.grad_norm([before_dense[0][1], G])
    max_norm = 0.5 * true_norm if (E + n_rows) % 2 else 2.0 * true_norm          # (a clip that bites in half of the cases)
    want = optim_ref.step(KINDS[kind], before_dense, before_tables, LR, max_norm)
    norm, coef = _capi_step(KINDS[kind], [(dw, dg, ds)], [_arg(t)], LR, max_norm, dev)
    assert abs(norm - want["norm"]) <= 1e-6 * want["norm"] and abs(coef - want["coef"]) <= 1e-6 * want["coef"]
    # per element: the order of a k-fold fp32 sum
    ids_h, absrows = torch.from_numpy(t["ids_host"]), torch.from_numpy(np.abs(t["rows_host"])).double()
    ok = (ids_h >= 0) & (ids_h < V)
    count = torch.zeros(V, dtype=torch.float64).index_add_(0, ids_h[ok], torch.ones(int(ok.sum()), dtype=torch.float64))
    extra = count[:, None] * 2.0 ** -24 * torch.zeros(V, E, dtype=torch.float64).index_add_(0, ids_h[ok], absrows[ok])
    extra[count <= 2] = 0.0                                         # one- and two-term sums do not depend on order
    w_want, s_want = want["tables"][0]
    _check_weights(t["w"], w_want, LR, extra=extra, what="table w")
    _check_weights(dw, want["dense"][0][0], LR, what="dense w")
    if ada:
        _check_sums(t["state"], s_want, extra=extra, what="table sums")
        _check_sums(ds, want["dense"][0][1], what="dense sums")
    assert float(dg.abs().max()) == 0.0
    # rows no id names, and rows whose gradient is zero, keep their bits; so do the guard rows and (SGD) the whole state
    w1, s1 = t["w_full"].cpu(), t["s_full"].cpu()
    untouched = torch.ones(V + 2, dtype=torch.bool)
    named = np.unique(t["ids_host"][(t["ids_host"] >= 0) & (t["ids_host"] < TOPN)])
    untouched[torch.from_numpy(named) + 1] = False
    assert int(untouched.sum()) >= V + 2 - TOPN and _same_bits(w1[untouched], w0[untouched]) and _same_bits(s1[untouched], s0[untouched])
    if not ada:
        assert _same_bits(s1, s0)
    moved = (w1[~untouched] != w0[~untouched]).any(1)
    assert bool(moved.all())                                        # every named row did move
    assert bool((t["owner"] == -1).all())                          # the workspace convention


def test_second_step_on_the_same_workspace(dev):
    """A second step with other ids on the workspace the first one used gives the bits a fresh workspace gives (no id more than twice)."""
    E, n_rows = 50, 65
    for kind in sorted(KINDS):
        ada = kind == "adagrad"
        t = _table_case(E, n_rows, 300, dev, ada)
        _capi_step(KINDS[kind], [], [_arg(t)], LR, 0.3, dev)
        rng = np.random.RandomState(9)
        ids2 = np.concatenate([rng.permutation(40)[:33], rng.permutation(40)[:32] + 30]).astype(np.int64)
        assert np.bincount(ids2).max() <= 2 and len(ids2) == n_rows
        rows2 = 0.01 * synthetic.normal(310, (n_rows, E))
        fresh = dict(t, w_full=t["w_full"].clone(), s_full=t["s_full"].clone(), owner=torch.full((V,), -1, dtype=torch.int32, device=dev),
                     scratch=torch.zeros(n_rows, dtype=torch.int32, device=dev))
        fresh["w"], fresh["state"] = fresh["w_full"][1:V + 1], fresh["s_full"][1:V + 1] if ada else None
        out = []
        for case in (t, fresh):
            case["ids"], case["rows"] = to_dev(ids2, dev), to_dev(rows2, dev)
            out.append(_capi_step(KINDS[kind], [], [_arg(case)], LR, 0.3, dev))
        assert out[0] == out[1]
        assert _same_bits(t["w_full"], fresh["w_full"]) and _same_bits(t["s_full"], fresh["s_full"])
        assert bool((t["owner"] == -1).all()) and bool((fresh["owner"] == -1).all())


def test_more_tables_than_one_argument_block(dev):
    n = _lib.OPTIM_TABLES_PER_LAUNCH + 1
    cases = [_table_case(7, 20 + i, 400 + 10 * i, dev, True, ids=np.random.RandomState(i).randint(0, TOPN, size=20 + i).astype(np.int64))
             for i in range(n)]
    before = [(t["w"].cpu().clone(), t["state"].cpu().clone(), torch.from_numpy(t["ids_host"]), torch.from_numpy(t["rows_host"])) for t in cases]
    want = optim_ref.step(optim_ref.ADAGRAD, [], before, LR, 0.05)
    assert want["coef"] < 1.0
    norm, coef = _capi_step(_lib.OPTIM_ADAGRAD, [], [_arg(t) for t in cases], LR, 0.05, dev)
    assert abs(norm - want["norm"]) <= 1e-6 * want["norm"] and abs(coef - want["coef"]) <= 1e-6 * want["coef"]
    for i, (t, (w_want, s_want)) in enumerate(zip(cases, want["tables"])):
        extra = 20 * 2.0 ** -24 * float(np.abs(t["rows_host"]).sum(0).max())
        _check_weights(t["w"], w_want, LR, extra=extra, what="table %d" % i)
        _check_sums(t["state"], s_want, extra=extra, what="sums %d" % i)
        assert bool((t["owner"] == -1).all())


def test_deterministic_merge_is_defined_bit_for_bit(dev):
    """GCNPT_OPT_DETERMINISTIC: the 130-fold id gives the same bits on two runs, and they are the bits of fp32 adds in ascending token
    position starting from the owner's row (max_norm = 0: coef is exactly 1, so w' = w - lr * G in fp32)."""
    E, n_rows = 300, 200
    old = _lib.set_option(_lib.OPT_DETERMINISTIC, 1)
    try:
        runs = []
        for _ in range(2):
            t = _table_case(E, n_rows, 77, dev, False)
            _capi_step(_lib.OPTIM_SGD, [], [_arg(t)], LR, 0.0, dev)
            runs.append((t["w_full"].cpu(), t["rows"].cpu()))
    finally:
        _lib.set_option(_lib.OPT_DETERMINISTIC, old)
    assert _same_bits(runs[0][0], runs[1][0]) and _same_bits(runs[0][1], runs[1][1])
    ids, rows = t["ids_host"], torch.from_numpy(t["rows_host"])
    w0 = torch.from_numpy(synthetic.normal(77 + 2, (V, E)))
    for i in (11, 9, 5):
        at = np.flatnonzero(ids == i)
        G = rows[at[0]].clone()
        for p in at[1:]:
            G = G + rows[p]                                        # fp32, ascending token position
        assert _same_bits(runs[0][1][at[0]], G), i                 # the owner's row of `rows` holds the merged gradient
        assert _same_bits(runs[0][0][1 + i], w0[i] - torch.tensor(LR) * G), i


# ---- through optim.py ---------------------------------------------------------------------------------------------------------------
def _params(dev, shapes, seed):
    return [torch.nn.Parameter(to_dev(synthetic.normal(seed + i, s), dev)) for i, s in enumerate(shapes)]


@pytest.mark.parametrize("name", ["sgd", "adagrad", "myadagrad"])
def test_optimizer_object_dense_sparse_and_skipped(dev, name):
    from gcn_over_pruned_trees_amd import optim
    kind = optim_ref.SGD if name == "sgd" else optim_ref.ADAGRAD
    ps = _params(dev, [(V, 50), (33, 7), (5,), (12, 3), (4, 6)], 800)
    ids, _ = _table_ids(65, 3)
    ids = ids.clip(0, V - 1)                                          # (sparse_coo_tensor itself wants indices inside the table)
    rows = 0.01 * synthetic.normal(801, (65, 50))
    ps[0].grad = torch.sparse_coo_tensor(to_dev(ids, dev).unsqueeze(0), to_dev(rows, dev), size=(V, 50))
    ps[1].grad = to_dev(0.02 * synthetic.normal(802, (33, 7)), dev)
    ps[2].grad = to_dev(0.02 * synthetic.normal(803, (5,)), dev)
    ps[3].grad = None                                                 # skipped, as torch does
    ps[4].grad = to_dev(0.02 * synthetic.normal(804, (6, 4)), dev).t()      # not contiguous: copied once
    assert not ps[4].grad.is_contiguous()
    opt = optim.get_optimizer(name, ps, LR, 0.05)
    sums0 = [s.cpu().clone() for s in opt.state] if kind else [None] * 5
    assert not kind or all(float(s.min()) == float(s.max()) == np.float32(0.1) for s in sums0)       # MyAdagrad's init_accu_value
    w0 = [p.data.cpu().clone() for p in ps]
    want = optim_ref.step(kind, [(w0[i], ps[i].grad.cpu(), sums0[i]) for i in (1, 2, 4)],
                          [(w0[0], sums0[0], torch.from_numpy(ids), torch.from_numpy(rows))], LR, 0.05)
    assert want["coef"] < 1.0
    dense_grads = [ps[i].grad for i in (1, 2, 4)]
    assert opt.step() is None
    torch.cuda.synchronize()
    assert abs(float(opt.last_norm) - want["norm"]) <= 1e-6 * want["norm"] and abs(float(opt.last_coef) - want["coef"]) <= 1e-6 * want["coef"]
    extra = 33 * 2.0 ** -24 * float(np.abs(rows).sum(0).max())
    _check_weights(ps[0].data, want["tables"][0][0], LR, extra=extra)
    for j, i in enumerate((1, 2, 4)):
        _check_weights(ps[i].data, want["dense"][j][0], LR, what=i)
        if kind:
            _check_sums(opt.state[i], want["dense"][j][1], what=i)
        assert ps[i].grad is dense_grads[j] and float(ps[i].grad.abs().max()) == 0.0          # cleared in place
    assert ps[0].grad is None                                         # a sparse gradient is dropped
    assert _same_bits(ps[3].data.cpu(), w0[3]) and ps[3].grad is None
    if kind:
        assert _same_bits(opt.state[3].cpu(), sums0[3])
        sd = opt.state_dict()
        other = optim.get_optimizer(name, ps, 0.1, 1.0)
        other.load_state_dict(sd)
        assert all(torch.equal(a, b) for a, b in zip(other.state, opt.state)) and other.param_groups[0]["lr"] == LR
    # a step without any gradient moves nothing
    opt.zero_grad(set_to_none=True)
    w1 = [p.data.clone() for p in ps]
    opt.step()
    torch.cuda.synchronize()
    assert all(_same_bits(a, p.data) for a, p in zip(w1, ps)) and float(opt.last_norm) == 0.0 and float(opt.last_coef) == 1.0


def test_lr_dev_is_read_by_a_captured_step(dev):
    """One captured step(), replayed under two learning rates: the update follows the device scalar (the reference's lr decay)."""
    from gcn_over_pruned_trees_amd import optim
    (p,) = _params(dev, [(40, 9)], 820)
    g0 = to_dev(synthetic.normal(821, (40, 9)), dev)
    p.grad = g0.clone()
    opt = optim.get_optimizer("sgd", [p], 0.5, 0.0)
    w0 = p.data.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        opt.step()                                                    # warm-up, eager
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert _same_bits(p.data, w0 - 0.5 * g0)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        opt.step()                                                    # no host sync: it captures at all
    p.data.copy_(w0)
    p.grad.copy_(g0)
    graph.replay()
    torch.cuda.synchronize()
    assert _same_bits(p.data, w0 - 0.5 * g0) and float(p.grad.abs().max()) == 0.0
    w1 = p.data.clone()
    p.grad.copy_(g0)
    opt.param_groups[0]["lr"] = 0.125                                  # torch_utils.change_lr
    opt.sync_lr()
    graph.replay()
    torch.cuda.synchronize()
    assert _same_bits(p.data, w1 - 0.125 * g0) and not _same_bits(p.data, w1 - 0.5 * g0)


def test_moved_buffers_are_followed(dev):
    """p.data re-homed after the optimizer was built (clone, then .to(dev) again): the next step() moves the live weights."""
    from gcn_over_pruned_trees_amd import optim
    model = torch.nn.Sequential(torch.nn.Linear(6, 5), torch.nn.Linear(5, 3)).to(dev)
    opt = optim.get_optimizer("sgd", list(model.parameters()), 0.5, 0.0)
    p = model[0].weight
    old = p.data
    p.data = p.data.clone()
    model = model.to(dev)
    assert p.data.data_ptr() != old.data_ptr()
    old_bits = old.clone()
    for q in model.parameters():
        q.grad = torch.ones_like(q)
    w0 = [q.data.clone() for q in model.parameters()]
    opt.step()
    torch.cuda.synchronize()
    assert all(_same_bits(q.data, a - 0.5) for q, a in zip(model.parameters(), w0))
    assert _same_bits(old, old_bits)                                   # the abandoned buffer was not written


# ---- the module against the reference's recorded loop ---------------------------------------------------------------------------------
def _traj():
    spec = importlib.util.spec_from_file_location("make_golden_trajectory", os.path.join(GOLDEN, "make_golden_trajectory.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)                                       # (imports nothing but this repository until its main() runs)
    return mod


def _traj_setup(g, dev):
    """The three batches and the initial state dict, regenerated from the fixture's seeds and checked against its checksums."""
    mk = _traj()
    assert int(g["seed"]) == mk.SEED
    batches = []
    for j in range(mk.N_BATCHES):
        inp, labels = mk.inputs(j)
        assert int(inp[0].sum()) == int(g["words_sum:%d" % j]) and int(inp[5].sum()) == int(g["head_sum:%d" % j])
        assert int(labels.sum()) == int(g["labels_sum:%d" % j])
        batches.append((tuple(to_dev(a, dev) for a in inp), to_dev(labels, dev)))
    sd = mk.params(json.loads(str(g["shapes"])))
    for k, v in sd.items():
        assert abs(float(v.astype(np.float64).sum()) - float(g["sum:" + k])) < 1e-6, k
    return batches, sd


def _traj_model(gcn, g, case, sd, dev, **kw):
    opt = dict(json.loads(str(g[case + ":opt"])), cuda=True, gcn_dtype="fp32", gcn_native_embed=True, gcn_native_head=True, **kw)
    m = gcn.GCNClassifier(opt)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()}, strict=True)
    return m.to(dev).train(), opt


def _dense_adagrad_step(params, sums, lr):
    """MyAdagrad's dense branch (utils/torch_utils.py:86-88), restated on the device in fp32."""
    for p in params:
        if p.grad is not None:
            s = sums.setdefault(p, torch.full_like(p.data, 0.1))
            s.addcmul_(p.grad, p.grad)
            p.data.addcdiv_(p.grad, s.sqrt().add_(1e-10), value=-lr)


def _run_trajectory(model, o, batches, steps, native):
    from gcn_over_pruned_trees_amd import optim
    params = [p for p in model.parameters() if p.requires_grad]
    losses, norms, coefs, sums = [], [], [], {}
    if native:
        opt = optim.get_optimizer(o["optim"], params, o["lr"], o["max_grad_norm"])
    elif o["optim"] == "sgd":
        opt = torch.optim.SGD(params, lr=o["lr"])
    for s in range(steps):
        inputs, labels = batches[s % len(batches)]
        logits, pooled = model(inputs)
        loss = model.loss(logits, pooled, labels)
        loss.backward()
        losses.append(loss.detach().clone())
        if native:
            opt.step()
            norms.append(opt.last_norm.clone())
            coefs.append(opt.last_coef.clone())
        else:
            norms.append(torch.nn.utils.clip_grad_norm_(model.parameters(), o["max_grad_norm"]).clone())
            if o["optim"] == "sgd":
                opt.step()
            else:
                _dense_adagrad_step(params, sums, o["lr"])
            model.zero_grad(set_to_none=False)
    torch.cuda.synchronize()
    final = {k: v.detach().cpu().numpy() for k, v in model.state_dict().items()}
    return (np.array([float(x) for x in losses]), np.array([float(x) for x in norms]), np.array([float(x) for x in coefs]), final)


def _dev(a, ref):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(ref, np.float64)).max())


@pytest.mark.parametrize("case", ["sgd", "sgd_clip", "adagrad"])
def test_trajectory_matches_the_reference_recording(api, dev, case):
    """Six steps of the reference's own loop (train.py:220-227 on GCNTrainer, recorded by tests/golden/make_golden_trajectory.py) with the
    native optimizer on the row-sparse word gradient, next to the same six steps on the existing torch path (dense gradients,
    clip_grad_norm_, torch.optim.SGD / a dense restated Adagrad), whose deviation from the recording is d_torch.  Losses, pre-clip norms
    and every final parameter: deviation <= max(4 * d_torch, 1e-6 * max|ref|) and never above 1e-4 * max|ref|."""
    gcn, _ = api
    g = load_golden("train_trajectory.npz")
    batches, sd = _traj_setup(g, dev)
    steps = int(g["steps"])
    model_n, o = _traj_model(gcn, g, case, sd, dev, gcn_sparse_emb_grad=True)
    model_t, _ = _traj_model(gcn, g, case, sd, dev, gcn_sparse_emb_grad=False)
    init = {k: v.detach().cpu().numpy().copy() for k, v in model_n.state_dict().items()}      # (the word table is in the state dict twice)
    l_n, n_n, coefs, f_n = _run_trajectory(model_n, o, batches, steps, native=True)
    l_t, n_t, _, f_t = _run_trajectory(model_t, o, batches, steps, native=False)
    checks = [("losses", l_n, l_t, g[case + ":losses"]), ("norms", n_n, n_t, g[case + ":norms"])]
    checks += [(k, f_n[k], f_t[k], g["%s:final:%s" % (case, k)]) for k in sorted(f_n)]
    bad = []
    for name, got, torch_path, ref in checks:
        scale = float(np.abs(ref).max())
        d_native, d_torch = _dev(got, ref), _dev(torch_path, ref)
        print("trajectory %-8s %-32s native %.3e  torch %.3e  max|ref| %.3e" % (case, name, d_native, d_torch, scale))
        if not (d_native <= max(4 * d_torch, 1e-6 * scale) and d_native <= 1e-4 * scale):
            bad.append((name, d_native, d_torch, scale))
    assert not bad, bad
    bites = json.loads(str(g["cases"]))[case]["max_grad_norm"] < g[case + ":norms"]
    assert bites.all() or not bites.any()
    assert ((coefs < 1.0) == bites).all() and (bites.all() or (coefs == 1.0).all())
    moved = [k for k in f_n if _dev(f_n[k], init[k]) > 0]
    assert "gcn_model.emb.weight" in moved and len(moved) >= 10
    if case == "sgd_clip":                                             # topn = 20: the other word rows are not fine-tuned
        assert np.array_equal(f_n["gcn_model.emb.weight"][20:], init["gcn_model.emb.weight"][20:])
        assert not np.array_equal(f_n["gcn_model.emb.weight"][2:20], init["gcn_model.emb.weight"][2:20])


def test_whole_training_step_captures_with_the_optimizer(api, dev):
    """Forward, loss, backward and optimizer.step() of the small model as ONE hipGraph (gcn_check_trees off, graph-safe RNG): three
    replays against three eager steps from the same start.  Bound as the trajectory's, with the deviation d of a SECOND eager run from
    the first in d_torch's place (what float-atomic order alone moves): <= max(4 * d, 1e-6 * max|ref|), never above 1e-4 * max|ref|."""
    from gcn_over_pruned_trees_amd import optim
    gcn, _ = api
    g = load_golden("train_trajectory.npz")
    batches, sd = _traj_setup(g, dev)
    inputs, labels = batches[0]
    model, o = _traj_model(gcn, g, "adagrad", sd, dev, gcn_sparse_emb_grad=True, gcn_check_trees=False, gcn_graph_rng=True)
    params = [p for p in model.parameters() if p.requires_grad]
    opt = optim.get_optimizer("adagrad", params, o["lr"], 0.5)         # (0.5: the clip bites too)
    start = [p.data.clone() for p in params]
    state0 = opt.state_dict()

    def step():
        logits, pooled = model(inputs)
        loss = model.loss(logits, pooled, labels)
        loss.backward()
        opt.step()
        return loss.detach()

    def restart():
        for p, a in zip(params, start):
            p.data.copy_(a)
        opt.load_state_dict(state0)
        opt.zero_grad()

    def eager():
        restart()
        losses = [step().clone() for _ in range(3)]
        torch.cuda.synchronize()
        return [float(x) for x in losses], [p.data.cpu().numpy().copy() for p in params]

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                                        # warm-up: dense gradients exist (zeroed) from here on
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        loss = step()
    restart()
    got_losses = []
    for _ in range(3):
        graph.replay()
        got_losses.append(loss.clone())
    torch.cuda.synchronize()
    got_losses, got = [float(x) for x in got_losses], [p.data.cpu().numpy().copy() for p in params]
    l1, w1 = eager()
    l2, w2 = eager()
    assert float(opt.last_coef) < 1.0
    assert any(_dev(a, b.cpu().numpy()) > 1e-3 for a, b in zip(w1, start))          # (three steps moved the weights)
    for name, a, ref, again in [("losses", got_losses, l1, l2)] + [("param %d" % i, a, b, c) for i, (a, b, c) in enumerate(zip(got, w1, w2))]:
        scale, d_graph, d_eager = float(np.abs(ref).max()), _dev(a, ref), _dev(again, ref)
        print("capture %-10s graph %.3e  eager again %.3e  max|ref| %.3e" % (name, d_graph, d_eager, scale))
        assert d_graph <= max(4 * d_eager, 1e-6 * scale) and d_graph <= 1e-4 * scale, name
