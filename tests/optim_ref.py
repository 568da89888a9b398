"""float64 restatement of the reference's update (train.py:225-227): torch.nn.utils.clip_grad_norm_, then torch.optim.SGD or MyAdagrad
(utils/torch_utils.py:10-90 with lr_decay = 0, weight_decay = 0), on lists of dense tensors and of row-sparse (ids, rows) tables.
tests/test_optim_capi.py pins it to quadruples recorded from the reference's own loop (tests/golden/train_trajectory.npz); the GPU tests
compare the kernels with it."""
import torch

SGD, ADAGRAD = 0, 1


def _f64(t):
    return torch.as_tensor(t).detach().to("cpu", torch.float64)


def coalesce(ids, rows, V):
    """[V,E] float64: rows summed per id; ids outside [0, V) contribute nothing."""
    ids, rows = torch.as_tensor(ids).detach().cpu().long(), _f64(rows)
    ok = (ids >= 0) & (ids < V)
    return torch.zeros(V, rows.shape[1], dtype=torch.float64).index_add_(0, ids[ok], rows[ok])


def grad_norm(grads):
    """clip_grad_norm_'s total norm of a list of (dense or coalesced) gradients."""
    return float(torch.sqrt(sum((_f64(g) ** 2).sum() for g in grads))) if grads else 0.0


def clip_coef(norm, max_norm):
    return min(1.0, max_norm / (norm + 1e-6)) if max_norm > 0 else 1.0


def update(kind, w, g, state, lr, coef):
    """One tensor: (w', state') in float64 (state' None for SGD)."""
    w, gh = _f64(w), _f64(g) * coef
    if kind == SGD:
        return w - lr * gh, None
    state = _f64(state) + gh * gh
    return w - lr * gh / (state.sqrt() + 1e-10), state


def step(kind, dense, tables, lr, max_norm):
    """dense: [(w, g, state or None)], tables: [(w [V,E], state or None, ids [n], rows [n,E])].
    Returns dict(norm, coef, dense=[(w', state')], tables=[(w', state')], G=[coalesced gradients])."""
    G = [coalesce(ids, rows, w.shape[0]) for w, _, ids, rows in tables]
    norm = grad_norm([g for _, g, _ in dense] + G)
    coef = clip_coef(norm, max_norm)
    return dict(norm=norm, coef=coef, G=G,
                dense=[update(kind, w, g, st, lr, coef) for w, g, st in dense],
                tables=[update(kind, w, Gi, st, lr, coef) for (w, st, _, _), Gi in zip(tables, G)])
