"""Shared by the CPU and GPU test modules: rebuild fixture inputs, tolerances, device helpers, the row tile's LDS count."""
import contextlib
import functools

import numpy as np

from conftest import dense_from_coo, load_golden
from gcn_over_pruned_trees_amd.utils import synthetic

# fp32 tolerances stated by SURVEY.md 8c: fwd max-abs <= 1e-5 * max|h|, grads rel <= 1e-4
FWD_RTOL = 1e-5
GRAD_RTOL = 1e-4


def max_rel(a, b):
    """max |a-b| / max |b|  (normwise, the form SURVEY.md 8c states its tolerances in)."""
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def fro_rel(a, b):
    """||a-b||_F / ||b||_F."""
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return float(np.sqrt(((a - b) ** 2).sum()) / max(np.sqrt((b ** 2).sum()), 1e-30))


def layer_case(name):
    """Load a layers_*.npz fixture; regenerate seed-defined inputs and verify their checksums."""
    g = load_golden(name)
    B, T, din, hidden, layers, seed = (int(g[k]) for k in ("B", "T", "din", "hidden", "layers", "seed"))
    if "x" in g:
        x, gy = g["x"], g["gy"]
        Ws = [g["W%d" % l] for l in range(layers)]
        bs = [g["b%d" % l] for l in range(layers)]
    else:
        Ws, bs = synthetic.layer_params(seed + 1, [din] + [hidden] * layers)
        x = synthetic.normal(seed + 2, (B, T, din))
        gy = synthetic.normal(seed + 3, (B, T, hidden))
    assert abs(float(x.astype(np.float64).sum()) - float(g["x_sum"])) < 1e-6
    assert abs(float(gy.astype(np.float64).sum()) - float(g["gy_sum"])) < 1e-6
    for l in range(layers):
        assert abs(float(Ws[l].astype(np.float64).sum()) - float(g["W%d_sum" % l])) < 1e-6
    g.update(x=x, gy=gy, Ws=Ws, bs=bs, adj=dense_from_coo(g["coo"], B, T),
             masks=np.arange(T)[None, :] >= g["lens"][:, None])
    return g


@functools.lru_cache(maxsize=None)
def star_parse_case():
    """Star-shaped parses, for the paths that ordinary trees (rows of <= 4 entries) never reach: B = 6, T = 120, K = 3, one head with
    13 ... 38 kept children per sentence, more than 64 rows with edges in some sentence.  Returns (batch, the C oracle's result, K);
    shared between tests, so read only."""
    from oracle import prune_ref
    B, T, K = 6, 120, 3
    rng = np.random.RandomState(77)
    g = synthetic.random_tree_batch(78, B, T, np.array([120, 118, 115, 110, 104, 100], np.int32))
    for b in range(B):
        n = int(g["lens"][b])
        hub = int(g["subj_span"][b, 0])                                   # a subject token: on the path, so its children survive K >= 1
        kids = rng.permutation(np.setdiff1d(np.arange(n), [hub]))[: 13 + 5 * b]
        # re-hang `kids` under the hub unless that would detach the hub from the root (skip the hub's own ancestors)
        anc, a = set(), hub
        while g["head"][b, a] != 0:
            a = int(g["head"][b, a]) - 1
            anc.add(a)
        for c in kids:
            if int(c) not in anc:
                g["head"][b, c] = hub + 1
    want = prune_ref.batch_adj(g["head"], g["subj_pos"], g["obj_pos"], g["deprel"], g["lens"], K)
    assert want["rc"] == 0
    A = want["adj"] != 0
    assert (A.sum(2).max(1) >= 13).all(), "the fixture must have a row with more than 12 entries in every sentence"
    assert (A.any(2).sum(1) > 64).any(), "and more than 64 rows with edges in some sentence"
    return g, want, K


LAYER_CASES = ["layers_c1_l1.npz", "layers_c1_l2.npz", "layers_c2s.npz", "layers_c3s.npz", "layers_c5s.npz"]


# ---- GPU test modules: the bodies of their `dev` / `api` fixtures, host arrays to the device, pruned trees, scoped options ----
def cuda_dev():
    import torch
    assert torch.cuda.is_available(), "gpu-marked tests need the MI355X"
    return torch.device("cuda:0")


def gcn_api():
    from gcn_over_pruned_trees_amd import _lib
    from gcn_over_pruned_trees_amd.model import gcn, tree
    _lib.lib()
    return gcn, tree


def to_dev(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def prune(tree, tb, K, dev):
    T = tb["head"].shape[1]
    masks = np.arange(T)[None, :] >= tb["lens"][:, None]
    return tree.prune_to_csr(to_dev(tb["head"], dev), to_dev(tb["subj_pos"], dev), to_dev(tb["obj_pos"], dev), to_dev(tb["deprel"], dev), K,
                             masks=to_dev(masks, dev))


@contextlib.contextmanager
def options(**kv):
    """gcnpt_set_option for the duration of a with-block, keys by name: options(WIDE_BWD=1, DETERMINISTIC=1)."""
    from gcn_over_pruned_trees_amd import _lib
    old = []
    try:
        for k, v in kv.items():
            key = getattr(_lib, "OPT_" + k)
            old.append((key, _lib.set_option(key, v)))
        yield
    finally:
        for key, v in reversed(old):
            _lib.set_option(key, v)


# ---- a restatement of rowtile_shape + rowtile_lds_bytes (csrc/rowtile_body.h), default options ----
ROWS, WAVE, LDS_MAX = 32, 64, 160 * 1024


def _lds_stride_dw(payload):
    s = -(-payload // 4) * 4
    while (s & 15) != 8:
        s += 4
    return s


def _out_stride_dw(payload):
    s = -(-payload // 4) * 4
    while (s & 7) != 4:
        s += 4
    return s


def rowtile_lds(N, K, NOUT, ct, ot, vec, bwd):
    """LDS bytes the one-shot row tile asks for over N rows: the contraction runs over K (forward: Din; backward-data: H), the output
    is NOUT wide (forward: H; backward-data: Din); ct / ot bytes of the MFMA operand / output; rows read by vectors (vec) or element
    by element.  The S tile, the out tile (bwd: the larger of it and the Z tile, two tiles of width K), the adjacency tables, the bias
    of a column pass."""
    kstep = 32 if ct == 2 else 16
    kpad = -(-K // kstep) * kstep
    n_tiles = -(-NOUT // 16)
    four = vec and -(-N // ROWS) > 256 and (n_tiles <= 24 or -(-n_tiles // 20) <= -(-n_tiles // 32))
    if not vec:
        nwv, ntw = 8, 4
    elif four:
        nwv, ntw = 4, (2 if n_tiles <= 8 else 3 if n_tiles <= 12 else 4 if n_tiles <= 16 else 6 if 20 < n_tiles <= 24 else 5)
    else:
        nwv, ntw = 8, (2 if n_tiles <= 16 else 3 if n_tiles <= 24 else 4)
    stride = _lds_stride_dw(kpad * ct // 4) * 4 // ct
    ncols = nwv * ntw * 16
    ostride = _out_stride_dw(min(-(-NOUT // 16) * 16, ncols) * ot // 4) * 4 // ot
    s_bytes, o_bytes = ROWS * stride * ct, ROWS * ostride * ot
    return s_bytes + (max(s_bytes, o_bytes) if bwd else o_bytes) + ROWS * 13 * 4 + max(nwv * WAVE, ncols) * 4
