"""The K-fitted shape of the one-shot row-tile kernel (csrc/rowtile_body.h, rowtile_shape: layers of <= 16 column tiles and <= 7 k-steps
hold exactly their k-steps of weight fragments and gather their own rows 2 chunks per thread), through the C-ABI on two-layer stacks of
80 rows (B = 2, T = 40: two full 32-row tiles and a ragged one): forward, backward from dY and Y, backward on a handed-down dZ, and the
sweep whose bottom launch carries the upper layer's weight gradient -- against the float64-accumulating oracle at the tolerances of
test_gpu_parity.py, and bit for bit against the column-split form (GCNPT_OPT_COL_SPLIT), which never had the filler requests."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from helpers import FWD_RTOL, GRAD_RTOL, cuda_dev, gcn_api, max_rel, options, prune, to_dev

pytestmark = pytest.mark.gpu

BF16_FWD = 2e-2         # test_gpu_parity.py: bf16 forward and gradients (the latter against the oracle driven by the device's activations)
BF16_GRAD = 2e-2
B, T = 2, 40

# Din -> H -> H.  bf16 k-steps are 32 wide, fp32 ones 16:
#   200 / 224   exactly 7 bf16 k-steps in every launch (fp32: 13 / 14 k-steps, the 13- and 12-step shapes)
#   225         8 bf16 k-steps in the bottom layer, and rows no vector load or store can take (the element shape there); 200 above
#   232         8 bf16 k-steps with vector rows: must still take the 12-step shape
#   8 -> 16     one k-step
#   112         exactly 7 fp32 k-steps
WIDTHS = [(200, 200), (224, 200), (225, 200), (232, 200), (8, 16), (112, 112)]
PRECISIONS = [torch.bfloat16, torch.float32]


class _Stack:
    """A two-layer stack at the C-ABI in uniform precision `dt` (activations and MFMA operands): weights packed, the forward with its S
    images (gcnpt_layers_fwd), the backward sweeps (gcnpt_layers_bwd / _bwd_dz / _bwd_range) into buffers pre-filled with NaN."""

    def __init__(self, dev, trees, x, Ws, bs, dt):
        from gcn_over_pruned_trees_amd import _lib
        from gcn_over_pruned_trees_amd.model.gcn import WeightPack
        self.lib, self.dev, self.trees, self.x, self.bs, self.dt = _lib, dev, trees, x, bs, dt
        self.cd = _lib.dtype_code(dt)
        self.dims = [tuple(w.shape) for w in Ws]                # (H, K) per layer
        self.pk = WeightPack(Ws, self.cd, dev)
        _lib.check(_lib.lib().gcnpt_pack_weights_multi(_lib.stream(), *self.pk.c_args()))
        torch.cuda.synchronize()

    def _ints(self, v):
        return (ctypes.c_int * 2)(*v)

    def fwd(self):
        """Returns (layer outputs, S images)."""
        lib, t = self.lib, self.trees
        outs = [torch.full((B, T, H), float("nan"), dtype=self.dt, device=self.dev) for H, _ in self.dims]
        sf = [torch.full((lib.lib().gcnpt_frag_bytes(B * T, K, self.cd),), 0xFF, dtype=torch.uint8, device=self.dev) for _, K in self.dims]
        lib.check(lib.lib().gcnpt_layers_fwd(
            lib.stream(), 2, lib.ptr(self.x), self.cd, lib.ptr_array(self.pk.wf), lib.ptr_array(self.bs), lib.ptr(t.row_ptr), lib.ptr(t.col_idx),
            lib.ptr(t.ell), lib.ptr(t.ell), B, T, self._ints([k for _, k in self.dims]), self._ints([h for h, _ in self.dims]),
            lib.ptr_array(outs), self._ints([self.cd, self.cd]), self.cd, (ctypes.c_float * 2)(0.0, 0.0), (ctypes.c_uint64 * 2)(0, 0),
            lib.ptr_array(sf), None))
        torch.cuda.synchronize()
        return outs, sf

    def bwd(self, outs, sf, g, gy_is_dz, pieces=None):
        """The sweep (pieces: one launch at a time through gcnpt_layers_bwd_range).  Returns (dh, dZ images, dW, db, grid of each piece)."""
        lib, t = self.lib, self.trees
        dh = [torch.full((B, T, K), float("nan"), dtype=self.dt, device=self.dev) for _, K in self.dims]
        zf = [torch.full((lib.lib().gcnpt_frag_bytes(B * T, H, self.cd),), 0xFF, dtype=torch.uint8, device=self.dev) for H, _ in self.dims]
        dW = [torch.full((H, K), float("nan"), device=self.dev) for H, K in self.dims]
        db = [torch.full((H,), float("nan"), device=self.dev) for H, _ in self.dims]
        args = (lib.stream(), 2, lib.ptr(g), lib.ptr_array(outs), self._ints([self.cd, self.cd]), lib.ptr_array(self.pk.wb), lib.ptr(t.ell),
                lib.ptr(t.rowT_ptr), lib.ptr(t.colT_idx), lib.ptr(t.ellT), B, T, self._ints([k for _, k in self.dims]),
                self._ints([h for h, _ in self.dims]), lib.ptr_array(dh), self._ints([self.cd, self.cd]), self.cd, (ctypes.c_float * 2)(1.0, 1.0),
                lib.ptr_array(zf), lib.ptr_array(sf), lib.ptr_array(dW), lib.ptr_array(db))
        L = lib.lib()
        grids = []
        if pieces is None:
            lib.check((L.gcnpt_layers_bwd_dz if gy_is_dz else L.gcnpt_layers_bwd)(*args))
        else:
            for k in range(pieces):
                lib.check(L.gcnpt_layers_bwd_range(*args, 1 if gy_is_dz else 0, k, 1))
                v = [ctypes.c_int() for _ in range(4)]
                lib.check(L.gcnpt_last_launch(*[ctypes.byref(q) for q in v]))
                grids.append(v[0].value)
                torch.cuda.synchronize()
        torch.cuda.synchronize()
        return dh, zf, dW, db, grids


@functools.lru_cache(maxsize=None)
def _case(widths, dt):
    """One stack per (widths, precision), shared by the tests below and read only: the stack, the forward's results, its inputs on the
    host (x as the device holds it, i.e. rounded to `dt`) and the dense adjacency."""
    from gcn_over_pruned_trees_amd.utils import synthetic
    dev = cuda_dev()
    _, tree = gcn_api()
    din, hid = widths
    seed = 900 + din + hid
    tb = synthetic.random_tree_batch(seed, B, T, np.array([40, 33], np.int32))
    trees = prune(tree, tb, 1, dev)
    Wn, bn = synthetic.layer_params(seed + 1, [din, hid, hid])
    x = to_dev(synthetic.normal(seed + 2, (B, T, din)), dev).to(dt)
    gyn = synthetic.normal(seed + 3, (B, T, hid))
    st = _Stack(dev, trees, x, [to_dev(w, dev) for w in Wn], [to_dev(b, dev) for b in bn], dt)
    outs, sf = st.fwd()
    adj = trees.to_dense().cpu().numpy().astype(np.float32)
    return dict(st=st, outs=outs, sf=sf, adj=adj, xn=x.float().cpu().numpy(), Wn=Wn, bn=bn, gyn=gyn, gy=to_dev(gyn, dev).to(dt))


def _f(t):
    return t.detach().float().cpu().numpy()


def _top_dz(c):
    """The top layer's dZ ready-made, as the pooling's hand-over leaves it: dY * 1[Y > 0] / (deg + 1), in the stack's precision."""
    y1 = c["outs"][1].float()
    den = to_dev((c["adj"] != 0).sum(2).astype(np.float32) + 1.0, y1.device).unsqueeze(-1)     # the adjacency carries deprel labels
    return torch.where(y1 > 0, c["gy"].float() / den, torch.zeros_like(y1)).to(c["st"].dt)


def _check_grads(c, dh, dW, db):
    """dx, dW_l, db_l against the oracle differentiated through the device's own activations (relu' is a step function: a
    pre-activation rounded to the other side of zero would otherwise move whole gradient terms)."""
    from oracle import gcn_ref
    acts = [_f(o) for o in c["outs"]]
    dx, dWs, dbs = gcn_ref.gcn_backward(c["adj"], c["xn"], c["Wn"], c["bn"], _f(c["gy"]), acts=acts)
    tol = GRAD_RTOL if c["st"].dt == torch.float32 else BF16_GRAD
    errs = dict(dx=max_rel(_f(dh[0]), dx))
    for l in range(2):
        errs["dW%d" % l] = max_rel(_f(dW[l]), dWs[l])
        errs["db%d" % l] = max_rel(_f(db[l]), dbs[l])
    print("grads vs oracle:", {k: "%.2e" % v for k, v in errs.items()}, "tol %.0e" % tol)
    assert all(v <= tol for v in errs.values()), errs


@pytest.mark.parametrize("dt", PRECISIONS, ids=["bf16", "fp32"])
@pytest.mark.parametrize("widths", WIDTHS, ids=lambda w: "%dto%d" % w)
def test_forward_vs_oracle(widths, dt):
    """Both layers' outputs against oracle/gcn_ref.py (fp32: FWD_RTOL; bf16: 2e-2); every row and every image element is written."""
    from oracle import gcn_ref
    c = _case(widths, dt)
    _, _, (_, _, saved) = gcn_ref.gcn_forward(c["adj"], c["xn"], c["Wn"], c["bn"], return_saved=True)
    tol = FWD_RTOL if dt == torch.float32 else BF16_FWD
    for l in range(2):
        got = _f(c["outs"][l])
        assert not np.isnan(got).any(), "layer %d: an output element was not written" % l
        assert not torch.isnan(c["sf"][l].view(dt)).any(), "S image %d: an element was not written" % l
        err = max_rel(got, saved[l][2])
        print("layer %d forward vs oracle: %.2e (tol %.0e)" % (l, err, tol))
        assert err <= tol, l
    assert float(c["outs"][1].float().abs().max()) > 0


@pytest.mark.parametrize("entry", ["dy", "dz"])
@pytest.mark.parametrize("dt", PRECISIONS, ids=["bf16", "fp32"])
@pytest.mark.parametrize("widths", WIDTHS, ids=lambda w: "%dto%d" % w)
def test_backward_sweep_vs_oracle(widths, dt, entry):
    """The backward sweep from dY and Y (gcnpt_layers_bwd: the top launch derives dZ) and from a ready-made top dZ (gcnpt_layers_bwd_dz:
    every launch runs on handed-down dZ rows).  In both, the bottom layer's launch carries the top layer's weight gradient (3 row tiles,
    uniform precision).  dx, dW_l and db_l against the oracle (fp32: GRAD_RTOL; bf16: 2e-2); dh and the dZ images fully written."""
    c = _case(widths, dt)
    g = _top_dz(c) if entry == "dz" else c["gy"]
    with options(DETERMINISTIC=1):
        dh, zf, dW, db, _ = c["st"].bwd(c["outs"], c["sf"], g, entry == "dz")
    for l in range(2):
        assert not torch.isnan(dh[l].float()).any(), "dh[%d]: an element was not written" % l
        assert not torch.isnan(zf[l].view(dt)).any(), "dZ image %d: an element was not written" % l
    _check_grads(c, dh, dW, db)


@pytest.mark.parametrize("dt", PRECISIONS, ids=["bf16", "fp32"])
@pytest.mark.parametrize("widths", WIDTHS, ids=lambda w: "%dto%d" % w)
def test_bottom_launch_carries_upper_weight_gradient(widths, dt):
    """The sweep one launch at a time (gcnpt_layers_bwd_range): its second launch, layer 0's backward-data in the K-fitted shape, has the
    passenger workgroups of layer 1's weight gradient behind its 3 row tiles (grid >= 8 + 8), the third is layer 0's weight gradient
    alone; the pieces give the whole sweep's results bit for bit (deterministic weight gradients), and those meet the oracle."""
    c = _case(widths, dt)
    with options(DETERMINISTIC=1):
        whole = c["st"].bwd(c["outs"], c["sf"], c["gy"], False)
        parts = c["st"].bwd(c["outs"], c["sf"], c["gy"], False, pieces=3)
    assert parts[4][0] == 3 and parts[4][1] >= 16, parts[4]
    for l in range(2):
        assert torch.equal(whole[0][l], parts[0][l]), "dh[%d]" % l
        assert torch.equal(whole[1][l], parts[1][l]), "dZ image %d" % l
        assert torch.equal(whole[2][l], parts[2][l]) and torch.equal(whole[3][l], parts[3][l]), "dW / db %d" % l
    _check_grads(c, parts[0], parts[2], parts[3])


@pytest.mark.parametrize("entry", ["dy", "dz"])
@pytest.mark.parametrize("widths", WIDTHS, ids=lambda w: "%dto%d" % w)
def test_one_shot_equals_column_split_form(widths, entry):
    """bf16 (the column-split form exists for bf16 MFMA operands): with GCNPT_OPT_COL_SPLIT = 1 every launch with vector rows takes the
    column-split form, whose waves always held exactly the layer's k-steps.  Rows (both layers' outputs, the handed-down dZ, dx) and
    both fragment images (S of the forward, dZ of the backward) of the one-shot form are bit-identical to it; the weight gradients come
    from identical images in differently grouped launches (a column-split launch carries no passenger): 1e-5."""
    c = _case(widths, torch.bfloat16)
    st = c["st"]
    res = []
    for cs in (0, 1):
        with options(COL_SPLIT=cs, DETERMINISTIC=1):
            outs, sf = st.fwd()
            g = _top_dz(c) if entry == "dz" else c["gy"]
            res.append((outs, sf) + st.bwd(outs, sf, g, entry == "dz")[:4])
    a, b = res
    for l in range(2):
        assert torch.equal(a[0][l], c["outs"][l]), "the shared forward's layer %d" % l
        assert torch.equal(a[0][l], b[0][l]), "output rows of layer %d" % l
        assert torch.equal(a[1][l], b[1][l]), "S image %d" % l
        assert torch.equal(a[2][l], b[2][l]), "dh[%d]" % l
        assert torch.equal(a[3][l], b[3][l]), "dZ image %d" % l
        assert max_rel(_f(b[4][l]), _f(a[4][l])) <= 1e-5 and max_rel(_f(b[5][l]), _f(a[5][l])) <= 1e-5, "dW / db %d" % l
    assert float(a[2][0].float().abs().max()) > 0
