"""CPU-side checks of the native output head's entry points (include/gcnpt.h gcnpt_head_linear_fwd / _bwd, gcnpt_head_loss_fwd / _bwd): the
symbols are exported and bound, argument validation returns GCNPT_E_INVALID with a text that names the entry point before anything is
launched, the Python ops refuse CPU tensors, and the option leaves the module surface alone.  No compute is launched here."""
import ctypes

import pytest

from gcn_over_pruned_trees_amd import _lib

NAMES = ("gcnpt_head_linear_fwd", "gcnpt_head_linear_bwd", "gcnpt_head_loss_fwd", "gcnpt_head_loss_bwd")


def test_head_symbols_exported_and_bound():
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert name in _lib.SIGNATURES, name
        assert hasattr(handle, name), name
    assert _lib.lib().gcnpt_abi_version() == 7                      # nothing existing changed


def _calls(p):
    """name -> f(**overrides): the entry point called with valid-looking arguments (never launched: one is always bad)."""
    L = _lib.lib()
    base = dict(x=p, ldx=8, w=p, b=p, y=p, dy=p, dx=p, ld_dx=8, dw=p, db=p, M=4, K=8, N=3, relu=1,
                logits=p, labels=p, pooled=p, ldp=6, H=6, l2=0.003, C=5, loss=p, probs=p, pred=p, status=p, dloss=p, dlogits=p, dpooled=p)

    def linear_fwd(**kw):
        a = dict(base, **kw)
        return L.gcnpt_head_linear_fwd(None, a["x"], a["ldx"], a["w"], a["b"], a["y"], a["M"], a["K"], a["N"], a["relu"])

    def linear_bwd(**kw):
        a = dict(base, **kw)
        return L.gcnpt_head_linear_bwd(None, a["dy"], a["y"], a["x"], a["ldx"], a["w"], a["dx"], a["ld_dx"], a["dw"], a["db"], a["M"], a["K"],
                                       a["N"], a["relu"])

    def loss_fwd(**kw):
        a = dict(base, **kw)
        return L.gcnpt_head_loss_fwd(None, a["logits"], a["labels"], a["pooled"], a["ldp"], a["H"], a["l2"], a["M"], a["C"], a["loss"],
                                     a["probs"], a["pred"], a["status"])

    def loss_bwd(**kw):
        a = dict(base, **kw)
        return L.gcnpt_head_loss_bwd(None, a["dloss"], a["logits"], a["labels"], a["pooled"], a["ldp"], a["H"], a["l2"], a["M"], a["C"],
                                     a["dlogits"], a["dpooled"])
    return {"head_linear_fwd": linear_fwd, "head_linear_bwd": linear_bwd, "head_loss_fwd": loss_fwd, "head_loss_bwd": loss_bwd}


LINEAR_BAD = (dict(M=0), dict(M=-2), dict(K=0), dict(N=0), dict(N=-1), dict(ldx=7), dict(relu=2), dict(relu=-1), dict(x=None), dict(w=None))
LOSS_BAD = (dict(M=0), dict(C=0), dict(C=-5), dict(logits=None), dict(ldp=5), dict(H=0), dict(l2=-0.5), dict(l2=float("nan")))
BAD = {
    "head_linear_fwd": LINEAR_BAD + (dict(b=None), dict(y=None)),
    "head_linear_bwd": LINEAR_BAD + (dict(dy=None), dict(dw=None), dict(db=None), dict(ld_dx=7),
                                     dict(y=None)),                                         # relu = 1 needs the forward's output
    "head_loss_fwd": LOSS_BAD + (dict(loss=None, probs=None, pred=None, status=None),     # no output at all
                                 dict(labels=None)),                                        # the loss wanted without labels
    "head_loss_bwd": LOSS_BAD + (dict(dloss=None), dict(dlogits=None, dpooled=None), dict(labels=None), dict(pooled=None)),
}


@pytest.mark.parametrize("name", sorted(BAD))
def test_head_argument_validation_needs_no_gpu(name):
    L = _lib.lib()
    buf = ctypes.create_string_buffer(256)
    call = _calls(ctypes.addressof(buf))[name]
    for bad in BAD[name]:
        assert call(**bad) == _lib.E_INVALID, bad
        assert L.gcnpt_last_error().startswith((name + ":").encode()), (bad, L.gcnpt_last_error())
    assert call(M=0) == _lib.E_INVALID and b"positive" in L.gcnpt_last_error()
    if "linear" in name:
        assert call(ldx=7) == _lib.E_INVALID and b"ldx" in L.gcnpt_last_error()
        assert call(relu=2) == _lib.E_INVALID and b"relu" in L.gcnpt_last_error()
    else:
        assert call(ldp=5) == _lib.E_INVALID and b"ldp" in L.gcnpt_last_error()
        assert call(l2=-0.5) == _lib.E_INVALID and b"l2" in L.gcnpt_last_error()
    if name == "head_linear_bwd":
        assert call(y=None) == _lib.E_INVALID and b"ReLU mask" in L.gcnpt_last_error()
    if name == "head_loss_fwd":
        assert call(labels=None) == _lib.E_INVALID and b"needs labels" in L.gcnpt_last_error()


def test_head_ops_refuse_cpu_tensors():
    import torch
    from gcn_over_pruned_trees_amd.model import gcn
    x, w, b = torch.zeros(3, 8), torch.zeros(4, 8), torch.zeros(4)
    with pytest.raises(TypeError):
        gcn.linear_act(x, w, b, relu=True)
    with pytest.raises(TypeError):
        gcn.head_loss(torch.zeros(3, 4), torch.zeros(3, dtype=torch.int64), torch.zeros(3, 8), 0.003)
    with pytest.raises(TypeError):
        gcn.head_predict(torch.zeros(3, 4))


def test_native_head_keeps_the_module_surface():
    import inspect
    from gcn_over_pruned_trees_amd.model import gcn
    opt = dict(vocab_size=50, emb_dim=8, pos_dim=2, ner_dim=2, hidden_dim=16, num_layers=2, input_dropout=0.0, gcn_dropout=0.5,
               prune_k=1, pooling="max", mlp_layers=3, rnn=False, dataset="tacred", num_class=42, topn=10, cuda=False)
    plain, native = gcn.GCNClassifier(opt), gcn.GCNClassifier(dict(opt, gcn_native_head=True))
    assert list(plain.state_dict().keys()) == list(native.state_dict().keys())
    assert [n for n, _ in plain.named_modules()] == [n for n, _ in native.named_modules()]
    assert list(inspect.signature(gcn.GCNClassifier.forward).parameters) == ["self", "inputs", "trees"]
    assert list(inspect.signature(gcn.GCNClassifier.loss).parameters) == ["self", "logits", "pooling_output", "labels"]
    assert list(inspect.signature(gcn.GCNClassifier.predict).parameters) == ["self", "logits"]
    # the torch formulation of the loss (option off) is what the reference's trainer computes; it runs anywhere
    import torch
    logits, pooled = torch.randn(5, 42), torch.randn(5, 16)
    labels = torch.arange(5)
    m = gcn.GCNClassifier(dict(opt, pooling_l2=0.003, conv_l2=0.01))
    want = torch.nn.functional.cross_entropy(logits, labels) + m.conv_l2() * 0.01 + 0.003 * (pooled ** 2).sum(1).mean()
    assert abs(float(m.loss(logits, pooled, labels).detach()) - float(want.detach())) <= 1e-6 * abs(float(want))
    probs, pred = m.predict(logits)
    assert torch.equal(pred, logits.argmax(1)) and torch.allclose(probs.sum(1), torch.ones(5))
