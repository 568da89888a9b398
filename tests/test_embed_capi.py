"""CPU-side checks of the embedding front end's entry points (include/gcnpt.h gcnpt_embed_fwd / gcnpt_embed_bwd): the symbols are exported
and bound, and argument validation returns GCNPT_E_INVALID with a text that names the entry point before anything is launched.  No
compute is launched here."""
import ctypes

import pytest

from gcn_over_pruned_trees_amd import _lib

NAMES = ("gcnpt_embed_fwd", "gcnpt_embed_bwd")


def test_embed_symbols_exported_and_bound():
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert name in _lib.SIGNATURES, name
        assert hasattr(handle, name), name
    assert _lib.lib().gcnpt_abi_version() == 7                      # nothing existing changed


def _calls(p):
    """name -> f(**overrides): the entry point called with valid-looking arguments (never launched: one is always bad)."""
    L = _lib.lib()
    base = dict(words=p, dense=None, pos=p, ner=p, emb=p, pos_emb=p, ner_emb=p, V=(50, 47, 15), E=(8, 4, 2), cu=None, B=2, T=5, n_rows=0,
                out=p, dtype=_lib.F32, p_emb=0.0, p_in=0.0, g=p, d_emb=p, d_rows=None, d_dense=None, d_pos=p, d_ner=p)

    def fwd(**kw):
        a = dict(base, **kw)
        return L.gcnpt_embed_fwd(None, a["words"], a["dense"], a["pos"], a["ner"], a["emb"], a["pos_emb"], a["ner_emb"], *a["V"], *a["E"],
                                 a["cu"], a["B"], a["T"], a["n_rows"], a["out"], a["dtype"], a["p_emb"], a["p_in"], 1, 2, None, None)

    def bwd(**kw):
        a = dict(base, **kw)
        return L.gcnpt_embed_bwd(None, a["g"], a["dtype"], a["words"], a["pos"], a["ner"], *a["V"], *a["E"], a["cu"], a["B"], a["T"],
                                 a["n_rows"], a["p_emb"], a["p_in"], 1, 2, None, 0, 0, a["d_emb"], a["d_rows"], a["d_dense"], a["d_pos"],
                                 a["d_ner"])
    return {"embed_fwd": fwd, "embed_bwd": bwd}


COMMON_BAD = (dict(B=0), dict(B=-3), dict(T=0), dict(E=(0, 4, 2)), dict(E=(8, -1, 2)), dict(dtype=7), dict(p_emb=1.0), dict(p_in=-0.1),
              dict(p_in=1.5), dict(cu=True, n_rows=0), dict(cu=True, n_rows=-4), dict(pos=None))


@pytest.mark.parametrize("name", ["embed_fwd", "embed_bwd"])
def test_embed_argument_validation_needs_no_gpu(name):
    L = _lib.lib()
    buf = ctypes.create_string_buffer(256)
    p = ctypes.addressof(buf)
    call = _calls(p)[name]
    extra = {
        "embed_fwd": (dict(out=None), dict(emb=None), dict(pos_emb=None), dict(ner_emb=None),
                      dict(dense=p),                                    # word ids AND a dense source
                      dict(words=None)),                                # neither
        "embed_bwd": (dict(g=None), dict(d_emb=None, d_pos=None, d_ner=None),            # no output at all
                      dict(d_rows=p),                                   # dense and row-sparse word gradient together
                      dict(d_emb=None, d_dense=p),                      # word ids AND a dense source's gradient
                      dict(words=None)),                                # a word table gradient without the ids
    }[name]
    for bad in COMMON_BAD + extra:
        kw = dict(bad, cu=p) if bad.get("cu") is True else bad
        assert call(**kw) == _lib.E_INVALID, bad
        assert (name + ":").encode() in L.gcnpt_last_error(), (bad, L.gcnpt_last_error())
    assert call(B=0) == _lib.E_INVALID and b"positive" in L.gcnpt_last_error()
    assert call(cu=p, n_rows=0) == _lib.E_INVALID and b"n_rows" in L.gcnpt_last_error()
    assert call(dtype=7) == _lib.E_INVALID and b"dtype" in L.gcnpt_last_error()
    assert call(p_emb=1.0) == _lib.E_INVALID and b"[0, 1)" in L.gcnpt_last_error()


def test_embed_inputs_refuses_cpu_tensors():
    import torch
    from gcn_over_pruned_trees_amd.model import gcn
    ids = torch.zeros((2, 5), dtype=torch.int64)
    emb, pos_emb, ner_emb = torch.nn.Embedding(10, 8, padding_idx=0), torch.nn.Embedding(4, 2), torch.nn.Embedding(3, 2)
    with pytest.raises(TypeError):
        gcn.embed_inputs(ids, ids, ids, emb, pos_emb, ner_emb)
    with pytest.raises(TypeError):                                  # the dense word source likewise
        gcn.embed_inputs(torch.zeros(2, 5, 8), ids, ids, None, pos_emb.weight, None)
