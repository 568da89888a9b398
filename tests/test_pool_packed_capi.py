"""CPU-side checks of the poolings on token-packed rows (include/gcnpt.h gcnpt_pool3_fwd_packed / gcnpt_pool3_bwd_packed /
gcnpt_pool3_bwd_dz_packed): the symbols are exported and bound, and argument validation returns GCNPT_E_INVALID with a text that names
the entry point before anything is launched.  No compute is launched here."""
import ctypes

import pytest

from gcn_over_pruned_trees_amd import _lib

NAMES = ("gcnpt_pool3_fwd_packed", "gcnpt_pool3_bwd_packed", "gcnpt_pool3_bwd_dz_packed")


def test_packed_pool_symbols_exported_and_bound():
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert name in _lib.SIGNATURES, name
        assert hasattr(handle, name), name
    assert _lib.lib().gcnpt_abi_version() == 7                      # nothing existing changed


def _calls(p):
    """name -> f(**overrides): the entry point called with valid-looking arguments (never launched: one is always bad)."""
    L = _lib.lib()
    base = dict(cu=p, B=2, T=5, n_rows=7, H=8, type=0, dtype=_lib.F32, argmax=p)

    def fwd(**kw):
        a = dict(base, **kw)
        return L.gcnpt_pool3_fwd_packed(None, p, a["dtype"], p, p, p, a["cu"], a["B"], a["T"], a["n_rows"], a["H"], a["type"], p, a["argmax"])

    def bwd(**kw):
        a = dict(base, **kw)
        return L.gcnpt_pool3_bwd_packed(None, p, a["argmax"], p, p, p, a["cu"], a["B"], a["T"], a["n_rows"], a["H"], a["type"], p, a["dtype"])

    def bwd_dz(**kw):
        a = dict(base, **kw)
        return L.gcnpt_pool3_bwd_dz_packed(None, p, a["argmax"], p, p, p, a["cu"], a["B"], a["T"], a["n_rows"], a["H"], a["type"], p, p, 1.0, p,
                                           a["dtype"])
    return {"pool3_fwd_packed": fwd, "pool3_bwd_packed": bwd, "pool3_bwd_dz_packed": bwd_dz}


@pytest.mark.parametrize("name", ["pool3_fwd_packed", "pool3_bwd_packed", "pool3_bwd_dz_packed"])
def test_packed_pool_argument_validation_needs_no_gpu(name):
    L = _lib.lib()
    buf = ctypes.create_string_buffer(256)
    call = _calls(ctypes.addressof(buf))[name]
    for bad in (dict(cu=None), dict(B=0), dict(n_rows=0), dict(type=3), dict(dtype=7), dict(type=0, argmax=None), dict(T=0), dict(H=0),
                dict(type=-1)):
        assert call(**bad) == _lib.E_INVALID, bad
        assert (name + ":").encode() in L.gcnpt_last_error(), (bad, L.gcnpt_last_error())
    assert call(cu=None) == _lib.E_INVALID and b"null" in L.gcnpt_last_error()
    assert call(type=0, argmax=None) == _lib.E_INVALID and b"argmax" in L.gcnpt_last_error()


def test_packed_pool_dz_needs_y_and_ell():
    L = _lib.lib()
    buf = ctypes.create_string_buffer(256)
    p = ctypes.addressof(buf)
    assert L.gcnpt_pool3_bwd_dz_packed(None, p, p, p, p, p, p, 2, 5, 7, 8, 0, None, p, 1.0, p, _lib.F32) == _lib.E_INVALID
    assert b"pool3_bwd_dz_packed: null" in L.gcnpt_last_error()
    assert L.gcnpt_pool3_bwd_dz_packed(None, p, p, p, p, p, p, 2, 5, 7, 8, 0, p, None, 1.0, p, _lib.F32) == _lib.E_INVALID


def test_pool3_packed_refuses_cpu_tensors_and_wrong_trees():
    import torch
    from gcn_over_pruned_trees_amd.model import gcn
    pos = torch.zeros((2, 5), dtype=torch.int64)
    with pytest.raises(TypeError):
        gcn.pool3_packed(torch.zeros(7, 8), None, pos, pos)
