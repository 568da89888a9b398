"""CPU-side checks of the token-packed forms of the relation-aware layers (include/gcnpt.h: gcnpt_full_agg_*_packed,
gcnpt_diag_layer_*_packed, gcnpt_pack_ids): the symbols are exported and bound, the ABI version stands (the additions are additive), and
every argument check returns an error with a message before anything is launched -- so none of this needs a GPU."""
import ctypes
import os

from gcn_over_pruned_trees_amd import _lib

NEW = ("gcnpt_full_agg_fwd_packed", "gcnpt_full_agg_bwd_packed", "gcnpt_diag_layer_fwd_packed", "gcnpt_diag_layer_bwd_packed", "gcnpt_pack_ids")


def test_packed_deprel_symbols_are_exported_and_bound():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert hasattr(handle, name), "libgcnpt.so does not export %s" % name
        assert name in _lib.SIGNATURES, "%s is not bound in _lib" % name
        assert list(getattr(_lib.lib(), name).argtypes) == list(_lib.SIGNATURES[name][1])
    assert _lib.lib().gcnpt_abi_version() == _lib.ABI_VERSION == 7


def _refused(rc, *words):
    msg = _lib.lib().gcnpt_last_error()
    assert rc == _lib.E_INVALID, (rc, msg)
    for w in words:
        assert w in msg, (w, msg)


def test_packed_deprel_argument_checks_need_no_gpu():
    L = _lib.lib()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    # full_agg forward: (stream, yf, yr, self, pos, row_ptr, col_idx, label, keep_f, keep_r, n_live, n_rows, nnz_cap, H, M, out, p, seed, seed_dev)
    fwd = lambda **kw: L.gcnpt_full_agg_fwd_packed(*[kw.get(k, v) for k, v in (  # noqa: E731
        ("stream", None), ("yf", p), ("yr", None), ("self_term", None), ("pos", None), ("row_ptr", p), ("col_idx", p), ("label", p),
        ("keep_f", None), ("keep_r", None), ("n_live", p), ("n_rows", 4), ("nnz_cap", 12), ("H", 8), ("M", 4), ("out", p), ("drop_p", 0.0),
        ("seed", 0), ("seed_dev", None))])
    for k in ("yf", "row_ptr", "col_idx", "label", "n_live", "out"):
        _refused(fwd(**{k: None}), b"full_agg_fwd_packed", b"null")
    for k in ("n_rows", "nnz_cap", "H"):
        for bad in (0, -3):
            _refused(fwd(**{k: bad}), b"full_agg_fwd_packed", b"positive")
    _refused(fwd(M=-1), b"positive")
    _refused(fwd(drop_p=1.0), b"drop_p")
    bwd = lambda **kw: L.gcnpt_full_agg_bwd_packed(*[kw.get(k, v) for k, v in (  # noqa: E731
        ("stream", None), ("dy", p), ("y", p), ("pos", None), ("row_ptr", p), ("col_idx", p), ("label", p), ("keep_f", None), ("keep_r", None),
        ("n_live", p), ("n_rows", 4), ("nnz_cap", 12), ("H", 8), ("M", 4), ("scale", 1.0), ("dagg", p), ("dyf", p), ("dyr", None))])
    for k in ("dy", "y", "row_ptr", "col_idx", "label", "n_live", "dagg", "dyf"):
        _refused(bwd(**{k: None}), b"full_agg_bwd_packed", b"null")
    for k in ("n_rows", "nnz_cap", "H"):
        _refused(bwd(**{k: 0}), b"full_agg_bwd_packed", b"positive")
    # diag forward: (stream, h, dtype, E, deprel, row_ptr, col_idx, label, n_live, n_rows, nnz_cap, H, out, p, seed, seed_dev)
    dfwd = lambda **kw: L.gcnpt_diag_layer_fwd_packed(*[kw.get(k, v) for k, v in (  # noqa: E731
        ("stream", None), ("h", p), ("dtype", _lib.F32), ("E", p), ("deprel", p), ("row_ptr", p), ("col_idx", p), ("label", p), ("n_live", p),
        ("n_rows", 4), ("nnz_cap", 12), ("H", 8), ("out", p), ("drop_p", 0.0), ("seed", 0), ("seed_dev", None))])
    for k in ("h", "E", "deprel", "row_ptr", "col_idx", "label", "n_live", "out"):
        _refused(dfwd(**{k: None}), b"diag_layer_fwd_packed", b"null")
    for k, bad in (("n_rows", 0), ("n_rows", -1), ("nnz_cap", 0), ("H", 0), ("dtype", 5)):
        _refused(dfwd(**{k: bad}), b"diag_layer_fwd_packed", b"bad argument")
    _refused(dfwd(drop_p=-0.1), b"drop_p")
    dbwd = lambda **kw: L.gcnpt_diag_layer_bwd_packed(*[kw.get(k, v) for k, v in (  # noqa: E731
        ("stream", None), ("dY", p), ("Y", p), ("h", p), ("dtype", _lib.BF16), ("E", p), ("deprel", p), ("row_ptr", p), ("col_idx", p),
        ("label", p), ("rowT_ptr", p), ("colT_idx", p), ("n_live", p), ("n_rows", 4), ("nnz_cap", 12), ("H", 8), ("dh", p), ("dE", p),
        ("scale", 1.0))])
    for k in ("dY", "Y", "h", "E", "deprel", "row_ptr", "col_idx", "label", "rowT_ptr", "colT_idx", "n_live", "dh", "dE"):
        _refused(dbwd(**{k: None}), b"diag_layer_bwd_packed", b"null")
    for k, bad in (("n_rows", 0), ("nnz_cap", -2), ("H", 0), ("dtype", -1)):
        _refused(dbwd(**{k: bad}), b"diag_layer_bwd_packed", b"bad argument")
    # pack_ids: (stream, src, cu_seqlens, B, T, dst, n_rows, fill)
    ids = lambda **kw: L.gcnpt_pack_ids(*[kw.get(k, v) for k, v in (  # noqa: E731
        ("stream", None), ("src", p), ("cu", p), ("B", 2), ("T", 4), ("dst", p), ("n_rows", 6), ("fill", 0))])
    for k in ("src", "cu", "dst"):
        _refused(ids(**{k: None}), b"pack_ids", b"null")
    for k in ("B", "T", "n_rows"):
        for bad in (0, -1):
            _refused(ids(**{k: bad}), b"pack_ids", b"positive")
    assert buf.raw == b"\0" * 64                                   # nothing ran: the host buffer the "device" pointers name is untouched


def test_pack_rows_points_integer_tensors_to_pack_ids():
    """PackedTrees.pack_rows keeps refusing integer rows (before it touches the library) and names the method that takes them."""
    import pytest
    import torch
    from gcn_over_pruned_trees_amd.model import tree

    class _Trees(object):
        B, T, N = 1, 4, 4
        cu_seqlens = None
    with pytest.raises(TypeError, match="pack_ids"):
        tree._move_rows(torch.zeros((1, 4, 2), dtype=torch.int64), _Trees(), unpack=False)
