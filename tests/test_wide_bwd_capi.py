"""CPU-side checks of the wide form of the layer backward-data (csrc/wide_kernels.hip, wide_bwd_kernel): its option and where the
dispatcher takes it, i.e. where the one-shot row tile's backward is refused for its LDS.  No compute is launched here: the calls
below are refused before any launch."""
import ctypes
import re

import pytest

from helpers import LDS_MAX, rowtile_lds


def _lib():
    from gcn_over_pruned_trees_amd import _lib as lib
    return lib


def _bwd_lds(N, din, H, ct, ot, vec):
    """rowtile_bwd_too_wide's byte count (rowtile_shape + rowtile_lds_bytes, csrc/rowtile_body.h) for a backward-data launch: the
    contraction runs over H (Kpad), the output is Din wide."""
    return rowtile_lds(N, H, din, ct, ot, vec, True)


def _refused_vec(N, din, H, ct, ot, vec):
    return _bwd_lds(N, din, H, ct, ot, vec) > LDS_MAX


def test_wide_bwd_option():
    lib = _lib()
    L = lib.lib()
    assert lib.OPT_WIDE_BWD == 6
    assert L.gcnpt_get_option(lib.OPT_WIDE_BWD) == -1
    # the other options keep their defaults; key 5 stays unknown (tests/test_wide_capi.py)
    assert L.gcnpt_get_option(lib.OPT_DETERMINISTIC) == 0 and L.gcnpt_get_option(lib.OPT_FOUR_WAVES) == -1
    assert L.gcnpt_get_option(lib.OPT_SIDE_TILES) == 192 and L.gcnpt_get_option(lib.OPT_COL_SPLIT) == -1
    assert L.gcnpt_get_option(lib.OPT_WIDE_FORM) == -1
    assert L.gcnpt_set_option(5, 0) == lib.E_INVALID and L.gcnpt_get_option(5) == lib.E_INVALID
    assert L.gcnpt_set_option(7, 0) == lib.E_INVALID
    for bad in (2, -2):
        assert L.gcnpt_set_option(lib.OPT_WIDE_BWD, bad) == lib.E_INVALID
        assert b"wide_bwd" in L.gcnpt_last_error()
    assert L.gcnpt_get_option(lib.OPT_WIDE_BWD) == -1
    old = lib.set_option(lib.OPT_WIDE_BWD, 0)
    try:
        for v in (-1, 0, 1):
            assert L.gcnpt_set_option(lib.OPT_WIDE_BWD, v) == lib.OK
            assert L.gcnpt_get_option(lib.OPT_WIDE_BWD) == v
            assert L.gcnpt_get_option(lib.OPT_WIDE_FORM) == -1          # the forward's option is a separate key
    finally:
        lib.set_option(lib.OPT_WIDE_BWD, old)
    assert L.gcnpt_get_option(lib.OPT_WIDE_BWD) == -1


@pytest.mark.parametrize("N", [5000, 40 * 300])
@pytest.mark.parametrize("din", [200, 360, 1084])
def test_boundary(N, din):
    """The widest hidden layer the row tile's backward holds: fp32 608, bf16 1216 (16-byte rows; element loads and float32 or bf16
    dh alike), whatever the input width and the batch."""
    for vec in (True, False):
        for ot in (4, 2):
            assert not _refused_vec(N, din, 608, 4, ot, vec) and _refused_vec(N, din, 609, 4, ot, vec)
            assert not _refused_vec(N, din, 1216, 2, ot, vec) and _refused_vec(N, din, 1217, 2, ot, vec)


_P = ctypes.c_void_p(1 << 20)           # a 16-byte-aligned dummy address: never dereferenced by a refused call


def _bwd_data(lib, B, T, din, H, compute, dh_dtype, src_is_dz=0):
    L = lib.lib()
    return L.gcnpt_layer_bwd_data(None, _P, _P, dh_dtype, _P, _P, _P, _P, _P, B, T, din, H, _P, dh_dtype, compute, 1.0, _P, _P, _P, None, 1.0,
                                  src_is_dz)


@pytest.mark.parametrize("compute", ["fp32", "bf16"])
def test_option_zero_refuses_exactly_the_restated_bytes(compute):
    """GCNPT_OPT_WIDE_BWD = 0 takes the row tile everywhere: past the boundary gcnpt_layer_bwd_data returns GCNPT_E_UNSUPPORTED before
    any launch, and the byte count in its message is the restatement's, so rowtile_bwd_too_wide (the same count) holds exactly there."""
    lib = _lib()
    L = lib.lib()
    cd = lib.F32 if compute == "fp32" else lib.BF16
    ct = 4 if cd == lib.F32 else 2
    first = 609 if cd == lib.F32 else 1217
    old = lib.set_option(lib.OPT_WIDE_BWD, 0)
    try:
        for B, T, din in ((50, 100, 360), (400, 100, 200), (3, 41, 1084)):
            for H in (first, first + 7, first + 15, 768, 1024, 2048):
                if H < first:
                    continue
                for dz in (0, 1):
                    for dh_dtype in ((lib.F32,) if cd == lib.F32 else (lib.F32, lib.BF16)):
                        rc = _bwd_data(lib, B, T, din, H, cd, dh_dtype, dz)
                        assert rc == lib.E_UNSUPPORTED, (B, T, din, H, dz)
                        msg = L.gcnpt_last_error().decode()
                        got = int(re.search(r"needs (\d+) B of LDS", msg).group(1))
                        want = _bwd_lds(B * T, din, H, ct, 4 if dh_dtype == lib.F32 else 2, H % 8 == 0)
                        assert got == want and want > LDS_MAX, (B, T, din, H, got, want)
    finally:
        lib.set_option(lib.OPT_WIDE_BWD, old)
