"""CPU-side checks of the wide form of the layer forward (csrc/wide_kernels.hip): its option, the host-only query
gcnpt_layer_fwd_needs_s_frag, and the refusal of a wide layer without an S image.  No compute is launched here."""
import ctypes

import pytest

from helpers import LDS_MAX, rowtile_lds


def _lib():
    from gcn_over_pruned_trees_amd import _lib as lib
    return lib


def _refused(N, din, H, ct, ot=4):
    """gcnpt_layer_fwd_needs_s_frag restated: the one-shot forward refused for rows 16-byte aligned OR not."""
    return _refused_vec(N, din, H, ct, ot, din % 4 == 0) or _refused_vec(N, din, H, ct, ot, False)


def _refused_vec(N, din, H, ct, ot, vec):
    """rowtile_shape + rowtile_lds_bytes (csrc/rowtile_body.h) for a forward layer: does the one-shot row tile ask for more than
    160 KiB of LDS?"""
    return rowtile_lds(N, din, H, ct, ot, vec, False) > LDS_MAX


def test_wide_form_option():
    lib = _lib()
    L = lib.lib()
    assert lib.OPT_WIDE_FORM == 4
    assert L.gcnpt_get_option(lib.OPT_WIDE_FORM) == -1
    # the other options keep their defaults
    assert L.gcnpt_get_option(lib.OPT_DETERMINISTIC) == 0 and L.gcnpt_get_option(lib.OPT_FOUR_WAVES) == -1
    assert L.gcnpt_get_option(lib.OPT_SIDE_TILES) == 192 and L.gcnpt_get_option(lib.OPT_COL_SPLIT) == -1
    assert L.gcnpt_set_option(lib.OPT_WIDE_FORM, 2) == lib.E_INVALID and L.gcnpt_set_option(lib.OPT_WIDE_FORM, -2) == lib.E_INVALID
    assert b"wide_form" in L.gcnpt_last_error()
    assert L.gcnpt_set_option(5, 0) == lib.E_INVALID
    old = lib.set_option(lib.OPT_WIDE_FORM, 0)
    try:
        assert L.gcnpt_get_option(lib.OPT_WIDE_FORM) == 0
        assert L.gcnpt_layer_fwd_needs_s_frag(5000, 1084, 200, lib.F32) == 0          # never: the refusal comes back
        lib.set_option(lib.OPT_WIDE_FORM, 1)
        assert L.gcnpt_get_option(lib.OPT_WIDE_FORM) == 1
        assert L.gcnpt_layer_fwd_needs_s_frag(5000, 360, 200, lib.BF16) == 1          # always
    finally:
        lib.set_option(lib.OPT_WIDE_FORM, old)
    assert L.gcnpt_get_option(lib.OPT_WIDE_FORM) == -1


def test_needs_s_frag_query():
    lib = _lib()
    q = lib.lib().gcnpt_layer_fwd_needs_s_frag
    assert q(5000, 360, 200, lib.BF16) == 0                 # the C2 headline shape
    assert q(5000, 1024, 200, lib.F32) == 0                 # the widest fp32 input the row tile holds at H = 200
    assert q(5000, 1040, 200, lib.F32) == 1 and q(5000, 1084, 200, lib.F32) == 1      # BERT-large + POS + NER
    assert q(5000, 1084, 200, lib.BF16) == 0                # bf16 operands hold about twice the width
    assert q(5000, 4096, 40, lib.BF16) == 1
    assert q(0, 1084, 200, lib.F32) == lib.E_INVALID and q(10, 0, 200, lib.F32) == lib.E_INVALID
    assert q(10, 1084, 0, lib.F32) == lib.E_INVALID and q(10, 1084, 200, 7) == lib.E_INVALID


@pytest.mark.parametrize("N", [5000, 30000], ids=["8_waves", "4_waves"])
@pytest.mark.parametrize("ct", [4, 2], ids=["fp32", "bf16"])
def test_needs_s_frag_matches_the_lds_count(N, ct):
    """The query is the dispatch's predicate: the one-shot launch's LDS bytes above 160 KiB (at the 4-wave batch size, B = 300
    sentences of 100 tokens, too), over widths around the limits, odd widths (element loads: 8-wave form) included.  Knowing no
    pointers, the query answers for rows of any alignment: the element-load shape is never smaller than the vector shapes."""
    lib = _lib()
    q = lib.lib().gcnpt_layer_fwd_needs_s_frag
    dt = lib.F32 if ct == 4 else lib.BF16
    lo, hi = (984, 1112) if ct == 4 else (1984, 2240)
    seen = set()
    for H in (40, 200, 300, 520):
        for din in list(range(lo, hi, 4)) + [lo + 1, hi - 3, 1085, 4096]:
            want = _refused(N, din, H, ct)
            assert q(N, din, H, dt) == int(want), (N, din, H, ct)
            seen.add(want)
    assert seen == {False, True}


_REFUSAL_CHILD = r"""
import ctypes, sys
sys.path.insert(0, sys.argv[1])
from gcn_over_pruned_trees_amd import _lib as lib
L = lib.lib()
fake = ctypes.c_void_p(1 << 20)
out = []
rc = L.gcnpt_layer_fwd(None, fake, lib.F32, fake, fake, fake, fake, fake, None, 4, 40, 1084, 200, fake, lib.F32, lib.F32, 0.0, 0, None, None)
out.append((rc, L.gcnpt_last_error().decode()))
ints = lambda v: (ctypes.c_int * 2)(*v)
ptrs = (ctypes.c_void_p * 2)(1 << 20, 1 << 20)
f32 = ints([lib.F32, lib.F32])
# the wide layer is the SECOND one: nothing of the first may be enqueued either
rc = L.gcnpt_layers_fwd(None, 2, fake, lib.F32, ptrs, ptrs, fake, fake, fake, None, 4, 40, ints([200, 1084]), ints([1084, 200]), ptrs, f32,
                        lib.F32, (ctypes.c_float * 2)(0.0, 0.0), (ctypes.c_uint64 * 2)(0, 0), None, None)
out.append((rc, L.gcnpt_last_error().decode()))
st = lib.Step()
st.n_layers, st.B, st.T, st.compute_dtype, st.parts = 2, 4, 40, lib.F32, lib.STEP_PACK | lib.STEP_FWD
for l, (d, h) in enumerate(((200, 1084), (1084, 200))):
    st.W[l] = st.bias[l] = st.w_fwd[l] = st.w_bwd[l] = st.out[l] = 1 << 20
    st.Din[l], st.H[l], st.out_dtype[l] = d, h, lib.F32
st.x, st.x_dtype, st.row_ptr, st.col_idx, st.ell = 1 << 20, lib.F32, 1 << 20, 1 << 20, 1 << 20
rc = L.gcnpt_layers_step(None, ctypes.byref(st))
out.append((rc, L.gcnpt_last_error().decode()))
print(repr(out))
"""


def test_wide_layer_without_s_frag_is_refused_without_a_gpu():
    """Argument validation comes before any HIP call: a layer that takes the wide form and has no S image gets GCNPT_E_INVALID and a
    message that names the query -- from gcnpt_layer_fwd, from gcnpt_layers_fwd when the wide layer is not the first one, and from
    gcnpt_layers_step before its weight pack.  The calls get fake device pointers, so they run in a child process that sees no GPU:
    should validation ever move behind a launch, the launch fails with a HIP error there instead of touching a card."""
    import ast
    import os
    import subprocess
    import sys
    from conftest import ROOT
    lib = _lib()
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, "-c", _REFUSAL_CHILD, ROOT], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    res = ast.literal_eval(r.stdout.strip().splitlines()[-1])
    assert len(res) == 3
    for (rc, msg), what in zip(res, ("layer_fwd", "layers_fwd", "layers_step")):
        assert rc == lib.E_INVALID and "s_frag" in msg and "needs_s_frag" in msg, (what, rc, msg)
    assert "layer 1" in res[1][1] and "layer 1" in res[2][1]
