"""CPU-side checks of the native optimizer step (include/gcnpt.h gcnpt_optim_step, gcn_over_pruned_trees_amd.optim): the symbols are
exported and bound, the ctypes mirrors of the descriptor structs lay out as the header declares them, argument validation returns
GCNPT_E_INVALID with a text that names the entry point before anything is launched, the Python surface refuses what it cannot do, and
the float64 restatement the GPU tests compare against (tests/optim_ref.py) reproduces what the reference's own loop recorded
(tests/golden/train_trajectory.npz).  No compute is launched here."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import optim_ref
from conftest import ROOT, load_golden
from gcn_over_pruned_trees_amd import _lib


def test_optim_symbols_exported_and_bound():
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("gcnpt_optim_step", "gcnpt_optim_partials_floats"):
        assert name in _lib.SIGNATURES, name
        assert hasattr(handle, name), name
    assert _lib.lib().gcnpt_abi_version() == 7                      # nothing existing changed
    L = _lib.lib()
    assert L.gcnpt_optim_partials_floats(0, 0) == 2                 # host-only arithmetic: the norm and coef slots alone
    assert L.gcnpt_optim_partials_floats(1, 0) > 2 and L.gcnpt_optim_partials_floats(65, 0) > L.gcnpt_optim_partials_floats(64, 0)
    assert L.gcnpt_optim_partials_floats(1, 9) > L.gcnpt_optim_partials_floats(1, 8)


def _header_struct(name):
    """[(field, C type)] of `typedef struct ... { ... } name;` in include/gcnpt.h."""
    text = open(os.path.join(ROOT, "include", "gcnpt.h")).read()
    body = re.search(r"typedef struct \w+ \{([^}]*)\} %s;" % name, text).group(1)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        m = re.match(r"((?:const )?(?:long long|int64_t|int32_t|float|int))\s*(\**)\s*([\w, ]+)$", decl)
        base = m.group(1) + m.group(2)
        fields += [(f.strip(), base) for f in m.group(3).split(",")]
    return fields


@pytest.mark.parametrize("cname,mirror,size", [("gcnpt_optim_tensor_t", _lib.OptimTensor, 32), ("gcnpt_optim_table_t", _lib.OptimTable, 64)])
def test_optim_struct_mirrors_match_the_header(cname, mirror, size):
    fields = _header_struct(cname)
    assert [f for f, _ in fields] == [f for f, _ in mirror._fields_]
    off = 0
    for (name, ctype), (_, mtype) in zip(fields, mirror._fields_):
        want = ctypes.c_void_p if ctype.endswith("*") else {"long long": ctypes.c_longlong, "int": ctypes.c_int}[ctype]
        assert mtype is want, (name, ctype)
        width = ctypes.sizeof(want)
        off = (off + width - 1) // width * width                   # natural alignment, as the C ABI lays a struct out
        assert getattr(mirror, name).offset == off, name
        off += width
    assert ctypes.sizeof(mirror) == (off + 7) // 8 * 8 == size
    assert (_lib.OPTIM_SGD, _lib.OPTIM_ADAGRAD, _lib.OPTIM_NORM, _lib.OPTIM_COEF) == (0, 1, 0, 1)
    text = open(os.path.join(ROOT, "include", "gcnpt.h")).read()
    assert "#define GCNPT_OPTIM_TENSORS_PER_LAUNCH %d\n" % _lib.OPTIM_TENSORS_PER_LAUNCH in text
    assert "#define GCNPT_OPTIM_TABLES_PER_LAUNCH %d\n" % _lib.OPTIM_TABLES_PER_LAUNCH in text


def _call(p, **kw):
    """gcnpt_optim_step with one valid-looking tensor and table (host buffers: never launched, one argument is always bad)."""
    a = dict(kind=_lib.OPTIM_SGD, w=p, g=p, state=p, n=5, n_tensors=1, tw=p, tstate=p, ids=p, rows=p, owner=p, scratch=p, V=7, E=3, n_rows=4,
             n_tables=1, max_norm=5.0, lr=0.1, lr_dev=None, partials=p, tensors=True, tables=True)
    a.update(kw)
    tensors = (_lib.OptimTensor * 1)((a["w"], a["g"], a["state"], a["n"]))
    tables = (_lib.OptimTable * 1)((a["tw"], a["tstate"], a["ids"], a["rows"], a["owner"], a["scratch"], a["V"], a["E"], a["n_rows"], 0))
    return _lib.lib().gcnpt_optim_step(None, a["kind"], tensors if a["tensors"] else None, a["n_tensors"], tables if a["tables"] else None,
                                       a["n_tables"], a["max_norm"], a["lr"], a["lr_dev"], 1, a["partials"])


BAD = (dict(w=None), dict(g=None), dict(n=0), dict(n=-3), dict(kind=2), dict(kind=-1), dict(kind=_lib.OPTIM_ADAGRAD, state=None),
       dict(kind=_lib.OPTIM_ADAGRAD, tstate=None), dict(E=0), dict(E=-2), dict(V=0), dict(n_tensors=-1), dict(n_tables=-1), dict(n_rows=-1),
       dict(lr=float("nan")), dict(lr=-0.1), dict(max_norm=float("nan")), dict(max_norm=-1.0), dict(partials=None), dict(tw=None),
       dict(ids=None), dict(rows=None), dict(owner=None), dict(scratch=None), dict(tensors=False), dict(tables=False))


def test_optim_argument_validation_needs_no_gpu():
    L = _lib.lib()
    buf = ctypes.create_string_buffer(512)
    p = (ctypes.addressof(buf) + 15) // 16 * 16
    for bad in BAD:
        assert _call(p, **bad) == _lib.E_INVALID, bad
        assert L.gcnpt_last_error().startswith(b"gcnpt_optim_step:"), (bad, L.gcnpt_last_error())
    assert _call(p, n=0) == _lib.E_INVALID and b"positive" in L.gcnpt_last_error()
    assert _call(p, kind=7) == _lib.E_INVALID and b"kind" in L.gcnpt_last_error()
    assert _call(p, kind=_lib.OPTIM_ADAGRAD, state=None) == _lib.E_INVALID and b"state" in L.gcnpt_last_error()
    assert _call(p, lr=float("nan")) == _lib.E_INVALID and b"lr" in L.gcnpt_last_error()
    assert _call(p, max_norm=-1.0) == _lib.E_INVALID and b"max_norm" in L.gcnpt_last_error()
    assert _call(p, w=p + 2) == _lib.E_INVALID and b"aligned" in L.gcnpt_last_error()


def test_optim_python_surface_refusals():
    from gcn_over_pruned_trees_amd import optim
    w = torch.nn.Parameter(torch.zeros(3, 4))
    for name in ("adam", "adamax", "adadelta"):
        with pytest.raises(ValueError, match="torch's"):
            optim.get_optimizer(name, [w], 0.1, 5.0)
    for name in ("sgd", "adagrad", "myadagrad"):
        with pytest.raises(TypeError):                                 # CPU parameters: there is no CPU path
            optim.get_optimizer(name, [w], 0.1, 5.0)


def test_restatement_matches_the_reference_recording():
    """tests/optim_ref.py in float64 against the fp32 arithmetic the reference's loop recorded: within 1e-6 * max|value|."""
    import json
    g = load_golden("train_trajectory.npz")
    cases, s = json.loads(str(g["cases"])), int(g["probe_step"])
    close = lambda got, want: float((got - torch.from_numpy(want).double()).abs().max()) <= 1e-6 * float(np.abs(want).max())  # noqa: E731
    # MyAdagrad, no clipping at this step
    c = cases["adagrad"]
    norm = float(g["adagrad:norms"][s])
    assert norm < c["max_grad_norm"]
    w, st = optim_ref.update(optim_ref.ADAGRAD, g["adagrad:probe_before"], g["adagrad:probe_grad"], g["adagrad:probe_sum_before"], c["lr"],
                             optim_ref.clip_coef(norm, c["max_grad_norm"]))
    assert close(w, g["adagrad:probe_after"]) and close(st, g["adagrad:probe_sum_after"])
    assert float(np.abs(g["adagrad:probe_after"] - g["adagrad:probe_before"]).max()) > 1e-3          # (the step moved something)
    # SGD under a clip that bites: the coefficient comes from the recorded pre-clip norm of all parameters
    c = cases["sgd_clip"]
    norm = float(g["sgd_clip:norms"][s])
    coef = optim_ref.clip_coef(norm, c["max_grad_norm"])
    assert norm > c["max_grad_norm"] and coef < 1.0
    w, _ = optim_ref.update(optim_ref.SGD, g["sgd_clip:probe_before"], g["sgd_clip:probe_grad"], None, c["lr"], coef)
    assert close(w, g["sgd_clip:probe_after"])
    assert not close(optim_ref.update(optim_ref.SGD, g["sgd_clip:probe_before"], g["sgd_clip:probe_grad"], None, c["lr"], 1.0)[0],
                     g["sgd_clip:probe_after"])                                                      # (and the clip is visible at this bound)
    # the property the three cases were chosen for
    for case, bites in (("sgd", False), ("sgd_clip", True), ("adagrad", False)):
        assert all((n > cases[case]["max_grad_norm"]) == bites for n in g[case + ":norms"]), case
    # coalescing and the norm of a row-sparse gradient
    ids, rows = torch.tensor([3, 1, 3, -1, 5, 3]), torch.arange(12, dtype=torch.float32).reshape(6, 2)
    G = optim_ref.coalesce(ids, rows, 5)
    assert torch.equal(G[3], rows[0].double() + rows[2] + rows[5]) and torch.equal(G[1], rows[1].double()) and float(G[[0, 2, 4]].abs().sum()) == 0
    out = optim_ref.step(optim_ref.SGD, [(torch.ones(3), torch.full((3,), 2.0), None)], [(torch.ones(5, 2), None, ids, rows)], 0.5, 1.0)
    assert abs(out["norm"] - float(torch.sqrt(12.0 + (G ** 2).sum()))) < 1e-12 and abs(out["coef"] - 1.0 / (out["norm"] + 1e-6)) < 1e-15
    assert torch.allclose(out["tables"][0][0], 1.0 - 0.5 * out["coef"] * G, rtol=0, atol=1e-15)
