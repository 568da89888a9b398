"""
The last three lines of the reference's training step (train.py:225-227):

    torch.nn.utils.clip_grad_norm_(trainer.model.parameters(), opt['max_grad_norm'])
    trainer.optimizer.step()
    trainer.optimizer.zero_grad()

as ONE call, `optimizer.step()`, over gcnpt_optim_step (csrc/optim_kernels.hip): at most four launches, no host sync, no sort, capturable
with the forward and backward in one hipGraph.  Dense gradients are cleared by the update launch; a row-sparse word-table gradient
(opt['gcn_sparse_emb_grad']: p.grad is an uncoalesced sparse COO tensor of token ids and rows) updates only the rows the batch used and is
set to None afterwards.  The parameters are taken WHERE THEY LIVE: nothing is flattened or re-homed, and the device pointers of p.data and
p.grad are read at every step(), so buffers moved by .to(), an EMA swap or nn.LSTM.flatten_parameters() are followed.

get_optimizer mirrors utils/torch_utils.py:93-106 for 'sgd' and 'adagrad' / 'myadagrad' (MyAdagrad, accumulator initialised to 0.1); the
other names stay torch's.
"""
import torch

from . import _lib

KINDS = {"sgd": _lib.OPTIM_SGD, "adagrad": _lib.OPTIM_ADAGRAD, "myadagrad": _lib.OPTIM_ADAGRAD}


class NativeOptimizer(object):
    """clip_grad_norm_ + SGD / MyAdagrad + zero_grad over gcnpt_optim_step.  param_groups = [{'params', 'lr'}] as torch's optimizers have
    it, so the reference's torch_utils.change_lr / Trainer.update_lr work unchanged; the learning rate is mirrored into the one-element
    device tensor `lr_dev` that the kernels read (by step(), or by sync_lr(); inside a graph capture step() leaves lr_dev alone, so a
    replayed step follows whatever sync_lr() or the caller wrote into it between replays).  last_norm / last_coef: the pre-clip gradient
    norm and the clip coefficient of the latest step, as device tensors (never read here)."""

    def __init__(self, kind, parameters, lr, max_grad_norm=0.0, init_accu_value=0.1):
        if kind not in (_lib.OPTIM_SGD, _lib.OPTIM_ADAGRAD):
            raise ValueError("NativeOptimizer: unknown kind %r" % (kind,))
        params = list(parameters)
        if not params:
            raise ValueError("NativeOptimizer: no parameters")
        for p in params:
            self._check_param(p)
        if len({p.device for p in params}) != 1:
            raise ValueError("NativeOptimizer: the parameters live on several devices")
        self.kind = kind
        self.max_grad_norm = float(max_grad_norm or 0.0)
        self.param_groups = [{"params": params, "lr": float(lr)}]
        dev = params[0].device
        self.state = [torch.full_like(p.data, init_accu_value, memory_format=torch.contiguous_format) if kind == _lib.OPTIM_ADAGRAD else None
                      for p in params]
        self.lr_dev = torch.full((1,), float(lr), dtype=torch.float32, device=dev)
        self._lr_mirrored = float(lr)
        n = int(_lib.lib().gcnpt_optim_partials_floats(len(params), len(params)))
        self._partials = torch.zeros(n, dtype=torch.float32, device=dev)
        self.last_norm, self.last_coef = self._partials[_lib.OPTIM_NORM], self._partials[_lib.OPTIM_COEF]
        self._owner = {}           # parameter index -> int32 [V] workspace, all -1 between steps
        self._scratch = {}         # parameter index -> int32 [>= n_rows]

    @staticmethod
    def _check_param(p):
        if not torch.is_tensor(p):
            raise TypeError("NativeOptimizer: parameters must be tensors, got %s" % type(p))
        if not p.is_cuda:
            raise TypeError("NativeOptimizer runs on the GPU only (parameter on %s); there is no CPU path" % p.device)
        if p.dtype != torch.float32:
            raise TypeError("NativeOptimizer updates float32 parameters, got %s" % p.dtype)

    def sync_lr(self):
        """Mirrors param_groups[0]['lr'] into lr_dev (one fill, no sync).  Call it between replays of a captured step after update_lr."""
        lr = float(self.param_groups[0]["lr"])
        if lr != self._lr_mirrored:
            self.lr_dev.fill_(lr)
            self._lr_mirrored = lr

    def zero_grad(self, set_to_none=False):
        for p in self.param_groups[0]["params"]:
            if p.grad is None:
                continue
            if set_to_none or p.grad.is_sparse:
                p.grad = None
            else:
                p.grad.detach_()
                p.grad.zero_()

    def state_dict(self):
        return {"kind": self.kind, "lr": float(self.param_groups[0]["lr"]), "max_grad_norm": self.max_grad_norm,
                "sums": [s.clone() if s is not None else None for s in self.state]}

    def load_state_dict(self, sd):
        if sd["kind"] != self.kind or len(sd["sums"]) != len(self.state):
            raise ValueError("NativeOptimizer.load_state_dict: the state is of another optimizer (kind %r, %d tensors)" % (sd["kind"], len(sd["sums"])))
        self.param_groups[0]["lr"] = float(sd["lr"])
        self.max_grad_norm = float(sd["max_grad_norm"])
        for mine, theirs in zip(self.state, sd["sums"]):
            if mine is not None:
                if tuple(mine.shape) != tuple(theirs.shape):
                    raise ValueError("NativeOptimizer.load_state_dict: a sum of shape %s for a parameter of shape %s" % (tuple(theirs.shape), tuple(mine.shape)))
                mine.copy_(theirs)

    def _workspace(self, i, V, n_rows, dev):
        owner = self._owner.get(i)
        if owner is None or owner.numel() != V or owner.device != dev:
            owner = self._owner[i] = torch.full((V,), -1, dtype=torch.int32, device=dev)
        scratch = self._scratch.get(i)
        if scratch is None or scratch.numel() < n_rows or scratch.device != dev:
            scratch = self._scratch[i] = torch.empty((max(n_rows, 1),), dtype=torch.int32, device=dev)
        return owner, scratch

    def step(self):
        """clip + update + clear.  Returns nothing and never synchronises."""
        params = self.param_groups[0]["params"]
        if not torch.cuda.is_current_stream_capturing():
            self.sync_lr()
        tensors, tables, keep, sparse, copied = [], [], [], [], []
        for i, p in enumerate(params):
            g = p.grad
            if g is None:
                continue
            w = p.data
            self._check_param(w)
            if not w.is_contiguous():
                raise RuntimeError("NativeOptimizer: parameter %d is not contiguous" % i)
            st = self.state[i]
            if st is not None and st.device != w.device:
                st = self.state[i] = st.to(w.device)
            if g.is_sparse:
                if g.sparse_dim() != 1 or w.dim() != 2 or tuple(g.shape) != tuple(w.shape):
                    raise RuntimeError("NativeOptimizer: parameter %d: a sparse gradient must be row-sparse over a [V,E] table" % i)
                ids, rows = g._indices()[0], g._values()
                if rows.dtype != torch.float32 or not rows.is_contiguous():
                    rows = rows.to(torch.float32).contiguous()
                if not ids.is_contiguous():
                    ids = ids.contiguous()
                n_rows = int(ids.shape[0])
                owner, scratch = self._workspace(i, int(w.shape[0]), n_rows, w.device)
                keep += [ids, rows]
                tables.append((w.data_ptr(), st.data_ptr() if st is not None else None, ids.data_ptr(), rows.data_ptr(), owner.data_ptr(),
                               scratch.data_ptr(), int(w.shape[0]), int(w.shape[1]), n_rows, 0))
                sparse.append(p)
            else:
                if not g.is_cuda:
                    raise TypeError("NativeOptimizer runs on the GPU only (gradient on %s)" % g.device)
                gc = g
                if g.dtype != torch.float32 or not g.is_contiguous():
                    gc = g.to(torch.float32).contiguous()            # copied once; the original is cleared below
                    copied.append(g)
                    keep.append(gc)
                if w.numel() == 0:
                    continue
                tensors.append((w.data_ptr(), gc.data_ptr(), st.data_ptr() if st is not None else None, w.numel()))
        c_tensors = (_lib.OptimTensor * max(len(tensors), 1))(*tensors)
        c_tables = (_lib.OptimTable * max(len(tables), 1))(*tables)
        _lib.check(_lib.lib().gcnpt_optim_step(_lib.stream(), self.kind, c_tensors, len(tensors), c_tables, len(tables), self.max_grad_norm,
                                               self._lr_mirrored, self.lr_dev.data_ptr(), 1, self._partials.data_ptr()))
        for g in copied:
            g.zero_()
        for p in sparse:
            p.grad = None
        del keep


def get_optimizer(name, parameters, lr, max_grad_norm=0.0):
    """utils/torch_utils.py:93-106 for the optimizers the native step knows: 'sgd' (torch.optim.SGD, no weight decay) and 'adagrad' /
    'myadagrad' (MyAdagrad, init_accu_value = 0.1, lr_decay = 0, weight_decay = 0), with clip_grad_norm_(max_grad_norm) folded into
    step().  'adam', 'adamax' and 'adadelta' stay torch's."""
    if name not in KINDS:
        raise ValueError("optimizer %r has no native step: only %s do; %r stays torch's (utils/torch_utils.get_optimizer)"
                         % (name, ", ".join(sorted(KINDS)), name))
    return NativeOptimizer(KINDS[name], parameters, lr, max_grad_norm)
