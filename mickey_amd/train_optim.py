"""The tail of a training step on the HIP kernels: the finite checks, the gradient-norm clip, the skip of a bad step and the Adam update.

After its two backward passes the reference trainer (lib/models/MicKey/model.py:104-145) runs five isnan / isinf checks that each
synchronise with the host, torch.nn.utils.clip_grad_norm_, an isnan scan over every parameter's gradient that ends in one more
synchronisation, and torch.optim.Adam.step: several hundred small launches.  Here that is THREE launches (mk_optim_* in
mk_train_optim.hip) that follow a table of tensors in device memory: the sum of squares of every gradient per chunk in fp64, the sum
of the chunks in chunk order (a non-finite sum IS the finite check), and the clip and the Adam update of every chunk -- skipped on
the device when anything was not finite.  No host synchronisation, no atomics, results bit-identical from run to run.

    HipAdam(params, lr, betas, eps, weight_decay)     a torch.optim.Optimizer: param groups, StepLR, Lightning's self.optimizers()
        .step(closure=None)                           plain Adam, one launch
        .step_guarded(max_norm=None, also_finite=())  the three launches; returns the device tensor [ok, total_norm]
        .from_torch(opt)                              adopts the groups and the exp_avg / exp_avg_sq tensors of a torch.optim.Adam
        .state_dict() / .load_state_dict()            torch.optim.Adam's layout, either optimiser continues the other's checkpoint
    plan_chunks(numels, chunk_elems)                  the chunk map, a pure host function of the element counts
    adam_formula(...), guarded_step_formula(...)      the same maths in plain torch, any device / float dtype

Every step re-reads every parameter, gradient and state tensor and checks it on the host before anything is launched (the kernels
follow pointers from the table: a wrong row would be a GPU fault): fp32, on the optimiser's one device, non-overlapping and dense,
gradient and state in the parameter's memory order.  Violations raise ValueError naming the parameter's index, CPU tensors
MickeyHipError.  A parameter without a gradient is left out and its step count does not advance, as in torch.

Not covered: amsgrad, maximize, AdamW-style decoupled decay, half-precision parameters, sparse gradients, hipGraph capture of a
step (the table is uploaded from the host when a row changed), parameters on several devices.
"""
import math
import struct

import torch

from . import _native
from ._train_common import is_number, is_real

CHUNK_ELEMS = 4096   # elements of one chunk == mk_optim_chunk_elems() (tests/test_train_optim_cpu.py)
FLAG_NORM, FLAG_PARAM = _native.MK_OPTIM_NORM, _native.MK_OPTIM_PARAM
_ROW = struct.Struct("=" + "".join(code for _, code in _native.STRUCTS["mk_optim_row"]))   # mickey_hip.h's fields, in order
ROW_WORDS = _ROW.size // 8
_REFUSED = ("amsgrad", "maximize", "capturable", "differentiable", "decoupled_weight_decay")


# ---- the maths in plain torch (any device, any float dtype) -----------------------------------------------------------------
def adam_formula(p, g, m, v, step, lr, beta1, beta2, eps, weight_decay=0.0):
    """torch/optim/adam.py's single-tensor update restated: -> (p, m, v, step + 1), nothing modified.  L2 weight_decay is added to
    g first; with t = step + 1:  m = beta1 m + (1 - beta1) g,  v = beta2 v + (1 - beta2) g^2,
    p -= (lr / (1 - beta1^t)) m / (sqrt(v) / sqrt(1 - beta2^t) + eps)."""
    t = step + 1
    if weight_decay != 0:
        g = g + weight_decay * p
    m = beta1 * m + (1 - beta1) * g
    v = beta2 * v + (1 - beta2) * g * g
    step_size = lr / (1 - beta1 ** t)
    p = p - step_size * (m / (v.sqrt() / math.sqrt(1 - beta2 ** t) + eps))
    return p, m, v, t


def _per_tensor(hyper, n):
    hyper = [hyper] * n if isinstance(hyper, dict) else list(hyper)
    if len(hyper) != n:
        raise ValueError("guarded_step_formula: %d hyper-parameter sets for %d parameters" % (len(hyper), n))
    return hyper


def guarded_step_formula(params, grads, state, hyper, max_norm=None, also_finite=()):
    """model.py:104-145 restated for lists of tensors: the finite check of every gradient and of the also_finite tensors, the global
    L2 norm of the gradients (sums of squares taken in double), clip_grad_norm_'s coefficient min(1, max_norm / (norm + 1e-6)), and
    adam_formula per tensor -- or nothing at all when anything was not finite.  params[i], grads[i] (None: left out, as in torch)
    and state[i] = {"step", "exp_avg", "exp_avg_sq"} are updated in place (the gradient only when it is clipped); hyper is one dict
    {"lr", "betas", "eps", "weight_decay"} or one per parameter.  -> (ok, total_norm, clip_coef), Python numbers (this one reads
    its tensors)."""
    hyper = _per_tensor(hyper, len(params))
    live = [i for i, g in enumerate(grads) if g is not None]
    total = math.sqrt(sum(float(grads[i].detach().double().pow(2).sum()) for i in live)) if live else 0.0
    ok = math.isfinite(total) and all(bool(torch.isfinite(t).all()) for t in also_finite)
    coef = 1.0 if max_norm is None else min(1.0, max_norm / (total + 1e-6))
    if not ok:
        return False, total, coef
    with torch.no_grad():
        for i in live:
            h, s, g = hyper[i], state[i], grads[i]
            if coef < 1.0:
                g.mul_(coef)
            p, m, v, t = adam_formula(params[i], g, s["exp_avg"], s["exp_avg_sq"], s["step"], h["lr"], h["betas"][0], h["betas"][1],
                                      h["eps"], h.get("weight_decay", 0.0))
            params[i].copy_(p)
            s["exp_avg"].copy_(m)
            s["exp_avg_sq"].copy_(v)
            s["step"] = t
    return True, total, coef


# ---- the chunk map -----------------------------------------------------------------------------------------------------------
def plan_chunks(numels, chunk_elems=CHUNK_ELEMS):
    """-> int32 CPU tensor [chunks, 2]: for every chunk its tensor and its index inside that tensor, tensors in order, chunk i of a
    tensor covering elements [i chunk_elems, min((i + 1) chunk_elems, numel)).  A function of the element counts alone."""
    if any(n <= 0 for n in numels) or chunk_elems <= 0:
        raise ValueError("plan_chunks: element counts and chunk_elems must be positive, got %s, %s" % (list(numels), chunk_elems))
    counts = torch.tensor([-(-n // chunk_elems) for n in numels], dtype=torch.int64)
    rows = torch.repeat_interleave(torch.arange(len(numels), dtype=torch.int64), counts)
    first = torch.cumsum(counts, 0) - counts
    index = torch.arange(rows.numel(), dtype=torch.int64) - first[rows]
    return torch.stack((rows, index), 1).to(torch.int32)


def _nchunks(numel):
    return -(-numel // CHUNK_ELEMS)


# ---- host checks ------------------------------------------------------------------------------------------------------------
def _order(t):
    """(size, stride) of the dimensions that hold more than one element, innermost first"""
    return sorted(((st, n) for n, st in zip(t.shape, t.stride()) if n != 1))


def _dense(t):
    """non-overlapping and dense: some order of the dimensions walks t's memory without a gap"""
    if t.is_contiguous():
        return True
    span = 1
    for st, n in _order(t):
        if st != span:
            return False
        span *= n
    return True


def _same_order(a, b):
    """same shape assumed: equal strides in every dimension that holds more than one element"""
    return a.stride() == b.stride() or all(sa == sb for n, sa, sb in zip(a.shape, a.stride(), b.stride()) if n != 1)


def _plain(t, device):
    """the common case: a dense strided fp32 tensor in row-major order on `device` (a GPU: _check_device decided that)"""
    return torch.is_tensor(t) and t.dtype is torch.float32 and t.layout is torch.strided and t.device == device and t.is_contiguous()


def _check_layout(fn, what, t, like=None):
    """t may enter the table: an fp32, strided, non-empty dense tensor (with `like`, of its shape and memory order)"""
    if not torch.is_tensor(t):
        raise ValueError("%s: %s must be a tensor, got %s" % (fn, what, type(t).__name__))
    if t.layout != torch.strided:
        raise ValueError("%s: %s is %s; sparse tensors are not covered" % (fn, what, t.layout))
    if t.dtype != torch.float32:
        raise ValueError("%s: %s must be float32, got %s (half-precision parameters are not covered)" % (fn, what, t.dtype))
    if t.numel() == 0:
        raise ValueError("%s: %s is empty %s" % (fn, what, tuple(t.shape)))
    if not _dense(t):
        raise ValueError("%s: %s must be non-overlapping and dense, got shape %s with strides %s" % (fn, what, tuple(t.shape), t.stride()))
    if like is not None:
        if t.shape != like.shape:
            raise ValueError("%s: %s has shape %s, its parameter %s" % (fn, what, tuple(t.shape), tuple(like.shape)))
        if not _same_order(t, like):
            raise ValueError("%s: %s must have the strides of its parameter, got %s against %s" % (fn, what, t.stride(), like.stride()))


def _check_device(fn, what, t, device):
    """t is on a GPU (else MickeyHipError) -- on `device` unless that is None; checked after every layout of its row -> t.device"""
    if not t.is_cuda:
        raise _native.MickeyHipError("%s: %s is on %s; needs device tensors, mickey_amd has no CPU fallback" % (fn, what, t.device))
    if device is not None and t.device != device:
        raise ValueError("%s: %s is on %s, the optimiser's tensors are on %s" % (fn, what, t.device, device))
    return t.device


def _check_hyper(fn, group):
    lr, betas, eps, wd = group["lr"], group["betas"], group["eps"], group["weight_decay"]
    if not is_number(lr):
        raise ValueError("%s: lr must be a finite non-negative number, got %r" % (fn, lr))
    if not (isinstance(betas, (tuple, list)) and len(betas) == 2 and all(is_real(b) and 0.0 <= b < 1.0 for b in betas)):
        raise ValueError("%s: betas must be two numbers in [0, 1), got %r" % (fn, betas))
    if not is_number(eps):
        raise ValueError("%s: eps must be a finite non-negative number, got %r" % (fn, eps))
    if not is_number(wd):
        raise ValueError("%s: weight_decay must be a finite non-negative number, got %r" % (fn, wd))
    for key in _REFUSED:
        if group.get(key):
            raise ValueError("%s: %s is not covered" % (fn, key))


# ---- the optimiser -----------------------------------------------------------------------------------------------------------
class HipAdam(torch.optim.Optimizer):
    """torch.optim.Adam (L2 weight_decay) on mk_optim_*.  Per parameter the state holds exp_avg, exp_avg_sq (the parameter's shape
    and memory order) and step: fp32 device cells, one per chunk of the tensor and all equal (each workgroup owns its cell), so
    that a step skipped on the device costs no host synchronisation.  state_dict() turns them into torch's 0-d CPU tensors."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0):
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
        _check_hyper("HipAdam", defaults)
        super().__init__(params, defaults)
        self._table = None       # (the rows' bytes, the device tensor) of the last upload
        self._map = None         # (the element counts, the device tensor) of the last upload
        self._partials = None
        self._go = None          # the state block of a plain step: { 1, 0, 1, 0 }

    # -- adoption and checkpoints
    @classmethod
    def from_torch(cls, opt):
        """A HipAdam over the param groups of the torch.optim.Adam `opt` (lr, betas, eps, weight_decay and any extra keys, e.g.
        a scheduler's initial_lr) that adopts the very exp_avg / exp_avg_sq tensors of its state and continues at its step counts.
        amsgrad, maximize, capturable, differentiable and decoupled_weight_decay raise ValueError."""
        if not isinstance(opt, torch.optim.Adam):
            raise ValueError("HipAdam.from_torch: needs a torch.optim.Adam, got %s" % type(opt).__name__)
        for group in opt.param_groups:
            _check_hyper("HipAdam.from_torch", group)
        skip = set(_REFUSED) | {"foreach", "fused"}
        new = cls([{k: v for k, v in group.items() if k not in skip} for group in opt.param_groups])
        for p, s in opt.state.items():
            if len(s):
                new.state[p] = {"step": new._cells(p, float(s["step"])), "exp_avg": s["exp_avg"], "exp_avg_sq": s["exp_avg_sq"]}
        return new

    @staticmethod
    def _cells(p, value):
        return torch.full((_nchunks(p.numel()),), value, dtype=torch.float32, device=p.device)

    def state_dict(self):
        """torch.optim.Adam's layout: exp_avg and exp_avg_sq per parameter, step as a 0-d fp32 CPU tensor.  Reading the step counts
        is the one place of this class that synchronises with the device (one copy for all of them)."""
        sd = super().state_dict()
        entries = [s for s in sd["state"].values() if "step" in s]
        if entries:
            steps = torch.stack([s["step"][0] for s in entries]).cpu()
            sd["state"] = {k: dict(s) for k, s in sd["state"].items()}
            for s, value in zip([s for s in sd["state"].values() if "step" in s], steps):
                s["step"] = value.clone()
        for group in sd["param_groups"]:   # what torch.optim.Adam writes beside ours
            for key, value in (("amsgrad", False), ("maximize", False), ("foreach", None), ("capturable", False),
                               ("differentiable", False), ("fused", None), ("decoupled_weight_decay", False)):
                group.setdefault(key, value)
        return sd

    def load_state_dict(self, state_dict):
        """Takes a state_dict of this class or of torch.optim.Adam."""
        for group in state_dict["param_groups"]:
            _check_hyper("HipAdam.load_state_dict", {**self.defaults, **group})
        super().load_state_dict(state_dict)
        for p, s in self.state.items():
            if "step" in s:
                s["step"] = self._cells(p, float(s["step"]))   # (a CPU scalar: torch keeps `step` where the checkpoint had it)
        self._table = None

    # -- one step
    def _gather(self, fn, also_finite):
        """Every host check, before any launch -> (rows, keep, numels, param rows, device): the table's rows as tuples, every tensor
        they point to, the element count of every row, and how many of the rows are parameters (they come first)."""
        rows, keep, numels = [], [], []
        f32, strided = torch.float32, torch.strided
        device = None
        index = -1
        for group in self.param_groups:
            _check_hyper(fn, group)
            lr, (b1, b2), eps, wd = float(group["lr"]), group["betas"], float(group["eps"]), float(group["weight_decay"])
            for p in group["params"]:
                index += 1
                g = p.grad
                if g is None:
                    continue
                s = self.state[p]
                if len(s) == 0:
                    s["step"] = self._cells(p, 0.0)
                    s["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    s["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                m, v, step = s["exp_avg"], s["exp_avg_sq"], s["step"]
                n = p.numel()
                # the common case is decided cheaply (a few hundred tensors are looked at every step); anything else goes through
                # the checks that accept it (another dense memory order) or say what is wrong
                try:
                    plain = (p.dtype is f32 and g.dtype is f32 and m.dtype is f32 and v.dtype is f32 and step.dtype is f32
                             and g.layout is strided and n > 0 and p.is_contiguous() and g.is_contiguous() and m.is_contiguous()
                             and v.is_contiguous() and step.is_contiguous() and g.shape == p.shape and m.shape == p.shape
                             and v.shape == p.shape and step.numel() == _nchunks(n) and p.device == device and g.device == device
                             and m.device == device and v.device == device and step.device == device)
                except AttributeError:   # something in the state is no tensor: the checks below say what
                    plain = False
                if not plain:
                    what = "parameter %d" % index
                    _check_layout(fn, what, p)
                    _check_layout(fn, "the gradient of " + what, g, like=p)
                    _check_layout(fn, "exp_avg of " + what, m, like=p)
                    _check_layout(fn, "exp_avg_sq of " + what, v, like=p)
                    device = _check_device(fn, what, p, device)
                    _check_device(fn, "the gradient of " + what, g, device)
                    _check_device(fn, "exp_avg of " + what, m, device)
                    _check_device(fn, "exp_avg_sq of " + what, v, device)
                    if not (torch.is_tensor(step) and _plain(step, device) and step.numel() == _nchunks(n)):
                        raise ValueError("%s: the step cells of parameter %d are not the %d fp32 device cells this class made"
                                         % (fn, index, _nchunks(n)))
                rows.append((p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), step.data_ptr(), n, lr, float(b1), float(b2), eps,
                             wd, FLAG_NORM | FLAG_PARAM))
                keep.append((p, g, m, v, step))
                numels.append(n)
        nparams = len(rows)
        for j, t in enumerate(also_finite):
            what = "also_finite[%d]" % j
            _check_layout(fn, what, t)
            device = _check_device(fn, what, t, device)
            rows.append((0, t.data_ptr(), 0, 0, 0, t.numel(), 0.0, 0.0, 0.0, 0.0, 0.0, 0))
            keep.append(t)
            numels.append(t.numel())
        return rows, keep, numels, nparams, device

    @staticmethod
    def _upload(cpu, device):
        """through a fresh pinned tensor: torch's host allocator keeps it alive until the copy has run"""
        return cpu.pin_memory().to(device, non_blocking=True)

    def _tables(self, rows, numels, device):
        """the device table and chunk map for these rows: uploaded again only when a row (a pointer, an lr ...) or a count changed"""
        blob = b"".join(_ROW.pack(*r) for r in rows)
        if self._table is None or self._table[0] != blob or self._table[1].device != device:
            self._table = (blob, self._upload(torch.frombuffer(bytearray(blob), dtype=torch.int64), device))
        numels = tuple(numels)
        if self._map is None or self._map[0] != numels or self._map[1].device != device:
            self._map = (numels, self._upload(plan_chunks(numels), device))
        return self._table[1], self._map[1]

    def _run(self, fn, guarded, max_norm, also_finite):
        rows, keep, numels, nparams, device = self._gather(fn, also_finite)
        if not rows:
            return None
        chunks = sum(_nchunks(n) for n in numels)
        param_chunks = sum(_nchunks(n) for n in numels[:nparams])
        with torch.cuda.device(device):
            table, cmap = self._tables(rows, numels, device)
            stream = _native.stream()
            if guarded:
                if self._partials is None or self._partials.numel() < 2 * chunks or self._partials.device != device:
                    self._partials = torch.empty((2 * chunks,), dtype=torch.float64, device=device)
                state = torch.empty((4,), dtype=torch.float32, device=device)
                _native.call("mk_optim_grad_stats", table.data_ptr(), len(rows), cmap.data_ptr(), chunks, self._partials.data_ptr(), stream)
                _native.call("mk_optim_reduce", self._partials.data_ptr(), chunks, -1.0 if max_norm is None else float(max_norm),
                             state.data_ptr(), stream)
            else:
                if self._go is None or self._go.device != device:
                    self._go = torch.tensor([1.0, 0.0, 1.0, 0.0], dtype=torch.float32, device=device)
                state = self._go
            if param_chunks:
                _native.call("mk_optim_adam", table.data_ptr(), len(rows), cmap.data_ptr(), param_chunks, state.data_ptr(), stream)
        del keep   # (referenced until here: every launch that follows the table is enqueued)
        return state

    @torch.no_grad()
    def step(self, closure=None):
        """Plain Adam: one launch (mk_optim_adam) over every parameter that has a gradient."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        self._run("HipAdam.step", False, None, ())
        return loss

    @torch.no_grad()
    def step_guarded(self, max_norm=None, also_finite=()):
        """Three launches: when every gradient and every tensor of also_finite (fp32 device tensors) is free of NaN and Inf, clip the
        gradients to the global L2 norm max_norm as clip_grad_norm_ does (None: no clipping; the .grad tensors are rewritten only when
        the norm exceeds it) and take the Adam step; else change nothing at all.  Returns the fp32 device tensor [ok, total_norm]
        (ok 1 or 0; the norm before clipping) and never reads it: whether to call .item() is the caller's choice.  None when there
        is neither a gradient nor an also_finite tensor."""
        if max_norm is not None and not is_number(max_norm):
            raise ValueError("HipAdam.step_guarded: max_norm must be None or a finite non-negative number, got %r" % (max_norm,))
        self._opt_called = True   # what torch's lr schedulers look at to tell that the optimiser stepped before they did
        state = self._run("HipAdam.step_guarded", True, max_norm, tuple(also_finite))
        return None if state is None else state[:2]
