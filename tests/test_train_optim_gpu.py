"""mickey_amd.train_optim on the GPU: HipAdam.step_guarded / step against guarded_step_formula in fp64 on the same fp32 gradients.

Tensor set (E = mk_optim_chunk_elems()): element counts 1 (a 0-d parameter, as dustbin_score is), 3, 4, 5, E - 1, E, E + 1, 2 E + 3, a
4-D channels_last weight whose gradient has its strides, a parameter without a gradient, and four tensors of E + 5 elements in which
p, g, m, v in turn start 4 bytes past a 16-byte boundary (the 16-byte path falls back per tensor).  Every p, g, m, v lies in a
tests/helpers/guarded.py window that is checked after every step.  Two param groups with different lr, the second with weight decay.

Five steps: clipped (norm > max_norm), a NaN gradient, an Inf gradient, a NaN in an also_finite tensor only, unclipped.  The three
bad steps must leave p, g, m, v and step bit-identical with ok == 0; the good step after them shows that the count did not move.
The gradients are drawn independently of the parameters, so that errors do not feed back.

Bound, per tensor: e = max |x - x64| / max |x64| <= max(2 e_torch32, 2e-6), with e_torch32 what torch.optim.Adam (fp32) +
clip_grad_norm_ gives on the same GPU in the same test, for exp_avg, exp_avg_sq and the UPDATE p_new - p_old (in fp64 from the fp32
values; on p itself a step of lr would be invisible).  Parameters are of the order of lr (1e-3), so the final rounding of p is
far below the update (2^-24 |p| against lr).  total_norm: within 2^-23 relative of the fp64 norm (fp64 accumulation, one rounding).
Every measured figure goes to profiles/train_optim_parity.txt.
"""
import copy
import os

import pytest
import torch
from torch import nn

from tests.helpers.guarded import bits, guarded

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLOOR = 2e-6
RESULTS = []
MAX_NORM = 5.0
STEPS = (("clipped", 1.0), ("nan", 1.0), ("inf", 1.0), ("also_nan", 1.0), ("unclipped", 0.01))
GROUPS = (dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.0), dict(lr=2e-3, betas=(0.8, 0.99), eps=1e-8, weight_decay=0.01))


@pytest.fixture(scope="module")
def to():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from mickey_amd import train_optim
    yield train_optim
    if RESULTS:
        try:
            with open(os.path.join(ROOT, "profiles", "train_optim_parity.txt"), "w") as f:
                f.write("# tests/test_train_optim_gpu.py: max |x - x64| / max |x64| against guarded_step_formula of mickey_amd.train_optim in fp64 on the same fp32 gradients;\n")
                f.write("# bound: max(2 * e_torch32, 2e-6), e_torch32 = torch.optim.Adam (fp32) + clip_grad_norm_ on the same GPU; upd = p_new - p_old\n")
                f.write("# one line per case: tensor e_hip/e_torch32 for each of its tensors, every figure of the run\n")
                cases = {}
                for case, name, e_hip, e_t in RESULTS:
                    cases.setdefault(case, []).append("%s %.1e/%.1e" % (name, e_hip, e_t))
                for case, figs in cases.items():
                    f.write("%s: %s\n" % (case, "  ".join(figs)))
        except OSError:
            pass   # a read-only checkout: the assertions have run all the same


def _err(a, ref):
    return float((a.double() - ref).abs().max() / ref.abs().max())


def _bound(case, name, got, ref, t32):
    e_hip, e_t = _err(got, ref), _err(t32, ref)
    RESULTS.append((case, name, e_hip, e_t))
    print("%s %s: e_hip %.3e  e_torch32 %.3e  bound %.3e" % (case, name, e_hip, e_t, max(2 * e_t, FLOOR)))
    return e_hip <= max(2 * e_t, FLOOR), (case, name, e_hip, e_t)


# ---- the tensor set ------------------------------------------------------------------------------------------------------------------
def _specs(E):
    """(name, shape, channels_last, which of p g m v starts 4 bytes past a 16-byte boundary, has a gradient, group)"""
    specs = [("n1", (), False, None, True, 0), ("n3", (3,), False, None, True, 1), ("n4", (2, 2), False, None, True, 0),
             ("n5", (5,), False, None, True, 1), ("E-1", (E - 1,), False, None, True, 0), ("E", (E // 64, 64), False, None, True, 1),
             ("E+1", (E + 1,), False, None, True, 0), ("2E+3", (2 * E + 3,), False, None, True, 1),
             ("cl", (6, 4, 3, 3), True, None, True, 0), ("nograd", (7,), False, None, False, 1)]
    specs += [("mis_" + which, (E + 5,), False, which, True, i % 2) for i, which in enumerate("pgmv")]
    return specs


class Window:
    """one fp32 tensor of `shape` inside a guarded window; off = 1: it starts one element past the window's 256-byte aligned start"""

    def __init__(self, shape, cl, off, dev, value=None):
        n = 1
        for s in shape:
            n *= s
        flat, self._check = guarded(1, n + off, torch.float32, dev, fill=0.0)
        self.pad = flat[0, :off]
        self.pad_bits = bits(self.pad).clone()
        flat = flat[0, off:]
        if cl:
            N, C, H, W = shape
            self.t = flat.view(N, H, W, C).permute(0, 3, 1, 2)
        else:
            self.t = flat.view(shape)
        assert self.t.data_ptr() % 16 == 4 * off and self.t.shape == torch.Size(shape)
        if value is not None:
            self.t.copy_(value)

    def check(self):
        self._check()
        assert torch.equal(bits(self.pad), self.pad_bits), "the element in front of a misaligned tensor was overwritten"


class Set:
    """the parameters (fp32, in guarded windows unless plain) with their gradients and state, a HipAdam over them, and the same
    start as plain tensors for the references"""

    def __init__(self, to, dev, guard=True, seed=0):
        from mickey_amd import _native
        E = int(_native.query("mk_optim_chunk_elems"))
        self.specs = _specs(E)
        gen = torch.Generator().manual_seed(1234 + seed)
        self.init, self.win, self.params = [], [], []
        ref_opt_groups = [[], []]
        for name, shape, cl, mis, has_grad, group in self.specs:
            p0 = (torch.randn(shape, generator=gen) * 1e-3).to(dev)
            if cl:
                p0 = p0.contiguous(memory_format=torch.channels_last)
            self.init.append(p0)
            w = {k: Window(shape, cl, int(mis == k), dev, value=p0 if k == "p" else None) if guard or mis == k else None for k in "pgmv"}
            self.win.append(w)
            p = nn.Parameter(w["p"].t if w["p"] is not None else p0.clone(memory_format=torch.preserve_format))
            self.params.append(p)
            ref_opt_groups[group].append(p)
        adam = torch.optim.Adam([dict(params=ps, **hp) for ps, hp in zip(ref_opt_groups, GROUPS)])
        for p, w, (_, _, _, _, has_grad, _) in zip(self.params, self.win, self.specs):
            if has_grad:   # the state in windows of ours: from_torch adopts the very tensors
                m = w["m"].t if w["m"] is not None else torch.zeros_like(p, memory_format=torch.preserve_format)
                v = w["v"].t if w["v"] is not None else torch.zeros_like(p, memory_format=torch.preserve_format)
                adam.state[p] = dict(step=torch.tensor(0.0), exp_avg=m, exp_avg_sq=v)
        self.opt = to.HipAdam.from_torch(adam)
        self.hyper = [GROUPS[s[5]] for s in self.specs]

    def set_grads(self, grads, fresh=False):
        """grads[i] None: no gradient.  Into the window's tensor where there is one, else into the kept .grad (or a new tensor)"""
        self.old = [p.grad for p in self.params] if fresh else None     # kept alive: the new gradients lie at other addresses
        for p, w, g in zip(self.params, self.win, grads):
            if g is None:
                p.grad = None
            elif w["g"] is not None:
                w["g"].t.copy_(g)
                p.grad = w["g"].t
            elif p.grad is None or fresh:
                p.grad = g.clone(memory_format=torch.preserve_format)
            else:
                p.grad.copy_(g)

    def check(self):
        for w in self.win:
            for x in w.values():
                if x is not None:
                    x.check()

    def snapshot(self):
        out = []
        for p in self.params:
            s = self.opt.state.get(p, {})
            out.append([t.detach().clone(memory_format=torch.preserve_format) if t is not None else None
                        for t in (p, p.grad, s.get("exp_avg"), s.get("exp_avg_sq"), s.get("step"))])
        return out


def _same_bits(a, b):
    for ra, rb in zip(a, b):
        for x, y in zip(ra, rb):
            if (x is None) != (y is None) or (x is not None and not torch.equal(bits(x), bits(y))):
                return False
    return True


def _draw(specs, init, gen, kind, scale, dev):
    grads = []
    for (name, shape, cl, mis, has_grad, group), p0 in zip(specs, init):
        if not has_grad:
            grads.append(None)
            continue
        g = (torch.randn(shape, generator=gen) * scale).to(dev)
        grads.append(g.contiguous(memory_format=torch.channels_last) if cl else g)
    extra = torch.randn(33, generator=gen).to(dev)
    # the offender sits in the last, partial quad of the second chunk of the 2E+3 tensor / in the misaligned gradient
    if kind == "nan":
        grads[7][-1] = float("nan")
    if kind == "inf":
        grads[11][-4] = -float("inf")
    if kind == "also_nan":
        extra[32] = float("nan")
    return grads, extra


def _run(to, dev, guard=True, fresh=False, collect=None):
    """the five steps on a new Set -> [(status, snapshot)] per step; collect(step index, kind, set, before, grads, extra, status)"""
    s = Set(to, dev, guard=guard)
    gen = torch.Generator().manual_seed(99)
    out = []
    for i, (kind, scale) in enumerate(STEPS):
        grads, extra = _draw(s.specs, s.init, gen, kind, scale, dev)
        s.set_grads(grads, fresh=fresh and i % 2 == 1)
        before = s.snapshot()
        status = s.opt.step_guarded(max_norm=MAX_NORM, also_finite=(extra, extra[:5]))
        s.check()
        out.append((status.clone(), s.snapshot()))
        if collect:
            collect(i, kind, s, before, grads, extra, status)
    return out


# ---- 1: five steps against the fp64 formula ---------------------------------------------------------------------------------------------
def test_five_guarded_steps_against_fp64(to):
    dev = torch.device("cuda")
    ref_state = {}

    def collect(i, kind, s, before, grads, extra, status):
        if not ref_state:   # the two references start where the set started
            ref_state["p64"] = [p.double() for p in s.init]
            ref_state["s64"] = [dict(step=0, exp_avg=torch.zeros_like(p), exp_avg_sq=torch.zeros_like(p)) for p in ref_state["p64"]]
            ref_state["p32"] = [nn.Parameter(p.clone(memory_format=torch.preserve_format)) for p in s.init]
            by_group = [[p for p, sp in zip(ref_state["p32"], s.specs) if sp[5] == k] for k in (0, 1)]
            ref_state["adam"] = torch.optim.Adam([dict(params=ps, **hp) for ps, hp in zip(by_group, GROUPS)])
        after = s.snapshot()
        ok, total = (float(x) for x in status.cpu())
        live = [j for j, g in enumerate(grads) if g is not None]
        if kind in ("nan", "inf", "also_nan"):
            assert ok == 0.0
            assert _same_bits(before, after), "a skipped step changed something"
            g64 = [None if g is None else g.double() for g in grads]
            assert to.guarded_step_formula(ref_state["p64"], g64, ref_state["s64"], s.hyper, MAX_NORM, (extra,))[0] is False
            return
        assert ok == 1.0
        # the fp64 reference on the same fp32 gradients
        p64_old = [p.clone() for p in ref_state["p64"]]
        g64 = [None if g is None else g.double() for g in grads]
        ok64, total64, coef64 = to.guarded_step_formula(ref_state["p64"], g64, ref_state["s64"], s.hyper, MAX_NORM, (extra,))
        assert ok64 and (coef64 < 1.0) == (kind == "clipped")
        print("step %d %s: total_norm %.9g against %.17g in fp64" % (i, kind, total, total64))
        assert abs(total - total64) <= 2.0 ** -23 * total64
        # torch fp32 on the same GPU
        p32_old = [p.detach().clone() for p in ref_state["p32"]]
        for p, g in zip(ref_state["p32"], grads):
            p.grad = None if g is None else g.clone(memory_format=torch.preserve_format)
        torch.nn.utils.clip_grad_norm_(ref_state["p32"], MAX_NORM)
        ref_state["adam"].step()
        # the gradient: g coef where the norm was above max_norm (one fp32 multiply), its own bits where not
        coef32 = torch.tensor(MAX_NORM, dtype=torch.float32) / (torch.tensor(total, dtype=torch.float32) + torch.tensor(1e-6, dtype=torch.float32))
        for j in live:
            want = grads[j] * coef32.to(dev) if kind == "clipped" else grads[j]
            assert torch.equal(bits(after[j][1]), bits(want)), (kind, s.specs[j][0])
        verdicts = []
        for j in live:
            name = s.specs[j][0]
            st32 = ref_state["adam"].state[ref_state["p32"][j]]
            case = "step %d %s" % (i, kind)
            verdicts.append(_bound(case, name + ".m", after[j][2], ref_state["s64"][j]["exp_avg"], st32["exp_avg"]))
            verdicts.append(_bound(case, name + ".v", after[j][3], ref_state["s64"][j]["exp_avg_sq"], st32["exp_avg_sq"]))
            verdicts.append(_bound(case, name + ".upd", after[j][0].double() - before[j][0].double(), ref_state["p64"][j] - p64_old[j],
                                   ref_state["p32"][j].detach().double() - p32_old[j].double()))
            upd = (ref_state["p64"][j] - p64_old[j]).abs().max()
            assert upd >= 2.0 ** -10 * ref_state["p64"][j].abs().max(), "the update must not drown in the rounding of p"
            assert torch.equal(after[j][4], torch.full_like(after[j][4], float(ref_state["s64"][j]["step"])))    # every chunk's cell
        for fine, why in verdicts:
            assert fine, why
        nograd = [j for j, g in enumerate(grads) if g is None]
        assert nograd and all(_same_bits([before[j]], [after[j]]) and len(s.opt.state.get(s.params[j], {})) == 0 for j in nograd)

    out = _run(to, dev, collect=collect)
    assert [float(st[0]) for st, _ in out] == [1.0, 0.0, 0.0, 0.0, 1.0]
    assert sorted({s["step"] for s in ref_state["s64"]}) == [0, 2]      # (0: the parameter without a gradient)


# ---- 2: determinism, fresh gradient storage, plain step ----------------------------------------------------------------------------------
def test_the_same_steps_twice_give_the_same_bits(to):
    dev = torch.device("cuda")
    a, b = _run(to, dev), _run(to, dev)
    for (sa, xa), (sb, xb) in zip(a, b):
        assert torch.equal(bits(sa), bits(sb)) and _same_bits(xa, xb)


def test_fresh_gradient_storage_gives_the_same_results(to):
    """steps that keep .grad alternate with steps after which it is None and comes back at another address (zero_grad's default)"""
    dev = torch.device("cuda")
    seen = []

    def addresses(i, kind, s, *rest):
        seen.append([p.grad.data_ptr() for p in s.params if p.grad is not None])

    kept = _run(to, dev, guard=False)
    fresh = _run(to, dev, guard=False, fresh=True, collect=addresses)
    assert seen[0] != seen[1] and seen[1] == seen[2] and seen[2] != seen[3]
    for (sa, xa), (sb, xb) in zip(kept, fresh):
        assert torch.equal(bits(sa), bits(sb)) and _same_bits(xa, xb)
    guarded_run = _run(to, dev)                       # and the windows change nothing either
    assert _same_bits(kept[-1][1], guarded_run[-1][1])


def test_plain_step_is_the_guarded_step_without_clip(to):
    dev = torch.device("cuda")
    a, b = Set(to, dev), Set(to, dev)
    gen = torch.Generator().manual_seed(5)
    for _ in range(2):
        grads, extra = _draw(a.specs, a.init, gen, "plain", 1.0, dev)
        a.set_grads(grads)
        b.set_grads(grads)
        assert a.opt.step() is None
        status = b.opt.step_guarded()
        a.check()
        b.check()
        assert float(status[0]) == 1.0
        assert _same_bits(a.snapshot(), b.snapshot())
    assert a.opt.step(lambda: torch.tensor(3.0)) == 3.0


def test_an_lr_changed_on_the_host_is_picked_up(to):
    dev = torch.device("cuda")
    p = nn.Parameter(torch.zeros(5, device=dev))
    opt = to.HipAdam([p], lr=1e-2)
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=1, gamma=0.5)
    p.grad = torch.ones(5, device=dev)
    opt.step_guarded()
    sched.step()
    first = p.detach().clone()
    opt.step_guarded()
    torch.testing.assert_close(first, torch.full((5,), -1e-2, device=dev), rtol=1e-5, atol=0)
    torch.testing.assert_close(p.detach() - first, torch.full((5,), -5e-3, device=dev), rtol=1e-5, atol=0)


# ---- 3: nothing in the step waits for the device --------------------------------------------------------------------------------------
def test_step_guarded_returns_before_the_queue_drains(to):
    """a guarded step enqueued behind some milliseconds of BatchNorm forward returns to Python before that work's completion event is done"""
    from mickey_amd import ops
    dev = torch.device("cuda")
    s = Set(to, dev, guard=False)
    gen = torch.Generator().manual_seed(3)
    grads, extra = _draw(s.specs, s.init, gen, "plain", 1.0, dev)
    s.set_grads(grads)
    M, C = 1 << 21, 256
    x = torch.zeros((M, C), device=dev)
    y = torch.empty_like(x)
    work = torch.empty((ops.bn_chunks(M) * 2 * C,), device=dev)
    gamma, beta, rm, rv = (torch.ones(C, device=dev) for _ in range(4))
    nbt = torch.zeros((), dtype=torch.int64, device=dev)

    def long_kernel():
        for _ in range(2):
            ops.train_bn_fwd(x, gamma, beta, rm, rv, nbt, True, 0.1, 1e-5, relu=False, want_saved=False, out=y, work=work)

    long_kernel()                                       # code objects, the table's first upload
    s.opt.step_guarded(max_norm=MAX_NORM, also_finite=(extra,))
    torch.cuda.synchronize()
    done = torch.cuda.Event()
    long_kernel()
    done.record()
    status = s.opt.step_guarded(max_norm=MAX_NORM, also_finite=(extra,))
    still_running = not done.query()
    torch.cuda.synchronize()
    assert still_running, "step_guarded returned only after the work enqueued in front of it had finished"
    assert float(status[0]) == 1.0


# ---- 4: checkpoints ----------------------------------------------------------------------------------------------------------------------
def _tiny(dev, seed):
    g = torch.Generator().manual_seed(seed)
    return [nn.Parameter((torch.randn(s, generator=g) * 1e-3).to(dev)) for s in ((), (7,), (4100,), (3, 5))]


def _feed(params, gen, dev):
    for p in params:
        p.grad = torch.randn(p.shape, generator=gen).to(dev)


@pytest.mark.parametrize("direction", ["torch_to_hip", "hip_to_torch"])
def test_state_dict_round_trip(to, direction):
    """two steps with one optimiser, load_state_dict into the other, one more step: compared with the first one continuing"""
    dev = torch.device("cuda")
    hp = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.01)
    a, b = _tiny(dev, 0), _tiny(dev, 0)
    make = {"torch": lambda ps: torch.optim.Adam(ps, **hp), "hip": lambda ps: to.HipAdam(ps, **hp)}
    src, dst = direction.split("_to_")
    first, other = make[src](a), make[dst](b)
    gen = torch.Generator().manual_seed(11)
    for _ in range(2):
        _feed(a, gen, dev)
        first.step()
    sd = first.state_dict()
    assert all(s["step"].device.type == "cpu" and s["step"].shape == () and float(s["step"]) == 2.0 for s in sd["state"].values())
    other.load_state_dict(copy.deepcopy(sd))      # as a checkpoint file would: load_state_dict keeps tensors that already fit
    with torch.no_grad():
        for pa, pb in zip(a, b):
            pb.copy_(pa)
    _feed(a, gen, dev)
    for pa, pb in zip(a, b):
        pb.grad = pa.grad.clone()
    before = [p.detach().clone() for p in a]
    first.step()
    other.step()
    for i, (pa, pb, p0) in enumerate(zip(a, b, before)):
        ua, ub = pa.detach().double() - p0.double(), pb.detach().double() - p0.double()
        e = float((ua - ub).abs().max() / ua.abs().max())
        print("%s tensor %d: update differs by %.3e" % (direction, i, e))
        assert e <= FLOOR, (direction, i, e)
        sa, sb = first.state[pa], other.state[pb]
        assert _err(sb["exp_avg"], sa["exp_avg"].double()) <= FLOOR and _err(sb["exp_avg_sq"], sa["exp_avg_sq"].double()) <= FLOOR
    assert all(float(s["step"]) == 3.0 for s in other.state_dict()["state"].values())


# ---- 5: backward_step ----------------------------------------------------------------------------------------------------------------
class _Net(nn.Module):
    def __init__(self):
        super().__init__()
        self.a, self.b = nn.Linear(8, 16), nn.Linear(16, 7)

    def forward(self, x):
        return self.b(torch.tanh(self.a(x)))


def _wire(net, x, branch):
    """batch / outputs / avg_loss as training_step leaves them (model.py:118-134): the heads' tensors stay in the graph, the pose
    loss is taken on detached copies that keep their gradients"""
    o = net(x)
    batch = dict(kps0=o[:, 0:2], kps1=o[:, 2:4], depth_kp0=o[:, 4:5], depth_kp1=o[:, 5:6], final_scores=torch.sigmoid(o[:, 6]))
    if branch != "kps":
        batch["kps0"], batch["kps1"] = batch["kps0"].detach(), batch["kps1"].detach()
    if branch == "scores":
        batch["depth_kp0"], batch["depth_kp1"] = batch["depth_kp0"].detach(), batch["depth_kp1"].detach()
    outputs = {k: batch[src].detach().clone().requires_grad_(True) for k, src in
               (("kps0", "kps0"), ("kps1", "kps1"), ("depth0", "depth_kp0"), ("depth1", "depth_kp1"))}
    avg_loss = sum(((i + 1) * t * t).sum() + t.sum() for i, t in enumerate(outputs.values()))
    return batch, outputs, avg_loss


def _reference_backward_step(batch, outputs, probs_grad, avg_loss, opt, params):
    """model.py:91-147 with torch.optim.Adam, host checks and all"""
    opt.zero_grad()
    avg_loss.backward()
    grads = [outputs[k].grad for k in ("kps0", "kps1", "depth0", "depth1")]
    if any(bool(torch.isnan(t).any() or torch.isinf(t).any()) for t in [probs_grad[0]] + grads):
        return False
    log_scores = torch.log(batch["final_scores"] + 1e-16)
    if batch["kps0"].requires_grad:
        torch.autograd.backward((log_scores, batch["kps0"], batch["kps1"], batch["depth_kp0"], batch["depth_kp1"]), (probs_grad[0], *grads))
    elif batch["depth_kp0"].requires_grad:
        torch.autograd.backward((log_scores, batch["depth_kp0"], batch["depth_kp1"]), (probs_grad[0], grads[2], grads[3]))
    else:
        torch.autograd.backward((log_scores,), (probs_grad[0],))
    torch.nn.utils.clip_grad_norm_(params, max_norm=5)
    if sum(bool(torch.isnan(p.grad).any()) for p in params if p.grad is not None) != 0:
        return False
    opt.step()
    return True


@pytest.mark.parametrize("branch", ["kps", "depth", "scores"])
def test_backward_step(to, branch):
    from mickey_amd import train_step
    dev = torch.device("cuda")
    torch.manual_seed(17)
    nets = {"hip": _Net().to(dev)}
    nets["t32"] = _Net().to(dev)
    nets["t32"].load_state_dict(nets["hip"].state_dict())
    nets["f64"] = _Net().to(dev).double()
    nets["f64"].load_state_dict(nets["hip"].state_dict())
    hp = dict(lr=5e-2, eps=1e-6)      # lr of the order of the weights: the update is far above the rounding of p
    opts = {"hip": to.HipAdam(nets["hip"].parameters(), **hp), "t32": torch.optim.Adam(nets["t32"].parameters(), **hp),
            "f64": torch.optim.Adam(nets["f64"].parameters(), **hp)}
    gen = torch.Generator().manual_seed(23)
    assert train_step.backward_step(nets["hip"], {}, {}, [None], None, 0, opts["hip"]) is None
    for step in range(3):
        x = torch.randn(32, 8, generator=gen).to(dev)
        probs = torch.randn(32, generator=gen).to(dev) * (30.0 if step == 0 else 0.5)     # the first step is clipped
        if step == 1:
            probs[7] = float("nan")
        old = {k: [p.detach().clone() for p in n.parameters()] for k, n in nets.items()}
        for k in ("t32", "f64"):
            xx, pp = (x.double(), probs.double()) if k == "f64" else (x, probs)
            batch, outputs, avg_loss = _wire(nets[k], xx, branch)
            assert _reference_backward_step(batch, outputs, [pp], avg_loss, opts[k], list(nets[k].parameters())) == (step != 1)
        batch, outputs, avg_loss = _wire(nets["hip"], x, branch)
        status = train_step.backward_step(nets["hip"], batch, outputs, [probs], avg_loss, 1, opts["hip"])
        assert status.shape == (2,) and status.is_cuda and float(status[0]) == float(step != 1)
        new = {k: [p.detach() for p in n.parameters()] for k, n in nets.items()}
        if step == 1:
            assert all(torch.equal(bits(a), bits(b)) for a, b in zip(old["hip"], new["hip"])), "a NaN in probs_grad must leave the parameters alone"
            continue
        names = [n for n, _ in nets["hip"].named_parameters()]
        verdicts = []
        for j, name in enumerate(names):
            upd = {k: new[k][j].double() - old[k][j].double() for k in nets}
            case = "backward_step %s step %d" % (branch, step)
            verdicts.append(_bound(case, name + ".upd", upd["hip"], upd["f64"], upd["t32"]))
            st = {k: opts[k].state[list(nets[k].parameters())[j]] for k in nets}
            verdicts.append(_bound(case, name + ".m", st["hip"]["exp_avg"], st["f64"]["exp_avg"], st["t32"]["exp_avg"]))
            verdicts.append(_bound(case, name + ".v", st["hip"]["exp_avg_sq"], st["f64"]["exp_avg_sq"], st["t32"]["exp_avg_sq"]))
        for fine, why in verdicts:
            assert fine, why
