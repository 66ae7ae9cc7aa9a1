"""mickey_amd.train_attention on the GPU: forward and the three gradients of the trainable linear attention.

The yardstick is linear_attention_formula (the in-repo restatement of att_layers/attention.py:46-64, checked against the reference's
own fp64 autograd by tests/test_train_attention_cpu.py) under fp64 autograd on the device, on the same inputs.  For out, gQ, gK, gV

    e = max |x - x64| / max |x64|   <=   max(2 * e_torch32, 2e-6)

e_torch32 = the same error of the same formula run by torch in fp32 on the same GPU; 2e-6 = the project's fp32-grade bound
(DESIGN.md section 4); 2 = the margin between two fp32 summation orders over up to 1938 terms.  Every measured figure goes to
profiles/train_attention_parity.txt.

The case L = S = 1 is ill-conditioned for gQ and gK: with one key the output does not depend on q or k except through eps, the true
gradients are of order eps / den (1e-8 here) and any fp32 evaluation returns the rounding noise of two cancelling terms of order 1.
Measured: e_hip 1.05 (gQ), 1.30 (gK) against e_torch32 2.70, 4.87 -- both are noise; the rule is applied to it as to every case."""
import copy
import itertools
import os

import numpy as np
import pytest
import torch
from torch import nn

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "linattn_grad.npz")
FLOOR = 2e-6
EPS = 1e-6
RESULTS = []
NAMES = ("out", "gQ", "gK", "gV")


@pytest.fixture(scope="module")
def ta():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from mickey_amd import train_attention
    yield train_attention
    if RESULTS:
        try:
            with open(os.path.join(ROOT, "profiles", "train_attention_parity.txt"), "w") as f:
                f.write("# tests/test_train_attention_gpu.py: max |x - x64| / max |x64| against linear_attention_formula under fp64 autograd\n")
                f.write("# bound: max(2 * e_torch32, 2e-6), e_torch32 = the same formula in torch fp32 on the same GPU\n")
                f.write("# %-40s %-22s %12s %12s %12s\n" % ("case", "tensor", "e_hip", "e_torch32", "bound"))
                for r in RESULTS:
                    f.write("%-42s %-22s %12.3e %12.3e %12.3e\n" % r)
        except OSError:
            pass   # a read-only checkout: the assertions have run all the same


def _err(a, ref):
    ref = ref.detach().double().cpu()
    return float((a.detach().double().cpu() - ref).abs().max() / ref.abs().max())


def _inputs(N, L, S, C, seed=0):
    g = torch.Generator().manual_seed(seed + 1000 * N + 10 * L + S + C)
    H = C // 16
    q = (1.5 * torch.randn((N, L, H, 16), generator=g)).cuda()   # both branches of elu
    k = (1.5 * torch.randn((N, S, H, 16), generator=g)).cuda()
    v = torch.randn((N, S, H, 16), generator=g).cuda()
    go = torch.randn((N, L, H, 16), generator=g).cuda()
    return q, k, v, go


def _formula(ta, q, k, v, go, dtype, eps=EPS):
    x = [t.detach().to(dtype).requires_grad_(True) for t in (q, k, v)]
    out = ta.linear_attention_formula(*x, eps)
    return (out.detach(),) + tuple(torch.autograd.grad(out, x, go.to(dtype)))


def _hip(ta, q, k, v, go, need=(True, True, True), eps=EPS):
    x = [t.detach().requires_grad_(n) for t, n in zip((q, k, v), need)]
    out = ta.linear_attention_train(*x, eps)
    grads = iter(torch.autograd.grad(out, [t for t, n in zip(x, need) if n], go))
    return (out.detach(),) + tuple(next(grads) if n else None for n in need)


def _check(case, got, ref, t32, names=NAMES):
    """Prints and records every figure, then asserts the bound of the module docstring."""
    rows = []
    for name, g, r, t in zip(names, got, ref, t32):
        e_hip, e_t = _err(g, r), _err(t, r)
        rows.append((case, name, e_hip, e_t, max(2 * e_t, FLOOR)))
        print("%s %s: e_hip %.3e  e_torch32 %.3e  bound %.3e" % rows[-1])
    RESULTS.extend(rows)
    for case, name, e_hip, e_t, bound in rows:
        assert e_hip <= bound, (case, name, e_hip, e_t, bound)


@pytest.mark.parametrize("N,L,S,C", [(1, 1, 1, 16), (2, 37, 29, 128), (3, 200, 333, 64), (1, 1938, 700, 128), (8, 1938, 1938, 128)])
def test_parity_per_shape(ta, N, L, S, C):
    q, k, v, go = _inputs(N, L, S, C)
    got = _hip(ta, q, k, v, go)
    assert got[0].shape == q.shape and got[0].is_contiguous() and got[0].dtype == torch.float32
    assert got[1].shape == q.shape and got[2].shape == k.shape and got[3].shape == v.shape
    _check("N%d L%d S%d C%d" % (N, L, S, C), got, _formula(ta, q, k, v, go, torch.float64), _formula(ta, q, k, v, go, torch.float32))


@pytest.mark.parametrize("tag", ["a", "b"])
def test_parity_on_the_golden_fixture(ta, tag):
    z = np.load(GOLDEN)
    q, k, v, go = (torch.from_numpy(z["%s_%s" % (n, tag)]).cuda() for n in ("q", "k", "v", "go"))
    eps = float(z["eps"])
    got = _hip(ta, q, k, v, go, eps=eps)
    ref, t32 = _formula(ta, q, k, v, go, torch.float64, eps), _formula(ta, q, k, v, go, torch.float32, eps)
    case = "golden %s N%d L%d S%d C%d" % (tag, q.shape[0], q.shape[1], k.shape[1], q.shape[2] * 16)
    _check(case, got, ref, t32)
    # and against what the reference's own autograd stored
    stored = tuple(torch.from_numpy(z["%s_%s" % (n, tag)]) for n in ("out", "gq", "gk", "gv"))
    _check(case, got, stored, t32, names=tuple(n + " (stored)" for n in NAMES))


def test_gradient_magnitude_zero_and_non_finite(ta):
    N, L, S, C = 2, 70, 45, 128
    q, k, v, go = _inputs(N, L, S, C, seed=5)
    ref, t32 = _formula(ta, q, k, v, go, torch.float64), _formula(ta, q, k, v, go, torch.float32)
    base = _hip(ta, q, k, v, go)
    for p in (-40, 20):
        s = 2.0 ** p
        got = _hip(ta, q, k, v, go * s)
        # the backward is linear in gO and a power of two is exact: the scaled bits, hence the same relative bounds
        for u, b in zip(got[1:], base[1:]):
            assert torch.equal(u, b * s), p
        _check("N2 L70 S45 C128 gO*2^%d" % p, tuple(u / s for u in got[1:]), ref[1:], t32[1:], names=NAMES[1:])
    zero = _hip(ta, q, k, v, torch.zeros_like(go))
    for u in zero[1:]:
        assert float(u.abs().max()) == 0.0 and bool(torch.isfinite(u).all())
    fin = lambda t: torch.isfinite(t)   # noqa: E731
    for bad in (float("nan"), float("inf"), -float("inf")):
        g = go.clone()
        g[0, 3, 2, 5] = bad   # image 0, token 3, head 2, channel 5
        _, gq, gk, gv = _hip(ta, q, k, v, g)
        assert not bool(fin(gq[0, 3, 2]).any()), bad                      # that token's gQ (through gnum and gden)
        assert not bool(fin(gk[0, :, 2]).any()), bad                      # gK of that (image, head) (through gM and gks)
        assert not bool(fin(gv[0, :, 2, 5]).any()), bad                   # gV: column 5 of gM
        mask = torch.ones_like(gq, dtype=torch.bool)
        mask[0, 3, 2] = False
        assert bool(fin(gq[mask]).all()) and torch.equal(gq[mask], base[1][mask])
        assert bool(fin(gk[1]).all()) and bool(fin(gv[1]).all()) and torch.equal(gk[1], base[2][1]) and torch.equal(gv[1], base[3][1])
        heads = [h for h in range(8) if h != 2]
        assert torch.equal(gk[0][:, heads], base[2][0][:, heads]) and torch.equal(gv[0][:, heads], base[3][0][:, heads])
    for bad in (float("nan"), float("inf")):
        qq = q.clone()
        qq[1, 7, 4, 9] = bad
        out, gq, gk, gv = _hip(ta, qq, k, v, go)
        assert not bool(fin(out[1, 7, 4]).any()) and not bool(fin(gq[1, 7, 4]).any()), bad
        assert not bool(fin(gk[1, :, 4]).any()) and not bool(fin(gv[1, :, 4]).any()), bad
        mask = torch.ones_like(out, dtype=torch.bool)
        mask[1, 7, 4] = False
        assert torch.equal(out[mask], base[0][mask]) and torch.equal(gq[mask], base[1][mask])
        assert torch.equal(gk[0], base[2][0]) and torch.equal(gv[0], base[3][0])
    # the forward is untouched by all of this
    assert torch.equal(_hip(ta, q, k, v, go)[0], base[0])


@pytest.mark.parametrize("N,L,S,C", [(2, 37, 29, 128), (3, 200, 333, 64), (8, 1938, 1938, 128)])
def test_two_runs_are_bit_identical(ta, N, L, S, C):
    q, k, v, go = _inputs(N, L, S, C, seed=3)
    a = _hip(ta, q, k, v, go)
    torch.cuda.synchronize()
    b = _hip(ta, q, k, v, go)
    for u, w in zip(a, b):
        assert torch.equal(u, w)


def test_batch_invariance(ta):
    q, k, v, go = _inputs(8, 1938, 1938, 128, seed=11)
    full = _hip(ta, q, k, v, go)
    for i in (0, 5, 7):
        one = _hip(ta, q[i:i + 1], k[i:i + 1], v[i:i + 1], go[i:i + 1])
        for u, w in zip(one, full):
            assert torch.equal(u[0], w[i]), i
    # cross attention, a ragged last chunk on both sides
    q, k, v, go = _inputs(3, 200, 333, 64, seed=12)
    full = _hip(ta, q, k, v, go)
    one = _hip(ta, q[2:3].clone(), k[2:3].clone(), v[2:3].clone(), go[2:3].clone())
    for u, w in zip(one, full):
        assert torch.equal(u[0], w[2])


def test_needs_input_grad(ta, monkeypatch):
    from mickey_amd import ops
    q, k, v, go = _inputs(2, 90, 75, 128, seed=7)
    full = _hip(ta, q, k, v, go)
    seen = []
    real = ops.linattn_train_bwd

    def spy(*args):
        r = real(*args)
        seen.append((tuple(args[-1]), tuple(t is not None for t in r)))
        return r
    monkeypatch.setattr(ops, "linattn_train_bwd", spy)
    for need in itertools.product((False, True), repeat=3):
        if not any(need):
            continue
        got = _hip(ta, q, k, v, go, need=need)
        assert seen[-1] == (need, need)   # the kernels were asked for, and returned, exactly the wanted gradients
        assert torch.equal(got[0], full[0])
        for n, u, w in zip(need, got[1:], full[1:]):
            assert (u is None and not n) or torch.equal(u, w), need
        # through .backward(): no gradient lands on an input that does not require one
        x = [t.detach().clone().requires_grad_(n) for t, n in zip((q, k, v), need)]
        ta.linear_attention_train(*x).backward(go)
        for n, t, w in zip(need, x, full[1:]):
            assert (t.grad is None) if not n else torch.equal(t.grad, w), need
    n_calls = len(seen)
    out = ta.linear_attention_train(q, k, v)   # nothing requires grad: no graph
    assert out.grad_fn is None and torch.equal(out, full[0]) and len(seen) == n_calls


def test_layouts_give_identical_results(ta):
    N, L, C = 2, 83, 128
    H = C // 16
    q, k, v, go = _inputs(N, L, L, C, seed=9)
    base = _hip(ta, q, k, v, go)
    packed = torch.cat([t.reshape(N, L, C) for t in (q, k, v)], dim=2)   # one [N, L, 3C] buffer, as a fused q | k | v projection writes
    views = [packed[:, :, i * C:(i + 1) * C].view(N, L, H, 16) for i in range(3)]
    assert all(not t.is_contiguous() and t.data_ptr() == packed.data_ptr() + 4 * C * i for i, t in enumerate(views))
    assert all(ta._rows(t) is t for t in views)   # read in place: no copy
    for u, w in zip(_hip(ta, *views, go), base):
        assert torch.equal(u, w)
    # layouts the kernels do not read in place are made contiguous first: head-major storage, odd offsets, expanded images
    head_major = [t.permute(0, 2, 1, 3).contiguous().permute(0, 2, 1, 3) for t in (q, k, v)]
    assert all(not t.is_contiguous() and ta._rows(t) is not t for t in head_major)
    for u, w in zip(_hip(ta, *head_major, go), base):
        assert torch.equal(u, w)
    odd = torch.zeros(q.numel() + 1, device="cuda")
    odd[1:] = q.reshape(-1)
    q_odd = odd[1:].view(q.shape)
    assert q_odd.data_ptr() % 16 != 0
    for u, w in zip(_hip(ta, q_odd, k, v, go), base):
        assert torch.equal(u, w)
    go_t = go.permute(0, 2, 1, 3).contiguous().permute(0, 2, 1, 3)
    for u, w in zip(_hip(ta, q, k, v, go_t), base):
        assert torch.equal(u, w)
    # the gradient reaches the packed buffer through the views
    p = packed.clone().requires_grad_(True)
    ta.linear_attention_train(*[p[:, :, i * C:(i + 1) * C].view(N, L, H, 16) for i in range(3)]).backward(go)
    assert torch.equal(p.grad, torch.cat([t.reshape(N, L, C) for t in base[1:]], dim=2))


def test_saved_memory(ta):
    N, L, S, C = 8, 1938, 1938, 128
    q, k, v, _ = _inputs(N, L, S, C, seed=13)
    limit = (q.numel() + k.numel() + v.numel() + N * (C // 16) * 272) * 4

    def saved_bytes(fn):
        kept = []

        def pack(t):
            kept.append(t)
            return t
        with torch.autograd.graph.saved_tensors_hooks(pack, lambda t: t):
            out = fn()
        return sum(t.numel() * t.element_size() for t in kept), out

    x = [t.detach().requires_grad_(True) for t in (q, k, v)]
    hip_bytes, out = saved_bytes(lambda: ta.linear_attention_train(*x))
    torch_bytes, _ = saved_bytes(lambda: ta.linear_attention_formula(*x))
    print("saved by autograd: HIP %.1f MiB (limit %.1f MiB), the torch formula %.1f MiB" % (hip_bytes / 2 ** 20, limit / 2 ** 20, torch_bytes / 2 ** 20))
    assert out.grad_fn is not None and 0 < hip_bytes <= limit
    # only q requires grad: still no more than the inputs and the block
    only_q, _ = saved_bytes(lambda: ta.linear_attention_train(x[0], k, v))
    assert 0 < only_q <= limit
    with torch.no_grad():
        none, out = saved_bytes(lambda: ta.linear_attention_train(*x))
    assert none == 0 and out.grad_fn is None
    none, out = saved_bytes(lambda: ta.linear_attention_train(q, k, v))
    assert none == 0 and out.grad_fn is None


def test_wrong_arguments_raise_on_the_device_too(ta):
    from mickey_amd import _native
    q, k, v, _ = _inputs(2, 5, 7, 128)
    with pytest.raises(ValueError):
        ta.linear_attention_train(q.half(), k.half(), v.half())
    with torch.autocast("cuda", dtype=torch.float16):
        with pytest.raises(ValueError):
            ta.linear_attention_train(q.half(), k, v)
    with pytest.raises(ValueError):
        ta.linear_attention_train(q, k, v[:, :6])
    with pytest.raises(_native.MickeyHipError):
        ta.linear_attention_train(q, k.cpu(), v)


# ---- end to end: a stand-in for the reference's att_layers (its attribute names and call contract, none of its code) ------------
class _Att(nn.Module):
    def __init__(self, eps=EPS):
        super().__init__()
        from mickey_amd import train_attention
        self.feature_map = lambda x: nn.functional.elu(x) + 1
        self.formula = train_attention.linear_attention_formula
        self.eps = eps
        self.attention = "linear"

    def forward(self, queries, keys, values):
        return self.formula(queries, keys, values, self.eps).contiguous()


class _Layer(nn.Module):
    def __init__(self, d, heads):
        super().__init__()
        self.heads = heads
        self.q_proj, self.k_proj, self.v_proj, self.merge = (nn.Linear(d, d, bias=False) for _ in range(4))
        self.attention = _Att()
        self.mlp = nn.Sequential(nn.Linear(2 * d, 2 * d, bias=False), nn.ReLU(), nn.Linear(2 * d, d, bias=False))
        self.norm1, self.norm2 = nn.LayerNorm(d), nn.LayerNorm(d)

    def forward(self, x, src):
        n, d = x.shape[0], x.shape[2]
        split = lambda t: t.view(n, -1, self.heads, d // self.heads)   # noqa: E731
        msg = self.attention(split(self.q_proj(x)), split(self.k_proj(src)), split(self.v_proj(src)))
        msg = self.norm1(self.merge(msg.view(n, -1, d)))
        return x + self.norm2(self.mlp(torch.cat([x, msg], dim=2)))


class _Stack(nn.Module):
    def __init__(self, d=128, heads=8, layers=3):
        super().__init__()
        self.layers = nn.ModuleList([_Layer(d, heads) for _ in range(layers)])

    def forward(self, x):
        for layer in self.layers:
            x = layer(x, x)
        return x


def test_encoder_stack_end_to_end_and_adam_step(ta):
    torch.manual_seed(21)
    N, L, d = 2, 300, 128
    model = _Stack(d).cuda()
    x = torch.randn((N, L, d), device="cuda")
    gy = torch.randn((N, L, d), device="cuda")

    def run(m, dtype):
        m.zero_grad(set_to_none=True)
        y = m(x.to(dtype))
        y.backward(gy.to(dtype))
        return [y.detach()] + [p.grad.detach().clone() for p in m.parameters()]

    ref = run(copy.deepcopy(model).double(), torch.float64)
    t32 = run(copy.deepcopy(model), torch.float32)
    keys = list(model.state_dict().keys())
    params = list(model.parameters())
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    assert ta.use_hip_attention(model) == 3 and ta.use_hip_attention(model) == 0
    assert all(isinstance(layer.attention, ta.LinearAttention) for layer in model.layers)
    assert list(model.state_dict().keys()) == keys and all(a is b for a, b in zip(model.parameters(), params))
    got = run(model, torch.float32)
    names = ["y"] + ["d " + n for n, _ in model.named_parameters()]
    assert len(got) == len(ref) == len(names) == 1 + 3 * 10
    _check("stack d128 h8 x3, N2 L300", got, ref, t32, names=names)
    before = [p.detach().clone() for p in params]
    opt.step()
    assert all(bool(torch.isfinite(p).all()) and not torch.equal(p, b) for p, b in zip(params, before))
