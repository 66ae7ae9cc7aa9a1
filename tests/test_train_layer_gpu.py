"""mickey_amd.train_layer on the GPU: the whole trainable EncoderLayer (forward and all twelve gradients), its single ops, the
module and the swap.

The yardstick is encoder_layer_formula (the in-repo restatement of att_layers/transformer_utils.py:51-66, checked against the
reference's own fp64 autograd by tests/test_train_layer_cpu.py) under fp64 autograd on the device, on the same inputs.  For the
output and every gradient

    e = max |x - x64| / max |x64|   <=   max(2 * e_torch32, 2e-6)

e_torch32 = the same error of the same formula run by torch in fp32 on the same GPU; 2e-6 = the project's fp32-grade bound
(DESIGN.md section 4).  Every measured figure goes to profiles/train_layer_parity.txt.

The ReLU: a pre-activation that is zero to rounding may take either mask, and one flipped unit moves a gradient by far more than
2e-6.  Whole-layer gradient parity therefore runs on inputs whose fp64 pre-activations satisfy min |[x | m] W1^T| >= 1e-5 (about ten
times the fp32 error of a 256-term product at these magnitudes): xavier weights, unit-normal inputs, LayerNorm affine
1 + 0.1 randn / 0.1 randn, the first seed of range(64) that qualifies; the test FAILS if none does.  No element is left out of any
comparison.  A weight gradient sums rows in chunks of 128 x ceil(steps / 32) rows: 600 rows (3, 200) are 5 chunks with a ragged
last one, 3876 rows (the per-op cases) 31.

The case L = S = 1 is ill-conditioned for the gradients of wq and wk, as it is for gQ and gK of the attention alone (tests/
test_train_attention_gpu.py): with one key the output does not depend on q or k except through eps, and any fp32 evaluation returns
the rounding noise of two cancelling terms.  Measured: e_hip 0.93 (gwq), 3.60 (gwk) against e_torch32 2.64, 2.57 -- both are noise;
the rule is applied to it as to every case."""
import copy
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FLOOR = 2e-6
MARGIN = 1e-5
WEIGHTS = ("wq", "wk", "wv", "wm", "w1", "w2", "ln1_w", "ln1_b", "ln2_w", "ln2_b")
RESULTS = []
NOTES = []
_CASES = {}


@pytest.fixture(scope="module")
def tl():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from mickey_amd import train_layer
    yield train_layer
    if RESULTS:
        try:
            with open(os.path.join(ROOT, "profiles", "train_layer_parity.txt"), "w") as f:
                f.write("# tests/test_train_layer_gpu.py: max |x - x64| / max |x64| against encoder_layer_formula (or F.linear / F.layer_norm)\n")
                f.write("# under fp64 autograd; bound: max(2 * e_torch32, 2e-6), e_torch32 = the same formula in torch fp32 on the same GPU\n")
                f.write("# %-40s %-22s %12s %12s %12s\n" % ("case", "tensor", "e_hip", "e_torch32", "bound"))
                for r in RESULTS:
                    f.write("%-42s %-22s %12.3e %12.3e %12.3e\n" % r)
                for n in NOTES:
                    f.write("# %s\n" % n)
        except OSError:
            pass   # a read-only checkout: the assertions have run all the same


def load_golden():
    z = dict(np.load(os.path.join(GOLDEN, "encoder_layer_grad.npz")))
    for tag in ("self", "cross"):
        for part in ("proj", "mlp"):
            z.update(np.load(os.path.join(GOLDEN, "encoder_layer_grad_%s_%s.npz" % (tag, part))))
    return z


def _err(a, ref):
    ref = ref.detach().double().cpu()
    return float((a.detach().double().cpu() - ref).abs().max() / ref.abs().max())


def _check(case, names, got, ref, t32):
    """Prints and records every figure, then asserts the bound of the module docstring."""
    assert len(names) == len(got) == len(ref) == len(t32)
    rows = []
    for name, g, r, t in zip(names, got, ref, t32):
        assert g.shape == r.shape and g.dtype == torch.float32, (case, name)
        e_hip, e_t = _err(g, r), _err(t, r)
        rows.append((case, name, e_hip, e_t, max(2 * e_t, FLOOR)))
        print("%s %s: e_hip %.3e  e_torch32 %.3e  bound %.3e" % rows[-1])
    RESULTS.extend(rows)
    for case, name, e_hip, e_t, bound in rows:
        assert e_hip <= bound, (case, name, e_hip, e_t, bound)


def _draw(N, L, S, seed):
    """(x, source or None, the ten parameters, go) on the CPU: xavier weights, unit-normal inputs, affine 1 + 0.1 randn / 0.1 randn"""
    g = torch.Generator().manual_seed(seed)
    w = []
    for shape in ((128, 128),) * 4 + ((256, 256), (128, 256)):
        bound = (6.0 / (shape[0] + shape[1])) ** 0.5
        w.append((torch.rand(shape, generator=g) * 2 - 1) * bound)
    for _ in range(2):
        w.append(1 + 0.1 * torch.randn(128, generator=g))
        w.append(0.1 * torch.randn(128, generator=g))
    x = torch.randn((N, L, 128), generator=g)
    src = None if S is None else torch.randn((N, S, 128), generator=g)
    go = torch.randn((N, L, 128), generator=g)
    return x, src, w, go


def _preact_margin(tl, x, src, w):
    """min |[x | m] W1^T| of the layer in fp64"""
    x, w = x.double(), [t.double() for t in w]
    src = x if src is None else src.double()
    N, L, _ = x.shape
    q, k, v = (F.linear(t, ww).view(N, -1, 8, 16) for t, ww in ((x, w[0]), (src, w[1]), (src, w[2])))
    from mickey_amd.train_attention import linear_attention_formula
    m = F.layer_norm(F.linear(linear_attention_formula(q, k, v, 1e-6).reshape(N, L, 128), w[3]), (128,), w[6], w[7], 1e-5)
    return float(F.linear(torch.cat([x, m], dim=2), w[4]).abs().min())


def _case(tl, N, L, S):
    """The first seed of range(64) whose fp64 pre-activations keep MARGIN from zero, on the device, with both references; computed
    once per shape and shared (nothing in it is modified)."""
    key = (N, L, S)
    if key not in _CASES:
        for seed in range(64):
            x, src, w, go = _draw(N, L, S, seed)
            if _preact_margin(tl, x.cuda(), None if src is None else src.cuda(), [t.cuda() for t in w]) >= MARGIN:
                break
        else:
            pytest.fail("no seed of range(64) keeps the ReLU's pre-activations %g from zero at %s" % (MARGIN, key))
        ins = (x.cuda(), None if src is None else src.cuda(), [t.cuda() for t in w], go.cuda())
        _CASES[key] = (seed, ins, _formula(tl, *ins, torch.float64), _formula(tl, *ins, torch.float32))
    return _CASES[key]


def _names(src):
    return ("out", "gx") + (() if src is None else ("gsource",)) + tuple("g" + n for n in WEIGHTS)


def _formula(tl, x, src, w, go, dtype):
    xd = x.detach().to(dtype).requires_grad_(True)
    sd = None if src is None else src.detach().to(dtype).requires_grad_(True)
    wd = [t.detach().to(dtype).requires_grad_(True) for t in w]
    out = tl.encoder_layer_formula(xd, xd if sd is None else sd, *wd)
    return (out.detach(),) + tuple(torch.autograd.grad(out, [xd] + ([] if sd is None else [sd]) + wd, go.to(dtype)))


def _hip(tl, x, src, w, go, need_x=True, need_w=True):
    """(out, gx, [gsource], the ten parameter gradients); None where not asked for"""
    xd = x.detach().requires_grad_(need_x)
    sd = None if src is None else src.detach().requires_grad_(need_x)
    wd = [t.detach().requires_grad_(need_w) for t in w]
    out = tl.encoder_layer_train(xd, xd if sd is None else sd, *wd)
    assert out.shape == x.shape and out.dtype == torch.float32 and out.is_contiguous()
    ins = ([xd] + ([] if sd is None else [sd]) if need_x else []) + (wd if need_w else [])
    grads = iter(torch.autograd.grad(out, ins, go))
    res = [out.detach()]
    for t in [xd] + ([] if sd is None else [sd]) + wd:
        res.append(next(grads) if t.requires_grad else None)
    return tuple(res)


# ---- 1: the whole layer ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,L,S", [(1, 1, None), (2, 37, 29), (3, 200, None), (1, 130, 333),
                                   (1, 65, None), (2, 129, 63), (1, 64, 128)])   # L, S at the edges of the 64-token chunks
def test_layer_parity_per_shape(tl, N, L, S):
    seed, ins, ref, t32 = _case(tl, N, L, S)
    got = _hip(tl, *ins)
    _check("N%d L%d S%s seed %d" % (N, L, "self" if S is None else S, seed), _names(ins[1]), got, ref, t32)


@pytest.mark.parametrize("tag", ["self", "cross"])
def test_layer_parity_on_the_golden_fixture(tl, tag):
    z = load_golden()
    x, go = torch.from_numpy(z["x_" + tag]).cuda(), torch.from_numpy(z["go_" + tag]).cuda()
    src = None if tag == "self" else torch.from_numpy(z["source_" + tag]).cuda()
    w = [torch.from_numpy(z[n]).cuda() for n in WEIGHTS]
    got = _hip(tl, x, src, w, go)
    ref, t32 = _formula(tl, x, src, w, go, torch.float64), _formula(tl, x, src, w, go, torch.float32)
    names = _names(src)
    _check("golden " + tag, names, got, ref, t32)
    stored = tuple(torch.from_numpy(z["%s_%s" % (n, tag)]) for n in names)   # what the reference's own autograd stored
    _check("golden " + tag, tuple(n + " (stored)" for n in names), got, stored, t32)


# ---- 2: the single ops -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,K,N", [(1, 128, 128), (75, 128, 384), (3876, 256, 256), (3876, 256, 128)])
def test_linear_train_parity(tl, M, K, N):
    g = torch.Generator().manual_seed(M + K + N)
    x, go = torch.randn((M, K), generator=g).cuda(), torch.randn((M, N), generator=g).cuda()
    w = ((torch.rand((N, K), generator=g) * 2 - 1) * (6.0 / (N + K)) ** 0.5).cuda()

    def run(fn, dtype):
        a, b = x.to(dtype).requires_grad_(True), w.to(dtype).requires_grad_(True)
        y = fn(a, b)
        return (y.detach(),) + tuple(torch.autograd.grad(y, (a, b), go.to(dtype)))
    _check("linear_train M%d K%d N%d" % (M, K, N), ("out", "gx", "gw"), run(tl.linear_train, torch.float32), run(F.linear, torch.float64),
           run(F.linear, torch.float32))


@pytest.mark.parametrize("M", [1, 75, 3876])
def test_layernorm_train_parity(tl, M):
    g = torch.Generator().manual_seed(M)
    x, go = (torch.randn((M, 128), generator=g) * 1.5 + 0.3).cuda(), torch.randn((M, 128), generator=g).cuda()
    w, b = (1 + 0.1 * torch.randn(128, generator=g)).cuda(), (0.1 * torch.randn(128, generator=g)).cuda()

    def run(fn, dtype):
        a = [t.to(dtype).requires_grad_(True) for t in (x, w, b)]
        y = fn(*a)
        return (y.detach(),) + tuple(torch.autograd.grad(y, a, go.to(dtype)))
    torch_ln = lambda a, ww, bb: F.layer_norm(a, (128,), ww, bb, 1e-5)   # noqa: E731
    _check("layernorm_train M%d" % M, ("out", "gx", "gweight", "gbias"), run(lambda a, ww, bb: tl.layernorm_train(a, ww, bb, 1e-5), torch.float32),
           run(torch_ln, torch.float64), run(torch_ln, torch.float32))


# ---- 3: forward at a training size ---------------------------------------------------------------------------------------------
def test_forward_at_two_images_of_1938_tokens(tl):
    x, _, w, _ = _draw(2, 1938, None, 3)
    x, w = x.cuda(), [t.cuda() for t in w]
    with torch.no_grad():
        out = tl.encoder_layer_train(x, x, *w)
        again = tl.encoder_layer_train(x, x, *w)
        x0 = x[:1].clone()
        alone = tl.encoder_layer_train(x0, x0, *w)
        ref = tl.encoder_layer_formula(x.double(), x.double(), *[t.double() for t in w])
        t32 = tl.encoder_layer_formula(x, x, *w)
    _check("forward N2 L1938 self", ("out",), (out,), (ref,), (t32,))
    assert torch.equal(out, again)
    assert torch.equal(out[:1], alone)   # image 0 of the batch gets the bits it gets alone


# ---- 4: properties of the backward ---------------------------------------------------------------------------------------------
def test_backward_is_deterministic_linear_and_carries_non_finite_values(tl):
    N, L, S = 2, 70, 45
    x, src, w, go = _draw(N, L, S, 11)
    x, src, w, go = x.cuda(), src.cuda(), [t.cuda() for t in w], go.cuda()
    base = _hip(tl, x, src, w, go)
    again = _hip(tl, x, src, w, go)
    for a, b in zip(base, again):
        assert torch.equal(a, b)
    for p in (-40, 20):
        s = 2.0 ** p
        got = _hip(tl, x, src, w, go * s)
        for name, u, b in zip(_names(src)[1:], got[1:], base[1:]):
            assert torch.equal(u, b * s), (p, name)   # linear in go, a power of two is exact: the scaled bits
    zero = _hip(tl, x, src, w, torch.zeros_like(go))
    for name, u in zip(_names(src)[1:], zero[1:]):
        assert float(u.abs().max()) == 0.0 and bool(torch.isfinite(u).all()), name
    fin = torch.isfinite
    for bad in (float("nan"), float("inf"), -float("inf")):
        g = go.clone()
        g[0, 3, 5] = bad   # image 0, token 3, channel 5
        got = _hip(tl, x, src, w, g)
        gx, gs = got[1], got[2]
        assert not bool(fin(gx[0, 3]).any()), bad                       # that row of gx
        for name, u in zip(WEIGHTS, got[3:]):
            assert not bool(fin(u).all()), (bad, name)                  # every weight and LayerNorm gradient sees it
        assert torch.equal(gx[1], base[1][1]) and torch.equal(gs[1], base[2][1]), bad   # image 1 is untouched
        assert bool(fin(gx[1]).all()) and bool(fin(gs[1]).all())


# ---- 5: needs_input_grad, no_grad ------------------------------------------------------------------------------------------------
def test_only_the_gradients_asked_for(tl):
    x, _, w, go = _draw(2, 70, None, 12)
    x, w, go = x.cuda(), [t.cuda() for t in w], go.cuda()
    full = _hip(tl, x, None, w, go)
    frozen = _hip(tl, x, None, w, go, need_w=False)
    assert torch.equal(frozen[1], full[1]) and all(g is None for g in frozen[2:])
    no_x = _hip(tl, x, None, w, go, need_x=False)
    assert no_x[1] is None
    for name, a, b in zip(WEIGHTS, no_x[2:], full[2:]):
        assert torch.equal(a, b), name
    # single parameters: each gradient alone has the bits of the full run
    for i in (0, 2, 4, 7, 8):
        wd = [t.detach().requires_grad_(j == i) for j, t in enumerate(w)]
        out = tl.encoder_layer_train(x, x, *wd)
        (g,) = torch.autograd.grad(out, [wd[i]], go)
        assert torch.equal(g, full[2 + i]), WEIGHTS[i]
    packed = []
    with torch.autograd.graph.saved_tensors_hooks(lambda t: packed.append(t) or t, lambda t: t):
        with torch.no_grad():
            xd = x.detach().requires_grad_(True)
            out = tl.encoder_layer_train(xd, xd, *[t.detach().requires_grad_(True) for t in w])
        assert out.grad_fn is None and not out.requires_grad
        out2 = tl.encoder_layer_train(x, x, *w)   # nothing requires a gradient
        assert out2.grad_fn is None
    assert packed == []
    assert torch.equal(out, full[0]) and torch.equal(out2, full[0])


# ---- 6: what the node keeps for backward -------------------------------------------------------------------------------------------
def _saved_bytes(fn, params):
    own = {p.untyped_storage().data_ptr() for p in params}
    seen = {}

    def pack(t):
        st = t.untyped_storage()
        if st.data_ptr() not in own:
            seen[st.data_ptr()] = st.nbytes()
        return t
    with torch.autograd.graph.saved_tensors_hooks(pack, lambda t: t):
        out = fn()
    assert out.requires_grad
    return sum(seen.values())


@pytest.mark.parametrize("N,L,S,cap", [(2, 300, None, 10.25), (2, 300, 200, 11.25)])
def test_saved_memory(tl, N, L, S, cap):
    x, src, w, _ = _draw(N, L, S, 13)
    x = x.cuda().requires_grad_(True)
    src = x if src is None else src.cuda().requires_grad_(True)
    w = [nn.Parameter(t.cuda()) for t in w]
    unit = N * L * 128 * 4
    hip = _saved_bytes(lambda: tl.encoder_layer_train(x, src, *w), w) / unit
    torch_ = _saved_bytes(lambda: tl.encoder_layer_formula(x, src, *w), w) / unit
    NOTES.append("saved for backward at N%d L%d S%s, units of rows x 128 x 4 bytes: HipEncoderLayer %.3f (cap %.2f), the formula in torch %.3f"
                 % (N, L, "self" if S is None else S, hip, cap, torch_))
    print(NOTES[-1])
    assert hip <= cap, (hip, cap)


# ---- 7: layouts ----------------------------------------------------------------------------------------------------------------
def test_layouts_give_the_contiguous_bits(tl):
    N, Hh, Ww = 2, 6, 7
    L = Hh * Ww
    x, _, w, go = _draw(N, L, None, 14)
    x, w, go = x.cuda(), [t.cuda() for t in w], go.cuda()
    base = _hip(tl, x, None, w, go)
    nchw = x.transpose(1, 2).reshape(N, 128, Hh, Ww).contiguous()
    from_nchw = nchw.flatten(2).transpose(1, 2)                                          # [N, L, 128] with stride 1 along L
    cl = nchw.contiguous(memory_format=torch.channels_last).permute(0, 2, 3, 1).reshape(N, L, 128)   # dense rows of an NHWC buffer
    buf = torch.empty(N * L * 128 + 1, device="cuda")
    off = buf[1:].view(N, L, 128)                                                        # 4 bytes into its storage
    off.copy_(x)
    wide = torch.zeros((N, L, 160), device="cuda")                                       # rows 640 bytes apart, read in place
    wide[:, :, :128] = x
    assert not from_nchw.is_contiguous() and cl.is_contiguous() and off.data_ptr() % 16 == 4
    for name, t in (("nchw view", from_nchw), ("channels_last", cl), ("offset", off), ("wide rows", wide[:, :, :128])):
        assert torch.equal(t, x), name
        got = _hip(tl, t, None, w, go)
        for a, b in zip(got, base):
            assert torch.equal(a, b), name
        assert got[1].shape == x.shape
    g_t = go.transpose(1, 2).contiguous().transpose(1, 2)                                # a strided incoming gradient
    xd = x.detach().requires_grad_(True)
    (gx,) = torch.autograd.grad(tl.encoder_layer_train(xd, xd, *w), [xd], g_t)
    assert torch.equal(gx, base[1])


# ---- 8: module and swap, end to end --------------------------------------------------------------------------------------------
class _Att(nn.Module):
    """The attribute contract of the reference's Attention(attention='linear'), none of its code."""

    def __init__(self, eps=1e-6):
        super().__init__()
        self.feature_map = lambda t: F.elu(t) + 1
        self.eps = eps
        self.attention = "linear"

    def forward(self, queries, keys, values):
        from mickey_amd.train_attention import linear_attention_formula
        return linear_attention_formula(queries, keys, values, self.eps)


class _Layer(nn.Module):
    """The attribute names of the reference's EncoderLayer; the forward is encoder_layer_formula on its own parameters."""

    def __init__(self, d=128, nhead=8):
        super().__init__()
        self.dim, self.nhead = d // nhead, nhead
        self.q_proj = nn.Linear(d, d, bias=False)
        self.k_proj = nn.Linear(d, d, bias=False)
        self.v_proj = nn.Linear(d, d, bias=False)
        self.attention = _Att()
        self.merge = nn.Linear(d, d, bias=False)
        self.mlp = nn.Sequential(nn.Linear(2 * d, 2 * d, bias=False), nn.ReLU(True), nn.Linear(2 * d, d, bias=False))
        self.norm1 = nn.LayerNorm(d)
        self.norm2 = nn.LayerNorm(d)

    def forward(self, x, source):
        N, L, C = x.shape
        q = self.q_proj(x).view(N, L, self.nhead, self.dim)
        k = self.k_proj(source).view(N, -1, self.nhead, self.dim)
        v = self.v_proj(source).view(N, -1, self.nhead, self.dim)
        m = self.norm1(self.merge(self.attention(q, k, v).reshape(N, L, C)))
        return x + self.norm2(self.mlp(torch.cat([x, m], dim=2)))


class _Stack(nn.Module):
    def __init__(self):
        super().__init__()
        self.layers = nn.ModuleList([_Layer(), _Layer(), _Layer()])

    def forward(self, x):
        for layer in self.layers:
            x = layer(x, x)
        return x


def _stack(seed):
    torch.manual_seed(seed)
    m = _Stack()
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in m.named_parameters():
            if p.dim() == 2:
                p.copy_((torch.rand(p.shape, generator=g) * 2 - 1) * (6.0 / (p.shape[0] + p.shape[1])) ** 0.5)
            elif name.endswith("weight"):
                p.copy_(1 + 0.1 * torch.randn(p.shape, generator=g))
            else:
                p.copy_(0.1 * torch.randn(p.shape, generator=g))
    x = torch.randn((2, 6 * 7, 128), generator=g)
    go = torch.randn((2, 6 * 7, 128), generator=g)
    return m, x, go


def _stack_margin(m, x):
    pre = []
    md = copy.deepcopy(m).double()
    hooks = [layer.mlp[0].register_forward_hook(lambda mod, i, o: pre.append(float(o.detach().abs().min()))) for layer in md.layers]
    with torch.no_grad():
        md(x.double())
    for h in hooks:
        h.remove()
    assert len(pre) == 3
    return min(pre)


def _run_model(m, x, go, dtype):
    m = copy.deepcopy(m).to(dtype)
    y = m(x.to(dtype))
    grads = torch.autograd.grad(y, list(m.parameters()), go.to(dtype))
    return (y.detach(),) + tuple(grads)


@pytest.mark.parametrize("attention", ["plain", "use_hip_attention before", "use_hip_attention after"])
def test_swap_end_to_end(tl, attention):
    from mickey_amd import train_attention as ta
    for seed in range(64):
        m, x, go = _stack(seed)
        if _stack_margin(m, x) >= MARGIN:
            break
    else:
        pytest.fail("no seed of range(64) keeps the pre-activations of all three layers %g from zero" % MARGIN)
    m, x, go = m.cuda(), x.cuda(), go.cuda()
    ref, t32 = _run_model(m, x, go, torch.float64), _run_model(m, x, go, torch.float32)
    keys = list(m.state_dict().keys())
    params = dict(m.named_parameters())
    assert len(params) == 30
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)   # created BEFORE the swap
    if attention == "use_hip_attention before":
        assert ta.use_hip_attention(m) == 3
    assert tl.use_hip_encoder_layers(m) == 3
    assert tl.use_hip_encoder_layers(m) == 0
    if attention == "use_hip_attention after":
        assert ta.use_hip_attention(m) == 3
        assert tl.use_hip_encoder_layers(m) == 0
    assert all(type(layer) is tl.HipEncoderLayer for layer in m.layers)
    assert list(m.state_dict().keys()) == keys
    for n, p in m.named_parameters():
        assert p is params[n], n
    y = m(x)
    y.backward(go)
    names = ("out",) + tuple("g " + n for n in params)
    _check("stack of 3, 2 x 42 tokens, seed %d, %s" % (seed, attention), names, (y.detach(),) + tuple(p.grad for p in params.values()), ref, t32)
    before = {n: p.detach().clone() for n, p in params.items()}
    opt.step()
    for n, p in params.items():
        assert bool(torch.isfinite(p).all()) and not torch.equal(p, before[n]), n
    assert len(opt.state) == 30


# ---- 9: validation ---------------------------------------------------------------------------------------------------------------
def test_bad_arguments_raise_on_the_device(tl):
    from mickey_amd import _native
    x, src, w, _ = _draw(2, 5, 7, 15)
    xc, sc, wc = x.cuda(), src.cuda(), [t.cuda() for t in w]
    for a, b, ww in ((x, sc, wc), (xc, src, wc), (xc, sc, w), (xc, sc, wc[:4] + [w[4]] + wc[5:])):
        with pytest.raises(_native.MickeyHipError):
            tl.encoder_layer_train(a, b, *ww)
    with torch.autocast("cuda", dtype=torch.float16):
        h = xc.half()
    bad = [(h, sc), (xc, sc.double()), (xc.reshape(10, 128), sc), (xc[:, :, :64], sc[:, :, :64]), (xc, sc[:1]), (xc[:, :0], sc), (xc, sc[:, :0]),
           (xc[:0], sc[:0])]
    for a, b in bad:
        with pytest.raises(ValueError):
            tl.encoder_layer_train(a, b, *wc)
    for i in range(10):
        with pytest.raises(ValueError):
            tl.encoder_layer_train(xc, sc, *(wc[:i] + [wc[i].double()] + wc[i + 1:]))
    for eps in (float("nan"), float("inf"), -1.0, None, True):
        with pytest.raises(ValueError):
            tl.encoder_layer_train(xc, sc, *wc, ln2_eps=eps)
    with pytest.raises(_native.MickeyHipError):
        tl.linear_train(xc, w[0])
    with pytest.raises(ValueError):
        tl.linear_train(xc, wc[5])          # K
    with pytest.raises(_native.MickeyHipError):
        tl.layernorm_train(x, wc[6], wc[7])
    with pytest.raises(ValueError):
        tl.layernorm_train(xc.double(), wc[6], wc[7])
