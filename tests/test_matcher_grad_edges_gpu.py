"""-m gpu: the matcher's backward kernels (mk_matcher_bwd.hip: sweep 1, its merge, the dustbin reduction, sweep 2 for either side,
its merge, and the log-sum merge of the training forward), ELEMENT by element against the fp64 formulas, at the smallest shapes
where a ragged 32-tile, an empty column chunk, an idle wave, a merge block or a batch offset can go wrong -- with every output,
`lse` and `work` inside guard rows (tests/helpers/guarded.py) and `work` full of the sentinel, so that a store outside a buffer
or a read of a partial nobody wrote is seen.  mk_dual_softmax_train / mk_dual_softmax_bwd are called directly, as
ops.dual_softmax_train_fwd / ops.dual_softmax_bwd call them.

Metric: err = |got - g64| / M for every output element, g64 = tests/helpers/matcher_refs.py::formula_grads on .double() inputs,
M = the same expression with every term replaced by its absolute value (the gradients cancel: relative to |g| an fp32 evaluation
has no bounded error, and a norm hides single elements).  A case passes when |got - g64| <= tol * M + 2 TINY with
tol = 4 x max(floor32g, 2^-20), floor32g = the largest err of formula_grads run in fp32 on the same inputs, per output kind and
case: a property of the reference and the inputs alone (both taken over the elements with M >= TINY; below that the 2 TINY
decides).  Where M == 0 the output must be an exact zero.  The factor 4 is the forward suite's, for the same reasons (log2
domain, v_exp_f32, another summation order, no lo x lo on the split path).  The backward is fed the fp64 log-sums rounded to
fp32, so that an error shared by forward and backward cannot cancel; test_chain_forward_lse feeds it the forward kernel's own,
and so does the hot family: at its log2-domain logits of 147.7 fp32 values are 2^-16 apart, an injected lse leaves
2 v - lr - lc of the planted duplicates to the rounding of the backward's v alone (measured: err up to 1.1e-4 on g_scr, 56 x
the floor), while the forward's own log-sums carry the same rounding and it cancels (measured: 1.1 x the floor).  `lse` itself
is compared absolutely (it is a logarithm) with 4 x max(floor32_lse, 2^-20).  Measured worst cases:
profiles/matcher_grad_edges_parity.txt."""
import pytest
import torch

from mickey_amd import ops
from tests.helpers import matcher_refs as R
from tests.helpers.guarded import bits, sentinel_bits, window

pytestmark = pytest.mark.gpu

SENT = sentinel_bits(torch.float32)
CASES = R.grad_cases()
WORST = {}     # (output kind, path, family) -> (err / max(floor32g, 2^-20), err, floor32g) of the worst element seen
CHAIN_D = {}   # (n0, n1, path) -> measured max |lse_kernel - lse64|
ALL = (True, True, True, True, True)


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module", autouse=True)
def _report_worst():
    yield
    for (kind, path, family), (ratio, err, fl) in sorted(WORST.items()):
        print("matcher grad edges worst err / max(floor32g, 2^-20): %-8s %-5s %-12s %.3f  (err %.3e, floor32g %.3e; allowed %.0f)"
              % (kind, path, family, ratio, err, fl, R.FACTOR))
    for (n0, n1, path), d in sorted(CHAIN_D.items()):
        print("matcher grad edges chain d = max |lse_kernel - lse64|: %dx%d %-5s %.3e" % (n0, n1, path, d))


def _nv():
    from mickey_amd import _native
    return _native


def _path(split):
    return "split" if split else "exact"


def _written(t):
    return not bool((bits(t) == SENT).any())


def _put(dev, c, pairs=None):
    """the case's fp32 inputs on the device (of the pairs `pairs` only): d0, d1, s0, s1, G, db"""
    out = []
    for k in ("d0", "d1", "s0", "s1", "G"):
        t = c[k]
        out.append(None if t is None else (t if pairs is None else t[pairs]).contiguous().to(dev))
    return out + [None if c["db"] is None else c["db"].to(dev)]


# ---- calling the entry points on guarded buffers ------------------------------------------------------------------------------
def _forward(split, d0, d1, s0, s1, db):
    """mk_dual_softmax_train -> (output [B, n0, n1] (final_scores, or scores without s0 / s1), lse [B, 2, nmax]); output, lse and
    work in guarded windows, every guard checked, the output and the used slots of lse found fully overwritten."""
    nv = _nv()
    dev = d0.device
    B, C, n0 = d0.shape
    n1 = d1.shape[2]
    nmax = max(n0, n1)
    out, c_out = window(B * n0, n1, dev)
    lse, c_lse = window(B * 2, nmax, dev)
    work, c_work = window(1, nv.query("mk_dual_softmax_train_work_floats", B, n0, n1, int(split)), dev)
    has_kp = s0 is not None
    nv.call("mk_dual_softmax_train", nv.ptr(d0), nv.ptr(d1), nv.ptr(s0), nv.ptr(s1), 1.0 / R.TEMPERATURE, nv.ptr(db),
            None if has_kp else nv.ptr(out), None, nv.ptr(out) if has_kp else None, nv.ptr(lse), nv.ptr(work), B, C, n0, n1, int(split),
            nv.stream())
    torch.cuda.synchronize()
    for chk in (c_out, c_lse, c_work):
        chk()
    lse = lse.view(B, 2, nmax)
    assert _written(out), "the forward output: elements left unwritten"
    assert _written(lse[:, 0, :n0]) and _written(lse[:, 1, :n1]), "lse: used slots left unwritten"
    return out.view(B, n0, n1), lse


def _backward(split, d0, d1, s0, s1, db, lse, G, want=ALL, shift=0, work_fill=None):
    """mk_dual_softmax_bwd -> [g_dsc0 [B, 128, n0], g_dsc1 [B, 128, n1], g_scr0 [B, n0], g_scr1 [B, n1], g_dustbin [B]] (None where
    not wanted: passed as null).  Every output and `work` (sentinel-filled, or work_fill) in guarded windows; after the call every
    guard is checked and every wanted output found fully overwritten."""
    nv = _nv()
    dev = d0.device
    B, C, n0 = d0.shape
    n1 = d1.shape[2]
    want = [w and ok for w, ok in zip(want, (True, True, s0 is not None, s0 is not None, db is not None))]
    shapes = ((B * C, n0), (B * C, n1), (B, n0), (B, n1), (1, B))
    outs, checks = [], []
    for w, (rows, cols) in zip(want, shapes):
        o, chk = window(rows, cols, dev, shift) if w else (None, None)
        outs.append(o)
        if w:
            checks.append(chk)
    work, chk = window(1, nv.query("mk_dual_softmax_bwd_work_floats", B, n0, n1, int(split)), dev)
    checks.append(chk)
    if work_fill is not None:
        work.fill_(work_fill)
    nv.call("mk_dual_softmax_bwd", nv.ptr(d0), nv.ptr(d1), nv.ptr(s0), nv.ptr(s1), 1.0 / R.TEMPERATURE, nv.ptr(db), nv.ptr(lse), nv.ptr(G),
            *[nv.ptr(o) for o in outs], nv.ptr(work), B, C, n0, n1, int(split), nv.stream())
    torch.cuda.synchronize()
    for chk in checks:
        chk()
    full = ((B, C, n0), (B, C, n1), (B, n0), (B, n1), (B,))
    for o, name in zip(outs, R.GRAD_KINDS):
        assert o is None or _written(o), "g_%s: elements left unwritten" % name
    return [None if o is None else o.view(sh) for o, sh in zip(outs, full)]


def _lse_in(c, dev, pairs=None):
    """the fp64 log-sums rounded to fp32, on the device: what the backward is fed"""
    l = c["lse64"] if pairs is None else c["lse64"][pairs]
    return l.float().contiguous().to(dev)


# ---- the metric ---------------------------------------------------------------------------------------------------------------
def _where(kind, shape, i, got, ref):
    idx = []
    for s in reversed(shape):
        idx.append(i % s)
        i //= s
    idx = idx[::-1]
    k = idx[-1]
    if kind == "dustbin":
        pos = "pair %d" % idx[0]
    elif len(shape) == 3:
        pos = "pair %d, channel %d, keypoint %d = position %d of its 32-tile" % (idx[0], idx[1], k, k % 32)
    else:
        pos = "pair %d, keypoint %d = position %d of its 32-tile" % (idx[0], k, k % 32)
    return "%s: got %r, fp64 %r" % (pos, float(got), float(ref))


def _metric(kind, path, family, got, g64, M, floor, what, extra=0.0):
    """The element-wise metric of the module docstring for one output (got: device or CPU tensor; g64, M: fp64, CPU).  extra is
    added to the relative tolerance (matcher_refs.lse_term)."""
    got = got.detach().double().cpu().reshape(g64.shape)
    flat, ref, Mf = got.reshape(-1), g64.reshape(-1), M.reshape(-1)
    name = "g_%s (%s, %s)" % (kind, path, what)
    finite = torch.isfinite(flat)
    if not bool(finite.all()):
        i = int(torch.nonzero(~finite)[0])
        raise AssertionError("%s: %d non-finite outputs, first at %s" % (name, int((~finite).sum()), _where(kind, g64.shape, i, flat[i], ref[i])))
    zero = (Mf == 0) & (flat != 0)
    if bool(zero.any()):
        i = int(torch.nonzero(zero)[0])
        raise AssertionError("%s: %d non-zero outputs where every term of the sum is zero, first at %s"
                             % (name, int(zero.sum()), _where(kind, g64.shape, i, flat[i], ref[i])))
    diff = (flat - ref).abs()
    err = torch.where(Mf >= R.TINY, diff / Mf.clamp_min(R.TINY), torch.zeros_like(diff))   # (below TINY: the absolute 2 TINY)
    worst, fl = float(err.max()), max(floor, R.SPACING)
    tol = R.FACTOR * fl + extra
    key = (kind, path, family + (" own lse" if extra else ""))   # (with the forward's lse: err over tol / 4, the term for d included)
    if key not in WORST or worst * R.FACTOR / tol > WORST[key][0]:
        WORST[key] = (worst * R.FACTOR / tol, worst, floor)
    bad = ~(diff <= tol * Mf + 2 * R.TINY)
    if bool(bad.any()):
        i = int(torch.where(bad, err, torch.full_like(err, -1.0)).argmax())
        raise AssertionError("%s: err / max(floor32g, 2^-20) = %.3f > %.0f (err = |got - fp64| / M = %.3e, floor32g %.3e%s) at %s, M %r; "
                             "%d of %d elements outside" % (name, float(err[i]) / fl, R.FACTOR, float(err[i]), floor,
                                                            ", + %.3e for lse" % extra if extra else "",
                                                            _where(kind, g64.shape, i, flat[i], ref[i]), float(Mf[i]), int(bad.sum()), bad.numel()))


def _check_grads(path, family, c, got, what, extra=0.0, pairs=None):
    for k, kind in enumerate(R.GRAD_KINDS):
        if got[k] is None:
            continue
        g64, M = (c["g64"][k], c["M"][k]) if pairs is None else (c["g64"][k][pairs], c["M"][k][pairs])
        _metric(kind, path, family, got[k], g64, M, c["floor"][k], what, extra)


def _same(a, b, what):
    """bit-identical outputs; names the first differing element"""
    assert (a is None) == (b is None), what
    if a is None:
        return
    ne = bits(a.reshape(b.shape)) != bits(b)
    if bool(ne.any()):
        i = torch.nonzero(ne)[0].tolist()
        raise AssertionError("%s: %d of %d elements differ, first at index %r (position %d of its 32-tile)"
                             % (what, int(ne.sum()), ne.numel(), i, i[-1] % 32))


def _same_all(got, ref, what):
    for g, r, kind in zip(got, ref, R.GRAD_KINDS):
        _same(g, r, "%s: g_%s" % (what, kind))


# ---- the tests ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n0,n1,split,db", CASES["test_backward_elementwise"])
def test_backward_elementwise(n0, n1, split, db):
    """B = 2, dense G, scores with planted zeros, lse injected: all five gradients; then scr0 = scr1 = null (g_scr null): the
    descriptor and dustbin gradients against the reference with s = 1."""
    dev = _dev()
    what = "unit n0=%d n1=%d dustbin=%r" % (n0, n1, db)
    c = R.grad_case("unit", 2, n0, n1, db, "dense")
    d0, d1, s0, s1, G, dbt = _put(dev, c)
    got = _backward(split, d0, d1, s0, s1, dbt, _lse_in(c, dev), G)
    assert [g is not None for g in got] == [True, True, True, True, db is not None]
    _check_grads(_path(split), "unit", c, got, what)
    c1 = R.grad_case("unit", 2, n0, n1, db, "dense", False)
    got = _backward(split, d0, d1, None, None, dbt, _lse_in(c1, dev), G)
    assert [g is not None for g in got] == [True, True, False, False, db is not None]
    _check_grads(_path(split), "unit", c1, got, what + " without scores")


@pytest.mark.parametrize("family,gkind,n0,n1,split", CASES["test_backward_sparse_G_and_hot"])
def test_backward_sparse_G_and_hot(family, gkind, n0, n1, split):
    """The trainer's sparse REINFORCE G (5 % of the cells, divided by final + 1e-16: rows with no cell must come out as exact
    zeros) on both paths; the hot descriptors (logits past what 2^v2 can hold without the log-sums) on the exact path."""
    dev = _dev()
    for db in R.DUSTBINS:
        c = R.grad_case(family, 2, n0, n1, db, gkind)
        d0, d1, s0, s1, G, dbt = _put(dev, c)
        what = "%s %s G n0=%d n1=%d dustbin=%r" % (family, gkind, n0, n1, db)
        if family == "hot":
            # fed the forward's lse, with the term of test_chain_forward_lse for it: matcher_refs.lse_term says why
            _, lse = _forward(split, d0, d1, s0, s1, dbt)
            d = _check_lse(c, lse, _path(split), what, family)
            got = _backward(split, d0, d1, s0, s1, dbt, lse.contiguous(), G)
            _check_grads(_path(split), family, c, got, what + ", the forward's lse", extra=R.lse_term(d))
            continue
        got = _backward(split, d0, d1, s0, s1, dbt, _lse_in(c, dev), G)
        _check_grads(_path(split), "sparse", c, got, what)


def _check_lse(c, lse, path, what, family="unit"):
    """lse [B, 2, nmax] of the forward kernel against the fp64 log-sums, absolutely, over the slots in use -> max |difference|"""
    got = lse.double().cpu()
    assert bool(torch.isfinite(got[c["used"]]).all()), what
    diff = torch.where(c["used"], (got - c["lse64"]).abs(), torch.zeros_like(got))
    d, fl = float(diff.max()), max(c["floor_lse"], R.SPACING)
    key = ("lse", path, family)
    if key not in WORST or d / fl > WORST[key][0]:
        WORST[key] = (d / fl, d, c["floor_lse"])
    if not d <= R.FACTOR * fl:
        b, side, k = torch.nonzero(diff == diff.max())[0].tolist()
        raise AssertionError("lse (%s, %s): |lse - lse64| / max(floor32_lse, 2^-20) = %.3f > %.0f (%.3e, floor32_lse %.3e) at pair %d, "
                             "side %d, keypoint %d = position %d of its 32-tile: got %r, fp64 %r"
                             % (path, what, d / fl, R.FACTOR, d, c["floor_lse"], b, side, k, k % 32, float(got[b, side, k]),
                                float(c["lse64"][b, side, k])))
    return d


@pytest.mark.parametrize("n0,n1,split,db", CASES["test_lse_elementwise"])
def test_lse_elementwise(n0, n1, split, db):
    """The log-sums mk_dual_softmax_train saves for the backward; its output is bit-equal to the inference matcher's."""
    dev = _dev()
    what = "unit n0=%d n1=%d dustbin=%r" % (n0, n1, db)
    c = R.grad_case("unit", 2, n0, n1, db, "dense")
    d0, d1, s0, s1, _, dbt = _put(dev, c)
    fin, lse = _forward(split, d0, d1, s0, s1, dbt)
    _check_lse(c, lse, _path(split), what)
    sc, lse1 = _forward(split, d0, d1, None, None, dbt)
    _same(lse1[:, 0, :n0], lse[:, 0, :n0].contiguous(), what + ": row log-sums of the scores-only call")
    _same(lse1[:, 1, :n1], lse[:, 1, :n1].contiguous(), what + ": column log-sums of the scores-only call")
    ref_sc, _, ref_fin = ops.dual_softmax(d0, d1, s0, s1, R.TEMPERATURE, float(c["db"]) if db is not None else None, want_kp=False,
                                          split=split)
    _same(fin, ref_fin, what + ": final_scores against mk_dual_softmax" + ("_split" if split else ""))
    _same(sc, ref_sc, what + ": scores against mk_dual_softmax" + ("_split" if split else ""))


@pytest.mark.parametrize("n0,n1,split", CASES["test_chain_forward_lse"])
def test_chain_forward_lse(n0, n1, split):
    """The backward fed the forward kernel's own lse.  d = max |lse_kernel - lse64| (measured here against the reference: a
    property of the backward's input) scales A or Bm by 2^-d; each term of dS holds at most one A and one Bm: + 2 ln2 d."""
    dev = _dev()
    what = "unit n0=%d n1=%d dustbin=0.7, the forward's lse" % (n0, n1)
    c = R.grad_case("unit", 2, n0, n1, 0.7, "dense")
    d0, d1, s0, s1, G, dbt = _put(dev, c)
    _, lse = _forward(split, d0, d1, s0, s1, dbt)
    d = _check_lse(c, lse, _path(split), what)
    CHAIN_D[(n0, n1, _path(split))] = d
    got = _backward(split, d0, d1, s0, s1, dbt, lse.contiguous(), G)
    _check_grads(_path(split), "unit", c, got, what, extra=R.lse_term(d))


@pytest.mark.parametrize("n0,n1,split", CASES["test_unused_lse_slots_and_dirty_work"])
def test_unused_lse_slots_and_dirty_work(n0, n1, split):
    """NaN in lse[:, side, n:nmax] and `work` full of NaN: bit-identical to the clean call (whose `work` holds the sentinel)."""
    dev = _dev()
    c = R.grad_case("unit", 2, n0, n1, 0.7, "dense")
    d0, d1, s0, s1, G, dbt = _put(dev, c)
    lse = _lse_in(c, dev)
    clean = _backward(split, d0, d1, s0, s1, dbt, lse, G, work_fill=0.0)
    _check_grads(_path(split), "unit", c, clean, "unit n0=%d n1=%d, work zeroed" % (n0, n1))
    dirty = lse.clone()
    dirty[:, 0, n0:] = float("nan")
    dirty[:, 1, n1:] = float("nan")
    assert int(torch.isnan(dirty).sum()) == 2 * abs(n0 - n1)
    for fill in (None, float("nan")):
        got = _backward(split, d0, d1, s0, s1, dbt, dirty, G, work_fill=fill)
        _same_all(got, clean, "n0=%d n1=%d, NaN in the unused lse slots, work filled with %s" % (n0, n1, "the sentinel" if fill is None else "NaN"))


@pytest.mark.parametrize("B,n0,n1,split", CASES["test_batches"])
def test_batches(B, n0, n1, split):
    """B = 1 and B = 8, 9 (either branch of decode_unit_grid, 9 padded to 16 units): the metric for every pair, and pair p of the
    batch bit-identical to pair p alone."""
    dev = _dev()
    what = "unit B=%d n0=%d n1=%d dustbin=0.7" % (B, n0, n1)
    c = R.grad_case("unit", B, n0, n1, 0.7, "dense")
    d0, d1, s0, s1, G, dbt = _put(dev, c)
    full = _backward(split, d0, d1, s0, s1, dbt, _lse_in(c, dev), G)
    _check_grads(_path(split), "unit", c, full, what)
    for p in range(B if B > 1 else 0):
        pr = slice(p, p + 1)
        e0, e1, t0, t1, Gp, _ = _put(dev, c, pr)
        one = _backward(split, e0, e1, t0, t1, dbt, _lse_in(c, dev, pr), Gp)
        _same_all(one, [f[pr] for f in full], "%s: pair %d alone against the batch" % (what, p))


@pytest.mark.parametrize("B,n0,n1,split", CASES["test_pair_isolation"])
def test_pair_isolation(B, n0, n1, split):
    """Pair 1's G all NaN: pairs 0 and 2 bit-identical to the clean call, pair 1 non-finite everywhere."""
    dev = _dev()
    c = R.grad_case("unit", B, n0, n1, 0.7, "dense")
    d0, d1, s0, s1, G, dbt = _put(dev, c)
    lse = _lse_in(c, dev)
    clean = _backward(split, d0, d1, s0, s1, dbt, lse, G)
    Gn = G.clone()
    Gn[1] = float("nan")
    got = _backward(split, d0, d1, s0, s1, dbt, lse, Gn)
    for g, r, kind in zip(got, clean, R.GRAD_KINDS):
        for p in (0, 2):
            _same(g[p:p + 1], r[p:p + 1], "NaN in pair 1's G: g_%s of pair %d" % (kind, p))
        assert not bool(torch.isfinite(g[1]).any()), "g_%s of the pair whose G is NaN has finite elements" % kind


@pytest.mark.parametrize("n0,n1,split", CASES["test_output_subsets"])
def test_output_subsets(n0, n1, split):
    """g_dsc0 alone, g_dsc1 alone, the two score gradients alone, g_dustbin alone (every other pointer null): bit-identical to
    the full call."""
    dev = _dev()
    c = R.grad_case("unit", 2, n0, n1, 0.7, "dense")
    d0, d1, s0, s1, G, dbt = _put(dev, c)
    lse = _lse_in(c, dev)
    full = _backward(split, d0, d1, s0, s1, dbt, lse, G)
    _check_grads(_path(split), "unit", c, full, "unit n0=%d n1=%d" % (n0, n1))
    for want in R.GRAD_SUBSETS:
        got = _backward(split, d0, d1, s0, s1, dbt, lse, G, want=want)
        assert [g is not None for g in got] == list(want)
        _same_all(got, [f if w else None for f, w in zip(full, want)], "outputs %r alone against the full call" % (want,))


@pytest.mark.parametrize("n0,n1,split", CASES["test_misaligned_outputs"])
def test_misaligned_outputs(n0, n1, split):
    """The five outputs 4 and 8 bytes off a 16-byte boundary: bit-identical to the aligned call, neighbours untouched."""
    dev = _dev()
    c = R.grad_case("unit", 2, n0, n1, 0.7, "dense")
    d0, d1, s0, s1, G, dbt = _put(dev, c)
    lse = _lse_in(c, dev)
    full = _backward(split, d0, d1, s0, s1, dbt, lse, G)
    _check_grads(_path(split), "unit", c, full, "unit n0=%d n1=%d" % (n0, n1))
    for shift in (1, 2):
        got = _backward(split, d0, d1, s0, s1, dbt, lse, G, shift=shift)
        _same_all(got, full, "outputs %d floats past a 16-byte boundary against the aligned call" % shift)
