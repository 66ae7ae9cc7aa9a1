"""-m gpu: the matcher's forward kernels (mk_matcher.hip: exact-fp32 and split-fp16 dual softmax, Sinkhorn, mutual-NN), ELEMENT by
element against the fp64 oracle, at the smallest shapes where a ragged 32-tile, a chunk boundary, a store width or a batch offset
can go wrong -- with every output, `work`, `matches` and `count` inside guard rows (tests/helpers/guarded.py), so that a store
outside a buffer is seen.  The entry points are called directly, as ops.dual_softmax / ops.sinkhorn / ops.mutual_nn call them.

Metric (dual softmax, Sinkhorn): rel = |P - P64| / P64 wherever P64 >= 1e-30, P <= 2e-30 elsewhere, everything finite.  Tolerance
per case: 4 x max(floor32, 2^-20), floor32 = the fp32 ORACLE's own element-wise error on the same inputs (a property of the
reference: tests/helpers/matcher_refs.py; test_matcher_edges_cpu.py shows that the ordinary inputs leave no element out of the
relative comparison).  2^-20 is the spacing of a logit v2 in [8, 16).  The factor 4: against the fp32 oracle a kernel rounds once
more (scaling into the log2 domain), uses v_exp_f32 / v_log_f32 in place of libm, sums in another order and, on the split path,
drops the lo x lo term (<= 2^-22 per product); each at most doubles the reference's own error.  Measured worst cases:
profiles/matcher_edges_parity.txt.  kp_scores is scr0^T scr1 in fp32, bit for bit.

Mutual-NN is exact: count and the match list equal tests/helpers/matcher_refs.py::mutual_nn_ref (first index wins either arg-max,
equal scores in ascending row order), the rest of `matches` keeps what the test put there."""
import pytest
import torch

from tests.helpers import matcher_refs as R
from tests.helpers.guarded import bits, guarded, sentinel_bits
from tests.helpers.guarded import window as _window

pytestmark = pytest.mark.gpu

LOG2E = 1.4426950408889634
SENT = sentinel_bits(torch.float32)
PRESET = -7                 # what `matches` holds before a mutual-NN call
WORST = {}                  # (kernel, input family) -> (rel / max(floor32, 2^-20), rel, floor32) of the worst element seen


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module", autouse=True)
def _report_worst():
    yield
    for (kernel, family), (ratio, rel, fl) in sorted(WORST.items()):
        print("matcher edges worst rel / max(floor32, 2^-20): %-28s %-5s %.3f  (rel %.3e, floor32 %.3e; allowed %.0f)"
              % (kernel, family, ratio, rel, fl, R.FACTOR))


def _nv():
    from mickey_amd import _native
    return _native


def _written(t):
    return not bool((bits(t) == SENT).any())


def _metric(kernel, family, got, ref64, floor, what):
    """The element-wise metric of the module docstring; got [B, n0, n1] (any device), ref64 fp64 on the CPU."""
    got = got.detach().double().cpu().reshape(ref64.shape)
    B, n0, n1 = ref64.shape

    def where(i):
        b, r, c = i // (n0 * n1), (i // n1) % n0, i % n1
        return "pair %d, row %d, column %d = position (%d, %d) of its 32-tile: got %r, fp64 %r" % (
            b, r, c, r % 32, c % 32, float(got.reshape(-1)[i]), float(ref64.reshape(-1)[i]))

    finite = torch.isfinite(got)
    if not bool(finite.all()):
        raise AssertionError("%s, %s: %d non-finite outputs, first at %s" % (kernel, what, int((~finite).sum()),
                                                                            where(int(torch.nonzero(~finite.reshape(-1))[0]))))
    big = ref64 >= R.TINY
    rel = torch.where(big, (got - ref64).abs() / ref64.clamp_min(R.TINY), torch.zeros_like(got))
    worst = float(rel.max())
    fl = max(floor, R.SPACING)
    key = (kernel, family)
    if key not in WORST or worst / fl > WORST[key][0]:
        WORST[key] = (worst / fl, worst, floor)
    if not worst / fl <= R.FACTOR:
        raise AssertionError("%s, %s: rel / max(floor32, 2^-20) = %.3f > %.0f (rel %.3e, floor32 %.3e) at %s; %d of %d elements "
                             "outside" % (kernel, what, worst / fl, R.FACTOR, worst, floor, where(int(rel.argmax())),
                                          int((rel > R.FACTOR * fl).sum()), rel.numel()))
    small = (~big) & ~(got <= 2 * R.TINY)
    if bool(small.any()):
        raise AssertionError("%s, %s: %d outputs above 2e-30 where the reference is below 1e-30, first at %s"
                             % (kernel, what, int(small.sum()), where(int(torch.nonzero(small.reshape(-1))[0]))))


def _same(a, b, what):
    """bit-identical [B, n0, n1] outputs; names the first differing element"""
    ne = bits(a.reshape(b.shape)) != bits(b)
    if bool(ne.any()):
        i = torch.nonzero(ne)[0].tolist()
        raise AssertionError("%s: %d of %d elements differ, first at pair %d, row %d, column %d = position (%d, %d) of its 32-tile"
                             % (what, int(ne.sum()), ne.numel(), i[0], i[1], i[2], i[1] % 32, i[2] % 32))


# ---- calling the entry points on guarded buffers ------------------------------------------------------------------------------
def _outputs(want, B, n0, n1, dev, shift=0):
    """One [B * n0, n1] window per wanted output, None (passed as null) for the others -> (outputs, their checks)"""
    outs, checks = [], []
    for w in want:
        o, chk = _window(B * n0, n1, dev, shift) if w else (None, None)
        outs.append(o)
        if w:
            checks.append(chk)
    return outs, checks


def _finish(outs, checks, B, n0, n1):
    """after a call: every guard intact, every wanted output fully overwritten -> the outputs as [B, n0, n1]"""
    torch.cuda.synchronize()
    for chk in checks:
        chk()
    for o, name in zip(outs, ("scores", "kp_scores", "final_scores")):
        assert o is None or _written(o), "%s: elements left unwritten" % name
    return [None if o is None else o.view(B, n0, n1) for o in outs]


def _dual_softmax(split, d0, d1, s0, s1, dustbin, want=(True, True, True), shift=0, scr1_shift=0):
    """mk_dual_softmax / mk_dual_softmax_split on device inputs.  want: (scores, kp_scores, final_scores); an output not wanted
    is passed as null; s0 = s1 = None: null scr.  -> [scores, kp, final] as [B, n0, n1] device tensors (None where not wanted),
    after every guard was checked and every wanted output found fully overwritten."""
    nv = _nv()
    dev = d0.device
    B, C, n0 = d0.shape
    n1 = d1.shape[2]
    outs, checks = _outputs(want, B, n0, n1, dev, shift)
    if split:
        nwork = nv.query("mk_dual_softmax_split_work_floats", B, n0, n1)
    else:
        nwork = nv.query("mk_dual_softmax_work_floats", B, n0, n1, int(not want[0] and not want[2]))
    work, chk = _window(1, nwork, dev)
    checks.append(chk)
    if s1 is not None and scr1_shift:
        buf = torch.empty((s1.numel() + scr1_shift,), device=dev, dtype=torch.float32)
        buf[scr1_shift:].copy_(s1.reshape(-1))
        s1 = buf[scr1_shift:]
        assert s1.data_ptr() % 8 == 4
    nv.call("mk_dual_softmax_split" if split else "mk_dual_softmax", nv.ptr(d0), nv.ptr(d1), nv.ptr(s0), nv.ptr(s1), 1.0 / R.TEMPERATURE,
            int(dustbin is not None), float(dustbin) if dustbin is not None else 0.0, nv.ptr(outs[0]), nv.ptr(outs[1]), nv.ptr(outs[2]),
            nv.ptr(work), B, C, n0, n1, nv.stream())
    return _finish(outs, checks, B, n0, n1)


def _sinkhorn(d0, d1, s0, s1, alpha, iters, want=(True, True, True)):
    """mk_sinkhorn likewise -> ([scores, kp, final], u [B, n0 + 1], v [B, ldz]) with u, v read back from `work` (log2 domain;
    layout Z, u, v, part as in sinkhorn_impl)."""
    nv = _nv()
    dev = d0.device
    B, C, n0 = d0.shape
    n1 = d1.shape[2]
    outs, checks = _outputs(want, B, n0, n1, dev)
    work, chk = _window(1, nv.query("mk_sinkhorn_work_floats", B, n0, n1), dev)
    checks.append(chk)
    nv.call("mk_sinkhorn", nv.ptr(d0), nv.ptr(d1), nv.ptr(s0), nv.ptr(s1), float(alpha), int(iters), nv.ptr(outs[0]), nv.ptr(outs[1]),
            nv.ptr(outs[2]), nv.ptr(work), B, C, n0, n1, nv.stream())
    outs = _finish(outs, checks, B, n0, n1)
    ldz, ldu = (n1 + 1 + 3) // 4 * 4, (n0 + 1 + 3) // 4 * 4
    ou = B * (n0 + 1) * ldz
    u = work[ou:ou + B * ldu].view(B, ldu)[:, :n0 + 1]
    v = work[ou + B * ldu:ou + B * ldu + B * ldz].view(B, ldz)
    assert _written(work[:ou + B * ldu + B * ldz]), "Z, u or v: elements left unwritten"
    return outs, u.cpu(), v.cpu()


def _to(dev, c, pairs=None):
    ts = [c[k] if pairs is None else c[k][pairs] for k in ("d0", "d1", "s0", "s1")]
    return [t.contiguous().to(dev) for t in ts]


def _check_full(kernel, family, c, outs, what):
    sc, kp, fin = outs
    _metric(kernel, family, sc, c["P64"], c["floor"], what + " scores")
    assert torch.equal(kp.cpu(), c["kp32"]), what + ": kp_scores is not scr0^T scr1 in fp32"
    _metric(kernel + " final", family, fin, c["F64"], c["floor_final"], what + " final_scores")


# ---- dual softmax ---------------------------------------------------------------------------------------------------------------
def _ds_name(split):
    return "dual_softmax " + ("split" if split else "exact")


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("n0,n1", R.DS_SHAPES)
def test_dual_softmax_elementwise(n0, n1, split):
    """B = 2, C = 128, dustbin none / 0.7 / 8.0 (at 8.0 a dustbin term lost on either side is a large relative error); the hot family
    on the exact path.  All three outputs, then scores only (null scr), final only (exact path: computed in place in `final`) and
    kp only (exact path: the stored correlation lives in the own_copy region of `work`) -- each bit-identical to the full call."""
    dev = _dev()
    for family in ("unit", "hot") if (not split and (n0, n1) in R.DS_HOT_SHAPES) else ("unit",):
        for db in R.DUSTBINS:
            c = R.dual_softmax_case(family, 2, 128, n0, n1, db)
            d0, d1, s0, s1 = _to(dev, c)
            what = "%s n0=%d n1=%d dustbin=%r" % (family, n0, n1, db)
            full = _dual_softmax(split, d0, d1, s0, s1, db)
            _check_full(_ds_name(split), family, c, full, what)
            sc = _dual_softmax(split, d0, d1, None, None, db, want=(True, False, False))
            _same(sc[0], full[0], what + ": scores of the scores-only call")
            fin = _dual_softmax(split, d0, d1, s0, s1, db, want=(False, False, True))
            _same(fin[2], full[2], what + ": final_scores of the final-only call")
            kp = _dual_softmax(split, d0, d1, s0, s1, db, want=(False, True, False))
            _same(kp[1], full[1], what + ": kp_scores of the kp-only call")


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("n0,n1", R.DS_B9_SHAPES)
def test_dual_softmax_nine_pairs_and_batch_invariance(n0, n1, split):
    """B = 9: the XCD decode (9 units padded to 16); pair b of the batch is bit-identical to a B = 1 call on pair b (both paths fix
    their chunk counts for this)."""
    dev = _dev()
    c = R.dual_softmax_case("unit", 9, 128, n0, n1, 0.7)
    d0, d1, s0, s1 = _to(dev, c)
    what = "unit B=9 n0=%d n1=%d" % (n0, n1)
    full = _dual_softmax(split, d0, d1, s0, s1, 0.7)
    _check_full(_ds_name(split), "unit", c, full, what)
    for b in range(9):
        one = _dual_softmax(split, *_to(dev, c, slice(b, b + 1)), 0.7)
        for o, f, name in zip(one, full, ("scores", "kp_scores", "final_scores")):
            _same(o, f[b:b + 1], "%s: %s of pair %d alone against the batch" % (what, name, b))


@pytest.mark.parametrize("C", R.DS_SMALL_C)
@pytest.mark.parametrize("n0,n1", R.DS_B9_SHAPES)
def test_dual_softmax_exact_fewer_channels(n0, n1, C):
    """The FULLC = false instantiation of the exact path."""
    dev = _dev()
    c = R.dual_softmax_case("unit", 2, C, n0, n1, 8.0)
    d0, d1, s0, s1 = _to(dev, c)
    what = "unit C=%d n0=%d n1=%d" % (C, n0, n1)
    full = _dual_softmax(False, d0, d1, s0, s1, 8.0)
    _check_full("dual_softmax exact C<128", "unit", c, full, what)
    fin = _dual_softmax(False, d0, d1, s0, s1, 8.0, want=(False, False, True))
    _same(fin[2], full[2], what + ": final_scores of the final-only call")


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("n0,n1", R.DS_MISALIGNED_SHAPES)
def test_dual_softmax_misaligned_outputs(n0, n1, split):
    """Outputs 4 and 8 bytes off a 16-byte boundary (the 4- and 8-byte store forms of both apply kernels, unreachable through
    ops.dual_softmax), on the exact path also scr1 4 bytes off: bit-identical to the aligned call, neighbours untouched."""
    dev = _dev()
    c = R.dual_softmax_case("unit", 2, 128, n0, n1, 0.7)
    d0, d1, s0, s1 = _to(dev, c)
    what = "unit n0=%d n1=%d" % (n0, n1)
    full = _dual_softmax(split, d0, d1, s0, s1, 0.7)
    _check_full(_ds_name(split), "unit", c, full, what)
    variants = [dict(shift=1), dict(shift=2)] + ([] if split else [dict(scr1_shift=1)])
    for kw in variants:
        for want in ((True, True, True), (False, False, True)):
            got = _dual_softmax(split, d0, d1, s0, s1, 0.7, want=want, **kw)
            for o, f, name in zip(got, full, ("scores", "kp_scores", "final_scores")):
                if o is not None:
                    _same(o, f, "%s %r: %s against the aligned call" % (what, kw, name))


# ---- Sinkhorn -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n0,n1", R.SK_SHAPES)
def test_sinkhorn_elementwise(n0, n1):
    """B = 2; unit and wide inputs; (alpha, iters) in SK_PARAMS (iters = 0 included).  scores + kp + final, then scores only (null
    scr) and final only, bit-identical; the iterates u, v read back from `work` against the fp64 ones (absolutely: they are
    logarithms), the pad entries of v exactly 0."""
    dev = _dev()
    for C in (128, 32) if (n0, n1) in R.SK_C32_SHAPES else (128,):
        for family in ("unit", "wide"):
            for alpha, iters in R.SK_PARAMS:
                c = R.sinkhorn_case(family, 2, C, n0, n1, alpha, iters)
                d0, d1, s0, s1 = _to(dev, c)
                what = "%s C=%d n0=%d n1=%d alpha=%g iters=%d" % (family, C, n0, n1, alpha, iters)
                full, u2, v2 = _sinkhorn(d0, d1, s0, s1, alpha, iters)
                _check_full("sinkhorn", family, c, full, what)
                # iterates: natural log = log2-domain value / log2(e)
                tol = R.tolerance(c["floor"])
                for name, got, ref in (("u", u2.double() / LOG2E, c["u64"]), ("v", v2[:, :n1 + 1].double() / LOG2E, c["v64"])):
                    assert bool(torch.isfinite(got).all()), what
                    err = (got - ref).abs()
                    key = ("sinkhorn " + name, family)
                    fl = max(c["floor"], R.SPACING)
                    if key not in WORST or float(err.max()) / fl > WORST[key][0]:
                        WORST[key] = (float(err.max()) / fl, float(err.max()), c["floor"])
                    if not float(err.max()) <= tol:
                        i = int(err.argmax())
                        b, k = i // ref.shape[1], i % ref.shape[1]
                        raise AssertionError("sinkhorn, %s: |%s - %s64| = %.3e > %.3e at pair %d, index %d (of %d): got %r, fp64 %r"
                                             % (what, name, name, float(err.max()), tol, b, k, ref.shape[1] - 1,
                                                float(got[b, k]), float(ref[b, k])))
                assert bool((v2[:, n1 + 1:] == 0).all()) and not bool(torch.signbit(v2[:, n1 + 1:]).any()), what + ": pad entries of v"
                sc, _, _ = _sinkhorn(d0, d1, None, None, alpha, iters, want=(True, False, False))
                _same(sc[0], full[0], what + ": scores of the scores-only call")
                fin, _, _ = _sinkhorn(d0, d1, s0, s1, alpha, iters, want=(False, False, True))
                _same(fin[2], full[2], what + ": final_scores of the final-only call")


# ---- mutual nearest neighbours -----------------------------------------------------------------------------------------------
def _mutual_nn(scores):
    """mk_mutual_nn on device scores [B, n0, n1] -> (matches int32 [B, n0, 2], count int32 [B]) on the CPU; `matches` pre-set to
    PRESET, matches / count / work inside guards."""
    nv = _nv()
    dev = scores.device
    B, n0, n1 = scores.shape
    m, cm = guarded(B * n0, 2, torch.float32, dev)
    mi = m.view(torch.int32)
    mi.fill_(PRESET)
    cnt, cc = guarded(1, B, torch.float32, dev)
    work, cw = guarded(1, 2 * B * (n0 + n1), torch.float32, dev)
    nv.call("mk_mutual_nn", nv.ptr(scores), nv.ptr(m), nv.ptr(cnt), nv.ptr(work), B, n0, n1, nv.stream())
    torch.cuda.synchronize()
    for chk in (cm, cc, cw):
        chk()
    assert _written(cnt), "count: elements left unwritten"
    return mi.cpu().view(B, n0, 2), cnt.view(torch.int32).cpu()[0]


def _check_matches(matches, count, ref, what):
    for b, mb in enumerate(ref):
        n = int(count[b])
        assert n == mb.shape[0], "%s: pair %d has %d matches, the reference %d" % (what, b, n, mb.shape[0])
        got = matches[b, :n].long()
        if not torch.equal(got, mb):
            i = int(torch.nonzero((got != mb).any(1))[0])
            raise AssertionError("%s: pair %d, match %d of %d is %r, the reference has %r" % (what, b, i, n, got[i].tolist(), mb[i].tolist()))
        assert bool((matches[b, n:] == PRESET).all()), "%s: pair %d: `matches` written past count" % (what, b)


@pytest.mark.parametrize("B", R.MNN_BATCHES)
@pytest.mark.parametrize("n0,n1", R.MNN_SHAPES)
def test_mutual_nn_exact(n0, n1, B):
    """Planted mutual maxima on 5 score levels (the sort's tie rule), duplicated columns and rows (the first index wins an
    arg-max), an all -inf row, maxima in the excluded last column / row; npow2 up to 4096 (more than one key per thread); the
    batched call equals the B = 1 calls pair by pair."""
    dev = _dev()
    sc, _ = R.mutual_nn_scores(B, n0, n1)
    ref = R.mutual_nn_ref(sc)
    scd = sc.to(dev)
    what = "B=%d n0=%d n1=%d" % (B, n0, n1)
    matches, count = _mutual_nn(scd)
    _check_matches(matches, count, ref, what)
    if B > 1:
        for b in range(B):
            m1, c1 = _mutual_nn(scd[b:b + 1].contiguous())
            assert int(c1[0]) == int(count[b]) and torch.equal(m1[0], matches[b]), "%s: pair %d alone differs from the batch" % (what, b)


@pytest.mark.parametrize("B,n0,n1", R.MNN_LIMIT_CASES)
def test_mutual_nn_above_8192_rows(B, n0, n1):
    """n0 > 8192: more than 64 KiB of sort keys in LDS (mk_mutual_nn asks for it once), up to the documented maximum 16384."""
    dev = _dev()
    sc, _ = R.mutual_nn_scores(B, n0, n1)
    matches, count = _mutual_nn(sc.to(dev))
    _check_matches(matches, count, R.mutual_nn_ref(sc), "B=%d n0=%d n1=%d" % (B, n0, n1))
