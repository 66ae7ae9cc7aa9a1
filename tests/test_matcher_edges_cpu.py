"""No GPU: the references and input builders of tests/test_matcher_edges_gpu.py (tests/helpers/matcher_refs.py) are what that
file takes them for -- no element of an ordinary case escapes the relative comparison, the hot inputs do need a running maximum,
the planted mutual-NN scores do contain ties, duplicates and edge rows -- and the host-side argument checks of the matcher's
entry points refuse what they promise to refuse before anything is launched."""
import os

import pytest
import torch

from oracle import mickey_oracle as O
from tests.helpers import matcher_refs as R


# ---- ordinary inputs: every element is compared relatively -------------------------------------------------------------------
def test_ordinary_dual_softmax_inputs_leave_no_element_out():
    lo = float("inf")
    for family, B, C, n0, n1, db, split in R.dual_softmax_cases():
        if family != "unit" or split:
            continue
        c = R.dual_softmax_case(family, B, C, n0, n1, db)
        lo = min(lo, float(c["P64"].min()))
        assert float(c["P64"].min()) >= R.TINY, (B, C, n0, n1, db, float(c["P64"].min()))
        assert float(c["F64"].min()) >= R.TINY
        assert 0.0 < c["floor"] < 5e-5 or (n0, n1) == (1, 1), (n0, n1, db, c["floor"])     # the fp32 oracle is an fp32 computation
        # unit-norm descriptors never need the running maximum (the split path's premise)
        assert c["v2max"] <= 1.0 / R.TEMPERATURE * 1.4426950408889634 * (1 + 1e-6)
    print("dual softmax, unit inputs: smallest P64 %.3g" % lo)


def test_ordinary_sinkhorn_inputs_leave_no_element_out_and_wide_is_wide():
    lo = {"unit": float("inf"), "wide": float("inf")}
    hi = {"unit": 0.0, "wide": 0.0}
    for family, B, C, n0, n1, alpha, iters in R.sinkhorn_cases():
        c = R.sinkhorn_case(family, B, C, n0, n1, alpha, iters)
        mn, mx = float(c["P64"].min()), float(c["P64"].max())
        assert mn >= R.TINY, (family, C, n0, n1, alpha, iters, mn)
        lo[family], hi[family] = min(lo[family], mn), max(hi[family], mx)
        if family == "wide" and min(n0, n1) >= 62 and iters == 10:
            assert mx / mn > 1e12, (n0, n1, alpha, mn, mx)     # the unit family is flat to a few per cent
    print("sinkhorn: smallest / largest P64 %r / %r" % (lo, hi))
    assert lo["wide"] < 1e-20 and hi["wide"] > 0.5


def test_sinkhorn_iterates_reproduce_the_oracle():
    for family, n0, n1, alpha, iters in (("wide", 63, 64, 1.3, 10), ("unit", 7, 3, -2.0, 3), ("unit", 1, 1, 1.0, 0)):
        d0, d1 = R.descriptors(family, 2, 128, n0, n1)
        u, v, P = R.sinkhorn_uv64(d0, d1, alpha, iters)
        assert torch.equal(P, R.sinkhorn64(d0, d1, alpha, iters))
        assert u.shape == (2, n0 + 1) and v.shape == (2, n1 + 1)


# ---- hot inputs ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n0,n1", R.DS_HOT_SHAPES + [(97, 64), (77, 200), (255, 257)])
def test_hot_inputs_need_the_running_maximum(n0, n1):
    assert min(n0, n1) >= 64
    for db in R.DUSTBINS:
        c = R.dual_softmax_case("hot", 2, 128, n0, n1, db)
        assert c["v2max"] > 128.0, c["v2max"]                    # 2^v2 overflows fp32: a sum without the running maximum is inf
        big = c["P64"] >= R.TINY
        share = float(big.double().mean())
        assert share >= 0.85, (n0, n1, db, share)
        assert float(c["P32"][~big].max() if bool((~big).any()) else 0.0) <= 2 * R.TINY
        assert bool(torch.isfinite(c["P32"]).all()) and c["floor"] < 1e-3, c["floor"]
        # the peaks are where they were planted
        for k in R.hot_keypoints(n0, n1):
            assert float(c["P64"][:, k, k].min()) > 0.9
    assert all(min(s) >= 64 for s in R.DS_HOT_SHAPES)


# ---- the mutual-NN reference and builder --------------------------------------------------------------------------------------
def test_torch_max_returns_the_first_maximal_index():
    x = torch.tensor([[0.5, 2.0, 2.0, 1.0, 2.0], [3.0, 3.0, 0.0, 3.0, 1.0], [float("-inf")] * 5])
    for dim in (0, 1):
        v, idx = x.max(dim)
        xs = x if dim == 1 else x.t()
        for r in range(xs.shape[0]):
            best, bi = None, None
            for j in range(xs.shape[1]):
                if best is None or float(xs[r, j]) > best:
                    best, bi = float(xs[r, j]), j
            assert int(idx[r]) == bi and float(v[r]) == best
    big = torch.zeros((3, 300))
    big[:, 70], big[:, 134], big[:, 6 + 64 * 4] = 1.0, 1.0, 1.0
    assert big.max(1).indices.tolist() == [70, 70, 70] and big.t().contiguous().max(0).indices.tolist() == [70, 70, 70]


@pytest.mark.parametrize("n0,n1", R.MNN_SHAPES)
def test_mutual_nn_builder_plants_what_it_promises(n0, n1):
    for B in R.MNN_BATCHES:
        sc, info = R.mutual_nn_scores(B, n0, n1)
        assert sc.shape == (B, n0, n1)
        ref = R.mutual_nn_ref(sc)
        assert len(ref) == B
        # tie-free continuous scores: the deterministic reference is the oracle's
        cont, _ = R.mutual_nn_scores(B, n0, n1, plants=False)
        for b, mb in enumerate(R.mutual_nn_ref(cont)):
            assert torch.equal(mb, O.mutual_nn_matches(cont[b:b + 1]))
        if n0 < 16 or n1 < 16:
            continue
        for b in range(B):
            mb, d = ref[b], info[b]
            assert mb.shape[0] >= 8, (n0, n1, b, mb.shape)
            v = sc[b, mb[:, 0], mb[:, 1]]
            assert bool((v[:-1] >= v[1:]).all())
            eq = v[:-1] == v[1:]
            assert int(eq.sum()) >= 3
            assert bool((mb[:-1, 0] < mb[1:, 0])[eq].all())                       # equal scores: ascending row
            sub = sc[b, :-1, :-1]
            assert int(((sub == sub.max(1, keepdim=True).values).sum(1) > 1)[torch.isfinite(sub.max(1).values)].sum()) >= 1
            assert int(((sub == sub.max(0, keepdim=True).values).sum(0) > 1).sum()) >= 1
            assert d["dup_cols"] and d["dup_rows"] and d["inf_row"] is not None
            assert d["lastcol_row"] is not None and d["lastrow_col"] is not None
            assert d["inf_row"] not in mb[:, 0].tolist()
            got = {(int(r), int(c)) for r, c in mb.tolist()}
            # every planted pair is a match; of a duplicate the first index is the match, the later one is not
            assert set(d["planted"]) <= got
            for r, c, c2 in d["dup_cols"]:
                assert float(sc[b, r, c]) == float(sc[b, r, c2]) and c2 > c and (r, c2) not in got
            for r, r2, c in d["dup_rows"]:
                assert float(sc[b, r, c]) == float(sc[b, r2, c]) and r2 > r and (r2, c) not in got
            assert int(sc[b, d["lastcol_row"]].argmax()) == n1 - 1 and int(sc[b, :, d["lastrow_col"]].argmax()) == n0 - 1


def test_mutual_nn_limit_cases_have_matches():
    for B, n0, n1 in R.MNN_LIMIT_CASES:
        sc, _ = R.mutual_nn_scores(B, n0, n1)
        assert all(m.shape[0] >= 1 for m in R.mutual_nn_ref(sc))


# ---- the entry points' argument checks ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from mickey_amd import build, _native
    if not os.path.exists(build.lib_path()):
        build.build(verbose=False)
    return _native.load()


def _refused(lib, rc, *words):
    """MK_ERR_INVALID_ARGUMENT (1; a launch error is 2: nothing was launched) and an error text that says why"""
    msg = lib.mk_last_error()
    assert rc == 1, (rc, msg)
    assert all(w in msg for w in words), msg


def test_dual_softmax_rejects_bad_arguments_without_a_device(lib):
    p = 16   # any non-null, 16-byte aligned address: the argument checks run before anything touches it
    ok = dict(dsc0=p, dsc1=p, scr0=p, scr1=p, invt=10.0, ud=0, db=0.0, sc=p, kp=p, fin=p, work=p, B=2, C=128, n0=8, n1=8)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.mk_dual_softmax(a["dsc0"], a["dsc1"], a["scr0"], a["scr1"], a["invt"], a["ud"], a["db"], a["sc"], a["kp"], a["fin"],
                                   a["work"], a["B"], a["C"], a["n0"], a["n1"], None)

    for C in (3, 130, 0):
        _refused(lib, call(C=C), b"mk_dual_softmax", b"C")
    _refused(lib, call(B=0), b"mk_dual_softmax")
    _refused(lib, call(n0=0), b"mk_dual_softmax")
    _refused(lib, call(scr0=None, fin=None), b"scr0")             # kp without scr0
    _refused(lib, call(scr1=None, kp=None), b"scr1")              # final without scr1
    _refused(lib, call(scr0=None, scr1=None, sc=None), b"scr0")
    _refused(lib, call(work=None), b"null")
    _refused(lib, call(dsc0=None), b"null")
    _refused(lib, call(dsc1=None), b"null")


def test_dual_softmax_split_rejects_bad_arguments_without_a_device(lib):
    p = 16
    ok = dict(dsc0=p, dsc1=p, scr0=p, scr1=p, invt=10.0, ud=0, db=0.0, sc=p, kp=p, fin=p, work=p, B=2, C=128, n0=8, n1=8)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.mk_dual_softmax_split(a["dsc0"], a["dsc1"], a["scr0"], a["scr1"], a["invt"], a["ud"], a["db"], a["sc"], a["kp"],
                                         a["fin"], a["work"], a["B"], a["C"], a["n0"], a["n1"], None)

    _refused(lib, call(C=64), b"mk_dual_softmax_split", b"128")
    _refused(lib, call(C=126), b"128")
    _refused(lib, call(work=8), b"16-byte")
    _refused(lib, call(work=None), b"null")
    for invt in (0.0, -10.0, 100.0):
        _refused(lib, call(invt=invt), b"temperature")
    _refused(lib, call(scr0=None), b"scr0")
    _refused(lib, call(B=0), b"mk_dual_softmax_split")


def test_sinkhorn_rejects_bad_arguments_without_a_device(lib):
    p = 16
    ok = dict(dsc0=p, dsc1=p, scr0=p, scr1=p, alpha=1.0, iters=10, sc=p, kp=p, fin=p, work=p, B=2, C=128, n0=8, n1=8)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.mk_sinkhorn(a["dsc0"], a["dsc1"], a["scr0"], a["scr1"], a["alpha"], a["iters"], a["sc"], a["kp"], a["fin"], a["work"],
                               a["B"], a["C"], a["n0"], a["n1"], None)

    _refused(lib, call(sc=None, fin=None), b"mk_sinkhorn")        # neither scores nor final_scores (kp_scores alone)
    _refused(lib, call(iters=-1), b"mk_sinkhorn")
    _refused(lib, call(work=8), b"16-byte")
    _refused(lib, call(work=None), b"null")
    for C in (127, 0, 130):
        _refused(lib, call(C=C), b"mk_sinkhorn")
    _refused(lib, call(scr0=None), b"scr0")
    _refused(lib, call(n1=0), b"mk_sinkhorn")


def test_mutual_nn_rejects_bad_arguments_without_a_device(lib):
    p = 16
    _refused(lib, lib.mk_mutual_nn(p, p, p, p, 1, 1, 8, None), b"mk_mutual_nn")
    _refused(lib, lib.mk_mutual_nn(p, p, p, p, 1, 8, 1, None), b"mk_mutual_nn")
    _refused(lib, lib.mk_mutual_nn(p, p, p, p, 1, 16385, 8, None), b"mk_mutual_nn", b"16385")
    _refused(lib, lib.mk_mutual_nn(p, p, p, p, 0, 8, 8, None), b"mk_mutual_nn")
    for k in range(4):
        a = [p, p, p, p]
        a[k] = None
        _refused(lib, lib.mk_mutual_nn(a[0], a[1], a[2], a[3], 1, 8, 8, None), b"mk_mutual_nn")
