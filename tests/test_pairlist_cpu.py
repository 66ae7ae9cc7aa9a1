"""Pair-list mode (README "Pair-list mode") without a device: host validation of the pair list, the model's host checks (before
anything touches the library), sharding of a pair-list batch and the ABI of the *_pairs entry points."""
import copy
import os
import re

import numpy as np
import pytest
import torch

from mickey_amd import distributed as D
from mickey_amd import ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = [[2, 0], [0, 2], [1, 1], [2, 1], [0, 1]]   # N = 3, P = 5: every image on both sides, one self pair


# ---- ops.check_pair_index ---------------------------------------------------------------------------------------------------------
def test_pair_index_accepted_forms():
    for idx in (PAIRS, np.array(PAIRS, np.int64), np.array(PAIRS, np.uint8), torch.tensor(PAIRS, dtype=torch.int32),
                torch.tensor(PAIRS, dtype=torch.int64)):
        out = ops.check_pair_index(idx, 5, 3)
        assert out.dtype == np.int32 and out.shape == (5, 2) and out.tolist() == PAIRS
    # duplicated pairs, self pairs and unused images are legal; two sets of different sizes
    assert ops.check_pair_index([[0, 0], [0, 0], [3, 3]], 3, 12).tolist() == [[0, 0], [0, 0], [3, 3]]
    assert ops.check_pair_index([[2, 3], [0, 0]], 2, (3, 4)).tolist() == [[2, 3], [0, 0]]


@pytest.mark.parametrize("index, P, N", [
    ([2, 0, 1, 1, 0], 5, 3),                                   # wrong shape: one column
    ([[2, 0, 1]] * 5, 5, 3),                                   # three columns
    ([[[2, 0]]] * 5, 5, 3),                                    # three dimensions
    (np.array(PAIRS, np.float64), 5, 3),                       # float dtype
    (torch.tensor(PAIRS, dtype=torch.float32), 5, 3),
    (torch.tensor(PAIRS) > 0, 5, 3),                           # bool
    ([[2, 0], [0, -1]], 2, 3),                                 # negative
    ([[2, 0], [0, 3]], 2, 3),                                  # >= N
    ([[3, 0], [0, 2]], 2, 3),
    ([[2, 3], [0, 0]], 2, (4, 3)),                             # >= N1 of a two-set call
    (PAIRS, 4, 3),                                             # wrong P
    (PAIRS, 6, 3),
    ([], 0, 0),                                                # no image
])
def test_bad_pair_index_raises(index, P, N):
    with pytest.raises(ValueError):
        ops.check_pair_index(index, P, N)


def test_ops_modes_are_mutually_exclusive():
    d = torch.zeros(3, 128, 8)
    for fn, args in ((ops.dual_softmax, (d, d)), (ops.sinkhorn, (d, d, 1.0)),
                     (ops.gather_backproject, (None,) * 8 + (4,))):
        with pytest.raises(ValueError):
            fn(*args, keyframe_index=[0, 1, 2], pair_index=[[0, 1]])


# ---- the model's host checks ------------------------------------------------------------------------------------------------------
class _Boom:
    """stands in for the library: any touch fails the test"""
    def __getattr__(self, name):
        raise AssertionError("the library was touched (%s) before the arguments were checked" % name)


def _data(N=3, pairs=PAIRS):
    return {"images": torch.zeros(N, 3, 28, 28), "K_color": torch.eye(3).repeat(N, 1, 1), "pair_index": pairs}


def test_model_validates_before_anything_touches_the_library(monkeypatch):
    from mickey_amd import _native
    from mickey_amd.config import default_cfg
    from mickey_amd.model import MickeyRelativePose
    monkeypatch.setattr(_native, "load", lambda: _Boom())
    monkeypatch.setattr(_native, "_lib", None)
    monkeypatch.setattr(ops, "call", lambda *a: _Boom().call)
    monkeypatch.setattr(ops, "query", lambda *a: _Boom().query)
    model = MickeyRelativePose(default_cfg())   # CPU-resident, no weights: a launch attempt would raise something else
    bad = [dict(_data(), image0=torch.zeros(5, 3, 28, 28)),                   # images together with image0
           dict(_data(), image1=torch.zeros(5, 3, 28, 28)),
           dict(_data(), keyframe_index=[0, 0, 0, 0, 0]),                     # pair_index together with keyframe_index
           dict(_data(), K_color=torch.eye(3).repeat(5, 1, 1)),               # K_color per pair, not per image
           dict(_data(), K_color=torch.eye(3).repeat(2, 1, 1)),
           dict(_data(), K_color=torch.eye(4).repeat(3, 1, 1)),
           dict(_data(), images=torch.zeros(3, 1, 28, 28)),
           {k: v for k, v in _data().items() if k != "images"},
           {k: v for k, v in _data().items() if k != "K_color"},
           _data(pairs=[[0, 3]]), _data(pairs=[[-1, 0]]), _data(pairs=[0, 1]), _data(pairs=[]),
           _data(pairs=torch.tensor(PAIRS, dtype=torch.float32))]
    for data in bad:
        with pytest.raises(ValueError):
            model(data)
        with pytest.raises(ValueError):
            model(data, return_inliers=True)
    assert not model._wants_graph(_data(), False)
    cfg = copy.deepcopy(default_cfg())
    cfg["AMD"]["GRAPH"] = True
    graphed = MickeyRelativePose(cfg)
    assert not graphed._wants_graph(_data(), False)


# ---- distributed.shard_batch ------------------------------------------------------------------------------------------------------
def _pl_batch(N, pairs, pair_base=0):
    P = len(pairs)
    g = torch.Generator().manual_seed(N * 31 + P)
    return {"images": torch.arange(N, dtype=torch.float32).reshape(N, 1, 1, 1).expand(N, 3, 2, 2).clone(),
            "K_color": torch.rand((N, 3, 3), generator=g), "pair_index": torch.tensor(pairs),
            "pair_names": [("a%d" % i, "b%d" % j) for i, j in pairs], "gt": torch.rand((P, 4), generator=g), "scene_id": "s0",
            "pair_base": pair_base}


@pytest.mark.parametrize("world", [1, 2, 3])
@pytest.mark.parametrize("pairs, N", [
    ([[i, i + 1] for i in range(7)], 8),                                         # a sequence
    ([[k, 3 + q] for k in range(3) for q in range(2)] + [[5, 5]], 6),            # keyframes x queries, one self pair; image 5 unused
    (PAIRS + [[0, 1], [2, 0]], 4),                                               # duplicates; image 3 unused
])
def test_shard_batch_on_a_pair_list(world, pairs, N):
    data = _pl_batch(N, pairs, pair_base=10)
    P = len(pairs)
    assert D.num_pairs(data) == P
    seen = []
    for r in range(world):
        lo, hi = D.shard_range(P, r, world)
        loc = D.shard_batch(data, r, world)
        assert D.num_pairs(loc) == hi - lo and loc["pair_base"] == 10 + lo
        lp = loc["pair_index"].tolist()
        assert loc["pair_index"].shape == (hi - lo, 2)
        # only the images this rank's pairs use, in order of first use
        want = list(dict.fromkeys(i for row in pairs[lo:hi] for i in row))
        assert [int(v) for v in loc["images"][:, 0, 0, 0]] == want
        assert loc["K_color"].shape[0] == len(want) and all(torch.equal(loc["K_color"][j], data["K_color"][g]) for j, g in enumerate(want))
        assert sorted({i for row in lp for i in row}) == list(range(len(want)))
        # per-pair entries are sliced, the rest is passed through
        assert loc["pair_names"] == data["pair_names"][lo:hi] and torch.equal(loc["gt"], data["gt"][lo:hi]) and loc["scene_id"] == "s0"
        seen += [[want[i], want[j]] for i, j in lp]
    assert seen == pairs   # concatenated and mapped back through the kept images: the global list, in order


def test_shard_batch_without_a_pair_list_is_unchanged():
    data = {"image0": torch.rand(5, 3, 2, 2), "image1": torch.rand(5, 3, 2, 2), "names": list("abcde")}
    loc = D.shard_batch(data, 1, 2)
    assert torch.equal(loc["image0"], data["image0"][3:]) and loc["names"] == ["d", "e"] and loc["pair_base"] == 3
    assert D.num_pairs(data) == 5


# ---- the ABI ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def nv():
    from mickey_amd import build, _native
    if not os.path.exists(build.lib_path()):
        build.build(verbose=False)
    _native.load()
    return _native


ENTRIES = ("mk_dual_softmax_pairs", "mk_dual_softmax_split_pairs", "mk_sinkhorn_pairs", "mk_gather_backproject_pairs")


def test_pairs_entry_points_are_declared_exported_and_bound(nv):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mickey_hip.h")).read(), flags=re.S)
    lib = nv.load()
    for name in ENTRIES + ("mk_dsc_split_planes", "mk_dual_softmax_split_planes"):
        m = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, hdr, re.S)
        assert m and name in nv.SIGNATURES and hasattr(lib, name), name
        params = [p.strip() for p in m.group(1).split(",")]
        assert len(params) == len(nv.SIGNATURES[name][1]), name
        if name in ENTRIES:   # the plain call's arguments + the two maps and their row counts, in front of the stream
            plain = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name[:-len("_pairs")], hdr, re.S).group(1).split(",")
            assert len(params) == len(plain) + 4
            assert [p.split()[-1] for p in params[-5:]] == ["idx0", "idx1", "N0", "N1", "stream"]
            assert nv.SIGNATURES[name][1] == nv.SIGNATURES[name[:-len("_pairs")]][1][:-1] + "ppiip"
    assert nv.missing_symbols() == []
    # the planes region covers N0 + N1 images, or the N of a shared set; the rest is per pair
    per_pair = nv.query("mk_dual_softmax_split_planes_work_floats", 5, 300, 257)
    blk = 16 * 1024 // 4   # floats per block of 32 keypoints
    assert nv.query("mk_dsc_split_planes_floats", 7, 300) == 7 * 10 * blk
    assert nv.query("mk_dual_softmax_split_pairs_work_floats", 5, 300, 257, 3, 40, 0) == (3 * 10 + 40 * 9) * blk + per_pair
    assert nv.query("mk_dual_softmax_split_pairs_work_floats", 5, 300, 300, 40, 40, 1) == \
        40 * 10 * blk + nv.query("mk_dual_softmax_split_planes_work_floats", 5, 300, 300)
    assert nv.query("mk_dual_softmax_split_work_floats", 5, 300, 257) == 5 * 19 * blk + per_pair


def test_pairs_entry_points_reject_bad_arguments_without_a_device(nv):
    lib = nv.load()
    p = 16   # any non-null address: the argument checks run before anything touches it

    def ds(name, d0=p, d1=p, work=p, i0=p, i1=p, N0=3, N1=3):
        return getattr(lib, name)(d0, d1, None, None, 10.0, 0, 0.0, p, None, None, work, 2, 128, 8, 8, i0, i1, N0, N1, None)

    def sk(d0=p, d1=p, work=p, sc=p, i0=p, i1=p, N0=3, N1=3):
        return lib.mk_sinkhorn_pairs(d0, d1, None, None, 1.0, 10, sc, None, None, work, 2, 128, 8, 8, i0, i1, N0, N1, None)

    def gb(idx=p, X=p, i0=p, i1=p, N0=3, N1=3):
        return lib.mk_gather_backproject_pairs(idx, p, p, p, p, p, p, p, X, p, p, p, 2, 20, 8, 8, 8, i0, i1, N0, N1, None)

    calls = [lambda **kw: ds("mk_dual_softmax_pairs", **kw), lambda **kw: ds("mk_dual_softmax_split_pairs", **kw), sk, gb]
    # null pointers
    for name in ENTRIES[:2]:
        for kw in (dict(d0=None), dict(d1=None), dict(work=None)):
            assert ds(name, **kw) == 1 and b"null" in lib.mk_last_error(), (name, kw)
    for kw in (dict(d0=None), dict(work=None), dict(sc=None)):
        assert sk(**kw) == 1 and b"null" in lib.mk_last_error(), kw
    for kw in (dict(idx=None), dict(X=None)):
        assert gb(**kw) == 1 and b"null" in lib.mk_last_error(), kw
    # a non-positive row count behind a map; a row count other than B on an identity side (B = 2 in every call above)
    for call in calls:
        for kw in (dict(N0=0), dict(N0=-1), dict(N1=0), dict(N1=-4), dict(i0=None, N0=3), dict(i1=None, N1=1),
                   dict(i0=None, i1=None, N0=2, N1=3)):
            assert call(**kw) != 0, kw
            assert (b"N0" if "N0" in kw and kw["N0"] != 2 else b"N1") in lib.mk_last_error(), kw
    # row counts are not limited by the pair count (no K <= B rule here): these get past the map checks and stop at a later one
    assert ds("mk_dual_softmax_split_pairs", N0=50, N1=70, work=24) == 1 and b"aligned" in lib.mk_last_error()
    assert lib.mk_dsc_split_planes(None, p, 3, 128, 8, None) == 1 and b"null" in lib.mk_last_error()
    assert lib.mk_dsc_split_planes(p, p, 3, 64, 8, None) == 1
    assert lib.mk_dual_softmax_split_planes(p, None, None, None, 10.0, 0, 0.0, p, None, None, p, 2, 8, 8, p, p, 3, 3, None) == 1
    assert lib.mk_dual_softmax_split_planes(p, p, None, None, 10.0, 0, 0.0, p, None, None, p, 2, 8, 8, p, p, 0, 3, None) == 1
    with pytest.raises(nv.MickeyHipError):
        nv.call("mk_sinkhorn_pairs", None, None, None, None, 1.0, 10, None, None, None, None, 0, 0, 0, 0, None, None, 0, 0, None)
