"""Keyframe mode (README "Keyframe mode") without a device: host validation of the pair -> keyframe map, sharding of a
keyframe batch, the feeder's record grouping and the ABI's argument checks of the *_kf entry points."""
import os
import pathlib

import numpy as np
import pytest
import torch

from mickey_amd import distributed as D
from mickey_amd import ops
from mickey_amd.input_pipeline import group_keyframes


@pytest.mark.parametrize("index, B, K", [
    ([0, 1], 3, 2),                                      # wrong length
    ([0, 1, 1, 0], 3, 2),
    ([0, 2, 1], 3, 2),                                   # out of range
    ([0, -1, 1], 3, 2),                                  # negative
    (np.array([0.0, 1.0, 1.0]), 3, 2),                   # float dtype
    (torch.tensor([0.0, 1.0, 0.0]), 3, 2),
    (torch.tensor([[0, 1, 0]]), 3, 2),                   # not one entry per pair
    ([0, 0, 0], 3, 0),                                   # no keyframe
    ([0, 1, 2], 3, 4),                                   # more keyframes than pairs
])
def test_bad_keyframe_index_raises(index, B, K):
    with pytest.raises(ValueError):
        ops.check_keyframe_index(index, B, K)


def test_keyframe_index_accepted_forms():
    for idx in ([2, 0, 2, 1, 0], np.array([2, 0, 2, 1, 0], np.int64), torch.tensor([2, 0, 2, 1, 0], dtype=torch.int32),
                np.array([2, 0, 2, 1, 0], np.uint8)):
        out = ops.check_keyframe_index(idx, 5, 3)
        assert out.dtype == np.int32 and out.tolist() == [2, 0, 2, 1, 0]


def test_model_validates_before_any_launch():
    from mickey_amd.config import default_cfg
    from mickey_amd.model import MickeyRelativePose
    model = MickeyRelativePose(default_cfg())   # CPU-resident, no weights: any launch attempt would raise something else
    data = {"image0": torch.zeros(2, 3, 28, 28), "image1": torch.zeros(3, 3, 28, 28), "K_color0": torch.eye(3).repeat(3, 1, 1),
            "K_color1": torch.eye(3).repeat(3, 1, 1), "keyframe_index": [0, 2, 1]}
    with pytest.raises(ValueError):
        model(data)
    assert not model._wants_graph(dict(data, keyframe_index=[0, 1, 1]), False)


def _kf_batch(B, K, kf, pair_base=0):
    g = torch.Generator().manual_seed(B * 31 + K)
    return {"image0": torch.arange(K, dtype=torch.float32).reshape(K, 1, 1, 1).expand(K, 3, 2, 2).clone(),
            "image1": torch.rand((B, 3, 2, 2), generator=g), "K_color0": torch.rand((B, 3, 3), generator=g),
            "K_color1": torch.rand((B, 3, 3), generator=g), "keyframe_index": torch.tensor(kf),
            "pair_names": [("a%d" % b, "q%d" % b) for b in range(B)], "scene_id": "s0", "pair_base": pair_base}


@pytest.mark.parametrize("world", [2, 3])
def test_shard_batch_keeps_only_the_referenced_keyframes(world):
    kf = [2, 0, 2, 1, 0, 3, 3]
    data = _kf_batch(7, 4, kf, pair_base=10)
    seen = []
    for r in range(world):
        lo, hi = D.shard_range(7, r, world)
        loc = D.shard_batch(data, r, world)
        lk = loc["keyframe_index"].tolist()
        assert loc["pair_base"] == 10 + lo
        assert loc["image1"].shape[0] == hi - lo and torch.equal(loc["image1"], data["image1"][lo:hi])
        assert torch.equal(loc["K_color0"], data["K_color0"][lo:hi]) and loc["pair_names"] == data["pair_names"][lo:hi]
        # only the keyframes this rank's pairs use, in order of first use
        want = list(dict.fromkeys(kf[lo:hi]))
        assert loc["image0"].shape[0] == len(want) and sorted(set(lk)) == list(range(len(want)))
        assert [int(v) for v in loc["image0"][:, 0, 0, 0]] == want
        # composed back: the local pairing is the global one
        assert [want[i] for i in lk] == kf[lo:hi]
        for b in range(hi - lo):
            assert torch.equal(loc["image0"][lk[b]], data["image0"][kf[lo + b]])
        assert D.num_pairs(loc) == hi - lo
        seen += [want[i] for i in lk]
    assert seen == kf


def test_shard_batch_without_keyframes_is_unchanged():
    data = {"image0": torch.rand(5, 3, 2, 2), "image1": torch.rand(5, 3, 2, 2), "names": list("abcde")}
    loc = D.shard_batch(data, 1, 2)
    assert torch.equal(loc["image0"], data["image0"][3:]) and loc["names"] == ["d", "e"] and loc["pair_base"] == 3
    assert "keyframe_index" not in loc and D.num_pairs(data) == 5


def test_feeder_groups_records_by_image0_path(tmp_path):
    from mickey_amd import mapfree_eval as ME
    from tests.helpers import tiny_mapfree
    tiny_mapfree.make(str(tmp_path), "val", scenes=("s00460", "s00461"), queries=11, size=(28, 28))
    recs = ME.dataset_records(str(tmp_path), "val", (28, 28))
    assert len(recs) == 6
    batches = [recs[0:4], recs[4:6]]
    kfs, idx = group_keyframes(batches[0])          # 3 pairs of scene 0, 1 of scene 1: K = 2 across the boundary
    assert kfs == [0, 3] and idx == [0, 0, 0, 1]
    kfs, idx = group_keyframes(batches[1])
    assert kfs == [0] and idx == [0, 0]
    # order of first appearance, not of the path
    kfs, idx = group_keyframes([recs[3], recs[0], recs[4], recs[1]])
    assert kfs == [0, 1] and idx == [0, 1, 0, 1]
    # per-pair K_color0 stays with the records (the feeder stacks it per record)
    assert all(np.array_equal(r["K_color0"], recs[0]["K_color0"]) for r in recs[:3])
    # pathlib paths are paths too
    kfs, idx = group_keyframes([dict(recs[0], image0=os.fspath(recs[0]["image0"])), dict(recs[1], image0=pathlib.Path(recs[1]["image0"]))])
    assert kfs == [0] and idx == [0, 0]


def test_feeder_never_merges_arrays_or_bytes():
    a = np.zeros((4, 4, 3), np.uint8)
    recs = [{"image0": a, "image1": a}, {"image0": a, "image1": a}, {"image0": b"xx", "image1": a}, {"image0": b"xx", "image1": a}]
    kfs, idx = group_keyframes(recs)
    assert kfs == [0, 1, 2, 3] and idx == [0, 1, 2, 3]


@pytest.fixture(scope="module")
def nv():
    from mickey_amd import build, _native
    if not os.path.exists(build.lib_path()):
        build.build(verbose=False)
    _native.load()
    return _native


def test_kf_entry_points_reject_bad_arguments_without_a_device(nv):
    lib = nv.load()
    p = 16   # any non-null address: the argument checks run before anything touches it
    # null pointers
    assert lib.mk_dual_softmax_kf(None, p, None, None, 10.0, 0, 0.0, p, None, None, p, 2, 128, 8, 8, p, 1, None) == 1
    assert b"null" in lib.mk_last_error()
    assert lib.mk_dual_softmax_split_kf(p, None, None, None, 10.0, 0, 0.0, p, None, None, p, 2, 128, 8, 8, p, 1, None) == 1
    assert lib.mk_sinkhorn_kf(p, p, None, None, 1.0, 10, None, None, None, p, 2, 128, 8, 8, p, 1, None) == 1
    assert lib.mk_gather_backproject_kf(None, p, p, p, p, p, p, p, p, p, p, p, 2, 20, 8, 8, 8, p, 1, None) == 1
    # K <= 0 with a map, K > B, K != B without one
    for K in (0, -1, 3):
        assert lib.mk_dual_softmax_kf(p, p, None, None, 10.0, 0, 0.0, p, None, None, p, 2, 128, 8, 8, p, K, None) == 1
        assert b"K" in lib.mk_last_error()
        assert lib.mk_dual_softmax_split_kf(p, p, None, None, 10.0, 0, 0.0, p, None, None, p, 2, 128, 8, 8, p, K, None) == 1
        assert lib.mk_sinkhorn_kf(p, p, None, None, 1.0, 10, p, None, None, p, 2, 128, 8, 8, p, K, None) == 1
        assert lib.mk_gather_backproject_kf(p, p, p, p, p, p, p, p, p, p, p, p, 2, 20, 8, 8, 8, p, K, None) == 1
    assert lib.mk_dual_softmax_kf(p, p, None, None, 10.0, 0, 0.0, p, None, None, p, 2, 128, 8, 8, None, 1, None) == 1
    assert lib.mk_gather_backproject_kf(p, p, p, p, p, p, p, p, p, p, p, p, 2, 20, 8, 8, 8, None, 1, None) == 1
    with pytest.raises(nv.MickeyHipError):
        nv.call("mk_sinkhorn_kf", None, None, None, None, 1.0, 10, None, None, None, None, 0, 0, 0, 0, None, 0, None)
