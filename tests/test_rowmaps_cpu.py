"""ops._row_maps: the one normaliser of the three calling modes of the matcher / solver wrappers (plain, keyframe_index=,
pair_index=), without a device and without the library: host lists go to a CPU "device".  And the one caller that may not pass
the mode keywords straight through: the standard pipeline.match call under bench.py's stage profiler."""
import pytest
import torch

from mickey_amd import ops

CPU = torch.device("cpu")


def _is_map(t, entries):
    return torch.is_tensor(t) and t.dtype == torch.int32 and t.is_contiguous() and t.tolist() == entries


def test_no_map_is_the_plain_call():
    assert ops._row_maps(None, None, 5, 5, CPU) == ("", (), (), 5)
    assert ops._row_maps(None, None, 5, 5, CPU, P=5) == ("", (), (), 5)


def test_keyframe_list():
    kf = [2, 0, 1, 1, 0]   # B = 5 pairs over K = 3 keyframes
    suffix, maps, rows, P = ops._row_maps(kf, None, 3, 5, CPU)
    assert suffix == "_kf" and rows == (3,) and P == 5
    assert len(maps) == 1 and _is_map(maps[0], kf)


def test_pair_list():
    pairs = [[2, 3], [0, 0], [1, 3], [2, 1]]   # P = 4 pairs over (N0, N1) = (3, 4) images
    suffix, maps, rows, P = ops._row_maps(None, pairs, 3, 4, CPU)
    assert suffix == "_pairs" and rows == (3, 4) and P == 4
    assert len(maps) == 2 and _is_map(maps[0], [p[0] for p in pairs]) and _is_map(maps[1], [p[1] for p in pairs])
    assert ops._row_maps(None, pairs, 3, 4, CPU, P=4)[3] == 4
    with pytest.raises(ValueError):   # the pair count the caller knows disagrees with the list
        ops._row_maps(None, pairs, 3, 4, CPU, P=5)


def test_both_maps_raise():
    with pytest.raises(ValueError):
        ops._row_maps([0, 1, 2], [[0, 1]], 3, 3, CPU)


@pytest.mark.parametrize("kf, K, B", [
    ([0, 1, 2], 4, 3),          # more keyframes than pairs
    ([0, 3, 1, 2, 0], 3, 5),    # an entry equal to K
])
def test_bad_keyframe_map_still_raises(kf, K, B):
    with pytest.raises(ValueError):
        ops._row_maps(kf, None, K, B, CPU)


def test_bad_pair_entry_still_raises():
    with pytest.raises(ValueError):
        ops._row_maps(None, [[2, 3], [0, 4]], 3, 4, CPU)   # an entry equal to N1


# ---- pipeline.match and the benchmark's stage profiler -----------------------------------------------------------------------------
class _FakeOps:
    """stands in for mickey_amd.ops: every wrapper returns three Nones and remembers its keywords"""
    def __init__(self):
        self.seen = {}

    def __getattr__(self, name):
        def fn(*a, **k):
            self.seen[name] = set(k)
            return None, None, None
        return fn


@pytest.mark.parametrize("matcher", ["DualSoftmax", "Sinkhorn"])
def test_standard_match_call_fits_the_stage_profiler(monkeypatch, matcher):
    """bench.py's StageProfiler wraps the ops wrappers and computes each launch's bytes from the call's own arguments; its byte
    count for dual_softmax takes the standard call's keywords and no others.  The standard forward (no map) must go on fitting
    it: a mode keyword handed through as None would end a profiled benchmark run with a TypeError."""
    import copy
    import bench
    from mickey_amd import pipeline
    from mickey_amd.config import default_cfg

    class Event:
        def __init__(self, enable_timing=False):
            pass

        def record(self):
            pass

    fake = _FakeOps()
    prof = bench.StageProfiler()
    prof.wrap(fake)
    prof.on = True
    monkeypatch.setattr(torch.cuda, "Event", Event)
    monkeypatch.setattr(pipeline, "ops", fake)
    cfg = copy.deepcopy(default_cfg())
    cfg["FEATURE_MATCHER"]["TYPE"] = matcher
    W = type("W", (), {"dustbin": None})
    d = torch.zeros(2, 128, 8)
    s = torch.zeros(2, 8)
    pipeline.match(W, cfg, d, d, s, s)   # (a keyword the byte count does not take raises TypeError here)
    assert [r[0] for r in prof.records] == ["matcher"]
    assert ("dual_softmax" if matcher == "DualSoftmax" else "sinkhorn") in fake.seen
