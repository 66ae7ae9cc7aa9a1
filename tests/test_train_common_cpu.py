"""mickey_amd._train_common without a GPU: what the train_*.py wrappers share and no other test reaches -- the swap traversal on
stand-in modules, a dual-softmax matcher registered under two parents, the in-place-or-copy decision of every layout adapter over a
table of stride patterns, and the exception class of arguments that are wrong in two ways at once.

The expected columns of LAYOUTS and TWICE_BAD are not derived from the code under test: they are what _rows, _rows2d, _channels_last,
_weight2d and the public ops of the commit BEFORE the shared module existed answered on these very inputs, recorded here as literals.
"""
import pytest
import torch
from torch import nn


# ---- the traversal -----------------------------------------------------------------------------------------------------------
class _Old(nn.Module):
    pass


class _New(nn.Module):
    def __init__(self, old):
        super().__init__()
        self.old_id = id(old)


class _Tree(nn.Module):
    def __init__(self):
        super().__init__()
        self.a = _Old()
        self.box = nn.Sequential(self.a, nn.ReLU(), _Old())   # self.a: one module under two parents
        self.register_module("absent", None)
        self.target = _Old()
        self.inner = nn.Module()
        self.inner.target = _Old()
        self.inner.other = _Old()


def _make(m):
    return _New(m) if isinstance(m, _Old) else None


def test_swap_modules_keeps_one_module_one_and_counts_registrations():
    from mickey_amd._train_common import swap_modules
    t = _Tree()
    olds = [t.a, t.box[2], t.target, t.inner.target, t.inner.other]
    seen = []

    def make(m):
        seen.append(m)
        return _make(m)

    assert swap_modules(t, make) == 6                       # five modules, one of them registered twice
    assert type(t.a) is _New and t.box[0] is t.a and t.a.old_id == id(olds[0])
    assert sorted(n.old_id for n in (t.a, t.box[2], t.target, t.inner.target, t.inner.other)) == sorted(id(o) for o in olds)
    assert all(m is not None for m in seen) and t.absent is None and "absent" in t._modules   # the None child: skipped, kept
    assert type(t.box[1]) is nn.ReLU and type(t.inner) is nn.Module
    assert list(t._modules) == ["a", "box", "absent", "target", "inner"]   # registration order survives
    assert swap_modules(t, make) == 0                       # a second call finds nothing
    assert swap_modules(_Old(), _make) == 0                 # the root itself has no parent to be replaced in


def test_swap_modules_name_restricts_the_search():
    from mickey_amd._train_common import swap_modules
    t = _Tree()
    assert swap_modules(t, _make, name="target") == 2
    assert type(t.target) is _New and type(t.inner.target) is _New
    assert type(t.a) is _Old and type(t.box[2]) is _Old and type(t.inner.other) is _Old
    assert swap_modules(t, _make, name="nothing_has_this_name") == 0
    assert swap_modules(t, _make) == 4                      # the rest: a (twice), box[2], inner.other


def test_swap_modules_a_raising_make_propagates_and_keeps_what_was_done():
    from mickey_amd._train_common import swap_modules
    t = _Tree()
    refuse = t.inner.target

    def make(m):
        if m is refuse:
            raise ValueError("not covered")
        return _make(m)

    with pytest.raises(ValueError, match="not covered"):
        swap_modules(t, make)
    assert type(t.a) is _New and t.box[0] is t.a and type(t.box[2]) is _New and type(t.target) is _New   # done before the error
    assert t.inner.target is refuse and type(t.inner.other) is _Old                                        # not reached


def test_adopt_takes_children_parameters_buffers_and_the_training_flag():
    from mickey_amd._train_common import adopt
    old = nn.Module()
    old.lin = nn.Linear(4, 4)
    old.p = nn.Parameter(torch.ones(3))
    old.register_buffer("kept", torch.zeros(2))
    old.register_buffer("scratch", torch.zeros(2), persistent=False)
    old.eval()

    class Twin(nn.Module):
        def __init__(self):
            raise AssertionError("adopt does not run __init__")

    new = adopt(Twin, old)
    assert type(new) is Twin and new.lin is old.lin and new.p is old.p and new.kept is old.kept and new.scratch is old.scratch
    assert list(new.state_dict()) == list(old.state_dict()) == ["p", "kept", "lin.weight", "lin.bias"]
    assert new.training is False and adopt(Twin, old.train()).training is True


# ---- the matcher under two parents ---------------------------------------------------------------------------------------------
class _Matcher(nn.Module):
    def __init__(self, dustbin=True):
        super().__init__()
        self.temperature = 0.1
        self.use_dustbin = dustbin
        if dustbin:
            self.dustbin_score = nn.Parameter(torch.tensor(1.))


class _Holder(nn.Module):
    def __init__(self, matcher):
        super().__init__()
        self.matching_mat = matcher


def test_a_matcher_under_two_parents_becomes_one_dual_softmax():
    from mickey_amd import train_matcher as tm
    shared = _Matcher()
    shared.eval()
    dustbin = shared.dustbin_score
    model = nn.ModuleDict({"first": _Holder(shared), "second": _Holder(shared), "own": _Holder(_Matcher(dustbin=False))})
    keys = list(model.state_dict())
    assert tm.use_hip_matcher(model, split=False) == 3
    one = model["first"].matching_mat
    assert type(one) is tm.DualSoftmax and model["second"].matching_mat is one
    assert one.dustbin_score is dustbin and one.use_dustbin and one.split is False and not one.training
    other = model["own"].matching_mat
    assert type(other) is tm.DualSoftmax and other is not one and not other.use_dustbin and other.training
    assert list(model.state_dict()) == keys
    assert len({id(p) for p in model.parameters()}) == 1 and next(model.parameters()) is dustbin
    assert tm.use_hip_matcher(model) == 0


# ---- the layout rule ---------------------------------------------------------------------------------------------------------
def _flat(n, offset=0):
    return torch.arange(n + offset, dtype=torch.float32)[offset:]


def _packed_third(i):
    return _flat(2 * 5 * 384).view(2, 5, 3, 8, 16)[:, :, i]                 # q, k or v of one packed [N, L, 3 C] buffer


# (adapter, case, the tensor, read in place?)
LAYOUTS = [
    ("rows", "contiguous", lambda: _flat(1280).view(2, 5, 8, 16), True),
    ("rows", "packed third q", lambda: _packed_third(0), True),
    ("rows", "packed third k", lambda: _packed_third(1), True),
    ("rows", "packed third v", lambda: _packed_third(2), True),
    ("rows", "head-major storage", lambda: _flat(1280).view(2, 8, 5, 16).permute(0, 2, 1, 3), False),
    ("rows", "dense at an odd storage offset", lambda: _flat(1280, 1).view(2, 5, 8, 16), False),
    ("rows", "expanded image dimension", lambda: _flat(640).view(1, 5, 8, 16).expand(2, 5, 8, 16), True),
    ("rows", "images 4 elements apart (overlapping images, whole rows)", lambda: _flat(1284).as_strided((2, 5, 8, 16), (4, 128, 16, 1)), True),
    ("rows", "row stride 130", lambda: _flat(1300).as_strided((2, 5, 8, 16), (650, 130, 16, 1)), False),
    ("rows", "image stride 642", lambda: _flat(1300).as_strided((2, 5, 8, 16), (642, 128, 16, 1)), False),
    ("rows", "overlapping rows", lambda: _flat(1300).as_strided((2, 5, 8, 16), (640, 64, 16, 1)), False),
    ("rows", "one token, any token stride", lambda: _flat(1300).as_strided((2, 1, 8, 16), (128, 3, 16, 1)), True),
    ("rows2d", "contiguous", lambda: _flat(1280).view(2, 5, 128), True),
    ("rows2d", "contiguous 2-D", lambda: _flat(1280).view(10, 128), True),
    ("rows2d", "packed third", lambda: _flat(3840).view(2, 5, 384)[..., 128:256], True),
    ("rows2d", "dense at an odd storage offset", lambda: _flat(1280, 1).view(2, 5, 128), False),
    ("rows2d", "packed third at an odd storage offset", lambda: _flat(3840, 1).view(2, 5, 384)[..., 128:256], False),
    ("rows2d", "expanded image dimension", lambda: _flat(640).view(1, 5, 128).expand(2, 5, 128), False),
    ("rows2d", "token-major storage", lambda: _flat(1280).view(5, 2, 128).permute(1, 0, 2), False),
    ("rows2d", "row stride 130", lambda: _flat(1300).as_strided((2, 5, 128), (650, 130, 1)), False),
    ("rows2d", "2-D slice of wider rows", lambda: _flat(2560).view(10, 256)[:, :128], False),
    ("rows2d", "one image, wider rows", lambda: _flat(1280).view(1, 5, 256)[..., :128], True),
    ("rows2d", "one token per image, wider rows", lambda: _flat(2560).view(2, 5, 256)[:, 2:3, :128], False),
    ("channels_last", "channels_last memory", lambda: _flat(2240).view(2, 5, 7, 32).permute(0, 3, 1, 2), True),
    ("channels_last", "NCHW contiguous", lambda: _flat(2240).view(2, 32, 5, 7), False),
    ("channels_last", "channels_last at an odd storage offset", lambda: _flat(2240, 3).view(2, 5, 7, 32).permute(0, 3, 1, 2), False),
    ("channels_last", "channel slice of a wider channels_last map", lambda: _flat(4480).view(2, 5, 7, 64).permute(0, 3, 1, 2)[:, :32], False),
    ("weight2d", "contiguous", lambda: _flat(64).view(2, 32, 1, 1), True),
    ("weight2d", "1x1 weight sliced from a wider one", lambda: _flat(128).view(2, 64, 1, 1)[:, :32], False),
    ("weight2d", "two rows of a taller one", lambda: _flat(128).view(4, 32, 1, 1)[1:3], True),
    ("weight2d", "two rows of a taller one, 8 bytes off", lambda: _flat(120).view(4, 30, 1, 1)[1:3], False),
    ("weight", "contiguous", lambda: _flat(128 * 128).view(128, 128), True),
    ("weight", "transposed", lambda: _flat(128 * 128).view(128, 128).t(), False),
    ("weight", "dense at an odd storage offset", lambda: _flat(128, 1), False),
]


@pytest.mark.parametrize("adapter,case,build,in_place", LAYOUTS, ids=["%s: %s" % (a, c) for a, c, _, _ in LAYOUTS])
def test_layout_decision(adapter, case, build, in_place):
    from mickey_amd import _train_common, train_attention, train_layer, train_tails
    fn = {"rows": train_attention._rows, "rows2d": train_layer._rows2d, "channels_last": train_tails._channels_last,
          "weight2d": train_tails._weight2d, "weight": _train_common.aligned_copy}[adapter]
    t = build()
    assert (t.data_ptr() % 16 != 0) == ("odd storage offset" in case or "bytes off" in case)   # what the case says it is
    out = fn(t)
    same_memory = out.data_ptr() == t.data_ptr() and out.untyped_storage().data_ptr() == t.untyped_storage().data_ptr()
    assert same_memory == in_place
    if adapter in ("rows", "channels_last", "weight"):
        assert (out is t) == in_place                       # the tensor itself, not a view of it
    if adapter == "rows2d":
        assert out.dim() == 2 and out.shape[1] == t.shape[-1] and out.stride(1) == 1
        if in_place:
            assert out.stride(0) == (t.stride(-2) if t.dim() > 1 and t.shape[-2] > 1 else t.shape[-1])
    if not in_place:
        kernel_view = out.permute(0, 2, 3, 1) if adapter == "channels_last" else out
        assert kernel_view.is_contiguous() and out.data_ptr() % 16 == 0
    assert torch.equal(out.reshape(-1) if adapter in ("rows2d", "weight2d") else out,
                       t.reshape(-1) if adapter in ("rows2d", "weight2d") else t)


# ---- arguments that are wrong in two ways: the class of the error ----------------------------------------------------------------
def _w(*shape):
    return torch.zeros(*shape)


def _layer_weights():
    return [_w(128, 128), _w(128, 128), _w(128, 128), _w(128, 128), _w(256, 256), _w(128, 256), _w(128), _w(128), _w(128), _w(128)]


# (op, what is wrong besides living on the CPU, the call, "hip" = MickeyHipError / "value" = ValueError)
TWICE_BAD = [
    ("conv3x3_train", "dtype", lambda m: m.train_heads.conv3x3_train(_w(1, 32, 4, 4).half(), _w(8, 32, 3, 3)), "hip"),
    ("conv3x3_train", "rank", lambda m: m.train_heads.conv3x3_train(_w(32, 4, 4), _w(8, 32, 3, 3)), "hip"),
    ("conv3x3_train", "channels", lambda m: m.train_heads.conv3x3_train(_w(1, 30, 4, 4), _w(8, 30, 3, 3)), "hip"),
    ("linear_attention_train", "dtype", lambda m: m.train_attention.linear_attention_train(*[_w(1, 3, 8, 16).half()] * 3), "value"),
    ("linear_attention_train", "rank", lambda m: m.train_attention.linear_attention_train(*[_w(3, 8, 16)] * 3), "value"),
    ("linear_attention_train", "eps", lambda m: m.train_attention.linear_attention_train(*[_w(1, 3, 8, 16)] * 3, eps=-1.0), "value"),
    ("encoder_layer_train", "dtype", lambda m: m.train_layer.encoder_layer_train(_w(1, 3, 128).double(), _w(1, 3, 128), *_layer_weights()), "value"),
    ("encoder_layer_train", "rank", lambda m: m.train_layer.encoder_layer_train(_w(3, 128), _w(3, 128), *_layer_weights()), "value"),
    ("linear_train", "dtype", lambda m: m.train_layer.linear_train(_w(3, 32).half(), _w(48, 32)), "value"),
    ("linear_train", "rank", lambda m: m.train_layer.linear_train(_w(3, 32), _w(48, 32, 1)), "value"),
    ("layernorm_train", "dtype", lambda m: m.train_layer.layernorm_train(_w(3, 128), _w(128).double(), _w(128)), "value"),
    ("layernorm_train", "width", lambda m: m.train_layer.layernorm_train(_w(3, 64), _w(128), _w(128)), "value"),
    ("score_tail_train", "dtype", lambda m: m.train_tails.score_tail_train(_w(1, 64, 4, 4).half(), _w(1, 64, 1, 1)), "value"),
    ("score_tail_train", "temperature", lambda m: m.train_tails.score_tail_train(_w(1, 64, 4, 4), _w(1, 64, 1, 1), temperature=0.0), "value"),
    ("offset_tail_train", "weight shape", lambda m: m.train_tails.offset_tail_train(_w(1, 64, 4, 4), _w(1, 64, 1, 1)), "value"),
    ("depth_tail_train", "rank", lambda m: m.train_tails.depth_tail_train(_w(64, 4, 4), _w(1, 64, 1, 1)), "value"),
    ("desc_l2norm_train", "width", lambda m: m.train_tails.desc_l2norm_train(_w(1, 130, 4, 4)), "value"),
    ("dual_softmax_train", "dtype", lambda m: m.train_matcher.dual_softmax_train(_w(1, 128, 5).half(), _w(1, 128, 6).half()), "value"),
    ("dual_softmax_train", "rank", lambda m: m.train_matcher.dual_softmax_train(_w(128, 5), _w(128, 6)), "value"),
    ("dual_softmax_train", "nothing else", lambda m: m.train_matcher.dual_softmax_train(_w(1, 128, 5), _w(1, 128, 6)), "value"),
]


@pytest.mark.parametrize("op,wrong,call,kind", TWICE_BAD, ids=["%s: CPU and %s" % (o, w) for o, w, _, _ in TWICE_BAD])
def test_exception_class_of_cpu_tensors_that_are_also_wrong(op, wrong, call, kind, monkeypatch):
    import mickey_amd
    from mickey_amd import _native, train_attention, train_heads, train_layer, train_matcher, train_tails   # noqa: F401

    def touched(*a, **k):
        raise AssertionError("%s reached the library" % op)

    monkeypatch.setattr(_native, "load", touched)
    expected = _native.MickeyHipError if kind == "hip" else ValueError
    with pytest.raises(expected) as e:
        call(mickey_amd)
    assert type(e.value) is expected                        # (MickeyHipError is no ValueError, but pin the exact class anyway)
    assert str(e.value).startswith(op)
