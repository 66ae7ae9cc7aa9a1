"""-m gpu: pair-list mode (README "Pair-list mode") is the standard forward on the materialised pairs, bit for bit.

  * each *_pairs entry point == the entry point without a suffix on the materialised operands (dsc[i0], dsc[i1], scr[i0], ...);
  * the *_kf entry points are the idx1 = NULL case of the *_pairs ones;
  * a pair whose map entry is out of range is refused before any load: its outputs stay unwritten, the other pairs are right
    and nothing is written outside the buffers;
  * the model's pair-list forward == its standard forward on images[pair_index[:, 0]], images[pair_index[:, 1]] (every per-pair
    output, the poses, the inlier lists) and the per-image outputs == the expanded forward's rows of that image, in five
    configurations, for any chunking, with one encode per image, under the batch-level invalid rule, with AMD.GRAPH: True
    (stays eager) and at the benchmarked size."""
import copy

import pytest
import torch

from tests.helpers import guarded

pytestmark = pytest.mark.gpu

PAIRS3 = [[2, 0], [0, 2], [1, 1], [2, 1], [0, 1]]   # N = 3, P = 5 (padded to 8 units): every image on both sides, one self pair
PAIRS12 = [[11, 0], [3, 7], [7, 3], [0, 11], [5, 5], [11, 11], [1, 0], [3, 1], [7, 7]]   # N = 12 > P = 9 (padded to 16): 2, 4, 6, 8, 9, 10 unused
PAIRS34 = [[2, 3], [0, 0], [1, 3], [2, 1], [0, 2]]   # two sets: N0 = 3, N1 = 4


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _unit_dsc(n, nimg, g, dev, C=128):
    d = torch.randn((nimg, C, n), generator=g)
    return (d / d.norm(dim=1, keepdim=True)).to(dev).contiguous()


def _eq(a, b):
    if a is None or b is None:
        return a is None and b is None
    return torch.equal(a, b)


def _maps(pairs, dev):
    t = torch.tensor(pairs, device=dev, dtype=torch.long)
    return t[:, 0].contiguous(), t[:, 1].contiguous()


def _matchers_equal_materialised(dsc0, dsc1, scr0, scr1, pairs):
    """every dual-softmax variant (and Sinkhorn) with pair_index= against the plain call on the materialised operands"""
    from mickey_amd import ops
    dev = dsc0.device
    i0, i1 = _maps(pairs, dev)
    e0, e1, es0, es1 = dsc0[i0].contiguous(), dsc1[i1].contiguous(), scr0[i0].contiguous(), scr1[i1].contiguous()
    pi = torch.tensor(pairs, device=dev, dtype=torch.int32)
    for split in (False, True):
        for dustbin in (None, 1.25):
            for lean in (False, True):
                kw = dict(temperature=0.1, dustbin=dustbin, want_scores=not lean, want_kp=not lean, want_final=True, split=split)
                want = ops.dual_softmax(e0, e1, es0, es1, **kw)
                got = ops.dual_softmax(dsc0, dsc1, scr0, scr1, pair_index=pi, **kw)
                for w, o in zip(want, got):
                    assert _eq(w, o), (split, dustbin, lean)
                # a host list takes the same kernels
                assert torch.equal(ops.dual_softmax(dsc0, dsc1, scr0, scr1, pair_index=pairs, **kw)[2], want[2])
    want = ops.sinkhorn(e0, e1, 1.0, 10, es0, es1, want_scores=True, want_kp=True, want_final=True)
    got = ops.sinkhorn(dsc0, dsc1, 1.0, 10, scr0, scr1, want_scores=True, want_kp=True, want_final=True, pair_index=pi)
    assert all(torch.equal(w, o) for w, o in zip(want, got))
    got = ops.sinkhorn(dsc0, dsc1, 1.0, 10, scr0, scr1, want_scores=False, want_kp=False, want_final=True, pair_index=pairs)
    assert torch.equal(got[2], want[2]) and got[0] is None


# ---- 1: the entry points against materialised operands -----------------------------------------------------------------------------
@pytest.mark.parametrize("n", [257, 258, 196])   # 1-, 2- and 4-float store paths; 257 / 258 / 196 end in a partial 32-row block
@pytest.mark.parametrize("pairs, N", [(PAIRS3, 3), (PAIRS12, 12)], ids=["N3_P5", "N12_P9"])
def test_matchers_pairs_equal_materialised_one_set(n, pairs, N):
    dev = _dev()
    g = torch.Generator().manual_seed(n * 7 + N)
    dsc = _unit_dsc(n, N, g, dev)
    scr = torch.rand((N, n), generator=g).to(dev)
    _matchers_equal_materialised(dsc, dsc, scr, scr, pairs)


def test_matchers_pairs_equal_materialised_two_sets():
    dev = _dev()
    g = torch.Generator().manual_seed(41)
    n0, n1 = 300, 257
    dsc0, dsc1 = _unit_dsc(n0, 3, g, dev), _unit_dsc(n1, 4, g, dev)
    scr0, scr1 = torch.rand((3, n0), generator=g).to(dev), torch.rand((4, n1), generator=g).to(dev)
    _matchers_equal_materialised(dsc0, dsc1, scr0, scr1, PAIRS34)


def _gather_case(N0, N1, P, n0, n1, rows, k, dev, seed=5):
    g = torch.Generator().manual_seed(seed)
    fs = torch.rand((P, n0, n1), generator=g).to(dev)
    kps0 = (torch.rand((N0, 2, n0), generator=g) * 500).to(dev)
    dep0 = (torch.rand((N0, 1, n0), generator=g) * 5 + 0.1).to(dev)
    kps1 = (torch.rand((N1, 2, n1), generator=g) * 500).to(dev)
    dep1 = (torch.rand((N1, 1, n1), generator=g) * 5 + 0.1).to(dev)
    Km = torch.tensor([[500.0, 0, 250], [0, 510, 260], [0, 0, 1]])
    K0 = (Km + torch.rand((P, 3, 3), generator=g) * torch.tensor([[5.0, 0, 5], [0, 5, 5], [0, 0, 0]])).to(dev)
    K1 = (Km + torch.rand((P, 3, 3), generator=g) * torch.tensor([[5.0, 0, 5], [0, 5, 5], [0, 0, 0]])).to(dev)
    idx = torch.randint(0, n0 * n1, (P * rows, k), generator=g, dtype=torch.int32).to(dev)
    return idx, fs, kps0, dep0, kps1, dep1, K0, K1


@pytest.mark.parametrize("pairs, N0, N1, n0, n1", [(PAIRS3, 3, 3, 257, 257), (PAIRS12, 12, 12, 196, 196), (PAIRS34, 3, 4, 300, 257)],
                         ids=["N3_P5", "N12_P9", "two_sets"])
def test_gather_backproject_pairs_equals_materialised(pairs, N0, N1, n0, n1):
    from mickey_amd import ops
    dev = _dev()
    rows, k = 4, 96
    idx, fs, kps0, dep0, kps1, dep1, K0, K1 = _gather_case(N0, N1, len(pairs), n0, n1, rows, k, dev)
    if N0 == N1 and n0 == n1:   # one image set on both sides
        kps1, dep1 = kps0, dep0
    i0, i1 = _maps(pairs, dev)
    want = ops.gather_backproject(idx, fs, kps0[i0], dep0[i0], kps1[i1], dep1[i1], K0, K1, rows)
    got = ops.gather_backproject(idx, fs, kps0, dep0, kps1, dep1, K0, K1, rows,
                                 pair_index=torch.tensor(pairs, device=dev, dtype=torch.int32))
    assert all(torch.equal(w, o) for w, o in zip(want, got))
    got = ops.gather_backproject(idx, fs, kps0, dep0, kps1, dep1, K0, K1, rows, pair_index=pairs)
    assert all(torch.equal(w, o) for w, o in zip(want, got))


# ---- 2: _kf is the idx1 = NULL case ------------------------------------------------------------------------------------------------
def test_kf_is_the_pairs_call_without_a_second_map():
    from mickey_amd import ops
    dev = _dev()
    g = torch.Generator().manual_seed(9)
    kmap = [2, 0, 2, 1, 0]
    K, B, n0, n1 = 3, 5, 300, 257
    kf = torch.tensor(kmap, device=dev, dtype=torch.int32)
    dsc0, dsc1 = _unit_dsc(n0, K, g, dev), _unit_dsc(n1, B, g, dev)
    scr0, scr1 = torch.rand((K, n0), generator=g).to(dev), torch.rand((B, n1), generator=g).to(dev)
    for split in (False, True):
        kw = dict(temperature=0.1, dustbin=1.25, split=split)
        want = ops.dual_softmax(dsc0, dsc1, scr0, scr1, keyframe_index=kf, **kw)
        got = ops.dual_softmax(dsc0, dsc1, scr0, scr1, pair_index=(kf, None), **kw)
        assert all(torch.equal(w, o) for w, o in zip(want, got)), split
    want = ops.sinkhorn(dsc0, dsc1, 1.0, 10, scr0, scr1, want_kp=True, want_final=True, keyframe_index=kf)
    got = ops.sinkhorn(dsc0, dsc1, 1.0, 10, scr0, scr1, want_kp=True, want_final=True, pair_index=(kf, None))
    assert all(torch.equal(w, o) for w, o in zip(want, got))
    idx, fs, kps0, dep0, kps1, dep1, K0, K1 = _gather_case(K, B, B, n0, n1, 4, 96, dev)
    want = ops.gather_backproject(idx, fs, kps0, dep0, kps1, dep1, K0, K1, 4, keyframe_index=kf)
    got = ops.gather_backproject(idx, fs, kps0, dep0, kps1, dep1, K0, K1, 4, pair_index=(kf, None))
    assert all(torch.equal(w, o) for w, o in zip(want, got))
    # both maps absent: the plain call
    e0, es0 = dsc0[kf.long()].contiguous(), scr0[kf.long()].contiguous()
    want = ops.dual_softmax(e0, dsc1, es0, scr1, temperature=0.1, split=True)
    got = ops.dual_softmax(e0, dsc1, es0, scr1, temperature=0.1, split=True, pair_index=(None, None))
    assert all(torch.equal(w, o) for w, o in zip(want, got))


# ---- 3: out-of-range entries -------------------------------------------------------------------------------------------------------
def _untouched(t):
    return bool((guarded.bits(t) == guarded.sentinel_bits(t.dtype)).all())


def _written(t):
    return not bool((guarded.bits(t) == guarded.sentinel_bits(t.dtype)).any())


# (which map, which pair, the entry): one below the range, one just past it, one far past it
BAD_ENTRIES = [(0, 1, -1), (1, 0, 3), (1, 2, 1 << 30)]


@pytest.mark.parametrize("entry", ["mk_dual_softmax_pairs", "mk_dual_softmax_split_pairs", "mk_sinkhorn_pairs"])
@pytest.mark.parametrize("side, bad_pair, value", BAD_ENTRIES)
def test_matcher_pairs_refuse_an_out_of_range_entry(entry, side, bad_pair, value):
    from mickey_amd import _native as nv, ops
    dev = _dev()
    g = torch.Generator().manual_seed(17)
    N, n, C = 3, 70, 128
    pairs = [[2, 0], [0, 2], [1, 1]]
    P = len(pairs)
    dsc, scr = _unit_dsc(n, N, g, dev), torch.rand((N, n), generator=g).to(dev)
    if entry == "mk_sinkhorn_pairs":
        want = ops.sinkhorn(dsc, dsc, 1.0, 10, scr, scr, want_scores=True, want_kp=True, want_final=True, pair_index=pairs)
    else:
        want = ops.dual_softmax(dsc, dsc, scr, scr, temperature=0.1, dustbin=1.25, split="split" in entry, pair_index=pairs)
    maps = torch.tensor(pairs, dtype=torch.int32).t().contiguous()
    maps[side, bad_pair] = value
    maps = maps.to(dev)
    outs, checks = zip(*[guarded.guarded(P * n, n, torch.float32, dev) for _ in range(3)])
    if entry == "mk_dual_softmax_pairs":
        nwork = nv.query("mk_dual_softmax_work_floats", P, n, n, 0)
    elif entry == "mk_dual_softmax_split_pairs":
        nwork = nv.query("mk_dual_softmax_split_pairs_work_floats", P, n, n, N, N, 1)
    else:
        nwork = nv.query("mk_sinkhorn_work_floats", P, n, n)
    work, wcheck = guarded.guarded(1, nwork, torch.float32, dev)
    tail = (nv.ptr(outs[0]), nv.ptr(outs[1]), nv.ptr(outs[2]), nv.ptr(work), P, C, n, n, nv.ptr(maps[0]), nv.ptr(maps[1]), N, N, nv.stream())
    if entry == "mk_sinkhorn_pairs":
        nv.call(entry, nv.ptr(dsc), nv.ptr(dsc), nv.ptr(scr), nv.ptr(scr), 1.0, 10, *tail)
    else:
        nv.call(entry, nv.ptr(dsc), nv.ptr(dsc), nv.ptr(scr), nv.ptr(scr), 10.0, 1, 1.25, *tail)
    torch.cuda.synchronize()
    for chk in checks + (wcheck,):
        chk()
    for o, w, name in zip(outs, want, ("scores", "kp_scores", "final_scores")):
        o = o.reshape(P, n, n)
        for p in range(P):
            if p == bad_pair:
                assert _untouched(o[p]), "%s: the refused pair %d was written" % (name, p)
            else:
                assert _written(o[p]) and torch.equal(o[p], w[p]), "%s: pair %d" % (name, p)


@pytest.mark.parametrize("side, bad_pair, value", BAD_ENTRIES)
def test_gather_backproject_pairs_refuses_an_out_of_range_entry(side, bad_pair, value):
    from mickey_amd import _native as nv, ops
    dev = _dev()
    N, n, rows, k = 3, 70, 4, 96
    pairs = [[2, 0], [0, 2], [1, 1]]
    P = len(pairs)
    idx, fs, kps, dep, _, _, K0, K1 = _gather_case(N, N, P, n, n, rows, k, dev)
    want = ops.gather_backproject(idx, fs, kps, dep, kps, dep, K0, K1, rows, pair_index=pairs)
    maps = torch.tensor(pairs, dtype=torch.int32).t().contiguous()
    maps[side, bad_pair] = value
    maps = maps.to(dev)
    outs, checks = zip(*[guarded.guarded(P * rows, k * w, torch.float32, dev) for w in (3, 3, 1, 6)])
    nv.call("mk_gather_backproject_pairs", nv.ptr(idx), nv.ptr(fs), nv.ptr(kps), nv.ptr(dep), nv.ptr(kps), nv.ptr(dep), nv.ptr(K0), nv.ptr(K1),
            *[nv.ptr(o) for o in outs], P, rows, k, n, n, nv.ptr(maps[0]), nv.ptr(maps[1]), N, N, nv.stream())
    torch.cuda.synchronize()
    for chk in checks:
        chk()
    for o, w, name in zip(outs, want, ("X", "Y", "wts", "corr")):
        o, w = o.reshape(P, -1), w.reshape(P, -1)
        for p in range(P):
            if p == bad_pair:
                assert _untouched(o[p]), "%s: the refused pair %d was written" % (name, p)
            else:
                assert _written(o[p]) and torch.equal(o[p], w[p]), "%s: pair %d" % (name, p)


# ---- 4 - 9: the model ---------------------------------------------------------------------------------------------------------------
PER_PAIR = ("scores", "kp_scores", "final_scores", "R", "t", "inliers")
PER_IMAGE = ("kps", "depth_kp", "scr", "dsc", "depth_map")   # pair-list key; the standard forward's are kps0 / kps1, ..., depth0_map / depth1_map
CONFIGS = {
    "headline": {"ENCODER_DTYPE": "bf16"},
    "split_heads": {"ENCODER_DTYPE": "fp16", "HEADS_DTYPE": "split"},
    "fp32": {"ENCODER_DTYPE": "fp32"},
    "sinkhorn": {"ENCODER_DTYPE": "bf16"},
    "lean_fp32_corr": {"ENCODER_DTYPE": "bf16", "LEAN": True, "MATCHER_CORR": "fp32"},
}
MODEL_PAIRS = [[3, 1], [0, 3], [3, 2], [1, 0], [0, 3]]   # N = 4, P = 5: unsorted, images repeated on each side, a duplicated pair


def _model(cfg, amd, sinkhorn=False):
    from mickey_amd import synthetic as syn
    from mickey_amd.model import MickeyRelativePose
    c = copy.deepcopy(cfg)
    c["AMD"]["GRAPH"] = False
    c["AMD"].update(amd)
    if sinkhorn:
        c["FEATURE_MATCHER"]["TYPE"] = "Sinkhorn"
    model = MickeyRelativePose(c)
    model.load_state_dict(syn.mickey_state_dict(c, seed=0))
    return model.cuda()


def _image_set(N, H, W, dev, seed=77):
    """N images and per-image intrinsics that differ"""
    from mickey_amd import synthetic as syn
    batch = syn.synthetic_batch(B=N, H=H, W=W, seed=seed)
    K = batch["K_color0"].clone()
    K[:, 0, 0] += torch.arange(N, dtype=torch.float32)
    K[:, 1, 2] -= 0.5 * torch.arange(N, dtype=torch.float32)
    return batch["image0"].to(dev), K.to(dev)


def _expanded(images, K, pairs, pair_base):
    i0, i1 = _maps(pairs, images.device)
    return {"image0": images[i0], "image1": images[i1], "K_color0": K[i0], "K_color1": K[i1], "pair_base": pair_base}


def _pairlist(images, K, pairs, pair_base):
    return {"images": images, "K_color": K, "pair_index": pairs, "pair_base": pair_base}


def _run(model, data, inliers=False, seed=3):
    model.reseed(seed, 0)
    model(data, return_inliers=inliers)
    return data


def _same_pairs(std, pl, keys=PER_PAIR):
    for k in keys:
        if k in std:
            assert k in pl and torch.equal(std[k], pl[k]), k
    if "inliers_list" in std:
        assert len(std["inliers_list"]) == len(pl["inliers_list"])
        assert all(torch.equal(a, b) for a, b in zip(std["inliers_list"], pl["inliers_list"]))


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_forward_equals_expanded_forward(cfg, name):
    dev = _dev()
    model = _model(cfg, dict(CONFIGS[name], PAIRLIST_SCORES=True), sinkhorn=name == "sinkhorn")
    N, H, W = 4, 182, 196
    images, K = _image_set(N, H, W, dev)
    pairs = torch.tensor(MODEL_PAIRS, dtype=torch.int32, device=dev)   # given as a device tensor
    std = _run(model, _expanded(images, K, MODEL_PAIRS, 3), inliers=not model.lean)
    pl = _run(model, _pairlist(images, K, pairs, 3), inliers=not model.lean)
    _same_pairs(std, pl)
    assert ("scores" in pl) == (not model.lean) and "final_scores" in pl
    assert torch.equal(pl["K_color0"], std["K_color0"]) and torch.equal(pl["K_color1"], std["K_color1"])
    assert pl["kps_shape"] == std["kps0_shape"] and pl["down_factor"] == std["down_factor"]
    for k in PER_IMAGE:
        assert pl[k].shape[0] == N, k
        for side in (0, 1):
            sk = k.replace("depth_map", "depth%d_map") % side if k == "depth_map" else "%s%d" % (k, side)
            for p, row in enumerate(MODEL_PAIRS):
                assert torch.equal(std[sk][p], pl[k][row[side]]), (k, side, p)
    assert torch.isfinite(pl["R"]).all() and pl["pair_index"] is pairs


@pytest.fixture(scope="module")
def headline(cfg):
    """one headline-configuration model for the tests below; `amd` sets AMD keys that the forward reads per call"""
    model = _model(cfg, CONFIGS["headline"])
    defaults = copy.deepcopy(model.cfg["AMD"])

    def amd(**kw):
        model.cfg["AMD"].clear()
        model.cfg["AMD"].update(defaults)
        model.cfg["AMD"].update(kw)
        model.graph_mode = model.cfg["AMD"]["GRAPH"]
        model._graphs.clear()
        return model

    yield amd
    amd()


def test_chunking_does_not_change_anything(headline):
    dev = _dev()
    images, K = _image_set(4, 182, 196, dev)
    ref = _run(headline(PAIRLIST_SCORES=True), _pairlist(images, K, MODEL_PAIRS, 3), inliers=True)
    model = headline(PAIRLIST_SCORES=True, PAIR_CHUNK=2, IMAGE_CHUNK=3)
    out = _run(model, _pairlist(images, K, MODEL_PAIRS, 3), inliers=True)
    _same_pairs(ref, out)
    for k in PER_IMAGE + ("K_color0", "K_color1"):
        assert torch.equal(ref[k], out[k]), k
    # one Philox call number per forward, whatever the chunking: the counter stands where one standard forward leaves it
    assert model._calls == 1 and int(model._ctr.item()) == 2
    std = _run(model, _expanded(images, K, MODEL_PAIRS, 3))
    assert model._calls == 1 and int(model._ctr.item()) == 2
    _same_pairs(std, out, keys=("R", "t", "inliers"))
    # without PAIRLIST_SCORES the dense matrices stay out of `data`; the poses are the same
    plain = _run(headline(PAIR_CHUNK=2), _pairlist(images, K, MODEL_PAIRS, 3))
    assert not any(k in plain for k in ("scores", "kp_scores", "final_scores"))
    _same_pairs(std, plain, keys=("R", "t", "inliers"))


def test_every_image_is_encoded_once(headline, monkeypatch):
    from mickey_amd import pipeline
    dev = _dev()
    model = headline()
    images, K = _image_set(4, 182, 196, dev)
    seen = []
    real = pipeline.encoder_forward

    def counting(W, ws, img):
        seen.append(sum(t.shape[0] for t in img) if isinstance(img, (list, tuple)) else img.shape[0])
        return real(W, ws, img)

    monkeypatch.setattr(pipeline, "encoder_forward", counting)
    _run(model, _pairlist(images, K, MODEL_PAIRS, 0))
    assert sum(seen) == 4
    seen.clear()
    _run(model, _expanded(images, K, MODEL_PAIRS, 0))
    assert sum(seen) == 10


def test_one_invalid_pair_zeroes_every_pose(headline, monkeypatch):
    """One image is all-NaN and only the last pair -- the last chunk -- uses it.  The NaN does not reach the matcher on its own in
    either forward (the heads' ReLUs are maximum instructions, which drop a NaN operand: measured, both forwards return the same
    non-zero poses), so the test first checks exactly that, then carries the NaN over to that image's keypoint scores, where the
    sampler meets it as a NaN probability and sets the invalid word: every pose of the batch is zero in both forwards."""
    from mickey_amd import pipeline
    dev = _dev()
    model = headline(PAIR_CHUNK=2)
    images, K = _image_set(5, 182, 196, dev)
    images[4] = float("nan")
    pairs = [[3, 1], [0, 3], [3, 2], [1, 0], [2, 4]]
    std = _run(model, _expanded(images, K, pairs, 0))
    pl = _run(model, _pairlist(images, K, pairs, 0))
    _same_pairs(std, pl, keys=("R", "t", "inliers"))
    enc, heads, bad = pipeline.encoder_forward, pipeline.heads_forward, []

    def encoder(W, ws, img):
        ims = img if isinstance(img, (list, tuple)) else [img]
        bad.append(torch.cat([torch.isnan(t[:, 0, 0, 0]) for t in ims]))
        return enc(W, ws, img)

    def heads_nan(*a, **kw):
        scr, kps, depth, dsc = heads(*a, **kw)
        return scr.masked_fill_(bad.pop().view(-1, 1, 1), float("nan")), kps, depth, dsc

    monkeypatch.setattr(pipeline, "encoder_forward", encoder)
    monkeypatch.setattr(pipeline, "heads_forward", heads_nan)
    std = _run(model, _expanded(images, K, pairs, 0))
    pl = _run(model, _pairlist(images, K, pairs, 0))
    assert bool(torch.isnan(pl["scr"][4]).all()) and not bool(torch.isnan(pl["scr"][:4]).any())
    for k in ("R", "t", "inliers"):
        assert torch.equal(std[k], pl[k]) and not bool(pl[k].any()), k
    # the same forward without the bad pair: the standard forward's poses, and they are poses
    std4 = _run(model, _expanded(images, K, pairs[:4], 0))
    ok = _run(model, _pairlist(images, K, pairs[:4], 0))
    _same_pairs(std4, ok, keys=("R", "t", "inliers"))
    assert torch.isfinite(ok["R"]).all() and bool(ok["R"].any())


def test_graph_mode_leaves_pair_list_mode_eager(headline):
    dev = _dev()
    images, K = _image_set(3, 182, 196, dev, seed=5)
    pairs = [[0, 1], [1, 2]]
    ref = _run(headline(PAIRLIST_SCORES=True), _pairlist(images, K, pairs, 0), seed=1)
    graphed = headline(PAIRLIST_SCORES=True, GRAPH=True)
    assert graphed.graph_mode is True
    out = _run(graphed, _pairlist(images, K, pairs, 0), seed=1)
    assert len(graphed._graphs) == 0
    for k in ("final_scores", "R", "t", "inliers", "kps", "dsc"):
        assert torch.equal(ref[k], out[k]), k


def test_bench_size_headline(headline):
    dev = _dev()
    model = headline()
    images, K = _image_set(9, 720, 540, dev, seed=1234)
    pairs = [[i, i + 1] for i in range(8)]   # a 9-frame sequence
    std = _run(model, _expanded(images, K, pairs, 0))
    pl = _run(model, _pairlist(images, K, pairs, 0))
    _same_pairs(std, pl, keys=("R", "t", "inliers"))
    assert torch.isfinite(pl["R"]).all()
