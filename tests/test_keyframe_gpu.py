"""-m gpu: keyframe mode (README "Keyframe mode") is the standard forward on the expanded batch, bit for bit.

  * each *_kf entry point == the entry point without _kf on the materialised operand 0 (dsc0[map], scr0[map], kps0[map], ...);
  * the model's keyframe forward == its standard forward on image0[map] (every per-pair output, the poses, the inlier lists) and
    the per-keyframe outputs == the expanded forward's rows of that keyframe -- at a small size in four configurations and at
    the benchmarked size;
  * AMD.GRAPH: True leaves keyframe mode eager;
  * the Map-free harness with --share_keyframes writes the same submission.zip and decodes fewer frames."""
import copy
import zipfile

import pytest
import torch

pytestmark = pytest.mark.gpu

MAP = [2, 0, 2, 1, 0]   # K = 3, B = 5


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


@pytest.mark.parametrize("n0, n1", [(300, 257), (196, 196)])
def test_matcher_kf_equals_materialised(n0, n1):
    from mickey_amd import ops
    dev = _dev()
    g = torch.Generator().manual_seed(n0 * 7 + n1)
    K, B = 3, len(MAP)
    m = torch.tensor(MAP, device=dev, dtype=torch.long)
    kf = torch.tensor(MAP, device=dev, dtype=torch.int32)
    dsc0, dsc1 = _unit_dsc(n0, K, g, dev), _unit_dsc(n1, B, g, dev)
    scr0, scr1 = torch.rand((K, n0), generator=g).to(dev), torch.rand((B, n1), generator=g).to(dev)
    e0, es0 = dsc0[m].contiguous(), scr0[m].contiguous()
    for split in (False, True):
        for dustbin in (None, 1.25):
            for lean in (False, True):
                kw = dict(temperature=0.1, dustbin=dustbin, want_scores=not lean, want_kp=not lean, want_final=True, split=split)
                want = ops.dual_softmax(e0, dsc1, es0, scr1, **kw)
                got = ops.dual_softmax(dsc0, dsc1, scr0, scr1, keyframe_index=kf, **kw)
                for w, o in zip(want, got):
                    assert _eq(w, o), (split, dustbin, lean)
                # a host map (list) takes the same kernels
                assert torch.equal(ops.dual_softmax(dsc0, dsc1, scr0, scr1, keyframe_index=MAP, **kw)[2], want[2])
    want = ops.sinkhorn(e0, dsc1, 1.0, 10, es0, scr1, want_scores=True, want_kp=True, want_final=True)
    got = ops.sinkhorn(dsc0, dsc1, 1.0, 10, scr0, scr1, want_scores=True, want_kp=True, want_final=True, keyframe_index=kf)
    assert all(torch.equal(w, o) for w, o in zip(want, got))
    got = ops.sinkhorn(dsc0, dsc1, 1.0, 10, scr0, scr1, want_scores=False, want_kp=False, want_final=True, keyframe_index=kf)
    assert torch.equal(got[2], want[2]) and got[0] is None


def test_gather_backproject_kf_equals_materialised():
    from mickey_amd import ops
    dev = _dev()
    g = torch.Generator().manual_seed(5)
    K, B, n0, n1, rows, k = 3, len(MAP), 300, 257, 4, 96
    m = torch.tensor(MAP, device=dev, dtype=torch.long)
    fs = torch.rand((B, n0, n1), generator=g).to(dev)
    kps0 = (torch.rand((K, 2, n0), generator=g) * 500).to(dev)
    dep0 = (torch.rand((K, 1, n0), generator=g) * 5 + 0.1).to(dev)
    kps1 = (torch.rand((B, 2, n1), generator=g) * 500).to(dev)
    dep1 = (torch.rand((B, 1, n1), generator=g) * 5 + 0.1).to(dev)
    Km = torch.tensor([[500.0, 0, 250], [0, 510, 260], [0, 0, 1]])
    K0 = (Km + torch.rand((B, 3, 3), generator=g) * torch.tensor([[5.0, 0, 5], [0, 5, 5], [0, 0, 0]])).to(dev)
    K1 = (Km + torch.rand((B, 3, 3), generator=g) * torch.tensor([[5.0, 0, 5], [0, 5, 5], [0, 0, 0]])).to(dev)
    idx = torch.randint(0, n0 * n1, (B * rows, k), generator=g, dtype=torch.int32).to(dev)
    want = ops.gather_backproject(idx, fs, kps0[m], dep0[m], kps1, dep1, K0, K1, rows)
    got = ops.gather_backproject(idx, fs, kps0, dep0, kps1, dep1, K0, K1, rows,
                                 keyframe_index=torch.tensor(MAP, device=dev, dtype=torch.int32))
    assert all(torch.equal(w, o) for w, o in zip(want, got))


PER_PAIR = ("kps1", "depth_kp1", "scr1", "dsc1", "depth1_map", "scores", "kp_scores", "final_scores", "R", "t", "inliers")
PER_KEYFRAME = ("kps0", "depth_kp0", "scr0", "dsc0", "depth0_map")
CONFIGS = {
    "headline": {"ENCODER_DTYPE": "bf16"},
    "split_heads": {"ENCODER_DTYPE": "fp16", "HEADS_DTYPE": "split"},
    "fp32": {"ENCODER_DTYPE": "fp32"},
    "sinkhorn": {"ENCODER_DTYPE": "bf16"},
    "lean_fp32_corr": {"ENCODER_DTYPE": "bf16", "LEAN": True, "MATCHER_CORR": "fp32"},
}


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


def _compare(model, frames0, frames1, kmap, K0, K1, pair_base, inliers=True):
    """standard forward on image0[map] vs keyframe forward; returns (expanded data, keyframe data)"""
    dev = frames1.device
    m = torch.as_tensor(kmap, dtype=torch.long)
    std = {"image0": frames0[m.to(dev)], "image1": frames1, "K_color0": K0, "K_color1": K1, "pair_base": pair_base}
    kfd = {"image0": frames0, "image1": frames1, "K_color0": K0, "K_color1": K1, "pair_base": pair_base, "keyframe_index": kmap}
    model.reseed(3, 0)
    model(std, return_inliers=inliers)
    model.reseed(3, 0)
    model(kfd, return_inliers=inliers)
    for k in PER_PAIR:
        if k in std:
            assert k in kfd and torch.equal(std[k], kfd[k]), k
    for k in PER_KEYFRAME:
        assert kfd[k].shape[0] == frames0.shape[0], k
        for b, j in enumerate(m.tolist()):
            assert torch.equal(std[k][b], kfd[k][j]), (k, b, j)
    if inliers:
        assert len(std["inliers_list"]) == len(kfd["inliers_list"])
        assert all(torch.equal(a, b) for a, b in zip(std["inliers_list"], kfd["inliers_list"]))
    assert kfd["keyframe_index"] is kmap
    return std, kfd


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_forward_equals_expanded_forward(cfg, name):
    from mickey_amd import synthetic as syn
    dev = _dev()
    model = _model(cfg, CONFIGS[name], sinkhorn=name == "sinkhorn")
    B, K, H, W = 5, 2, 182, 196
    batch = syn.synthetic_batch(B=B, H=H, W=W, seed=77)
    frames0 = batch["image0"][:K].to(dev)
    kmap = torch.tensor([1, 0, 1, 1, 0], dtype=torch.int32, device=dev)   # unsorted, given as a device tensor
    K0 = batch["K_color0"].to(dev)
    K0[:, 0, 0] += torch.arange(B, device=dev, dtype=torch.float32)    # per-pair intrinsics of image 0
    std, kfd = _compare(model, frames0, batch["image1"].to(dev), kmap, K0, batch["K_color1"].to(dev), pair_base=3,
                        inliers=not model.lean)
    assert torch.isfinite(kfd["R"]).all()


def test_bench_size_headline(cfg):
    from mickey_amd import synthetic as syn
    dev = _dev()
    model = _model(cfg, CONFIGS["headline"])
    B = 32
    batch = syn.synthetic_batch(B=B, H=720, W=540, seed=1234)
    frames0 = batch["image0"][:1].to(dev)
    kmap = [0] * B
    std, kfd = _compare(model, frames0, batch["image1"].to(dev), kmap, batch["K_color0"].to(dev), batch["K_color1"].to(dev),
                        pair_base=0, inliers=False)
    for k in ("final_scores", "R", "t", "inliers"):
        assert torch.equal(std[k], kfd[k]), k


def test_graph_mode_leaves_keyframe_mode_eager(cfg):
    from mickey_amd import synthetic as syn
    dev = _dev()
    model = _model(cfg, {"ENCODER_DTYPE": "bf16"})
    batch = syn.synthetic_batch(B=2, H=182, W=196, seed=5)
    data = {k: v.to(dev) for k, v in batch.items()}
    data["image0"] = data["image0"][:1]
    data["keyframe_index"] = [0, 0]
    model.reseed(1, 0)
    ref = dict(data)
    model(ref)
    graphed = _model(cfg, {"ENCODER_DTYPE": "bf16", "GRAPH": True})
    graphed.reseed(1, 0)
    out = dict(data)
    graphed(out)
    assert len(graphed._graphs) == 0
    for k in ("final_scores", "R", "t", "inliers", "kps0", "kps1"):
        assert torch.equal(ref[k], out[k]), k


def test_mapfree_share_keyframes_same_zip_fewer_decodes(cfg, tmp_path):
    from mickey_amd import mapfree_eval as ME, synthetic as syn
    from mickey_amd.model import MickeyRelativePose
    from tests.helpers import tiny_mapfree
    dev = _dev()
    tiny_mapfree.make(str(tmp_path), "val", scenes=("s00460", "s00461"), queries=11, size=(196, 182))
    model = MickeyRelativePose(cfg)
    model.load_state_dict(syn.mickey_state_dict(cfg, seed=0))
    model = model.to(dev)
    resize = (196, 182)
    recs = ME.dataset_records(str(tmp_path), "val", resize)
    assert len(recs) == 6   # batches of 4 + 2: the first spans both scenes (K = 2)
    zips, decoded = [], []
    for share in (False, True):
        model.reseed(7, 0)
        out = tmp_path / ("kf" if share else "std") / "submission.zip"
        stats = {}
        ME.predict_to_zip(model, recs, batch_size=4, resize=resize, output_zip=out, device=dev, share_keyframes=share, stats=stats)
        with zipfile.ZipFile(out) as z:   # (the archive's own bytes carry the write time of each member)
            zips.append({n: z.read(n) for n in z.namelist()})
        decoded.append(stats["frames_decoded"])
    assert sorted(zips[0]) == ["pose_s00460.txt", "pose_s00461.txt"] and zips[0] == zips[1]
    assert decoded == [12, 6 + 3]   # 2 x 6 frames; shared: 6 queries + keyframes 2 (first batch) + 1 (second)
