"""-m gpu: the call sequence of the reference's inference callers (demo_inference.py:79-138, submission.py:32-68 -- restated
call for call in tests/helpers/caller_sequence.py, because the GPU box has no reference tree) driving the REAL HIP forward:
build_model(cfg with attribute + key access, Lightning-style checkpoint without DINOv2 keys + the hub file beside it) ->
.cuda() inside build_model -> model(data, return_inliers=True) with float64 intrinsics -> the keys the callers read back."""
import os
import sys
import zipfile

import numpy as np
import pytest
import torch
import yaml

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))


def rel(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


@pytest.fixture()
def workdir(tmp_path, monkeypatch):
    """A MicKey-style checkpoint (state_dict WITHOUT the frozen DINOv2 weights, reference model.py:291-298) + the hub file,
    tiny ViT so the CPU oracle beside it takes seconds; the config as a YAML on disk merged through cfg.merge_from_file."""
    from mickey_amd import synthetic as syn
    from mickey_amd.config import default_cfg
    cfg = default_cfg()
    cfg["MICKEY"]["DINOV2"]["CHANNEL_DIM"] = 128
    sd = syn.mickey_state_dict(cfg, seed=0, arch="vit_tiny_test")
    torch.save({"state_dict": {k: v for k, v in sd.items() if "dinov2" not in k}, "epoch": 3, "pytorch-lightning_version": "2.0"},
               tmp_path / "mickey.ckpt")
    torch.save({k[len(syn.DINO_PREFIX):]: v for k, v in sd.items() if k.startswith(syn.DINO_PREFIX)}, tmp_path / "dinov2.pth")
    monkeypatch.setenv("MICKEY_DINOV2_WEIGHTS", str(tmp_path / "dinov2.pth"))
    return tmp_path, sd


def _write_yaml(tmp_path, float16):
    # only what the caller's YAML carries: the reference's groups (no AMD group -> every AMD default, i.e. ENCODER_DTYPE auto
    # follows MICKEY.DINOV2.FLOAT16 exactly as the reference's switch does)
    y = {"MODEL": "MicKey", "MICKEY": {"DINOV2": {"CHANNEL_DIM": 128, "FLOAT16": bool(float16), "DOWN_FACTOR": 14}}}
    p = tmp_path / ("config_%d.yaml" % int(float16))
    yaml.safe_dump(y, open(p, "w"))
    return str(p)


@pytest.mark.parametrize("float16", [False, True])
def test_demo_sequence_on_the_hip_forward(workdir, float16):
    import caller_sequence as CS
    from lib.models.builder import build_model                   # the drop-in's import path, as demo_inference.py:3
    from mickey_amd.config import default_cfg
    from oracle import mickey_oracle as O
    tmp_path, sd = workdir
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    g = torch.Generator().manual_seed(5)
    im0, im1 = torch.rand((1, 3, 190, 200), generator=g), torch.rand((1, 3, 190, 200), generator=g)   # not multiples of 14
    K0 = np.array([[274.85, 0, 100.3], [0, 274.85, 95.9], [0, 0, 1.0]])                              # float64, as np.loadtxt gives
    K1 = np.array([[274.53, 0, 100.4], [0, 274.53, 95.9], [0, 0, 1.0]])
    cfg = default_cfg()
    model, data, read = CS.demo_sequence(build_model, cfg, _write_yaml(tmp_path, float16), str(tmp_path / "mickey.ckpt"),
                                         im0, im1, K0, K1, return_inliers=True)
    assert next(model.parameters()).device.type == "cuda" and not model.training
    assert model.lp_dtype == (torch.float16 if float16 else torch.float32)       # followed the reference's own switch
    assert data["K_color0"].dtype == torch.float64                               # the caller's tensor is left as it came
    assert read["depth0"].shape == (1, 13, 14) and read["scr0"].shape == (1, 182) and read["n_matches"] == 2048
    assert read["R"].shape == (1, 3, 3) and read["t"].shape == (1, 1, 3) and read["inliers"].shape == (1, 1)
    assert read["inliers_list"].dim() == 2 and read["inliers_list"].shape[1] in (5, 7)
    assert all(t.is_cuda for t in (read["R"], read["t"], read["depth0"], read["scr0"]))
    det = torch.linalg.det(read["R"].double().cpu())
    assert torch.isfinite(read["R"]).all() and (float((det - 1).abs().max()) < 1e-4 or float(read["R"].abs().sum()) == 0.0)
    # what the HIP forward left in `data` == the oracle on the same checkpoint and inputs
    ocfg = default_cfg()
    ocfg["MICKEY"]["DINOV2"]["CHANNEL_DIM"] = 128
    odata = {"image0": im0, "image1": im1}
    with torch.no_grad():
        odata.update(O.compute_correspondences(sd, ocfg, odata, heads=2))
    # FLOAT16: False -> the exact parity mode, 1e-4.  FLOAT16: True -> fp16 operands: only a sanity bound here (this tiny ViT has
    # no noise-floor fixture; the 16-bit bounds proper are asserted on ViT-L in tests/test_model_gpu.py)
    tol = 1e-2 if float16 else 1e-4
    for k in ("kps0", "depth_kp0", "scr0", "dsc0", "dsc1", "scores", "final_scores"):
        assert rel(data[k], odata[k]) < tol, (k, rel(data[k], odata[k]))


def test_submission_sequence_on_the_hip_forward(workdir):
    import caller_sequence as CS
    from lib.models.builder import build_model
    from mickey_amd.config import default_cfg
    from mickey_amd import submission_io as sio
    tmp_path, sd = workdir
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    cfg = default_cfg()
    cfg.merge_from_file(_write_yaml(tmp_path, True))
    model = build_model(cfg, checkpoint=str(tmp_path / "mickey.ckpt"))
    g = torch.Generator().manual_seed(3)
    K = torch.from_numpy(np.array([[300.0, 0, 98.0], [0, 300.0, 91.0], [0, 0, 1.0]]))   # float64
    loader = []
    for b in range(2):
        B = 3 - b                                                                        # a ragged last batch
        loader.append({"image0": torch.rand((B, 3, 182, 196), generator=g), "image1": torch.rand((B, 3, 182, 196), generator=g),
                       "K_color0": K.repeat(B, 1, 1), "K_color1": K.repeat(B, 1, 1), "scene_id": ["s%05d" % (i % 2) for i in range(B)],
                       "pair_names": (["seq0/frame_00000.jpg"] * B, ["seq1/frame_%05d.jpg" % (10 * b + i) for i in range(B)]),
                       "T_0to1": torch.eye(4).repeat(B, 1, 1)})
    zpath = str(tmp_path / "submission.zip")
    res = CS.submission_sequence(model, loader, sio.mat2quat, zpath)
    assert sorted(res) == ["s00000", "s00001"] and sum(len(v) for v in res.values()) == 5
    assert loader[0]["T_0to1"].is_cuda and loader[0]["scene_id"] == ["s00000", "s00001", "s00000"]    # pass-through keys
    with zipfile.ZipFile(zpath) as z:
        assert sorted(z.namelist()) == ["pose_s00000.txt", "pose_s00001.txt"]
        for n in z.namelist():
            poses = sio.load_poses(z.read(n).decode().splitlines())     # the evaluator's reader (benchmark/utils.py:18-78) restated
            assert len(poses) == len(res[n[5:-4]])
    # the drop-in's own sink writes the same lines from the same forward
    model.reseed()
    res2 = sio.predict([{k: (v.clone() if torch.is_tensor(v) else v) for k, v in d.items()} for d in loader], model,
                       to_device=CS.data_to_model_device)
    model.reseed()
    res3 = CS.submission_sequence(model, loader, sio.mat2quat, str(tmp_path / "again.zip"))
    for scene in res3:
        assert [str(p) for p in res2[scene]] == res3[scene]
