"""Map-free evaluation harness, host side: it takes paths and skips cleanly; its scene parsing yields the reference
dataset's pairs, names and intrinsics (compared with what lib/datasets/mapfree.py yields, stored in tests/golden)."""
import json
import os

import numpy as np

from mickey_amd import mapfree_eval as ME
from tests.helpers import tiny_mapfree


def test_skips_cleanly_without_dataset_or_checkpoint(tmp_path, capsys):
    assert ME.main(["--dataset_path", str(tmp_path / "nowhere"), "--checkpoint", str(tmp_path / "none.ckpt")]) == 0
    out = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert out["skipped"] and len(out["reasons"]) == 2
    tiny_mapfree.make(str(tmp_path / "data"), "val", queries=3)
    assert ME.main(["--dataset_path", str(tmp_path / "data"), "--split", "val", "--checkpoint", ""]) == 0
    out = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert out["skipped"] and out["reasons"] == ["checkpoint  not found"]
    os.makedirs(tmp_path / "data" / "val" / "broken_scene")
    assert any("intrinsics.txt" in w for w in ME.missing_inputs(str(tmp_path / "data"), "val", __file__))


def test_evaluator_leg_reports_instead_of_failing(tmp_path):
    metrics, msg = ME.run_evaluator(None, tmp_path / "s.zip", tmp_path, "val")
    assert metrics is None and "evaluator not found" in msg
    metrics, msg = ME.run_evaluator(str(tmp_path), tmp_path / "s.zip", tmp_path, "val")
    assert metrics is None and "evaluator not found" in msg
    (tmp_path / "benchmark").mkdir()
    (tmp_path / "benchmark" / "mapfree.py").write_text("raise SystemExit(3)\n")
    metrics, msg = ME.run_evaluator(str(tmp_path), tmp_path / "s.zip", tmp_path, "val")
    assert metrics is None and "rc 3" in msg
    (tmp_path / "benchmark" / "mapfree.py").write_text("import json; print(json.dumps({'AUC @ VCRE < 90px': 0.5}))\n")
    metrics, msg = ME.run_evaluator(str(tmp_path), tmp_path / "s.zip", tmp_path, "val")
    assert msg == "ok" and metrics == {"AUC @ VCRE < 90px": 0.5}
    assert ME.run_evaluator(str(tmp_path), tmp_path / "s.zip", tmp_path, "test")[0] is None


def test_records_follow_the_dataset_layout(tmp_path):
    split_root = tiny_mapfree.make(str(tmp_path), "val", scenes=("s1", "s0"), queries=11, size=(126, 168))
    recs = ME.dataset_records(str(tmp_path), "val", (126, 168))
    # scenes sorted; key frame against every 5th query frame: 0, 5, 10
    assert [r["scene_id"] for r in recs] == ["s0"] * 3 + ["s1"] * 3
    assert [r["pair_names"][1] for r in recs[:3]] == ["seq1/frame_00000.jpg", "seq1/frame_00005.jpg", "seq1/frame_00010.jpg"]
    assert all(r["pair_names"][0] == "seq0/frame_00000.jpg" and os.path.isfile(r["image0"]) and os.path.isfile(r["image1"]) for r in recs)
    assert recs[0]["K_color0"].dtype == np.float32 and recs[0]["K_color0"].shape == (3, 3)


def test_records_match_the_reference_dataset(tmp_path, golden):
    """Against what the reference's MapFreeScene yields over the same tiny dataset (tests/golden/mapfree_records.npz, written
    by oracle/make_golden.py), at the stored size and at a larger model size."""
    import torch
    from mickey_amd.input_pipeline import correct_intrinsic_scale, decode_rgb
    ref = golden("mapfree_records")
    W, H = (int(x) for x in ref["size"])   # model size == stored size: the reference's image tensors are the decoded bytes / 255
    W2, H2 = (int(x) for x in ref["size2"])
    tiny_mapfree.make(str(tmp_path), "test", queries=int(ref["queries"]), size=(W, H))
    recs = ME.dataset_records(str(tmp_path), "test", (W, H))
    assert len(recs) == len(ref["scene_id"]) == 2 * 3
    for i, a in enumerate(recs):
        assert a["scene_id"] == ref["scene_id"][i] and list(a["pair_names"]) == list(ref["pair_names"][i])
        assert np.array_equal(a["Kori_color0"], ref["Kori_color0"][i])
        img0 = decode_rgb(a["image0"]).astype(np.float64) / 255.0
        assert list(img0.transpose(2, 0, 1).shape) == list(ref["image0_shape"][i])
        assert abs(float(np.float32(img0).astype(np.float64).sum()) - float(ref["image0_sum"][i])) < 1e-2
    # intrinsics at a model resolution different from the stored one: the feeder's rescale == the reference's
    for i, a in enumerate(recs):
        K = correct_intrinsic_scale(torch.from_numpy(a["K_color0"]), W2 / W, H2 / H).numpy()
        assert np.allclose(K, ref["K_color0_size2"][i], rtol=0, atol=1e-4)
        Ks, _, size = ME.read_intrinsics(os.path.dirname(os.path.dirname(a["image0"])), (W2, H2))
        assert np.allclose(Ks[a["pair_names"][0]], ref["K_color0_size2"][i], rtol=0, atol=1e-4) and size == (W, H)
