"""Write tests/golden/pose_metrics.npz from THE REFERENCE's own validation metrics (CPU only).

    python tools/make_golden_pose_metrics.py    (needs the reference checkout: MICKEY_REFERENCE_ROOT, oracle/ref_shim.py)

Calls the reference's pose_error_torch and vcre_torch (lib/utils/metrics.py:12-53, 83-125) in fp32, as the trainer does
(lib/models/MicKey/model.py:76-85), on seeded poses, and its precision_recall (lib/benchmarks/utils.py:138-188) on a few record sets.

Poses (16): ground truth a rotation of up to 40 degrees about a random axis with a translation of 0.3 .. 1.5 m; the estimate is
Rgt Rres with a residual rotation of 2 .. 178 degrees (half of them about an axis near the optical one, the others of at most
40 degrees about any axis) and tgt + a step of 0.02 .. 0.6 m.  A pose is kept when every eye-grid point lies at least 0.3 m in front
of the camera after the residual transform and the angle between t and tgt lies in [2, 178] degrees, so that every acos is
well conditioned.  Intrinsics: Map-free-like (f 580 .. 610, principal point near (270, 360)).

Record sets for precision_recall (confidences fp32, tp bool, failures): all tied | all distinct | one tie group of N - 1 | heavy random
ties with failures 0 and 2 | tp all false | tp all true | one record.

Stored: the inputs (fp32), the reference's outputs (fp32, as it returns them) and, per set, precision_recall's three outputs.  Data
only, a few KB.  tests/test_train_eval_cpu.py checks the in-repo fp64 restatement (tests/helpers/metric_refs.py) against the file.
"""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_shim  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "pose_metrics.npz")
SEED = 20261021
NPOSES = 16


def _rot(axis, deg):
    axis = axis / np.linalg.norm(axis)
    a = np.radians(deg)
    Kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(a) * Kx + (1 - np.cos(a)) * (Kx @ Kx)


def poses(rng, grid):
    R, t, T, K = [], [], [], []
    while len(R) < NPOSES:
        Rgt = _rot(rng.standard_normal(3), rng.uniform(0, 40))
        tgt = rng.standard_normal(3)
        tgt *= rng.uniform(0.3, 1.5) / np.linalg.norm(tgt)
        if len(R) % 2 == 0:
            Rres = _rot(np.array([0, 0, 1.0]) + 0.1 * rng.standard_normal(3), rng.uniform(2, 178))
        else:
            Rres = _rot(rng.standard_normal(3), rng.uniform(2, 40))
        Re = Rgt @ Rres
        step = rng.standard_normal(3)
        te = tgt + step * rng.uniform(0.02, 0.6) / np.linalg.norm(step)
        moved = (Rgt.T @ (Re @ grid.T + (te - tgt)[:, None])).T
        ang = np.degrees(np.arccos(np.clip(te @ tgt / (np.linalg.norm(te) * np.linalg.norm(tgt)), -1, 1)))
        if moved[:, 2].min() < 0.3 or not 2.0 <= ang <= 178.0:
            continue
        Tm = np.eye(4)
        Tm[:3, :3], Tm[:3, 3] = Rgt, tgt
        f = rng.uniform(580, 610)
        R.append(Re), t.append(te[None]), T.append(Tm)
        K.append(np.array([[f, 0, 270 + rng.uniform(-5, 5)], [0, f * rng.uniform(0.99, 1.01), 360 + rng.uniform(-5, 5)], [0, 0, 1]]))
    return [np.stack(v).astype(np.float32) for v in (R, t, T, K)]


def record_sets(rng):
    """[(confidences fp32 [N], tp bool [N], failures)]"""
    n = 37
    tp = rng.random(n) < 0.6
    distinct = rng.permutation(n).astype(np.float32) * 1.5 + 3.0
    group = np.full(n, 11.0, np.float32)
    group[5] = 40.0
    heavy = rng.integers(0, 6, 200).astype(np.float32) * 7.25
    tph = rng.random(200) < 0.5
    return [(np.full(n, 17.5, np.float32), tp, 0), (distinct, tp, 0), (group, tp, 0), (heavy, tph, 0), (heavy, tph, 2),
            (distinct, np.zeros(n, bool), 2), (heavy, np.ones(200, bool), 0), (np.array([3.0], np.float32), np.array([True]), 0)]


def generate():
    """{name: array}: everything the fixture holds, from the reference's own functions."""
    ref_shim.install()
    added = []
    if "transforms3d" not in sys.modules:   # imported by lib/benchmarks/* for functions this path never calls
        t3, q = types.ModuleType("transforms3d"), types.ModuleType("transforms3d.quaternions")
        q.quat2mat = q.mat2quat = q.qinverse = q.rotate_vector = q.qmult = None
        t3.quaternions = q
        sys.modules["transforms3d"], sys.modules["transforms3d.quaternions"] = t3, q
        added = ["transforms3d", "transforms3d.quaternions"]
    try:
        from lib.benchmarks.reprojection import get_grid_multipleheight
        from lib.benchmarks.utils import precision_recall
        from lib.utils.metrics import pose_error_torch, vcre_torch
        rng = np.random.default_rng(SEED)
        grid = get_grid_multipleheight()[:, :3]
        R, t, T, K = poses(rng, grid)
        out = {"R": R, "t": t, "T_0to1": T, "Kori_color0": K, "eye_grid": grid.astype(np.float32)}
        args = [torch.from_numpy(v) for v in (R, t, T)]
        for k, v in pose_error_torch(*args, reduce=None).items():
            out["ref_" + k] = v.numpy()
        out["ref_repr_err"] = vcre_torch(*args, torch.from_numpy(K), reduce=None)["repr_err"].numpy()
        for s, (conf, tp, failures) in enumerate(record_sets(rng)):
            prec, rec, ap = precision_recall(inliers=conf, tp=tp, failures=failures)
            out.update({"set%d_conf" % s: conf, "set%d_tp" % s: tp, "set%d_failures" % s: np.int64(failures),
                        "set%d_prec" % s: np.asarray(prec), "set%d_rec" % s: np.asarray(rec), "set%d_ap" % s: np.float64(ap)})
        out["num_sets"] = np.int64(s + 1)
        return out
    finally:
        for name in added:
            del sys.modules[name]
        ref_shim.uninstall()


def main():
    out = generate()
    np.savez_compressed(OUT, **out)
    for k in sorted(out):
        print("  %-22s %-8s %s" % (k, out[k].dtype, out[k].shape))
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))
    assert os.path.getsize(OUT) < 100 << 10


if __name__ == "__main__":
    main()
