"""fp64 restatements of the validation metrics for the tests of mickey_amd.train_eval: the per-pair pose / VCRE formulas
(reference lib/utils/metrics.py:12-53, 83-125) and the epoch summary (lib/models/MicKey/model.py:205-280 with the average precision
of lib/benchmarks/utils.py:138-188 in its all-pairs form).  numpy only; NaNs propagate as in torch (np.clip / minimum / maximum)."""
import numpy as np

COLUMNS = ("t_err_ang", "t_err_scale", "t_err_scale_sym", "t_err_euc", "R_err", "repr_err")


def eye_grid():
    """The 196 eye-grid points (lib/benchmarks/reprojection.py:32-56) as the kernels form them: fp32 values, point
    p = (j * 7 + i) * 7 + k at ((i - 3) 0.3, (j - 1.5) 0.3, k 0.3 + 1.8).  -> float64 [196, 3]"""
    f = np.float32
    p = np.arange(196)
    k, i, j = p % 7, (p // 7) % 7, p // 49
    x = (i.astype(f) - f(3.0)) * f(0.3)
    y = (j.astype(f) - f(1.5)) * f(0.3)
    z = k.astype(f) * f(0.3) + f(1.8)     # (the same fp32 value with and without a fused multiply-add, for all seven k)
    return np.stack([x, y, z], 1).astype(np.float64)


def _proj(K, P):
    q = np.einsum("bij,bpj->bpi", K, P)
    return q[..., :2] / (q[..., 2:3] + 1e-16)


def pose_metrics_ref(R, t, T, K, W=540.0, H=720.0):
    """R [B, 3, 3], t [B, 1, 3], T [B, 4, 4], K [B, 3, 3] -> float64 [B, 6] in the order of COLUMNS, every step in fp64."""
    R, t, T, K = (np.asarray(v, dtype=np.float64) for v in (R, t, T, K))
    t = t.reshape(-1, 3)
    Rg, tg = T[:, :3, :3], T[:, :3, 3]
    with np.errstate(all="ignore"):
        st, sg = np.sqrt((t * t).sum(-1)), np.sqrt((tg * tg).sum(-1))
        a = np.degrees(np.arccos(np.clip((t * tg).sum(-1) / (st * sg + 1e-9), -1.0, 1.0)))
        t_ang = np.minimum(a, 180.0 - a)
        scale = st / sg
        sym = np.maximum(st / sg, sg / st)
        euc = np.sqrt(((t - tg) ** 2).sum(-1))
        r_err = np.degrees(np.arccos(np.clip(((R * Rg).sum((-1, -2)) - 1.0) / 2.0, -1.0, 1.0)))
        e = np.broadcast_to(eye_grid(), (R.shape[0], 196, 3))
        uv_gt = _proj(K, e)
        moved = np.einsum("bij,bpj->bpi", R, e) + (t - tg)[:, None, :]
        uv = _proj(K, np.einsum("bji,bpj->bpi", Rg, moved))        # Rgt^T (R e + t - tgt)
        hi = np.array([W, H], dtype=np.float64)
        d = np.clip(uv_gt, 0.0, hi) - np.clip(uv, 0.0, hi)
        vcre = np.sqrt((d * d).sum(-1) + 1e-6).mean(-1)
    return np.stack([t_ang, scale, sym, euc, r_err, vcre], 1)


def rank_keys(conf):
    """Confidences as the summary ranks them: a value that is not finite counts as -inf."""
    c = np.asarray(conf, dtype=np.float64).copy()
    c[~np.isfinite(c)] = -np.inf
    return c


def average_precision_ref(conf, tp, failures=0):
    """AP = 1 / (N + failures) * sum_i cumTP_i / cumN_i, cumN_i = #{j: c_j >= c_i}, cumTP_i = #{j: c_j >= c_i and tp_j}."""
    c = rank_keys(conf)
    tp = np.asarray(tp).astype(bool).reshape(-1)
    ge = c[None, :] >= c[:, None]                      # [i, j]
    cum_n = ge.sum(1)
    cum_tp = (ge & tp[None, :]).sum(1)
    return float((cum_tp.astype(np.float64) / cum_n.astype(np.float64)).sum() / (len(c) + failures))


def accepted(records, thresholds):
    """The three acceptance tests (strict, fp32 values against the thresholds) -> bool [3, N]"""
    r = np.asarray(records, dtype=np.float32)
    th = [np.float32(v) for v in thresholds]
    return np.stack([(r[:, 3] < th[0]) & (r[:, 4] < th[1]), (r[:, 3] < th[2]) & (r[:, 4] < th[3]), r[:, 5] < th[4]])


def summary_ref(records, failures=0, thresholds=(0.25, 5, 0.5, 10, 90), losses=None):
    """The 16 values of mk_pose_summary's `out` in fp64 from records fp32 [N, 8] (and losses fp32 [S, 3])."""
    r = np.asarray(records, dtype=np.float32)
    n = r.shape[0]
    acc = accepted(r, thresholds)
    out = np.zeros(16)
    out[0] = n
    out[1] = (~np.isfinite(r[:, 6])).sum()
    with np.errstate(all="ignore"):
        out[2:6] = r[:, [0, 3, 4, 5]].astype(np.float64).sum(0) / n
    for k in range(3):
        out[6 + 2 * k] = acc[k].sum() / (n + failures)
        out[7 + 2 * k] = average_precision_ref(r[:, 6], acc[k], failures)
    if losses is not None:
        out[12:15] = np.asarray(losses, dtype=np.float64).mean(0)
    return out
