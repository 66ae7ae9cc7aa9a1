"""-m gpu: the heads' linear attention with its projections inside (mk_linattn_kv_fused, mk_linattn_apply_fused) against the
launches it replaces -- mk_gemm_grouped (fp32 q | k | v) -> mk_linattn_kv -> mk_linattn_apply -> mk_gemm_ln128 -- on the same
inputs.  The fused kernels compute the same accumulators and sum everything in the same order: every comparison is torch.equal.
Shapes: L = 35 (one ragged chunk), L = 99 = 64 + 35 (a ragged second chunk whose last 16-row block holds 3 rows), L = 64 exactly;
and, sized from the device's CU count, enough images that a workgroup WALKS: `chunk += gridDim.x` of the kv kernel and
`tile += step` of the apply kernel take further trips, each with its prefetch of the next chunk or tile."""
import copy
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

C = 128
SHAPES = [(4, 3, 5, 7), (4, 2, 9, 11), (1, 1, 8, 8)]   # G, nimg, gh, gw
DTYPES = [torch.float16, torch.bfloat16]
SENTINEL = 7.0


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


_CASES = {}


def _case(G, nimg, gh, gw, dtype, keep=True):
    """Inputs and the unfused results of one case, computed once and shared (nothing below writes into them).  keep = False: not
    kept for later tests (the walking cases hold hundreds of MB)."""
    key = (G, nimg, gh, gw, dtype)
    if key in _CASES:
        return _CASES[key]
    from mickey_amd import ops
    dev = _dev()
    L = gh * gw
    M = nimg * L
    gen = torch.Generator(device="cuda").manual_seed(1000 * G + 100 * nimg + L)
    rn = lambda *shape, s=1.0: torch.randn(shape, device=dev, generator=gen) * s  # noqa: E731
    # q, k, v = randn * ~2: both branches of phi (x > 0 and x <= 0) are taken everywhere
    cat = rn(G, M, 2 * C).to(dtype)                        # lda = 2C: x = cat[:, :, :C]
    cat[:, :, C:] = SENTINEL
    qkv_w = rn(G, 3 * C, C, s=2.0 / math.sqrt(C)).to(dtype)
    merge_w = rn(G, C, C, s=1.5 / math.sqrt(C)).to(dtype)
    lw, lb = 1.0 + 0.3 * rn(G, C), 0.2 * rn(G, C)
    qkv = torch.empty((G, M, 3 * C), device=dev, dtype=torch.float32)
    ops.gemm_grouped(cat, qkv_w, None, qkv, G, M, 3 * C, C, 2 * C, C, 3 * C, M * 2 * C, 3 * C * C, 0, M * 3 * C)
    assert float((qkv[:, :, :2 * C] > 0).float().mean()) > 0.3 and float((qkv[:, :, :2 * C] < 0).float().mean()) > 0.3
    kv = torch.full((G * nimg * (C // 16), 272), float("nan"), device=dev)
    work = torch.full((ops.linattn_work_floats(G, nimg, L, C),), float("nan"), device=dev)
    ops.linattn_kv(qkv, kv, work, G, nimg, L, C)
    msg = torch.full((G, M, C), SENTINEL, device=dev, dtype=dtype)
    ops.linattn_apply(qkv, kv, msg, C, G, nimg, L, C)
    out = cat.clone()
    ops.gemm_ln128(msg, merge_w, lw, lb, 1e-5, out[:, :, C:], G, M, C, ldo=2 * C)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(kv).all()) and bool(torch.isfinite(work).all())
    c = dict(cat=cat, qkv_w=qkv_w, merge_w=merge_w, lw=lw, lb=lb, kv=kv, work=work, msg=msg, out=out, L=L, M=M)
    if keep:
        _CASES[key] = c
    return c


def _kv_fused(c, G, nimg, cat=None):
    from mickey_amd import ops
    kv = torch.full_like(c["kv"][:G * nimg * (C // 16)], float("nan"))
    work = torch.full((ops.linattn_work_floats(G, nimg, c["L"], C),), float("nan"), device=kv.device)
    ops.linattn_kv_fused(c["cat"] if cat is None else cat, c["qkv_w"], kv, work, G, nimg, c["L"], C)
    return kv, work


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("G,nimg,gh,gw", SHAPES)
def test_kv_fused_equals_gemm_then_linattn_kv(G, nimg, gh, gw, dtype):
    """kv and the per-chunk partials, pre-filled with NaN: every element is written, with the bits of the two launches."""
    c = _case(G, nimg, gh, gw, dtype)
    kv, work = _kv_fused(c, G, nimg)
    assert torch.equal(work, c["work"])
    assert torch.equal(kv, c["kv"])


def _padded(c, G):
    """cat with two sentinel rows in front of and behind every group's M rows: a write outside [0, M) shows."""
    M = c["M"]
    buf = torch.full((G, M + 4, 2 * C), SENTINEL, device=c["cat"].device, dtype=c["cat"].dtype)
    buf[:, 2:M + 2] = c["cat"]
    return buf, buf[:, 2:M + 2]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("G,nimg,gh,gw", SHAPES)
def test_apply_fused_equals_the_four_launches(G, nimg, gh, gw, dtype):
    """cat[:, :, C:] after the one launch = gemm_grouped -> linattn_apply -> gemm_ln128; the first column half (the input) and the
    rows around the group's M rows keep their values."""
    from mickey_amd import ops
    c = _case(G, nimg, gh, gw, dtype)
    buf, cat = _padded(c, G)
    ops.linattn_apply_fused(cat, c["qkv_w"], c["kv"], cat[:, :, C:], G, nimg, c["L"], C, merge_w=c["merge_w"], ln_w=c["lw"], ln_b=c["lb"])
    assert torch.equal(cat[:, :, C:], c["out"][:, :, C:])
    assert torch.equal(cat[:, :, :C], c["cat"][:, :, :C])
    assert bool((buf[:, :2] == SENTINEL).all()) and bool((buf[:, -2:] == SENTINEL).all())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("G,nimg,gh,gw", SHAPES)
def test_apply_fused_without_merge_writes_msg(G, nimg, gh, gw, dtype):
    """merge_w = None: the launch stops at msg (what mk_linattn_apply writes), here into the second column half."""
    from mickey_amd import ops
    c = _case(G, nimg, gh, gw, dtype)
    buf, cat = _padded(c, G)
    ops.linattn_apply_fused(cat, c["qkv_w"], c["kv"], cat[:, :, C:], G, nimg, c["L"], C)
    assert torch.equal(cat[:, :, C:], c["msg"])
    assert torch.equal(cat[:, :, :C], c["cat"][:, :, :C])
    assert bool((buf[:, :2] == SENTINEL).all()) and bool((buf[:, -2:] == SENTINEL).all())


@pytest.mark.parametrize("dtype", DTYPES)
def test_fused_kernels_are_batch_invariant(dtype):
    """Image i of the nimg = 3 case run alone gives the bits it gives inside the batch, for both kernels."""
    from mickey_amd import ops
    G, nimg, gh, gw = SHAPES[0]
    c = _case(G, nimg, gh, gw, dtype)
    L, H = c["L"], C // 16
    kv3, work3 = _kv_fused(c, G, nimg)
    nchunk = work3.numel() // (G * nimg * H * 272)
    for i in range(nimg):
        one = c["cat"][:, i * L:(i + 1) * L].contiguous()
        kv1, work1 = _kv_fused(c, G, 1, cat=one)
        assert torch.equal(kv1.view(G, H, 272), kv3.view(G, nimg, H, 272)[:, i])
        assert torch.equal(work1.view(G, H * nchunk * 272), work3.view(G, nimg, H * nchunk * 272)[:, i])
        for merge in (True, False):
            kw = dict(merge_w=c["merge_w"], ln_w=c["lw"], ln_b=c["lb"]) if merge else {}
            cat1 = one.clone()
            ops.linattn_apply_fused(cat1, c["qkv_w"], kv1, cat1[:, :, C:], G, 1, L, C, **kw)
            ref = (c["out"][:, :, C:] if merge else c["msg"])[:, i * L:(i + 1) * L]
            assert torch.equal(cat1[:, :, C:], ref), (i, merge)


# ---- the walk loops: shapes from the CU count, the trip counts asserted from the launch rules of mk_linattn.hip ----------------------
def _cus():
    _dev()
    return torch.cuda.get_device_properties(0).multi_processor_count


def _kv_trips(gi, L):
    """chunks each workgroup of an image walks: per_img = min(ceil(8 CUs / gi), nchunk) workgroups, chunk += per_img"""
    nchunk = (L + 63) // 64
    per_img = min((8 * _cus() + gi - 1) // gi, nchunk)
    return [len(range(b, nchunk, per_img)) for b in range(per_img)]


def _apply_trips(gi, L):
    """16-token tiles each (workgroup, wave) of an image walks: per_img = min(ceil(CUs / gi), ceil(L / 128)), tile += 8 per_img"""
    ntile = (L + 15) // 16
    per_img = min((_cus() + gi - 1) // gi, (L + 127) // 128)
    return [[len(range(b * 8 + wv, ntile, per_img * 8)) for wv in range(8)] for b in range(per_img)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("per_cu", [8, 4])
def test_kv_fused_walks_its_chunks(per_cu, dtype):
    """L = 131 = 64 + 64 + 3.  gi = 8 CUs: one workgroup per image walks all 3 chunks, the last ragged (both branches of the prefetch:
    the chunk's next token set, the next chunk's first).  gi = 4 CUs: two workgroups per image walk 2 chunks and 1 chunk."""
    G, nimg, L = 1, per_cu * _cus(), 131
    assert _kv_trips(G * nimg, L) == ([3] if per_cu == 8 else [2, 1])
    c = _case(G, nimg, 1, L, dtype, keep=False)
    kv, work = _kv_fused(c, G, nimg)
    assert torch.equal(work, c["work"])
    assert torch.equal(kv, c["kv"])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("halves,L", [(2, 131), (1, 300)])
def test_apply_fused_walks_its_tiles(halves, L, dtype):
    """gi = CUs, L = 131: one workgroup per image, 9 sixteen-token tiles, wave 0 takes two.  gi = CUs / 2, L = 300: two workgroups
    per image, 19 tiles, waves 0 .. 2 of the first take two.  With and without merge_w."""
    G = 2
    nimg = halves * _cus() // 4
    assert G * nimg == halves * _cus() // 2
    trips = _apply_trips(G * nimg, L)
    if halves == 2:
        assert trips == [[2, 1, 1, 1, 1, 1, 1, 1]]
    else:
        assert trips == [[2, 2, 2, 1, 1, 1, 1, 1], [1] * 8] and (L + 15) // 16 == 19
    from mickey_amd import ops
    c = _case(G, nimg, 1, L, dtype, keep=False)
    for merge in (True, False):
        buf, cat = _padded(c, G)
        kw = dict(merge_w=c["merge_w"], ln_w=c["lw"], ln_b=c["lb"]) if merge else {}
        ops.linattn_apply_fused(cat, c["qkv_w"], c["kv"], cat[:, :, C:], G, nimg, L, C, **kw)
        assert torch.equal(cat[:, :, C:], c["out"][:, :, C:] if merge else c["msg"]), merge
        assert torch.equal(cat[:, :, :C], c["cat"][:, :, :C])
        assert bool((buf[:, :2] == SENTINEL).all()) and bool((buf[:, -2:] == SENTINEL).all())


def test_heads_forward_fused_equals_unfused(cfg):
    """pipeline.heads_forward on a 5 x 7 grid, 2 images, synthetic weights: AMD.LINATTN_FUSED on and off give the same scr / kps /
    depth / dsc bit for bit (fp16 heads, the default).  A small encoder arch keeps the weights quick to make: the heads only see D."""
    from mickey_amd import ops, pipeline, synthetic as syn, weights
    dev = _dev()
    nimg, gh, gw = 2, 5, 7
    c = copy.deepcopy(cfg)
    c["MICKEY"]["DINOV2"]["CHANNEL_DIM"] = syn.VIT_ARCH["vit_tiny_test"][0]
    sd = syn.mickey_state_dict(c, seed=0, arch="vit_tiny_test")
    W = weights.prepare(sd, c, dev, torch.float16, heads_dtype=torch.float16)
    feat = torch.zeros((ops.bordered_rows(nimg, gh, gw), W.D), device=dev, dtype=torch.float16)
    gen = torch.Generator(device="cuda").manual_seed(5)
    feat[ops.bordered_index(nimg, gh, gw, dev)] = torch.randn((nimg * gh * gw, W.D), device=dev, generator=gen).half()
    outs = {}
    for fused in (True, False):
        c["AMD"]["LINATTN_FUSED"] = fused
        ws = pipeline.Workspace()
        outs[fused] = [t.clone() for t in pipeline.heads_forward(W, ws, feat, nimg, gh, gw, c)]
        assert (("att_qkv", (4, nimg * gh * gw, 3 * C), torch.float32) in ws.bufs) == (not fused)
    for a, b, name in zip(outs[True], outs[False], ("scr", "kps", "depth", "dsc")):
        assert bool(torch.isfinite(a).all()), name
        assert torch.equal(a, b), name
