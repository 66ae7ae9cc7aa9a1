"""Input pipeline in front of the hot path: image files -> device batches at the rate the GPU
consumes them.

The reference feeds the model through a torch DataLoader whose workers run cv2 decode + cv2.resize + float conversion
on host cores and ship fp32 CHW tensors (9.3 MB per pair) to the GPU (reference lib/datasets/utils.py:61-78,
lib/datasets/mapfree.py:108-160, submission.py:76-86: 8 workers).  At 250+ pairs/s per GPU that is the wall.  Here:

  * host cores only DECODE (PIL, which releases the GIL: a thread pool scales) straight into PINNED uint8 staging slots
    -- 2.3 MB per pair instead of 9.3 MB cross PCIe;
  * a ring of such slots is copied to the device on a side stream (`non_blocking`), overlapping the previous batch's
    forward; an event per slot orders copy -> preprocess -> reuse;
  * resize + /255 + HWC->CHW run on the GPU (csrc/mk_input.hip), intrinsics are rescaled as the reference does
    (`correct_intrinsic_scale`, utils.py:86-99).

`PairFeeder` yields `data` dicts with the keys the model reads (image0, image1, K_color0, K_color1) plus pass-through
metadata (scene_id, pair_names), i.e. what MapFreeScene.__getitem__ + the default collate produce for inference.  With
share_keyframes, records of a batch that name the same image-0 file share one decoded frame and the batch is a keyframe-mode
batch (image0 [K, ...], keyframe_index [B]: README, "Keyframe mode").
"""
import concurrent.futures
import io
import os

import numpy as np
import torch

from . import ops


def correct_intrinsic_scale(K, scale_x, scale_y):
    """reference lib/datasets/utils.py:86-99: intrinsics of an image resized by (scale_x, scale_y), pixel centres at
    integer coordinates."""
    T = torch.eye(3, dtype=K.dtype)
    T[0, 0] = scale_x
    T[0, 2] = scale_x / 2 - 0.5
    T[1, 1] = scale_y
    T[1, 2] = scale_y / 2 - 0.5
    return T @ K


def decode_rgb(src):
    """JPEG / PNG file path, bytes or file object -> uint8 [H, W, 3] RGB (what cv2.imread + BGR2RGB give the reference)."""
    from PIL import Image
    if isinstance(src, (bytes, bytearray)):
        src = io.BytesIO(src)
    with Image.open(src) as im:
        return np.asarray(im.convert("RGB"))


def _collate(vals):
    """torch's default_collate for the metadata the dataset attaches: tuples are transposed (pair_names -> (names0,
    names1)), arrays / tensors stacked, everything else kept as a list."""
    v0 = vals[0]
    if isinstance(v0, (tuple, list)):
        return tuple(list(x) for x in zip(*vals))
    if isinstance(v0, np.ndarray):
        return torch.from_numpy(np.stack(vals))
    if torch.is_tensor(v0):
        return torch.stack(vals)
    return list(vals)


class FrameRing:
    """`slots` pinned uint8 staging buffers of [B, 2, Hs, Ws, 3] and their device twins; H2D copies on a side stream."""

    def __init__(self, B, Hs, Ws, device, slots=3):
        self.B, self.Hs, self.Ws, self.device = B, Hs, Ws, torch.device(device)
        self.host = [torch.empty((B, 2, Hs, Ws, 3), dtype=torch.uint8).pin_memory() for _ in range(slots)]
        self.dev = [torch.empty((B, 2, Hs, Ws, 3), dtype=torch.uint8, device=self.device) for _ in range(slots)]
        self.copied = [torch.cuda.Event() for _ in range(slots)]
        self.consumed = [torch.cuda.Event() for _ in range(slots)]
        self.stream = torch.cuda.Stream(self.device)
        self._first = [True] * slots

    def upload(self, slot):
        """Enqueue the copy of host slot -> device slot on the side stream (after the slot's previous consumer)."""
        with torch.cuda.stream(self.stream):
            if not self._first[slot]:
                self.stream.wait_event(self.consumed[slot])
            self.dev[slot].copy_(self.host[slot], non_blocking=True)
            self.copied[slot].record(self.stream)
        self._first[slot] = False

    def to_model_input(self, slot, H, W, n=None):
        """On the CURRENT stream: wait for the slot's copy, run resize + /255 + CHW, release the slot.
        Returns (image0, image1) fp32 [n, 3, H, W]."""
        n = self.B if n is None else n
        cur = torch.cuda.current_stream(self.device)
        cur.wait_event(self.copied[slot])
        frames = self.dev[slot][:n].reshape(n * 2, self.Hs, self.Ws, 3)
        out = ops.preprocess_u8(frames, H, W).reshape(n, 2, 3, H, W)
        self.consumed[slot].record(cur)
        return out[:, 0], out[:, 1]


def group_keyframes(batch):
    """Keyframe grouping of one batch of records (PairFeeder(share_keyframes=True)): -> (keyframes, keyframe_index) where
    keyframes lists the record index that supplies each distinct image 0, in order of first appearance, and keyframe_index[b]
    is the keyframe of record b.  Only image 0s given as file paths are merged (equal path = one frame); arrays and bytes are
    never merged."""
    first, keyframes, index = {}, [], []
    for b, r in enumerate(batch):
        src = r["image0"]
        key = os.fspath(src) if isinstance(src, (str, os.PathLike)) else None
        if key is None or key not in first:
            if key is not None:
                first[key] = len(keyframes)
            index.append(len(keyframes))
            keyframes.append(b)
        else:
            index.append(first[key])
    return keyframes, index


class PairFeeder:
    """Iterate device batches over a list of pair records.

    records: sequence of dicts with `image0`, `image1` (paths / bytes / already-decoded uint8 arrays), `K_color0`,
    `K_color1` (3x3, intrinsics of the STORED frames) and optional pass-through keys (scene_id, pair_names, ...).
    All frames must share one stored size (Map-free: 540 x 720); `resize` = (W, H) the model runs at.
    """

    def __init__(self, records, batch_size, resize, device="cuda:0", workers=None, slots=3, batches=None, share_keyframes=False):
        """batches: explicit list of record lists (each at most batch_size long, empty ones allowed) instead of cutting
        `records` into runs of batch_size -- a rank of a sharded evaluation passes its slice of every global batch, so it
        decodes, pins and uploads only the frames it will process; an empty slice yields a dict with 0-row tensors.
        share_keyframes: the records of a batch whose `image0` is the same path are decoded once (group_keyframes); the K
        distinct frames go to ring column 0, rows [0, K), and the batch carries `keyframe_index` (keyframe mode of the model).
        `frames_decoded` counts the frames this feeder has decoded so far."""
        self.share_keyframes = bool(share_keyframes)
        self.frames_decoded = 0
        self._batches = None if batches is None else [list(b) for b in batches]
        if self._batches is not None:
            records = [r for b in self._batches for r in b]
        self.records, self.B, self.resize = list(records), int(batch_size), (int(resize[0]), int(resize[1]))
        self.device = torch.device(device)
        # decode pool: half of the cores THIS process may run on (a rank pinned by distributed.pin_rank sizes its pool to its
        # own share; os.cpu_count() would give every one of 8 ranks a pool for the whole machine)
        ncpu = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 4)
        self.workers = workers or min(32, max(2, ncpu // 2))
        self.slots = slots
        self._ring = None

    def __len__(self):
        return len(self._batches) if self._batches is not None else (len(self.records) + self.B - 1) // self.B

    def _empty(self, H, W):
        z = lambda *s: torch.zeros(s, device=self.device)  # noqa: E731
        out = {"image0": z(0, 3, H, W), "image1": z(0, 3, H, W), "K_color0": z(0, 3, 3), "K_color1": z(0, 3, 3)}
        if self.share_keyframes:
            out["keyframe_index"] = torch.zeros((0,), dtype=torch.int64)
        return out

    @staticmethod
    def _decode_into(dst, src):
        img = src if isinstance(src, np.ndarray) else decode_rgb(src)
        if img.shape != tuple(dst.shape):
            raise ValueError("frame of size %s in a stream of %s frames" % (img.shape, tuple(dst.shape)))
        dst.numpy()[...] = img

    def __iter__(self):
        recs = self.records
        W, H = self.resize
        if not recs:
            for _ in (self._batches or []):   # a rank that owns nothing still steps through every global batch
                yield self._empty(H, W)
            return
        first = recs[0]["image0"]
        probe = first if isinstance(first, np.ndarray) else decode_rgb(first)
        Hs, Ws = probe.shape[:2]
        if self._ring is None or (self._ring.Hs, self._ring.Ws) != (Hs, Ws) or self._batches is not None:
            ring_b = max(len(b) for b in self._batches) if self._batches is not None else self.B
            self._ring = FrameRing(ring_b, Hs, Ws, self.device, self.slots)
        ring = self._ring
        sx, sy = W / Ws, H / Hs
        batches = self._batches if self._batches is not None else [recs[i:i + self.B] for i in range(0, len(recs), self.B)]
        with concurrent.futures.ThreadPoolExecutor(self.workers) as pool:
            def stage(bi):
                slot = bi % self.slots
                if not ring._first[slot]:
                    ring.copied[slot].synchronize()     # the pinned buffer is free once its last upload has left it
                futs = []
                kfs = group_keyframes(batches[bi])[0] if self.share_keyframes else range(len(batches[bi]))
                for i, b in enumerate(kfs):   # (without sharing: every record's own image 0, row i = record i)
                    futs.append(pool.submit(self._decode_into, ring.host[slot][i, 0], batches[bi][b]["image0"]))
                for i, r in enumerate(batches[bi]):
                    futs.append(pool.submit(self._decode_into, ring.host[slot][i, 1], r["image1"]))
                self.frames_decoded += len(futs)
                return slot, futs
            pending = {}
            ahead = min(self.slots - 1, len(batches))
            for bi in range(ahead):
                pending[bi] = stage(bi)
            for bi, batch in enumerate(batches):
                slot, futs = pending.pop(bi)
                for f in futs:
                    f.result()
                if len(batch):          # an empty slice has nothing to copy (the slot's pinned memory holds stale frames)
                    ring.upload(slot)
                nxt = bi + ahead
                if nxt < len(batches):
                    pending[nxt] = stage(nxt)   # decode the batch after next while this one is copied / computed
                n = len(batch)
                if n == 0:
                    yield self._empty(H, W)
                    continue
                im0, im1 = ring.to_model_input(slot, H, W, n)
                if self.share_keyframes:
                    kfs, kfi = group_keyframes(batch)
                    im0 = im0[:len(kfs)]   # the K keyframes (rows >= K of column 0 hold stale frames: dropped here)
                K0 = torch.stack([correct_intrinsic_scale(torch.as_tensor(r["K_color0"], dtype=torch.float32), sx, sy) for r in batch])
                K1 = torch.stack([correct_intrinsic_scale(torch.as_tensor(r["K_color1"], dtype=torch.float32), sx, sy) for r in batch])
                data = {"image0": im0, "image1": im1, "K_color0": K0.to(self.device, non_blocking=True),
                        "K_color1": K1.to(self.device, non_blocking=True)}
                if self.share_keyframes:
                    data["keyframe_index"] = torch.tensor(kfi, dtype=torch.int64)
                for k in batch[0]:
                    if k not in data:
                        data[k] = _collate([r[k] for r in batch])
                yield data


def bench_h2d(model, B, H, W, steps=3):
    """PCIe-inclusive rate for bench.py --include-h2d: already-DECODED uint8 frames sit in pageable host memory (what a
    decoder pool hands over); the timed loop stages them into the pinned ring, copies, preprocesses and runs the
    forward.  JPEG decoding itself (host cores, ~3-5 ms per 540x720 frame per core) is outside this figure."""
    import time
    dev = next(model.parameters()).device
    g = np.random.default_rng(0)
    frames = [g.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(8)]
    K = np.array([[549.7018, 0, 268.6665], [0, 549.7018, 351.8357], [0, 0, 1.0]], dtype=np.float32)
    recs = [{"image0": frames[i % 8], "image1": frames[(i + 3) % 8], "K_color0": K, "K_color1": K} for i in range(B * (steps + 1))]
    feeder = PairFeeder(recs, B, (W, H), device=dev)
    it = iter(feeder)
    model(next(it))                      # warm-up batch (ring allocation, first-touch)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n = 0
    for data in it:
        model(data)
        n += data["image0"].shape[0]
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return {"value": n / dt, "unit": "pairs/s", "steps": steps,
            "what": "uint8 frames in host memory -> pinned ring -> H2D (side stream) -> resize/normalise kernel -> forward; "
                    "JPEG decode excluded", "bytes_per_pair_over_pcie": 2 * H * W * 3}
