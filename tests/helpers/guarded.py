"""Guarded output buffers for kernel tests: a [rows, cols] window inside one flat allocation whose every other element -- guard
rows in front and behind, and the cols..ld slack of every row -- holds a sentinel bit pattern, so that a store one row past M or
one column past N is seen instead of landing in somebody else's allocation."""
import torch

# Finite, non-zero, far outside anything test data of unit scale produces (fp16 5.5e4, bf16 / fp32 1.1e36); compared as
# integers of the same width, so -0.0 / NaN payloads / a rewritten equal value of another sign cannot hide.
_SENTINEL = {torch.float16: (torch.int16, 0x7AB7), torch.bfloat16: (torch.int16, 0x7B57), torch.float32: (torch.int32, 0x7B57A3C5)}
ALIGN = 256   # bytes: the window starts on this boundary (the kernels' widest vector access is 16 B)


def int_dtype(dtype):
    """Integer dtype of the same width as `dtype`."""
    return _SENTINEL[dtype][0]


def sentinel_bits(dtype):
    """The sentinel of `dtype` as an integer of its width."""
    return _SENTINEL[dtype][1]


def bits(t):
    """`t` reinterpreted as integers of the same width (any strides)."""
    return t.view(int_dtype(t.dtype))


def guarded(rows, cols, dtype, device, ld=None, fill=None):
    """-> (view, check).  view: [rows, cols] with row stride ld >= cols (default cols), 256-byte aligned, at least 4 full rows and at
    least 256 bytes of guard in front of it and behind it.  Everything but the window holds the sentinel, and so does the window
    itself unless `fill` (a number or a tensor that broadcasts to [rows, cols]) pre-sets it.  check() asserts that every element
    outside the window still holds the sentinel and names the first offender as (row, column) relative to the window: rows < 0 /
    >= rows are guard rows, columns >= cols the row slack."""
    ld = cols if ld is None else ld
    assert rows > 0 and cols > 0 and ld >= cols
    idt, sbits = _SENTINEL[dtype]
    esz = torch.empty((), dtype=dtype).element_size()
    guard = max(4 * ld, ALIGN // esz)
    flat = torch.full((ALIGN // esz + guard + rows * ld + guard,), sbits, dtype=idt, device=device)
    off = guard + (-(flat.data_ptr() + guard * esz) % ALIGN) // esz
    assert (flat.data_ptr() + off * esz) % ALIGN == 0 and off >= guard and off + rows * ld + guard <= flat.numel()
    view = flat.view(dtype)[off:off + rows * ld].view(rows, ld)[:, :cols]
    outside = torch.ones(flat.numel(), dtype=torch.bool, device=device)
    outside[off:off + rows * ld].view(rows, ld)[:, :cols] = False
    if fill is not None:
        if torch.is_tensor(fill):
            view.copy_(fill)
        else:
            view.fill_(fill)

    def check():
        bad = outside & (flat != sbits)
        if bool(bad.any()):
            rel = int(torch.nonzero(bad)[0]) - off
            row, col = rel // ld, rel % ld     # floor division: elements in front of the window get negative rows
            raise AssertionError("guard overwritten at (row %d, column %d) of a [%d, %d] window with ld %d: %d of %d guard elements "
                                 "changed" % (row, col, rows, cols, ld, int(bad.sum()), int(outside.sum())))

    return view, check


def window(rows, cols, dev, shift=0):
    """-> (flat fp32 view of rows * cols elements, check).  shift = 0: a guarded [rows, cols] window (256-byte aligned).  shift = 1 /
    2: the same elements taken `shift` floats into a guarded [1, rows * cols + 2] window -- 4 / 8 bytes off every 16-byte boundary;
    check() then also looks at the skipped elements in front of and behind the view."""
    n = rows * cols
    if shift == 0:
        w, check = guarded(rows, cols, torch.float32, dev)
        assert w.is_contiguous()
        return w.view(-1), check
    big, check0 = guarded(1, n + 2, torch.float32, dev)
    view = big[0, shift:shift + n]
    assert view.data_ptr() % 16 == 4 * shift
    sent = sentinel_bits(torch.float32)

    def check():
        check0()
        skipped = torch.cat([bits(big[0, :shift]), bits(big[0, shift + n:])])
        assert skipped.numel() == 2 and bool((skipped == sent).all()), "an element next to a misaligned output was overwritten"

    return view, check


def vt_perm(t):
    """Column of V^T that holds token t: bits 2 and 3 of the token index swapped."""
    return (t & ~12) | ((t & 4) << 1) | ((t & 8) >> 1)


def pad_mask(ntok, pad):
    """The set of V^T columns that are padding: {perm(t) : ntok <= t < pad}, which is NOT columns >= ntok."""
    return {vt_perm(t) for t in range(ntok, pad)}
