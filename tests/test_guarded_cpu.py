"""The guarded-buffer helper of the kernel tests (tests/helpers/guarded.py) on CPU tensors: its geometry, and that check() sees
a stray write wherever one can land -- with the right coordinates."""
import re

import pytest
import torch

from tests.helpers.guarded import ALIGN, bits, guarded, pad_mask, sentinel_bits, vt_perm

DTYPES = [torch.float32, torch.bfloat16, torch.float16]


def _flat(view):
    """The whole allocation behind a guarded view, as integers, and the window's offset in it."""
    esz = view.element_size()
    base = view.untyped_storage().data_ptr()
    n = view.untyped_storage().nbytes() // esz
    flat = torch.empty(0, dtype=view.dtype).set_(view.untyped_storage(), 0, (n,), (1,))
    return bits(flat), (view.data_ptr() - base) // esz


def _where(check):
    with pytest.raises(AssertionError) as e:
        check()
    m = re.search(r"\(row (-?\d+), column (\d+)\)", str(e.value))
    assert m, str(e.value)
    return int(m.group(1)), int(m.group(2))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows,cols,ld", [(5, 12, 20), (1, 4, 4), (7, 64, 72), (3, 1, 1), (257, 192, 200)])
def test_geometry(rows, cols, ld, dtype):
    view, check = guarded(rows, cols, dtype, "cpu", ld=ld)
    assert tuple(view.shape) == (rows, cols) and view.stride(1) == 1 and (rows == 1 or view.stride(0) == ld)
    assert view.data_ptr() % ALIGN == 0
    flat, off = _flat(view)
    esz = view.element_size()
    front, back = off, flat.numel() - off - rows * ld
    assert front >= 4 * ld and front * esz >= 256 and back >= 4 * ld and back * esz >= 256
    s = sentinel_bits(dtype)
    assert bool((flat == s).all())                       # guards, slack and (no fill) the window
    x = torch.tensor(s, dtype=bits(view).dtype).view(dtype)
    assert bool(torch.isfinite(x.float())) and abs(float(x)) > 1e4
    check()
    view.zero_()                                         # every window element may change
    check()
    assert int((flat != s).sum()) == rows * cols


@pytest.mark.parametrize("dtype", DTYPES)
def test_fill_presets_the_window_only(dtype):
    view, check = guarded(6, 8, dtype, "cpu", ld=16, fill=1.5)
    assert bool((view == 1.5).all())
    check()
    t = torch.arange(48, dtype=torch.float32).reshape(6, 8)
    view2, check2 = guarded(6, 8, dtype, "cpu", ld=16, fill=t)
    assert torch.equal(view2.float(), t)
    check2()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("ld", [12, 20])
def test_check_has_teeth(ld, dtype):
    rows, cols = 5, 12

    def fresh():
        view, check = guarded(rows, cols, dtype, "cpu", ld=ld, fill=0.0)
        flat, off = _flat(view)
        return view, check, flat, off

    view, check, flat, off = fresh()        # one element in front of the window
    flat[off - 1] = 0
    assert _where(check) == (-1, ld - 1)
    view, check, flat, off = fresh()        # one element behind the window's last element
    flat[off + (rows - 1) * ld + cols] = 0
    assert _where(check) == ((rows - 1, cols) if ld > cols else (rows, 0))
    if ld > cols:                           # the ld slack of a middle row, first and last slack column
        for c in (cols, ld - 1):
            view, check, flat, off = fresh()
            flat[off + 2 * ld + c] = 0
            assert _where(check) == (2, c)
    view, check, flat, off = fresh()        # the last guard row, its last element = the last element of the allocation's guard
    back = flat.numel() - off - rows * ld
    assert back >= 4 * ld
    flat[off + rows * ld + 4 * ld - 1] = 0
    assert _where(check) == (rows + 3, ld - 1)
    view, check, flat, off = fresh()        # and the first guard row in front
    flat[off - 4 * ld] = 0
    assert _where(check) == (-4, 0)
    view, check, flat, off = fresh()        # the first offender is named, the count is of all of them
    flat[off + ld + cols:off + ld + ld] = 0
    flat[off - 2] = 0
    assert _where(check) == (-1, ld - 2)
    view, check, flat, off = fresh()        # a write that changes one bit only (compared as integers, not as values)
    flat[off - 1] = flat[off - 1] ^ 1
    assert _where(check) == (-1, ld - 1)
    view, check, flat, off = fresh()        # writes inside the window pass, whatever they write
    view[0, 0] = 3.0
    view[rows - 1, cols - 1] = -7.0
    view[2] = float("nan")
    check()


def test_pad_mask_follows_the_vt_permutation():
    for t in range(64):
        assert vt_perm(vt_perm(t)) == t and (vt_perm(t) & ~12) == (t & ~12)
    assert [vt_perm(t) for t in (0, 3, 4, 7, 8, 11, 12, 15, 16, 20)] == [0, 3, 8, 11, 4, 7, 12, 15, 16, 24]
    assert pad_mask(64, 64) == set()
    assert pad_mask(65, 128) == set(range(64, 128)) - {64}
    assert pad_mask(1, 64) == set(range(1, 64))
    # where padding is not "columns >= ntok": 5 tokens occupy columns {0, 1, 2, 3, 8}
    assert pad_mask(5, 64) == set(range(64)) - {0, 1, 2, 3, 8}
    assert 4 in pad_mask(5, 64) and 8 not in pad_mask(5, 64)
    for ntok, pad in ((333, 384), (63, 64), (65, 192), (9, 64)):
        m = pad_mask(ntok, pad)
        live = {vt_perm(t) for t in range(ntok)}
        assert len(m) == pad - ntok and not (m & live) and (m | live) == set(range(pad))
