"""tests/_guarded.py catches what it is for -- on the CPU, with torch operations standing in for a kernel that oversteps its operands."""
import pytest
import torch

import _guarded as G

DTYPES = [torch.float32, torch.bfloat16, torch.float64, torch.int16, torch.uint8]
SHAPES = [(1,), (7,), (2, 3), (1, 5, 3), (1, 5, 7, 9, 64), (2, 9, 2, 24, 64), (1, 3, 20, 11, 3), (2, 4, 37)]


def _expected_band(shape, item):
    slab = 1
    if len(shape) >= 3:
        slab = shape[-1]
        for e in shape[2:-1]:
            slab *= e + 2
    n = max(4096, slab)
    q = 512 // item
    return -(-n // q) * q


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES)
def test_layout_and_rounding(shape, dtype):
    for run in ("A", "B"):
        fill = G.fill_for(dtype, run)
        h = G.guarded(shape, dtype, fill)
        item = h.buf.element_size()
        n = h.t.numel()
        assert h.buf.dim() == 1 and h.buf.dtype == dtype and h.t.dtype == dtype
        assert tuple(h.t.shape) == tuple(shape) and h.t.is_contiguous()
        assert h.band == _expected_band(shape, item) and h.band >= 4096 and (h.band * item) % 512 == 0
        assert h.buf.numel() == n + 2 * h.band
        assert h.t.data_ptr() - h.buf.data_ptr() == h.band * item                     # in the middle, 512-byte steps from the start
        assert h.t.untyped_storage().data_ptr() == h.buf.untyped_storage().data_ptr()   # a view, not a copy
        assert G.intact(h) and h.damaged() == []
        assert G.unchanged(h, h.t.clone())


def test_band_is_one_padded_slab_where_that_is_larger():
    assert G.band_elems((1, 5, 7, 9, 64), torch.float32) == 6400                        # (H + 2)(W + 2) C = 6336 -> 50 * 128 (512 bytes)
    assert G.band_elems((1, 3, 20, 11, 3), torch.float32) == 4096                       # 22 * 13 * 3 = 858 < 4096
    assert G.band_elems((1, 16, 16, 16, 64), torch.bfloat16) == 18 * 18 * 64
    assert G.band_elems((1, 5, 7, 9, 3), torch.float64) == 4096
    assert G.band_elems((2, 6, 14, 10, 64), torch.float32) == 16 * 12 * 64
    assert G.band_elems((1, 1, 5, 5, 64), torch.float32) == 4096                        # 7 * 7 * 64 = 3136 < 4096
    assert G.band_elems((1, 1, 7, 7, 67), torch.float32) == -(-9 * 9 * 67 // 128) * 128  # 5427 -> 5504: rounded up to 512 bytes


def test_fills():
    assert G.fill_for(torch.int16, "B") == 0x5A5A and G.fill_for(torch.int16, "A") == -1
    assert G.fill_for(torch.uint8, "A") == 0xFF and G.fill_for(torch.uint8, "B") == 0x00
    assert G.fill_for(torch.float32, "B") == 1234.5 and G.fill_for(torch.float32, "A") != G.fill_for(torch.float32, "A")
    h = G.guarded((3,), torch.bfloat16, G.NAN)
    assert bool(torch.isnan(h.buf).all())                                               # the NaN pattern of bf16, not of fp32
    h = G.guarded((3,), torch.int16, -1)
    assert bool((h.buf.view(torch.uint8) == 0xFF).all())                                # all ones
    h = G.guarded((3,), torch.int64, G.fill_for(torch.int64, "B"))
    assert bool((h.buf.view(torch.uint8) == 0x5A).all())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("where", [-1, "end"])
def test_a_write_one_element_outside_the_view_is_seen(dtype, where):
    for run in ("A", "B"):
        h = G.guarded((2, 3, 5), dtype, G.fill_for(dtype, run))
        flat = h.buf
        i = h.band - 1 if where == -1 else h.band + h.numel
        flat[i] = 3                                                                     # the stand-in kernel's stray store
        assert not G.intact(h)
        assert h.damaged() == [-1 if where == -1 else h.numel]
        # the same value as the fill is, rightly, not a change
        h2 = G.guarded((2, 3, 5), dtype, G.fill_for(dtype, run))
        h2.buf[i] = G.fill_for(dtype, run)
        assert G.intact(h2)


def test_a_nan_of_another_bit_pattern_in_a_nan_band_is_seen():
    h = G.guarded((4,), torch.float32, G.NAN)
    h.buf.view(torch.int32)[h.band + 4] = 0x7FC00001                                    # still a NaN, not the fill's bits
    assert bool(torch.isnan(h.buf[h.band + 4])) and not G.intact(h)


def test_interior_writes_are_seen_by_unchanged_only():
    for dtype in DTYPES:
        h = G.guarded((5, 4), dtype, G.fill_for(dtype, "A"))
        h.t.copy_(torch.arange(20).reshape(5, 4).to(dtype))
        snap = h.t.clone()
        assert G.unchanged(h, snap)
        h.t[4, 3] = 7
        assert not G.unchanged(h, snap) and G.intact(h)
    h = G.guarded((2,), torch.float32, G.SENTINEL)
    h.t.copy_(torch.tensor([0.0, 1.0]))
    snap = h.t.clone()
    h.t[0] = -0.0                                                                       # equal as numbers, not as bits
    assert not G.unchanged(h, snap)


def test_a_reduction_one_element_too_wide_is_poisoned_or_shifted():
    x = torch.arange(1.0, 13.0).reshape(3, 4)
    got = {}
    for name, fill in (("nan", G.NAN), ("finite", G.SENTINEL), ("zeros", 0.0)):
        h = G.guarded_like(x, fill)
        start = h.band
        got[name] = float(h.buf[start:start + h.numel + 1].sum())                       # the stand-in kernel reads one element too many
        assert float(h.buf[start:start + h.numel].sum()) == 78.0                        # the right slice is untouched by the fill
        assert G.intact(h) and G.unchanged(h, x)                                        # a read leaves no trace in memory: only the value tells
    assert got["nan"] != got["nan"]
    assert got["zeros"] == 78.0 and got["finite"] == 78.0 + 1234.5 and got["finite"] != got["zeros"]
    # "times zero" does not save an overhanging load from a NaN neighbour
    h = G.guarded_like(x, G.NAN)
    wts = torch.ones(13)
    wts[12] = 0.0
    assert bool(torch.isnan((h.buf[h.band:h.band + 13] * wts).sum()))


@pytest.mark.parametrize("nbytes", [1, 4, 6, 4096, 2048 * 64 * 4, 27 * 64 * 64 * 4 + 2])
def test_exact_workspace(nbytes):
    h = G.exact_workspace(nbytes, G.NAN, G.SENTINEL)
    usable = (nbytes + 3) // 4 * 4
    assert h.t.dtype == torch.float32 and h.t.numel() * 4 == usable and usable - nbytes in (0, 1, 2, 3)
    assert bool(torch.isnan(h.t).all()) and G.intact(h)
    raw = h.buf.view(torch.uint8)
    first = h.band * 4
    raw[first + usable - 1] = 1                                                         # the last usable byte: fine
    assert G.intact(h)
    raw[first + usable] ^= 0x40                                                         # a consumer that touches byte `nbytes` (rounded up to 4)
    assert not G.intact(h) and h.damaged() == [h.numel]
    h = G.exact_workspace(nbytes, G.SENTINEL, G.NAN)
    h.buf.view(torch.uint8)[h.band * 4 - 1] ^= 0x01                                      # and one byte in front of it
    assert not G.intact(h) and h.damaged() == [-1]


def test_guarded_like_copies():
    x = torch.randn(2, 3, 4, 5, 6).to(torch.bfloat16)
    h = G.guarded_like(x, G.NAN)
    assert torch.equal(h.t, x) and h.t.dtype == torch.bfloat16 and G.intact(h) and G.unchanged(h, x)
    assert h.t.data_ptr() != x.data_ptr()
