"""Guard bands around operands, in plain torch (nothing from the package), on whatever device is asked for.

    guarded(shape, dtype, fill, device)      a handle h: h.buf is ONE flat allocation, h.t a contiguous view of `shape` in the middle of it,
                                             with a band of h.band elements holding `fill` on either side.  The interior starts as `fill` too.
    intact(h)                                both bands still hold the fill, bit for bit (integer views: NaN != NaN).
    unchanged(h, snapshot)                   the interior equals `snapshot` (h.t.clone() taken before the launch), bit for bit.
    exact_workspace(nbytes, fill_inside, fill_band, device)
                                             a float32 workspace whose usable size is nbytes rounded up to 4 and not one byte more.

Band length in elements: the larger of 4096 and one padded slab of the operand -- the product of all but the first two extents after adding
2 to each spatial extent, (H + 2) (W + 2) C for (N,D,H,W,C) -- rounded up so that its byte length is a multiple of 512: the view keeps the
512-byte alignment every torch allocation has (alignment is deliberately not a variable here).  Every tile overhang of the library stays
within one row or plane of a tile; the band is far larger than any of them.

Fills: floating types take a quiet NaN or the finite sentinel 1234.5 (bf16: the NaN of that type); int16 mask words 0x5A5A or all ones;
uint8 flag arrays 0xFF or 0x00; wider integers (offset and descriptor tables) the same byte patterns.  fill_for(dtype, run) names the fill of
run "A" (NaN, all ones, 0xFF) and of run "B" (the finite sentinel, 0x5A5A, 0x00)."""
import math

import torch

SENTINEL, SENTINEL_WORD = 1234.5, 0x5A5A            # tests/test_gpu_pow2_scaling.py
NAN = float("nan")
MIN_BAND = 4096
ALIGN = 512
_INT_VIEW = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def fill_for(dtype, run):
    """The fill of `run` ("A" or "B") for a tensor of `dtype`."""
    assert run in ("A", "B")
    if dtype.is_floating_point:
        return NAN if run == "A" else SENTINEL
    if dtype == torch.uint8:
        return 0xFF if run == "A" else 0x00
    if dtype == torch.int16:
        return -1 if run == "A" else SENTINEL_WORD
    return -1 if run == "A" else int.from_bytes(b"\x5a" * torch.empty((), dtype=dtype).element_size(), "little")


def band_elems(shape, dtype):
    """Band length on each side, in elements."""
    shape = tuple(int(s) for s in shape)
    slab = 1
    if len(shape) >= 3:
        slab = shape[-1]
        for e in shape[2:-1]:
            slab *= e + 2
    item = torch.empty((), dtype=dtype).element_size()
    assert ALIGN % item == 0
    q = ALIGN // item
    return (max(MIN_BAND, slab) + q - 1) // q * q


def _bits(t):
    """A view of t as integers of its element size (NaN compares equal to itself there)."""
    return t if not t.dtype.is_floating_point else t.view(_INT_VIEW[t.element_size()])


class Guarded:
    def __init__(self, buf, band, shape, fill):
        n = 1
        for s in shape:
            n *= int(s)
        self.buf, self.band, self.fill, self.numel = buf, band, fill, n
        self.t = buf[band:band + n].view(tuple(shape))
        self._pattern = _bits(torch.full((1,), fill, dtype=buf.dtype, device=buf.device))

    def bands(self):
        return self.buf[:self.band], self.buf[self.band + self.numel:]

    def damaged(self):
        """Flat indices RELATIVE TO THE VIEW of the band elements that no longer hold the fill (negative: in front of it)."""
        lo, hi = (_bits(b) != self._pattern for b in self.bands())
        return [int(i) - self.band for i in lo.nonzero().reshape(-1)[:8]] + [int(i) + self.numel for i in hi.nonzero().reshape(-1)[:8]]


def guarded(shape, dtype, fill, device="cpu"):
    shape = tuple(int(s) for s in shape)
    band = band_elems(shape, dtype)
    n = math.prod(shape)
    buf = torch.full((2 * band + n,), fill, dtype=dtype, device=device)
    h = Guarded(buf, band, shape, fill)
    assert h.t.is_contiguous() and h.t.data_ptr() - buf.data_ptr() == band * buf.element_size()
    assert (band * buf.element_size()) % ALIGN == 0 and len(h.bands()[1]) == band
    return h


def guarded_like(t, fill):
    """A guarded copy of t: same shape, dtype, device and contents."""
    h = guarded(t.shape, t.dtype, fill, t.device)
    h.t.copy_(t)
    return h


def intact(h):
    lo, hi = h.bands()
    return bool((_bits(lo) == h._pattern).all()) and bool((_bits(hi) == h._pattern).all())


def unchanged(h, snapshot):
    return snapshot.shape == h.t.shape and snapshot.dtype == h.t.dtype and bool(torch.equal(_bits(h.t), _bits(snapshot)))


def exact_workspace(nbytes, fill_inside, fill_band, device="cpu"):
    """A float32 workspace of exactly (nbytes + 3) // 4 elements between two bands of at least MIN_BAND elements: numel * 4 is what a
    caller hands to the library as ws_bytes."""
    n = (int(nbytes) + 3) // 4
    h = guarded((n,), torch.float32, fill_band, device)
    h.t.fill_(fill_inside)
    assert h.t.numel() * 4 == (int(nbytes) + 3) // 4 * 4
    return h
