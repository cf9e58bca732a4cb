"""The packed weight streams of the 64->64 layers, element by element against float64 / exact rationals (tests/_wino_ref.py).

The Winograd kernels never read the Keras kernel: they read the five streams that fdn_pack_conv64_weights* re-forms after every optimizer
step, and a stream's rounding is the one error of the algorithm that is the same for every voxel and step.  csrc/conv64_pack.h claims: the
F(4,3) x F(4,3) stream is formed in double and rounded ONCE (half an ulp); its bf16 x 3 copy is u = hi + mid + lo exactly, every piece
round-to-nearest-even.  The convolution tests would not notice a pack that lost three ulps, truncated a piece or misplaced an element of a
stream few grids read (their bounds are 20 - 100 times the measured error).  Here every element of every stream, both directions, through
every pack entry point, for kernels at an aligned and at an odd offset of the flat parameter buffer:

    direct         bit-equal to w at the decoded index
    F(4,3)^2 fp32  |u - U| <= 0.5 ulp(u) (1 + 2^-20) against float64, and == the correctly rounded exact rational on 3000 sampled elements
    1-D, F(2,3)xF(4,3)   fp32 fma chains over rounded constants: |u - U| <= 4 * 2^-24 sum|G||w|, resp. 7 * 2^-24 sum|Gh||Gw||w| (one
                   rounding per constant and per fma; tests/test_wino_ref_host.py runs the same arithmetic in numpy)
    bf16 x 3       hi + mid + lo == u exactly; hi, mid, lo the RNE bf16 of u, u - hi, u - hi - mid
    bf16 operand stream (fdn_pack_conv64_weights_bf16[_batch])   RNE_bf16(w) at the decoded index
    _batch_streams with one bit   the other streams keep their bytes

One layer is (27,64,64): there is no smaller shape.  Weights: tests/_wino_ref.py stream_test_kernel (N(0, 0.05) + a block of exact values).
Subnormal, infinite and NaN weights are out of scope (conv64_pack.h: "finite weights")."""
import importlib

import numpy as np
import pytest
import torch

import _wino_ref as R

pytestmark = pytest.mark.gpu

SZ = 27 * 64 * 64
OFFSETS = (8, 8 + SZ + 1)                 # floats: 16-byte aligned / odd (a kernel behind a head's 1-float bias)
FILL = 0x7FC12345                         # a NaN no pack writes
ENTRIES = ("single", "batch", "streams")
DIRECTIONS = ("fwd", "dgrad")


@pytest.fixture(scope="module")
def ops(fdn):
    return fdn.ops


@pytest.fixture(scope="module")
def bops(fdn):
    return importlib.import_module("4dflownet_amd.ops_bf16")


@pytest.fixture(scope="module")
def layers():
    return [R.stream_test_kernel(5), R.stream_test_kernel(6)]


@pytest.fixture(scope="module")
def flat(layers):
    assert OFFSETS[0] % 4 == 0 and OFFSETS[1] % 2 == 1
    buf = np.full(OFFSETS[-1] + SZ + 3, 0.125, np.float32)
    for o, w in zip(OFFSETS, layers):
        buf[o:o + SZ] = w.ravel()
    t = torch.from_numpy(buf).cuda()
    assert t.data_ptr() % 16 == 0
    return t


def _filled(*shape):
    return torch.full(shape, FILL, dtype=torch.int32, device="cuda").view(torch.float32)


def _host(t):
    """A pack as the uint32 words it holds."""
    return t.contiguous().view(torch.int32).cpu().numpy().view(np.uint32)


@pytest.fixture(scope="module")
def packs(fdn, ops, flat):
    """{entry: uint32 [layer][direction][PACK_FLOATS]}; "streams": {bit: the same after a launch restricted to that stream}.  Every buffer is
    pre-filled with FILL."""
    n = len(OFFSETS)
    offs = torch.tensor(OFFSETS, device="cuda", dtype=torch.int64)
    out = {}
    single = _filled(n, 2, ops.CONV64_PACK_FLOATS)
    for i, o in enumerate(OFFSETS):
        ops.pack_conv64_weights(flat[o:o + SZ].view(3, 3, 3, 64, 64), wp_fwd=single[i, 0], wp_dgrad=single[i, 1])
    out["single"] = _host(single)
    batch = _filled(n, 2, ops.CONV64_PACK_FLOATS)
    ops.check(fdn._lib.load().fdn_pack_conv64_weights_batch(flat.data_ptr(), offs.data_ptr(), n, batch.data_ptr(),
                                                            torch.cuda.current_stream().cuda_stream), "fdn_pack_conv64_weights_batch")
    out["batch"] = _host(batch)
    out["streams"] = {}
    for bit in R.STREAM_BIT.values():
        p = _filled(n, 2, ops.CONV64_PACK_FLOATS)
        ops.pack_conv64_weights_batch(flat, offs, p, streams=(bit, bit))
        out["streams"][bit] = _host(p)
    torch.cuda.synchronize()
    return out


def stream_words(packs, entry, stream, layer, d):
    """The uint32 words of one stream of one pack as `entry` wrote it."""
    p = packs[entry][R.STREAM_BIT[stream]] if entry == "streams" else packs[entry]
    o, size = R.STREAMS[stream]
    return p[layer, d, o:o + size]


@pytest.fixture(scope="module")
def ref(layers):
    """float64 references, once: {(stream, layer, direction): U64 over the slots}, {...: sum |G||w|}, and the sampled exact values."""
    U, mag, exact = {}, {}, {}
    rng = np.random.default_rng(2)
    for i, w in enumerate(layers):
        for direction in DIRECTIONS:
            for stream in ("w", "h2", "h4"):
                U[stream, i, direction] = R.U64(w, stream, direction)
            for stream in ("w", "h2"):
                mag[stream, i, direction] = R.magnitude64(w, stream, direction)
            at = rng.choice(R.slots("h4"), 3000 // len(layers), replace=False)
            exact[i, direction] = (at, np.asarray([R.round_f32(v) for v in R.U_exact(w, "h4", direction, at)], np.float32))
    return U, mag, exact


def test_every_float_of_every_pack_is_written(packs):
    """No slot of the 423 x 4096 floats is left out by the full packs (the streams tile the pack: tests/test_wino_ref_host.py)."""
    for entry in ("single", "batch"):
        assert not (packs[entry] == FILL).any(), entry


@pytest.mark.parametrize("entry", ENTRIES)
def test_direct_stream_is_the_kernel_bit_for_bit(packs, layers, entry):
    for d, direction in enumerate(DIRECTIONS):
        src = R.source_index("direct", direction)
        for i, w in enumerate(layers):
            assert np.array_equal(stream_words(packs, entry, "direct", i, d), w.ravel().view(np.uint32)[src]), (direction, i)


@pytest.mark.parametrize("entry", ENTRIES)
def test_f43xf43_stream_is_float64_rounded_once(packs, ref, entry, capsys):
    """Half an ulp of the stored value against float64 (2^-20 relative slack for float64's own error), everywhere; the correctly rounded exact
    rational on 3000 sampled elements."""
    U, _, exact = ref
    worst = 0.0
    for d, direction in enumerate(DIRECTIONS):
        for i in range(len(OFFSETS)):
            u = stream_words(packs, entry, "h4", i, d).view(np.float32)
            assert np.isfinite(u).all()
            ulp = np.spacing(np.abs(u)).astype(np.float64)
            err = np.abs(u.astype(np.float64) - U["h4", i, direction])
            worst = max(worst, float((err / ulp).max()))
            bad = err > 0.5 * ulp * (1 + 2.0 ** -20)
            assert not bad.any(), (direction, i, int(bad.sum()), float((err / ulp).max()))
            at, want = exact[i, direction]
            assert np.array_equal(u[at], want), (direction, i, int((u[at] != want).sum()))
    with capsys.disabled():
        print("\n[pack-streams] %s F(4,3)xF(4,3): max |u - U| = %.5f ulp" % (entry, worst))
    assert worst > 0.4                                        # (the measurement resolves half an ulp: some element comes close to it)


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("stream,factor", [("w", 4), ("h2", 7)])
def test_fma_chain_streams_stay_inside_their_rounding_bound(packs, ref, entry, stream, factor, capsys):
    """fp32 fma chains over fp32-rounded constants: one rounding per constant plus one per fma, relative to sum |G||w|."""
    U, mag, _ = ref
    worst = 0.0
    for d, direction in enumerate(DIRECTIONS):
        for i in range(len(OFFSETS)):
            u = stream_words(packs, entry, stream, i, d).view(np.float32)
            assert np.isfinite(u).all()
            err = np.abs(u.astype(np.float64) - U[stream, i, direction])
            m = mag[stream, i, direction]
            assert (err <= factor * 2.0 ** -24 * m).all(), (direction, i, float((err[m > 0] / m[m > 0]).max() * 2.0 ** 24))
            worst = max(worst, float((err[m > 0] / m[m > 0]).max() * 2.0 ** 24))
    with capsys.disabled():
        print("\n[pack-streams] %s %s: max |u - U| = %.2f x 2^-24 sum|G||w| (bound %d)" % (entry, stream, worst, factor))


@pytest.mark.parametrize("entry", ENTRIES)
def test_bf16x3_stream_is_an_exact_rne_split(packs, entry):
    """u = hi + mid + lo exactly, u the fp32 stream's value; hi = RNE(u), mid = RNE(u - hi), lo = RNE(u - hi - mid), bit for bit."""
    d4, d4s = R.decode("h4"), R.decode("h4s")
    back = R.encode("h4", **{n: d4s[n] for n in R.COORDS["h4"]})              # slot of the fp32 stream each bf16 slot belongs to
    for d, direction in enumerate(DIRECTIONS):
        for i in range(len(OFFSETS)):
            u = stream_words(packs, entry, "h4", i, d).view(np.float32)
            bits = stream_words(packs, entry, "h4s", i, d).view(np.uint16)
            assert bits.size == R.slots("h4s")
            piece = {p: np.empty(u.size, np.uint16) for p in range(3)}
            for p in range(3):
                sel = d4s["piece"] == p
                piece[p][back[sel]] = bits[sel]
            hi, mid, lo = (R.bf16_to_f32(piece[p]) for p in range(3))
            f = lambda a: a.astype(np.float64)
            assert np.array_equal(f(hi) + f(mid) + f(lo), f(u)), (direction, i)
            assert np.array_equal(piece[0], R.bf16_rne_bits(u)), (direction, i)
            r1 = u - hi
            assert np.array_equal(f(r1), f(u) - f(hi))                            # (exact in fp32)
            assert np.array_equal(piece[1], R.bf16_rne_bits(r1)), (direction, i)
            r2 = r1 - mid
            assert np.array_equal(f(r2), f(r1) - f(mid))
            assert np.array_equal(piece[2], R.bf16_rne_bits(r2)), (direction, i)
    assert np.array_equal(np.sort(back[d4s["piece"] == 0]), np.arange(d4["k"].size))


@pytest.mark.parametrize("stream", list(R.STREAM_BIT))
def test_a_single_stream_launch_leaves_the_other_streams_alone(packs, stream):
    """fdn_pack_conv64_weights_batch_streams with one bit: that stream equals the full pack's, every other float keeps its bytes."""
    p = packs["streams"][R.STREAM_BIT[stream]]
    o, size = R.STREAMS[stream]
    assert np.array_equal(p[:, :, o:o + size], packs["batch"][:, :, o:o + size])
    assert (p[:, :, :o] == FILL).all() and (p[:, :, o + size:] == FILL).all()


def test_streams_launch_with_different_masks_per_direction(ops, flat, packs):
    """Forward and dgrad masks are independent: (F(4,3)^2 | direct) forward, 1-D dgrad."""
    offs = torch.tensor(OFFSETS, device="cuda", dtype=torch.int64)
    p = _filled(len(OFFSETS), 2, ops.CONV64_PACK_FLOATS)
    ops.pack_conv64_weights_batch(flat, offs, p, streams=(ops.PACK_STREAM_WINO_H4 | ops.PACK_STREAM_DIRECT, ops.PACK_STREAM_WINO_W))
    p = _host(p)
    want = np.full_like(p, FILL)
    for d, names in enumerate((("direct", "h4"), ("w",))):
        for name in names:
            o, size = R.STREAMS[name]
            want[:, d, o:o + size] = packs["batch"][:, d, o:o + size]
    assert np.array_equal(p, want)


@pytest.mark.parametrize("entry", ["single", "batch"])
def test_bf16_operand_stream_is_rne_of_the_kernel(bops, flat, layers, entry):
    """fdn_pack_conv64_weights_bf16[_batch]: every element RNE_bf16(w) at its decoded index (truncation fails on about half of them)."""
    n = len(OFFSETS)
    packs = torch.full((n, 2, bops.PACK_ELEMS), 0x7FC1, dtype=torch.int16, device="cuda").view(torch.bfloat16)
    if entry == "single":
        for i, o in enumerate(OFFSETS):
            bops.pack_conv64_weights(flat[o:o + SZ].view(3, 3, 3, 64, 64), wp_fwd=packs[i, 0], wp_dgrad=packs[i, 1])
    else:
        bops.pack_conv64_weights_batch(flat, torch.tensor(OFFSETS, device="cuda", dtype=torch.int64), packs)
    got = packs.view(torch.int16).cpu().numpy().view(np.uint16)
    for d, direction in enumerate(DIRECTIONS):
        src = R.source_index("bf16", direction)
        for i, w in enumerate(layers):
            want = R.bf16_rne_bits(w.ravel()[src])
            assert np.array_equal(got[i, d], want), (direction, i, int((got[i, d] != want).sum()))
            trunc = (w.ravel()[src].view(np.uint32) >> 16).astype(np.uint16)
            assert (trunc != want).mean() > 0.3                               # (the operands tell the two roundings apart)
