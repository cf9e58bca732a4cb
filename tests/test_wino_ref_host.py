"""The float64 / rational Winograd model of tests/_wino_ref.py, checked on the host: the transform identities in exact arithmetic, the
stream decodings as bijections, the model against the oracle's plain float64 convolution, and the arithmetic facts the GPU stream tests
(tests/test_gpu_pack_streams.py) build their bounds on."""
from fractions import Fraction as Fr

import numpy as np
import pytest

import _wino_ref as R


@pytest.mark.parametrize("name", ["F43", "F43s", "F23"])
def test_transform_identity_holds_exactly(name):
    """A^T[(G g) (.) (B^T d)] = correlation(d, g) for every unit g and d, in Fractions."""
    assert R.identity_residual(name) == 0
    G, Bt, At = R.transform(name)
    n = len(R.POINTS[name])
    assert len(G) == len(Bt) == n and len(At) == n - 2 and all(len(r) == n for r in Bt)


def test_G_is_what_the_pack_header_documents():
    """csrc/conv64_pack.h spells the three G matrices out; the ones derived from the points are those."""
    F = Fr
    assert R.transform("F43")[0] == [[F(1, 4), 0, 0], [F(-1, 6)] * 3, [F(-1, 6), F(1, 6), F(-1, 6)], [F(1, 24), F(1, 12), F(1, 6)],
                                     [F(1, 24), F(-1, 12), F(1, 6)], [0, 0, 1]]
    assert R.transform("F23")[0] == [[1, 0, 0], [F(1, 2)] * 3, [F(1, 2), F(-1, 2), F(1, 2)], [0, 0, 1]]
    assert R.transform("F43s")[0] == [[F(64, 81), 0, 0], [F(-128, 243), F(-32, 81), F(-8, 27)], [F(-128, 243), F(32, 81), F(-8, 27)],
                                      [F(32, 243), F(16, 81), F(8, 27)], [F(32, 243), F(-16, 81), F(8, 27)], [0, 0, 1]]


@pytest.mark.parametrize("stream", ["direct", "w", "h2", "h4", "h4s", "bf16"])
def test_decode_is_a_bijection_onto_the_coordinate_set(stream):
    """Every coordinate tuple of the stream is hit by exactly one slot, and encode is decode's inverse."""
    d = R.decode(stream)
    names = R.COORDS[stream]
    ext = [R.extent(stream, n) for n in names]
    n = R.slots(stream)
    assert int(np.prod(ext)) == n
    for name, e in zip(names, ext):
        assert d[name].min() == 0 and d[name].max() == e - 1
    flat = np.ravel_multi_index(tuple(d[name] for name in names), ext)
    assert np.array_equal(np.sort(flat), np.arange(n))                 # onto, and no tuple twice
    assert np.array_equal(R.encode(stream, **{name: d[name] for name in names}), np.arange(n))
    assert set(np.unique(d["sign"])) == ({-1, 1} if stream == "h2" else {1})
    assert stream != "h2" or ((d["sign"] == -1) == (d["xh"] == 2)).all()


def test_the_five_streams_tile_the_pack():
    """Offsets 0, 27, 81, 153, 261 x 4096 floats, back to back, 423 x 4096 in all: no float of a pack is left out or claimed twice."""
    at = 0
    for stream, off in zip(("direct", "w", "h2", "h4", "h4s"), (0, 27, 81, 153, 261)):
        o, size = R.STREAMS[stream]
        assert o == at == off * 4096
        assert R.slots(stream) == size * (2 if stream == "h4s" else 1)      # the bf16 x 3 stream: two 2-byte slots per float
        at += size
    assert at == R.PACK_FLOATS == 423 * 4096
    assert R.slots("bf16") == 27 * 4096


@pytest.mark.parametrize("direction", ["fwd", "dgrad"])
def test_copy_streams_read_every_weight_once(direction):
    """The direct and bf16 operand streams are permutations of the Keras kernel; dgrad: taps flipped, channels transposed."""
    for stream in ("direct", "bf16"):
        src = R.source_index(stream, direction)
        assert np.array_equal(np.sort(src), np.arange(27 * 4096))
        d = R.decode(stream, direction)
        assert np.array_equal(src, (d["layer_tap"] * 64 + d["cin"]) * 64 + d["cout"])
    w = np.arange(27 * 4096, dtype=np.float64).reshape(27, 64, 64)
    g = R.effective_kernel(w, direction)
    t, k, c = 5, 7, 40
    assert g.reshape(27, 64, 64)[t, k, c] == (w[t, k, c] if direction == "fwd" else w[26 - t, c, k])


@pytest.fixture(scope="module")
def operands():
    rng = np.random.default_rng(11)
    w = rng.standard_normal((3, 3, 3, 64, 64)) * 0.05
    x = {H: rng.standard_normal((1, 3, H, 8, 64)) for H in (8, 6, 5)}
    return w, x


@pytest.mark.parametrize("route,H", [("h4", 8), ("h2", 6), ("w", 5)])
def test_wino_conv_with_U64_is_the_plain_convolution(oracle, operands, route, H):
    """(1,3,8,8), (1,3,6,8), (1,3,5,8): the smallest grids of the three routes, both clamped faces and one interior plane.  Forward in clamp
    mode against conv3d_linear; zero mode with the dgrad stream against conv3d_dgrad on the strictly interior voxels (where the fold adds
    nothing).  1e-12 of the result's scale."""
    w, xs = operands
    x = xs[H]
    for stream in (route, "h4s") if route == "h4" else (route,):
        for direction, mode in (("fwd", "clamp"), ("dgrad", "zero")):
            vals = R.U64(w, stream, direction)
            if stream == "h4s":                                             # every piece slot carries its value: any one piece's slots
                U = R.dense(vals, stream)
                assert np.array_equal(U[..., 0], U[..., 1]) and np.array_equal(U[..., 0], U[..., 2])
                U = U[..., 0]
            else:
                U = R.dense(vals, stream)
            got = R.wino_conv(x, U, route, mode).numpy()
            if direction == "fwd":
                ref = oracle.conv3d_linear(x, w)
            else:
                ref = oracle.conv3d_dgrad(x, w, x.shape)
                got, ref = got[:, 1:-1, 1:-1, 1:-1], ref[:, 1:-1, 1:-1, 1:-1]
            assert ref.size and np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max(), (stream, direction)


def test_wino_conv_absolute_bounds_the_signed_result(operands):
    w, xs = operands
    U = R.dense(R.U64(w, "h4", "fwd"), "h4")
    y = R.wino_conv(xs[8], U, "h4", "clamp").numpy()
    ya = R.wino_conv(xs[8], U, "h4", "clamp", absolute=True).numpy()
    assert (np.abs(y) <= ya * (1 + 1e-12)).all() and ya.min() > 0


def test_round_f32_rounds_to_nearest_even():
    one, ulp = Fr(1), Fr(1, 2 ** 23)
    assert R.round_f32(one + ulp / 2) == np.float32(1.0)                        # tie: to even
    assert R.round_f32(one + 3 * ulp / 2) == np.float32(1.0) + np.float32(2.0 ** -22)
    assert R.round_f32(one + ulp / 2 + Fr(1, 2 ** 80)) == np.nextafter(np.float32(1), np.float32(2))
    assert R.round_f32(-(2 - ulp / 4)) == np.float32(-2.0)                      # carries into the next binade
    assert R.round_f32(Fr(1, 3)) == np.float32(1.0 / 3.0) and R.round_f32(Fr(0)) == 0
    for v in (0.1, -7.3e-30, 3.0e30):
        assert R.round_f32(Fr(float(np.float32(v)))) == np.float32(v)


@pytest.fixture(scope="module")
def kernel():
    return R.stream_test_kernel(5)


@pytest.mark.parametrize("direction", ["fwd", "dgrad"])
def test_float64_then_round_is_the_correctly_rounded_value(kernel, direction):
    """What the F(4,3) x F(4,3) pack does (form U in double, round once) against the exact rational value on 3000 slots: the same fp32 number,
    and float64's own error stays under 2^-20 of an fp32 ulp -- the slack the GPU test grants its float64 reference."""
    vals = R.U64(kernel, "h4", direction)
    at = np.random.default_rng(3).choice(vals.size, 3000, replace=False)
    exact = R.U_exact(kernel, "h4", direction, at)
    worst = 0.0
    for s, v in zip(at, exact):
        u = R.round_f32(v)
        assert np.float32(vals[s]) == u
        if v != 0:
            ulp = float(np.spacing(np.abs(u)))
            assert abs(Fr(float(vals[s])) - v) <= Fr(ulp) / 2 ** 20
            worst = max(worst, float(abs(Fr(float(u)) - v) / Fr(ulp)))
    assert 0.45 < worst <= 0.5


def _fma32(a, b, c):
    """fp32 fma of fp32 arrays: the product of two 24-bit significands is exact in float64; the sum is rounded to 53 bits and then to 24 (a
    double rounding that moves a result only when it lies within 2^-29 of a tie)."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


@pytest.mark.parametrize("direction", ["fwd", "dgrad"])
def test_fp32_fma_chains_stay_inside_the_stream_bounds(kernel, direction):
    """The 1-D and F(2,3) x F(4,3) packs are fp32 fma chains over fp32-rounded constants (conv64_pack.h).  Every term carries the rounding
    of its constant and of each fma it passes through: 1 + 3 roundings along W, 3 more fmas along H (Gh's entries are exact).  The GPU test
    allows 4 * 2^-24 sum|G||w| and 7 * 2^-24 sum|Gh||Gw||w|; the same arithmetic in numpy stays inside."""
    g = R.effective_kernel(kernel, direction).astype(np.float32)
    G = R.f64(R.transform("F43")[0]).astype(np.float32)
    H = R.f64(R.transform("F23")[0]).astype(np.float32)
    r = np.zeros((3, 3, 6, 64, 64), np.float32)                                   # [kd][kh][xw]
    for t in range(3):
        r = _fma32(G[None, None, :, t, None, None], g[:, :, None, t], r)
    e = np.abs(r.astype(np.float64) - R.dense_U64(kernel, "w", direction))
    mag = np.einsum("xt,abtkc->abxkc", np.abs(R.f64(R.transform("F43")[0])), np.abs(g.astype(np.float64)))
    assert (e <= 4 * 2.0 ** -24 * mag).all()
    v = np.zeros((4, 6, 3, 64, 64), np.float32)                                   # [xh][xw][kd]
    for kh in range(3):
        v = _fma32(H[:, None, None, kh, None, None], r[:, kh].transpose(1, 0, 2, 3)[None], v)
    e = np.abs(v.astype(np.float64) - R.dense_U64(kernel, "h2", direction))
    mag = np.einsum("hb,xt,abtkc->hxakc", np.abs(R.f64(R.transform("F23")[0])), np.abs(R.f64(R.transform("F43")[0])), np.abs(g.astype(np.float64)))
    assert (e <= 7 * 2.0 ** -24 * mag).all()


def test_bf16_split_is_exact_on_the_test_kernel(kernel):
    """u = hi + mid + lo exactly when each piece is the RNE bf16 of what the pieces before it leave (finite, normal u)."""
    u = R.U64(kernel, "h4", "fwd").astype(np.float32)
    hi = R.bf16_to_f32(R.bf16_rne_bits(u))
    r1 = u - hi
    mid = R.bf16_to_f32(R.bf16_rne_bits(r1))
    r2 = r1 - mid
    lo = R.bf16_to_f32(R.bf16_rne_bits(r2))
    assert np.array_equal(r1.astype(np.float64), u.astype(np.float64) - hi.astype(np.float64))       # the remainders are exact in fp32
    assert np.array_equal(hi.astype(np.float64) + mid.astype(np.float64) + lo.astype(np.float64), u.astype(np.float64))
    import torch
    assert np.array_equal(torch.from_numpy(u).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16), R.bf16_rne_bits(u))
