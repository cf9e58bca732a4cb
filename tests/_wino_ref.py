"""A float64 / rational model of the Winograd 64->64 convolutions and of their packed weight streams (host only; nothing from the package).

Transforms.  A Toom-Cook algorithm F(m,3) on n = m + 2 interpolation points p_0 .. p_{n-2}, inf is the identity

    A^T [(G g) (.) (B^T d)] = correlation(d, g),      y_i = sum_j d[i + j] g[j],  i < m, j < 3

G and A^T follow from the points (csrc/conv64_pack.h: G[k][j] = p_k^j / prod_{l != k} (p_k - p_l), last row (0,0,1); A^T = the Vandermonde
matrix of the points with the column (0,..,0,1) for inf); B^T is SOLVED from the identity in fractions.Fraction, for every unit g and d.
Nothing here is copied from kernel code.  Three of them:

    F43   F(4,3) on 0, +-1, +-2, inf        the 1-D stream, and the W axis of the F(2,3) x F(4,3) stream
    F43s  F(4,3) on 0, +-3/4, +-3/2, inf    both axes of the F(4,3) x F(4,3) stream
    F23   F(2,3) on 0, +-1, inf             the H axis of the F(2,3) x F(4,3) stream.  conv64_pack.h's Gh has Lavin & Gray's row (1,0,0) for the
                                            point 0 where the formula gives (-1,0,0): a row of G may carry any factor that the same row of
                                            B^T undoes, and the solve puts it there.

Streams.  A pack (include/fdn.h: FDN_CONV64_PACK_FLOATS = 423 * 4096 floats) holds five streams; LAYOUT spells each one's index order as the
layout comments of csrc/conv64_pack.h give it (slowest index first), and the bf16 operand stream of fdn_pack_conv64_weights_bf16 from the
comment above pack_conv64_bf16_kernel (csrc/conv64_bf16.hip).  decode(stream) maps every slot to its coordinates, encode(stream, ...) back.
Coordinates are those of the DIRECTION's own convolution: k = the contracted channel, c = the produced one, taps (kd, kh, kw) in the order
that convolution applies them; effective_kernel(w, direction) is the kernel it applies (dgrad: taps flipped, channels transposed).

Values.  U64(w, stream, direction) is the float64 value of every slot, U_exact(...) the exact Fraction of sampled ones, round_f32 the
correctly rounded fp32 number of a Fraction.

Model.  wino_conv(x, U, route, mode) is the Winograd-domain convolution in float64 of a dense stream U (dense(values, stream) scatters a
decoded DEVICE stream): with U64 it is the plain convolution up to float64 rounding, with a device stream it shows what that stream's
rounding alone does to the result.  Tiles start at voxel 0 as the kernels' do (the forward's output box, the inner box of the fused dgrad).
mode "clamp" = edge-replicated input (forward), "zero" = zero outside (the inner box of the fused dgrad: the full correlation of dz)."""
from fractions import Fraction as Fr
import math

import numpy as np
import torch

INF = "inf"
POINTS = {"F43": (Fr(0), Fr(1), Fr(-1), Fr(2), Fr(-2), INF),
          "F43s": (Fr(0), Fr(3, 4), Fr(-3, 4), Fr(3, 2), Fr(-3, 2), INF),
          "F23": (Fr(0), Fr(1), Fr(-1), INF)}
ROW_FACTOR = {"F23": (Fr(-1), Fr(1), Fr(1), Fr(1))}
R = 3


def _solve(M, rhs):
    """The solution of the consistent over-determined system M b = rhs, in Fractions (Gauss-Jordan; asserts consistency and full rank)."""
    rows = [list(r) + [v] for r, v in zip(M, rhs)]
    n = len(M[0])
    piv = 0
    for col in range(n):
        p = next(i for i in range(piv, len(rows)) if rows[i][col] != 0)      # StopIteration = rank deficient
        rows[piv], rows[p] = rows[p], rows[piv]
        rows[piv] = [v / rows[piv][col] for v in rows[piv]]
        for i in range(len(rows)):
            if i != piv and rows[i][col] != 0:
                f = rows[i][col]
                rows[i] = [a - f * b for a, b in zip(rows[i], rows[piv])]
        piv += 1
    assert all(v == 0 for r in rows[n:] for v in r), "the identity has no solution"
    return [rows[i][n] for i in range(n)]


def make_transform(name):
    """(G, Bt, At) of POINTS[name] as lists of lists of Fractions: G n x 3, Bt n x n, At m x n."""
    pts = POINTS[name]
    n = len(pts)
    m = n - R + 1
    fin = pts[:-1]
    fac = ROW_FACTOR.get(name, (Fr(1),) * n)
    G = []
    for k, p in enumerate(fin):
        den = Fr(1)
        for l, q in enumerate(fin):
            if l != k:
                den *= p - q
        G.append([fac[k] * p ** j / den for j in range(R)])
    G.append([Fr(0)] * (R - 1) + [fac[n - 1]])
    At = [[p ** i for p in fin] + [Fr(1 if i == m - 1 else 0)] for i in range(m)]
    # A^T[i][k] G[k][j] B^T[k][e] summed over k = [e == i + j], for every output i, tap j and input position e
    M = [[At[i][k] * G[k][j] for k in range(n)] for i in range(m) for j in range(R)]
    cols = [_solve(M, [Fr(1 if e == i + j else 0) for i in range(m) for j in range(R)]) for e in range(n)]
    Bt = [[cols[e][k] for e in range(n)] for k in range(n)]
    return G, Bt, At


_TRANSFORMS = {}


def transform(name):
    if name not in _TRANSFORMS:
        _TRANSFORMS[name] = make_transform(name)
    return _TRANSFORMS[name]


def f64(mat):
    """A Fraction matrix as float64 (each entry correctly rounded)."""
    return np.asarray([[float(v) for v in row] for row in mat], np.float64)


def identity_residual(name):
    """max |A^T[(G g) (.) (B^T d)] - correlation(d, g)| over all unit g, d: a Fraction, zero when the identity holds exactly."""
    G, Bt, At = transform(name)
    n, m = len(G), len(At)
    worst = Fr(0)
    for j in range(R):
        for e in range(n):
            for i in range(m):
                y = sum(At[i][k] * G[k][j] * Bt[k][e] for k in range(n))
                worst = max(worst, abs(y - (1 if e == i + j else 0)))
    return worst


# ------------------------------------------------------------------------------------------------------------------------------------
# streams
# ------------------------------------------------------------------------------------------------------------------------------------
UNIT = 64 * 64
# offset and size of each stream inside a pack, in floats (the bf16 x 3 stream: three 2-byte pieces per value in 162 * 4096 float-sized slots)
STREAMS = {"direct": (0 * UNIT, 27 * UNIT), "w": (27 * UNIT, 54 * UNIT), "h2": (81 * UNIT, 72 * UNIT), "h4": (153 * UNIT, 108 * UNIT),
           "h4s": (261 * UNIT, 162 * UNIT)}
PACK_FLOATS = 423 * UNIT
STREAM_BIT = {"direct": 1, "w": 2, "h2": 4, "h4": 8, "h4s": 16}
# index order, slowest first: (name, extent)
LAYOUT = {
    "direct": (("half", 2), ("tap", 27), ("g", 4), ("kh", 2), ("j", 64), ("s", 4)),
    "w": (("half", 2), ("kd", 3), ("kh3", 3), ("xw", 6), ("g", 4), ("kh", 2), ("j", 64), ("s", 4)),
    "h2": (("nb", 4), ("xh", 4), ("kd", 3), ("xw", 6), ("g", 4), ("q", 4), ("i", 16), ("s", 4)),
    "h4": (("nb", 4), ("xh", 6), ("kd", 3), ("xw", 6), ("g", 4), ("q", 4), ("i", 16), ("s", 4)),
    "h4s": (("nb", 4), ("xh", 6), ("pass", 2), ("kd", 3), ("xw", 6), ("piece", 3), ("q", 4), ("i", 16), ("j8", 8)),
    "bf16": (("slice", 4), ("bc", 9), ("a", 3), ("kh", 2), ("row", 64), ("k8", 8)),
}
# the coordinates of each stream, in the order dense() lays them out
COORDS = {"direct": ("tap", "k", "c"), "w": ("kd", "kh3", "xw", "k", "c"), "h2": ("xh", "xw", "kd", "k", "c"),
          "h4": ("xh", "xw", "kd", "k", "c"), "h4s": ("xh", "xw", "kd", "k", "c", "piece"), "bf16": ("tap", "k", "c")}
EXTENT = {"tap": 27, "k": 64, "c": 64, "kd": 3, "kh3": 3, "piece": 3}


def slots(stream):
    return int(np.prod([e for _, e in LAYOUT[stream]]))


def extent(stream, coord):
    return EXTENT.get(coord) or dict(LAYOUT[stream])[coord]


def _row_channel(j):
    """c(j): row j of a 32-row MFMA tile lands in accumulator register (i & 3) + 4 (i >> 3) of lane half (i >> 2) & 1, i = j & 31."""
    return (j & 32) + 16 * ((j >> 2) & 1) + (j & 3) + 4 * ((j & 31) >> 3)


def _channel_row(c):
    return (c & 32) + 8 * ((c >> 2) & 3) + 4 * ((c >> 4) & 1) + (c & 3)


def decode(stream, direction=None):
    """{coordinate: int array over the stream's slots}, plus "sign" (-1 where the stored value is the negated one).  With a direction also
    the LAYER's channels and depth tap behind the direction's own: "cin", "cout", "layer_kd" (dgrad: c, k and the flipped tap), and for the
    streams that copy weights "layer_tap"."""
    n = slots(stream)
    rest = np.arange(n, dtype=np.int64)
    f = {}
    for name, ext in reversed(LAYOUT[stream]):
        f[name] = rest % ext
        rest = rest // ext
    assert not rest.any()
    out = {"sign": np.ones(n, np.int64)}
    if stream in ("direct", "w"):
        out["k"] = 32 * f["half"] + 8 * f["g"] + 4 * f["kh"] + f["s"]
        out["c"] = _row_channel(f["j"])
    elif stream in ("h2", "h4"):
        out["k"] = 16 * f["g"] + 4 * f["q"] + f["s"]
        out["c"] = 16 * f["nb"] + f["i"]
    elif stream == "h4s":
        out["k"] = 32 * f["pass"] + 8 * f["q"] + f["j8"]
        out["c"] = 16 * f["nb"] + f["i"]
    else:
        out["k"] = 16 * f["slice"] + 8 * f["kh"] + f["k8"]
        out["c"] = _row_channel(f["row"])
        out["tap"] = 9 * f["a"] + f["bc"]
    for name in COORDS[stream]:
        if name not in out:
            out[name] = f[name]
    if stream == "h2":
        out["sign"] = np.where(out["xh"] == 2, -1, 1)
    if direction is not None:
        flip = direction == "dgrad"
        assert flip or direction == "fwd"
        out["cin"], out["cout"] = (out["c"], out["k"]) if flip else (out["k"], out["c"])
        if "tap" in out:
            out["layer_tap"] = 26 - out["tap"] if flip else out["tap"]
        else:
            out["layer_kd"] = 2 - out["kd"] if flip else out["kd"]
    return out


def encode(stream, **co):
    """The slot of given coordinates (arrays or ints): the layout's index formula, written out."""
    k, c = np.asarray(co["k"]), np.asarray(co["c"])
    if stream == "direct":
        return ((((k >> 5) * 27 + co["tap"]) * 4 + ((k >> 3) & 3)) * 2 + ((k >> 2) & 1)) * 256 + _channel_row(c) * 4 + (k & 3)
    if stream == "w":
        vt = (np.asarray(co["kd"]) * 3 + co["kh3"]) * 6 + co["xw"]
        return ((((k >> 5) * 54 + vt) * 4 + ((k >> 3) & 3)) * 2 + ((k >> 2) & 1)) * 256 + _channel_row(c) * 4 + (k & 3)
    if stream in ("h2", "h4"):
        nh = extent(stream, "xh")
        unit = (((c >> 4) * nh + co["xh"]) * 3 + co["kd"]) * 6 + co["xw"]
        return unit * 1024 + (k >> 4) * 256 + ((k >> 2) & 3) * 64 + (c & 15) * 4 + (k & 3)
    if stream == "h4s":
        unit = ((((c >> 4) * 6 + co["xh"]) * 2 + (k >> 5)) * 3 + co["kd"]) * 6 + co["xw"]
        return unit * 1536 + np.asarray(co["piece"]) * 512 + ((k >> 3) & 3) * 128 + (c & 15) * 8 + (k & 7)
    tap = np.asarray(co["tap"])
    return (((((k >> 4) * 9 + tap % 9) * 3 + tap // 9) * 2 + ((k >> 3) & 1)) * 64 + _channel_row(c)) * 8 + (k & 7)


def effective_kernel(w, direction):
    """(3,3,3,k,c): the kernel the direction's convolution applies.  fwd: the Keras kernel (k = cin, c = cout); dgrad: taps flipped and
    channels transposed (k = the layer's cout, c = its cin)."""
    w = np.asarray(w).reshape(3, 3, 3, 64, 64)
    if direction == "fwd":
        return w
    assert direction == "dgrad"
    return np.ascontiguousarray(w[::-1, ::-1, ::-1].transpose(0, 1, 2, 4, 3))


def source_index(stream, direction):
    """For the streams that copy weights (direct, bf16): the flat index into the Keras kernel (27,64,64) each slot holds."""
    d = decode(stream)
    if direction == "fwd":
        return (d["tap"] * 64 + d["k"]) * 64 + d["c"]
    return ((26 - d["tap"]) * 64 + d["c"]) * 64 + d["k"]


_AXES = {"w": (None, "F43"), "h2": ("F23", "F43"), "h4": ("F43s", "F43s"), "h4s": ("F43s", "F43s")}


def _int_form(G):
    """(L G as an exact float64 integer matrix, L), L the common denominator of G's entries."""
    L = 1
    for row in G:
        for v in row:
            L = L * Fr(v).denominator // math.gcd(L, Fr(v).denominator)
    return np.asarray([[float(Fr(v) * L) for v in row] for row in G], np.float64), float(L)


def _sum2(terms):
    """Compensated sum (Ogita, Rump & Oishi's Sum2): as accurate as a sum carried in twice the precision, then rounded."""
    s, comp = terms[0], 0.0
    for p in terms[1:]:
        t = s + p
        z = t - s
        comp = comp + ((s - (t - z)) + (p - z))
        s = t
    return s + comp


def dense_U64(w, stream, direction):
    """The float64 stream in dense coordinate order (COORDS[stream] without piece), signs NOT applied: U = Gh g Gw^T per (kd, k, c).
    A Winograd-domain value is a CANCELLING sum (|U| can be 1e-4 of sum |Gh||Gw||g|), and a plain float64 sum is good to 2^-53 of the latter
    only.  So: L G is an integer matrix, an integer of <= 16 bits times an fp32 weight is exact in float64, the exact terms are summed with
    compensation, and the one division by L rounds once -- U64 is within an ulp or two of float64 of the VALUE, 2^-28 of an fp32 ulp."""
    g = effective_kernel(np.asarray(w, np.float64), direction)          # (exactness as described: for fp32 weights)
    if stream == "direct":
        return g.reshape(27, 64, 64)
    th, tw = _AXES[stream]
    Gw, Lw = _int_form(transform(tw)[0])
    if th is None:
        return _sum2([Gw[:, t][None, None, :, None, None] * g[:, :, None, t] for t in range(3)]) / Lw          # [kd][kh][xw][k][c]
    Gh, Lh = _int_form(transform(th)[0])
    terms = [(Gh[:, b][:, None, None, None, None] * Gw[:, t][None, :, None, None, None]) * g[:, b, t][None, None]
             for b in range(3) for t in range(3)]
    return _sum2(terms) / (Lh * Lw)                                                                           # [xh][xw][kd][k][c]


def _gather(densearr, stream, d):
    names = [n for n in COORDS[stream] if n != "piece"]
    return densearr[tuple(d[n] for n in names)]


def U64(w, stream, direction):
    """float64 value of every slot of the stream as the device stores it (the negated F(2,3) row included; bf16 x 3: the value whose pieces
    the slot belongs to)."""
    d = decode(stream)
    return _gather(dense_U64(w, stream, direction), stream, d) * d["sign"]


def magnitude64(w, stream, direction):
    """sum |Gh||Gw||g| of every slot: the scale of the fp32 streams' rounding bounds."""
    g = np.abs(effective_kernel(np.asarray(w, np.float64), direction))
    th, tw = _AXES[stream]
    Gw = np.abs(f64(transform(tw)[0]))
    if th is None:
        m = np.einsum("xt,abtkc->abxkc", Gw, g)
    else:
        m = np.einsum("hb,xt,abtkc->hxakc", np.abs(f64(transform(th)[0])), Gw, g)
    return _gather(m, stream, decode(stream))


def U_exact(w, stream, direction, at):
    """Exact Fractions of the slots `at` (fp32 weights are rationals)."""
    g = effective_kernel(np.asarray(w, np.float32), direction)
    d = decode(stream)
    th, tw = _AXES[stream]
    Gw = transform(tw)[0]
    Gh = transform(th)[0] if th else None
    out = []
    for s in at:
        kd, k, c, xw = int(d["kd"][s]), int(d["k"][s]), int(d["c"][s]), int(d["xw"][s])
        if Gh is None:
            v = sum(Gw[xw][t] * Fr(float(g[kd, int(d["kh3"][s]), t, k, c])) for t in range(3))
        else:
            xh = int(d["xh"][s])
            v = sum(Gh[xh][b] * Gw[xw][t] * Fr(float(g[kd, b, t, k, c])) for b in range(3) for t in range(3))
        out.append(v * int(d["sign"][s]))
    return out


def round_f32(v):
    """The fp32 number nearest to the Fraction v, ties to even (normal range), as np.float32."""
    if v == 0:
        return np.float32(0.0)
    a = abs(v)
    e = a.numerator.bit_length() - a.denominator.bit_length()
    if Fr(2) ** e > a:
        e -= 1
    assert Fr(2) ** e <= a < Fr(2) ** (e + 1) and -126 <= e <= 127
    q = a / Fr(2) ** (e - 23)
    n = q.numerator // q.denominator
    rem = q - n
    if rem > Fr(1, 2) or (rem == Fr(1, 2) and (n & 1)):
        n += 1
    r = np.float32(math.ldexp(n, e - 23))
    return -r if v < 0 else r


def bf16_rne_bits(x):
    """Round-to-nearest-even bf16 bit patterns (uint16) of finite fp32 numbers, by integer arithmetic on the bit pattern."""
    b = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return ((b + 0x7FFF + ((b >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_to_f32(bits):
    return (np.asarray(bits, np.uint16).astype(np.uint32) << 16).view(np.float32)


def stream_test_kernel(seed):
    """The Keras kernel (27,64,64) fp32 of the stream tests: N(0, 0.05), with the columns (cin < 8, cout < 16) replaced by exact values --
    +-0, powers of two from 2^-100 to 2^100 (equal over a column's 27 taps, stepping by tap, and both extremes inside one column), values
    one ulp apart (around ordinary numbers and around a power of two), and all-equal columns.  No subnormal, infinite or NaN weight, and
    no stream value leaves fp32's normal range."""
    rng = np.random.default_rng(seed)
    w = (rng.standard_normal((27, 64, 64)) * 0.05).astype(np.float32)
    t = np.arange(27)
    one = np.float32(1.0)
    expo = [-100, -80, -60, -40, -20, -10, -1, 0, 1, 10, 20, 40, 60, 80, 100, 3]
    for c in range(16):
        w[:, 0, c] = np.where((t + c) & 1 if c >= 8 else c & 1, np.float32(0.0), np.float32(-0.0))
        w[:, 1, c] = np.float32(2.0) ** expo[c]
        w[:, 2, c] = np.where(t & 1, -1.0, 1.0).astype(np.float32) * np.float32(2.0) ** (expo[c] // 2 + (t % 3) - (t // 9))
        w[:, 3, c] = np.where((t + c) % 3 == 0, np.float32(2.0) ** 100, np.float32(2.0) ** -100)
        base = np.float32(w[0, 4, c]) if c & 1 else np.float32(1.0 + c / 16.0)
        near = np.stack([base, np.nextafter(base, np.float32(np.inf)), np.nextafter(base, np.float32(-np.inf))])
        w[:, 4, c] = near[(t + c) % 3]
        w[:, 5, c] = w[0, 5, c]
        p2 = np.float32(2.0) ** (c - 8)
        near = np.stack([p2, np.nextafter(p2, np.float32(np.inf)), np.nextafter(p2, np.float32(0.0))])
        w[:, 6, c] = near[(t // 3 + c) % 3] * (one if c & 2 else -one)
        w[:, 7, c] = np.where(t % 3 == 1, w[0, 7, c], np.float32(0.0))
    assert np.isfinite(w).all() and (np.abs(w[w != 0]) >= 2.0 ** -101).all()
    return w


def dense(values, stream):
    """A decoded stream in dense coordinate order, float64, with the stored signs taken out: values[slot] -> U[COORDS[stream]]."""
    d = decode(stream)
    names = COORDS[stream]
    out = np.zeros([extent(stream, n) for n in names], np.float64)
    out[tuple(d[n] for n in names)] = np.asarray(values, np.float64) * d["sign"]
    return out


# ------------------------------------------------------------------------------------------------------------------------------------
# the convolution in the Winograd domain
# ------------------------------------------------------------------------------------------------------------------------------------
ROUTES = {"h4": ("F43s", "F43s"), "h2": ("F23", "F43"), "w": (None, "F43")}


def pad1(x, mode):
    if mode == "zero":
        return torch.nn.functional.pad(x, (0, 0, 1, 1, 1, 1, 1, 1))
    assert mode == "clamp"
    for ax in (1, 2, 3):
        n = x.shape[ax]
        x = torch.cat([x.narrow(ax, 0, 1), x, x.narrow(ax, n - 1, 1)], dim=ax)
    return x


def wino_conv(x, U, route, mode, absolute=False):
    """y (N,D,H,W,64) float64 = the route's Winograd algorithm on x (N,D,H,W,64) with the dense stream U (h4 / h2: [xh][xw][kd][k][c],
    w: [kd][kh][xw][k][c]); torch, on x's device.  absolute: A^T, U and the transformed input B^T x B by their absolute values -- the
    scale sum |A^T| (|U| (.) |B^T x|) |A| that a relative perturbation of U's elements is measured against."""
    th, tw = ROUTES[route]
    x = torch.as_tensor(x).to(torch.float64)
    dev = x.device
    t = lambda a: torch.as_tensor(np.abs(a) if absolute else a, dtype=torch.float64, device=dev)
    U = torch.as_tensor(U, dtype=torch.float64, device=dev)
    if absolute:
        U = U.abs()
    N, D, H, W, _ = x.shape
    _, Btw, Atw = transform(tw)
    assert W % 4 == 0
    xp = pad1(x, mode)                                                     # (N, D+2, H+2, W+2, C)
    if th is None:
        tiles = xp.unfold(3, 6, 4)                                          # (N, D+2, H+2, ntw, C, 6)
        V = torch.einsum("xe,ndhtke->ndhtxk", torch.as_tensor(f64(Btw), device=dev), tiles)
        if absolute:
            V = V.abs()
        M = 0
        for kd in range(3):
            for kh in range(3):
                M = M + torch.einsum("ndhtxk,xkc->ndhtxc", V[:, kd:kd + D, kh:kh + H], U[kd, kh])
        Y = torch.einsum("ix,ndhtxc->ndhtic", t(f64(Atw)), M)
        return Y.reshape(N, D, H, W, 64)
    _, Bth, Ath = transform(th)
    mh = len(Ath)
    assert H % mh == 0
    tiles = xp.unfold(2, mh + 2, mh).unfold(3, 6, 4)                        # (N, D+2, nth, ntw, C, mh+2, 6)
    V = torch.einsum("af,xe,ndstkfe->ndstaxk", torch.as_tensor(f64(Bth), device=dev), torch.as_tensor(f64(Btw), device=dev), tiles)
    if absolute:
        V = V.abs()
    M = 0
    for kd in range(3):
        M = M + torch.einsum("ndstaxk,axkc->ndstaxc", V[:, kd:kd + D], U[:, :, kd])
    Y = torch.einsum("ia,jx,ndstaxc->ndsitjc", t(f64(Ath)), t(f64(Atw)), M)
    return Y.reshape(N, D, H, W, 64)
