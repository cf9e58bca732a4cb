"""Float64 reference of the three 64 -> 1 head operations, in plain torch on whatever device the operands live on.

Elementary operations only (pad, slice, broadcast multiply-add, matmul) and nothing from the package, so that on the GPU it scales to the
10^6-voxel grids where the numpy oracle takes minutes.  tests/test_head_ref.py holds every function here to oracle/flownet_oracle.py at
1e-12 of scale; that is what licenses using them as the reference of tests/test_gpu_head_walks.py and of the head cases of
tests/test_gpu_plan_coverage.py.

With one output channel the edge-clamped 3x3x3 convolution factors (csrc/heads_mfma.hip) into a per-voxel product with the 27 x 64 weight
matrix and a 27-point stencil on scalars; tap t = (a, b, c) = 9 a + 3 b + c reads the input at clamp(o + t - 1):
    forward : y[o]     = b + sum_t x[clamp(o + t - 1)] . w[t]
    backward: A[i][t]  = sum_{o : clamp(o + t - 1) = i} dz[o]          (MirrorPadGrad on scalars)
              dx[i][c] = sum_t A[i][t] w[t][c]          dW[t][c] = sum_i A[i][t] x[i][c]"""
import torch

F64 = torch.float64


def edge_pad(z, dim):
    """One replicated element on both sides of `dim`."""
    L = z.shape[dim]
    return torch.cat([z.narrow(dim, 0, 1), z, z.narrow(dim, L - 1, 1)], dim)


def _scatter_axis(z, dim):
    """[out_0, out_1, out_2], out_t[i] = sum of z[o] over the o with clamp(o + t - 1, 0, L - 1) == i along `dim`: z is written at offset
    t - 1 into a zero-padded axis of L + 2 elements, whose two halo elements are then added onto the edge elements."""
    L = z.shape[dim]
    pad = [0] * (2 * z.dim())
    pad[2 * (z.dim() - 1 - dim)] = pad[2 * (z.dim() - 1 - dim) + 1] = 2
    zp = torch.nn.functional.pad(z, pad)                    # z[o] at index o + 2
    outs = []
    for t in range(3):
        P = zp.narrow(dim, 2 - t, L + 2)                    # P[p] = z[p - t]: the padded position (index + 1) of o + t - 1
        out = P.narrow(dim, 1, L).clone()
        out.narrow(dim, 0, 1).add_(P.narrow(dim, 0, 1))
        out.narrow(dim, L - 1, 1).add_(P.narrow(dim, L + 1, 1))
        outs.append(out)
    return outs


def head_fold(dz, dims):
    """A (N,D,H,W,27) float64: the scalar gradient dz (N*D*H*W values) scattered over the edge-clamped 3x3x3 neighbourhood."""
    z = dz.reshape(dims).to(F64)
    taps = [zc for za in _scatter_axis(z, 1) for zb in _scatter_axis(za, 2) for zc in _scatter_axis(zb, 3)]
    return torch.stack(taps, dim=-1)


def head_fwd_ref(x, w, b=None):
    """x (N,D,H,W,64), w (3,3,3,64,1), b (1,) or None -> y (N,D,H,W) float64."""
    N, D, H, W = x.shape[:4]
    z = torch.matmul(x.to(F64), w.reshape(27, 64).to(F64).t())          # z[v][t] = x[v] . w[t]
    zp = edge_pad(edge_pad(edge_pad(z, 1), 2), 3)                      # zp[q] = z[clamp(q - 1)]
    y = torch.zeros((N, D, H, W), dtype=F64, device=x.device)
    if b is not None:
        y += b.reshape(-1)[0].to(F64)
    for a in range(3):
        for bb in range(3):
            for c in range(3):
                y += zp[:, a:a + D, bb:bb + H, c:c + W, (a * 3 + bb) * 3 + c]
    return y


def head_dgrad_ref(dz, w, dims):
    """dz: N*D*H*W scalars, w (3,3,3,64,1) -> dx (N,D,H,W,64) float64; the act' factor is the caller's."""
    return torch.matmul(head_fold(dz, dims), w.reshape(27, 64).to(F64))


def _wgrad(x, dz):
    N, D, H, W = x.shape[:4]
    dw = torch.zeros((27, 64), dtype=F64, device=x.device)
    for n in range(N):                                                    # (per sample: one float64 copy of a sample's rows at a time)
        A = head_fold(dz.reshape(N, D, H, W)[n:n + 1], (1, D, H, W)).reshape(-1, 27)
        dw += torch.matmul(A.t(), x[n].reshape(-1, 64).to(F64))
    return dw.reshape(3, 3, 3, 64, 1)


def head_wgrad_ref(x, dz):
    """x (N,D,H,W,64), dz: N*D*H*W scalars -> dW (3,3,3,64,1) float64."""
    return _wgrad(x, dz)


def head_wgrad_bound(x, dz):
    """sum |x||dz| over the terms of every dW element: what any summation order of the fp32 products obeys to a few ulp."""
    return _wgrad(x.abs(), dz.abs())
