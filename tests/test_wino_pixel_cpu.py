"""A CPU model of the pixel form of the fp32 Winograd DecoderBlock kernel (conv_wino_f32.hip, PIX = true): conv3x3(pad 1) over the
nearest-x2 upsample, with GEMM rows = SOURCE pixels.  Per source pixel, the 3x3 patch around it (zeros outside the image) goes through
the tile form's input transform [d0 - d1, d1, d2 - d1] along each axis; position (r, c) is multiplied with slab
[2 (r == 2) + (c == 2)][3 r + c] of the tile form's packed filters U = G g G^T [4][9][Cout][Cin]; output parity (u, v) of the pixel is
(M[u][v] + M[u][v + 1]) + (M[u + 1][v] + M[u + 1][v + 1]) and goes to (2 y + u, 2 x + v).  Pins that mapping without a GPU: float64
against conv2d(interpolate) to rounding, fp32 within the GPU tests' bound (2e-5 of the reference's largest element)."""

import pytest
import torch
import torch.nn.functional as F


def _pack_wino(w):
    """w [Cout, 3, 3, Cin] -> U [4][9][Cout][Cin] as rs_pack_phase_weight + rs_pack_wino_phase_weight produce it: the phase taps of parity
    p along an axis are (w0, w1 + w2) for p = 0 and (w0 + w1, w2) for p = 1; U = G g G^T, G = [1 0; 1 1; 0 1]."""
    def taps(p, t):  # t [.., 3, ..] along dim 0 -> the two phase taps
        return (t[0], t[1] + t[2]) if p == 0 else (t[0] + t[1], t[2])

    wy = w.permute(1, 2, 0, 3)  # [3][3][Cout][Cin]
    u = []
    for py in (0, 1):
        for px in (0, 1):
            gy = taps(py, wy)  # 2 x [3][Cout][Cin]
            g = [taps(px, gy[0]), taps(px, gy[1])]  # g[r][s] [Cout][Cin]
            g00, g01, g10, g11 = g[0][0], g[0][1], g[1][0], g[1][1]
            u.append(torch.stack([g00, g00 + g01, g01, g00 + g10, (g00 + g01) + (g10 + g11), g01 + g11, g10, g10 + g11, g11]))
    return torch.stack(u)


def _slab(r, c):
    return 2 * int(r == 2) + int(c == 2)


def _pixel_form(x, u, slab=_slab):
    """x [N, C, H, W], u [4][9][Cout][C] -> [N, Cout, 2 H, 2 W] in x's dtype."""
    n, _, h, w = x.shape
    xp = F.pad(x, (1, 1, 1, 1))
    d = [[xp[:, :, r:r + h, c:c + w] for c in range(3)] for r in range(3)]
    t = [[d[r][0] - d[r][1], d[r][1], d[r][2] - d[r][1]] for r in range(3)]  # along x
    v = [[t[0][c] - t[1][c] for c in range(3)], [t[1][c] for c in range(3)], [t[2][c] - t[1][c] for c in range(3)]]  # along y
    m = [[torch.einsum("nchw,oc->nohw", v[r][c], u[slab(r, c)][3 * r + c]) for c in range(3)] for r in range(3)]
    out = x.new_zeros(n, u.shape[2], 2 * h, 2 * w)
    for a in (0, 1):
        for b in (0, 1):
            out[:, :, a::2, b::2] = (m[a][b] + m[a][b + 1]) + (m[a + 1][b] + m[a + 1][b + 1])
    return out


def _case(h, w, cin, cout, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(2, cin, h, w, generator=g, dtype=torch.float64)
    wk = torch.randn(cout, 3, 3, cin, generator=g, dtype=torch.float64) * (2.0 / (9 * cin)) ** 0.5
    ref = F.conv2d(F.interpolate(x, scale_factor=2, mode="nearest"), wk.permute(0, 3, 1, 2), padding=1)
    return x, wk, ref


@pytest.mark.parametrize("h,w", [(12, 10), (15, 17), (1, 1), (8, 9)])
def test_pixel_form_float64_matches_the_reference(h, w):
    x, wk, ref = _case(h, w, 24, 8, 3)
    got = _pixel_form(x, _pack_wino(wk))
    assert float((got - ref).abs().max()) <= 1e-13 * max(1.0, float(ref.abs().max()))


@pytest.mark.parametrize("h,w", [(12, 10), (15, 17)])
def test_pixel_form_fp32_within_the_gpu_bound(h, w):
    x, wk, ref = _case(h, w, 320, 16, 4)
    got = _pixel_form(x.float(), _pack_wino(wk.float()))
    assert got.dtype == torch.float32
    err = float((got.double() - ref).abs().max())
    assert err <= 2e-5 * max(1.0, float(ref.abs().max())), err


def test_slab_mapping_is_the_only_one_of_its_kind():
    """Positions 0 / 2 along an axis need parity 0's / parity 1's filters (w0 resp. w2); position 1 is the same in both.  Any other slab
    for a position with r or c != 1 is off by whole taps, far outside rounding."""
    x, wk, ref = _case(6, 7, 16, 4, 5)
    u = _pack_wino(wk)
    scale = float(ref.abs().max())
    for r in range(3):
        for c in range(3):
            for s in range(4):
                def slab(rr, cc):
                    return s if (rr, cc) == (r, c) else _slab(rr, cc)
                err = float((_pixel_form(x, u, slab) - ref).abs().max())
                same = (r == 1 or (s >> 1) == int(r == 2)) and (c == 1 or (s & 1) == int(c == 2))
                assert (err <= 1e-13 * scale) == same, (r, c, s, err)
