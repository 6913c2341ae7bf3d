// The clDice topology loss (Shit et al., CVPR 2021) and its soft skeleton: rs_soft_skeleton_* and rs_cldice_* in
// include/robosat_hip.h, DESIGN.md section 7j.
//
//   E_0 = X, E_{k+1} = erode(E_k), O_k = dilate(E_{k+1}), D_k = relu(E_k - O_k), k = 0 .. iters
//   S_0 = D_0, S_k = S_{k-1} + relu(D_k - S_{k-1} * D_k), S = S_iters
//   erode = min(min over N C S, min over W C E), dilate = max over the 3x3 square; nothing lies beyond the plane's edge
//
// Forward: iters + 2 launches.  Launch j reads E_j (and E_{j-1}, S_{j-2} at the thread's own pixel), writes E_{j+1} and S_{j-1}: no
// launch reads a neighbour that a block of the same launch writes.  Every subtraction, product and sum of the skeleton is one rounded
// fp32 operation (__fsub_rn, __fmul_rn, __fadd_rn: no contraction), so the forward equals the op-by-op evaluation bit for bit.
// Backward: one launch for the pixel-local chain through the S updates (it leaves G_k = dL/dD_k * relu'(E_k - O_k) per level), then
// iters + 2 launches in gather form, level iters + 1 down to 0: every cell of E_k collects from the at most 9 dilation windows and
// the at most 5 erosions that selected it, the selections recomputed from E_k by the tie rules.  No atomics anywhere: the same input
// gives the same bits in every run.  Nothing is read back and nothing allocated: every call can be captured into a graph.
#include "common.h"

namespace {

constexpr int kSkMaxIters = 64;
constexpr int kSkTileW = 64, kSkTileH = 4;  // a block's pixels: one wave per row of 64
constexpr int kCdMaxC = 8;
constexpr int kCdBlocks = 64;  // per plane, as rs_tversky_sums

struct SkPixel {
  long i;  // index of the pixel in the [M][H][W] array
  int y, x;
  bool live;
};

// blockIdx.x = (plane * tilesY + tileY) * tilesX + tileX
__device__ __forceinline__ SkPixel sk_pixel(int H, int W, int tilesX, int tilesY) {
  const unsigned b = blockIdx.x;  // (the grid has fewer than 2^31 blocks: sk_shape_ok)
  const unsigned row = b / (unsigned)tilesX;
  const int tx = (int)(b - row * (unsigned)tilesX);
  const long m = row / (unsigned)tilesY;
  const int ty = (int)(row - (unsigned)m * (unsigned)tilesY);
  SkPixel p;
  p.y = ty * kSkTileH + (int)(threadIdx.x >> 6);
  p.x = tx * kSkTileW + (int)(threadIdx.x & 63);
  p.live = p.y < H && p.x < W;
  p.i = (m * H + p.y) * W + p.x;
  return p;
}

__device__ __forceinline__ float sk_relu(float v) { return v > 0.f ? v : 0.f; }

// max over the 3x3 square of `E` around the pixel, cells outside the plane left out
__device__ __forceinline__ float sk_dilate(const float* __restrict__ E, const SkPixel& p, int H, int W) {
  float o = E[p.i];
#pragma unroll
  for (int dy = -1; dy <= 1; ++dy) {
    if (p.y + dy < 0 || p.y + dy >= H) continue;
#pragma unroll
    for (int dx = -1; dx <= 1; ++dx) {
      if (p.x + dx < 0 || p.x + dx >= W) continue;
      o = fmaxf(o, E[p.i + (long)dy * W + dx]);
    }
  }
  return o;
}

// Launch j of the forward.  Ej = E_j; Enext = E_{j+1} (null in the last launch); for j >= 1 also S_{j-1} from Eprev = E_{j-1} and
// Sprev = S_{j-2} (null for j = 1: S_0 = D_0).
__global__ __launch_bounds__(256) void skel_fwd_kernel(const float* __restrict__ Ej, const float* __restrict__ Eprev,
                                                       const float* __restrict__ Sprev, float* __restrict__ Enext,
                                                       float* __restrict__ Sout, int H, int W, int tilesX, int tilesY) {
  const SkPixel p = sk_pixel(H, W, tilesX, tilesY);
  if (!p.live) return;
  const float c = Ej[p.i];
  if (Enext) {
    float v = c, h = c;
    if (p.y > 0) v = fminf(v, Ej[p.i - W]);
    if (p.y < H - 1) v = fminf(v, Ej[p.i + W]);
    if (p.x > 0) h = fminf(h, Ej[p.i - 1]);
    if (p.x < W - 1) h = fminf(h, Ej[p.i + 1]);
    Enext[p.i] = fminf(v, h);
  }
  if (Sout) {
    const float d = sk_relu(__fsub_rn(Eprev[p.i], sk_dilate(Ej, p, H, W)));
    float s = d;
    if (Sprev) {
      const float sp = Sprev[p.i];
      s = __fadd_rn(sp, sk_relu(__fsub_rn(d, __fmul_rn(sp, d))));
    }
    Sout[p.i] = s;
  }
}

// E_k of the saved state: E_0 is the input itself, E_1 .. E_{iters+1} the state's first iters + 1 planes, S_0 .. S_{iters-1} follow.
__device__ __forceinline__ const float* sk_E(const float* X, const float* state, long plane, int k) {
  return k == 0 ? X : state + (long)(k - 1) * plane;
}

// The pixel-local chain of the backward: from dL/dS_iters down the S updates; G[k] = dL/dD_k where E_k - O_k > 0, else 0.
__global__ __launch_bounds__(256) void skel_bwd_chain_kernel(const float* __restrict__ X, const float* __restrict__ state,
                                                             const float* __restrict__ grad, float* __restrict__ G, long plane,
                                                             int iters, int H, int W, int tilesX, int tilesY) {
  const SkPixel p = sk_pixel(H, W, tilesX, tilesY);
  if (!p.live) return;
  const float* S = state + (long)(iters + 1) * plane;
  float g = grad[p.i];
  for (int k = iters; k >= 0; --k) {
    const float diff = __fsub_rn(sk_E(X, state, plane, k)[p.i], sk_dilate(sk_E(X, state, plane, k + 1), p, H, W));
    const float d = sk_relu(diff);
    float gd = g;
    if (k >= 1) {
      const float sp = S[(long)(k - 1) * plane + p.i];
      const float gr = __fsub_rn(d, __fmul_rn(sp, d)) > 0.f ? g : 0.f;  // relu'(0) = 0
      gd = gr - gr * sp;
      g = g - gr * d;  // dL/dS_{k-1}
    }
    G[(long)k * plane + p.i] = diff > 0.f ? gd : 0.f;
  }
}

// Level k of the backward in gather form: out = dL/dE_k = G_k (k <= iters) - the G_{k-1} of the dilation windows whose first maximum
// in row-major order this cell is (k >= 1) + the shares of gnext = dL/dE_{k+1} of the erosions that selected this cell (k <= iters).
// The cell reads E_k in the 5x5 square around itself.  Gk, Gprev and gnext are null where the level has no such term.
__global__ __launch_bounds__(256) void skel_bwd_level_kernel(const float* __restrict__ Ek, const float* __restrict__ Gk,
                                                             const float* __restrict__ Gprev, const float* __restrict__ gnext,
                                                             float* __restrict__ out, int H, int W, int tilesX, int tilesY) {
  const SkPixel p = sk_pixel(H, W, tilesX, tilesY);
  if (!p.live) return;
  float nb[5][5];  // E_k around the cell; a cell outside the plane holds a value that is never looked at
  bool iny[5], inx[5];
#pragma unroll
  for (int a = 0; a < 5; ++a) {
    iny[a] = p.y + a - 2 >= 0 && p.y + a - 2 < H;
    inx[a] = p.x + a - 2 >= 0 && p.x + a - 2 < W;
  }
#pragma unroll
  for (int a = 0; a < 5; ++a)
#pragma unroll
    for (int b = 0; b < 5; ++b) nb[a][b] = (iny[a] && inx[b]) ? Ek[p.i + (long)(a - 2) * W + (b - 2)] : 0.f;
  const float c = nb[2][2];
  float acc = Gk ? Gk[p.i] : 0.f;
  if (Gprev) {
    // window centre q = (2 + qy, 2 + qx) in nb coordinates; the cell itself sits at (2, 2)
#pragma unroll
    for (int qy = -1; qy <= 1; ++qy) {
#pragma unroll
      for (int qx = -1; qx <= 1; ++qx) {
        if (!iny[2 + qy] || !inx[2 + qx]) continue;
        const float g = Gprev[p.i + (long)qy * W + qx];
        if (g == 0.f) continue;
        bool first = true;
#pragma unroll
        for (int uy = -1; uy <= 1; ++uy) {
#pragma unroll
          for (int ux = -1; ux <= 1; ++ux) {
            const int a = 2 + qy + uy, b = 2 + qx + ux;
            if (!iny[a] || !inx[b]) continue;
            const bool before = a < 2 || (a == 2 && b < 2);  // row-major: scanned before this cell
            first = first && (before ? nb[a][b] < c : nb[a][b] <= c);
          }
        }
        if (first) acc -= g;  // dL/dO_{k-1} = -G_{k-1}
      }
    }
  }
  if (gnext) {
    // q = this cell and its four neighbours: (dy, dx) of q relative to the cell
    const int qdy[5] = {0, -1, 1, 0, 0};
    const int qdx[5] = {0, 0, 0, -1, 1};
#pragma unroll
    for (int j = 0; j < 5; ++j) {
      const int a = 2 + qdy[j], b = 2 + qdx[j];
      if (!iny[a] || !inx[b]) continue;
      const float g = gnext[p.i + (long)qdy[j] * W + qdx[j]];
      if (g == 0.f) continue;
      // v of q over N C S and h over W C E, each with the offset of the first cell attaining it
      float v = nb[a][b], h = nb[a][b];
      int vo = 0, ho = 0;
      if (iny[a - 1]) { v = nb[a - 1][b]; vo = -1; }
      if (iny[a - 1] && nb[a][b] < v) { v = nb[a][b]; vo = 0; }
      if (iny[a + 1] && nb[a + 1][b] < v) { v = nb[a + 1][b]; vo = 1; }
      if (inx[b - 1]) { h = nb[a][b - 1]; ho = -1; }
      if (inx[b - 1] && nb[a][b] < h) { h = nb[a][b]; ho = 0; }
      if (inx[b + 1] && nb[a][b + 1] < h) { h = nb[a][b + 1]; ho = 1; }
      const float wv = v < h ? 1.f : (v == h ? 0.5f : 0.f);
      const float wh = 1.f - wv;
      // the cell is q's vertical candidate at offset -qdy (q in the same column) and its horizontal one at -qdx (same row)
      if (qdx[j] == 0 && vo == -qdy[j] && wv != 0.f) acc += wv * g;
      if (qdy[j] == 0 && ho == -qdx[j] && wh != 0.f) acc += wh * g;
    }
  }
  out[p.i] = acc;
}

// P = softmax(logits)[n][c] and Y = (target == c) for the classes of `mask`, both 0 at an ignored pixel
__global__ __launch_bounds__(256) void cldice_planes_kernel(const float* __restrict__ x, const long long* __restrict__ tgt,
                                                            float* __restrict__ P, float* __restrict__ Y, int C, int K, long HW,
                                                            unsigned mask, int ignore) {
  const long hw = (long)blockIdx.x * 256 + threadIdx.x;
  const long n = blockIdx.y;
  if (hw >= HW) return;
  const int t = (int)tgt[n * HW + hw];
  if (t == ignore) {
    for (int j = 0; j < K; ++j) {
      P[(n * K + j) * HW + hw] = 0.f;
      Y[(n * K + j) * HW + hw] = 0.f;
    }
    return;
  }
  float v[kCdMaxC];
  float mx = -INFINITY;
#pragma unroll
  for (int c = 0; c < kCdMaxC; ++c) {
    v[c] = c < C ? x[(n * C + c) * HW + hw] : -INFINITY;
    mx = fmaxf(mx, v[c]);
  }
  float sum = 0.f;
#pragma unroll
  for (int c = 0; c < kCdMaxC; ++c) {
    v[c] = c < C ? expf(v[c] - mx) : 0.f;
    sum += v[c];
  }
  int j = 0;
#pragma unroll
  for (int c = 1; c < kCdMaxC; ++c) {
    if (!(mask >> c & 1u)) continue;
    P[(n * K + j) * HW + hw] = v[c] / sum;
    Y[(n * K + j) * HW + hw] = c == t ? 1.f : 0.f;
    ++j;
  }
}

// partial[(plane * nblk + b) * 4 + {sum S_P Y, sum S_P, sum S_Y P, sum S_Y}] of the block's pixels, in fp64
__global__ __launch_bounds__(256) void cldice_partial_kernel(const float* __restrict__ P, const float* __restrict__ Y,
                                                             const float* __restrict__ SP, const float* __restrict__ SY,
                                                             double* __restrict__ partial, long HW, int nblk) {
  __shared__ double red[4][4];
  const long m = blockIdx.y;
  double acc[4] = {0, 0, 0, 0};
  for (long hw = (long)blockIdx.x * 256 + threadIdx.x; hw < HW; hw += (long)nblk * 256) {
    const long i = m * HW + hw;
    const double sp = (double)SP[i], sy = (double)SY[i];
    acc[0] += sp * (double)Y[i];
    acc[1] += sp;
    acc[2] += sy * (double)P[i];
    acc[3] += sy;
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const double s = rs_wave_sum(acc[i]);
    if (lane == 0) red[wave][i] = s;
  }
  __syncthreads();
  if (threadIdx.x < 4) {
    const int i = threadIdx.x;
    partial[(m * nblk + blockIdx.x) * 4 + i] = (red[0][i] + red[1][i]) + (red[2][i] + red[3][i]);
  }
}

// sums[plane * 4 + i] = the partial sums of the plane's blocks added in ascending block order
__global__ __launch_bounds__(256) void cldice_reduce_kernel(const double* __restrict__ partial, double* __restrict__ sums, long items,
                                                            int nblk) {
  const long it = (long)blockIdx.x * 256 + threadIdx.x;
  if (it >= items) return;
  const long m = it >> 2;
  const int i = (int)(it & 3);
  double s = 0;
  for (int b = 0; b < nblk; ++b) s += partial[(m * nblk + b) * 4 + i];
  sums[it] = s;
}

// One block.  Per pair: Tprec = (A + s) / (B + s), Tsens = (Cc + s) / (Dd + s), term = 1 - 2 Tprec Tsens / (Tprec + Tsens); the loss
// is the mean over the pairs, added by a tree over the threads (a fixed order).  coef[m * 3 + {alpha, beta, gamma}]:
// dL/dS_P = alpha Y + beta per pixel, dL/dP (through Tsens) = gamma S_Y.  A ratio with a zero denominator counts as 0 and has no
// gradient; Tprec + Tsens = 0 gives the term 1 and no gradient (only smooth = 0 gets there).
__global__ __launch_bounds__(256) void cldice_finalize_kernel(const double* __restrict__ sums, float* __restrict__ loss,
                                                              float* __restrict__ coef, int pairs, float smooth) {
  __shared__ double red[256];
  const double s = (double)smooth, scale = 1.0 / (double)pairs;
  double t = 0;
  for (int m = threadIdx.x; m < pairs; m += 256) {
    const double A = sums[m * 4l], B = sums[m * 4l + 1], Cc = sums[m * 4l + 2], Dd = sums[m * 4l + 3];
    const double bp = B + s, bs = Dd + s;
    const double tp = bp > 0.0 ? (A + s) / bp : 0.0, ts = bs > 0.0 ? (Cc + s) / bs : 0.0;
    const double sum = tp + ts;
    double term = 1.0, alpha = 0, beta = 0, gamma = 0;
    if (sum > 0.0) {
      term = 1.0 - 2.0 * tp * ts / sum;
      const double dtp = -2.0 * ts * ts / (sum * sum), dts = -2.0 * tp * tp / (sum * sum);
      if (bp > 0.0) {
        alpha = scale * dtp / bp;
        beta = -scale * dtp * (A + s) / (bp * bp);
      }
      if (bs > 0.0) gamma = scale * dts / bs;
    }
    coef[m * 3l] = (float)alpha;
    coef[m * 3l + 1] = (float)beta;
    coef[m * 3l + 2] = (float)gamma;
    t += term;
  }
  red[threadIdx.x] = t;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) loss[0] = (float)(red[0] * scale);
}

// dL/dS_P of the clDice term per pixel: alpha Y + beta
__global__ __launch_bounds__(256) void cldice_skel_grad_kernel(const float* __restrict__ Y, const float* __restrict__ coef,
                                                               float* __restrict__ g, long HW) {
  const long hw = (long)blockIdx.x * 256 + threadIdx.x;
  const long m = blockIdx.y;
  if (hw >= HW) return;
  g[m * HW + hw] = coef[m * 3] * Y[m * HW + hw] + coef[m * 3 + 1];
}

// dz_k = gout * p_k (g_k - sum_c g_c p_c), g_c = dP[c] + gamma_c S_Y[c] for the classes of `mask`, 0 for the others; 0 under an
// ignored pixel
__global__ __launch_bounds__(256) void cldice_bwd_kernel(const float* __restrict__ x, const long long* __restrict__ tgt,
                                                         const float* __restrict__ dP, const float* __restrict__ SY,
                                                         const float* __restrict__ coef, const float* __restrict__ gout,
                                                         float* __restrict__ dx, int C, int K, long HW, unsigned mask, int ignore) {
  const long hw = (long)blockIdx.x * 256 + threadIdx.x;
  const long n = blockIdx.y;
  if (hw >= HW) return;
  const int t = (int)tgt[n * HW + hw];
  if (t == ignore) {
    for (int c = 0; c < C; ++c) dx[(n * C + c) * HW + hw] = 0.f;
    return;
  }
  float v[kCdMaxC], g[kCdMaxC];
  float mx = -INFINITY;
#pragma unroll
  for (int c = 0; c < kCdMaxC; ++c) {
    v[c] = c < C ? x[(n * C + c) * HW + hw] : -INFINITY;
    mx = fmaxf(mx, v[c]);
  }
  float sum = 0.f;
#pragma unroll
  for (int c = 0; c < kCdMaxC; ++c) {
    v[c] = c < C ? expf(v[c] - mx) : 0.f;
    sum += v[c];
  }
  const float go = gout ? gout[0] : 1.f;
  float dot = 0.f;
  int j = 0;
  g[0] = 0.f;
#pragma unroll
  for (int c = 0; c < kCdMaxC; ++c) {
    v[c] = v[c] / sum;
    if (c == 0) continue;
    g[c] = 0.f;
    if (!(mask >> c & 1u)) continue;
    const long i = (n * K + j) * HW + hw;
    g[c] = dP[i] + coef[(n * K + j) * 3 + 2] * SY[i];
    dot += g[c] * v[c];
    ++j;
  }
#pragma unroll
  for (int c = 0; c < kCdMaxC; ++c)
    if (c < C) dx[(n * C + c) * HW + hw] = go * v[c] * (g[c] - dot);
}

// positive sizes, M * H * W < 2^31, and a grid of tiles that fits one launch dimension
bool sk_shape_ok(int M, int H, int W, int iters) {
  if (M <= 0 || H <= 0 || W <= 0 || iters < 0 || iters > kSkMaxIters) return false;
  if ((long)M * H * W >= (1l << 31)) return false;
  return (long)M * rs_cdiv(H, kSkTileH) * rs_cdiv(W, kSkTileW) < (1l << 31);
}

int cd_popcount(unsigned m) { return __builtin_popcount(m); }

// 2 <= C <= 8, a non-empty mask of classes 1 .. C-1, positive sizes, N * C * H * W < 2^31, an ignore label that is -1 or no class
bool cd_shape_ok(int N, int C, int H, int W, unsigned mask, int ignore) {
  if (N <= 0 || N > 65535 || C < 2 || C > kCdMaxC || H <= 0 || W <= 0) return false;
  if ((long)N * C * H * W >= (1l << 31)) return false;
  if (mask == 0u || (mask & 1u) || (mask >> C)) return false;
  return ignore == -1 || (ignore >= C && ignore <= 255);
}

int cd_blocks(long HW) {
  const long nb = (HW + 255) / 256;
  return nb < kCdBlocks ? (int)nb : kCdBlocks;
}

}  // namespace

extern "C" long rs_soft_skeleton_state_floats(int M, int H, int W, int iters, int save) {
  if (!sk_shape_ok(M, H, W, iters)) return RS_EINVAL;
  const long plane = (long)M * H * W;
  // saved: E_1 .. E_{iters+1}, S_0 .. S_{iters-1}; not saved: three E planes and two S planes in turn
  return save ? (2l * iters + 1) * plane : 5 * plane;
}

extern "C" int rs_soft_skeleton_fwd(const float* planes, float* skel, float* state, int M, int H, int W, int iters, int save,
                                    rs_stream_t stream) {
  if (!planes || !skel || !state || !sk_shape_ok(M, H, W, iters)) return RS_EINVAL;
  const long plane = (long)M * H * W;
  const int tilesX = rs_cdiv(W, kSkTileW), tilesY = rs_cdiv(H, kSkTileH);
  const unsigned grid = (unsigned)((long)M * tilesX * tilesY);
  hipStream_t s = (hipStream_t)stream;
  // E_k for k >= 1 and S_k for k < iters (S_iters is `skel`)
  auto E = [&](int k) -> float* { return state + (save ? (long)(k - 1) : (long)(k % 3)) * plane; };
  auto S = [&](int k) -> float* {
    if (k == iters) return skel;
    return state + (save ? (long)(iters + 1 + k) : (long)(3 + k % 2)) * plane;
  };
  for (int j = 0; j <= iters + 1; ++j) {
    const float* Ej = j == 0 ? planes : E(j);
    const float* Eprev = j == 0 ? nullptr : (j == 1 ? planes : E(j - 1));
    const float* Sprev = j >= 2 ? S(j - 2) : nullptr;
    float* Enext = j <= iters ? E(j + 1) : nullptr;
    float* Sout = j >= 1 ? S(j - 1) : nullptr;
    skel_fwd_kernel<<<grid, 256, 0, s>>>(Ej, Eprev, Sprev, Enext, Sout, H, W, tilesX, tilesY);
    const int rc = RS_LAUNCH_RESULT();
    if (rc) return rc;
  }
  return 0;
}

extern "C" long rs_soft_skeleton_bwd_workspace_bytes(int M, int H, int W, int iters) {
  if (!sk_shape_ok(M, H, W, iters)) return RS_EINVAL;
  return (long)(iters + 3) * M * H * W * (long)sizeof(float);  // G_0 .. G_iters and two planes of dL/dE in turn
}

extern "C" int rs_soft_skeleton_bwd(const float* planes, const float* state, const float* grad, float* dplanes, int M, int H, int W,
                                    int iters, void* workspace, rs_stream_t stream) {
  if (!planes || !state || !grad || !dplanes || !workspace || ((uintptr_t)workspace & 3) || !sk_shape_ok(M, H, W, iters))
    return RS_EINVAL;
  const long plane = (long)M * H * W;
  const int tilesX = rs_cdiv(W, kSkTileW), tilesY = rs_cdiv(H, kSkTileH);
  const unsigned grid = (unsigned)((long)M * tilesX * tilesY);
  hipStream_t s = (hipStream_t)stream;
  float* G = static_cast<float*>(workspace);
  float* gE[2] = {G + (long)(iters + 1) * plane, G + (long)(iters + 2) * plane};
  skel_bwd_chain_kernel<<<grid, 256, 0, s>>>(planes, state, grad, G, plane, iters, H, W, tilesX, tilesY);
  int rc = RS_LAUNCH_RESULT();
  if (rc) return rc;
  for (int k = iters + 1; k >= 0; --k) {
    const float* Ek = k == 0 ? planes : state + (long)(k - 1) * plane;
    const float* Gk = k <= iters ? G + (long)k * plane : nullptr;
    const float* Gprev = k >= 1 ? G + (long)(k - 1) * plane : nullptr;
    const float* gnext = k <= iters ? gE[(k + 1) & 1] : nullptr;
    float* out = k == 0 ? dplanes : gE[k & 1];
    skel_bwd_level_kernel<<<grid, 256, 0, s>>>(Ek, Gk, Gprev, gnext, out, H, W, tilesX, tilesY);
    rc = RS_LAUNCH_RESULT();
    if (rc) return rc;
  }
  return 0;
}

extern "C" int rs_cldice_planes(const float* logits, const long long* targets, float* P, float* Y, int N, int C, int H, int W,
                                int class_mask, int ignore, rs_stream_t stream) {
  if (!logits || !targets || !P || !Y || !cd_shape_ok(N, C, H, W, (unsigned)class_mask, ignore)) return RS_EINVAL;
  const long HW = (long)H * W;
  cldice_planes_kernel<<<dim3(rs_cdiv(HW, 256), N), 256, 0, (hipStream_t)stream>>>(logits, targets, P, Y, C, cd_popcount((unsigned)class_mask),
                                                                                  HW, (unsigned)class_mask, ignore);
  return RS_LAUNCH_RESULT();
}

extern "C" long rs_cldice_workspace_bytes(int pairs) {
  if (pairs <= 0 || pairs > 65535) return RS_EINVAL;
  return (long)pairs * kCdBlocks * 4 * (long)sizeof(double);
}

extern "C" int rs_cldice_sums(const float* P, const float* Y, const float* SP, const float* SY, double* sums, int pairs, int H, int W,
                              void* workspace, rs_stream_t stream) {
  if (!P || !Y || !SP || !SY || !sums || !workspace || ((uintptr_t)workspace & 7) || pairs <= 0 || pairs > 65535 || H <= 0 || W <= 0 ||
      (long)pairs * H * W >= (1l << 31))
    return RS_EINVAL;
  const long HW = (long)H * W;
  const int nblk = cd_blocks(HW);
  hipStream_t s = (hipStream_t)stream;
  double* part = static_cast<double*>(workspace);
  cldice_partial_kernel<<<dim3(nblk, pairs), 256, 0, s>>>(P, Y, SP, SY, part, HW, nblk);
  const int rc = RS_LAUNCH_RESULT();
  if (rc) return rc;
  cldice_reduce_kernel<<<rs_cdiv(4l * pairs, 256), 256, 0, s>>>(part, sums, 4l * pairs, nblk);
  return RS_LAUNCH_RESULT();
}

extern "C" int rs_cldice_finalize(const double* sums, float* loss, float* coef, int pairs, float smooth, rs_stream_t stream) {
  if (!sums || !loss || !coef || pairs <= 0 || pairs > 65535 || !(smooth - smooth == 0.f) || smooth < 0.f) return RS_EINVAL;
  cldice_finalize_kernel<<<1, 256, 0, (hipStream_t)stream>>>(sums, loss, coef, pairs, smooth);
  return RS_LAUNCH_RESULT();
}

extern "C" int rs_cldice_skel_grad(const float* Y, const float* coef, float* grad, int pairs, int H, int W, rs_stream_t stream) {
  if (!Y || !coef || !grad || pairs <= 0 || pairs > 65535 || H <= 0 || W <= 0 || (long)pairs * H * W >= (1l << 31)) return RS_EINVAL;
  const long HW = (long)H * W;
  cldice_skel_grad_kernel<<<dim3(rs_cdiv(HW, 256), pairs), 256, 0, (hipStream_t)stream>>>(Y, coef, grad, HW);
  return RS_LAUNCH_RESULT();
}

extern "C" int rs_cldice_bwd(const float* logits, const long long* targets, const float* dP, const float* SY, const float* coef,
                             const float* grad_out, float* dlogits, int N, int C, int H, int W, int class_mask, int ignore,
                             rs_stream_t stream) {
  if (!logits || !targets || !dP || !SY || !coef || !dlogits || !cd_shape_ok(N, C, H, W, (unsigned)class_mask, ignore)) return RS_EINVAL;
  const long HW = (long)H * W;
  cldice_bwd_kernel<<<dim3(rs_cdiv(HW, 256), N), 256, 0, (hipStream_t)stream>>>(logits, targets, dP, SY, coef, grad_out, dlogits, C,
                                                                               cd_popcount((unsigned)class_mask), HW, (unsigned)class_mask, ignore);
  return RS_LAUNCH_RESULT();
}
