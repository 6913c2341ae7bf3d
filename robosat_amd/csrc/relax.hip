// Boundary label relaxation for CrossEntropy / Focal (rs_label_set_plane, rs_nll_loss_fwd_rx / rs_nll_loss_bwd_rx in
// include/robosat_hip.h): at a pixel whose (2R+1)^2 neighbourhood holds several classes the loss maximises the
// probability of their union, -log sum_{c in S} p_c, instead of -log p_t (Zhu et al., CVPR 2019).
//
//   label_set_kernel   int64 labels -> one byte per pixel, bit c = "class c occurs among the valid pixels within R in x and in y".
//                      One launch: a block stages a 64 x 64 tile plus an apron of R as class bits in LDS, four pixels per dword, ORs
//                      along the rows, then along the columns, and stores.  OR is idempotent, so a window of n = 2R+1 is built by
//                      doubling, w_2k(i) = w_k(i) | w_k(i+k) up to the largest power of two p <= n, and one more OR of the two
//                      overlapping windows w_p(i) | w_p(i+n-p): log2(p) + 1 ORs per pass instead of n taps.
//   nll_*_rx_kernel    the IgnoreWeight body of loss.hip with one more byte load per pixel and the target's terms replaced by the
//                      set's: same launch geometry, same workspace, same guarded finalize, sums in double in the same fixed order.
//                      A pixel whose set is its own label alone does the arithmetic of the `_pw` kernels in their order.
#include <initializer_list>

#include "common.h"

namespace {

constexpr int kMaxC = 8;
constexpr int kLossBlocks = 1024;  // (as in loss.hip: the `_rx` calls use the workspace of rs_nll_loss_workspace_bytes)

constexpr int kRelaxMaxR = 16;
constexpr int kTile = 64;                         // output pixels per block and axis
constexpr int kStageRows = kTile + 2 * kRelaxMaxR;  // 96
constexpr int kStageDw = kStageRows / 4;           // 24 dwords of four class bytes per staged row
constexpr int kStride = kStageDw + 1;              // (odd: rows start in different LDS banks)
constexpr int kSetThreads = 256;

// dword `j` of row `row` of a staged buffer, 0 beyond its `rows` rows and `ndw` dwords
__device__ __forceinline__ unsigned int set_dw(const unsigned int* __restrict__ buf, int row, int j, int rows, int ndw) {
  return (row < rows && j < ndw) ? buf[row * kStride + j] : 0u;
}

// the four bytes that stand `k` bytes behind dword `j` of the row: byte b of the result is byte 4j + b + k of the row
__device__ __forceinline__ unsigned int set_dw_shifted(const unsigned int* __restrict__ buf, int row, int j, int k, int rows,
                                                           int ndw) {
  const int q = k >> 2, r = (k & 3) * 8;
  const unsigned long long lo = set_dw(buf, row, j + q, rows, ndw), hi = set_dw(buf, row, j + q + 1, rows, ndw);
  return (unsigned int)(((hi << 32) | lo) >> r);
}

// dst = src | (src moved by `k` bytes along the row) over `rows` x `ndw` dwords
__device__ __forceinline__ void set_or_row(const unsigned int* __restrict__ src, unsigned int* __restrict__ dst, int rows, int ndw, int k) {
  for (int i = threadIdx.x; i < rows * ndw; i += kSetThreads) {
    const int row = i / ndw, j = i - row * ndw;
    dst[row * kStride + j] = src[row * kStride + j] | set_dw_shifted(src, row, j, k, rows, ndw);
  }
  rs_lds_writes_done();
  __syncthreads();
}

// dst = src | (src moved by `k` rows) over `rows` x `ndw` dwords
__device__ __forceinline__ void set_or_col(const unsigned int* __restrict__ src, unsigned int* __restrict__ dst, int rows, int ndw, int k) {
  for (int i = threadIdx.x; i < rows * ndw; i += kSetThreads) {
    const int row = i / ndw, j = i - row * ndw;
    dst[row * kStride + j] = src[row * kStride + j] | set_dw(src, row + k, j, rows, ndw);
  }
  rs_lds_writes_done();
  __syncthreads();
}

// Staged byte (sy, sx) of the block is pixel (y0 - R + sy, x0 - R + sx): 1 << label at a valid pixel inside the image, 0 anywhere
// else.  After the row pass byte (sy, sx) holds the OR of the staged bytes sx .. sx + 2R of its row, after the column pass the OR
// of those over the rows sy .. sy + 2R: the set of the pixel (y0 + sy, x0 + sx).  `stage` keeps the staged bytes to the end (the
// store zeroes the ignored pixels by them); the passes alternate between `a` and `b`.
__global__ __launch_bounds__(kSetThreads) void label_set_kernel(const long long* __restrict__ tgt, uint8_t* __restrict__ sets, int H,
                                                                int W, int R, long long ignore) {
  __shared__ unsigned int stage[kStageRows * kStride], a[kStageRows * kStride], b[kStageRows * kStride];
  const int x0 = blockIdx.x * kTile, y0 = blockIdx.y * kTile;
  const long base = (long)blockIdx.z * H * W;
  const int n = 2 * R + 1;
  const int rows = kTile + 2 * R;    // staged rows, and staged bytes per row
  const int ndw = (rows + 3) >> 2;   // <= kStageDw
  for (int i = threadIdx.x; i < rows * ndw; i += kSetThreads) {
    const int sy = i / ndw, j = i - sy * ndw;
    const int y = y0 - R + sy;
    unsigned int d = 0;
    if (y >= 0 && y < H) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int sx = 4 * j + e, x = x0 - R + sx;
        if (sx < rows && x >= 0 && x < W) {
          const long long t = tgt[base + (long)y * W + x];
          if (t != ignore) d |= (1u << ((unsigned int)t & 7u)) << (8 * e);
        }
      }
    }
    stage[sy * kStride + j] = d;
  }
  rs_lds_writes_done();
  __syncthreads();

  int p = 2;
  while (2 * p <= n) p *= 2;  // the largest power of two <= n (n >= 3)
  const unsigned int* cur = stage;
  unsigned int* nxt = a;
  auto flip = [&] { cur = nxt, nxt = nxt == a ? b : a; };
  // rows: w_2, w_4 .. w_p, then w_p(i) | w_p(i + n - p)
  for (int k = 1; k < p; k *= 2) {
    set_or_row(cur, nxt, rows, ndw, k);
    flip();
  }
  set_or_row(cur, nxt, rows, ndw, n - p);
  flip();
  // columns: the same on whole rows; only the kTile / 4 dwords that are stored are carried on
  constexpr int odw = kTile / 4;
  for (int k = 1; k < p; k *= 2) {
    set_or_col(cur, nxt, rows, odw, k);
    flip();
  }
  set_or_col(cur, nxt, rows, odw, n - p);
  cur = nxt;

  for (int i = threadIdx.x; i < kTile * odw; i += kSetThreads) {
    const int ty = i / odw, j = i - ty * odw;
    const int y = y0 + ty, x = x0 + 4 * j;
    if (y >= H || x >= W) continue;
    unsigned int v = cur[ty * kStride + j];
    const unsigned int own = set_dw_shifted(stage, ty + R, j, R, rows, ndw);  // the staged bytes of these four pixels
    unsigned int keep = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) keep |= ((own >> (8 * e)) & 0xffu) ? (0xffu << (8 * e)) : 0u;
    v &= keep;
    const long at = base + (long)y * W + x;
    if (x + 3 < W && !((uintptr_t)(sets + at) & 3)) {
      *reinterpret_cast<unsigned int*>(sets + at) = v;
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (x + e < W) sets[at + e] = (uint8_t)(v >> (8 * e));
    }
  }
}

template <int C>
__device__ __forceinline__ void load_logits(const float* __restrict__ x, long n, long hw, long HW, float (&v)[C]) {
#pragma unroll
  for (int c = 0; c < C; ++c) v[c] = x[(n * C + c) * HW + hw];
}

// Per-pixel value of the (unnormalised) relaxed loss and, optionally, d/dx_c of it: pixel_loss of loss.hip, statement for statement,
// with log p_t -> log q = lse_S - lse and 1[c == t] -> r_c = exp(x_c - max_S) / sum_S.  lse_S has its own maximum, so a set whose
// logits all lie far below the largest one keeps its precision.  A set that is the label alone has max_S = x_t, sum_S = 1, lse_S =
// x_t and r_t = 1 exactly; a set of all C classes has max_S, sum_S and r_c equal to the softmax's own, so log q and the
// CrossEntropy gradient are exactly 0.
template <int C>
__device__ __forceinline__ float pixel_loss_rx(const float (&v)[C], unsigned int set, int mode, float gamma, float (*grad)[C]) {
  float mx = v[0];
#pragma unroll
  for (int c = 1; c < C; ++c) mx = fmaxf(mx, v[c]);
  float e[C], sum = 0.f;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    e[c] = expf(v[c] - mx);
    sum += e[c];
  }
  const float lse = logf(sum) + mx;
  float ms = -INFINITY;
#pragma unroll
  for (int c = 0; c < C; ++c) ms = ((set >> c) & 1u) ? fmaxf(ms, v[c]) : ms;
  float es[C], ssum = 0.f;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    es[c] = ((set >> c) & 1u) ? expf(v[c] - ms) : 0.f;
    ssum += es[c];
  }
  const float lses = logf(ssum) + ms;
  const float logq = lses - lse;  // log of the set's probability
  if (mode == 0) {
    if (grad) {
#pragma unroll
      for (int c = 0; c < C; ++c) (*grad)[c] = e[c] / sum - es[c] / ssum;
    }
    return -logq;
  }
  const float q = expf(logq);
  const float om = 1.f - q;
  const float pw = powf(om, gamma);
  if (grad) {
    // L = -(1-q)^g * log q ;  dL/dx_c = [ g (1-q)^(g-1) q log q - (1-q)^g ] * (r_c - p_c)   (the expression of pixel_loss, as written there)
    const float pwm1 = (gamma == 0.f) ? 0.f : gamma * powf(om, gamma - 1.f);
    const float k = pwm1 * q * logq - pw;
#pragma unroll
    for (int c = 0; c < C; ++c) (*grad)[c] = k * (es[c] / ssum - e[c] / sum);
  }
  return -pw * logq;
}

// partial[block] = (sum w*l, sum w) of the block; w is the weight of the pixel's OWN label, so sum w does not depend on the sets
template <int C>
__global__ __launch_bounds__(256) void nll_fwd_rx_kernel(const float* __restrict__ x, const long long* __restrict__ tgt,
                                                         const float* __restrict__ weight, double* __restrict__ partial, long P,
                                                         long HW, int mode, float gamma, int ignore, const float* __restrict__ pixw,
                                                         const uint8_t* __restrict__ sets) {
  __shared__ double red[2][4];
  double sl = 0, sw = 0;
  for (long p = (long)blockIdx.x * 256 + threadIdx.x; p < P; p += (long)gridDim.x * 256) {
    const int t = (int)tgt[p];
    if (t == ignore) continue;
    const long n = p / HW, hw = p - n * HW;
    float v[C];
    load_logits<C>(x, n, hw, HW, v);
    const unsigned int set = (unsigned int)sets[p] | (1u << (t & 7));  // (a valid pixel holds its own bit)
    const float w = (pixw ? pixw[p] : 1.f) * (weight ? weight[t] : 1.f);
    const float l = pixel_loss_rx<C>(v, set, mode, gamma, nullptr);
    sl += (double)(w * l);
    sw += (double)w;
  }
  sl = rs_wave_sum(sl);
  sw = rs_wave_sum(sw);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
    red[0][wave] = sl;
    red[1][wave] = sw;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    partial[blockIdx.x * 2] = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
    partial[blockIdx.x * 2 + 1] = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
  }
}

// loss = sum(w*l) / sum(w); stats[0] = loss, stats[1] = sum(w); no valid weight at all gives loss 0 and stats[1] = 0 (the guarded
// finalize of loss.hip, which is private to that file)
__global__ void nll_finalize_rx_kernel(const double* __restrict__ partial, int nblocks, float* __restrict__ loss,
                                       float* __restrict__ stats) {
  __shared__ double red[2][256];
  double sl = 0, sw = 0;
  for (int b = threadIdx.x; b < nblocks; b += 256) {
    sl += partial[b * 2];
    sw += partial[b * 2 + 1];
  }
  red[0][threadIdx.x] = sl;
  red[1][threadIdx.x] = sw;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) {
      red[0][threadIdx.x] += red[0][threadIdx.x + o];
      red[1][threadIdx.x] += red[1][threadIdx.x + o];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const float l = red[1][0] > 0.0 ? (float)(red[0][0] / red[1][0]) : 0.f;
    loss[0] = l;
    stats[0] = l;
    stats[1] = (float)red[1][0];
  }
}

// dx[c][p] = gout * w[t_p] * dl_p/dx_c / sum(w); +0.0f in every class plane of an ignored pixel and of a pixel of weight 0
template <int C>
__global__ __launch_bounds__(256) void nll_bwd_rx_kernel(const float* __restrict__ x, const long long* __restrict__ tgt,
                                                         const float* __restrict__ weight, const float* __restrict__ stats,
                                                         const float* __restrict__ gout, float* __restrict__ dx, long P, long HW,
                                                         int mode, float gamma, int ignore, const float* __restrict__ pixw,
                                                         const uint8_t* __restrict__ sets) {
  const long p = (long)blockIdx.x * 256 + threadIdx.x;
  if (p >= P) return;
  const long n = p / HW, hw = p - n * HW;
  const int t = (int)tgt[p];
  const float pw = (t == ignore || !pixw) ? 1.f : pixw[p];
  if (t == ignore || !(stats[1] > 0.f) || pw == 0.f) {
#pragma unroll
    for (int c = 0; c < C; ++c) dx[(n * C + c) * HW + hw] = 0.f;
    return;
  }
  float v[C], g[C];
  load_logits<C>(x, n, hw, HW, v);
  const unsigned int set = (unsigned int)sets[p] | (1u << (t & 7));
  const float w = pw * (weight ? weight[t] : 1.f);
  pixel_loss_rx<C>(v, set, mode, gamma, &g);
  const float k = (gout ? gout[0] : 1.f) * w / stats[1];
#pragma unroll
  for (int c = 0; c < C; ++c) dx[(n * C + c) * HW + hw] = k * g[c];
}

inline int loss_grid(long P) {
  const long nb = (P + 255) / 256;
  return nb < kLossBlocks ? (int)nb : kLossBlocks;
}

template <int C>
int run_fwd_rx(const float* x, const long long* t, const float* w, float* loss, float* stats, void* workspace, int N, int H, int W,
               int mode, float gamma, rs_stream_t stream, const float* pixw, int ignore, const uint8_t* sets) {
  const long HW = (long)H * W, P = (long)N * HW;
  hipStream_t s = (hipStream_t)stream;
  double* part = reinterpret_cast<double*>(workspace);
  const int grid = loss_grid(P);
  nll_fwd_rx_kernel<C><<<grid, 256, 0, s>>>(x, t, w, part, P, HW, mode, gamma, ignore, pixw, sets);
  nll_finalize_rx_kernel<<<1, 256, 0, s>>>(part, grid, loss, stats);
  return RS_LAUNCH_RESULT();
}

template <int C>
int run_bwd_rx(const float* x, const long long* t, const float* w, const float* stats, const float* gout, float* dx, int N, int H, int W,
               int mode, float gamma, rs_stream_t stream, const float* pixw, int ignore, const uint8_t* sets) {
  const long HW = (long)H * W, P = (long)N * HW;
  nll_bwd_rx_kernel<C><<<rs_cdiv(P, 256), 256, 0, (hipStream_t)stream>>>(x, t, w, stats, gout, dx, P, HW, mode, gamma, ignore, pixw, sets);
  return RS_LAUNCH_RESULT();
}

#define RS_DISPATCH_C(C, ...)                            \
  switch (C) {                                           \
    case 1: { constexpr int K = 1; return __VA_ARGS__; } \
    case 2: { constexpr int K = 2; return __VA_ARGS__; } \
    case 3: { constexpr int K = 3; return __VA_ARGS__; } \
    case 4: { constexpr int K = 4; return __VA_ARGS__; } \
    case 5: { constexpr int K = 5; return __VA_ARGS__; } \
    case 6: { constexpr int K = 6; return __VA_ARGS__; } \
    case 7: { constexpr int K = 7; return __VA_ARGS__; } \
    default: { constexpr int K = 8; return __VA_ARGS__; } \
  }

// -1 for "no pixel is ignored", or a label byte that is no class
bool ignore_ok(int ignore, int C) { return ignore == -1 || (ignore >= C && ignore <= 255); }

bool rx_args_ok(std::initializer_list<const void*> required, int N, int C, int H, int W, int mode, int ignore) {
  for (const void* p : required)
    if (!p) return false;
  return N > 0 && C > 0 && C <= kMaxC && H > 0 && W > 0 && mode >= 0 && mode <= 1 && ignore_ok(ignore, C);
}

// (the sizes the boundary and separation planes take)
bool plane_shape_ok(int N, int H, int W) {
  return N > 0 && N <= 65535 && H > 0 && W > 0 && H <= 4096 && W <= 4096 && (long)N * H * W < (1l << 29);
}

}  // namespace

extern "C" int rs_label_set_plane(const long long* targets, uint8_t* sets, int N, int C, int H, int W, int R, int ignore,
                                  rs_stream_t stream) {
  if (!targets || !sets || !plane_shape_ok(N, H, W) || C <= 0 || C > kMaxC || R < 1 || R > kRelaxMaxR || !ignore_ok(ignore, C))
    return RS_EINVAL;
  const dim3 grid(rs_cdiv(W, kTile), rs_cdiv(H, kTile), N);
  label_set_kernel<<<grid, kSetThreads, 0, (hipStream_t)stream>>>(targets, sets, H, W, R, (long long)ignore);
  return RS_LAUNCH_RESULT();
}

extern "C" int rs_nll_loss_fwd_rx(const float* logits, const long long* targets, const float* weight, float* loss, float* stats,
                                  int N, int C, int H, int W, int mode, float gamma, void* workspace, rs_stream_t stream,
                                  const float* pixel_weight, int ignore, const uint8_t* sets) {
  if (!rx_args_ok({logits, targets, loss, stats, workspace, sets}, N, C, H, W, mode, ignore)) return RS_EINVAL;
  RS_DISPATCH_C(C, run_fwd_rx<K>(logits, targets, weight, loss, stats, workspace, N, H, W, mode, gamma, stream, pixel_weight, ignore, sets));
}

extern "C" int rs_nll_loss_bwd_rx(const float* logits, const long long* targets, const float* weight, const float* stats,
                                  const float* grad_out, float* dlogits, int N, int C, int H, int W, int mode, float gamma,
                                  rs_stream_t stream, const float* pixel_weight, int ignore, const uint8_t* sets) {
  if (!rx_args_ok({logits, targets, stats, dlogits, sets}, N, C, H, W, mode, ignore)) return RS_EINVAL;
  RS_DISPATCH_C(C, run_bwd_rx<K>(logits, targets, weight, stats, grad_out, dlogits, N, H, W, mode, gamma, stream, pixel_weight, ignore, sets));
}
