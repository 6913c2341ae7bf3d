// Per-pixel classification losses and the confusion counts of the training loop, on NCHW logits [N][C][H][W] and
// int64 label maps [N][H][W] -- the tensors the reference's criteria receive (robosat/tools/train.py:185,226).
//
//   CrossEntropyLoss2d (robosat/losses.py:8-25):  NLLLoss(weight)(log_softmax(x, 1), t)
//       = sum_p w[t_p] * (lse_p - x[t_p][p]) / sum_p w[t_p]
//   FocalLoss2d (robosat/losses.py:28-50), gamma = 2 by default:
//       = sum_p w[t_p] * ( -(1 - s_t)^gamma * log s_t ) / sum_p w[t_p],   s = softmax(x, 1)
//   Metrics.add (robosat/metrics.py:27-41): argmax over classes, then the reference's pred/actual quotient trick.
//
// HBM-bound: one thread per pixel, plane-wise coalesced reads; reductions in fp64, two deterministic stages.
//
// Every loss kernel is ONE body with the per-pixel variant as a compile-time parameter (Px):
//   Plain          every pixel counts (rs_nll_loss_*, rs_miou_loss_*)
//   Ignore         the loss of the pixels whose label is not `ignore`, as if the ignored ones had been cut out of every image: an
//                  ignored pixel has no weight, no loss and a gradient of +0.0f in every class plane, its label byte never indexes
//                  `weight`, and its logits reach no result (rs_*_ig in include/robosat_hip.h)
//   IgnoreWeight   Ignore with one more load and one more multiply per pixel: the weight plane `pixw` [N][H][W] on top of the class
//                  weight (rs_nll_loss_*_pw; the plane itself: rs_boundary_weight_plane, further down)
// The variant's statements stand under `if constexpr`, each variant in the statement order it has always had (Plain reads the label
// behind the logits, the other two in front of them: an ignored pixel's logits are never read), so with no pixel ignored all
// three do the same arithmetic in the same order.  What a variant needs beyond the Plain arguments travels as one trailing kernel
// argument (see IgnoreAndWeight below), so a Plain or Ignore instantiation compiles to the instructions of the separate kernel it
// replaced; the IgnoreWeight ones take `pixw` in another place than theirs did and differ in how the arguments are loaded
// (profiles/loss_variants/).  A body shared through an inlined function does not keep the instructions: it is simplified on its
// own before it is inlined.
#include <initializer_list>

#include "common.h"

namespace {

constexpr int kMaxC = 8;
constexpr int kLossBlocks = 1024;

enum class Px { Plain, Ignore, IgnoreWeight };

template <int C>
__device__ __forceinline__ void load_logits(const float* __restrict__ x, long n, long hw, long HW, float (&v)[C]) {
#pragma unroll
  for (int c = 0; c < C; ++c) v[c] = x[(n * C + c) * HW + hw];
}

// per-pixel value of the (unnormalised) loss and, optionally, d/dx_c of it
template <int C>
__device__ __forceinline__ float pixel_loss(const float (&v)[C], int t, int mode, float gamma, float (*grad)[C]) {
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
  float xt = 0.f;
#pragma unroll
  for (int c = 0; c < C; ++c) xt = (c == t) ? v[c] : xt;
  const float logp = xt - lse;  // log softmax at the target
  if (mode == 0) {
    if (grad) {
#pragma unroll
      for (int c = 0; c < C; ++c) (*grad)[c] = e[c] / sum - (c == t ? 1.f : 0.f);
    }
    return -logp;
  }
  const float pt = expf(logp);
  const float om = 1.f - pt;
  const float pw = powf(om, gamma);
  if (grad) {
    // L = -(1-pt)^g * log pt ;  dL/dx_c = [ g (1-pt)^(g-1) pt log pt - (1-pt)^g ] * (1[c==t] - p_c)
    const float pwm1 = (gamma == 0.f) ? 0.f : gamma * powf(om, gamma - 1.f);
    const float k = pwm1 * pt * logp - pw;
#pragma unroll
    for (int c = 0; c < C; ++c) (*grad)[c] = k * ((c == t ? 1.f : 0.f) - e[c] / sum);
  }
  return -pw * logp;
}

// What a variant's kernel needs beyond the Plain arguments is ONE trailing argument: the pack `extra` holds nothing (Plain, which
// so keeps the argument list it has always had), `int ignore` (Ignore) or an IgnoreAndWeight, and `(extra, ...)` is that argument.
struct IgnoreAndWeight {
  int ignore;
  const float* pixw;
};

// partial[block] = (sum w*l, sum w) of the block
template <int C, Px V, typename... Extra>
__global__ __launch_bounds__(256) void nll_fwd_kernel(const float* __restrict__ x, const long long* __restrict__ tgt,
                                                      const float* __restrict__ weight, double* __restrict__ partial,
                                                      long P, long HW, int mode, float gamma, Extra... extra) {
  __shared__ double red[2][4];
  [[maybe_unused]] int ignore = 0;
  [[maybe_unused]] const float* pixw = nullptr;
  if constexpr (V == Px::Ignore) ignore = (extra, ...);
  if constexpr (V == Px::IgnoreWeight) ignore = (extra, ...).ignore, pixw = (extra, ...).pixw;
  double sl = 0, sw = 0;
  for (long p = (long)blockIdx.x * 256 + threadIdx.x; p < P; p += (long)gridDim.x * 256) {
    int t;
    if constexpr (V != Px::Plain) {
      t = (int)tgt[p];
      if (t == ignore) continue;
    }
    const long n = p / HW, hw = p - n * HW;
    float v[C];
    load_logits<C>(x, n, hw, HW, v);
    if constexpr (V == Px::Plain) t = (int)tgt[p];
    float w;
    if constexpr (V == Px::IgnoreWeight) w = pixw[p] * (weight ? weight[t] : 1.f);
    else w = weight ? weight[t] : 1.f;
    const float l = pixel_loss<C>(v, t, mode, gamma, nullptr);
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

// loss = sum(w*l) / sum(w); stats[0] = loss, stats[1] = sum(w).  Guarded (the Ignore variants): no valid weight at all
// (sum(w) == 0) gives loss 0, and stats[1] = 0 tells the backward; unguarded (Plain) it stays the NaN of 0 / 0.
template <bool Guarded>
__global__ void nll_finalize_kernel(const double* __restrict__ partial, int nblocks, float* __restrict__ loss,
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
    float l;
    if constexpr (Guarded) l = red[1][0] > 0.0 ? (float)(red[0][0] / red[1][0]) : 0.f;
    else l = (float)(red[0][0] / red[1][0]);
    loss[0] = l;
    stats[0] = l;
    stats[1] = (float)red[1][0];
  }
}

// dx[c][p] = gout * w[t_p] * dl_p/dx_c / sum(w)
template <int C, Px V, typename... Extra>
__global__ __launch_bounds__(256) void nll_bwd_kernel(const float* __restrict__ x, const long long* __restrict__ tgt,
                                                      const float* __restrict__ weight, const float* __restrict__ stats,
                                                      const float* __restrict__ gout, float* __restrict__ dx, long P, long HW,
                                                      int mode, float gamma, Extra... extra) {
  [[maybe_unused]] int ignore = 0;
  [[maybe_unused]] const float* pixw = nullptr;
  if constexpr (V == Px::Ignore) ignore = (extra, ...);
  if constexpr (V == Px::IgnoreWeight) ignore = (extra, ...).ignore, pixw = (extra, ...).pixw;
  const long p = (long)blockIdx.x * 256 + threadIdx.x;
  if (p >= P) return;
  const long n = p / HW, hw = p - n * HW;
  int t;
  if constexpr (V != Px::Plain) {
    t = (int)tgt[p];
    if (t == ignore || !(stats[1] > 0.f)) {
#pragma unroll
      for (int c = 0; c < C; ++c) dx[(n * C + c) * HW + hw] = 0.f;
      return;
    }
  }
  float v[C], g[C];
  load_logits<C>(x, n, hw, HW, v);
  if constexpr (V == Px::Plain) t = (int)tgt[p];
  float w;
  if constexpr (V == Px::IgnoreWeight) w = pixw[p] * (weight ? weight[t] : 1.f);
  else w = weight ? weight[t] : 1.f;
  pixel_loss<C>(v, t, mode, gamma, &g);
  const float k = (gout ? gout[0] : 1.f) * w / stats[1];
#pragma unroll
  for (int c = 0; c < C; ++c) dx[(n * C + c) * HW + hw] = k * g[c];
}

// counts[0..3] += (tn, fn, fp, tp) with the reference's naming: q = argmax/actual as floats; nan -> tn, +inf -> fn,
// 0 -> fp, 1 -> tp, anything else (only possible for C > 2) is dropped (robosat/metrics.py:35-41).
template <int C>
__global__ __launch_bounds__(256) void confusion_kernel(const float* __restrict__ x, const long long* __restrict__ tgt,
                                                        unsigned long long* __restrict__ counts, long P, long HW) {
  unsigned int c4[4] = {0, 0, 0, 0};
  for (long p = (long)blockIdx.x * 256 + threadIdx.x; p < P; p += (long)gridDim.x * 256) {
    const long n = p / HW, hw = p - n * HW;
    float v[C];
    load_logits<C>(x, n, hw, HW, v);
    int pred = 0;
    float best = v[0];
#pragma unroll
    for (int c = 1; c < C; ++c)
      if (v[c] > best) {  // torch.argmax: first maximal index
        best = v[c];
        pred = c;
      }
    const int act = (int)tgt[p];
    if (act == 0) {
      if (pred == 0) c4[0]++;  // 0/0 = nan
      else c4[1]++;            // k/0 = inf
    } else if (pred == 0) {
      c4[2]++;  // 0/k = 0
    } else if (pred == act) {
      c4[3]++;  // k/k = 1
    }
  }
  __shared__ unsigned int red[4];
  if (threadIdx.x < 4) red[threadIdx.x] = 0;
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    unsigned int s = c4[i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if ((threadIdx.x & 63) == 0) atomicAdd(&red[i], s);
  }
  __syncthreads();
  if (threadIdx.x < 4) atomicAdd(&counts[threadIdx.x], (unsigned long long)red[threadIdx.x]);
}

inline int loss_grid(long P) {
  const long nb = (P + 255) / 256;
  return nb < kLossBlocks ? (int)nb : kLossBlocks;
}

// (extra: the variant's trailing kernel arguments)
template <int C, Px V, typename... Extra>
int run_fwd(const float* x, const long long* t, const float* w, float* loss, float* stats, void* workspace, int N, int H, int W,
            int mode, float gamma, rs_stream_t stream, Extra... extra) {
  const long HW = (long)H * W, P = (long)N * HW;
  hipStream_t s = (hipStream_t)stream;
  double* part = reinterpret_cast<double*>(workspace);
  const int grid = loss_grid(P);
  nll_fwd_kernel<C, V><<<grid, 256, 0, s>>>(x, t, w, part, P, HW, mode, gamma, extra...);
  nll_finalize_kernel<V != Px::Plain><<<1, 256, 0, s>>>(part, grid, loss, stats);
  return RS_LAUNCH_RESULT();
}

template <int C, Px V, typename... Extra>
int run_bwd(const float* x, const long long* t, const float* w, const float* stats, const float* gout, float* dx, int N, int H, int W,
            int mode, float gamma, rs_stream_t stream, Extra... extra) {
  const long HW = (long)H * W, P = (long)N * HW;
  nll_bwd_kernel<C, V><<<rs_cdiv(P, 256), 256, 0, (hipStream_t)stream>>>(x, t, w, stats, gout, dx, P, HW, mode, gamma, extra...);
  return RS_LAUNCH_RESULT();
}

template <int C>
int run_conf(const float* x, const long long* t, unsigned long long* counts, long P, long HW, hipStream_t s) {
  confusion_kernel<C><<<loss_grid(P), 256, 0, s>>>(x, t, counts, P, HW);
  return RS_LAUNCH_RESULT();
}


// ---- mIoULoss2d (robosat/losses.py:53-83) ------------------------------------------------------------------------
// soft IoU per (class c, image n): inter = sum_p s_c m_c, union = sum_p (s_c + m_c - s_c m_c); miou = 1 - mean(inter/union);
// the reference returns Python max(miou, weighted NLL): whichever is larger, gradient through that branch only.
// Per-(n,c) sums: A = sum_{p: t=c} s_c, B = sum_p s_c, cnt = #{p: t=c}  =>  inter = A, union = B + cnt - A.
// Ignore: A, B, cnt and the two NLL sums all leave an ignored pixel out.
template <int C, bool Ignore, typename... Extra>
__global__ __launch_bounds__(256) void miou_partial_kernel(const float* __restrict__ x, const long long* __restrict__ tgt,
                                                           const float* __restrict__ weight, double* __restrict__ partial,
                                                           long HW, int nblk, Extra... extra) {
  // partial[(n*nblk + b)][3*C + 2]
  __shared__ double red[4][3 * C + 2];
  const long n = blockIdx.y;
  double acc[3 * C + 2];
#pragma unroll
  for (int i = 0; i < 3 * C + 2; ++i) acc[i] = 0;
  for (long hw = (long)blockIdx.x * 256 + threadIdx.x; hw < HW; hw += (long)nblk * 256) {
    int t;
    if constexpr (Ignore) {
      t = (int)tgt[n * HW + hw];
      if (t == (extra, ...)) continue;
    }
    float v[C];
    load_logits<C>(x, n, hw, HW, v);
    if constexpr (!Ignore) t = (int)tgt[n * HW + hw];
    float mx = v[0];
#pragma unroll
    for (int c = 1; c < C; ++c) mx = fmaxf(mx, v[c]);
    float e[C], sum = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      e[c] = expf(v[c] - mx);
      sum += e[c];
    }
    float xt = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const float sc = e[c] / sum;
      acc[c] += (c == t) ? (double)sc : 0.0;
      acc[C + c] += (double)sc;
      acc[2 * C + c] += (c == t) ? 1.0 : 0.0;
      xt = (c == t) ? v[c] : xt;
    }
    const float w = weight ? weight[t] : 1.f;
    acc[3 * C] += (double)(w * ((logf(sum) + mx) - xt));
    acc[3 * C + 1] += (double)w;
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < 3 * C + 2; ++i) {
    const double s = rs_wave_sum(acc[i]);
    if (lane == 0) red[wave][i] = s;
  }
  __syncthreads();
  if (threadIdx.x < 3 * C + 2) {
    const int i = threadIdx.x;
    partial[(n * nblk + blockIdx.x) * (3 * C + 2) + i] = (red[0][i] + red[1][i]) + (red[2][i] + red[3][i]);
  }
}

// The two finalize kernels stay two: they are different algorithms, not one body with a compare more.  The `_ig` form has to know
// whether an image has any valid pixel before it writes the image's coefficients, so it keeps A, B and cnt of all C classes in
// per-class arrays, and costs 16-53 % more for it (profiles/ignore_label/README.md); one template would either slow the plain
// path or be an `if constexpr` around two whole bodies.
//
// stats: [0] loss, [1] sum w, [2] branch (0 = miou, 1 = nll), [3 + n*C + c] = g for m=1, [3 + N*C + n*C + c] = g for m=0,
// [3 + 2*N*C] = the miou branch's value, [4 + 2*N*C] = the nll branch's numerator sum_i w_i l_i (data-parallel ranks
// exchange these two and [1] to take the reference's ONE branch decision over the global batch: robosat_amd/losses.py)
__global__ void miou_finalize_kernel(const double* __restrict__ partial, int N, int C, int nblk, float* __restrict__ loss,
                                     float* __restrict__ stats) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const int S = 3 * C + 2;
  double sl = 0, sw = 0, rsum = 0;
  for (int n = 0; n < N; ++n) {
    for (int c = 0; c < C; ++c) {
      double A = 0, B = 0, cnt = 0;
      for (int b = 0; b < nblk; ++b) {
        const double* p = partial + ((long)n * nblk + b) * S;
        A += p[c];
        B += p[C + c];
        cnt += p[2 * C + c];
      }
      const double U = B + cnt - A;
      rsum += A / U;
      const double k = 1.0 / ((double)C * (double)N);
      stats[3 + n * C + c] = (float)(-k / U);
      stats[3 + N * C + n * C + c] = (float)(k * A / (U * U));
    }
    for (int b = 0; b < nblk; ++b) {
      const double* p = partial + ((long)n * nblk + b) * S;
      sl += p[3 * C];
      sw += p[3 * C + 1];
    }
  }
  const float miou = (float)(1.0 - rsum / ((double)C * (double)N));
  const float nll = (float)(sl / sw);
  const bool use_nll = nll > miou;  // Python max(miou, nll): returns nll only if nll > miou
  loss[0] = use_nll ? nll : miou;
  stats[0] = loss[0];
  stats[1] = (float)sw;
  stats[2] = use_nll ? 1.f : 0.f;
  stats[3 + 2 * N * C] = miou;
  stats[4 + 2 * N * C] = (float)sl;
}

// miou_finalize_kernel with the stats layout kept.  An image with no valid pixel (sum_c cnt == 0) has ratio 1 and coefficients 0
// in every class -- no loss, no gradient -- and the mean stays over C * N terms; sum(w) == 0 gives nll = 0.
__global__ void miou_finalize_ig_kernel(const double* __restrict__ partial, int N, int C, int nblk, float* __restrict__ loss,
                                        float* __restrict__ stats) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const int S = 3 * C + 2;
  double sl = 0, sw = 0, rsum = 0;
  for (int n = 0; n < N; ++n) {
    // (one walk over the image's partials, as in miou_finalize_kernel: this thread is alone and every read is a round trip)
    double A[kMaxC], B[kMaxC], cnt[kMaxC], valid = 0;
    for (int c = 0; c < C; ++c) {
      A[c] = B[c] = cnt[c] = 0;
      for (int b = 0; b < nblk; ++b) {
        const double* p = partial + ((long)n * nblk + b) * S;
        A[c] += p[c];
        B[c] += p[C + c];
        cnt[c] += p[2 * C + c];
      }
      valid += cnt[c];
    }
    for (int c = 0; c < C; ++c) {
      if (valid == 0) {
        rsum += 1.0;
        stats[3 + n * C + c] = 0.f;
        stats[3 + N * C + n * C + c] = 0.f;
        continue;
      }
      const double U = B[c] + cnt[c] - A[c];
      rsum += A[c] / U;
      const double k = 1.0 / ((double)C * (double)N);
      stats[3 + n * C + c] = (float)(-k / U);
      stats[3 + N * C + n * C + c] = (float)(k * A[c] / (U * U));
    }
    for (int b = 0; b < nblk; ++b) {
      const double* p = partial + ((long)n * nblk + b) * S;
      sl += p[3 * C];
      sw += p[3 * C + 1];
    }
  }
  const float miou = (float)(1.0 - rsum / ((double)C * (double)N));
  const float nll = sw > 0.0 ? (float)(sl / sw) : 0.f;
  const bool use_nll = nll > miou;
  loss[0] = use_nll ? nll : miou;
  stats[0] = loss[0];
  stats[1] = (float)sw;
  stats[2] = use_nll ? 1.f : 0.f;
  stats[3 + 2 * N * C] = miou;
  stats[4 + 2 * N * C] = (float)sl;
}

template <int C, bool Ignore, typename... Extra>
__global__ __launch_bounds__(256) void miou_bwd_kernel(const float* __restrict__ x, const long long* __restrict__ tgt,
                                                       const float* __restrict__ weight, const float* __restrict__ stats,
                                                       const float* __restrict__ gout, float* __restrict__ dx, int N, long HW,
                                                       Extra... extra) {
  const long hw = (long)blockIdx.x * 256 + threadIdx.x;
  const long n = blockIdx.y;
  if (hw >= HW) return;
  int t;
  if constexpr (Ignore) {
    t = (int)tgt[n * HW + hw];
    if (t == (extra, ...)) {
#pragma unroll
      for (int c = 0; c < C; ++c) dx[(n * C + c) * HW + hw] = 0.f;
      return;
    }
  }
  float v[C], g[C];
  load_logits<C>(x, n, hw, HW, v);
  if constexpr (!Ignore) t = (int)tgt[n * HW + hw];
  const float go = gout ? gout[0] : 1.f;
  if (stats[2] > 0.5f) {
    const float w = weight ? weight[t] : 1.f;
    pixel_loss<C>(v, t, 0, 0.f, &g);
    const float k = go * w / stats[1];
#pragma unroll
    for (int c = 0; c < C; ++c) dx[(n * C + c) * HW + hw] = k * g[c];
    return;
  }
  float mx = v[0];
#pragma unroll
  for (int c = 1; c < C; ++c) mx = fmaxf(mx, v[c]);
  float sum = 0.f;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    v[c] = expf(v[c] - mx);
    sum += v[c];
  }
  float dot = 0.f;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    v[c] = v[c] / sum;
    g[c] = (c == t) ? stats[3 + n * C + c] : stats[3 + N * C + n * C + c];
    dot += g[c] * v[c];
  }
#pragma unroll
  for (int c = 0; c < C; ++c) dx[(n * C + c) * HW + hw] = go * v[c] * (g[c] - dot);
}

constexpr int kMiouBlocks = 64;  // per image

template <int C, bool Ignore, typename... Extra>
int run_miou_fwd(const float* x, const long long* t, const float* w, float* loss, float* stats, void* workspace, int N, int H, int W,
                 rs_stream_t stream, Extra... extra) {
  const long HW = (long)H * W, nb = (HW + 255) / 256;
  hipStream_t s = (hipStream_t)stream;
  double* part = reinterpret_cast<double*>(workspace);
  const int nblk = nb < kMiouBlocks ? (int)nb : kMiouBlocks;
  miou_partial_kernel<C, Ignore><<<dim3(nblk, N), 256, 0, s>>>(x, t, w, part, HW, nblk, extra...);
  if constexpr (Ignore) miou_finalize_ig_kernel<<<1, 64, 0, s>>>(part, N, C, nblk, loss, stats);
  else miou_finalize_kernel<<<1, 64, 0, s>>>(part, N, C, nblk, loss, stats);
  return RS_LAUNCH_RESULT();
}

template <int C, bool Ignore, typename... Extra>
int run_miou_bwd(const float* x, const long long* t, const float* w, const float* stats, const float* gout, float* dx, int N, int H,
                 int W, rs_stream_t stream, Extra... extra) {
  const long HW = (long)H * W;
  miou_bwd_kernel<C, Ignore><<<dim3(rs_cdiv(HW, 256), N), 256, 0, (hipStream_t)stream>>>(x, t, w, stats, gout, dx, N, HW, extra...);
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

// a variant's ignore label: none to check (Plain); no class and a label byte (Ignore); that, or -1 for "no pixel is ignored"
// (IgnoreWeight, and the weight plane itself)
bool ignore_ok(Px v, int ignore, int C) {
  if (v == Px::Plain) return true;
  return (v == Px::IgnoreWeight && ignore == -1) || (ignore >= C && ignore <= 255);
}

// What every entry point of the NLL and mIoU families refuses: a null among the pointers it requires (`weight` and `grad_out` may be
// null everywhere and are not among them), a shape or class count out of range, a mode that is neither CrossEntropy nor Focal (the
// mIoU entry points have none and pass 0), an ignore label its variant does not take.
bool loss_args_ok(std::initializer_list<const void*> required, int N, int C, int H, int W, int mode, Px v, int ignore) {
  for (const void* p : required)
    if (!p) return false;
  return N > 0 && C > 0 && C <= kMaxC && H > 0 && W > 0 && mode >= 0 && mode <= 1 && ignore_ok(v, ignore, C);
}

}  // namespace

extern "C" long rs_nll_loss_workspace_bytes(void) { return (long)kLossBlocks * 2 * (long)sizeof(double); }

extern "C" int rs_nll_loss_fwd(const float* logits, const long long* targets, const float* weight, float* loss, float* stats,
                               int N, int C, int H, int W, int mode, float gamma, void* workspace, rs_stream_t stream) {
  if (!loss_args_ok({logits, targets, loss, stats, workspace}, N, C, H, W, mode, Px::Plain, 0)) return RS_EINVAL;
  RS_DISPATCH_C(C, run_fwd<K, Px::Plain>(logits, targets, weight, loss, stats, workspace, N, H, W, mode, gamma, stream));
}

extern "C" int rs_nll_loss_fwd_ig(const float* logits, const long long* targets, const float* weight, float* loss, float* stats,
                                  int N, int C, int H, int W, int mode, float gamma, void* workspace, rs_stream_t stream,
                                  int ignore) {
  if (!loss_args_ok({logits, targets, loss, stats, workspace}, N, C, H, W, mode, Px::Ignore, ignore)) return RS_EINVAL;
  RS_DISPATCH_C(C, run_fwd<K, Px::Ignore>(logits, targets, weight, loss, stats, workspace, N, H, W, mode, gamma, stream, ignore));
}

extern "C" int rs_nll_loss_fwd_pw(const float* logits, const long long* targets, const float* weight, float* loss, float* stats,
                                  int N, int C, int H, int W, int mode, float gamma, void* workspace, rs_stream_t stream,
                                  const float* pixel_weight, int ignore) {
  if (!loss_args_ok({logits, targets, loss, stats, workspace, pixel_weight}, N, C, H, W, mode, Px::IgnoreWeight, ignore)) return RS_EINVAL;
  RS_DISPATCH_C(C, run_fwd<K, Px::IgnoreWeight>(logits, targets, weight, loss, stats, workspace, N, H, W, mode, gamma, stream,
                                                IgnoreAndWeight{ignore, pixel_weight}));
}

extern "C" int rs_nll_loss_bwd(const float* logits, const long long* targets, const float* weight, const float* stats,
                               const float* grad_out, float* dlogits, int N, int C, int H, int W, int mode, float gamma,
                               rs_stream_t stream) {
  if (!loss_args_ok({logits, targets, stats, dlogits}, N, C, H, W, mode, Px::Plain, 0)) return RS_EINVAL;
  RS_DISPATCH_C(C, run_bwd<K, Px::Plain>(logits, targets, weight, stats, grad_out, dlogits, N, H, W, mode, gamma, stream));
}

extern "C" int rs_nll_loss_bwd_ig(const float* logits, const long long* targets, const float* weight, const float* stats,
                                  const float* grad_out, float* dlogits, int N, int C, int H, int W, int mode, float gamma,
                                  rs_stream_t stream, int ignore) {
  if (!loss_args_ok({logits, targets, stats, dlogits}, N, C, H, W, mode, Px::Ignore, ignore)) return RS_EINVAL;
  RS_DISPATCH_C(C, run_bwd<K, Px::Ignore>(logits, targets, weight, stats, grad_out, dlogits, N, H, W, mode, gamma, stream, ignore));
}

extern "C" int rs_nll_loss_bwd_pw(const float* logits, const long long* targets, const float* weight, const float* stats,
                                  const float* grad_out, float* dlogits, int N, int C, int H, int W, int mode, float gamma,
                                  rs_stream_t stream, const float* pixel_weight, int ignore) {
  if (!loss_args_ok({logits, targets, stats, dlogits, pixel_weight}, N, C, H, W, mode, Px::IgnoreWeight, ignore)) return RS_EINVAL;
  RS_DISPATCH_C(C, run_bwd<K, Px::IgnoreWeight>(logits, targets, weight, stats, grad_out, dlogits, N, H, W, mode, gamma, stream,
                                                IgnoreAndWeight{ignore, pixel_weight}));
}

extern "C" int rs_confusion_counts(const float* scores, const long long* targets, unsigned long long* counts, int N, int C,
                                   int H, int W, rs_stream_t stream) {
  if (!scores || !targets || !counts || N <= 0 || C <= 0 || C > kMaxC || H <= 0 || W <= 0) return RS_EINVAL;
  const long HW = (long)H * W, P = (long)N * HW;
  hipStream_t s = (hipStream_t)stream;
  RS_DISPATCH_C(C, run_conf<K>(scores, targets, counts, P, HW, s));
}

extern "C" long rs_miou_loss_workspace_bytes(int N, int C) {
  if (N <= 0 || C <= 0 || C > kMaxC) return RS_EINVAL;
  return (long)N * kMiouBlocks * (3 * C + 2) * (long)sizeof(double);
}

extern "C" int rs_miou_loss_fwd(const float* logits, const long long* targets, const float* weight, float* loss, float* stats,
                                int N, int C, int H, int W, void* workspace, rs_stream_t stream) {
  if (!loss_args_ok({logits, targets, loss, stats, workspace}, N, C, H, W, 0, Px::Plain, 0)) return RS_EINVAL;
  RS_DISPATCH_C(C, run_miou_fwd<K, false>(logits, targets, weight, loss, stats, workspace, N, H, W, stream));
}

extern "C" int rs_miou_loss_fwd_ig(const float* logits, const long long* targets, const float* weight, float* loss, float* stats,
                                   int N, int C, int H, int W, void* workspace, rs_stream_t stream, int ignore) {
  if (!loss_args_ok({logits, targets, loss, stats, workspace}, N, C, H, W, 0, Px::Ignore, ignore)) return RS_EINVAL;
  RS_DISPATCH_C(C, run_miou_fwd<K, true>(logits, targets, weight, loss, stats, workspace, N, H, W, stream, ignore));
}

extern "C" int rs_miou_loss_bwd(const float* logits, const long long* targets, const float* weight, const float* stats,
                                const float* grad_out, float* dlogits, int N, int C, int H, int W, rs_stream_t stream) {
  if (!loss_args_ok({logits, targets, stats, dlogits}, N, C, H, W, 0, Px::Plain, 0)) return RS_EINVAL;
  RS_DISPATCH_C(C, run_miou_bwd<K, false>(logits, targets, weight, stats, grad_out, dlogits, N, H, W, stream));
}

extern "C" int rs_miou_loss_bwd_ig(const float* logits, const long long* targets, const float* weight, const float* stats,
                                   const float* grad_out, float* dlogits, int N, int C, int H, int W, rs_stream_t stream,
                                   int ignore) {
  if (!loss_args_ok({logits, targets, stats, dlogits}, N, C, H, W, 0, Px::Ignore, ignore)) return RS_EINVAL;
  RS_DISPATCH_C(C, run_miou_bwd<K, true>(logits, targets, weight, stats, grad_out, dlogits, N, H, W, stream, ignore));
}

// ---- the boundary weight plane (rs_boundary_weight_plane in include/robosat_hip.h) -------------------------------------------------
// The weight plane m [N][H][W] of the IgnoreWeight variant from the label raster in four launches: the complement of the boundary set
// as a byte mask, the two passes of rs_features_edt on it (features.hip, called as it is), the lookup d2 -> m.
namespace {

constexpr int kPlaneMaxR = 128;

// mask[p] = 0 at a boundary pixel (a valid pixel with a valid 4-neighbour of another label inside its image), 1 at any other valid
// pixel, 2 at an ignored one: non-zero = set for rs_features_edt, and the lookup needs no second look at the labels.  One thread per
// pixel; every neighbour read is guarded by its own row / column test, so W == 1 and H == 1 read nothing but the pixel itself.
__global__ __launch_bounds__(256) void boundary_mask_kernel(const long long* __restrict__ tgt, uint8_t* __restrict__ mask, long P,
                                                            int H, int W, long long ignore) {
  const long p = (long)blockIdx.x * 256 + threadIdx.x;
  if (p >= P) return;
  const long row = p / W;  // n * H + y
  const int x = (int)(p - row * W), y = (int)(row % H);
  const long long t = tgt[p];
  if (t == ignore) {
    mask[p] = 2;
    return;
  }
  bool edge = false;
  if (x > 0) {
    const long long q = tgt[p - 1];
    edge |= q != t && q != ignore;
  }
  if (x + 1 < W) {
    const long long q = tgt[p + 1];
    edge |= q != t && q != ignore;
  }
  if (y > 0) {
    const long long q = tgt[p - W];
    edge |= q != t && q != ignore;
  }
  if (y + 1 < H) {
    const long long q = tgt[p + W];
    edge |= q != t && q != ignore;
  }
  mask[p] = edge ? 0 : 1;
}

// m[p] = 0 at an ignored pixel, 1 at the cap, table[d2] below it (d2 < cap = R * R = the table's length)
__global__ __launch_bounds__(256) void boundary_lookup_kernel(const int* __restrict__ d2, const uint8_t* __restrict__ mask,
                                                              const float* __restrict__ table, float* __restrict__ m, long P, int cap) {
  const long p = (long)blockIdx.x * 256 + threadIdx.x;
  if (p >= P) return;
  const int d = d2[p];
  float v = 1.f;
  if (d >= 0 && d < cap) v = table[d];
  m[p] = mask[p] == 2 ? 0.f : v;
}

// (the sizes rs_features_edt takes: its own check refuses the rest, this one keeps the workspace query in step with it)
bool plane_shape_ok(int N, int H, int W) {
  return N > 0 && N <= 65535 && H > 0 && W > 0 && H <= 4096 && W <= 4096 && (long)N * H * W < (1l << 29);
}

}  // namespace

extern "C" long rs_boundary_weight_plane_workspace_bytes(int N, int H, int W) {
  if (!plane_shape_ok(N, H, W)) return RS_EINVAL;
  return 6 * (long)N * H * W;  // d2 int32, then the mask and g bytes
}

extern "C" int rs_boundary_weight_plane(const long long* targets, const float* table, float* plane, int N, int C, int H, int W, int R,
                                        int ignore, void* workspace, rs_stream_t stream) {
  if (!targets || !table || !plane || !workspace || ((uintptr_t)workspace & 3) || !plane_shape_ok(N, H, W) || C <= 0 || C > kMaxC ||
      R < 1 || R > kPlaneMaxR || !ignore_ok(Px::IgnoreWeight, ignore, C))
    return RS_EINVAL;
  const long P = (long)N * H * W;
  hipStream_t s = (hipStream_t)stream;
  int32_t* d2 = static_cast<int32_t*>(workspace);
  uint8_t* mask = reinterpret_cast<uint8_t*>(d2 + P);
  uint8_t* g = mask + P;
  boundary_mask_kernel<<<rs_cdiv(P, 256), 256, 0, s>>>(targets, mask, P, H, W, (long long)ignore);
  int rc = RS_LAUNCH_RESULT();
  if (rc) return rc;
  rc = rs_features_edt(mask, nullptr, g, d2, N, H, W, R, stream);
  if (rc) return rc;
  boundary_lookup_kernel<<<rs_cdiv(P, 256), 256, 0, s>>>(d2, mask, table, plane, P, R * R);
  return RS_LAUNCH_RESULT();
}
