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
  [[maybe_unused]] float pw = 0.f;
  if constexpr (V == Px::IgnoreWeight) {
    // a pixel of weight 0 -- one the hard-pixel plane drops -- is written like an ignored one: +0.0f in every class plane, where
    // 0 * g[c] would be -0.0f under a negative g[c]; its logits are not read
    pw = pixw[p];
    if (pw == 0.f) {
#pragma unroll
      for (int c = 0; c < C; ++c) dx[(n * C + c) * HW + hw] = 0.f;
      return;
    }
  }
  float v[C], g[C];
  load_logits<C>(x, n, hw, HW, v);
  if constexpr (V == Px::Plain) t = (int)tgt[p];
  float w;
  if constexpr (V == Px::IgnoreWeight) w = pw * (weight ? weight[t] : 1.f);
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

// ---- hard-pixel mining (rs_hard_pixel_plane / rs_hard_pixel_select in include/robosat_hip.h) -------------------------------------
// Per image the k-th largest of up to 2^31 - 1 uint32 keys, exactly, and the plane that keeps the pixels at or above it: the key
// plane (plane entry point only), then three rounds of [histogram of one digit of the valid keys that carry the prefix found so
// far; one small block per image that walks the bins from the top], 11 / 11 / 10 bits from the top, then the plane.  Every count is an
// integer sum, so the result depends on no order; the histograms are zeroed on the stream in every call, and nothing comes back to
// the host.
namespace {

constexpr int kHardThreads = 256;
constexpr int kHardMaxBins = 2048;
constexpr int kHardHistWords = 3 * kHardMaxBins;  // per image: one histogram per round
constexpr int kHardStateWords = 4;                // per image: prefix, remaining rank, and two words to spare
constexpr int kHardVoteRounds = 4;

// round R counts the digit (key >> shift) & (bins - 1) of the keys with key >> (shift + bits) == the prefix of the rounds before it
template <int R>
struct HardRound {
  static constexpr int bits = R == 2 ? 10 : 11;
  static constexpr int shift = R == 0 ? 21 : R == 1 ? 10 : 0;
  static constexpr int bins = 1 << bits;
};

// An image's pixels go to `bpi` blocks, `chunk` (a multiple of the block) consecutive ones each; block b of the launch works on image
// b / bpi.  Enough blocks to fill the device where the batch is small, at least 2048 pixels per block so that zeroing and flushing
// a histogram stay small beside counting.
struct HardGeom {
  int bpi;
  unsigned int chunk;
};

HardGeom hard_geom(int N, long HW) {
  long bpi = (HW + 2047) / 2048;
  const long want = (1024 + N - 1) / N;
  if (bpi > want) bpi = want;
  long chunk = (HW + bpi - 1) / bpi;
  chunk = (chunk + kHardThreads - 1) / kHardThreads * kHardThreads;
  bpi = (HW + chunk - 1) / chunk;  // (no empty block)
  return HardGeom{(int)bpi, (unsigned int)chunk};
}

// key = the bits of the unweighted cross-entropy where it is > 0, else 0 (-0.0f, a negative rounding result, NaN); 0 at an ignored
// pixel, whose logits are not read (its key counts nowhere: validity is decided from the label again).  One thread per pixel.
template <int C>
__global__ __launch_bounds__(kHardThreads) void hard_key_kernel(const float* __restrict__ x, const long long* __restrict__ tgt,
                                                                unsigned int* __restrict__ keys, long P, long HW, int ignore) {
  const long p = (long)blockIdx.x * kHardThreads + threadIdx.x;
  if (p >= P) return;
  const int t = (int)tgt[p];
  if (t == ignore) {
    keys[p] = 0u;
    return;
  }
  const long n = p / HW, hw = p - n * HW;
  float v[C];
  load_logits<C>(x, n, hw, HW, v);
  const float l = pixel_loss<C>(v, t, /*mode*/ 0, 0.f, nullptr);
  keys[p] = l > 0.f ? __float_as_uint(l) : 0u;
}

// The histograms of all three rounds start from zero in every call.  A kernel of the sequence, not a memset: a graph that holds the
// call then consists of kernel nodes alone, each ordered behind the one before it.
__global__ __launch_bounds__(kHardThreads) void hard_zero_kernel(unsigned int* __restrict__ words, long count) {
  const long i = (long)blockIdx.x * kHardThreads + threadIdx.x;
  if (i < count) words[i] = 0u;
}

// One count into the block's LDS histogram per lane that is `on`, with the lanes of a wave that hold the same digit added as one: up
// to kHardVoteRounds times the first lane still on names its digit, the lanes that hold it are counted by a ballot and leave, and that
// lane adds the count.  A trained network puts most pixels into one or two bins, which would otherwise be 64 LDS atomics on one
// address per wave and step; what is left after the votes are the rare digits, one atomic each.  Every lane of the wave calls this.
__device__ __forceinline__ void hard_vote_add(unsigned int* __restrict__ hist, bool on, unsigned int digit) {
  const int lane = threadIdx.x & 63;
  unsigned long long todo = __ballot(on);
  for (int r = 0; r < kHardVoteRounds && todo; ++r) {
    const int leader = __ffsll((long long)todo) - 1;
    const unsigned int d0 = (unsigned int)__shfl((int)digit, leader, 64);
    const unsigned long long same = __ballot(on && digit == d0);
    if (lane == leader) atomicAdd(&hist[d0], (unsigned int)__popcll(same));
    on = on && digit != d0;
    todo &= ~same;
  }
  if (on) atomicAdd(&hist[digit], 1u);
}

// ghist[image][round R][digit] += the block's counts: an LDS histogram, flushed with one integer atomic per non-empty bin.
template <int R>
__global__ __launch_bounds__(kHardThreads) void hard_hist_kernel(const unsigned int* __restrict__ keys, const long long* __restrict__ tgt,
                                                                 unsigned int* __restrict__ ghist, const unsigned int* __restrict__ state,
                                                                 unsigned int HW, int bpi, unsigned int chunk, int ignore) {
  using Rd = HardRound<R>;
  __shared__ unsigned int hist[Rd::bins];
  const int n = blockIdx.x / bpi, b = blockIdx.x - n * bpi;
  for (int i = threadIdx.x; i < Rd::bins; i += kHardThreads) hist[i] = 0;
  __syncthreads();
  [[maybe_unused]] unsigned int prefix = 0;
  if constexpr (R > 0) prefix = state[(long)n * kHardStateWords];
  const unsigned int lo = (unsigned int)b * chunk;
  const unsigned int hi = HW - lo < chunk ? HW : lo + chunk;  // (lo < HW: no block is empty)
  const long base = (long)n * HW;
  for (unsigned int at = lo; at < hi; at += kHardThreads) {  // (the whole wave makes every trip: hard_vote_add)
    const unsigned int hw = at + threadIdx.x;
    bool on = hw < hi;
    unsigned int key = 0;
    if (on) key = keys[base + hw];
    if constexpr (R > 0) on = on && (key >> (Rd::shift + Rd::bits)) == prefix;
    if (on && ignore >= 0) on = (int)tgt[base + hw] != ignore;
    hard_vote_add(hist, on, (key >> Rd::shift) & (Rd::bins - 1));
  }
  __syncthreads();
  unsigned int* out = ghist + (long)n * kHardHistWords + R * kHardMaxBins;
  for (int i = threadIdx.x; i < Rd::bins; i += kHardThreads) {
    const unsigned int c = hist[i];
    if (c) atomicAdd(&out[i], c);
  }
}

// One block per image: the digit of round R that holds the rank-th largest key, from the top bin down.  Thread t sums the
// bins/256 bins below bins - t * (bins/256), an exclusive scan over the threads gives the number of keys above its bins, and the one
// thread whose bins straddle the rank walks them.  Round 0 first makes V (the histogram's total: every valid key has a first digit)
// and k = min(V, max(1, ceil(fraction * V))), the rank to look for; the last round writes tau, capped, into info.
template <int R>
__global__ __launch_bounds__(kHardThreads) void hard_pick_kernel(const unsigned int* __restrict__ ghist, unsigned int* __restrict__ state,
                                                                 long long* __restrict__ info, double fraction, unsigned int cap) {
  using Rd = HardRound<R>;
  constexpr int per = Rd::bins / kHardThreads;
  __shared__ unsigned int scan[kHardThreads];
  const int n = blockIdx.x, t = threadIdx.x;
  const unsigned int* h = ghist + (long)n * kHardHistWords + R * kHardMaxBins;
  unsigned int* st = state + (long)n * kHardStateWords;
  unsigned int c[per], mine = 0;
#pragma unroll
  for (int j = 0; j < per; ++j) {
    c[j] = h[Rd::bins - 1 - (t * per + j)];
    mine += c[j];
  }
  scan[t] = mine;
  __syncthreads();
  for (int o = 1; o < kHardThreads; o <<= 1) {  // inclusive scan
    const unsigned int add = t >= o ? scan[t - o] : 0u;
    __syncthreads();
    scan[t] += add;
    __syncthreads();
  }
  const unsigned int above = scan[t] - mine;
  unsigned int rank, prefix = 0;
  if constexpr (R == 0) {
    const unsigned int V = scan[kHardThreads - 1];
    long long k = 0;
    if (V) {
      k = (long long)ceil(fraction * (double)V);
      k = k < 1 ? 1 : k;
      k = k > (long long)V ? (long long)V : k;
    }
    rank = (unsigned int)k;
    if (t == 0) {
      info[(long)n * 4] = (long long)V;
      info[(long)n * 4 + 1] = k;
      if (!V) st[0] = 0u, st[1] = 0u;
    }
  } else {
    rank = st[1];
    prefix = st[0];
  }
  __syncthreads();  // (every thread has read the state before one of them rewrites it)
  if (rank && above < rank && rank <= above + mine) {
    unsigned int acc = above;
#pragma unroll
    for (int j = 0; j < per; ++j) {
      if (acc < rank && rank <= acc + c[j]) {
        st[0] = (prefix << Rd::bits) | (unsigned int)(Rd::bins - 1 - (t * per + j));
        st[1] = rank - acc;
      }
      acc += c[j];
    }
  }
  if constexpr (R == 2) {
    __syncthreads();
    if (t == 0) {
      const unsigned int tau = st[0];  // (0 for an image without a valid pixel)
      info[(long)n * 4 + 2] = (long long)(tau < cap ? tau : cap);
      info[(long)n * 4 + 3] = 0;
    }
  }
}

// plane = base (1.0f without one) at a valid pixel with key >= tau, +0.0f anywhere else; info[n][3] += the number kept, one integer
// atomic per block.
__global__ __launch_bounds__(kHardThreads) void hard_plane_kernel(const unsigned int* __restrict__ keys, const long long* __restrict__ tgt,
                                                                  const float* __restrict__ basew, float* __restrict__ plane,
                                                                  long long* __restrict__ info, unsigned int HW, int bpi,
                                                                  unsigned int chunk, int ignore) {
  __shared__ unsigned int part[kHardThreads / 64];
  const int n = blockIdx.x / bpi, b = blockIdx.x - n * bpi;
  const unsigned int tau = (unsigned int)info[(long)n * 4 + 2];
  const bool any = info[(long)n * 4] > 0;
  const unsigned int lo = (unsigned int)b * chunk;
  const unsigned int hi = HW - lo < chunk ? HW : lo + chunk;
  const long base = (long)n * HW;
  unsigned int kept = 0;
  for (unsigned int hw = lo + threadIdx.x; hw < hi; hw += kHardThreads) {
    const long p = base + hw;
    bool keep = any && keys[p] >= tau;
    if (keep && ignore >= 0) keep = (int)tgt[p] != ignore;
    float v = 0.f;
    if (keep) v = basew ? basew[p] : 1.f;
    plane[p] = v;
    kept += keep ? 1u : 0u;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) kept += __shfl_xor(kept, o, 64);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = kept;
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned int tot = (part[0] + part[1]) + (part[2] + part[3]);
    if (tot) atomicAdd(reinterpret_cast<unsigned long long*>(info) + (long)n * 4 + 3, (unsigned long long)tot);
  }
}

// (an image's pixels are indexed by an unsigned int and counted in one; a launch's blocks by an int)
bool hard_shape_ok(int N, int H, int W) {
  if (N <= 0 || H <= 0 || W <= 0) return false;
  const long HW = (long)H * W;
  return HW < (1l << 31) && (long)N * ((HW + kHardThreads - 1) / kHardThreads) < (1l << 31);
}

// The fraction travels as the 64 bits of the double (the scalars of this ABI are int, long and float), the cap as a long that holds
// a uint32.
double hard_fraction_of(long bits) {
  static_assert(sizeof(long) == sizeof(double), "the fraction's bits travel in a long");
  double f;
  __builtin_memcpy(&f, &bits, sizeof f);
  return f;
}

bool hard_args_ok(int N, int H, int W, double fraction, long cap, int ignore, int C, const void* workspace) {
  return hard_shape_ok(N, H, W) && workspace && !((uintptr_t)workspace & 15) && fraction > 0.0 && fraction <= 1.0 &&  // (NaN fails both)
         cap >= 0 && cap <= 0xFFFFFFFFl && (ignore == -1 || (ignore >= C && ignore <= 255));
}

struct HardWorkspace {
  unsigned int* hist;
  unsigned int* state;
  unsigned int* keys;
};

HardWorkspace hard_carve(void* workspace, int N) {
  HardWorkspace ws;
  ws.hist = static_cast<unsigned int*>(workspace);
  ws.state = ws.hist + (long)N * kHardHistWords;
  ws.keys = ws.state + (long)N * kHardStateWords;
  return ws;
}

// the selection and the plane on the key plane `keys`: the histograms zeroed, three times (histogram, pick), the plane
int hard_select(const unsigned int* keys, const long long* t, const float* basew, float* plane, long long* info, int N, long HW,
                double fraction, unsigned int cap, int ignore, const HardWorkspace& ws, hipStream_t s) {
  const HardGeom g = hard_geom(N, HW);
  const int grid = N * g.bpi;
  hard_zero_kernel<<<rs_cdiv((long)N * kHardHistWords, kHardThreads), kHardThreads, 0, s>>>(ws.hist, (long)N * kHardHistWords);
  hard_hist_kernel<0><<<grid, kHardThreads, 0, s>>>(keys, t, ws.hist, ws.state, (unsigned int)HW, g.bpi, g.chunk, ignore);
  hard_pick_kernel<0><<<N, kHardThreads, 0, s>>>(ws.hist, ws.state, info, fraction, cap);
  hard_hist_kernel<1><<<grid, kHardThreads, 0, s>>>(keys, t, ws.hist, ws.state, (unsigned int)HW, g.bpi, g.chunk, ignore);
  hard_pick_kernel<1><<<N, kHardThreads, 0, s>>>(ws.hist, ws.state, info, fraction, cap);
  hard_hist_kernel<2><<<grid, kHardThreads, 0, s>>>(keys, t, ws.hist, ws.state, (unsigned int)HW, g.bpi, g.chunk, ignore);
  hard_pick_kernel<2><<<N, kHardThreads, 0, s>>>(ws.hist, ws.state, info, fraction, cap);
  hard_plane_kernel<<<grid, kHardThreads, 0, s>>>(keys, t, basew, plane, info, (unsigned int)HW, g.bpi, g.chunk, ignore);
  return RS_LAUNCH_RESULT();
}

template <int C>
int run_hard_keys(const float* x, const long long* t, unsigned int* keys, long P, long HW, int ignore, hipStream_t s) {
  hard_key_kernel<C><<<rs_cdiv(P, kHardThreads), kHardThreads, 0, s>>>(x, t, keys, P, HW, ignore);
  return RS_LAUNCH_RESULT();
}

int hard_keys(const float* x, const long long* t, unsigned int* keys, int C, long P, long HW, int ignore, hipStream_t s) {
  RS_DISPATCH_C(C, run_hard_keys<K>(x, t, keys, P, HW, ignore, s));
}

}  // namespace

extern "C" long rs_hard_pixel_workspace_bytes(int N, int H, int W) {
  if (!hard_shape_ok(N, H, W)) return RS_EINVAL;
  return ((long)N * (kHardHistWords + kHardStateWords) + (long)N * H * W) * (long)sizeof(unsigned int);
}

extern "C" int rs_hard_pixel_select(const unsigned* keys, const long long* targets, const float* base, float* plane, long long* info,
                                    int N, int H, int W, long fraction_bits, long cap, int ignore, void* workspace,
                                    rs_stream_t stream) {
  const double fraction = hard_fraction_of(fraction_bits);
  // (no class count here: the ignore label is -1 or a label byte; the labels are needed exactly where one is ignored)
  if (!keys || !plane || !info || !hard_args_ok(N, H, W, fraction, cap, ignore, 0, workspace) || (ignore >= 0 && !targets))
    return RS_EINVAL;
  return hard_select(keys, targets, base, plane, info, N, (long)H * W, fraction, (unsigned int)cap, ignore, hard_carve(workspace, N),
                     (hipStream_t)stream);
}

extern "C" int rs_hard_pixel_plane(const float* logits, const long long* targets, const float* base, float* plane, unsigned* keys_out,
                                   long long* info, int N, int C, int H, int W, long fraction_bits, long cap, int ignore,
                                   void* workspace, rs_stream_t stream) {
  const double fraction = hard_fraction_of(fraction_bits);
  if (!logits || !targets || !plane || !info || C <= 0 || C > kMaxC || !hard_args_ok(N, H, W, fraction, cap, ignore, C, workspace))
    return RS_EINVAL;
  const long HW = (long)H * W;
  hipStream_t s = (hipStream_t)stream;
  const HardWorkspace ws = hard_carve(workspace, N);
  unsigned int* keys = keys_out ? keys_out : ws.keys;
  const int rc = hard_keys(logits, targets, keys, C, (long)N * HW, HW, ignore, s);
  if (rc) return rc;
  return hard_select(keys, targets, base, plane, info, N, HW, fraction, (unsigned int)cap, ignore, ws, s);
}
