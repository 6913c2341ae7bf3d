// The Tversky loss family (Dice, soft Jaccard, focal Tversky) with a fused cross-entropy term, on NCHW logits [N][C][H][W] and int64
// label maps [N][H][W]: rs_tversky_sums / rs_tversky_finalize / rs_tversky_bwd in include/robosat_hip.h, DESIGN.md section 7g.
//
//   segment s = (image n, class c) per image, class c over the whole batch otherwise; over its valid pixels (label != ignore):
//   TP = sum_{t=c} p_c, SP = sum p_c, cnt = #{t=c};  TI = (TP + eps) / (TP + alpha (SP - TP) + beta (cnt - TP) + eps)
//   l_s = max(1 - TI, 0)^gamma;  T = the mean of l_s over the segments that count;  loss = T + lambda * weighted cross-entropy
//
// HBM-bound like loss.hip: one thread per pixel, plane-wise coalesced reads, every sum in fp64 and in a fixed order, no float atomics.
// The forward is three launches -- per-block partial sums, their reduction to the per-segment sums, the scalar stage -- so that
// data-parallel ranks can exchange the sums between the second and the third; the backward is one.
//
// The partial-sum kernel forms the sums miou_partial_kernel (loss.hip) forms, but is a kernel of its own: that one's instantiations
// keep their instructions (the header comment of loss.hip), and this one takes its ignore label as a run-time argument (-1 = none:
// no label equals it), reads the label in front of the logits in every call and so gives the same bits with and without one.
#include "common.h"

namespace {

constexpr int kTvMaxC = 8;
constexpr int kTvBlocks = 64;  // per image, as kMiouBlocks: 64 * 256 pixels per trip of the pixel loop

template <int C>
__device__ __forceinline__ void tv_load_logits(const float* __restrict__ x, long n, long hw, long HW, float (&v)[C]) {
#pragma unroll
  for (int c = 0; c < C; ++c) v[c] = x[(n * C + c) * HW + hw];
}

// partial[(n*nblk + b)][3*C + 2]: per class TP, SP, cnt of the block's valid pixels, then the cross-entropy numerator and denominator
template <int C>
__global__ __launch_bounds__(256) void tversky_partial_kernel(const float* __restrict__ x, const long long* __restrict__ tgt,
                                                              const float* __restrict__ weight, double* __restrict__ partial,
                                                              long HW, int nblk, int ignore) {
  __shared__ double red[4][3 * C + 2];
  const long n = blockIdx.y;
  double acc[3 * C + 2];
#pragma unroll
  for (int i = 0; i < 3 * C + 2; ++i) acc[i] = 0;
  for (long hw = (long)blockIdx.x * 256 + threadIdx.x; hw < HW; hw += (long)nblk * 256) {
    const int t = (int)tgt[n * HW + hw];
    if (t == ignore) continue;  // (its logits are not read)
    float v[C];
    tv_load_logits<C>(x, n, hw, HW, v);
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

// One block.  First every (image, entry) is summed over the image's blocks in ascending block order into img[n][3*C + 2]; then,
// per image, the class entries are laid out as sums[(n*C + c)*3 + {TP, SP, cnt}] and the two cross-entropy sums are added over the
// images in ascending order into sums[3*N*C], sums[3*N*C + 1]; for the batch form every entry is added over the images in ascending
// order into sums[c*3 + k], sums[3*C], sums[3*C + 1].
__global__ __launch_bounds__(256) void tversky_reduce_kernel(const double* __restrict__ partial, double* __restrict__ img,
                                                             double* __restrict__ sums, int N, int C, int nblk, int per_image) {
  const int S = 3 * C + 2;
  const long items = (long)N * S;
  for (long it = threadIdx.x; it < items; it += 256) {
    const long n = it / S;
    const int i = (int)(it - n * S);
    const double* p = partial + n * nblk * S + i;
    double s = 0;
    for (int b = 0; b < nblk; ++b) s += p[(long)b * S];
    img[it] = s;
  }
  __syncthreads();  // (img is read back by other threads of this block)
  // entry i of an image's row: class c = i % C of kind k = i / C for i < 3*C, then the two cross-entropy sums
  if (per_image) {
    for (long it = threadIdx.x; it < items; it += 256) {
      const long n = it / S;
      const int i = (int)(it - n * S);
      if (i < 3 * C) sums[(n * C + i % C) * 3 + i / C] = img[it];
    }
    if (threadIdx.x < 2) {
      double s = 0;
      for (int n = 0; n < N; ++n) s += img[(long)n * S + 3 * C + threadIdx.x];
      sums[3l * N * C + threadIdx.x] = s;
    }
  } else if (threadIdx.x < S) {
    const int i = threadIdx.x;
    double s = 0;
    for (int n = 0; n < N; ++n) s += img[(long)n * S + i];
    sums[i < 3 * C ? (i % C) * 3 + i / C : i] = s;
  }
}

struct TvParams {
  float alpha, beta, gamma, eps, lambda;
  int all_classes, per_image, world;
};

// The segments of one group -- the C classes of an image, or of the whole batch: the group's mean of l_s over the classes that count,
// and per class the two coefficients d loss / d p_c (for a pixel with t == c: g1, with t != c: g0), `scale` / (classes that count) each.
__device__ double tversky_group(const double* __restrict__ seg, int C, const TvParams& q, double scale, float* __restrict__ g1,
                                float* __restrict__ g0) {
  double valid = 0;
  int present = 0;
  for (int c = 0; c < C; ++c) {
    valid += seg[c * 3 + 2];
    present += seg[c * 3 + 2] > 0.0 ? 1 : 0;
  }
  const int np = q.all_classes ? (valid > 0.0 ? C : 0) : present;
  const double a = (double)q.alpha, b = (double)q.beta, gm = (double)q.gamma, eps = (double)q.eps;
  double tsum = 0;
  for (int c = 0; c < C; ++c) {
    const double TP = seg[c * 3], SP = seg[c * 3 + 1], cnt = seg[c * 3 + 2];
    const bool counts = q.all_classes ? valid > 0.0 : cnt > 0.0;
    double c1 = 0, c0 = 0;
    if (counts) {
      const double num = TP + eps;
      const double den = TP + a * (SP - TP) + b * (cnt - TP) + eps;
      if (den > 0.0) {  // (den == 0: TI = 1, l = 0, no gradient)
        const double u = 1.0 - num / den;
        double l, dl;  // l = max(u, 0)^gamma, dl = d l / d TI
        if (u > 0.0) {
          l = q.gamma == 1.f ? u : pow(u, gm);
          dl = q.gamma == 1.f ? -1.0 : -gm * pow(u, gm - 1.0);
        } else {
          l = 0.0;
          dl = q.gamma == 1.f ? -1.0 : 0.0;
        }
        tsum += l;
        const double k = scale * dl / ((double)np * den * den);
        c1 = k * (den - num * (1.0 - b));  // d TI / d p_c at a pixel of the class: through TP and SP
        c0 = k * (-a * num);               // ... at any other valid pixel: through SP only
      }
    }
    g1[c] = (float)c1;
    g0[c] = (float)c0;
  }
  return np ? tsum / (double)np : 0.0;
}

// stats: [0] loss, [1] T, [2] the cross-entropy numerator, [3] the denominator the backward divides by (sums' / world),
// [4 + s] g1 of segment s, [4 + S + s] g0, S = N*C per image and C otherwise.  One block; the images' terms are added by a tree
// over the threads: a fixed order.
__global__ __launch_bounds__(256) void tversky_finalize_kernel(const double* __restrict__ sums, float* __restrict__ loss,
                                                               float* __restrict__ stats, int N, int C, TvParams q) {
  __shared__ double red[256];
  const int groups = q.per_image ? N : 1;
  const int S = groups * C;
  // per image: T = (1/N) sum_n mean_c l; batch: T = mean_c l, and the coefficients times world (the ranks' gradients are averaged)
  const double scale = q.per_image ? 1.0 / (double)N : (double)q.world;
  double t = 0;
  for (int g = threadIdx.x; g < groups; g += 256)
    t += tversky_group(sums + (long)g * C * 3, C, q, scale, stats + 4 + (long)g * C, stats + 4 + S + (long)g * C);
  red[threadIdx.x] = t;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const double T = q.per_image ? red[0] / (double)N : red[0];
    const double num = sums[3l * S], den = sums[3l * S + 1];
    const double den_bwd = den / (double)q.world;
    // per image `num` is the rank's own and the ranks' losses are averaged; in the batch form it is the global one already
    double ce = 0;
    if (q.lambda > 0.f && den > 0.0) ce = (double)q.lambda * (q.per_image ? num / den_bwd : num / den);
    const float l = (float)(T + ce);
    loss[0] = l;
    stats[0] = l;
    stats[1] = (float)T;
    stats[2] = (float)num;
    stats[3] = (float)den_bwd;
  }
}

// dx[c][p] = gout * ( p_c (g_c - sum_j p_j g_j) + lambda w[t] (p_c - 1[c == t]) / den ), g_c = g1 or g0 of the pixel's segment of class c
template <int C>
__global__ __launch_bounds__(256) void tversky_bwd_kernel(const float* __restrict__ x, const long long* __restrict__ tgt,
                                                          const float* __restrict__ weight, const float* __restrict__ stats,
                                                          const float* __restrict__ gout, float* __restrict__ dx, int N, long HW,
                                                          int per_image, float lambda, int ignore) {
  const long hw = (long)blockIdx.x * 256 + threadIdx.x;
  const long n = blockIdx.y;
  if (hw >= HW) return;
  const int t = (int)tgt[n * HW + hw];
  if (t == ignore) {
#pragma unroll
    for (int c = 0; c < C; ++c) dx[(n * C + c) * HW + hw] = 0.f;
    return;
  }
  float v[C], g[C];
  tv_load_logits<C>(x, n, hw, HW, v);
  const float go = gout ? gout[0] : 1.f;
  const int S = per_image ? N * C : C;
  const float* g1 = stats + 4 + (per_image ? n * C : 0);
  const float* g0 = g1 + S;
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
    g[c] = (c == t) ? g1[c] : g0[c];
    dot += g[c] * v[c];
  }
  const float den = stats[3];
  if (lambda > 0.f && den > 0.f) {
    const float k = lambda * (weight ? weight[t] : 1.f) / den;
#pragma unroll
    for (int c = 0; c < C; ++c) dx[(n * C + c) * HW + hw] = go * (v[c] * (g[c] - dot) + k * (v[c] - (c == t ? 1.f : 0.f)));
    return;
  }
#pragma unroll
  for (int c = 0; c < C; ++c) dx[(n * C + c) * HW + hw] = go * v[c] * (g[c] - dot);
}

int tv_blocks(long HW) {
  const long nb = (HW + 255) / 256;
  return nb < kTvBlocks ? (int)nb : kTvBlocks;
}

template <int C>
int run_tversky_partial(const float* x, const long long* t, const float* w, double* part, int N, long HW, int ignore, hipStream_t s) {
  const int nblk = tv_blocks(HW);
  tversky_partial_kernel<C><<<dim3(nblk, N), 256, 0, s>>>(x, t, w, part, HW, nblk, ignore);
  return RS_LAUNCH_RESULT();
}

template <int C>
int run_tversky_bwd(const float* x, const long long* t, const float* w, const float* stats, const float* gout, float* dx, int N, long HW,
                    int per_image, float lambda, int ignore, hipStream_t s) {
  tversky_bwd_kernel<C><<<dim3(rs_cdiv(HW, 256), N), 256, 0, s>>>(x, t, w, stats, gout, dx, N, HW, per_image, lambda, ignore);
  return RS_LAUNCH_RESULT();
}

#define RS_TV_DISPATCH_C(C, ...)                          \
  switch (C) {                                            \
    case 2: { constexpr int K = 2; return __VA_ARGS__; }  \
    case 3: { constexpr int K = 3; return __VA_ARGS__; }  \
    case 4: { constexpr int K = 4; return __VA_ARGS__; }  \
    case 5: { constexpr int K = 5; return __VA_ARGS__; }  \
    case 6: { constexpr int K = 6; return __VA_ARGS__; }  \
    case 7: { constexpr int K = 7; return __VA_ARGS__; }  \
    default: { constexpr int K = 8; return __VA_ARGS__; } \
  }

// 2 <= C <= 8, positive sizes, N*C*H*W < 2^31 (and N within a launch's y dimension), an ignore label that is -1 or no class and a byte
bool tv_shape_ok(int N, int C, int H, int W, int ignore) {
  if (N <= 0 || N > 65535 || C < 2 || C > kTvMaxC || H <= 0 || W <= 0) return false;
  if ((long)N * C * H * W >= (1l << 31)) return false;
  return ignore == -1 || (ignore >= C && ignore <= 255);
}

bool tv_finite(float v) { return v - v == 0.f; }

}  // namespace

extern "C" long rs_tversky_workspace_bytes(int N, int C) {
  if (N <= 0 || N > 65535 || C < 2 || C > kTvMaxC) return RS_EINVAL;
  return (long)N * (kTvBlocks + 1) * (3 * C + 2) * (long)sizeof(double);
}

extern "C" int rs_tversky_sums(const float* logits, const long long* targets, const float* weight, double* sums, int N, int C, int H,
                               int W, int per_image, int ignore, void* workspace, rs_stream_t stream) {
  if (!logits || !targets || !sums || !workspace || ((uintptr_t)workspace & 7) || !tv_shape_ok(N, C, H, W, ignore)) return RS_EINVAL;
  const long HW = (long)H * W;
  hipStream_t s = (hipStream_t)stream;
  double* part = static_cast<double*>(workspace);
  double* img = part + (long)N * kTvBlocks * (3 * C + 2);
  const int rc = [&]() -> int { RS_TV_DISPATCH_C(C, run_tversky_partial<K>(logits, targets, weight, part, N, HW, ignore, s)); }();
  if (rc) return rc;
  tversky_reduce_kernel<<<1, 256, 0, s>>>(part, img, sums, N, C, tv_blocks(HW), per_image ? 1 : 0);
  return RS_LAUNCH_RESULT();
}

extern "C" int rs_tversky_finalize(const double* sums, float* loss, float* stats, int N, int C, float alpha, float beta, float gamma,
                                   float eps, float lambda, int all_classes, int per_image, int world, rs_stream_t stream) {
  if (!sums || !loss || !stats || N <= 0 || N > 65535 || C < 2 || C > kTvMaxC || world < 1) return RS_EINVAL;
  if (!tv_finite(alpha) || !tv_finite(beta) || !tv_finite(gamma) || !tv_finite(eps) || !tv_finite(lambda)) return RS_EINVAL;
  if (alpha < 0.f || beta < 0.f || (alpha == 0.f && beta == 0.f) || !(gamma > 0.f) || eps < 0.f || lambda < 0.f) return RS_EINVAL;
  const TvParams q{alpha, beta, gamma, eps, lambda, all_classes ? 1 : 0, per_image ? 1 : 0, world};
  tversky_finalize_kernel<<<1, 256, 0, (hipStream_t)stream>>>(sums, loss, stats, N, C, q);
  return RS_LAUNCH_RESULT();
}

extern "C" int rs_tversky_bwd(const float* logits, const long long* targets, const float* weight, const float* stats,
                              const float* grad_out, float* dlogits, int N, int C, int H, int W, int per_image, float lambda, int ignore,
                              rs_stream_t stream) {
  if (!logits || !targets || !stats || !dlogits || !tv_shape_ok(N, C, H, W, ignore) || !tv_finite(lambda) || lambda < 0.f)
    return RS_EINVAL;
  RS_TV_DISPATCH_C(C, run_tversky_bwd<K>(logits, targets, weight, stats, grad_out, dlogits, N, (long)H * W, per_image ? 1 : 0, lambda,
                                         ignore, (hipStream_t)stream));
}
