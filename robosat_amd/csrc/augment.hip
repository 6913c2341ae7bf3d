// Training-set augmentation beyond the reference's eight views (an extension; the `[augment]` table of the model config):
//
//   rs_tile_band_sums        sum of every band of every uint8 tile: what the contrast stage's band means are made of
//   rs_augment_tiles_jitter  rs_augment_tiles (postproc.hip) + a zoom-in window (image bilinear, mask nearest, integer
//                            coordinates) + brightness / contrast / saturation / gamma, still one pass from the bytes
//   rs_augment_tiles_rotate  the same with the window turned about its centre by any angle (fixed-point coordinates, the tile
//                            mirrored about its edges where the turned window leaves it)
//
// The definitions are in include/robosat_hip.h; tests/augment_ref.py and tests/augment_rotate_ref.py restate them in float64.
#include "common.h"

namespace {

// ---- band sums -------------------------------------------------------------------------------------------------------------
// The T tiles are one run of T*L bytes (L = S*S*C, a multiple of C: the band of byte g is g % C).  A block takes kSumSpan bytes of
// that run, cut at 16-byte ADDRESSES (the base may be any address: a slice of a larger tensor, or L no multiple of 16), and walks the
// tiles its span touches: per tile, 16 bytes per lane and load for the aligned inside, single bytes for the at most 15 + 15 at the
// two ends.  Per tile: uint32 per thread -> wave (shuffles) -> block (LDS) -> one 64-bit integer atomic per band.  Integers only:
// every run gives the same bits.
constexpr int kSumSpan = 64 * 1024;

template <int C>
__device__ __forceinline__ void sum_vec16(const u32x4 q, int r, unsigned int (&acc)[4]) {
  // p[k]: bytes of the vector at positions j with j % C == k; the vector starts at band r, so band c holds p[(c - r) mod C]
  unsigned int p[4] = {0, 0, 0, 0};
#pragma unroll
  for (int j = 0; j < 16; ++j) p[j % C] += (q[j >> 2] >> (8 * (j & 3))) & 255u;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    unsigned int v = p[0];
#pragma unroll
    for (int k = 1; k < C; ++k) v = ((c - r + C) % C == k) ? p[k] : v;
    acc[c] += v;
  }
}

template <int C>
__global__ __launch_bounds__(256) void band_sums_kernel(const uint8_t* __restrict__ images, unsigned long long* __restrict__ sums, long L,
                                                        long total) {
  __shared__ unsigned int part[4][4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  // u = g + mis: byte g of the run sits at an address that is u modulo 16
  const long mis = (long)((uintptr_t)images & 15);
  const long u0 = (long)blockIdx.x * kSumSpan, u1 = u0 + kSumSpan;
  const long g_lo = (u0 > mis ? u0 : mis) - mis, g_hi = (u1 < mis + total ? u1 : mis + total) - mis;
  if (g_lo >= g_hi) return;
  for (long t = g_lo / L; t * L < g_hi; ++t) {
    const long a = t * L > g_lo ? t * L : g_lo, e = (t + 1) * L < g_hi ? (t + 1) * L : g_hi;  // this block's bytes of tile t
    long va = ((a + mis + 15) & ~15L) - mis, ve = ((e + mis) & ~15L) - mis;                   // its whole 16-byte vectors
    if (va >= ve) va = ve = e;
    unsigned int acc[4] = {0, 0, 0, 0};
    for (long g = a + threadIdx.x; g < va; g += 256) {  // (at most 15 bytes, or the whole piece when it holds no vector)
      const unsigned int b = images[g];
      const int r = (int)(g % C);
#pragma unroll
      for (int c = 0; c < C; ++c) acc[c] += r == c ? b : 0u;
    }
    for (long g = ve + threadIdx.x; g < e; g += 256) {
      const unsigned int b = images[g];
      const int r = (int)(g % C);
#pragma unroll
      for (int c = 0; c < C; ++c) acc[c] += r == c ? b : 0u;
    }
    const u32x4* vp = reinterpret_cast<const u32x4*>(images + va);
    const int nvec = (int)((ve - va) >> 4);  // (at most kSumSpan / 16)
    const int r0 = (int)(va % C);
#pragma unroll 4
    for (int i = threadIdx.x; i < nvec; i += 256) sum_vec16<C>(vp[i], (r0 + i * (16 % C)) % C, acc);
#pragma unroll
    for (int c = 0; c < C; ++c) {
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) acc[c] += __shfl_xor(acc[c], o, 64);
      if (lane == 0) part[wave][c] = acc[c];
    }
    rs_lds_writes_done();
    __syncthreads();
    if (threadIdx.x < C) {
      const unsigned int tot = part[0][threadIdx.x] + part[1][threadIdx.x] + part[2][threadIdx.x] + part[3][threadIdx.x];
      if (tot) atomicAdd(&sums[t * C + threadIdx.x], (unsigned long long)tot);
    }
    __syncthreads();  // (part is written again for the next tile of this block)
  }
}

// ---- zoom + colour jitter ----------------------------------------------------------------------------------------------------
// One launch takes up to kJitItems items; their windows and factors travel in the kernel arguments (they are host values the
// entry point has validated), so a block reads its item's from scalar registers and every per-item branch is uniform.
constexpr int kJitItems = 64;

struct JitArgs {
  const uint8_t* images;       // [T][S][S][C]
  const uint8_t* masks;        // [T][S][S] (may be NULL)
  const int* index;            // [N] tile of the cache
  const int* op;               // [N]
  const long long* band_sums;  // [T][C] (may be NULL when no item has contrast)
  float* out;                  // [N][C][S][S]
  long long* out_mask;         // [N][S][S]
  float mean[4], stdv[4];
  rs_fastdiv div2s;  // by 2*S
  int S, rgb, al4, bpi;  // bpi: blocks per item
  int geom[kJitItems][3];     // (w, x0, y0)
  float color[kJitItems][4];  // (brightness, contrast, saturation, gamma)
};

__device__ __forceinline__ float clamp01(float v) { return fminf(fmaxf(v, 0.0f), 1.0f); }

template <int C>
__device__ __forceinline__ void load_px(const uint8_t* p, bool al4, float (&v)[C]) {
  if constexpr (C == 4) {
    if (al4) {
      const unsigned int w = *reinterpret_cast<const unsigned int*>(p);
      v[0] = (float)(w & 255u), v[1] = (float)((w >> 8) & 255u), v[2] = (float)((w >> 16) & 255u), v[3] = (float)(w >> 24);
      return;
    }
  }
#pragma unroll
  for (int c = 0; c < C; ++c) v[c] = (float)p[c];
}

// frame index j -> the two taps (relative to the window) and the weight of the second (half-pixel centres, taps clamped to the window)
__device__ __forceinline__ void bilinear_taps(int j, int w, int S, const rs_fastdiv d, int& i0, int& i1, float& f) {
  const int t = max((2 * j + 1) * w - S, 0);
  i0 = (int)rs_div((unsigned int)t, d);
  f = (float)(t - i0 * 2 * S) / (float)(2 * S);
  i1 = min(i0 + 1, w - 1);
}

template <int C, int V>
__global__ __launch_bounds__(256) void jitter_kernel(const JitArgs a) {
  const int S = a.S;
  const long SS = (long)S * S;
  const int n = blockIdx.x / a.bpi;  // one item per block
  const int q = (blockIdx.x - n * a.bpi) * 256 + threadIdx.x;
  const int w = a.geom[n][0], wx = a.geom[n][1], wy = a.geom[n][2];
  const float fb = a.color[n][0], fk = a.color[n][1], fs = a.color[n][2], fg = a.color[n][3];
  const int op = a.op[n];
  const long tile = a.index[n];
  const bool sat = a.rgb && fs != 1.0f;

  float bm[C];  // band means of the source tile, in ToTensor's units
  if (fk != 1.0f) {
    // lane l divides for band l & 3 (in float64: the quotient of two integers, rounded once), the others fetch it
    const int lc = min((int)threadIdx.x & 3, C - 1);
    const float m = (float)((double)a.band_sums[tile * C + lc] / ((double)SS * 255.0));
#pragma unroll
    for (int c = 0; c < C; ++c) bm[c] = __shfl(m, c, 4);
  }
  const int per_row = S / V;
  if (q >= S * per_row) return;
  const int yo = q / per_row, xo = (q - yo * per_row) * V;

  const uint8_t* img = a.images + tile * SS * C;
  const uint8_t* msk = a.masks ? a.masks + tile * SS : nullptr;
  float res[C][V];
  long long lab[V] = {};
#pragma unroll
  for (int e = 0; e < V; ++e) {
    int y = yo, x = xo + e;
    for (int r = (op >> 1) & 3; r > 0; --r) {  // undo the rotations, last first
      const int py = x, px = S - 1 - y;
      y = py;
      x = px;
    }
    if (op & 1) x = S - 1 - x;
    float v[C];
    if (w == S) {  // no zoom: the byte itself
      const long src = (long)y * S + x;
      load_px<C>(img + src * C, a.al4, v);
      if (msk) lab[e] = (long long)msk[src];
    } else {
      int xa, xb, ya, yb;
      float fx, fy;
      bilinear_taps(x, w, S, a.div2s, xa, xb, fx);
      bilinear_taps(y, w, S, a.div2s, ya, yb, fy);
      const uint8_t* r0 = img + ((long)(wy + ya) * S + wx) * C;
      const uint8_t* r1 = img + ((long)(wy + yb) * S + wx) * C;
      float p00[C], p01[C], p10[C], p11[C];
      load_px<C>(r0 + xa * C, a.al4, p00);
      load_px<C>(r0 + xb * C, a.al4, p01);
      load_px<C>(r1 + xa * C, a.al4, p10);
      load_px<C>(r1 + xb * C, a.al4, p11);
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const float top = p00[c] + fx * (p01[c] - p00[c]), bot = p10[c] + fx * (p11[c] - p10[c]);
        v[c] = top + fy * (bot - top);
      }
      if (msk) {
        const int mx = wx + (int)rs_div((unsigned int)((2 * x + 1) * w), a.div2s);
        const int my = wy + (int)rs_div((unsigned int)((2 * y + 1) * w), a.div2s);
        lab[e] = (long long)msk[(long)my * S + mx];
      }
    }
#pragma unroll
    for (int c = 0; c < C; ++c) v[c] = v[c] / 255.0f;
    if (fb != 1.0f) {
#pragma unroll
      for (int c = 0; c < C; ++c) v[c] = clamp01(v[c] * fb);
    }
    if (fk != 1.0f) {
#pragma unroll
      for (int c = 0; c < C; ++c) v[c] = clamp01(bm[c] + fk * (v[c] - bm[c]));
    }
    if constexpr (C >= 3) {
      if (sat) {
        const float g = 0.299f * v[0] + 0.587f * v[1] + 0.114f * v[2];
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = clamp01(g + fs * (v[c] - g));
      }
    }
    if (fg != 1.0f) {
#pragma unroll
      for (int c = 0; c < C; ++c) v[c] = clamp01(powf(v[c], fg));
    }
#pragma unroll
    for (int c = 0; c < C; ++c) res[c][e] = (v[c] - a.mean[c]) / a.stdv[c];
  }

  const long rem = (long)yo * S + xo;
  float* dst = a.out + (long)n * C * SS + rem;
  if constexpr (V == 4) {
#pragma unroll
    for (int c = 0; c < C; ++c) *reinterpret_cast<f32x4*>(dst + c * SS) = f32x4{res[c][0], res[c][1], res[c][2], res[c][3]};
    if (msk) {
      typedef long long s64x2 __attribute__((ext_vector_type(2)));
      s64x2* mp = reinterpret_cast<s64x2*>(a.out_mask + (long)n * SS + rem);
      mp[0] = s64x2{lab[0], lab[1]};
      mp[1] = s64x2{lab[2], lab[3]};
    }
  } else {
#pragma unroll
    for (int c = 0; c < C; ++c) dst[c * SS] = res[c][0];
    if (msk) a.out_mask[(long)n * SS + rem] = lab[0];
  }
}

template <int C>
int launch_jitter(const JitArgs& a, bool vec, int blocks, hipStream_t stream) {
  if (vec)
    jitter_kernel<C, 4><<<blocks, 256, 0, stream>>>(a);
  else
    jitter_kernel<C, 1><<<blocks, 256, 0, stream>>>(a);
  return RS_LAUNCH_RESULT();
}

// ---- zoom + free rotation + colour jitter ----------------------------------------------------------------------------------
// jitter_kernel's shape (one item per block, V pixels of an output row per thread, coalesced stores) with the source position
// of every pixel in 64-bit fixed point (the header's Ux, Uy: 2^-17 source pixels).  A and B are made once per item on the host,
// so a pixel costs no division: along an output row the position advances by a step that is uniform over the block.  The taps
// are gathers of bytes from a tile that sits in L2.
struct RotArgs {
  const uint8_t* images;       // [T][S][S][C]
  const uint8_t* masks;        // [T][S][S] (may be NULL)
  const int* index;            // [N] tile of the cache
  const int* op;               // [N]
  const long long* band_sums;  // [T][C] (may be NULL when no item has contrast)
  float* out;                  // [N][C][S][S]
  long long* out_mask;         // [N][S][S]
  float mean[4], stdv[4];
  int S, rgb, al4, bpi;  // bpi: blocks per item
  int geom[kJitItems][3];     // (w, x0, y0)
  int ab[kJitItems][2];       // (A, B): the window's scale times the angle's cosine and sine, in units of 2^-16
  float color[kJitItems][4];  // (brightness, contrast, saturation, gamma)
};

// the tile mirrored about its edges, the edge pixel repeated (one fold: the entry point admits no sample a whole tile outside)
__device__ __forceinline__ int fold(int i, int S) { return i < 0 ? -1 - i : (i >= S ? 2 * S - 1 - i : i); }

// output pixel (yo, xo) -> frame pixel (y, x) with the view `op` undone, rotations last first (as jitter_kernel does inline)
__device__ __forceinline__ void undo_view(int op, int S, int yo, int xo, int& y, int& x) {
  y = yo, x = xo;
  for (int r = (op >> 1) & 3; r > 0; --r) {
    const int py = x, px = S - 1 - y;
    y = py;
    x = px;
  }
  if (op & 1) x = S - 1 - x;
}

template <int C, int V>
__global__ __launch_bounds__(256) void rotate_kernel(const RotArgs a) {
  const int S = a.S;
  const long SS = (long)S * S;
  const int n = blockIdx.x / a.bpi;  // one item per block
  const int q = (blockIdx.x - n * a.bpi) * 256 + threadIdx.x;
  const int w = a.geom[n][0];
  const long long A = a.ab[n][0], B = a.ab[n][1];
  const long long cx = (long long)(2 * a.geom[n][1] + w) << 16, cy = (long long)(2 * a.geom[n][2] + w) << 16;
  const float fb = a.color[n][0], fk = a.color[n][1], fs = a.color[n][2], fg = a.color[n][3];
  const int op = a.op[n];
  const long tile = a.index[n];
  const bool sat = a.rgb && fs != 1.0f;

  float bm[C];  // band means of the source tile, in ToTensor's units (as in jitter_kernel)
  if (fk != 1.0f) {
    const int lc = min((int)threadIdx.x & 3, C - 1);
    const float m = (float)((double)a.band_sums[tile * C + lc] / ((double)SS * 255.0));
#pragma unroll
    for (int c = 0; c < C; ++c) bm[c] = __shfl(m, c, 4);
  }
  const int per_row = S / V;
  if (q >= S * per_row) return;
  const int yo = q / per_row, xo = (q - yo * per_row) * V;

  // the frame pixel of this thread's first output pixel, and the frame step of one output pixel to the right (uniform)
  int y, x, y0, x0, y1, x1;
  undo_view(op, S, yo, xo, y, x);
  undo_view(op, S, 0, 0, y0, x0);
  undo_view(op, S, 0, 1, y1, x1);
  const long long sx = x1 - x0, sy = y1 - y0;
  const long long dx = 2 * x + 1 - S, dy = 2 * y + 1 - S;
  long long ux = A * dx - B * dy + cx, uy = B * dx + A * dy + cy;
  const long long stepx = 2 * (A * sx - B * sy), stepy = 2 * (B * sx + A * sy);

  const uint8_t* img = a.images + tile * SS * C;
  const uint8_t* msk = a.masks ? a.masks + tile * SS : nullptr;
  float res[C][V];
  long long lab[V] = {};
#pragma unroll
  for (int e = 0; e < V; ++e) {
    if (msk) lab[e] = (long long)msk[(long)fold((int)(uy >> 17), S) * S + fold((int)(ux >> 17), S)];
    const long long tx = ux - 65536, ty = uy - 65536;  // (in the coordinates whose integers are the pixel centres)
    const int xi = (int)(tx >> 17), yi = (int)(ty >> 17);
    const float fx = (float)((int)tx & 131071) * (1.0f / 131072.0f), fy = (float)((int)ty & 131071) * (1.0f / 131072.0f);
    const int xa = fold(xi, S) * C, xb = fold(xi + 1, S) * C;
    const uint8_t* r0 = img + (long)fold(yi, S) * S * C;
    const uint8_t* r1 = img + (long)fold(yi + 1, S) * S * C;
    float p00[C], p01[C], p10[C], p11[C], v[C];
    load_px<C>(r0 + xa, a.al4, p00);
    load_px<C>(r0 + xb, a.al4, p01);
    load_px<C>(r1 + xa, a.al4, p10);
    load_px<C>(r1 + xb, a.al4, p11);
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const float top = p00[c] + fx * (p01[c] - p00[c]), bot = p10[c] + fx * (p11[c] - p10[c]);
      v[c] = top + fy * (bot - top);
    }
    ux += stepx;
    uy += stepy;
    // jitter_kernel's colour stages and normalisation, restated here: that kernel's text and instructions stay as they are
#pragma unroll
    for (int c = 0; c < C; ++c) v[c] = v[c] / 255.0f;
    if (fb != 1.0f) {
#pragma unroll
      for (int c = 0; c < C; ++c) v[c] = clamp01(v[c] * fb);
    }
    if (fk != 1.0f) {
#pragma unroll
      for (int c = 0; c < C; ++c) v[c] = clamp01(bm[c] + fk * (v[c] - bm[c]));
    }
    if constexpr (C >= 3) {
      if (sat) {
        const float g = 0.299f * v[0] + 0.587f * v[1] + 0.114f * v[2];
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = clamp01(g + fs * (v[c] - g));
      }
    }
    if (fg != 1.0f) {
#pragma unroll
      for (int c = 0; c < C; ++c) v[c] = clamp01(powf(v[c], fg));
    }
#pragma unroll
    for (int c = 0; c < C; ++c) res[c][e] = (v[c] - a.mean[c]) / a.stdv[c];
  }

  const long rem = (long)yo * S + xo;
  float* dst = a.out + (long)n * C * SS + rem;
  if constexpr (V == 4) {
#pragma unroll
    for (int c = 0; c < C; ++c) *reinterpret_cast<f32x4*>(dst + c * SS) = f32x4{res[c][0], res[c][1], res[c][2], res[c][3]};
    if (msk) {
      typedef long long s64x2 __attribute__((ext_vector_type(2)));
      s64x2* mp = reinterpret_cast<s64x2*>(a.out_mask + (long)n * SS + rem);
      mp[0] = s64x2{lab[0], lab[1]};
      mp[1] = s64x2{lab[2], lab[3]};
    }
  } else {
#pragma unroll
    for (int c = 0; c < C; ++c) dst[c * SS] = res[c][0];
    if (msk) a.out_mask[(long)n * SS + rem] = lab[0];
  }
}

template <int C>
int launch_rotate(const RotArgs& a, bool vec, int blocks, hipStream_t stream) {
  if (vec)
    rotate_kernel<C, 4><<<blocks, 256, 0, stream>>>(a);
  else
    rotate_kernel<C, 1><<<blocks, 256, 0, stream>>>(a);
  return RS_LAUNCH_RESULT();
}

// floor(a / b) for b > 0
inline long long floor_div(long long a, long long b) { return a / b - (a % b < 0 ? 1 : 0); }

}  // namespace

extern "C" int rs_tile_band_sums(const uint8_t* images, int64_t* sums, int T, int S, int C, rs_stream_t stream) {
  if (!images || !sums || T <= 0 || S <= 0 || C <= 0 || C > 4) return RS_EINVAL;
  const long L = (long)S * S * C, total = (long)T * L;
  const hipError_t rc = hipMemsetAsync(sums, 0, (size_t)T * C * sizeof(int64_t), (hipStream_t)stream);
  if (rc != hipSuccess) return (int)rc;
  const long blocks = (total + (long)((uintptr_t)images & 15) + kSumSpan - 1) / kSumSpan;
  if (blocks > 0x7fffffffL) return RS_EINVAL;
  unsigned long long* out = reinterpret_cast<unsigned long long*>(sums);
  switch (C) {
    case 1: band_sums_kernel<1><<<(int)blocks, 256, 0, (hipStream_t)stream>>>(images, out, L, total); break;
    case 2: band_sums_kernel<2><<<(int)blocks, 256, 0, (hipStream_t)stream>>>(images, out, L, total); break;
    case 3: band_sums_kernel<3><<<(int)blocks, 256, 0, (hipStream_t)stream>>>(images, out, L, total); break;
    default: band_sums_kernel<4><<<(int)blocks, 256, 0, (hipStream_t)stream>>>(images, out, L, total); break;
  }
  return RS_LAUNCH_RESULT();
}

extern "C" int rs_augment_tiles_jitter(const uint8_t* images, const uint8_t* masks, const int32_t* index, const int32_t* op,
                                       const int32_t* geom, const float* color, const int64_t* band_sums, const float* mean,
                                       const float* stdv, float* out_images, int64_t* out_masks, int N, int S, int C, int rgb,
                                       rs_stream_t stream) {
  if (!images || !index || !op || !geom || !color || !mean || !stdv || !out_images || N <= 0 || S <= 0 || S > 16384 || C <= 0 || C > 4)
    return RS_EINVAL;
  if (masks && !out_masks) return RS_EINVAL;
  if (rgb && C < 3) return RS_EINVAL;
  for (int n = 0; n < N; ++n) {
    const int w = geom[3 * n], x0 = geom[3 * n + 1], y0 = geom[3 * n + 2];
    if (w < 1 || w > S || x0 < 0 || y0 < 0 || x0 > S - w || y0 > S - w) return RS_EINVAL;
    if (color[4 * n + 1] != 1.0f && !band_sums) return RS_EINVAL;
  }
  // four pixels of a row per thread (16-byte stores) where the rows and the two outputs allow it
  const bool vec = S % 4 == 0 && !((uintptr_t)out_images & 15) && !((uintptr_t)out_masks & 15);
  JitArgs a;
  a.images = images;
  a.masks = masks;
  a.band_sums = reinterpret_cast<const long long*>(band_sums);
  for (int c = 0; c < 4; ++c) {
    a.mean[c] = c < C ? mean[c] : 0.0f;
    a.stdv[c] = c < C ? stdv[c] : 1.0f;
  }
  a.div2s = rs_make_fastdiv(2u * (unsigned int)S);
  a.S = S;
  a.rgb = rgb ? 1 : 0;
  a.al4 = ((uintptr_t)images & 3) == 0;
  a.bpi = rs_cdiv((long)S * (vec ? S / 4 : S), 256);
  const long SS = (long)S * S;
  for (int at = 0; at < N; at += kJitItems) {
    const int cnt = N - at < kJitItems ? N - at : kJitItems;
    a.index = index + at;
    a.op = op + at;
    a.out = out_images + (long)at * C * SS;
    a.out_mask = out_masks ? reinterpret_cast<long long*>(out_masks) + (long)at * SS : nullptr;
    for (int i = 0; i < cnt; ++i) {
      for (int k = 0; k < 3; ++k) a.geom[i][k] = geom[3 * (at + i) + k];
      for (int k = 0; k < 4; ++k) a.color[i][k] = color[4 * (at + i) + k];
    }
    for (int i = cnt; i < kJitItems; ++i) {
      a.geom[i][0] = S, a.geom[i][1] = a.geom[i][2] = 0;
      for (int k = 0; k < 4; ++k) a.color[i][k] = 1.0f;
    }
    const int blocks = cnt * a.bpi;
    int rc;
    switch (C) {
      case 1: rc = launch_jitter<1>(a, vec, blocks, (hipStream_t)stream); break;
      case 2: rc = launch_jitter<2>(a, vec, blocks, (hipStream_t)stream); break;
      case 3: rc = launch_jitter<3>(a, vec, blocks, (hipStream_t)stream); break;
      default: rc = launch_jitter<4>(a, vec, blocks, (hipStream_t)stream); break;
    }
    if (rc) return rc;
  }
  return 0;
}

extern "C" int rs_augment_tiles_rotate(const uint8_t* images, const uint8_t* masks, const int32_t* index, const int32_t* op,
                                       const int32_t* geom, const int32_t* rot, const float* color, const int64_t* band_sums,
                                       const float* mean, const float* stdv, float* out_images, int64_t* out_masks, int N, int S,
                                       int C, int rgb, rs_stream_t stream) {
  if (!images || !index || !op || !geom || !rot || !color || !mean || !stdv || !out_images || N <= 0 || S <= 0 || S > 16384 || C <= 0 ||
      C > 4)
    return RS_EINVAL;
  if (masks && !out_masks) return RS_EINVAL;
  if (rgb && C < 3) return RS_EINVAL;
  for (int n = 0; n < N; ++n) {
    const int w = geom[3 * n], x0 = geom[3 * n + 1], y0 = geom[3 * n + 2];
    if (w < 1 || w > S || x0 < 0 || y0 < 0 || x0 > S - w || y0 > S - w) return RS_EINVAL;
    if (color[4 * n + 1] != 1.0f && !band_sums) return RS_EINVAL;
    // a rotation, to the two roundings: anything else could stretch the window past the one fold of the mirror
    const long long c = rot[2 * n], s = rot[2 * n + 1];
    if (c < -65536 || c > 65536 || s < -65536 || s > 65536) return RS_EINVAL;
    const long long off = c * c + s * s - (1LL << 32);
    if (off < -(1LL << 17) || off > (1LL << 17)) return RS_EINVAL;
  }
  // four pixels of a row per thread (16-byte stores) where the rows and the two outputs allow it
  const bool vec = S % 4 == 0 && !((uintptr_t)out_images & 15) && !((uintptr_t)out_masks & 15);
  RotArgs a;
  a.images = images;
  a.masks = masks;
  a.band_sums = reinterpret_cast<const long long*>(band_sums);
  for (int c = 0; c < 4; ++c) {
    a.mean[c] = c < C ? mean[c] : 0.0f;
    a.stdv[c] = c < C ? stdv[c] : 1.0f;
  }
  a.S = S;
  a.rgb = rgb ? 1 : 0;
  a.al4 = ((uintptr_t)images & 3) == 0;
  a.bpi = rs_cdiv((long)S * (vec ? S / 4 : S), 256);
  const long SS = (long)S * S;
  for (int at = 0; at < N; at += kJitItems) {
    const int cnt = N - at < kJitItems ? N - at : kJitItems;
    a.index = index + at;
    a.op = op + at;
    a.out = out_images + (long)at * C * SS;
    a.out_mask = out_masks ? reinterpret_cast<long long*>(out_masks) + (long)at * SS : nullptr;
    for (int i = 0; i < cnt; ++i) {
      const long long w = geom[3 * (at + i)];
      for (int k = 0; k < 3; ++k) a.geom[i][k] = geom[3 * (at + i) + k];
      for (int k = 0; k < 2; ++k) a.ab[i][k] = (int)floor_div(2 * rot[2 * (at + i) + k] * w + S, 2LL * S);
      for (int k = 0; k < 4; ++k) a.color[i][k] = color[4 * (at + i) + k];
    }
    for (int i = cnt; i < kJitItems; ++i) {
      a.geom[i][0] = S, a.geom[i][1] = a.geom[i][2] = 0;
      a.ab[i][0] = 65536, a.ab[i][1] = 0;
      for (int k = 0; k < 4; ++k) a.color[i][k] = 1.0f;
    }
    const int blocks = cnt * a.bpi;
    int rc;
    switch (C) {
      case 1: rc = launch_rotate<1>(a, vec, blocks, (hipStream_t)stream); break;
      case 2: rc = launch_rotate<2>(a, vec, blocks, (hipStream_t)stream); break;
      case 3: rc = launch_rotate<3>(a, vec, blocks, (hipStream_t)stream); break;
      default: rc = launch_rotate<4>(a, vec, blocks, (hipStream_t)stream); break;
    }
    if (rc) return rc;
  }
  return 0;
}
