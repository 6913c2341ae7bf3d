// Dihedral test-time augmentation of `rs predict` / `rs serve` (an extension: the reference has none).  Both kernels are
// HBM-bound gathers between a tile and its V views; the network runs on the N*V views in between.
//
//   rs_tta_fan_out  tile n -> views n*V + v = g_v(tile), normalised NHWC4 (fp32 or bf16) for the stem
//   rs_tta_merge    probs of the N*V views -> per (pixel, class): the V values probs_v[c][g_v(p)], sorted ascending, summed in
//                   fp32 from the smallest, times 1/V; then the probabilities, the quantised bytes or the argmax byte
//
// op = f + 2*k, the encoding of rs_augment_tiles: FLIP_LEFT_RIGHT when f, then k counter-clockwise 90-degree rotations
// (np.rot90).  A dihedral op maps an aligned 32 x 32 block of the tile onto an aligned 32 x 32 block of the view (H, W are
// multiples of 32), so each block of both kernels moves whole blocks: coalesced reads, an LDS tile (row stride 33: the
// transposed reads of odd-k views are conflict-free), coalesced writes.
#include "common.h"

namespace {

constexpr int kTile = 32;
constexpr int kLd = kTile + 1;
constexpr int kMaxViews = 8;

struct TtaOps {
  int op[kMaxViews];
};

// tile pixel (y, x) of an H x W tile -> its position in the view of `op`
__device__ __forceinline__ void tta_fwd(int op, int H, int W, int& y, int& x) {
  if (op & 1) x = W - 1 - x;
  int h = H, w = W;
  for (int r = (op >> 1) & 3; r > 0; --r) {  // rot90: in[h][w] -> out[w][h], out[w-1-x][y] = in[y][x]
    const int ny = w - 1 - x;
    x = y;
    y = ny;
    const int t = h;
    h = w;
    w = t;
  }
}

// view pixel (y, x) -> the tile pixel it shows (the inverse of tta_fwd)
__device__ __forceinline__ void tta_inv(int op, int H, int W, int& y, int& x) {
  const int k = (op >> 1) & 3;
  int h = (k & 1) ? W : H;  // the view's shape
  for (int r = k; r > 0; --r) {  // undo the rotations, last first: out[i][j] = in[j][h_out-1-i]
    const int nx = h - 1 - y;
    y = x;
    x = nx;
    h = (h == H) ? W : H;
  }
  if (op & 1) x = W - 1 - x;
}

// ---- fan-out ----------------------------------------------------------------------------------------------------------
// One block per 32 x 32 block of one tile: the block's pixels are normalised once into LDS (four planes), then written to
// every view.  uint8 HWC: ((v/255 - mean)/std) in fp32 with IEEE divisions, the expression of rs_u8_to_nhwc4_norm; fp32 NCHW:
// the values as they are (rs_nchw_to_nhwc4).  Channels >= C are zero.  bf16 out: round to nearest even (= torch's .to()).
template <bool U8, typename TO>
__global__ __launch_bounds__(256) void tta_fan_out_kernel(const void* __restrict__ src, TO* __restrict__ out, f32x4 mean, f32x4 stdv,
                                                          const TtaOps ops, int V, int H, int W, int C) {
  __shared__ float s[4][kTile][kLd];
  const int n = blockIdx.y;
  const int bx = (int)(blockIdx.x % (unsigned)(W / kTile)), by = (int)(blockIdx.x / (unsigned)(W / kTile));
  const int y0 = by * kTile, x0 = bx * kTile;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int r = ty + 8 * i;
    const long pix = ((long)n * H + y0 + r) * W + x0 + tx;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if constexpr (U8) {
      const uint8_t* px = reinterpret_cast<const uint8_t*>(src) + pix * C;
#pragma unroll
      for (int c = 0; c < 4; ++c)
        if (c < C) v[c] = ((float)px[c] / 255.0f - mean[c]) / stdv[c];
    } else {
      const long HW = (long)H * W;
      const float* px = reinterpret_cast<const float*>(src) + (long)n * C * HW + (long)(y0 + r) * W + x0 + tx;
#pragma unroll
      for (int c = 0; c < 4; ++c)
        if (c < C) v[c] = px[c * HW];
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) s[c][r][tx] = v[c];
  }
  __syncthreads();
  for (int vi = 0; vi < V; ++vi) {
    const int op = ops.op[vi];
    int qy0 = y0, qx0 = x0;  // the view block this tile block lands in: the one holding the image of its first pixel
    tta_fwd(op, H, W, qy0, qx0);
    qy0 &= ~(kTile - 1);
    qx0 &= ~(kTile - 1);
    TO* o = out + (long)(n * V + vi) * H * W * 4;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int qy = qy0 + ty + 8 * i, qx = qx0 + tx;
      int py = qy, px = qx;
      tta_inv(op, H, W, py, px);
      py -= y0;
      px -= x0;
      const f32x4 v = {s[0][py][px], s[1][py][px], s[2][py][px], s[3][py][px]};
      rs_st4(o + ((long)qy * W + qx) * 4, v);
    }
  }
}

// ---- merge ------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void cswap(float& a, float& b) {
  const float lo = fminf(a, b), hi = fmaxf(a, b);
  a = lo;
  b = hi;
}

// Batcher's odd-even merge sort of 8 values, ascending (19 comparators).  Unused slots hold +inf and stay at the end.
__device__ __forceinline__ void sort8(float (&v)[kMaxViews]) {
  cswap(v[0], v[1]); cswap(v[2], v[3]); cswap(v[4], v[5]); cswap(v[6], v[7]);
  cswap(v[0], v[2]); cswap(v[1], v[3]); cswap(v[4], v[6]); cswap(v[5], v[7]);
  cswap(v[1], v[2]); cswap(v[5], v[6]);
  cswap(v[0], v[4]); cswap(v[1], v[5]); cswap(v[2], v[6]); cswap(v[3], v[7]);
  cswap(v[2], v[4]); cswap(v[3], v[5]);
  cswap(v[1], v[2]); cswap(v[3], v[4]); cswap(v[5], v[6]);
}

struct MergeArgs {
  const float* probs;     // [N*V][C][H][W]
  const double* anchors;  // [256] (quantize)
  float* out;             // probs: [N][C][H][W]
  uint8_t* qout;          // quantize: [N][H-2ov][W-2ov](][C-1]); argmax: [N][H][W]
  TtaOps ops;
  int V, mode, ov, N, C, H, W;
  float inv_v;
};

// One block per 32 x 32 block of one output tile, all classes in turn: for class c the V view blocks that hold the block's
// pixels come into LDS with coalesced row reads, each thread then gathers its 4 pixels' V values (transposed for odd k),
// sorts, sums and scales them.  The sorted sum makes the result independent of the order of the views: exactly
// equivariant under the mode's group (include/robosat_hip.h).
__global__ __launch_bounds__(256) void tta_merge_kernel(const MergeArgs a) {
  __shared__ float s[kMaxViews][kTile][kLd];
  __shared__ double anc[256];
  const int n = blockIdx.y, H = a.H, W = a.W, V = a.V, C = a.C, ov = a.ov;
  const int bx = (int)(blockIdx.x % (unsigned)(W / kTile)), by = (int)(blockIdx.x / (unsigned)(W / kTile));
  const int y0 = by * kTile, x0 = bx * kTile;
  if (a.mode == RS_TTA_QUANTIZE && (y0 + kTile <= ov || y0 >= H - ov || x0 + kTile <= ov || x0 >= W - ov))
    return;  // wholly inside the cropped border (uniform over the block, before any barrier)
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  if (a.mode == RS_TTA_QUANTIZE) anc[threadIdx.x] = a.anchors[threadIdx.x];
  const long HW = (long)H * W;
  float best[4] = {0.f, 0.f, 0.f, 0.f};
  int besti[4] = {0, 0, 0, 0};
  for (int c = 0; c < C; ++c) {
    __syncthreads();  // (the previous class's reads of `s` are done)
    for (int vi = 0; vi < V; ++vi) {
      int qy0 = y0, qx0 = x0;
      tta_fwd(a.ops.op[vi], H, W, qy0, qx0);
      qy0 &= ~(kTile - 1);
      qx0 &= ~(kTile - 1);
      // 16 bytes per lane: row t / 8, columns 4 * (t % 8) .. + 3 (eight lanes cover a row's 128 bytes)
      const int lr = threadIdx.x >> 3, lc = (threadIdx.x & 7) * 4;
      const f32x4 q = *reinterpret_cast<const f32x4*>(a.probs + ((long)(n * V + vi) * C + c) * HW + (long)(qy0 + lr) * W + qx0 + lc);
#pragma unroll
      for (int e = 0; e < 4; ++e) s[vi][lr][lc + e] = q[e];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int y = y0 + ty + 8 * i, x = x0 + tx;
      float v[kMaxViews];
#pragma unroll
      for (int vi = 0; vi < kMaxViews; ++vi) {
        v[vi] = __builtin_huge_valf();
        if (vi < V) {
          int qy = y, qx = x;
          tta_fwd(a.ops.op[vi], H, W, qy, qx);
          v[vi] = s[vi][qy & (kTile - 1)][qx & (kTile - 1)];
        }
      }
      sort8(v);
      float acc = v[0];
#pragma unroll
      for (int vi = 1; vi < kMaxViews; ++vi)
        if (vi < V) acc = acc + v[vi];
      const float m = acc * a.inv_v;
      if (a.mode == RS_TTA_PROBS) {
        a.out[((long)n * C + c) * HW + (long)y * W + x] = m;
      } else if (a.mode == RS_TTA_ARGMAX) {
        if (c == 0 || m > best[i]) {  // first maximum
          best[i] = m;
          besti[i] = c;
        }
      } else if (c > 0 && y >= ov && y < H - ov && x >= ov && x < W - ov) {
        // np.digitize(p, np.linspace(0, 1, 256)) in float64, as elementwise.hip:final_epilogue: 1-based, 256 wraps to 0
        const double pf = (double)m;
        int q = (int)(pf * 255.0);
        q = q < 0 ? 0 : (q > 255 ? 255 : q);
        while (q < 255 && anc[q + 1] <= pf) ++q;
        while (q >= 0 && anc[q] > pf) --q;
        const int Sh = H - 2 * ov, Sw = W - 2 * ov;
        a.qout[(((long)n * Sh + (y - ov)) * Sw + (x - ov)) * (C - 1) + (c - 1)] = (uint8_t)((q + 1) & 0xff);
      }
    }
  }
  if (a.mode == RS_TTA_ARGMAX) {
#pragma unroll
    for (int i = 0; i < 4; ++i) a.qout[(long)n * HW + (long)(y0 + ty + 8 * i) * W + x0 + tx] = (uint8_t)besti[i];
  }
}

// ops[v] in 0..7, V a power of two <= 8, whole 32 x 32 blocks, square tiles for the odd-k ops (their views are W x H)
bool tta_shape_ok(const int* ops, int V, int N, int H, int W, TtaOps& t) {
  if (!ops || (V != 1 && V != 2 && V != 4 && V != 8) || N <= 0 || H <= 0 || W <= 0 || (H % kTile) || (W % kTile)) return false;
  if (N > 65535) return false;  // (gridDim.y)
  for (int v = 0; v < kMaxViews; ++v) t.op[v] = 0;
  for (int v = 0; v < V; ++v) {
    if (ops[v] < 0 || ops[v] > 7) return false;
    if (((ops[v] >> 1) & 1) && H != W) return false;
    t.op[v] = ops[v];
  }
  return true;
}

}  // namespace

extern "C" int rs_tta_fan_out(const void* x, int x_kind, const float* mean, const float* stdv, void* out, int out_dtype,
                              const int* ops, int V, int N, int H, int W, int C, rs_stream_t stream) {
  TtaOps t;
  if (!x || !out || C <= 0 || C > 4 || !tta_shape_ok(ops, V, N, H, W, t)) return RS_EINVAL;
  if (x_kind != RS_TTA_IN_U8 && x_kind != RS_TTA_IN_F32) return RS_EINVAL;
  if (out_dtype != RS_F32 && out_dtype != RS_BF16) return RS_EINVAL;
  f32x4 m = {0.f, 0.f, 0.f, 0.f}, sd = {1.f, 1.f, 1.f, 1.f};
  if (x_kind == RS_TTA_IN_U8) {
    if (!mean || !stdv) return RS_EINVAL;
    for (int c = 0; c < C; ++c) {
      m[c] = mean[c];  // host arrays: C floats
      sd[c] = stdv[c];
    }
  }
  const dim3 grid((unsigned)((H / kTile) * (W / kTile)), (unsigned)N);
  hipStream_t s = (hipStream_t)stream;
  if (x_kind == RS_TTA_IN_U8 && out_dtype == RS_F32)
    tta_fan_out_kernel<true, float><<<grid, 256, 0, s>>>(x, reinterpret_cast<float*>(out), m, sd, t, V, H, W, C);
  else if (x_kind == RS_TTA_IN_U8)
    tta_fan_out_kernel<true, bf16_t><<<grid, 256, 0, s>>>(x, reinterpret_cast<bf16_t*>(out), m, sd, t, V, H, W, C);
  else if (out_dtype == RS_F32)
    tta_fan_out_kernel<false, float><<<grid, 256, 0, s>>>(x, reinterpret_cast<float*>(out), m, sd, t, V, H, W, C);
  else
    tta_fan_out_kernel<false, bf16_t><<<grid, 256, 0, s>>>(x, reinterpret_cast<bf16_t*>(out), m, sd, t, V, H, W, C);
  return RS_LAUNCH_RESULT();
}

extern "C" int rs_tta_merge(const float* probs, const int* ops, int V, int mode, const double* anchors, int overlap, void* out,
                            int N, int C, int H, int W, rs_stream_t stream) {
  MergeArgs a;
  if (!probs || !out || ((uintptr_t)probs & 15) || C < 1 || C > 8 || !tta_shape_ok(ops, V, N, H, W, a.ops)) return RS_EINVAL;
  if (mode == RS_TTA_QUANTIZE) {
    if (!anchors || C < 2 || overlap < 0 || 2 * overlap >= H || 2 * overlap >= W) return RS_EINVAL;
  } else if (mode != RS_TTA_PROBS && mode != RS_TTA_ARGMAX) {
    return RS_EINVAL;
  }
  a.probs = probs;
  a.anchors = anchors;
  a.out = reinterpret_cast<float*>(out);
  a.qout = reinterpret_cast<uint8_t*>(out);
  a.V = V;
  a.mode = mode;
  a.ov = mode == RS_TTA_QUANTIZE ? overlap : 0;
  a.N = N;
  a.C = C;
  a.H = H;
  a.W = W;
  a.inv_v = 1.0f / (float)V;
  const dim3 grid((unsigned)((H / kTile) * (W / kTile)), (unsigned)N);
  tta_merge_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(a);
  return RS_LAUNCH_RESULT();
}
