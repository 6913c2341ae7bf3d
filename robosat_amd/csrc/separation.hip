// The separation weight plane (rs_separation_weight_plane in include/robosat_hip.h): the second term of the U-Net paper's weight
// map, w0 * exp(-(d1 + d2)^2 / (2 sigma^2)) with d1, d2 the distances to the two nearest OBJECTS, added onto a base plane.  Integers
// up to the table lookup, so the plane is defined bit for bit.  Six launches on the caller's stream and one
// memset, no atomics of its own, nothing read back:
//   sep_class_kernel   int64 labels -> one byte per pixel (0 background, 1 object, 2 ignored) and the object mask for the labelling
//   rs_features_label  features.hip, called as it is: the 4-connected components of the object pixels, label = root pixel + 1
//   sep_row_kernel     per pixel the two nearest DISTINCT labels of its row within |dx| < D, each packed with its |dx|
//   sep_col_kernel     per background pixel the best two squared distances by distinct label over the rows |dy| < D, then
//                      s2 = a + b + isqrt(4ab), the table lookup, the base, and the one write of the plane
#include "common.h"

namespace {

constexpr int kSepMaxD = 32;   // SEPARATION_MAX_REACH
constexpr int kSepRows = 64;   // rows of a column-pass strip
constexpr int kSepErrBytes = 16;

// A candidate is (label << 5) | |dx| in one word: labels are <= H * W <= 2^24 (sep_shape_ok) and |dx| < D <= 32.  0 = none.
__device__ __forceinline__ int sep_pack(int label, int dx) { return (label << 5) | dx; }

bool sep_shape_ok(int N, int H, int W) {  // (the sizes rs_features_label takes)
  return N > 0 && N <= 65535 && H > 0 && W > 0 && H <= 4096 && W <= 4096 && (long)N * H * W < (1l << 29);
}

__global__ __launch_bounds__(256) void sep_class_kernel(const long long* __restrict__ tgt, uint8_t* __restrict__ cls,
                                                        uint8_t* __restrict__ mask, long P, long long C, long long ignore) {
  const long p = (long)blockIdx.x * 256 + threadIdx.x;
  if (p >= P) return;
  const long long t = tgt[p];
  const int c = t == ignore ? 2 : (t >= 1 && t < C) ? 1 : 0;
  cls[p] = (uint8_t)c;
  mask[p] = (uint8_t)(c == 1);
}

// One wave per 64 columns of a row, four rows' chunks per block (the grid covers every chunk: no loop, so the one barrier is reached
// by every wave).  The wave stages the labels of the columns x0 - 32 .. x0 + 95 in LDS (D <= 32: half a chunk either side; a column
// outside the row holds 0) and keeps their "is an object" bits in two ballots.  A lane then visits only the object pixels of its
// window, nearest first, left before right at equal |dx|, until it has met two different labels.
__global__ __launch_bounds__(256) void sep_row_kernel(const int* __restrict__ L, int* __restrict__ candA, int* __restrict__ candB,
                                                      long items, int chunks, int W, int D) {
  __shared__ int seg[4][128];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long item = (long)blockIdx.x * 4 + wave;
  const bool live = item < items;  // (wave-uniform)
  const long row = live ? item / chunks : 0;
  const int x0 = live ? (int)(item - row * chunks) * 64 : 0;
  const int* Lr = L + row * W;
  const int xl = x0 - 32 + lane, xr = x0 + 32 + lane;
  const int l0 = live && xl >= 0 && xl < W ? Lr[xl] : 0;
  const int l1 = live && xr < W ? Lr[xr] : 0;
  const unsigned long long lo = __ballot(l0 != 0), hi = __ballot(l1 != 0);
  seg[wave][lane] = l0;
  seg[wave][64 + lane] = l1;
  rs_lds_writes_done();
  __syncthreads();
  const int x = x0 + lane;
  if (!live || x >= W) return;
  int a = 0, b = 0;
  // the window's bits: bit D - 1 is the pixel itself, bit D - 1 +- dx its neighbours (position of bit 0 in the segment: lane + 33 - D >= 1)
  const int pos = lane + 33 - D;
  unsigned long long w = pos < 64 ? (lo >> pos) | (hi << (64 - pos)) : hi >> (pos - 64);
  w &= (1ull << (2 * D - 1)) - 1ull;
  if (w) {
    unsigned long long left = __brevll(w << (64 - D));  // bit dx = the pixel dx to the left (bit 0: the pixel itself)
    unsigned long long right = (w >> (D - 1)) & ~1ull;  // bit dx = the pixel dx to the right
    const int* s = seg[wave] + 32 + lane;
    int la = 0;
    while (left | right) {
      const int dl = left ? __ffsll((long long)left) - 1 : 64;
      const int dr = right ? __ffsll((long long)right) - 1 : 64;
      int dx, l;
      if (dl <= dr) {
        dx = dl;
        l = s[-dl];
        left &= left - 1ull;
      } else {
        dx = dr;
        l = s[dr];
        right &= right - 1ull;
      }
      if (!la) {
        la = l;
        a = sep_pack(l, dx);
      } else if (l != la) {
        b = sep_pack(l, dx);
        break;
      }
    }
  }
  candA[row * W + x] = a;
  candB[row * W + x] = b;
}

// floor(sqrt(n)) for 0 <= n < 2^24 (exact in float): sqrtf, then the integer fix-up in both directions
__device__ __forceinline__ int sep_isqrt(int n) {
  int r = (int)sqrtf((float)n);
  while (r * r > n) --r;
  while ((r + 1) * (r + 1) <= n) ++r;
  return r;
}

struct SepBest {  // the best two squared distances so far, by distinct label
  int la, va, lb, vb;
  __device__ __forceinline__ void merge(int cand, int dy2) {
    if (!cand) return;
    const int l = cand >> 5, dx = cand & 31;
    const int v = dy2 + dx * dx;
    if (l == la) {
      va = v < va ? v : va;
    } else if (v < va) {  // (also where l == lb: the old first becomes the second)
      lb = la;
      vb = va;
      la = l;
      va = v;
    } else if (l == lb) {
      vb = v < vb ? v : vb;
    } else if (v < vb) {
      lb = l;
      vb = v;
    }
  }
};

// A block takes 64 columns x kSepRows rows of one image.  It stages the candidates of the rows y0 - (D - 1) .. y0 + kSepRows - 1 + (D - 1)
// in LDS as two planes of words [rows][64] (a wave reads 64 consecutive words of a row: no bank conflict; at most 2 * 126 * 256 bytes
// = 63 KB at D = 32, so two blocks fit a CU).  A row outside the image and a column beyond W hold "none".  Every lane owns a column and
// walks |dy| outward until dy^2 >= the second best.  A strip without a single candidate writes the base and walks nothing.
template <bool BASE>
__global__ __launch_bounds__(256) void sep_col_kernel(const int* __restrict__ candA, const int* __restrict__ candB,
                                                      const uint8_t* __restrict__ cls, const float* __restrict__ table,
                                                      const float* __restrict__ base, float* __restrict__ plane, int H, int W, int D) {
  extern __shared__ __attribute__((aligned(16))) int sep_staged[];  // [2][kSepRows + 2 (D - 1)][64]
  const int n = blockIdx.z, y0 = blockIdx.y * kSepRows, x0 = blockIdx.x * 64;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int rows = kSepRows + 2 * (D - 1);
  int* sa = sep_staged;
  int* sb = sep_staged + rows * 64;
  const int x = x0 + lane;
  int any = 0;
  for (int r = wave; r < rows; r += 4) {
    const int yy = y0 - (D - 1) + r;
    int a = 0, b = 0;
    if (x < W && yy >= 0 && yy < H) {
      const long q = ((long)n * H + yy) * W + x;
      a = candA[q];
      b = a ? candB[q] : 0;  // (no first candidate, no second)
    }
    sa[r * 64 + lane] = a;
    sb[r * 64 + lane] = b;
    any |= a;
  }
  rs_lds_writes_done();
  any = __syncthreads_or(any);
  if (x >= W) return;
  const int cap = D * D;
  for (int ry = wave; ry < kSepRows && y0 + ry < H; ry += 4) {
    const long p = ((long)n * H + y0 + ry) * W + x;
    const int c = cls[p];
    float out;
    if constexpr (BASE)
      out = base[p];
    else
      out = c == 2 ? 0.f : 1.f;
    if (any && c == 0) {
      const int at = (ry + D - 1) * 64 + lane;
      SepBest best = {0, cap, 0, cap};
      best.merge(sa[at], 0);
      best.merge(sb[at], 0);
      for (int dy = 1; dy * dy < best.vb; ++dy) {  // (vb <= D * D: dy stays below D, inside the staged rows)
        const int dy2 = dy * dy;
        best.merge(sa[at - dy * 64], dy2);
        best.merge(sb[at - dy * 64], dy2);
        best.merge(sa[at + dy * 64], dy2);
        best.merge(sb[at + dy * 64], dy2);
      }
      if (best.vb < cap) {  // two objects in reach: 4ab < 4 * 2^20
        const int s2 = best.va + best.vb + sep_isqrt(4 * best.va * best.vb);
        if (s2 < cap) out += table[s2];
      }
    }
    plane[p] = out;
  }
}

}  // namespace

extern "C" long rs_separation_weight_plane_workspace_bytes(int N, int H, int W) {
  if (!sep_shape_ok(N, H, W)) return RS_EINVAL;
  return kSepErrBytes + 14 * (long)N * H * W;  // err, then labels and the two candidate planes (int32), then the class and mask bytes
}

extern "C" int rs_separation_weight_plane(const long long* targets, const float* table, const float* base, float* plane, int N, int C,
                                          int H, int W, int D, int ignore, void* workspace, rs_stream_t stream) {
  if (!targets || !table || !plane || !workspace || ((uintptr_t)workspace & 15) || !sep_shape_ok(N, H, W) || C < 1 || C > 256 || D < 1 ||
      D > kSepMaxD || !(ignore == -1 || (ignore >= 1 && ignore <= 255)))
    return RS_EINVAL;
  const long P = (long)N * H * W;
  hipStream_t s = (hipStream_t)stream;
  int32_t* err = static_cast<int32_t*>(workspace);
  int32_t* labels = err + kSepErrBytes / 4;
  int32_t* candA = labels + P;
  int32_t* candB = candA + P;
  uint8_t* cls = reinterpret_cast<uint8_t*>(candB + P);
  uint8_t* mask = cls + P;
  const hipError_t e = hipMemsetAsync(err, 0, kSepErrBytes, s);
  if (e != hipSuccess) return (int)e;
  sep_class_kernel<<<rs_cdiv(P, 256), 256, 0, s>>>(targets, cls, mask, P, (long long)C, (long long)ignore);
  int rc = RS_LAUNCH_RESULT();
  if (rc) return rc;
  rc = rs_features_label(mask, labels, err, N, H, W, stream);
  if (rc) return rc;
  const int chunks = (W + 63) / 64;
  const long items = (long)N * H * chunks;
  sep_row_kernel<<<rs_cdiv(items, 4), 256, 0, s>>>(labels, candA, candB, items, chunks, W, D);
  rc = RS_LAUNCH_RESULT();
  if (rc) return rc;
  const dim3 grid(chunks, (H + kSepRows - 1) / kSepRows, N);
  const size_t lds = (size_t)2 * (kSepRows + 2 * (D - 1)) * 64 * sizeof(int);
  if (base)
    sep_col_kernel<true><<<grid, 256, lds, s>>>(candA, candB, cls, table, base, plane, H, W, D);
  else
    sep_col_kernel<false><<<grid, 256, lds, s>>>(candA, candB, cls, table, nullptr, plane, H, W, D);
  return RS_LAUNCH_RESULT();
}
