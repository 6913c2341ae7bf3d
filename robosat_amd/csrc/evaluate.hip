// `rs evaluate` (robosat_amd/tools/evaluate.py): the counting passes over two rasters, per group of pixels (definitions in
// include/robosat_hip.h).  Integer work, HBM-bound: every pixel of both rasters is read once.
//
//   rs_eval_confusion  two class-index rasters -> per group the C x C matrix counts[actual][predicted] and the number of pixels with a
//                      value that is no class
//   rs_eval_boundary   two capped distance transforms (rs_features_edt) -> per group the sizes of the two boundary bands and of their
//                      intersection
//   rs_eval_prob_hist  the probability bytes of one class and the label raster -> per group the 2 x 256 histogram of (label is the
//                      class, byte) and the numbers of pixels with a bad and with an ignored label
//   rs_eval_centerline two skeletons and the capped distance transforms of their complements -> per group the straight and diagonal
//                      links of either skeleton and those whose two ends lie within rho of the other (at the end of the file: its
//                      threads own runs of a ROW, since a link has a neighbour below, not runs of the call)
//   rs_eval_select     (`--ignored unknown`) two class-index rasters, a class and the ignore value -> the two rasters coded unset /
//                      set / unknown and their set pixels as 0/1 masks: no counting, a pass that writes four byte planes
//   rs_eval_boundary_coded  rs_eval_boundary over the pixels that a coded plane does not call unknown
//
// The kernels share one shape.  A block of 256 threads covers kEvalBlock = 4096 consecutive pixels of the whole call, a thread 16
// consecutive ones, held in registers: a 16-byte load per raster (four for the int32 rasters) where the thread's first address is
// 16-byte aligned and its run ends within `pixels`, single loads with a bound check otherwise (the call's last thread; a raster that
// is a view at an odd offset).  Runs are laid over the call, not over the groups, so where a group begins (byte 63 for the second
// tile of a 7 x 9 batch) has no say in the alignment.  The block then walks the groups its pixels lie in -- one for a tile of at least
// 4096 pixels away from its ends, two where the block straddles a border, more only for tiles smaller than a block -- and per group
// counts the pixels of that group only, merges on chip and sends one 64-bit atomic add per non-empty cell.  No workgroup waits for
// another and every loop is bounded (the group loop by the block's 4096 pixels).
#include "common.h"

namespace {

constexpr int kEvalRun = 16;                            // consecutive pixels of a thread
constexpr int kEvalThreads = 256;                       // four waves
constexpr int kEvalBlock = kEvalRun * kEvalThreads;     // pixels of a block
constexpr int kEvalBad = 64;                            // the bin of pixels with a value >= C, behind the 8 x 8 cells
constexpr int kEvalBins = kEvalBad + 1;

// The thread's part [jlo, jhi) of its run that lies in group g: pixel j counts iff g*group <= base + j < min((g+1)*group, pixels).
__device__ __forceinline__ void eval_range(long base, long g, long group, long pixels, int& jlo, int& jhi) {
  long lo = g * group - base, hi = (g + 1) * group - base;
  const long top = pixels - base;
  if (hi > top) hi = top;
  jlo = lo < 0 ? 0 : lo > kEvalRun ? kEvalRun : (int)lo;
  jhi = hi < 0 ? 0 : hi > kEvalRun ? kEvalRun : (int)hi;
}

__device__ __forceinline__ void eval_load_bytes(const uint8_t* __restrict__ p, long base, long pixels, unsigned int (&w)[4]) {
  if (base + kEvalRun <= pixels && (reinterpret_cast<uintptr_t>(p + base) & 15) == 0) {
    const u32x4 q = *reinterpret_cast<const u32x4*>(p + base);
#pragma unroll
    for (int e = 0; e < 4; ++e) w[e] = q[e];
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) w[e] = 0;
#pragma unroll
    for (int j = 0; j < kEvalRun; ++j)
      if (base + j < pixels) w[j >> 2] |= (unsigned int)p[base + j] << ((j & 3) * 8);
  }
}

// Bit j set where 1 <= d2[base + j] <= dd.
__device__ __forceinline__ unsigned int eval_load_band(const int* __restrict__ d2, long base, long pixels, unsigned int dd) {
  unsigned int bits = 0;
  if (base + kEvalRun <= pixels && (reinterpret_cast<uintptr_t>(d2 + base) & 15) == 0) {
    u32x4 q[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) q[e] = *(reinterpret_cast<const u32x4*>(d2 + base) + e);
#pragma unroll
    for (int j = 0; j < kEvalRun; ++j) bits |= (unsigned int)(q[j >> 2][j & 3] - 1u < dd) << j;  // (0 wraps to 2^32 - 1: not in the band)
  } else {
#pragma unroll
    for (int j = 0; j < kEvalRun; ++j)
      if (base + j < pixels) bits |= (unsigned int)((unsigned int)d2[base + j] - 1u < dd) << j;
  }
  return bits;
}

// 0x01 in every byte of x that equals k, 0 in the others (exact: 0x7f + 0x7f leaves no carry for the next byte).
__device__ __forceinline__ unsigned int eval_eq_bytes(unsigned int x, unsigned int k) {
  const unsigned int t = x ^ (k * 0x01010101u);
  return (~(t | ((t & 0x7f7f7f7fu) + 0x7f7f7f7fu)) & 0x80808080u) >> 7;
}

// Bit j set where coded[base + j] is not 2 (a pixel beyond `pixels` reads 0: known, and in no band).
__device__ __forceinline__ unsigned int eval_load_known(const uint8_t* __restrict__ coded, long base, long pixels) {
  unsigned int w[4], unknown = 0;
  eval_load_bytes(coded, base, pixels, w);
#pragma unroll
  for (int e = 0; e < 4; ++e)  // (the four 0x01 bytes side by side: the product of cl_row_bits below)
    unknown |= ((eval_eq_bytes(w[e], 2u) * 0x00204081u >> 21) & 15u) << (4 * e);
  return ~unknown & 0xffffu;
}

__device__ __forceinline__ void eval_store_bytes(uint8_t* __restrict__ p, long base, long pixels, const unsigned int (&w)[4]) {
  if (base + kEvalRun <= pixels && (reinterpret_cast<uintptr_t>(p + base) & 15) == 0) {
    u32x4 q;
#pragma unroll
    for (int e = 0; e < 4; ++e) q[e] = w[e];
    *reinterpret_cast<u32x4*>(p + base) = q;
  } else {
#pragma unroll
    for (int j = 0; j < kEvalRun; ++j)
      if (base + j < pixels) p[base + j] = (uint8_t)(w[j >> 2] >> ((j & 3) * 8));
  }
}

// ---- confusion matrix per group --------------------------------------------------------------------------------------
// A pixel's cell is actual * C + predicted (< 64), or kEvalBad where either byte is >= C.  Per group: a thread turns its pixels into
// runs of equal cells and adds one run at a time to its wave's private histogram in LDS (a tile that is all one cell costs one LDS
// atomic per thread, not 16; the four private copies keep the waves off each other's counters), the four copies are summed per bin,
// and the bins that are not empty go out: at most C*C + 1 global atomics per block and group.
__global__ __launch_bounds__(kEvalThreads) void eval_confusion_kernel(const uint8_t* __restrict__ predicted, const uint8_t* __restrict__ actual,
                                                                      unsigned long long* __restrict__ counts,
                                                                      unsigned long long* __restrict__ bad, long pixels, long group, int C) {
  __shared__ unsigned int hist[4][kEvalBins];
  const long block0 = (long)blockIdx.x * kEvalBlock;
  const long base = block0 + (long)threadIdx.x * kEvalRun;
  unsigned int cells[4] = {0, 0, 0, 0};  // 16 cells, a byte each
  if (base < pixels) {
    unsigned int pw[4], aw[4];
    eval_load_bytes(predicted, base, pixels, pw);
    eval_load_bytes(actual, base, pixels, aw);
#pragma unroll
    for (int j = 0; j < kEvalRun; ++j) {
      const unsigned int p = (pw[j >> 2] >> ((j & 3) * 8)) & 255u, a = (aw[j >> 2] >> ((j & 3) * 8)) & 255u;
      const unsigned int cell = (p >= (unsigned int)C || a >= (unsigned int)C) ? (unsigned int)kEvalBad : a * C + p;
      cells[j >> 2] |= cell << ((j & 3) * 8);
    }
  }
  const long block1 = block0 + kEvalBlock < pixels ? block0 + kEvalBlock : pixels;  // (block0 < pixels: the grid is cdiv(pixels, kEvalBlock))
  const long g0 = block0 / group, g1 = (block1 - 1) / group;
  unsigned int* h = hist[threadIdx.x >> 6];
  const int cc = C * C;
  for (long g = g0; g <= g1; ++g) {
    for (int i = threadIdx.x; i < 4 * kEvalBins; i += kEvalThreads) (&hist[0][0])[i] = 0;
    __syncthreads();
    int jlo, jhi;
    eval_range(base, g, group, pixels, jlo, jhi);
    unsigned int cur = 0, run = 0;
#pragma unroll
    for (int j = 0; j < kEvalRun; ++j) {
      if (j >= jlo && j < jhi) {
        const unsigned int cell = (cells[j >> 2] >> ((j & 3) * 8)) & 255u;
        if (run && cell != cur) {
          atomicAdd(&h[cur], run);
          run = 0;
        }
        cur = cell;
        ++run;
      }
    }
    if (run) atomicAdd(&h[cur], run);
    __syncthreads();
    if (threadIdx.x < kEvalBins) {
      const int t = threadIdx.x;
      const unsigned int tot = hist[0][t] + hist[1][t] + hist[2][t] + hist[3][t];
      if (tot) {
        if (t == kEvalBad)
          atomicAdd(&bad[g], (unsigned long long)tot);
        else if (t < cc)  // (a cell is below C*C by construction)
          atomicAdd(&counts[g * cc + t], (unsigned long long)tot);
      }
    }
    __syncthreads();  // (the next group zeroes the histograms)
  }
}

// ---- boundary bands per group ----------------------------------------------------------------------------------------
// Three counters per group, so no histogram: a thread keeps its 16 pixels as two 16-bit masks, counts the bits of its part of the
// group, the wave sums over its lanes, the block over its waves, and up to three global atomics go out per block and group.
// CODED (rs_eval_boundary_coded): a pixel whose byte of `coded` is 2 is unknown and in neither band, whatever the transforms hold
// there (rs_features_edt takes non-zero for set, so it writes a distance at an unknown pixel); one more byte plane is read.
template <bool CODED>
__global__ __launch_bounds__(kEvalThreads) void eval_boundary_kernel(const int* __restrict__ d2_a, const int* __restrict__ d2_b,
                                                                     unsigned long long* __restrict__ counts, long pixels, long group,
                                                                     unsigned int dd, const uint8_t* __restrict__ coded) {
  __shared__ unsigned int part[4][3];
  const long block0 = (long)blockIdx.x * kEvalBlock;
  const long base = block0 + (long)threadIdx.x * kEvalRun;
  unsigned int ma = 0, mb = 0;
  if (base < pixels) {
    ma = eval_load_band(d2_a, base, pixels, dd);
    mb = eval_load_band(d2_b, base, pixels, dd);
    if (CODED) {
      const unsigned int known = eval_load_known(coded, base, pixels);
      ma &= known;
      mb &= known;
    }
  }
  const long block1 = block0 + kEvalBlock < pixels ? block0 + kEvalBlock : pixels;
  const long g0 = block0 / group, g1 = (block1 - 1) / group;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (long g = g0; g <= g1; ++g) {
    int jlo, jhi;
    eval_range(base, g, group, pixels, jlo, jhi);
    const unsigned int in = jhi > jlo ? ((1u << jhi) - 1u) & ~((1u << jlo) - 1u) : 0u;  // (jhi <= 16: no shift by 32)
    unsigned int n[3] = {(unsigned int)__popc(ma & in), (unsigned int)__popc(mb & in), (unsigned int)__popc(ma & mb & in)};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) n[k] += __shfl_xor(n[k], o, 64);
      if (lane == 0) part[wave][k] = n[k];
    }
    __syncthreads();
    if (threadIdx.x < 3) {
      const int t = threadIdx.x;
      const unsigned int tot = part[0][t] + part[1][t] + part[2][t] + part[3][t];
      if (tot) atomicAdd(&counts[g * 3 + t], (unsigned long long)tot);
    }
    __syncthreads();  // (the next group overwrites the partial sums)
  }
}

// ---- the coded rasters of `--ignored unknown` (rs_eval_select) ---------------------------------------------------------------------
// No counts: a thread reads its 16 bytes of both rasters and writes 16 bytes of each of the four planes, a word of four pixels at a
// time.  With u = (actual == ignore), set_p = (predicted == cls) and not u, set_g = (actual == cls) (a label that is the class is not
// the ignore value: ignore >= C > cls): coded = set | u << 1, mask = set.  Every output byte has one writer.
__global__ __launch_bounds__(kEvalThreads) void eval_select_kernel(const uint8_t* __restrict__ predicted, const uint8_t* __restrict__ actual,
                                                                   uint8_t* __restrict__ coded_p, uint8_t* __restrict__ coded_g,
                                                                   uint8_t* __restrict__ mask_p, uint8_t* __restrict__ mask_g, long pixels,
                                                                   unsigned int cls, unsigned int ignore) {
  const long base = ((long)blockIdx.x * kEvalThreads + threadIdx.x) * kEvalRun;
  if (base >= pixels) return;
  unsigned int pw[4], aw[4], cp[4], cg[4], mp[4], mg[4];
  eval_load_bytes(predicted, base, pixels, pw);
  eval_load_bytes(actual, base, pixels, aw);
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const unsigned int u = eval_eq_bytes(aw[e], ignore);
    mp[e] = eval_eq_bytes(pw[e], cls) & ~u;
    mg[e] = eval_eq_bytes(aw[e], cls);
    cp[e] = mp[e] | u << 1;
    cg[e] = mg[e] | u << 1;
  }
  eval_store_bytes(coded_p, base, pixels, cp);
  eval_store_bytes(coded_g, base, pixels, cg);
  eval_store_bytes(mask_p, base, pixels, mp);
  eval_store_bytes(mask_g, base, pixels, mg);
}

bool eval_shape_ok(long pixels, long group) { return pixels > 0 && pixels < (1l << 31) && group > 0 && pixels % group == 0; }

}  // namespace

extern "C" int rs_eval_config(int* block_pixels) {
  if (!block_pixels) return RS_EINVAL;
  *block_pixels = kEvalBlock;
  return 0;
}

extern "C" int rs_eval_confusion(const uint8_t* predicted, const uint8_t* actual, int64_t* counts, int64_t* bad, long pixels, long group,
                                 int C, rs_stream_t stream) {
  if (!predicted || !actual || !counts || !bad || (((uintptr_t)counts | (uintptr_t)bad) & 7) || !eval_shape_ok(pixels, group) || C < 2 ||
      C > 8)
    return RS_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const long groups = pixels / group;
  // (one fill where `bad` follows `counts` directly, as ops.mask_confusion lays them out: a fill costs about what the kernel does)
  const bool joined = bad == counts + groups * C * C;
  hipError_t e = hipMemsetAsync(counts, 0, groups * (C * C + (joined ? 1 : 0)) * sizeof(int64_t), s);
  if (e == hipSuccess && !joined) e = hipMemsetAsync(bad, 0, groups * sizeof(int64_t), s);
  if (e != hipSuccess) return (int)e;
  eval_confusion_kernel<<<rs_cdiv(pixels, kEvalBlock), kEvalThreads, 0, s>>>(predicted, actual, reinterpret_cast<unsigned long long*>(counts),
                                                                             reinterpret_cast<unsigned long long*>(bad), pixels, group, C);
  return RS_LAUNCH_RESULT();
}

extern "C" int rs_eval_boundary(const int32_t* d2_a, const int32_t* d2_b, int64_t* counts, long pixels, long group, int D,
                                rs_stream_t stream) {
  if (!d2_a || !d2_b || !counts || ((uintptr_t)counts & 7) || !eval_shape_ok(pixels, group) || D < 1 || D > 127) return RS_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const hipError_t e = hipMemsetAsync(counts, 0, pixels / group * 3 * sizeof(int64_t), s);
  if (e != hipSuccess) return (int)e;
  eval_boundary_kernel<false><<<rs_cdiv(pixels, kEvalBlock), kEvalThreads, 0, s>>>(d2_a, d2_b, reinterpret_cast<unsigned long long*>(counts),
                                                                                   pixels, group, (unsigned int)(D * D), nullptr);
  return RS_LAUNCH_RESULT();
}

extern "C" int rs_eval_boundary_coded(const int32_t* d2_a, const int32_t* d2_b, const uint8_t* coded, int64_t* counts, long pixels,
                                      long group, int D, rs_stream_t stream) {
  if (!d2_a || !d2_b || !coded || !counts || ((uintptr_t)counts & 7) || !eval_shape_ok(pixels, group) || D < 1 || D > 127) return RS_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const hipError_t e = hipMemsetAsync(counts, 0, pixels / group * 3 * sizeof(int64_t), s);
  if (e != hipSuccess) return (int)e;
  eval_boundary_kernel<true><<<rs_cdiv(pixels, kEvalBlock), kEvalThreads, 0, s>>>(d2_a, d2_b, reinterpret_cast<unsigned long long*>(counts),
                                                                                  pixels, group, (unsigned int)(D * D), coded);
  return RS_LAUNCH_RESULT();
}

extern "C" int rs_eval_select(const uint8_t* predicted, const uint8_t* actual, uint8_t* coded_p, uint8_t* coded_g, uint8_t* mask_p,
                              uint8_t* mask_g, long pixels, int C, int cls, int ignore, rs_stream_t stream) {
  if (!predicted || !actual || !coded_p || !coded_g || !mask_p || !mask_g || pixels <= 0 || pixels >= (1l << 31) || C < 2 || C > 8 ||
      cls < 1 || cls >= C || ignore < C || ignore > 255)
    return RS_EINVAL;
  eval_select_kernel<<<rs_cdiv(pixels, kEvalBlock), kEvalThreads, 0, (hipStream_t)stream>>>(predicted, actual, coded_p, coded_g, mask_p, mask_g,
                                                                                            pixels, (unsigned int)cls, (unsigned int)ignore);
  return RS_LAUNCH_RESULT();
}

// ---- confusion matrix per group with an ignore label (rs_eval_confusion_ig) ----------------------------------------------------
// eval_confusion_kernel with one more bin behind `bad`: a pixel whose ACTUAL byte equals `ignore` (>= C) and whose predicted byte
// is a class lies in no cell and is counted in ignored[g].  A predicted byte >= C is bad whatever lies under it, and so is an
// actual byte >= C other than `ignore`.  The kernel above is left as it is.
namespace {

constexpr int kEvalIgnored = kEvalBad + 1;
constexpr int kEvalBinsIg = kEvalIgnored + 1;

__global__ __launch_bounds__(kEvalThreads) void eval_confusion_ig_kernel(const uint8_t* __restrict__ predicted, const uint8_t* __restrict__ actual,
                                                                         unsigned long long* __restrict__ counts,
                                                                         unsigned long long* __restrict__ bad,
                                                                         unsigned long long* __restrict__ ignored, long pixels, long group,
                                                                         int C, unsigned int ignore) {
  __shared__ unsigned int hist[4][kEvalBinsIg];
  const long block0 = (long)blockIdx.x * kEvalBlock;
  const long base = block0 + (long)threadIdx.x * kEvalRun;
  unsigned int cells[4] = {0, 0, 0, 0};  // 16 cells, a byte each
  if (base < pixels) {
    unsigned int pw[4], aw[4];
    eval_load_bytes(predicted, base, pixels, pw);
    eval_load_bytes(actual, base, pixels, aw);
#pragma unroll
    for (int j = 0; j < kEvalRun; ++j) {
      const unsigned int p = (pw[j >> 2] >> ((j & 3) * 8)) & 255u, a = (aw[j >> 2] >> ((j & 3) * 8)) & 255u;
      const unsigned int cell = p >= (unsigned int)C ? (unsigned int)kEvalBad
                                : a == ignore        ? (unsigned int)kEvalIgnored
                                : a >= (unsigned int)C ? (unsigned int)kEvalBad
                                                       : a * C + p;
      cells[j >> 2] |= cell << ((j & 3) * 8);
    }
  }
  const long block1 = block0 + kEvalBlock < pixels ? block0 + kEvalBlock : pixels;
  const long g0 = block0 / group, g1 = (block1 - 1) / group;
  unsigned int* h = hist[threadIdx.x >> 6];
  const int cc = C * C;
  for (long g = g0; g <= g1; ++g) {
    for (int i = threadIdx.x; i < 4 * kEvalBinsIg; i += kEvalThreads) (&hist[0][0])[i] = 0;
    __syncthreads();
    int jlo, jhi;
    eval_range(base, g, group, pixels, jlo, jhi);
    unsigned int cur = 0, run = 0;
#pragma unroll
    for (int j = 0; j < kEvalRun; ++j) {
      if (j >= jlo && j < jhi) {
        const unsigned int cell = (cells[j >> 2] >> ((j & 3) * 8)) & 255u;
        if (run && cell != cur) {
          atomicAdd(&h[cur], run);
          run = 0;
        }
        cur = cell;
        ++run;
      }
    }
    if (run) atomicAdd(&h[cur], run);
    __syncthreads();
    if (threadIdx.x < kEvalBinsIg) {
      const int t = threadIdx.x;
      const unsigned int tot = hist[0][t] + hist[1][t] + hist[2][t] + hist[3][t];
      if (tot) {
        if (t == kEvalIgnored)
          atomicAdd(&ignored[g], (unsigned long long)tot);
        else if (t == kEvalBad)
          atomicAdd(&bad[g], (unsigned long long)tot);
        else if (t < cc)
          atomicAdd(&counts[g * cc + t], (unsigned long long)tot);
      }
    }
    __syncthreads();  // (the next group zeroes the histograms)
  }
}

}  // namespace

extern "C" int rs_eval_confusion_ig(const uint8_t* predicted, const uint8_t* actual, int64_t* counts, int64_t* bad, int64_t* ignored,
                                    long pixels, long group, int C, rs_stream_t stream, int ignore) {
  if (!predicted || !actual || !counts || !bad || !ignored || (((uintptr_t)counts | (uintptr_t)bad | (uintptr_t)ignored) & 7) ||
      !eval_shape_ok(pixels, group) || C < 2 || C > 8 || ignore < C || ignore > 255)
    return RS_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const long groups = pixels / group;
  // (one fill where `bad` and `ignored` follow `counts` directly, as ops.mask_confusion lays them out)
  const bool joined = bad == counts + groups * C * C && ignored == bad + groups;
  hipError_t e = hipMemsetAsync(counts, 0, groups * (C * C + (joined ? 2 : 0)) * sizeof(int64_t), s);
  if (e == hipSuccess && !joined) e = hipMemsetAsync(bad, 0, groups * sizeof(int64_t), s);
  if (e == hipSuccess && !joined) e = hipMemsetAsync(ignored, 0, groups * sizeof(int64_t), s);
  if (e != hipSuccess) return (int)e;
  eval_confusion_ig_kernel<<<rs_cdiv(pixels, kEvalBlock), kEvalThreads, 0, s>>>(
      predicted, actual, reinterpret_cast<unsigned long long*>(counts), reinterpret_cast<unsigned long long*>(bad),
      reinterpret_cast<unsigned long long*>(ignored), pixels, group, C, (unsigned int)ignore);
  return RS_LAUNCH_RESULT();
}

// ---- probability histogram per group (rs_eval_prob_hist) ---------------------------------------------------------------------
// `rs evaluate --probs`: the joint histogram of (label is the class, probability byte), 2 x 256 bins per group, and two counters
// for the pixels that are in none of them.  A pixel's cell is pos * 256 + q, or kProbBad / kProbIgnored behind the 512 bins.  The
// shape is eval_confusion_kernel's (16 pixels per thread in registers, the block walks its groups), with three differences that
// the 514 cells ask for:
//   * the four wave-private histograms are zeroed ONCE; the thread that merges a bin puts it back to zero (only where it was
//     not), so a group costs two reads of the histograms and no fill, and two barriers;
//   * a wave whose pixels of the group all lie in one cell (saturated tiles: nearly every pixel is (negative, byte 1)) adds its
//     count over the lanes and sends ONE LDS add, where 64 lanes adding to one address would be served one after another;
//   * otherwise runs of equal cells within a thread are merged as in the confusion kernel, one LDS atomic per run: 16 per
//     thread at worst (uniformly random bytes), into 512 counters of the wave's own copy.
// Per block and group at most 514 global 64-bit atomics go out, for non-empty cells only.  Counters in LDS are 32 bits: a block
// holds 4096 pixels.  No workgroup waits for another; every loop is bounded.
namespace {

constexpr int kProbBins = 512;                 // [pos][q]
constexpr int kProbBad = kProbBins;            // label >= C and not `ignore`
constexpr int kProbIgnored = kProbBins + 1;    // label == ignore
constexpr int kProbCells = kProbIgnored + 1;

__global__ __launch_bounds__(kEvalThreads) void eval_prob_hist_kernel(const uint8_t* __restrict__ prob, const uint8_t* __restrict__ actual,
                                                                      unsigned long long* __restrict__ hist_out,
                                                                      unsigned long long* __restrict__ skipped, long pixels, long group,
                                                                      unsigned int C, unsigned int cls, unsigned int ignore) {
  __shared__ unsigned int hist[4][kProbCells];
  const long block0 = (long)blockIdx.x * kEvalBlock;
  const long base = block0 + (long)threadIdx.x * kEvalRun;
  unsigned int qw[4] = {0, 0, 0, 0};  // 16 probability bytes
  unsigned int codes = 0;             // 16 x 2 bits: 0 negative, 1 positive, 2 bad, 3 ignored (cells kProbBad - 2 + code)
  if (base < pixels) {
    unsigned int aw[4];
    eval_load_bytes(prob, base, pixels, qw);
    eval_load_bytes(actual, base, pixels, aw);
#pragma unroll
    for (int j = 0; j < kEvalRun; ++j) {
      const unsigned int a = (aw[j >> 2] >> ((j & 3) * 8)) & 255u;
      const unsigned int code = a < C ? (unsigned int)(a == cls) : a == ignore ? 3u : 2u;  // (ignore is 256 where there is none)
      codes |= code << (2 * j);
    }
  }
  for (int i = threadIdx.x; i < 4 * kProbCells; i += kEvalThreads) (&hist[0][0])[i] = 0;
  __syncthreads();
  const long block1 = block0 + kEvalBlock < pixels ? block0 + kEvalBlock : pixels;
  const long g0 = block0 / group, g1 = (block1 - 1) / group;
  unsigned int* h = hist[threadIdx.x >> 6];
  const int lane = threadIdx.x & 63;
  for (long g = g0; g <= g1; ++g) {
    int jlo, jhi;
    eval_range(base, g, group, pixels, jlo, jhi);
    // the thread's first cell of the group, and whether all its pixels of the group lie in it
    unsigned int first = 0;
    bool same = true;
#pragma unroll
    for (int j = kEvalRun - 1; j >= 0; --j) {
      if (j >= jlo && j < jhi) {
        const unsigned int code = (codes >> (2 * j)) & 3u, q = (qw[j >> 2] >> ((j & 3) * 8)) & 255u;
        const unsigned int cell = code < 2u ? (code << 8) | q : (unsigned int)kProbBad - 2u + code;
        same = same && (j == jhi - 1 || cell == first);
        first = cell;
      }
    }
    unsigned int n = jhi > jlo ? (unsigned int)(jhi - jlo) : 0u;
    const unsigned long long live = __ballot(n != 0u);
    if (live) {  // (wave-uniform)
      const unsigned int lead = __shfl(first, __ffsll((long long)live) - 1, 64);
      if (__all(n == 0u || (same && first == lead))) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
        if (lane == 0) atomicAdd(&h[lead], n);
      } else {
        unsigned int cur = 0, run = 0;
#pragma unroll
        for (int j = 0; j < kEvalRun; ++j) {
          if (j >= jlo && j < jhi) {
            const unsigned int code = (codes >> (2 * j)) & 3u, q = (qw[j >> 2] >> ((j & 3) * 8)) & 255u;
            const unsigned int cell = code < 2u ? (code << 8) | q : (unsigned int)kProbBad - 2u + code;
            if (run && cell != cur) {
              atomicAdd(&h[cur], run);
              run = 0;
            }
            cur = cell;
            ++run;
          }
        }
        if (run) atomicAdd(&h[cur], run);
      }
    }
    __syncthreads();
    // merge: a thread owns cells t and t + 256 (threads 0 and 1 also the two counters behind them) in all four copies
    for (int t = threadIdx.x; t < kProbCells; t += kEvalThreads) {
      const unsigned int tot = hist[0][t] + hist[1][t] + hist[2][t] + hist[3][t];
      if (tot) {
        hist[0][t] = hist[1][t] = hist[2][t] = hist[3][t] = 0;
        if (t < kProbBins)
          atomicAdd(&hist_out[g * kProbBins + t], (unsigned long long)tot);
        else
          atomicAdd(&skipped[g * 2 + (t - kProbBins)], (unsigned long long)tot);
      }
    }
    __syncthreads();  // (the next group counts into the cells put back to zero)
  }
}

}  // namespace

extern "C" int rs_eval_prob_hist(const uint8_t* prob, const uint8_t* actual, int64_t* hist, int64_t* skipped, long pixels, long group, int C,
                                 int cls, int ignore, rs_stream_t stream) {
  if (!prob || !actual || !hist || !skipped || (((uintptr_t)hist | (uintptr_t)skipped) & 7) || !eval_shape_ok(pixels, group) || C < 2 ||
      C > 8 || cls < 1 || cls >= C || (ignore != -1 && (ignore < C || ignore > 255)))
    return RS_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const long groups = pixels / group;
  // (one fill where `skipped` follows `hist` directly, as ops.prob_histogram lays them out)
  const bool joined = skipped == hist + groups * kProbBins;
  hipError_t e = hipMemsetAsync(hist, 0, groups * (kProbBins + (joined ? 2 : 0)) * sizeof(int64_t), s);
  if (e == hipSuccess && !joined) e = hipMemsetAsync(skipped, 0, groups * 2 * sizeof(int64_t), s);
  if (e != hipSuccess) return (int)e;
  eval_prob_hist_kernel<<<rs_cdiv(pixels, kEvalBlock), kEvalThreads, 0, s>>>(
      prob, actual, reinterpret_cast<unsigned long long*>(hist), reinterpret_cast<unsigned long long*>(skipped), pixels, group,
      (unsigned int)C, (unsigned int)cls, ignore < 0 ? 256u : (unsigned int)ignore);
  return RS_LAUNCH_RESULT();
}

// ---- centre lines: links and matched links per group (rs_eval_centerline) ----------------------------------------------------
// `rs evaluate --centerline`: the buffer method on two skeletons.  A link runs from a set pixel to its E, S, SE or SW neighbour (the
// rule of rs_features_skeleton_links), so a thread needs the row below its pixels: runs are laid over ROWS here, not over the call.
// A row of W pixels is cut into cdiv(W, 16) runs; run r of the call is run r % RW of row r / RW of all B*H rows, a thread owns one
// run and a block 256 consecutive ones, which lie in consecutive tiles: a block may straddle tiles or hold many small ones.
//
// A thread keeps a row of a skeleton as 18 bits: bit 0 the pixel west of its run, bits 1..n its n <= 16 pixels, bit n + 1 the pixel east
// of them; the same for the row below.  Beyond the tile those pixels are the facing ones of the neighbouring tile through nbr, 0 where
// the tile is absent or no table was given.  The four kinds of link are then four words of bit logic.  The transforms are read ONLY
// by threads whose run starts a link (a skeleton is a percent or two of a raster): where W is a multiple of 4 the four rows of a whole
// run at once, 16-byte loads that do not wait for each other; otherwise the bits of the link ends are walked, one int32 load each, at
// most 18 per row.  Every index comes from cl_pixel, which gives -1 for anything outside the call's tiles; a distance counts only
// where a skeleton byte was read as set, so through the same index, and a load that has no pixel reads the call's first ones.
//
// Counts are merged as in eval_boundary_kernel: bit counts within a thread, a sum over the wave's lanes, the four waves in LDS, one
// 64-bit atomic add per block, group and non-zero counter.  The eight counters travel as four words of two 16-bit halves: a thread
// has at most 32 links of a kind, a wave 2048, a block 8192.  No workgroup waits for another; every loop is bounded (the bit walks
// by 18, the group loop by the block's 256 runs).
namespace {

constexpr int kClRun = 16;  // pixels of a thread's run (one row)
constexpr int kClCounters = 8;

// Slot of the tile at (dx, dy) from `tile` in the neighbour table (order NW N NE W E SW S SE), -1 where absent or out of range.
__device__ __forceinline__ int cl_slot(const int* __restrict__ nbr, int tile, int dx, int dy, int B) {
  const int k = (dy + 1) * 3 + (dx + 1);
  const int n = nbr[(long)tile * 8 + (k > 4 ? k - 1 : k)];
  return n >= 0 && n < B ? n : -1;
}

// Index in the call of pixel (x, y) of `tile`, x in -1 .. W and y in 0 .. H: the facing pixel of the neighbouring tile where it lies
// beyond the tile, -1 where there is none.  (B*H*W < 2^31: every index fits an int.)
template <bool STITCH>
__device__ __forceinline__ int cl_pixel(const int* __restrict__ nbr, int tile, int x, int y, int B, int H, int W) {
  const int dx = x < 0 ? -1 : x >= W ? 1 : 0, dy = y >= H ? 1 : 0;
  int slot = tile;
  if (dx | dy) {
    if (!STITCH) return -1;
    slot = cl_slot(nbr, tile, dx, dy, B);
    if (slot < 0) return -1;
  }
  return (slot * H + (y - dy * H)) * W + (x - dx * W);
}

// The three places a thread reads a row at: its own n pixels from `own`, one pixel at `west`, one at `east`; -1 where there is none.
struct ClRow {
  int own, west, east;
};

template <bool STITCH>
__device__ __forceinline__ ClRow cl_row(const int* __restrict__ nbr, int tile, int x0, int n, int y, int B, int H, int W) {
  ClRow r;
  r.own = cl_pixel<STITCH>(nbr, tile, x0, y, B, H, W);
  r.west = cl_pixel<STITCH>(nbr, tile, x0 - 1, y, B, H, W);
  r.east = cl_pixel<STITCH>(nbr, tile, x0 + n, y, B, H, W);
  return r;
}

// The 18 bits of a skeleton's row (non-zero = set).
__device__ __forceinline__ unsigned int cl_row_bits(const uint8_t* __restrict__ s, const ClRow& r, int n) {
  unsigned int bits = 0;
  if (r.own >= 0) {
    if (n == kClRun && (reinterpret_cast<uintptr_t>(s + r.own) & 15) == 0) {
      const u32x4 q = *reinterpret_cast<const u32x4*>(s + r.own);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        // bit 7 of every non-zero byte (no carry leaves a byte: 0x7f + 0x7f), then the four bits side by side: bit 8i moves to
        // 8i + 7j under the factor's term 2^(7j), no two terms meet, and bits 21 .. 24 are bytes 0 .. 3
        const unsigned int t = ((q[e] | ((q[e] & 0x7f7f7f7fu) + 0x7f7f7f7fu)) & 0x80808080u) >> 7;
        bits |= ((t * 0x00204081u >> 21) & 15u) << (4 * e + 1);
      }
    } else {
#pragma unroll
      for (int j = 0; j < kClRun; ++j)
        if (j < n) bits |= (unsigned int)(s[r.own + j] != 0) << (j + 1);
    }
  }
  // (no branch round the two single loads: where there is no pixel the call's first byte is read and masked away, so that the
  // loads of all four rows can be in flight together)
  bits |= (unsigned int)(s[r.west >= 0 ? r.west : 0] != 0) & (unsigned int)(r.west >= 0);
  bits |= ((unsigned int)(s[r.east >= 0 ? r.east : 0] != 0) & (unsigned int)(r.east >= 0)) << (n + 1);
  return bits;
}

// Bit k set where bit k of `need` is and d2 <= rr at that pixel.  `need` holds only pixels that cl_row_bits read as set.
__device__ __forceinline__ unsigned int cl_near_bits(const int* __restrict__ d2, const ClRow& r, int n, unsigned int need, int rr) {
  unsigned int bits = 0;
  for (int it = 0; it < kClRun + 2 && need; ++it) {
    const int k = __ffs((int)need) - 1;
    need &= need - 1u;
    const int at = k == 0 ? r.west : k == n + 1 ? r.east : r.own + (k - 1);
    if (at >= 0) bits |= (unsigned int)(d2[at] <= rr) << k;  // (at >= 0 by construction)
  }
  return bits;
}

// The same for a whole run of 16 at once, where every row of the transforms begins at a 16-byte boundary (`fast` in the kernel):
// four 16-byte loads and the two single ones, none depending on another, so that all four rows of a thread are one round trip to
// memory where the walk above is one per link end.  Where there is no pixel the call's first ones are read (B*H*W >= 16 here);
// the caller looks at the bits of link ends only, which are pixels that are there.
__device__ __forceinline__ unsigned int cl_near_row(const int* __restrict__ d2, const ClRow& r, int rr) {
  const u32x4* own = reinterpret_cast<const u32x4*>(d2 + (r.own >= 0 ? r.own : 0));
  u32x4 q[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) q[e] = own[e];
  const int west = d2[r.west >= 0 ? r.west : 0], east = d2[r.east >= 0 ? r.east : 0];
  unsigned int bits = (unsigned int)(west <= rr) | (unsigned int)(east <= rr) << (kClRun + 1);
#pragma unroll
  for (int j = 0; j < kClRun; ++j) bits |= (unsigned int)((int)q[j >> 2][j & 3] <= rr) << (j + 1);
  return bits;
}

// The links that start in a thread's run, one word per kind, from the bits c of its row and b of the row below.
struct ClLinks {
  unsigned int e, s, se, sw;
};

__device__ __forceinline__ ClLinks cl_links(unsigned int c, unsigned int b, int n) {
  const unsigned int own = ((1u << n) - 1u) << 1;
  ClLinks l;
  l.e = c & (c >> 1) & own;
  l.s = c & b & own;
  l.se = c & (b >> 1) & ~(c >> 1) & ~b & own;
  l.sw = c & (b << 1) & ~(c << 1) & ~b & own;
  return l;
}

// straight | diagonal << 16
__device__ __forceinline__ unsigned int cl_count(const ClLinks& l) {
  return (unsigned int)(__popc(l.e) + __popc(l.s)) | (unsigned int)(__popc(l.se) + __popc(l.sw)) << 16;
}

// The link ends in the thread's row and in the row below: where the other side's transform is looked at.
__device__ __forceinline__ unsigned int cl_ends_row(const ClLinks& l) { return l.e | l.s | l.se | l.sw | (l.e << 1); }
__device__ __forceinline__ unsigned int cl_ends_below(const ClLinks& l) { return l.s | (l.se << 1) | (l.sw >> 1); }

// The links with both ends near: nc, nb = the near bits of the row and of the row below, right at least at the link ends.
__device__ __forceinline__ ClLinks cl_matched(const ClLinks& l, unsigned int nc, unsigned int nb) {
  ClLinks m;
  m.e = l.e & nc & (nc >> 1);
  m.s = l.s & nc & nb;
  m.se = l.se & nc & (nb >> 1);
  m.sw = l.sw & nc & (nb << 1);
  return m;
}

template <bool STITCH>
__global__ __launch_bounds__(kEvalThreads) void eval_centerline_kernel(const uint8_t* __restrict__ skel_p, const uint8_t* __restrict__ skel_g,
                                                                       const int* __restrict__ d2_to_g, const int* __restrict__ d2_to_p,
                                                                       const int* __restrict__ nbr, unsigned long long* __restrict__ counts,
                                                                       int B, int H, int W, int rr) {
  __shared__ unsigned int part[4][kClCounters / 2];
  const int RW = (W + kClRun - 1) / kClRun;
  // (runs <= B*H*W < 2^31, and the grid's last run index is below runs + 256: 32-bit arithmetic, whose divisions are cheap)
  const unsigned int per_tile = (unsigned int)H * RW, runs = per_tile * B;
  const unsigned int r0 = blockIdx.x * kEvalThreads, r = r0 + threadIdx.x;
  // every row of both transforms begins at a 16-byte boundary (and then W >= 16 wherever a run is whole)
  const bool fast = (W & 3) == 0 && ((reinterpret_cast<uintptr_t>(d2_to_g) | reinterpret_cast<uintptr_t>(d2_to_p)) & 15) == 0;
  unsigned int w[kClCounters / 2] = {0, 0, 0, 0};
  int tile = -1;
  if (r < runs) {
    tile = (int)(r / per_tile);
    const unsigned int in_tile = r - tile * per_tile;
    const int y = (int)(in_tile / RW), x0 = (int)(in_tile - y * RW) * kClRun;
    const int n = W - x0 < kClRun ? W - x0 : kClRun;
    const ClRow cur = cl_row<STITCH>(nbr, tile, x0, n, y, B, H, W), below = cl_row<STITCH>(nbr, tile, x0, n, y + 1, B, H, W);
    const unsigned int pc = cl_row_bits(skel_p, cur, n), pb = cl_row_bits(skel_p, below, n);
    const unsigned int gc = cl_row_bits(skel_g, cur, n), gb = cl_row_bits(skel_g, below, n);
    const ClLinks lp = cl_links(pc, pb, n), lg = cl_links(gc, gb, n);
    w[0] = cl_count(lp);
    w[2] = cl_count(lg);
    if (w[0] | w[2]) {
      unsigned int pnc, pnb, gnc, gnb;  // near the OTHER skeleton: the prediction's link ends in d2_to_g, the label's in d2_to_p
      if (fast && n == kClRun) {
        pnc = cl_near_row(d2_to_g, cur, rr), pnb = cl_near_row(d2_to_g, below, rr);
        gnc = cl_near_row(d2_to_p, cur, rr), gnb = cl_near_row(d2_to_p, below, rr);
      } else {
        pnc = cl_near_bits(d2_to_g, cur, n, cl_ends_row(lp), rr), pnb = cl_near_bits(d2_to_g, below, n, cl_ends_below(lp), rr);
        gnc = cl_near_bits(d2_to_p, cur, n, cl_ends_row(lg), rr), gnb = cl_near_bits(d2_to_p, below, n, cl_ends_below(lg), rr);
      }
      w[1] = cl_count(cl_matched(lp, pnc, pnb));
      w[3] = cl_count(cl_matched(lg, gnc, gnb));
    }
  }
  const unsigned int r1 = r0 + kEvalThreads < runs ? r0 + kEvalThreads : runs;  // (r0 < runs: the grid is cdiv(runs, kEvalThreads))
  const int g0 = STITCH ? 0 : (int)(r0 / per_tile), g1 = STITCH ? 0 : (int)((r1 - 1) / per_tile);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int g = g0; g <= g1; ++g) {
    const bool mine = tile >= 0 && (STITCH || tile == g);
#pragma unroll
    for (int k = 0; k < kClCounters / 2; ++k) {
      unsigned int v = mine ? w[k] : 0u;
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);  // (each half at most 64 * 32: no carry)
      if (lane == 0) part[wave][k] = v;
    }
    __syncthreads();
    if (threadIdx.x < kClCounters) {
      const int t = threadIdx.x, sh = (t & 1) * 16;
      const unsigned int tot = ((part[0][t >> 1] >> sh) & 0xffffu) + ((part[1][t >> 1] >> sh) & 0xffffu) + ((part[2][t >> 1] >> sh) & 0xffffu) +
                               ((part[3][t >> 1] >> sh) & 0xffffu);
      if (tot) atomicAdd(&counts[(long)g * kClCounters + t], (unsigned long long)tot);
    }
    __syncthreads();  // (the next group overwrites the partial sums)
  }
}

}  // namespace

extern "C" int rs_eval_centerline(const uint8_t* skel_p, const uint8_t* skel_g, const int32_t* d2_to_g, const int32_t* d2_to_p,
                                  const int32_t* nbr, int64_t* counts, int B, int H, int W, int rho, rs_stream_t stream) {
  if (!skel_p || !skel_g || !d2_to_g || !d2_to_p || !counts || ((uintptr_t)counts & 7) || B < 1 || H < 1 || W < 1 || rho < 1 || rho > 127)
    return RS_EINVAL;
  const long hw = (long)H * W;  // (H, W < 2^31: no overflow)
  if (hw >= (1l << 31) || (long)B * hw >= (1l << 31)) return RS_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const hipError_t e = hipMemsetAsync(counts, 0, (nbr ? 1 : (long)B) * kClCounters * sizeof(int64_t), s);
  if (e != hipSuccess) return (int)e;
  const long runs = (long)B * H * ((W + kClRun - 1) / kClRun);
  unsigned long long* c = reinterpret_cast<unsigned long long*>(counts);
  if (nbr)
    eval_centerline_kernel<true><<<rs_cdiv(runs, kEvalThreads), kEvalThreads, 0, s>>>(skel_p, skel_g, d2_to_g, d2_to_p, nbr, c, B, H, W, rho * rho);
  else
    eval_centerline_kernel<false><<<rs_cdiv(runs, kEvalThreads), kEvalThreads, 0, s>>>(skel_p, skel_g, d2_to_g, d2_to_p, nullptr, c, B, H, W,
                                                                                      rho * rho);
  return RS_LAUNCH_RESULT();
}
