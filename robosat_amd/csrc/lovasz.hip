// LovaszLoss2d (reference robosat/losses.py:86-119) on the GPU, all images of the batch in one set of launches.
//
// Per image n, over the flattened C*H*W vector i (NCHW order, i = c*HW + hw) with the one-hot mask m_i as labels:
//     err_i   = 1 - (2 m_i - 1) * x_i
//     sort err descending (permutation pi), lab_r = m_{pi(r)}
//     inter_r = gts - cumsum(lab)_r ;  union_r = gts + cumsum(1 - lab)_r ;  jac_r = 1 - inter_r / union_r
//     delta_0 = jac_0, delta_r = jac_r - jac_{r-1}
//     loss_n  = sum_r relu(err_{pi(r)}) * delta_r ;   loss = mean_n loss_n
// gts = sum(m) = H*W exactly (one label per pixel).  All of inter/union/jac/delta are evaluated in fp32 with the same
// operations as the reference, so for the same permutation they are bit-identical to torch's.
// Gradient (what autograd gives the reference): d loss / d x_i = -(2 m_i - 1) * [err_i > 0] * delta_{rank(i)} / N.
//
// Sort = LSD radix sort, 4 passes x 8 bits, keys = order-preserving uint32 image of err (inverted for descending),
// payload = i | (m_i << 31).  Each pass: per-block digit histograms -> per-image exclusive scan (digit-major) ->
// stable scatter.  The scatter works on 8192-element tiles: every wave ranks its 2048 elements among equal digits
// (64-bit ballots per batch of 64 + wave-private running counters in LDS), the tile is first sorted by digit INSIDE LDS,
// and only then written out -- consecutive threads then write consecutive addresses of a digit's run, instead of 4-byte
// stores sprayed over 256 buckets (which cost the first version 0.39 ms per pass against a 0.07 ms traffic bound).
// The rest is a segmented prefix sum (block sums -> scan -> apply) fused with the Jaccard deltas, the dot product
// (fp64 partials) and the gradient scatter.  HBM-bound integer/byte work throughout.
//
// The same sort and scans also carry the multi-class Lovasz-Softmax loss (rs_lovasz_softmax_fwd, further down): the sort then
// runs over N*C (or C) segments of one class's errors instead of N segments of C*H*W hinge errors.
//
// Both losses also exist over the pixels whose label is not `ignore` (rs_lovasz_fwd_ig, rs_lovasz_softmax_fwd_ig): the loss of the
// valid pixels alone, as if the ignored ones had been cut out of every image and the rest packed in (n, h, w) order.  The kernels
// that look at a label or an error are templates over `bool Ignore`, the variant's statements under `if constexpr`; the sort, the
// scans and the workspace serve both as they are.  An ignored pixel's C entries get a key that sorts strictly behind every valid
// key -- an error of -inf in the hinge form (valid errors are finite), of -1 in the softmax form (valid errors lie in [0, 1]) -- and
// label bit 0.  The sort is stable, so they form the TAIL of their segment and the valid entries keep the order, the ranks and the
// label prefix counts they would have without them: every valid rank keeps its delta.  Each segment's gts is its number of set
// label bits, which only valid pixels have (in the hinge form: one per valid pixel, so gts = K of the image where the plain form
// has H*W).  The apply kernels add 0 to the loss for a tail entry and write +0.0f as its gradient.  With no pixel ignored an Ignore
// instantiation does the arithmetic of the plain one in the same order: the same bits.  A variant's kernel takes the arguments it
// uses, the plain ones in the places they have always had, so the instantiations are the instructions of the separate kernels they
// replaced, bar the few that profiles/loss_variants/README.md lists and times (an operand order in the apply kernels, which now
// share lovasz_load4, and the argument loads of the two Ignore kernels whose arguments moved).
#include <type_traits>

#include "common.h"

namespace {

// elements per 256-thread block of the sort kernels: 8192 (4 waves x 32 batches of 64; 68 KB of LDS: two blocks per CU) or,
// for the large sorts, 4096 (four blocks per CU: -9 % on the bs-32 step's 16.8 M keys, -14 % at 33.5 M; +7 % on a bs-8 step's
// 4.2 M keys, where twice as many per-block histograms outweigh it: profiles/r05/lovasz.txt).  Chosen by the total key count;
// the sort is exact and stable either way.
constexpr long kSmallSortKeys = 8L << 20;
inline int sort_chunk(long total_keys) { return total_keys >= kSmallSortKeys ? 4096 : 8192; }
constexpr int kScanChunk = 1024;  // elements per 256-thread block in the prefix-sum kernels

typedef unsigned int lv_u32x4 __attribute__((ext_vector_type(4)));
typedef long long lv_i64x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ uint32_t desc_key(float f) {
  const uint32_t u = __float_as_uint(f);
  const uint32_t asc = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return ~asc;
}

__device__ __forceinline__ float key_to_float(uint32_t key) {
  const uint32_t asc = ~key;
  const uint32_t u = (asc & 0x80000000u) ? (asc & 0x7fffffffu) : ~asc;
  return __uint_as_float(u);
}

// What an Ignore instantiation needs beyond the plain arguments is ONE trailing argument: the pack `extra` holds nothing (plain, which
// so keeps the argument list it has always had) or `int ignore` -- an IgnoredLabels where the plain kernel reads no labels -- and
// `(extra, ...)` is that argument.  (Written out where it is used: an accessor function inside a select's condition changed the
// instructions of lovasz_keys_kernel.)
struct IgnoredLabels {
  const long long* tgt;
  int ignore;
};

template <bool Ignore, typename... Extra>
__global__ void lovasz_keys_kernel(const float* __restrict__ x, const long long* __restrict__ tgt, uint32_t* __restrict__ keys,
                                   uint32_t* __restrict__ vals, long P, long HW, Extra... extra) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long n = blockIdx.y;
  if (i >= P) return;
  const long c = i / HW, hw = i - c * HW;
  const long long t = tgt[n * HW + hw];
  const uint32_t m = (t == c) ? 1u : 0u;
  const float v = x[n * P + i];
  float err;  // 1 - (2m-1)*x
  if constexpr (Ignore) err = (t == (extra, ...)) ? -INFINITY : 1.f - (m ? v : -v);
  else err = 1.f - (m ? v : -v);
  keys[n * P + i] = desc_key(err);
  vals[n * P + i] = (uint32_t)i | (m << 31);
}

// The same for HW % 4 == 0 (every tile size the tools produce): four consecutive pixels of one class plane per thread -- one
// 16-byte load of the logits, two of the int64 labels, two 16-byte stores (round 5: the scalar kernel ran at ~2.5 TB/s).
template <bool Ignore, typename... Extra>
__global__ __launch_bounds__(256) void lovasz_keys4_kernel(const float* __restrict__ x, const long long* __restrict__ tgt,
                                                           uint32_t* __restrict__ keys, uint32_t* __restrict__ vals, long P, long HW,
                                                           Extra... extra) {
  const long i = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
  const long n = blockIdx.y;
  if (i >= P) return;
  const long c = i / HW, hw = i - c * HW;  // (HW % 4 == 0: the four elements share the class plane)
  const f32x4 v = *reinterpret_cast<const f32x4*>(x + n * P + i);
  const lv_i64x2 t0 = *reinterpret_cast<const lv_i64x2*>(tgt + n * HW + hw), t1 = *reinterpret_cast<const lv_i64x2*>(tgt + n * HW + hw + 2);
  const long long t[4] = {t0[0], t0[1], t1[0], t1[1]};
  lv_u32x4 k, w;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const uint32_t m = (t[e] == c) ? 1u : 0u;
    float err;
    if constexpr (Ignore) err = (t[e] == (extra, ...)) ? -INFINITY : 1.f - (m ? v[e] : -v[e]);
    else err = 1.f - (m ? v[e] : -v[e]);
    k[e] = desc_key(err);
    w[e] = (uint32_t)(i + e) | (m << 31);
  }
  *reinterpret_cast<lv_u32x4*>(keys + n * P + i) = k;
  *reinterpret_cast<lv_u32x4*>(vals + n * P + i) = w;
}

// counts[n][b][256]
template <int CHUNK>
__global__ __launch_bounds__(256) void radix_hist_kernel(const uint32_t* __restrict__ keys, uint32_t* __restrict__ counts,
                                                         long P, int nblk, int shift) {
  __shared__ uint32_t hist[256];
  const int tid = threadIdx.x;
  const long n = blockIdx.y;
  const int b = blockIdx.x;
  hist[tid] = 0;
  __syncthreads();
  const long base = (long)b * CHUNK;
  if ((P & 3) == 0) {  // 16-byte loads: four consecutive keys per thread
    for (int k = 0; k < CHUNK / 1024; ++k) {
      const long i = base + (k * 256 + tid) * 4;
      if (i < P) {
        // (counting the lanes that share a digit by ballot and adding once per group was measured: -50 % on the passes whose
        // digits are concentrated -- sign + exponent -- and +60 % on the uniform ones; a wash over a sort: profiles/r05/lovasz.txt)
        const lv_u32x4 v = *reinterpret_cast<const lv_u32x4*>(keys + n * P + i);
#pragma unroll
        for (int e = 0; e < 4; ++e) atomicAdd(&hist[(v[e] >> shift) & 255u], 1u);
      }
    }
  } else {
    for (int k = 0; k < CHUNK / 256; ++k) {
      const long i = base + k * 256 + tid;
      if (i < P) atomicAdd(&hist[(keys[n * P + i] >> shift) & 255u], 1u);
    }
  }
  __syncthreads();
  counts[(n * nblk + b) * 256 + tid] = hist[tid];
}

// exclusive scan of counts in (digit-major, block-minor) order, per image; in place: counts -> offsets.  One block of 1024 per
// image: digit d = tid & 255, quarter g = tid >> 8 of the blocks (round 4: 256 threads walked all blocks twice -- 22-30 us of
// dependent round trips for a few hundred KB, four times per sort).
__global__ __launch_bounds__(1024) void radix_scan_kernel(uint32_t* __restrict__ counts, int nblk) {
  __shared__ uint32_t part[4][256];
  __shared__ uint32_t tot[256];
  const int d = threadIdx.x & 255, g = threadIdx.x >> 8;
  uint32_t* c = counts + (long)blockIdx.x * nblk * 256;
  const int q = (nblk + 3) / 4;
  const int b0 = g * q, b1 = (b0 + q) < nblk ? (b0 + q) : nblk;
  uint32_t s = 0;
  for (int b = b0; b < b1; ++b) s += c[(long)b * 256 + d];
  part[g][d] = s;
  __syncthreads();
  if (g == 0) tot[d] = (part[0][d] + part[1][d]) + (part[2][d] + part[3][d]);
  __syncthreads();
  if (threadIdx.x < 64) {  // exclusive scan of the 256 digit totals by one wave: 4 digits per lane
    const int l = threadIdx.x;
    const uint32_t t0 = tot[4 * l], t1 = tot[4 * l + 1], t2 = tot[4 * l + 2], t3 = tot[4 * l + 3];
    const uint32_t mine = t0 + t1 + t2 + t3;
    uint32_t inc = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t t = __shfl_up(inc, o, 64);
      if (l >= o) inc += t;
    }
    const uint32_t ex = inc - mine;
    tot[4 * l] = ex;
    tot[4 * l + 1] = ex + t0;
    tot[4 * l + 2] = ex + t0 + t1;
    tot[4 * l + 3] = ex + t0 + t1 + t2;
  }
  __syncthreads();
  uint32_t run = tot[d];
  for (int gg = 0; gg < g; ++gg) run += part[gg][d];
  for (int b = b0; b < b1; ++b) {
    const uint32_t t = c[(long)b * 256 + d];
    c[(long)b * 256 + d] = run;
    run += t;
  }
}

// The same scan for FEW long segments (the flattened Lovasz-Softmax: C segments of N*H*W keys, thousands of sort tiles each),
// where one 1024-thread block per segment walks its tiles' counts in a chain of dependent loads (143 us a pass at 2 x 2048
// tiles).  In three launches instead: per chunk of kScanTiles tiles, the digit sums (thread d = digit d: coalesced rows);
// radix_scan_kernel over those chunk sums (= each chunk's first offsets); per chunk, the tiles' offsets from there.
constexpr int kScanTiles = 64;

__global__ __launch_bounds__(256) void radix_chunk_sum_kernel(const uint32_t* __restrict__ counts, uint32_t* __restrict__ csum,
                                                              int nblk, int nchunk) {
  const long n = blockIdx.y;
  const int b0 = blockIdx.x * kScanTiles, b1 = (b0 + kScanTiles) < nblk ? (b0 + kScanTiles) : nblk;
  const uint32_t* c = counts + n * nblk * 256 + threadIdx.x;
  uint32_t s = 0;
  for (int b = b0; b < b1; ++b) s += c[(long)b * 256];
  csum[(n * nchunk + blockIdx.x) * 256 + threadIdx.x] = s;
}

__global__ __launch_bounds__(256) void radix_chunk_offsets_kernel(uint32_t* __restrict__ counts, const uint32_t* __restrict__ coff,
                                                                  int nblk, int nchunk) {
  const long n = blockIdx.y;
  const int b0 = blockIdx.x * kScanTiles, b1 = (b0 + kScanTiles) < nblk ? (b0 + kScanTiles) : nblk;
  uint32_t* c = counts + n * nblk * 256 + threadIdx.x;
  uint32_t run = coff[(n * nchunk + blockIdx.x) * 256 + threadIdx.x];
  for (int b = b0; b < b1; ++b) {
    const uint32_t t = c[(long)b * 256];
    c[(long)b * 256] = run;
    run += t;
  }
}

template <int CHUNK>
__global__ __launch_bounds__(256) void radix_scatter_kernel(const uint32_t* __restrict__ keys, const uint32_t* __restrict__ vals,
                                                            uint32_t* __restrict__ okeys, uint32_t* __restrict__ ovals,
                                                            const uint32_t* __restrict__ offsets, long P, int nblk, int shift,
                                                            int xcd_affine) {
  // Round 5: each element's rank inside its wave is fixed in the FIRST sweep -- one ballot match per batch of 64, the leader
  // of every digit group adds the group's size to the wave's counter with a RETURNING LDS atomic (= the elements of that digit
  // in the wave's earlier batches) and hands it to the group by a lane read -- and kept in a register; the second sweep is then
  // one table read + one 8-byte store per element.  Rounds 1-4 counted first (an atomic per element), matched again in the
  // second sweep and read + updated the running counters there: ~8 scattered LDS operations per element against ~4 now
  // (scattered = bank conflicts by construction: SQ_LDS_BANK_CONFLICT was 64 % of this kernel's LDS cycles).  Same output.
  constexpr int WCH = CHUNK / 4;       // elements per wave
  constexpr int NB = WCH / 64;         // batches of 64 per wave
  __shared__ u32x2 lkv[CHUNK];         // the tile, sorted by digit: (key, value)
  __shared__ uint32_t loc[4][256];     // per wave: histogram, then position of the wave's first element of each digit in the tile
  __shared__ uint32_t gdelta[256];     // global position of a digit's run minus its position in the tile
  __shared__ uint32_t wsum[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  long n = blockIdx.y;
  int b = blockIdx.x;
  if (xcd_affine) {  // all tiles of an image on one XCD (see lovasz_apply_kernel)
    const long L = (long)blockIdx.y * gridDim.x + blockIdx.x;
    const long k = L >> 3;
    n = (L & 7) + 8 * (k / nblk);
    b = (int)(k % nblk);
  }
  const long start = (long)b * CHUNK + wave * WCH;

  uint32_t key[NB], val[NB], rnk[NB];
#pragma unroll
  for (int w = 0; w < 4; ++w) loc[w][tid] = 0;
  __syncthreads();
  const unsigned long long lt = (1ull << lane) - 1ull;
#pragma unroll
  for (int k = 0; k < NB; ++k) {  // fully unrolled: key[] / val[] / rnk[] stay in registers
    const long i = start + k * 64 + lane;
    const bool valid = i < P;
    key[k] = 0xffffffffu;
    val[k] = 0;
    if (valid) {
      key[k] = keys[n * P + i];
      val[k] = vals[n * P + i];
    }
    const uint32_t d = (key[k] >> shift) & 255u;
    unsigned long long peers = __ballot(valid);
#pragma unroll
    for (int bit = 0; bit < 8; ++bit) {
      const bool one = (d >> bit) & 1u;
      const unsigned long long bm = __ballot(valid && one);
      peers &= one ? bm : ~bm;
    }
    // loc[wave][] is private to this wave and a wave's LDS operations execute in issue order: batch k + 1's atomic sees batch k's
    const int leader = __ffsll((long long)peers) - 1;
    uint32_t before = 0;
    if (valid && leader == lane) before = atomicAdd(&loc[wave][d], (uint32_t)__popcll(peers));
    before = __shfl(before, leader & 63, 64);
    rnk[k] = before + (uint32_t)__popcll(peers & lt);
  }
  __syncthreads();
  {  // digit-major, wave-minor exclusive offsets inside the tile (thread d owns digit d)
    const uint32_t c0 = loc[0][tid], c1 = loc[1][tid], c2 = loc[2][tid], c3 = loc[3][tid];
    const uint32_t tot = c0 + c1 + c2 + c3;
    uint32_t inc = tot;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t t = __shfl_up(inc, o, 64);
      if (lane >= o) inc += t;
    }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    uint32_t woff = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w)
      if (w < wave) woff += wsum[w];
    const uint32_t ex = woff + inc - tot;  // elements of smaller digits in the tile
    loc[0][tid] = ex;
    loc[1][tid] = ex + c0;
    loc[2][tid] = ex + c0 + c1;
    loc[3][tid] = ex + c0 + c1 + c2;
    gdelta[tid] = offsets[(n * nblk + b) * 256 + tid] - ex;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < NB; ++k) {
    if ((start + k * 64 + lane) < P) {
      u32x2 kv;
      kv[0] = key[k];
      kv[1] = val[k];
      lkv[loc[wave][(key[k] >> shift) & 255u] + rnk[k]] = kv;
    }
  }
  __syncthreads();
  const long tile0 = (long)b * CHUNK;
  const int count = (int)((P - tile0) < CHUNK ? (P - tile0) : CHUNK);
  for (int i = tid; i < count; i += 256) {
    const u32x2 kv = lkv[i];
    const uint32_t g = gdelta[(kv[0] >> shift) & 255u] + (uint32_t)i;
    okeys[n * P + g] = kv[0];
    ovals[n * P + g] = kv[1];
  }
}

__device__ __forceinline__ uint32_t block_exclusive_scan_256(uint32_t v, uint32_t* smem /*[4]*/, uint32_t* total) {
  // inclusive scan inside the wave
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t t = __shfl_up(inc, o, 64);
    if (lane >= o) inc += t;
  }
  if (lane == 63) smem[wave] = inc;
  __syncthreads();
  uint32_t woff = 0;
#pragma unroll
  for (int w = 0; w < 4; ++w)
    if (w < wave) woff += smem[w];
  *total = smem[0] + smem[1] + smem[2] + smem[3];
  return woff + inc - v;
}

// per-block number of labels among the sorted elements: bsum[n][b]
__global__ __launch_bounds__(256) void lovasz_blocksum_kernel(const uint32_t* __restrict__ vals, uint32_t* __restrict__ bsum,
                                                              long P, int nblk) {
  __shared__ uint32_t sm[4];
  const long n = blockIdx.y;
  const long r0 = (long)blockIdx.x * kScanChunk + threadIdx.x * 4;
  uint32_t s = 0;
  if ((P & 3) == 0 && r0 + 3 < P) {  // (P % 4 == 0: 16-byte aligned whatever the image)
    const lv_u32x4 v = *reinterpret_cast<const lv_u32x4*>(vals + n * P + r0);
    s = (v[0] >> 31) + (v[1] >> 31) + (v[2] >> 31) + (v[3] >> 31);
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (r0 + e < P) s += vals[n * P + r0 + e] >> 31;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) bsum[n * nblk + blockIdx.x] = sm[0] + sm[1] + sm[2] + sm[3];
}

// in-place exclusive scan of bsum[n][0..nblk) (one block per image)
__global__ __launch_bounds__(256) void lovasz_scan_blocks_kernel(uint32_t* __restrict__ bsum, int nblk) {
  __shared__ uint32_t sm[4];
  uint32_t* a = bsum + (long)blockIdx.x * nblk;
  const int per = (nblk + 255) / 256;
  const int i0 = threadIdx.x * per;
  uint32_t s = 0;
  for (int k = 0; k < per; ++k)
    if (i0 + k < nblk) s += a[i0 + k];
  uint32_t total;
  uint32_t run = block_exclusive_scan_256(s, sm, &total);
  for (int k = 0; k < per; ++k)
    if (i0 + k < nblk) {
      const uint32_t t = a[i0 + k];
      a[i0 + k] = run;
      run += t;
    }
}

// the four sorted entries of a thread of the apply kernels (ranks r0 .. r0 + 3 of segment n); returns their label count
__device__ __forceinline__ uint32_t lovasz_load4(const uint32_t* __restrict__ keys, const uint32_t* __restrict__ vals, long n, long P,
                                                 long r0, uint32_t (&lab)[4], uint32_t (&key)[4], uint32_t (&idx)[4]) {
  uint32_t s = 0;
  if ((P & 3) == 0 && r0 + 3 < P) {
    const lv_u32x4 v = *reinterpret_cast<const lv_u32x4*>(vals + n * P + r0), k = *reinterpret_cast<const lv_u32x4*>(keys + n * P + r0);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      lab[e] = v[e] >> 31;
      idx[e] = v[e] & 0x7fffffffu;
      key[e] = k[e];
      s += lab[e];
    }
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      lab[e] = 0;
      key[e] = 0;
      idx[e] = 0;
      if (r0 + e < P) {
        const uint32_t v = vals[n * P + r0 + e];
        lab[e] = v >> 31;
        idx[e] = v & 0x7fffffffu;
        key[e] = keys[n * P + r0 + e];
      }
      s += lab[e];
    }
  }
  return s;
}

// gts of the hinge form: one label per pixel, so H*W itself in the plain form; with pixels ignored, the images' valid pixel counts
// (gts_px[n], from lovasz_softmax_scan_blocks_kernel)
template <bool Ignore>
using hinge_gts_t = std::conditional_t<Ignore, const uint32_t* __restrict__, long>;

// Jaccard deltas, loss partials and the gradient scatter
template <bool Ignore>
__global__ __launch_bounds__(256) void lovasz_apply_kernel(const uint32_t* __restrict__ keys, const uint32_t* __restrict__ vals,
                                                           const uint32_t* __restrict__ boff, double* __restrict__ partial,
                                                           float* __restrict__ grad, long P, hinge_gts_t<Ignore> gts_arg, int nblk,
                                                           float inv_n, int xcd_affine) {
  __shared__ uint32_t sm[4];
  __shared__ double red[4];
  // The gradient scatter writes 4-byte values all over ONE image's 4 * P bytes (2 MB at 524 288 keys).  Blocks are dealt
  // round-robin over the 8 XCDs, each with an L2 of its own: with the natural (block, image) order every XCD holds a slice of
  // every cache line of the image.  When the image count divides by 8 and an image's gradient is at most half an L2 (2 MB: the
  // two-class 512^2 tiles of configs[2]), all blocks of an image run on ONE XCD instead (block L of the launch sits on XCD L % 8):
  // its L2 collects the image's lines whole before they leave -- lovasz_apply 217 -> 130 us at bs 32; at 4 MB per image (four
  // classes) the lines evict each other and the natural order is 3 % faster, so the rule stops there (profiles/r05/lovasz.txt).
  long n = blockIdx.y;
  int bx = blockIdx.x;
  if (xcd_affine) {
    const long L = (long)blockIdx.y * gridDim.x + blockIdx.x;
    const int x = (int)(L & 7);
    const long k = L >> 3;
    n = x + 8 * (k / nblk);
    bx = (int)(k % nblk);
  }
  const long r0 = (long)bx * kScanChunk + threadIdx.x * 4;
  uint32_t lab[4], key[4], idx[4];
  const uint32_t s = lovasz_load4(keys, vals, n, P, r0, lab, key, idx);
  uint32_t total;
  uint32_t cs = block_exclusive_scan_256(s, sm, &total) + boff[n * nblk + bx];  // labels strictly before r0
  float gts;
  if constexpr (Ignore) gts = (float)gts_arg[n];
  else gts = (float)gts_arg;
  double acc = 0;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const long r = r0 + e;
    if (r < P) {
      const float cs_prev = (float)cs;
      cs += lab[e];
      const float cs_inc = (float)cs;
      // reference: inter = gts - cumsum(lab); union = gts + cumsum(1 - lab); iou = 1 - inter / union
      const float jac = 1.f - (gts - cs_inc) / (gts + ((float)(r + 1) - cs_inc));
      float delta = jac;
      if (r > 0) {
        const float jac_p = 1.f - (gts - cs_prev) / (gts + ((float)r - cs_prev));
        delta = jac - jac_p;
      }
      const float err = key_to_float(key[e]);
      // (the tail has err = -inf: not above 0, like every valid entry inside its margin -- no loss term, gradient +0.0f)
      const float pos = err > 0.f ? err : 0.f;
      if constexpr (Ignore) {
        if (err > 0.f) acc += (double)(pos * delta);
      } else {
        acc += (double)(pos * delta);
      }
      if (grad) {
        const float g = err > 0.f ? delta : 0.f;
        grad[n * P + idx[e]] = (lab[e] ? -g : g) * inv_n;
      }
    }
  }
  acc = rs_wave_sum(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) partial[n * nblk + bx] = (red[0] + red[1]) + (red[2] + red[3]);
}

// (deterministic: a fixed element -> thread assignment and a fixed tree; 1024 threads with four independent accumulators each --
// round 4's 256 threads with one dependent chain took 41 us for the 16 384 partials of a bs-32 step)
__global__ __launch_bounds__(1024) void lovasz_finalize_kernel(const double* __restrict__ partial, long count, float inv_n,
                                                               float* __restrict__ loss) {
  __shared__ double red[1024];
  double a[4] = {0, 0, 0, 0};
  long i = threadIdx.x;
  for (; i + 3 * 1024 < count; i += 4 * 1024) {
    a[0] += partial[i];
    a[1] += partial[i + 1024];
    a[2] += partial[i + 2 * 1024];
    a[3] += partial[i + 3 * 1024];
  }
  for (; i < count; i += 1024) a[0] += partial[i];
  red[threadIdx.x] = (a[0] + a[1]) + (a[2] + a[3]);
  __syncthreads();
  for (int o = 512; o > 0; o >>= 1) {
    if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) loss[0] = (float)(red[0] * (double)inv_n);
}

__global__ void scale_by_scalar_kernel(const float* __restrict__ src, const float* __restrict__ scalar, float* __restrict__ dst,
                                       long n) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dst[i] = src[i] * scalar[0];
}

// ---- Lovasz-Softmax (Berman et al. 2018, arXiv 1705.08790): the multi-class loss of the paper --------------------------
// p = softmax(x) over the classes.  Segment s = (image n, class c) per image (S = N*C segments of HW keys, position hw) or
// class c over the batch (S = C segments of N*HW keys, position n*HW + hw).  Keys = desc_key(e), e = |1[y=c] - p_c| in fp32
// (in [0, 1]), payload = position | m << 31.  The stable sort puts equal errors in ascending position = ascending (n, h, w).
// Per segment: g = sum m, k_r = labels among ranks 0..r, I_r = g - k_r, U_r = g + r + 1 - k_r,
//     delta_0 = 1 / U_0 ,  delta_r = (I_{r-1} U_r - I_r U_{r-1}) / (U_r U_{r-1})   (exact int64 numerator, one division)
//     L_s = sum_r e_{pi(r)} delta_r   (fp64),   loss = sum_s w_s L_s
// with w_s = [c in P] / (groups * |P|) over the group's classes P (present: g > 0, or all), groups = N per image or 1.
// dL/dp_{c,i} = w_s (m_i ? -delta : +delta) at rank(i), then dL/dx_c = p_c (G_c - sum_k p_k G_k) per pixel.

template <int VEC>
__device__ __forceinline__ void lvs_load(const float* xp, float* v) {
  if constexpr (VEC == 4) {
    const f32x4 t = *reinterpret_cast<const f32x4*>(xp);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = t[e];
  } else {
    v[0] = xp[0];
  }
}

template <int VEC>
__device__ __forceinline__ void lvs_write(float* p, const float* v) {
  if constexpr (VEC == 4) *reinterpret_cast<f32x4*>(p) = f32x4{v[0], v[1], v[2], v[3]};
  else p[0] = v[0];
}

// max and 1 / (sum of exp) over the C logits of VEC consecutive pixels (xp: class 0 of the first); the softmax is lvs_prob
template <int VEC>
__device__ __forceinline__ void lvs_softmax_stats(const float* xp, long HW, int C, float* mx, float* sum /* -> 1 / sum */) {
  float v[VEC];
  lvs_load<VEC>(xp, mx);
  for (int c = 1; c < C; ++c) {
    lvs_load<VEC>(xp + c * HW, v);
#pragma unroll
    for (int e = 0; e < VEC; ++e) mx[e] = fmaxf(mx[e], v[e]);
  }
#pragma unroll
  for (int e = 0; e < VEC; ++e) sum[e] = 0.f;
  for (int c = 0; c < C; ++c) {
    lvs_load<VEC>(xp + c * HW, v);
#pragma unroll
    for (int e = 0; e < VEC; ++e) sum[e] += expf(v[e] - mx[e]);
  }
#pragma unroll
  for (int e = 0; e < VEC; ++e) sum[e] = 1.f / sum[e];  // (one division per pixel, not per class)
}

// (the keys and the Jacobian kernels both take p from here: the same fp32 value in both)
__device__ __forceinline__ float lvs_prob(float x, float mx, float inv_sum) { return expf(x - mx) * inv_sum; }

// offset of (class c, pixel q = n*HW + hw) in the segment-major key arrays; the position inside the segment is hw or q
__device__ __forceinline__ long lvs_seg_off(long q, long n, long hw, int c, int C, long NHW, long HW, int per_image) {
  return per_image ? ((n * C + c) * HW + hw) : ((long)c * NHW + q);
}

constexpr float kIgnoredSoftmaxErr = -1.f;  // the error of an ignored pixel's entries: behind every valid one, which lie in [0, 1]

// one thread per VEC consecutive pixels of one image (VEC = 4 needs HW % 4 == 0): C keys + C payloads each (probs: NCHW p)
template <int VEC, bool Ignore, typename... Extra>
__global__ __launch_bounds__(256) void lovasz_softmax_keys_kernel(const float* __restrict__ x, const long long* __restrict__ tgt,
                                                                  uint32_t* __restrict__ keys, uint32_t* __restrict__ vals,
                                                                  float* __restrict__ probs, long NHW, long HW, int C, int per_image,
                                                                  Extra... extra) {
  // the key must be fp32(1 - p) of the very p this kernel writes out: no fusing of 1 - e * inv_sum into one fma
#pragma clang fp contract(off)
  const long q = ((long)blockIdx.x * blockDim.x + threadIdx.x) * VEC;
  if (q >= NHW) return;
  const long n = q / HW, hw = q - n * HW;
  const float* xp = x + n * C * HW + hw;
  float mx[VEC], sum[VEC], v[VEC], pr[VEC];
  lvs_softmax_stats<VEC>(xp, HW, C, mx, sum);
  long long t[VEC];
  if constexpr (VEC == 4) {
    const lv_i64x2 t0 = *reinterpret_cast<const lv_i64x2*>(tgt + q), t1 = *reinterpret_cast<const lv_i64x2*>(tgt + q + 2);
    t[0] = t0[0]; t[1] = t0[1]; t[2] = t1[0]; t[3] = t1[1];
  } else {
    t[0] = tgt[q];
  }
  const uint32_t pos = (uint32_t)(per_image ? hw : q);
  for (int c = 0; c < C; ++c) {
    lvs_load<VEC>(xp + c * HW, v);
    uint32_t k[VEC], w[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      pr[e] = lvs_prob(v[e], mx[e], sum[e]);
      const uint32_t m = (t[e] == c) ? 1u : 0u;
      if constexpr (Ignore) k[e] = desc_key(t[e] == (extra, ...) ? kIgnoredSoftmaxErr : m ? 1.f - pr[e] : pr[e]);
      else k[e] = desc_key(m ? 1.f - pr[e] : pr[e]);
      w[e] = (pos + (uint32_t)e) | (m << 31);
    }
    const long o = lvs_seg_off(q, n, hw, c, C, NHW, HW, per_image);
    if constexpr (VEC == 4) {
      *reinterpret_cast<lv_u32x4*>(keys + o) = lv_u32x4{k[0], k[1], k[2], k[3]};
      *reinterpret_cast<lv_u32x4*>(vals + o) = lv_u32x4{w[0], w[1], w[2], w[3]};
    } else {
      keys[o] = k[0];
      vals[o] = w[0];
    }
    if (probs) lvs_write<VEC>(probs + (n * C + c) * HW + hw, pr);
  }
}

// lovasz_scan_blocks_kernel that also keeps each segment's total: gts[s] = g (foreground count of the segment)
__global__ __launch_bounds__(256) void lovasz_softmax_scan_blocks_kernel(uint32_t* __restrict__ bsum, uint32_t* __restrict__ gts,
                                                                         int nblk) {
  __shared__ uint32_t sm[4];
  uint32_t* a = bsum + (long)blockIdx.x * nblk;
  const int per = (nblk + 255) / 256;
  const int i0 = threadIdx.x * per;
  uint32_t s = 0;
  for (int k = 0; k < per; ++k)
    if (i0 + k < nblk) s += a[i0 + k];
  uint32_t total;
  uint32_t run = block_exclusive_scan_256(s, sm, &total);
  for (int k = 0; k < per; ++k)
    if (i0 + k < nblk) {
      const uint32_t t = a[i0 + k];
      a[i0 + k] = run;
      run += t;
    }
  if (threadIdx.x == 0) gts[blockIdx.x] = total;
}

// w[group * C + c] = [c in P] / (groups * |P|): one thread per group (an image, or the whole batch)
__global__ __launch_bounds__(256) void lovasz_softmax_weights_kernel(const uint32_t* __restrict__ gts, double* __restrict__ w,
                                                                     int groups, int C, int all_classes) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= groups) return;
  int cnt = 0;
  for (int c = 0; c < C; ++c) cnt += (all_classes || gts[(long)n * C + c] > 0) ? 1 : 0;
  // (cnt >= 1 whenever the group has a pixel: every pixel's class is present)
  const double inv = cnt > 0 ? 1.0 / ((double)groups * (double)cnt) : 0.0;
  for (int c = 0; c < C; ++c) w[(long)n * C + c] = (all_classes || gts[(long)n * C + c] > 0) ? inv : 0.0;
}

// closed-form deltas, weighted fp64 loss partials and the scatter of the weighted dL/dp (segment-major, like the keys); Ignore: a
// tail entry (negative error) adds nothing and gets dL/dp = +0.0f, whatever its delta
template <bool Ignore>
__global__ __launch_bounds__(256) void lovasz_softmax_apply_kernel(const uint32_t* __restrict__ keys, const uint32_t* __restrict__ vals,
                                                                   const uint32_t* __restrict__ boff, const uint32_t* __restrict__ gts,
                                                                   const double* __restrict__ w, double* __restrict__ partial,
                                                                   float* __restrict__ gp, long P, int nblk, int xcd_affine) {
  __shared__ uint32_t sm[4];
  __shared__ double red[4];
  long n = blockIdx.y;  // the segment
  int bx = blockIdx.x;
  if (xcd_affine) {  // all blocks of a segment on one XCD, as in lovasz_apply_kernel (segment count % 8 == 0)
    const long L = (long)blockIdx.y * gridDim.x + blockIdx.x;
    const long k = L >> 3;
    n = (L & 7) + 8 * (k / nblk);
    bx = (int)(k % nblk);
  }
  const long r0 = (long)bx * kScanChunk + threadIdx.x * 4;
  uint32_t lab[4], key[4], idx[4];
  const uint32_t s = lovasz_load4(keys, vals, n, P, r0, lab, key, idx);
  uint32_t total;
  long long k = block_exclusive_scan_256(s, sm, &total) + boff[n * nblk + bx];  // labels strictly before r0
  const long long g = gts[n];
  const double ws = w[n];
  double acc = 0;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const long long r = r0 + e;
    if (r < P) {
      const long long Ip = g - k, Up = g + r - k;  // I_{r-1}, U_{r-1}
      k += lab[e];
      const long long I = g - k, U = g + r + 1 - k;
      // U_r >= 1 always (U_r - I_r = r + 1); at r = 0, U_{-1} = g may be 0 and delta_0 = J_0 = 1 / U_0
      const double delta = r == 0 ? 1.0 / (double)U : (double)(Ip * U - I * Up) / (double)(U * Up);
      if constexpr (Ignore) {
        const float err = key_to_float(key[e]);
        const bool tail = err < 0.f;
        if (!tail) acc += (double)err * delta;
        if (gp) gp[n * P + idx[e]] = tail ? 0.f : (float)(ws * (lab[e] ? -delta : delta));
      } else {
        acc += (double)key_to_float(key[e]) * delta;
        if (gp) gp[n * P + idx[e]] = (float)(ws * (lab[e] ? -delta : delta));
      }
    }
  }
  acc = rs_wave_sum(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) partial[n * nblk + bx] = ws * ((red[0] + red[1]) + (red[2] + red[3]));
}

// per VEC pixels: grad[n, c] = p_c (G_c - sum_k p_k G_k) with G the weighted dL/dp (segment-major), in fp64; Ignore (which
// reads the labels for it: IgnoredLabels): +0.0f in every class plane of an ignored pixel
template <int VEC, bool Ignore, typename... Extra>
__global__ __launch_bounds__(256) void lovasz_softmax_jacobian_kernel(const float* __restrict__ x, const float* __restrict__ gp,
                                                                      float* __restrict__ grad, long NHW, long HW, int C, int per_image,
                                                                      Extra... extra) {
  const long q = ((long)blockIdx.x * blockDim.x + threadIdx.x) * VEC;
  if (q >= NHW) return;
  const long n = q / HW, hw = q - n * HW;
  const float* xp = x + n * C * HW + hw;
  float mx[VEC], sum[VEC], v[VEC], gv[VEC], out[VEC];
  [[maybe_unused]] bool skip[VEC];
  if constexpr (Ignore) {
#pragma unroll
    for (int e = 0; e < VEC; ++e) skip[e] = (extra, ...).tgt[q + e] == (extra, ...).ignore;
  }
  lvs_softmax_stats<VEC>(xp, HW, C, mx, sum);
  double dot[VEC];
#pragma unroll
  for (int e = 0; e < VEC; ++e) dot[e] = 0.0;
  for (int c = 0; c < C; ++c) {
    lvs_load<VEC>(xp + c * HW, v);
    lvs_load<VEC>(gp + lvs_seg_off(q, n, hw, c, C, NHW, HW, per_image), gv);
#pragma unroll
    for (int e = 0; e < VEC; ++e) dot[e] += (double)lvs_prob(v[e], mx[e], sum[e]) * (double)gv[e];
  }
  for (int c = 0; c < C; ++c) {
    lvs_load<VEC>(xp + c * HW, v);
    lvs_load<VEC>(gp + lvs_seg_off(q, n, hw, c, C, NHW, HW, per_image), gv);
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      if constexpr (Ignore) out[e] = skip[e] ? 0.f : (float)((double)lvs_prob(v[e], mx[e], sum[e]) * ((double)gv[e] - dot[e]));
      else out[e] = (float)((double)lvs_prob(v[e], mx[e], sum[e]) * ((double)gv[e] - dot[e]));
    }
    lvs_write<VEC>(grad + (n * C + c) * HW + hw, out);
  }
}

struct Carve {
  long P;
  int nblk_sort, nblk_scan;
  size_t keys0, vals0, keys1, vals1, counts, bsum, partial, total;
};

// S segments of P keys each, sorted and scanned independently (blockIdx.y = segment in every kernel above)
Carve carve_segments(long S, long P) {
  Carve c;
  c.P = P;
  c.nblk_sort = rs_cdiv(c.P, sort_chunk(S * c.P));
  c.nblk_scan = rs_cdiv(c.P, kScanChunk);
  const size_t arr = ((size_t)S * c.P * sizeof(uint32_t) + 255) & ~(size_t)255;
  size_t o = 0;
  c.keys0 = o; o += arr;
  c.vals0 = o; o += arr;
  c.keys1 = o; o += arr;
  c.vals1 = o; o += arr;
  c.counts = o; o += (((size_t)S * c.nblk_sort * 256 * sizeof(uint32_t)) + 255) & ~(size_t)255;
  c.bsum = o; o += (((size_t)S * c.nblk_scan * sizeof(uint32_t)) + 255) & ~(size_t)255;
  c.partial = o; o += (((size_t)S * c.nblk_scan * sizeof(double)) + 255) & ~(size_t)255;
  c.total = o;
  return c;
}

Carve carve(int N, int C, int H, int W) { return carve_segments(N, (long)C * H * W); }

// Stable LSD radix sort of S segments of cv.P keys each: (k0, v0) -> 4 passes x 8 bits through (k1, v1) -> sorted in (k0, v0).
// sc_affine: the scatter keeps a segment's tiles on one XCD (needs S % 8 == 0).  csum (nullable): scratch of
// S * cdiv(nblk_sort, kScanTiles) * 256 words for the chunked digit scan of few long segments; null = one block per segment.
void radix_sort_segments(uint32_t* k0, uint32_t* v0, uint32_t* k1, uint32_t* v1, uint32_t* counts, long S, const Carve& cv,
                         int sc_affine, hipStream_t s, uint32_t* csum = nullptr) {
  const int nchunk = rs_cdiv(cv.nblk_sort, kScanTiles);
  const long P = cv.P;
  const bool small_chunk = sort_chunk(S * P) == 4096;
  for (int pass = 0; pass < 4; ++pass) {
    const uint32_t* ik = (pass & 1) ? k1 : k0;
    const uint32_t* iv = (pass & 1) ? v1 : v0;
    uint32_t* ok = (pass & 1) ? k0 : k1;
    uint32_t* ov = (pass & 1) ? v0 : v1;
    if (small_chunk) radix_hist_kernel<4096><<<dim3(cv.nblk_sort, S), 256, 0, s>>>(ik, counts, P, cv.nblk_sort, pass * 8);
    else radix_hist_kernel<8192><<<dim3(cv.nblk_sort, S), 256, 0, s>>>(ik, counts, P, cv.nblk_sort, pass * 8);
    if (csum) {
      radix_chunk_sum_kernel<<<dim3(nchunk, S), 256, 0, s>>>(counts, csum, cv.nblk_sort, nchunk);
      radix_scan_kernel<<<S, 1024, 0, s>>>(csum, nchunk);
      radix_chunk_offsets_kernel<<<dim3(nchunk, S), 256, 0, s>>>(counts, csum, cv.nblk_sort, nchunk);
    } else {
      radix_scan_kernel<<<S, 1024, 0, s>>>(counts, cv.nblk_sort);
    }
    if (small_chunk) radix_scatter_kernel<4096><<<dim3(cv.nblk_sort, S), 256, 0, s>>>(ik, iv, ok, ov, counts, P, cv.nblk_sort, pass * 8, sc_affine);
    else radix_scatter_kernel<8192><<<dim3(cv.nblk_sort, S), 256, 0, s>>>(ik, iv, ok, ov, counts, P, cv.nblk_sort, pass * 8, sc_affine);
  }
}

// the workspace as typed pointers
struct SortBuffers {
  uint32_t *k0, *v0, *k1, *v1, *counts, *bsum;
  double* partial;
};

SortBuffers sort_buffers(void* workspace, const Carve& cv) {
  char* ws = reinterpret_cast<char*>(workspace);
  auto u32 = [ws](size_t offset) { return reinterpret_cast<uint32_t*>(ws + offset); };
  return {u32(cv.keys0), u32(cv.vals0), u32(cv.keys1), u32(cv.vals1), u32(cv.counts), u32(cv.bsum), reinterpret_cast<double*>(ws + cv.partial)};
}

bool lovasz_shape_ok(int N, int C, int H, int W) { return N > 0 && C > 0 && H > 0 && W > 0 && (long)C * H * W < (1L << 31); }

bool lovasz_ignore_ok(int ignore, int C) { return ignore >= C && ignore <= 255; }

// rs_lovasz_fwd (no `ignore`) and rs_lovasz_fwd_ig (`ignore` = the label)
template <bool Ignore, typename... Extra>
int lovasz_fwd(const float* logits, const long long* targets, float* loss, float* grad_unit, int N, int C, int H, int W, void* workspace,
               rs_stream_t stream, Extra... ignore) {
  const Carve cv = carve(N, C, H, W);
  const SortBuffers b = sort_buffers(workspace, cv);
  hipStream_t s = (hipStream_t)stream;
  const long P = cv.P, HW = (long)H * W;
  // the sort's scatter passes keep an image's tiles on one XCD too (its digit runs of 64-128 bytes then meet their neighbours'
  // in one L2): -5 % on a bs-32 sort, -3.5 % with four classes, +3 % at 8 images (one image per XCD: no slack) -> from 16 images
  const int sc_affine = (N % 8 == 0 && N >= 16 && rs_knobs().lovasz_xcd != 0) ? 1 : 0;

  if ((HW & 3) == 0) lovasz_keys4_kernel<Ignore><<<dim3(rs_cdiv(P / 4, 256), N), 256, 0, s>>>(logits, targets, b.k0, b.v0, P, HW, ignore...);
  else lovasz_keys_kernel<Ignore><<<dim3(rs_cdiv(P, 256), N), 256, 0, s>>>(logits, targets, b.k0, b.v0, P, HW, ignore...);
  radix_sort_segments(b.k0, b.v0, b.k1, b.v1, b.counts, N, cv, sc_affine, s);
  // after 4 passes the sorted data is back in (k0, v0)
  lovasz_blocksum_kernel<<<dim3(cv.nblk_scan, N), 256, 0, s>>>(b.v0, b.bsum, P, cv.nblk_scan);
  const float inv_n = 1.f / (float)N;
  const int xcd_affine = (N % 8 == 0 && P * 4 <= (2L << 20) && rs_knobs().lovasz_xcd != 0) ? 1 : 0;
  if constexpr (Ignore) {
    // the sort is done with its digit counts (at least 256 words per image): their first N words take the images' valid pixel
    // counts, so the workspace is rs_lovasz_workspace_bytes' as it stands
    uint32_t* gts_px = b.counts;
    lovasz_softmax_scan_blocks_kernel<<<N, 256, 0, s>>>(b.bsum, gts_px, cv.nblk_scan);
    lovasz_apply_kernel<true><<<dim3(cv.nblk_scan, N), 256, 0, s>>>(b.k0, b.v0, b.bsum, b.partial, grad_unit, P, gts_px, cv.nblk_scan, inv_n, xcd_affine);
  } else {
    lovasz_scan_blocks_kernel<<<N, 256, 0, s>>>(b.bsum, cv.nblk_scan);
    lovasz_apply_kernel<false><<<dim3(cv.nblk_scan, N), 256, 0, s>>>(b.k0, b.v0, b.bsum, b.partial, grad_unit, P, HW, cv.nblk_scan, inv_n, xcd_affine);
  }
  lovasz_finalize_kernel<<<1, 1024, 0, s>>>(b.partial, (long)N * cv.nblk_scan, inv_n, loss);
  return RS_LAUNCH_RESULT();
}

// the Lovasz-Softmax workspace: the sort / scan carve of its S segments, then g (uint32) and w (fp64) per segment
struct SoftmaxCarve {
  long S;
  Carve cv;
  size_t gts, w, csum, total;
  bool chunked_scan;
};

bool lovasz_softmax_shape_ok(int N, int C, int H, int W, int per_image) {
  if (N <= 0 || C < 2 || H <= 0 || W <= 0 || (long)N * C * H * W >= (1L << 31)) return false;
  return (per_image ? (long)N * C : (long)C) <= 65535;  // (segments = blockIdx.y of the sort kernels)
}

SoftmaxCarve carve_softmax(int N, int C, int H, int W, int per_image) {
  SoftmaxCarve c;
  const long HW = (long)H * W;
  c.S = per_image ? (long)N * C : (long)C;
  c.cv = carve_segments(c.S, per_image ? HW : (long)N * HW);
  size_t o = c.cv.total;
  c.gts = o; o += ((size_t)c.S * sizeof(uint32_t) + 255) & ~(size_t)255;
  c.w = o; o += ((size_t)c.S * sizeof(double) + 255) & ~(size_t)255;
  // more than 256 sort tiles per segment (each of radix_scan_kernel's four thread groups would walk over 64): chunked scan
  c.chunked_scan = c.cv.nblk_sort > 4 * kScanTiles;
  c.csum = o;
  if (c.chunked_scan) o += ((size_t)c.S * rs_cdiv(c.cv.nblk_sort, kScanTiles) * 256 * sizeof(uint32_t) + 255) & ~(size_t)255;
  c.total = o;
  return c;
}

// rs_lovasz_softmax_fwd (no `ignore`) and rs_lovasz_softmax_fwd_ig (`ignore` = the label)
template <bool Ignore, typename... Extra>
int lovasz_softmax_fwd(const float* logits, const long long* targets, float* loss, float* grad_unit, float* probs_out, int N, int C, int H,
                       int W, int per_image, int all_classes, void* workspace, rs_stream_t stream, Extra... ignore) {
  const SoftmaxCarve sc = carve_softmax(N, C, H, W, per_image);
  const Carve& cv = sc.cv;
  const SortBuffers b = sort_buffers(workspace, cv);
  char* ws = reinterpret_cast<char*>(workspace);
  uint32_t* gts = reinterpret_cast<uint32_t*>(ws + sc.gts);
  double* w = reinterpret_cast<double*>(ws + sc.w);
  hipStream_t s = (hipStream_t)stream;
  const long S = sc.S, HW = (long)H * W, NHW = (long)N * HW;
  const int pi = per_image ? 1 : 0;
  const int sc_affine = (S % 8 == 0 && S >= 16 && rs_knobs().lovasz_xcd != 0) ? 1 : 0;  // (the rule of lovasz_fwd, per segment)

  if ((HW & 3) == 0)
    lovasz_softmax_keys_kernel<4, Ignore><<<rs_cdiv(NHW / 4, 256), 256, 0, s>>>(logits, targets, b.k0, b.v0, probs_out, NHW, HW, C, pi, ignore...);
  else lovasz_softmax_keys_kernel<1, Ignore><<<rs_cdiv(NHW, 256), 256, 0, s>>>(logits, targets, b.k0, b.v0, probs_out, NHW, HW, C, pi, ignore...);
  radix_sort_segments(b.k0, b.v0, b.k1, b.v1, b.counts, S, cv, sc_affine, s, sc.chunked_scan ? reinterpret_cast<uint32_t*>(ws + sc.csum) : nullptr);
  lovasz_blocksum_kernel<<<dim3(cv.nblk_scan, S), 256, 0, s>>>(b.v0, b.bsum, cv.P, cv.nblk_scan);
  lovasz_softmax_scan_blocks_kernel<<<S, 256, 0, s>>>(b.bsum, gts, cv.nblk_scan);  // (g of a segment: its valid pixels of the class)
  const int groups = per_image ? N : 1;
  lovasz_softmax_weights_kernel<<<rs_cdiv(groups, 256), 256, 0, s>>>(gts, w, groups, C, all_classes ? 1 : 0);
  // the sort is done with (k1, v1): k1 holds the weighted dL/dp, segment-major
  float* gp = grad_unit ? reinterpret_cast<float*>(b.k1) : nullptr;
  const int xcd_affine = (S % 8 == 0 && cv.P * 4 <= (2L << 20) && rs_knobs().lovasz_xcd != 0) ? 1 : 0;  // (lovasz_fwd's rule)
  lovasz_softmax_apply_kernel<Ignore><<<dim3(cv.nblk_scan, S), 256, 0, s>>>(b.k0, b.v0, b.bsum, gts, w, b.partial, gp, cv.P, cv.nblk_scan, xcd_affine);
  if (grad_unit) {
    auto jacobian = [&](auto... extra) {
      if ((HW & 3) == 0)
        lovasz_softmax_jacobian_kernel<4, Ignore><<<rs_cdiv(NHW / 4, 256), 256, 0, s>>>(logits, gp, grad_unit, NHW, HW, C, pi, extra...);
      else lovasz_softmax_jacobian_kernel<1, Ignore><<<rs_cdiv(NHW, 256), 256, 0, s>>>(logits, gp, grad_unit, NHW, HW, C, pi, extra...);
    };
    if constexpr (Ignore) jacobian(IgnoredLabels{targets, ignore...});  // (it reads the labels to write exact zeros)
    else jacobian();
  }
  lovasz_finalize_kernel<<<1, 1024, 0, s>>>(b.partial, S * cv.nblk_scan, 1.f, loss);
  return RS_LAUNCH_RESULT();
}

}  // namespace

extern "C" long rs_lovasz_workspace_bytes(int N, int C, int H, int W) {
  if (!lovasz_shape_ok(N, C, H, W)) return RS_EINVAL;
  return (long)carve(N, C, H, W).total;
}

extern "C" int rs_lovasz_fwd(const float* logits, const long long* targets, float* loss, float* grad_unit, int N, int C,
                             int H, int W, void* workspace, rs_stream_t stream) {
  if (!logits || !targets || !loss || !workspace || !lovasz_shape_ok(N, C, H, W)) return RS_EINVAL;
  return lovasz_fwd<false>(logits, targets, loss, grad_unit, N, C, H, W, workspace, stream);
}

extern "C" int rs_lovasz_fwd_ig(const float* logits, const long long* targets, float* loss, float* grad_unit, int N, int C,
                                int H, int W, void* workspace, rs_stream_t stream, int ignore) {
  if (!logits || !targets || !loss || !workspace || !lovasz_shape_ok(N, C, H, W) || !lovasz_ignore_ok(ignore, C)) return RS_EINVAL;
  return lovasz_fwd<true>(logits, targets, loss, grad_unit, N, C, H, W, workspace, stream, ignore);
}

extern "C" int rs_scale_by_scalar(const float* src, const float* scalar, float* dst, long n, rs_stream_t stream) {
  if (!src || !scalar || !dst || n <= 0) return RS_EINVAL;
  scale_by_scalar_kernel<<<rs_cdiv(n, 256), 256, 0, (hipStream_t)stream>>>(src, scalar, dst, n);
  return RS_LAUNCH_RESULT();
}

extern "C" long rs_lovasz_softmax_workspace_bytes(int N, int C, int H, int W, int per_image) {
  if (!lovasz_softmax_shape_ok(N, C, H, W, per_image)) return RS_EINVAL;
  return (long)carve_softmax(N, C, H, W, per_image).total;
}

extern "C" int rs_lovasz_softmax_fwd(const float* logits, const long long* targets, float* loss, float* grad_unit, float* probs_out,
                                     int N, int C, int H, int W, int per_image, int all_classes, void* workspace, rs_stream_t stream) {
  if (!logits || !targets || !loss || !workspace || !lovasz_softmax_shape_ok(N, C, H, W, per_image)) return RS_EINVAL;
  return lovasz_softmax_fwd<false>(logits, targets, loss, grad_unit, probs_out, N, C, H, W, per_image, all_classes, workspace, stream);
}

extern "C" int rs_lovasz_softmax_fwd_ig(const float* logits, const long long* targets, float* loss, float* grad_unit, float* probs_out,
                                        int N, int C, int H, int W, int per_image, int all_classes, void* workspace, rs_stream_t stream,
                                        int ignore) {
  if (!logits || !targets || !loss || !workspace || !lovasz_softmax_shape_ok(N, C, H, W, per_image) || !lovasz_ignore_ok(ignore, C))
    return RS_EINVAL;
  return lovasz_softmax_fwd<true>(logits, targets, loss, grad_unit, probs_out, N, C, H, W, per_image, all_classes, workspace, stream, ignore);
}
