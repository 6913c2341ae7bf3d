// `rs features` on the device: the raster half of robosat/tools/features.py + robosat/features/core.py (class select, morphological
// open / close with a disc, 4-connected components, boundary edges).  Integer work, LDS / HBM bound.  Definitions: include/robosat_hip.h.
//
//   rs_features_clean       mask bytes -> bit-planes (one __ballot packs a wave's 64 pixels) -> erode, dilate, dilate, erode -> 0/1 bytes.
//                           A disc is a stack of horizontal runs: a pass ANDs (ORs) funnel-shifted words of the eps rows around a word.
//                           LDS form: one block per tile, both planes resident, no HBM between the passes.  HBM form: one launch per pass
//                           (the default: a batch of 16 tiles fills 16 CUs in the LDS form and all of them in this one).
//                           Both run the same morph_word() on the same bits.
//   rs_features_label       union-find over the pixel grid with atomicMin (lock-free; every loop counted against H*W), then flatten:
//                           the root of a component is its smallest y*W+x, so label = root + 1 is canonical.
//   rs_features_components  roots -> slots, area / bounding box per slot by integer atomics, min_area filter, compaction.
//   rs_features_edges       directed unit boundary edges of the kept components, compacted by one atomic per wave.
//   rs_features_overlaps    two label rasters -> (raster, label_a, label_b, shared pixels) through a hash table in global memory,
//                           equal pairs merged per thread, per wave and per block first (`rs features --dedupe`).
//   rs_features_scores      label raster + K planes of probability bytes -> the exact sum of every model's bytes per listed component:
//                           a segmented scan per wave, the block's waves merged in LDS, one 64-bit atomic per run (`rs features --score`).
// Stitched form (all tiles of a zoom level as one sparse raster; tables nbr [T][8] and origin [T][2] from the host):
//   rs_features_halo            tile + apron of A pixels from its 8 neighbours (A = reach of open + close), and the crop back.
//   rs_features_stitch_labels   per-tile canonical labels -> global index space, unions across right / down seams, flatten.
//   rs_features_components_stitched / rs_features_edges_stitched   the table and edge kernels with STITCH = true.
#include "common.h"

namespace {

constexpr int kMaxEps = 64;                  // a run reaches at most 32 bits to either side: one neighbouring word
constexpr int kLdsBytes = 160 * 1024;        // gfx950 LDS per workgroup
constexpr int kCleanThreads = 1024;

struct Disc {
  int eps;
  signed char lo[kMaxEps], hi[kMaxEps];  // row i (dy = i - eps/2): offsets lo..hi set
};

struct CleanArgs {
  const uint8_t* images;
  uint8_t* out;
  uint32_t* ws;  // HBM form: [B][2][H][Wd]
  int B, H, W, Wd, index;
  Disc open, close;
};

// One output word of erode (ERODE: AND over s of m[p + s], outside = 1) or dilate (OR over s of m[p - s], outside = 0).
// `src`: plane [H][Wd] whose bits beyond W are 0.
template <bool ERODE>
__device__ __forceinline__ uint32_t morph_word(const uint32_t* src, const Disc& d, int y, int wx, int H, int W, int Wd) {
  const uint32_t pad = ERODE ? 0xffffffffu : 0u;
  const int r = d.eps >> 1;
  const int tail = W & 31;
  const uint32_t valid_last = tail ? ((1u << tail) - 1u) : 0xffffffffu;
  uint32_t acc = pad;
  for (int i = 0; i < d.eps; ++i) {
    const int yy = ERODE ? y + (i - r) : y - (i - r);
    const int lo = ERODE ? d.lo[i] : -d.hi[i], hi = ERODE ? d.hi[i] : -d.lo[i];
    uint32_t prev = pad, cur = pad, next = pad;
    if (yy >= 0 && yy < H) {
      const uint32_t* row = src + (long)yy * Wd;
      cur = row[wx];
      if (ERODE && wx == Wd - 1) cur |= ~valid_last;
      if (wx > 0) prev = row[wx - 1];
      if (wx + 1 < Wd) {
        next = row[wx + 1];
        if (ERODE && wx + 1 == Wd - 1) next |= ~valid_last;
      }
    }
    for (int o = lo; o <= hi; ++o) {
      // bits x + o, x = 0..31
      uint32_t v;
      if (o == 0)
        v = cur;
      else if (o > 0)
        v = o == 32 ? next : __funnelshift_r(cur, next, o);
      else
        v = o == -32 ? prev : __funnelshift_r(prev, cur, 32 + o);
      acc = ERODE ? (acc & v) : (acc | v);
    }
  }
  if (wx == Wd - 1) acc &= valid_last;
  return acc;
}

// mask = (image == index) packed 32 pixels per word, bits beyond W zero.  Wave-uniform loop: every lane reaches the ballot.
__device__ __forceinline__ void select_pack(const uint8_t* img, uint32_t* plane, int H, int W, int Wd, int index, int wave, int nwaves,
                                            int lane) {
  const int chunks = (W + 63) >> 6;
  for (int item = wave; item < H * chunks; item += nwaves) {
    const int y = item / chunks, ch = item - y * chunks;
    const int x = ch * 64 + lane;
    const bool fg = x < W && img[(long)y * W + x] == (uint8_t)index;
    const unsigned long long m = __ballot(fg);
    if (lane == 0) plane[(long)y * Wd + ch * 2] = (uint32_t)m;
    if (lane == 32 && ch * 2 + 1 < Wd) plane[(long)y * Wd + ch * 2 + 1] = (uint32_t)(m >> 32);
  }
}

__global__ __launch_bounds__(kCleanThreads) void clean_lds_kernel(const CleanArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint32_t planes[];
  const int H = a.H, W = a.W, Wd = a.Wd, words = H * Wd;
  uint32_t* p0 = planes;
  uint32_t* p1 = planes + words;
  const long HW = (long)H * W;
  const uint8_t* img = a.images + (long)blockIdx.x * HW;
  select_pack(img, p0, H, W, Wd, a.index, threadIdx.x >> 6, kCleanThreads >> 6, threadIdx.x & 63);
  rs_lds_writes_done();
  __syncthreads();
  uint32_t* src = p0;
  uint32_t* dst = p1;
  for (int pass = 0; pass < 4; ++pass) {  // erode, dilate (open), dilate, erode (close)
    const Disc& d = pass < 2 ? a.open : a.close;
    if (d.eps <= 1) continue;  // (uniform)
    const bool erode = pass == 0 || pass == 3;
    for (int i = threadIdx.x; i < words; i += kCleanThreads) {
      const int y = i / Wd, wx = i - y * Wd;
      dst[i] = erode ? morph_word<true>(src, d, y, wx, H, W, Wd) : morph_word<false>(src, d, y, wx, H, W, Wd);
    }
    rs_lds_writes_done();
    __syncthreads();
    uint32_t* t = src;
    src = dst;
    dst = t;
  }
  uint8_t* out = a.out + (long)blockIdx.x * HW;
  for (long p = threadIdx.x; p < HW; p += kCleanThreads) {
    const int y = (int)(p / W), x = (int)(p - (long)y * W);
    out[p] = (uint8_t)((src[y * Wd + (x >> 5)] >> (x & 31)) & 1u);
  }
}

// HBM form: planes in global memory, one launch per stage.
__global__ __launch_bounds__(256) void clean_select_kernel(const CleanArgs a) {
  const int tile = blockIdx.y;
  const long words = (long)a.H * a.Wd;
  select_pack(a.images + (long)tile * a.H * a.W, a.ws + (long)tile * 2 * words, a.H, a.W, a.Wd, a.index,
              blockIdx.x * 4 + (threadIdx.x >> 6), gridDim.x * 4, threadIdx.x & 63);
}

template <bool ERODE>
__global__ __launch_bounds__(256) void clean_pass_kernel(const CleanArgs a, const Disc d, int from) {
  const int tile = blockIdx.y;
  const long words = (long)a.H * a.Wd;
  const uint32_t* src = a.ws + ((long)tile * 2 + from) * words;
  uint32_t* dst = a.ws + ((long)tile * 2 + (from ^ 1)) * words;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= words) return;
  const int y = (int)(i / a.Wd), wx = (int)(i - (long)y * a.Wd);
  dst[i] = morph_word<ERODE>(src, d, y, wx, a.H, a.W, a.Wd);
}

__global__ __launch_bounds__(256) void clean_unpack_kernel(const CleanArgs a, int from) {
  const int tile = blockIdx.y;
  const long HW = (long)a.H * a.W;
  const uint32_t* src = a.ws + ((long)tile * 2 + from) * (long)a.H * a.Wd;
  const long p = (long)blockIdx.x * 256 + threadIdx.x;
  if (p >= HW) return;
  const int y = (int)(p / a.W), x = (int)(p - (long)y * a.W);
  a.out[tile * HW + p] = (uint8_t)((src[(long)y * a.Wd + (x >> 5)] >> (x & 31)) & 1u);
}

bool make_disc(int eps, const int32_t* dx, Disc* d) {
  d->eps = eps;
  if (eps < 0 || eps > kMaxEps) return false;
  if (eps > 1 && !dx) return false;
  const int c = eps / 2;
  for (int i = 0; i < eps && eps > 1; ++i) {
    if (dx[i] < 0 || dx[i] > c) return false;
    const int lo = dx[i] < c ? dx[i] : c, hi = dx[i] < eps - 1 - c ? dx[i] : eps - 1 - c;
    d->lo[i] = (signed char)-lo;
    d->hi[i] = (signed char)hi;
  }
  return true;
}

// ---- labelling -------------------------------------------------------------------------------------------------------
// parent[p] = 1 + index of a pixel of the same component with a smaller or equal index (background 0); a root has parent[p] == p + 1.
// Links only ever decrease, so a chain from p has at most p + 1 <= H*W steps: that is the bound of every loop below.  A loop that runs
// out of its bound raises *err (the host turns it into an exception) instead of going on.

__device__ __forceinline__ int uf_find(int* L, int p, int bound, int* err) {
  int cur = p;
  for (int it = 0; it <= bound; ++it) {
    const int par = __hip_atomic_load(&L[cur], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - 1;
    if (par == cur) {
      if (cur != p) atomicMin(&L[p], cur + 1);  // compression: the root is an ancestor, and smaller
      return cur;
    }
    cur = par;
  }
  atomicOr(err, 1);
  return cur;
}

__device__ __forceinline__ void uf_union(int* L, int a, int b, int bound, int* err) {
  for (int it = 0; it <= bound; ++it) {
    a = uf_find(L, a, bound, err);
    b = uf_find(L, b, bound, err);
    if (a == b) return;
    if (a < b) {
      const int t = a;
      a = b;
      b = t;
    }
    const int old = atomicMin(&L[a], b + 1) - 1;  // a > b: hang root a under b
    if (old == a) return;                        // a was still a root: linked
    a = old;                                     // somebody linked a first: go on from where it points
  }
  atomicOr(err, 2);
}

// parent = start of the pixel's horizontal run inside its 64-pixel chunk (one ballot per chunk): rows are linked without a single atomic.
__global__ __launch_bounds__(256) void label_init_kernel(const uint8_t* __restrict__ m, int* __restrict__ L, int B, int H, int W) {
  const int lane = threadIdx.x & 63;
  const int chunks = (W + 63) >> 6;
  const long items = (long)B * H * chunks;
  for (long item = (long)blockIdx.x * 4 + (threadIdx.x >> 6); item < items; item += (long)gridDim.x * 4) {
    const long row = item / chunks;  // tile * H + y
    const int ch = (int)(item - row * chunks);
    const int y = (int)(row % H);
    const int x = ch * 64 + lane;
    const bool fg = x < W && m[row * W + x] != 0;
    const unsigned long long mask = __ballot(fg);
    if (x < W) {
      const unsigned long long below = ~mask & ((1ull << lane) - 1ull);  // background pixels of the chunk left of this lane
      const int start = below ? 64 - __clzll((long long)below) : 0;
      L[row * W + x] = fg ? y * W + ch * 64 + start + 1 : 0;
    }
  }
}

__global__ __launch_bounds__(256) void label_merge_kernel(const uint8_t* __restrict__ m, int* L, int* err, int B, int H, int W) {
  const long HW = (long)H * W;
  const long g = (long)blockIdx.x * 256 + threadIdx.x;
  if (g >= (long)B * HW) return;
  const long tile = g / HW;
  const int p = (int)(g - tile * HW);
  const uint8_t* mt = m + tile * HW;
  if (!mt[p]) return;
  int* Lt = L + tile * HW;
  const int y = p / W, x = p - y * W;
  const bool left = x > 0 && mt[p - 1];
  if (left && (x & 63) == 0) uf_union(Lt, p, p - 1, (int)HW, err);
  // (up is redundant where left and up-left are both set: the pixel to the left makes the same link)
  if (y > 0 && mt[p - W] && !(left && mt[p - W - 1])) uf_union(Lt, p, p - W, (int)HW, err);
}

__global__ __launch_bounds__(256) void label_flatten_kernel(int* L, int* err, int B, int H, int W) {
  const long HW = (long)H * W;
  const long g = (long)blockIdx.x * 256 + threadIdx.x;
  if (g >= (long)B * HW) return;
  const long tile = g / HW;
  const int p = (int)(g - tile * HW);
  int* Lt = L + tile * HW;
  if (Lt[p] == 0) return;
  const int root = uf_find(Lt, p, (int)HW, err);
  atomicMin(&Lt[p], root + 1);
}

// ---- component table ---------------------------------------------------------------------------------------------------
// raw rows: [label, area, x0, y0, x1, y1]; table rows: [tile, label, area, x0, y0, x1, y1] (bounding box inclusive).
// counters[0] = roots found, counters[1] = components kept: both counted past `capacity`, written only below it.
// STITCH: labels are global (1 + slot*H*W + y*W + x, a root has L[g] == g + 1), boxes in mosaic pixels (origin [B][2] = the
// tile's x, y offset), table rows [label, area, X0, Y0, X1, Y1].

template <bool STITCH>
__global__ __launch_bounds__(256) void comp_roots_kernel(const int* __restrict__ L, int* slotmap, int* raw, int* counters, long capacity,
                                                         int B, int H, int W) {
  const long HW = (long)H * W;
  const long g = (long)blockIdx.x * 256 + threadIdx.x;
  if (g >= (long)B * HW) return;
  const int p = STITCH ? (int)g : (int)(g % HW);
  if (L[g] != p + 1) return;
  const int slot = atomicAdd(&counters[0], 1);
  slotmap[g] = slot;
  if (slot < capacity) {
    int* r = raw + (long)slot * 6;
    r[0] = p + 1;
    r[1] = 0;
    r[2] = STITCH ? 0x7fffffff : W;
    r[3] = STITCH ? 0x7fffffff : H;
    r[4] = -1;
    r[5] = -1;
  }
}

// One set of atomics per horizontal run of a label inside a wave's 64 consecutive pixels, not per pixel (a blob's pixels all hit the six
// ints of one row: per pixel that serialised to 1.4 ms for a 512 x 512 x 16 batch).  A lane heads a run where the lane before it
// (__shfl_up) is another label, another row or another wave; the run ends at the next head or background lane (one ballot).
template <bool STITCH>
__global__ __launch_bounds__(256) void comp_stats_kernel(const int* __restrict__ L, const int* __restrict__ slotmap, int* raw,
                                                         long capacity, int B, int H, int W, const int* __restrict__ origin) {
  const long HW = (long)H * W;
  const long g = (long)blockIdx.x * 256 + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const bool in = g < (long)B * HW;  // (no early return: every lane reaches the shuffle and the ballot)
  const int lab = in ? L[g] : 0;
  const long tile = in ? g / HW : 0;
  const int p = (int)(g - tile * HW);
  const int y = p / W, x = p - y * W;
  const int before = __shfl_up(lab, 1, 64);
  const bool head = lab != 0 && (lane == 0 || x == 0 || before != lab);
  const unsigned long long ends = __ballot(head || lab == 0);
  if (!head) return;
  const unsigned long long above = lane == 63 ? 0ull : ends & ~((2ull << lane) - 1ull);
  const int len = (above ? __ffsll((long long)above) - 1 : 64) - lane;  // the run stays in this row: x == 0 is a head
  const int slot = slotmap[(STITCH ? 0 : tile * HW) + lab - 1];
  if (slot >= capacity) return;
  int* r = raw + (long)slot * 6;
  const int X = STITCH ? x + origin[tile * 2] : x, Y = STITCH ? y + origin[tile * 2 + 1] : y;
  atomicAdd(&r[1], len);
  atomicMin(&r[2], X);
  atomicMin(&r[3], Y);
  atomicMax(&r[4], X + len - 1);
  atomicMax(&r[5], Y);
}

template <bool STITCH>
__global__ __launch_bounds__(256) void comp_filter_kernel(const int* __restrict__ L, const int* __restrict__ slotmap,
                                                          const int* __restrict__ raw, int* table, int* counters, long capacity, int B,
                                                          int H, int W, int min_area) {
  const long HW = (long)H * W;
  const long g = (long)blockIdx.x * 256 + threadIdx.x;
  if (g >= (long)B * HW) return;
  const int p = STITCH ? (int)g : (int)(g % HW);
  if (L[g] != p + 1) return;
  const int slot = slotmap[g];
  if (slot >= capacity) return;
  const int* r = raw + (long)slot * 6;
  if (r[1] < min_area) return;
  const int k = atomicAdd(&counters[1], 1);
  if (k >= capacity) return;
  int* t = table + (long)k * (STITCH ? 6 : 7);
  if (!STITCH) t[0] = (int)(g / HW);
#pragma unroll
  for (int j = 0; j < 6; ++j) t[(STITCH ? 0 : 1) + j] = r[j];
}

// ---- boundary edges ------------------------------------------------------------------------------------------------------
template <bool STITCH>
__global__ __launch_bounds__(256) void edges_mark_kernel(const int* __restrict__ table, long rows, uint8_t* keep, int B, long HW) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= rows) return;
  if (STITCH) {
    const int lab = table[i * 6];
    if (lab >= 1 && lab <= B * HW) keep[lab - 1] = 1;
    return;
  }
  const int tile = table[i * 7], lab = table[i * 7 + 1];
  if (tile >= 0 && tile < B && lab >= 1 && lab <= HW) keep[(long)tile * HW + lab - 1] = 1;
}

// Slot of the tile at (dx, dy) from `tile` in the neighbour table (order NW N NE W E SW S SE), -1 where absent (or out of range).
__device__ __forceinline__ int nbr_slot(const int* __restrict__ nbr, int tile, int dx, int dy, int T) {
  const int k = (dy + 1) * 3 + (dx + 1);
  const int n = nbr[(long)tile * 8 + (k > 4 ? k - 1 : k)];
  return n >= 0 && n < T ? n : -1;
}

// Walking round the pixel with the pixel on the right: 0 top (x,y)->(x+1,y), 1 right, 2 bottom, 3 left.  Rows [tile, label, x, y, dir].
// *counter counts every edge; rows are written only below `capacity` (a first call with capacity 0 sizes the list).
// STITCH: global labels; the 4-neighbour across a seam is the facing pixel of the neighbour tile (absent = outside); rows
// [label, X, Y, dir] in mosaic pixels.
template <bool STITCH>
__global__ __launch_bounds__(256) void edges_emit_kernel(const int* __restrict__ L, const uint8_t* __restrict__ keep, int* edges,
                                                         long capacity, unsigned int* counter, int B, int H, int W,
                                                         const int* __restrict__ nbr, const int* __restrict__ origin) {
  const long HW = (long)H * W;
  const long g = (long)blockIdx.x * 256 + threadIdx.x;
  const int lane = threadIdx.x & 63;
  int lab = 0, x = 0, y = 0, tile = 0;
  unsigned int dirs = 0;
  if (g < (long)B * HW) {
    tile = (int)(g / HW);
    const int p = (int)(g - (long)tile * HW);
    lab = L[g];
    if (lab && keep[(STITCH ? 0 : (long)tile * HW) + lab - 1]) {
      y = p / W;
      x = p - y * W;
      if (STITCH) {
        // (label across the seam: the facing pixel of the neighbour tile, 0 where there is none)
        int up = 0, right = 0, down = 0, left = 0, n;
        if (y > 0) up = L[g - W];
        else if ((n = nbr_slot(nbr, tile, 0, -1, B)) >= 0) up = L[(long)n * HW + (long)(H - 1) * W + x];
        if (x < W - 1) right = L[g + 1];
        else if ((n = nbr_slot(nbr, tile, 1, 0, B)) >= 0) right = L[(long)n * HW + (long)y * W];
        if (y < H - 1) down = L[g + W];
        else if ((n = nbr_slot(nbr, tile, 0, 1, B)) >= 0) down = L[(long)n * HW + x];
        if (x > 0) left = L[g - 1];
        else if ((n = nbr_slot(nbr, tile, -1, 0, B)) >= 0) left = L[(long)n * HW + (long)y * W + W - 1];
        dirs = (up != lab ? 1u : 0u) | (right != lab ? 2u : 0u) | (down != lab ? 4u : 0u) | (left != lab ? 8u : 0u);
        x += origin[tile * 2];
        y += origin[tile * 2 + 1];
      } else {
        if (y == 0 || L[g - W] != lab) dirs |= 1u;
        if (x == W - 1 || L[g + 1] != lab) dirs |= 2u;
        if (y == H - 1 || L[g + W] != lab) dirs |= 4u;
        if (x == 0 || L[g - 1] != lab) dirs |= 8u;
      }
    }
  }
  const int n = __popc(dirs);
  int incl = n;  // inclusive prefix sum over the wave
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int v = __shfl_up(incl, o, 64);
    if (lane >= o) incl += v;
  }
  const int total = __shfl(incl, 63, 64);
  if (total == 0) return;  // (uniform)
  unsigned int base = 0;
  if (lane == 63) base = atomicAdd(counter, (unsigned int)total);
  base = __shfl(base, 63, 64);
  long k = (long)base + incl - n;
  for (int d = 0; d < 4; ++d)
    if (dirs & (1u << d)) {
      if (k < capacity) {
        int* e = edges + k * (STITCH ? 4 : 5);
        if (!STITCH) *e++ = tile;
        e[0] = lab;
        e[1] = x;
        e[2] = y;
        e[3] = d;
      }
      ++k;
    }
}

// ---- stitching: all tiles of a call as one sparse raster ------------------------------------------------------------------
// GATHER: dst [T][H+2A][W+2A] = the tile with an apron of A pixels from its 8 neighbours (`fill` where there is none);
// !GATHER (crop): dst [T][H][W] = the centre of src [T][H+2A][W+2A].  A <= min(H, W): one step in the table reaches every apron pixel.
template <bool GATHER>
__global__ __launch_bounds__(256) void halo_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, const int* __restrict__ nbr,
                                                   int T, int H, int W, int A, int fill) {
  const int Hp = H + 2 * A, Wp = W + 2 * A;
  const long HW = (long)H * W, HWp = (long)Hp * Wp;
  const long g = (long)blockIdx.x * 256 + threadIdx.x;
  if (g >= (long)T * (GATHER ? HWp : HW)) return;
  if (!GATHER) {
    const long tile = g / HW;
    const int p = (int)(g - tile * HW);
    const int y = p / W, x = p - y * W;
    dst[g] = src[tile * HWp + (long)(y + A) * Wp + x + A];
    return;
  }
  const int tile = (int)(g / HWp);
  const int p = (int)(g - (long)tile * HWp);
  int y = p / Wp - A, x = p % Wp - A;
  const int dy = y < 0 ? -1 : y >= H ? 1 : 0, dx = x < 0 ? -1 : x >= W ? 1 : 0;
  const int from = (dx | dy) ? nbr_slot(nbr, tile, dx, dy, T) : tile;
  y -= dy * H;
  x -= dx * W;
  dst[g] = from >= 0 ? src[(long)from * HW + (long)y * W + x] : (uint8_t)fill;
}

// Per-tile canonical labels (1 + y*W + x of the tile's root) -> parents in the global index space slot*H*W + y*W + x: still a forest
// whose links only decrease, now bounded by P = T*H*W, for the same uf_find / uf_union.
__global__ __launch_bounds__(256) void stitch_global_kernel(int* L, long P, long HW) {
  const long g = (long)blockIdx.x * 256 + threadIdx.x;
  if (g >= P) return;
  const int l = L[g];
  if (l) L[g] = (int)(g / HW * HW) + l;
}

// One thread per seam pixel: item < H the right seam (x = W-1 against the E tile's x = 0), else the down seam (y = H-1 against the S
// tile's y = 0).  A pair whose predecessor along the seam is set on both sides too is already joined through it on either side.
__global__ __launch_bounds__(256) void stitch_seam_kernel(int* L, const int* __restrict__ nbr, int* err, int T, int H, int W) {
  const long HW = (long)H * W;
  const long g = (long)blockIdx.x * 256 + threadIdx.x;
  if (g >= (long)T * (H + W)) return;
  const int tile = (int)(g / (H + W));
  const int item = (int)(g - (long)tile * (H + W));
  const bool right = item < H;
  const int n = right ? nbr_slot(nbr, tile, 1, 0, T) : nbr_slot(nbr, tile, 0, 1, T);
  if (n < 0) return;
  const int i = right ? item : item - H;
  const long step = right ? W : 1;
  const long a = tile * HW + (right ? (long)i * W + W - 1 : (long)(H - 1) * W + i);
  const long b = n * HW + (right ? (long)i * W : (long)i);
  if (!L[a] || !L[b]) return;  // (a label is 0 or positive throughout: concurrent unions never change which)
  if (i > 0 && L[a - step] && L[b - step]) return;
  uf_union(L, (int)a, (int)b, (int)(T * HW), err);
}

__global__ __launch_bounds__(256) void stitch_flatten_kernel(int* L, int* err, long P) {
  const long g = (long)blockIdx.x * 256 + threadIdx.x;
  if (g >= P) return;
  if (L[g] == 0) return;
  const int root = uf_find(L, (int)g, (int)P, err);
  atomicMin(&L[g], root + 1);
}

// ---- thinning: Guo-Hall, two sub-iterations per pair (definitions: include/robosat_hip.h) ---------------------------------
// Bit-planes as in the morphology: ws [B][2][H][Wd], 32 pixels per word, bits beyond W zero.  One thread per word judges its 32
// pixels on plane `from` and writes plane `from ^ 1`: the eight neighbour words are the rows above and below and the words shifted
// by one bit, the three sums of the rule are bit-sliced (a 4-term sum is two half-adders: x = the pairs' XORs, c = their ANDs).
struct ThinArgs {
  uint32_t* ws;
  const int* nbr;  // STITCH: [B][8]
  int B, H, W, Wd;
};

// Word wx of row y of the tile at (dx, dy) from `tile`, 0 where there is none (per tile: every other tile is none).
template <bool STITCH>
__device__ __forceinline__ uint32_t thin_word(const ThinArgs& a, int from, int tile, int dx, int dy, int y, int wx) {
  int slot = tile;
  if (dx | dy) {
    if (!STITCH) return 0u;
    slot = nbr_slot(a.nbr, tile, dx, dy, a.B);
    if (slot < 0) return 0u;
  }
  return a.ws[((long)slot * 2 + from) * a.H * a.Wd + (long)y * a.Wd + wx];
}

// Row yy (-1 .. H: one beyond is the facing row of the tile above / below) at word wx: c = the pixels x, w = x - 1, e = x + 1.
// The pixel left of word 0 is the W tile's last pixel, the pixel right of pixel W - 1 the E tile's first (for any W: it lands on
// bit (W - 1) & 31 of e, which cur >> 1 leaves 0).  Bits beyond W of w hold no pixel: the caller masks with its own pixels.
template <bool STITCH>
__device__ __forceinline__ void thin_row(const ThinArgs& a, int from, int tile, int yy, int wx, uint32_t& w, uint32_t& c, uint32_t& e) {
  const int dy = yy < 0 ? -1 : yy >= a.H ? 1 : 0;
  const int y = yy - dy * a.H;
  if (!STITCH && dy) {
    w = c = e = 0u;
    return;
  }
  c = thin_word<STITCH>(a, from, tile, 0, dy, y, wx);
  const int last = (a.W - 1) & 31;
  const uint32_t before = wx > 0 ? thin_word<STITCH>(a, from, tile, 0, dy, y, wx - 1) >> 31
                                 : (thin_word<STITCH>(a, from, tile, -1, dy, y, a.Wd - 1) >> last) & 1u;
  w = (c << 1) | before;
  if (wx < a.Wd - 1)
    e = (c >> 1) | (thin_word<STITCH>(a, from, tile, 0, dy, y, wx + 1) << 31);
  else
    e = (c >> 1) | ((thin_word<STITCH>(a, from, tile, 1, dy, y, 0) & 1u) << last);
}

// Exactly one / at least two / all four of four 1-bit terms, per bit.
__device__ __forceinline__ void sum4(uint32_t t1, uint32_t t2, uint32_t t3, uint32_t t4, uint32_t& one, uint32_t& ge2, uint32_t& four) {
  const uint32_t xa = t1 ^ t2, ca = t1 & t2, xb = t3 ^ t4, cb = t3 & t4;
  one = (xa ^ xb) & ~(ca | cb);
  ge2 = ca | cb | (xa & xb);
  four = ca & cb;
}

// SECOND: the second sub-iteration of a pair.  total / last: int32 in device memory, the pixels deleted (one atomic per wave).
template <bool STITCH, bool SECOND>
__global__ __launch_bounds__(256) void thin_pass_kernel(const ThinArgs a, int from, int* total, int* last) {
  const int tile = blockIdx.y;
  const long words = (long)a.H * a.Wd;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  uint32_t del = 0u;
  if (i < words) {  // (no early return: every lane reaches the shuffles)
    const int y = (int)(i / a.Wd), wx = (int)(i - (long)y * a.Wd);
    uint32_t p9, p2, p3, p8, p, p4, p7, p6, p5;
    thin_row<STITCH>(a, from, tile, y, wx, p8, p, p4);
    if (p) {
      thin_row<STITCH>(a, from, tile, y - 1, wx, p9, p2, p3);
      thin_row<STITCH>(a, from, tile, y + 1, wx, p7, p6, p5);
      uint32_t c1, n1, n1x, n2, n2x, unused;
      sum4(~p2 & (p3 | p4), ~p4 & (p5 | p6), ~p6 & (p7 | p8), ~p8 & (p9 | p2), c1, unused, unused);
      sum4(p9 | p2, p3 | p4, p5 | p6, p7 | p8, unused, n1, n1x);
      sum4(p2 | p3, p4 | p5, p6 | p7, p8 | p9, unused, n2, n2x);
      const uint32_t m = SECOND ? (p6 | p7 | ~p9) & p8 : (p2 | p3 | ~p5) & p4;
      del = p & c1 & n1 & n2 & ~(n1x & n2x) & ~m;  // min(N1, N2) in 2..3: both >= 2, not both 4
    }
    a.ws[((long)tile * 2 + (from ^ 1)) * words + i] = p & ~del;
  }
  int n = __popc(del);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
  if (n && (threadIdx.x & 63) == 0) {
    atomicAdd(total, n);
    if (last) atomicAdd(last, n);
  }
}

// masks != 0 -> plane 0 (one ballot per 64 pixels, as select_pack).
__global__ __launch_bounds__(256) void thin_pack_kernel(const uint8_t* __restrict__ masks, const ThinArgs a) {
  const int tile = blockIdx.y, lane = threadIdx.x & 63;
  const uint8_t* img = masks + (long)tile * a.H * a.W;
  uint32_t* plane = a.ws + (long)tile * 2 * a.H * a.Wd;
  const int chunks = (a.W + 63) >> 6;
  for (int item = blockIdx.x * 4 + (threadIdx.x >> 6); item < a.H * chunks; item += gridDim.x * 4) {  // (wave-uniform)
    const int y = item / chunks, ch = item - y * chunks;
    const int x = ch * 64 + lane;
    const unsigned long long m = __ballot(x < a.W && img[(long)y * a.W + x] != 0);
    if (lane == 0) plane[(long)y * a.Wd + ch * 2] = (uint32_t)m;
    if (lane == 32 && ch * 2 + 1 < a.Wd) plane[(long)y * a.Wd + ch * 2 + 1] = (uint32_t)(m >> 32);
  }
}

// ---- skeleton links ---------------------------------------------------------------------------------------------------------
// Global index of pixel (x, y) of `tile`, x and y at most one beyond it: the facing pixel of the neighbour tile, -1 where none is.
template <bool STITCH>
__device__ __forceinline__ long pixel_at(const int* __restrict__ nbr, int tile, int x, int y, int B, int H, int W) {
  const int dx = x < 0 ? -1 : x >= W ? 1 : 0, dy = y < 0 ? -1 : y >= H ? 1 : 0;
  int slot = tile;
  if (dx | dy) {
    if (!STITCH) return -1;
    slot = nbr_slot(nbr, tile, dx, dy, B);
    if (slot < 0) return -1;
  }
  return (long)slot * H * W + (long)(y - dy * H) * W + (x - dx * W);
}

// Links of skeleton pixel p: 0 E, 2 S, 1 SE where neither E nor S is set, 3 SW where neither W nor S is set; a pixel without any
// set 8-neighbour has no link at either end and emits one row with dir -1.  A link is emitted where either end's component is kept,
// under the label of p's where that is kept, else of the other end's.  Rows and counter as edges_emit_kernel.
template <bool STITCH>
__global__ __launch_bounds__(256) void links_emit_kernel(const uint8_t* __restrict__ S, const int* __restrict__ L,
                                                         const uint8_t* __restrict__ keep, int* links, long capacity, unsigned int* counter,
                                                         int B, int H, int W, const int* __restrict__ nbr, const int* __restrict__ origin) {
  const long HW = (long)H * W;
  const long g = (long)blockIdx.x * 256 + threadIdx.x;
  const int lane = threadIdx.x & 63;
  int x = 0, y = 0, tile = 0;
  int lab[5] = {0, 0, 0, 0, 0};  // label of the row for dir 0..3, [4]: the lone pixel
  unsigned int dirs = 0;
  if (g < (long)B * HW && S[g]) {
    tile = (int)(g / HW);
    const int p = (int)(g - (long)tile * HW);
    y = p / W;
    x = p - y * W;
    const long base = STITCH ? 0 : (long)tile * HW, top = STITCH ? (long)B * HW : HW;
    const int own = L[g];
    const bool own_kept = own >= 1 && own <= top && keep[base + own - 1];
    // E, SE, S, SW, W, NW, N, NE
    const int ox[8] = {1, 1, 0, -1, -1, -1, 0, 1}, oy[8] = {0, 1, 1, 1, 0, -1, -1, -1};
    long at[8];
    unsigned int set = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      at[k] = pixel_at<STITCH>(nbr, tile, x + ox[k], y + oy[k], B, H, W);
      if (at[k] >= 0 && S[at[k]]) set |= 1u << k;
    }
    const bool e = set & 1u, se = set & 2u, s = set & 4u, sw = set & 8u, w = set & 16u;
    const unsigned int want = (e ? 1u : 0u) | (se && !e && !s ? 2u : 0u) | (s ? 4u : 0u) | (sw && !w && !s ? 8u : 0u);
#pragma unroll
    for (int d = 0; d < 4; ++d)
      if (want & (1u << d)) {
        const int other = L[at[d]];
        const bool other_kept = other >= 1 && other <= top && keep[base + other - 1];
        if (own_kept || other_kept) {
          dirs |= 1u << d;
          lab[d] = own_kept ? own : other;
        }
      }
    if (!set && own_kept) {
      dirs = 16u;
      lab[4] = own;
    }
    if (STITCH) {
      x += origin[tile * 2];
      y += origin[tile * 2 + 1];
    }
  }
  const int n = __popc(dirs);
  int incl = n;  // inclusive prefix sum over the wave
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int v = __shfl_up(incl, o, 64);
    if (lane >= o) incl += v;
  }
  const int total = __shfl(incl, 63, 64);
  if (total == 0) return;  // (uniform)
  unsigned int first = 0;
  if (lane == 63) first = atomicAdd(counter, (unsigned int)total);
  first = __shfl(first, 63, 64);
  long k = (long)first + incl - n;
#pragma unroll
  for (int d = 0; d < 5; ++d)
    if (dirs & (1u << d)) {
      if (k < capacity) {
        int* r = links + k * (STITCH ? 4 : 5);
        if (!STITCH) *r++ = tile;
        r[0] = lab[d];
        r[1] = x;
        r[2] = y;
        r[3] = d < 4 ? d : -1;
      }
      ++k;
    }
}

// ---- overlap table of two label rasters (`rs features --dedupe`) -------------------------------------------------------------
// An open-addressing table in global memory: keys [S] uint64 = (raster * group + label_a) << 32 | label_b (never 0: label_a >= 1),
// then counts [S] int32; S a power of two >= 2 * capacity, linear probing from a mixed hash.  A slot is claimed by a 64-bit
// atomicCAS against 0 and counted by atomicAdd.  Masks are runs of one pair (a whole tile can be a single pair), so equal keys are
// merged before the table sees them: a thread owns kOvRun consecutive pixels and merges equal neighbours; then, kOvRounds times,
// the first lane of the wave that still holds a key broadcasts it, every lane hands over what it holds of that key, the wave sums
// it (shuffles) and that one lane adds it; the first round also merges the block's four waves through LDS.  What is left after the
// rounds (a wave over many small pairs) goes to the table per lane.
constexpr int kOvRun = 4;  // (one 16-byte load per raster; the code below spells out four keys)
constexpr int kOvRounds = 4;
constexpr long kOvMinSlots = 16;
constexpr int kOvMaxProbe = 1024;  // (at a load of 1/2 a probe sequence of a mixed hash is tens of slots at the very most)

long overlap_slots(long capacity) {
  long s = kOvMinSlots;
  while (s < 2 * capacity) s <<= 1;
  return s;
}

__device__ __forceinline__ unsigned long long ov_mix(unsigned long long k) {  // (the finaliser of splitmix64)
  k ^= k >> 30;
  k *= 0xbf58476d1ce4e5b9ull;
  k ^= k >> 27;
  k *= 0x94d049bb133111ebull;
  return k ^ (k >> 31);
}

// counts[slot of key] += n.  The probe loop is bounded by `probes` <= S; a probe that runs out raises counters[1], and once it is
// raised nobody probes any more (the rows of that call are void: the caller comes back with a larger table).
__device__ __forceinline__ void ov_add(unsigned long long* keys, int* counts, int* counters, unsigned long long mask, int probes,
                                       unsigned long long key, int n) {
  if (__hip_atomic_load(&counters[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;
  unsigned long long i = ov_mix(key) & mask;
  for (int it = 0; it < probes; ++it) {
    unsigned long long cur = __hip_atomic_load(&keys[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (cur == 0ull) cur = atomicCAS(&keys[i], 0ull, key);  // (a slot never changes once it holds a key)
    if (cur == 0ull || cur == key) {
      atomicAdd(&counts[i], n);
      return;
    }
    i = (i + 1) & mask;
  }
  atomicAdd(&counters[1], 1);
}

__global__ __launch_bounds__(256) void overlaps_count_kernel(const int* __restrict__ A, const int* __restrict__ B, unsigned long long* keys,
                                                             int* counts, int* counters, unsigned long long mask, int probes, long pixels,
                                                             long group, int vec) {
  const long p0 = ((long)blockIdx.x * 256 + threadIdx.x) * kOvRun;
  const int lane = threadIdx.x & 63;
  int a[kOvRun], b[kOvRun];
  if (vec && p0 + kOvRun <= pixels) {
    const int4 va = *reinterpret_cast<const int4*>(A + p0), vb = *reinterpret_cast<const int4*>(B + p0);
    a[0] = va.x, a[1] = va.y, a[2] = va.z, a[3] = va.w;
    b[0] = vb.x, b[1] = vb.y, b[2] = vb.z, b[3] = vb.w;
  } else {
#pragma unroll
    for (int j = 0; j < kOvRun; ++j) {
      const bool in = p0 + j < pixels;
      a[j] = in ? A[p0 + j] : 0;
      b[j] = in ? B[p0 + j] : 0;
    }
  }
  // (no early return: every lane reaches the ballots and shuffles below)
  unsigned long long key[kOvRun];
  int cnt[kOvRun];
  const long r0 = p0 < pixels ? p0 / group : 0;
  const bool one_raster = p0 + kOvRun <= (r0 + 1) * group;
#pragma unroll
  for (int j = 0; j < kOvRun; ++j) {
    const long raster = one_raster ? r0 : (p0 + j) / group;
    const bool both = a[j] != 0 && b[j] != 0;
    key[j] = both ? (unsigned long long)(unsigned int)(raster * group + a[j]) << 32 | (unsigned int)b[j] : 0ull;
    cnt[j] = both ? 1 : 0;
  }
#pragma unroll
  for (int j = 1; j < kOvRun; ++j)
    if (key[j] != 0ull && key[j] == key[j - 1]) {
      cnt[j] += cnt[j - 1];
      key[j - 1] = 0ull;
    }
  // round 0 also merges across the block's four waves through LDS (a tile that is one pair: one atomic per 1024 pixels)
  __shared__ unsigned long long wave_key[4];
  __shared__ int wave_cnt[4];
  const int wave = threadIdx.x >> 6;
  for (int round = 0; round < kOvRounds; ++round) {
    const unsigned long long mine = key[0] ? key[0] : key[1] ? key[1] : key[2] ? key[2] : key[3];
    const unsigned long long who = __ballot(mine != 0ull);
    if (!who && round > 0) return;  // (uniform; round 0 goes on to the barrier)
    const int leader = who ? __ffsll((long long)who) - 1 : 0;
    const unsigned int hi = (unsigned int)__shfl((int)(mine >> 32), leader, 64), lo = (unsigned int)__shfl((int)mine, leader, 64);
    const unsigned long long k = (unsigned long long)hi << 32 | lo;  // (0 where the wave holds nothing: matches no lane's key)
    int n = 0;
#pragma unroll
    for (int j = 0; j < kOvRun; ++j)
      if (k != 0ull && key[j] == k) {
        n += cnt[j];
        key[j] = 0ull;
      }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
    if (round == 0) {
      if (lane == 0) {
        wave_key[wave] = k;
        wave_cnt[wave] = n;
      }
      rs_lds_writes_done();
      __syncthreads();
      if (!who) return;  // (uniform)
      if (lane == leader) {  // the first wave of the block that holds k adds for all of them
        bool first = true;
        int total = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w)
          if (wave_key[w] == k) {
            first = first && w >= wave;
            total += wave_cnt[w];
          }
        if (first) ov_add(keys, counts, counters, mask, probes, k, total);
      }
    } else if (lane == leader) {
      ov_add(keys, counts, counters, mask, probes, k, n);
    }
  }
#pragma unroll
  for (int j = 0; j < kOvRun; ++j)
    if (key[j] != 0ull) ov_add(keys, counts, counters, mask, probes, key[j], cnt[j]);
}

// Slots in use -> rows [raster, label_a, label_b, count]: a block of 256 threads takes 256 * kOvRowsRun slots and draws its rows with
// one atomic (one per wave serialised the waves of a large table on the one counter); counters[0] counts every slot in use.
constexpr int kOvRowsRun = 8;

__global__ __launch_bounds__(256) void overlaps_rows_kernel(const unsigned long long* __restrict__ keys, const int* __restrict__ counts,
                                                            int* rows, long capacity, int* counters, long slots, long group) {
  __shared__ int wave_total[4];
  __shared__ int block_base;
  const long first = (long)blockIdx.x * (256 * kOvRowsRun) + threadIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned long long key[kOvRowsRun];
  int n = 0;
#pragma unroll
  for (int j = 0; j < kOvRowsRun; ++j) {
    const long i = first + j * 256;
    key[j] = i < slots ? keys[i] : 0ull;
    n += key[j] != 0ull ? 1 : 0;
  }
  int incl = n;  // inclusive prefix sum over the wave
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int v = __shfl_up(incl, o, 64);
    if (lane >= o) incl += v;
  }
  if (lane == 63) wave_total[wave] = incl;
  rs_lds_writes_done();
  __syncthreads();
  if (threadIdx.x == 0) {
    const int total = wave_total[0] + wave_total[1] + wave_total[2] + wave_total[3];
    block_base = total ? atomicAdd(&counters[0], total) : 0;
  }
  rs_lds_writes_done();
  __syncthreads();
  long k = (long)block_base + incl - n;
  for (int w = 0; w < wave; ++w) k += wave_total[w];
#pragma unroll
  for (int j = 0; j < kOvRowsRun; ++j) {
    if (key[j] == 0ull) continue;
    if (k < capacity) {
      const long at = (long)(key[j] >> 32);  // raster * group + label_a, label_a in 1 .. group
      const long raster = (at - 1) / group;
      int* r = rows + k * 4;
      r[0] = (int)raster;
      r[1] = (int)(at - raster * group);
      r[2] = (int)(unsigned int)key[j];
      r[3] = counts[first + j * 256];
    }
    ++k;
  }
}

// ---- capped squared Euclidean distance transform (`rs features --width`; definitions: include/robosat_hip.h) ------------------
// Two launches.  Row pass: g = the horizontal distance to the nearest unset pixel of the row, capped at R (a byte).  Column pass:
// d2 = min(R*R, min over dy of g(x, y + dy)^2 + dy^2).  Integers only, no atomics, every output written by exactly one thread.
constexpr int kEdtMaxR = 128;
constexpr int kEdtRows = 64;     // TH: rows of a column-pass strip
constexpr int kEdtNoRow = 255;   // g of a row that is not there: 255^2 > kEdtMaxR^2, so it never wins against the cap

// One wave per 64 columns of a row: a ballot of "unset" for the chunk and for ceil(R / 64) chunks either side, then count-leading /
// trailing-zeros on those words.  A column left of 0 / right of W - 1 is the W / E tile's (STITCH), or is not there at all; what
// lies more than one tile away is beyond R <= W.
template <bool STITCH>
__global__ __launch_bounds__(256) void edt_row_kernel(const uint8_t* __restrict__ m, const int* __restrict__ nbr, uint8_t* __restrict__ g,
                                                      int B, int H, int W, int R) {
  const int lane = threadIdx.x & 63;
  const int chunks = (W + 63) >> 6;
  const int side = (R + 63) >> 6;  // 1 or 2
  const long HW = (long)H * W;
  const long items = (long)B * H * chunks;
  for (long item = (long)blockIdx.x * 4 + (threadIdx.x >> 6); item < items; item += (long)gridDim.x * 4) {  // (wave-uniform)
    const long row = item / chunks;  // tile * H + y
    const int ch = (int)(item - row * chunks);
    const int tile = (int)(row / H), y = (int)(row - (long)tile * H);
    unsigned long long word[5];  // unset pixels of chunks ch - 2 .. ch + 2
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      word[k] = 0ull;
      if (k - 2 < -side || k - 2 > side) continue;  // (uniform)
      int x = (ch + k - 2) * 64 + lane;
      const int dx = x < 0 ? -1 : x >= W ? 1 : 0;
      x -= dx * W;
      int slot = tile;
      if (dx) slot = STITCH && x >= 0 && x < W ? nbr_slot(nbr, tile, dx, 0, B) : -1;
      word[k] = __ballot(slot >= 0 && m[(long)slot * HW + (long)y * W + x] == 0);
    }
    const int x = ch * 64 + lane;
    if (x < W) {  // (behind the ballots: every lane reaches them)
      const unsigned long long below = word[2] & ((2ull << lane) - 1ull);  // (lane 63: 2 << 63 wraps to 0, 0 - 1 = all ones)
      const unsigned long long above = word[2] & ~((1ull << lane) - 1ull);
      int left = R, right = R;
      if (below) left = lane - (63 - __clzll((long long)below));
      else if (word[1]) left = lane + 1 + __clzll((long long)word[1]);
      else if (word[0]) left = lane + 65 + __clzll((long long)word[0]);
      if (above) right = __ffsll((long long)above) - 1 - lane;
      else if (word[3]) right = 63 - lane + __ffsll((long long)word[3]);
      else if (word[4]) right = 127 - lane + __ffsll((long long)word[4]);
      const int d = left < right ? left : right;
      g[row * W + x] = (uint8_t)(d < R ? d : R);
    }
  }
}

// g of rows yy (one tile up or down at most) at the strip's 64 columns, as the column pass stages it.  A row above / below the tile is
// the N / S tile's (STITCH).  Where that tile is absent its pixels are unknown, not unset, but the unset pixels of the NW / NE
// (SW / SE) tile still count: from column x the nearest one in that row is x + 1 + g of the W-side tile's last column away, or
// W - x + g of the E-side tile's first column (their own row pass found nothing in the absent tile between).
template <bool STITCH>
__device__ __forceinline__ int edt_staged(const uint8_t* __restrict__ g, const int* __restrict__ nbr, int tile, int yy, int x, int B, int H,
                                          int W) {
  const int dy = yy < 0 ? -1 : yy >= H ? 1 : 0;
  const int y = yy - dy * H;
  const long HW = (long)H * W;
  if (!dy) return g[(long)tile * HW + (long)y * W + x];
  if (!STITCH || y < 0 || y >= H) return kEdtNoRow;
  const int n = nbr_slot(nbr, tile, 0, dy, B);
  if (n >= 0) return g[(long)n * HW + (long)y * W + x];
  const int w = nbr_slot(nbr, tile, -1, dy, B), e = nbr_slot(nbr, tile, 1, dy, B);
  int best = kEdtNoRow;
  if (w >= 0) best = min(best, x + 1 + (int)g[(long)w * HW + (long)y * W + W - 1]);
  if (e >= 0) best = min(best, W - x + (int)g[(long)e * HW + (long)y * W]);
  return best;
}

// A block takes 64 columns x kEdtRows rows of one tile: it stages g of the rows y0 - R .. y0 + kEdtRows - 1 + R in LDS (at most
// (64 + 256) * 64 bytes = 20 KB), then every lane owns a column (a wave reads 64 consecutive bytes: no bank conflict) and walks outward
// in |dy| until dy * dy >= the best so far.  Columns beyond W are staged as kEdtNoRow and written nowhere.
template <bool STITCH>
__global__ __launch_bounds__(256) void edt_col_kernel(const uint8_t* __restrict__ g, const int* __restrict__ nbr, int* __restrict__ d2,
                                                      int B, int H, int W, int R) {
  extern __shared__ __attribute__((aligned(16))) uint8_t staged[];  // [kEdtRows + 2R][64]
  const int tile = blockIdx.z, y0 = blockIdx.y * kEdtRows, x0 = blockIdx.x * 64;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int rows = kEdtRows + 2 * R;
  const int x = x0 + lane;
  for (int r = wave; r < rows; r += 4) staged[r * 64 + lane] = (uint8_t)(x < W ? edt_staged<STITCH>(g, nbr, tile, y0 - R + r, x, B, H, W) : kEdtNoRow);
  __syncthreads();
  if (x >= W) return;
  const int cap = R * R;
  for (int ry = wave; ry < kEdtRows && y0 + ry < H; ry += 4) {
    const uint8_t* at = staged + (ry + R) * 64 + lane;
    const int own = at[0];
    int best = min(cap, own * own);
    for (int d = 1; d * d < best; ++d) {  // (best <= R * R: d stays below R, inside the staged rows)
      const int up = at[-d * 64], down = at[d * 64];
      best = min(best, min(up * up, down * down) + d * d);
    }
    d2[((long)tile * H + y0 + ry) * W + x] = best;
  }
}

// ---- instances: seeds and regrowth (`rs features --split`; definitions: include/robosat_hip.h) -------------------------------
__global__ __launch_bounds__(256) void split_cores_kernel(const int* __restrict__ d2, uint8_t* __restrict__ cores, long pixels, int cap) {
  const long p = (long)blockIdx.x * 256 + threadIdx.x;
  if (p < pixels) cores[p] = d2[p] == cap ? 1 : 0;
}

// has[root of the Lm component] = 1 for every seed pixel (every racer stores the same byte).
__global__ __launch_bounds__(256) void split_mark_kernel(const int* __restrict__ Lm, const int* __restrict__ Ls, uint8_t* has, long pixels,
                                                         long group) {
  const long p = (long)blockIdx.x * 256 + threadIdx.x;
  if (p >= pixels || Ls[p] == 0) return;
  const int lm = Lm[p];
  if (lm >= 1 && lm <= group) has[p / group * group + lm - 1] = 1;
}

// (Lm, Ls and out may be one another: a thread reads its own pixel before it writes it, and nobody else's)
__global__ __launch_bounds__(256) void split_start_kernel(const int* Lm, const int* Ls, const uint8_t* __restrict__ has, int* out,
                                                          long pixels, long group) {
  const long p = (long)blockIdx.x * 256 + threadIdx.x;
  if (p >= pixels) return;
  const int lm = Lm[p], ls = Ls[p];
  int v = 0;
  if (ls != 0) v = ls;
  else if (lm >= 1 && lm <= group) v = has[p / group * group + lm - 1] ? -1 : lm;
  out[p] = v;
}

// A block of kGrowH x kGrowW pixels of one tile with an apron of K pixels, in LDS as [kGrowH + 2K][kGrowW + 2K]; thread t owns
// the region's pixels j * 256 + t.  `pend`: bit j = that pixel is -1 and not on the region's outermost ring (so its four neighbours
// are in LDS: no bounds in the step loop); `core`: bit j = the pixel is the block's own and inside the tile.
constexpr int kGrowH = 32, kGrowW = 64;
constexpr int kGrowMaxK = 16;
constexpr int kGrowRule = 12;  // steps per launch (profiles/features_split: 0.16 ms against 0.52 ms at K = 1 for 16 x 512 x 512)
constexpr int kGrowPer = ((kGrowH + 2 * kGrowMaxK) * (kGrowW + 2 * kGrowMaxK) + 255) / 256;  // 24

struct GrowArgs {
  const int* src;
  int* dst;
  const int* nbr;  // STITCH: [B][8]
  uint8_t* done;   // [2][blocks]: plane `to` = this block's pixels of dst are final
  int* counters;
  int B, H, W, K, steps, to, last;
};

template <bool STITCH>
__global__ __launch_bounds__(256) void grow_kernel(const GrowArgs a) {
  extern __shared__ __attribute__((aligned(16))) int region[];
  const int K = a.K, RH = kGrowH + 2 * K, RW = kGrowW + 2 * K, RN = RH * RW;
  const int tile = blockIdx.z, y0 = blockIdx.y * kGrowH - K, x0 = blockIdx.x * kGrowW - K;
  const long HW = (long)a.H * a.W;
  const long block = ((long)tile * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x, blocks = (long)gridDim.x * gridDim.y * gridDim.z;
  unsigned int pend = 0u, core = 0u;
  long at[kGrowPer];  // (of the core pixels only: where they go in dst)
#pragma unroll
  for (int j = 0; j < kGrowPer; ++j) {
    const int i = j * 256 + threadIdx.x;
    at[j] = -1;
    if (i >= RN) continue;
    const int ry = i / RW, rx = i - ry * RW;
    int y = y0 + ry, x = x0 + rx;
    const int dy = y < 0 ? -1 : y >= a.H ? 1 : 0, dx = x < 0 ? -1 : x >= a.W ? 1 : 0;
    int v = 0;
    if (!(dx | dy)) {
      const long g = (long)tile * HW + (long)y * a.W + x;
      v = a.src[g];
      if (ry >= K && ry < K + kGrowH && rx >= K && rx < K + kGrowW) {
        core |= 1u << j;
        at[j] = g;
      }
    } else if (STITCH) {  // (K <= min(H, W): one step in the table reaches the apron)
      y -= dy * a.H;
      x -= dx * a.W;
      const int n = y >= 0 && y < a.H && x >= 0 && x < a.W ? nbr_slot(a.nbr, tile, dx, dy, a.B) : -1;
      if (n >= 0) v = a.src[(long)n * HW + (long)y * a.W + x];
    }
    region[i] = v;
    if (v == -1 && ry > 0 && ry < RH - 1 && rx > 0 && rx < RW - 1) pend |= 1u << j;
  }
  // bit 0: a pixel of this block is still -1; bit 1: dst already holds this block (the byte is this block's own and is read by
  // thread 0 alone, before the barrier; the store below comes behind it, so no thread of this launch can see that store)
  uint8_t* done = a.done + (long)a.to * blocks + block;
  int state = (pend & core) ? 1 : 0;
  if (threadIdx.x == 0 && *done) state |= 2;
  rs_lds_writes_done();
  state = __syncthreads_or(state);
  if (!(state & 1)) {  // nothing left in this block: dst gets it once, then the block only looks
    if (state & 2) return;  // (uniform)
#pragma unroll
    for (int j = 0; j < kGrowPer; ++j)
      if (core & (1u << j)) a.dst[at[j]] = region[j * 256 + threadIdx.x];
    if (threadIdx.x == 0) *done = 1;
    return;
  }
  const unsigned int before = pend & core;
  for (int s = 0; s < a.steps; ++s) {
    int fresh[kGrowPer];
    unsigned int got = 0u;
#pragma unroll
    for (int j = 0; j < kGrowPer; ++j) {
      fresh[j] = 0;
      if (pend & (1u << j)) {
        const int i = j * 256 + threadIdx.x;
        const int n = region[i - RW], w = region[i - 1], e = region[i + 1], so = region[i + RW];
        const int v = n > 0 ? n : w > 0 ? w : e > 0 ? e : so > 0 ? so : 0;
        if (v > 0) {
          fresh[j] = v;
          got |= 1u << j;
        }
      }
    }
    __syncthreads();  // every neighbour has been read as it stood before the step
#pragma unroll
    for (int j = 0; j < kGrowPer; ++j)
      if (got & (1u << j)) region[j * 256 + threadIdx.x] = fresh[j];
    pend &= ~got;
    rs_lds_writes_done();
    if (!__syncthreads_or((int)pend)) break;  // (uniform)
  }
#pragma unroll
  for (int j = 0; j < kGrowPer; ++j)
    if (core & (1u << j)) a.dst[at[j]] = region[j * 256 + threadIdx.x];
  int assigned = __popc(before & ~pend), left = __popc(pend & core);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    assigned += __shfl_xor(assigned, o, 64);
    left += __shfl_xor(left, o, 64);
  }
  // one atomic per block and counter
  __shared__ int tally[2][4];
  if ((threadIdx.x & 63) == 0) {
    tally[0][threadIdx.x >> 6] = assigned;
    tally[1][threadIdx.x >> 6] = left;
  }
  rs_lds_writes_done();
  __syncthreads();
  if (threadIdx.x == 0) {
    assigned = tally[0][0] + tally[0][1] + tally[0][2] + tally[0][3];
    left = tally[1][0] + tally[1][1] + tally[1][2] + tally[1][3];
    if (assigned) atomicAdd(&a.counters[0], assigned);
    if (left && a.last) atomicAdd(&a.counters[1], left);
  }
}

// ---- per-component sums of probability bytes (`rs features --score`; definitions: include/robosat_hip.h) ----------------------
// rowmap [pixels]: -1, or the table row of the component whose label names that pixel (label = 1 + the pixel's index in its raster).
constexpr int kScoreMaxK = 8;
constexpr int kScorePairs = kScoreMaxK / 2;  // two models share a register: a block's sum is at most 256 * 255 < 2^16

__global__ __launch_bounds__(256) void score_rows_kernel(const int* __restrict__ table, long rows, int width, int* rowmap, long pixels,
                                                         long group) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= rows) return;
  const long raster = width == 7 ? table[i * 7] : 0;
  const int lab = table[i * width + (width == 7 ? 1 : 0)];
  if (raster >= 0 && raster < pixels / group && lab >= 1 && lab <= group) rowmap[raster * group + lab - 1] = (int)i;
}

// One atomic per model and run of a label, a run being consecutive pixels of one label in one raster inside the block's 256 (it may
// go on across the end of a raster row: sums do not care).  Inside a wave the bytes of a run are summed by a segmented suffix scan
// (__shfl_down, bounded by the run's end from one ballot); the run that ends a wave takes in the first runs of the waves behind it
// through LDS, so a tile that is one blob costs one atomic per model and 256 pixels (per pixel they would all hit one row's K words).
__global__ __launch_bounds__(256) void score_sum_kernel(const int* __restrict__ L, const uint8_t* __restrict__ q,
                                                        const int* __restrict__ rowmap, unsigned long long* sums, long pixels, long group,
                                                        int K) {
  __shared__ int join0[4], lab63[4], full[4];  // the label lane 0 may carry on from the wave before (0: none), lane 63's, "one run"
  __shared__ unsigned int tot0[4][kScorePairs];
  const long base = (long)blockIdx.x * 256;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long g = base + threadIdx.x;
  const bool in = g < pixels;  // (no early return: every lane reaches the shuffles, the ballot and the barrier)
  const int lab = in ? L[g] : 0;
  long raster = base / group;  // (uniform; only a block that holds a raster's border divides per lane)
  long off = base - raster * group + threadIdx.x;
  if (off >= group) {
    raster += off / group;
    off %= group;
  }
  unsigned int v[kScorePairs];
#pragma unroll
  for (int j = 0; j < kScorePairs; ++j) {
    v[j] = 0;
    if (lab != 0 && 2 * j < K) v[j] = q[(long)(2 * j) * pixels + g];
    if (lab != 0 && 2 * j + 1 < K) v[j] |= (unsigned int)q[(long)(2 * j + 1) * pixels + g] << 16;
  }
  const int before = __shfl_up(lab, 1, 64);
  const bool start = lane == 0 || before != lab || off == 0;
  const unsigned long long starts = __ballot(start);
  const unsigned long long above = lane == 63 ? 0ull : starts & ~((2ull << lane) - 1ull);
  const int end = above ? __ffsll((long long)above) - 1 : 64;  // the run is lanes [its start, end)
#pragma unroll
  for (int o = 1; o < 64; o <<= 1)
#pragma unroll
    for (int j = 0; j < kScorePairs; ++j)
      if (2 * j < K) {  // (uniform)
        const unsigned int t = (unsigned int)__shfl_down((int)v[j], o, 64);
        if (lane + o < end) v[j] += t;  // v = the sum over [lane, min(lane + 2 o, end))
      }
  if (lane == 0) {
    join0[wave] = off == 0 ? 0 : lab;
    full[wave] = end == 64;
#pragma unroll
    for (int j = 0; j < kScorePairs; ++j) tot0[wave][j] = v[j];
  }
  if (lane == 63) lab63[wave] = lab;
  rs_lds_writes_done();
  __syncthreads();
  if (!start || lab < 1 || lab > group) return;
  if (lane == 0 && wave > 0 && join0[wave] != 0 && join0[wave] == lab63[wave - 1]) return;  // the run began in an earlier wave
  if (end == 64)
    for (int w = wave + 1; w < 4; ++w) {
      if (join0[w] == 0 || join0[w] != lab63[w - 1]) break;
#pragma unroll
      for (int j = 0; j < kScorePairs; ++j) v[j] += tot0[w][j];
      if (!full[w]) break;
    }
  const int row = rowmap[raster * group + lab - 1];
  if (row < 0) return;  // (a component the table does not list)
#pragma unroll
  for (int j = 0; j < kScorePairs; ++j) {
    if (2 * j < K && (v[j] & 0xffffu)) atomicAdd(&sums[(long)row * K + 2 * j], (unsigned long long)(v[j] & 0xffffu));
    if (2 * j + 1 < K && (v[j] >> 16)) atomicAdd(&sums[(long)row * K + 2 * j + 1], (unsigned long long)(v[j] >> 16));
  }
}

int grow_fused() {
  const int k = rs_knobs().grow_fused;
  return k >= 1 && k <= kGrowMaxK ? k : kGrowRule;
}

long grow_blocks(int B, int H, int W) { return (long)B * rs_cdiv(H, kGrowH) * rs_cdiv(W, kGrowW); }

// (B rides in gridDim.y; 4 edges per pixel at the very most stay below 2^31 in the int32 edge counter)
bool shape_ok(int B, int H, int W) { return B > 0 && B <= 65535 && H > 0 && W > 0 && H <= 4096 && W <= 4096 && (long)B * H * W < (1l << 29); }

bool halo_ok(int T, int H, int W, int A) {
  return A >= 0 && H > 0 && W > 0 && A <= (H < W ? H : W) && shape_ok(T, H, W) && shape_ok(T, H + 2 * A, W + 2 * A);
}

}  // namespace

extern "C" int rs_features_clean_form(int H, int W) {
  if (H <= 0 || W <= 0) return RS_EINVAL;
  const long plane = (long)H * ((W + 31) / 32) * 4;
  return 2 * plane <= kLdsBytes ? 1 : 2;
}

extern "C" long rs_features_clean_workspace_bytes(int B, int H, int W) {
  if (B <= 0 || H <= 0 || W <= 0) return RS_EINVAL;
  return (long)B * 2 * H * ((W + 31) / 32) * 4;
}

extern "C" int rs_features_clean(const uint8_t* images, uint8_t* out, void* workspace, int B, int H, int W, int index, int eps_open,
                                 const int32_t* dx_open, int eps_close, const int32_t* dx_close, int form, rs_stream_t stream) {
  if (!images || !out || !shape_ok(B, H, W) || index < 0 || index > 255 || form < 0 || form > 2) return RS_EINVAL;
  CleanArgs a;
  if (!make_disc(eps_open, dx_open, &a.open) || !make_disc(eps_close, dx_close, &a.close)) return RS_EINVAL;
  a.images = images;
  a.out = out;
  a.ws = static_cast<uint32_t*>(workspace);
  a.B = B, a.H = H, a.W = W, a.Wd = (W + 31) / 32, a.index = index;
  const int fits = rs_features_clean_form(H, W);
  if (form == 0) form = 2;  // measured at 512 x 512, batch 16: 0.12 ms through HBM on every CU against 1.2 ms on 16 LDS-resident workgroups
  if (form == 1 && fits != 1) return RS_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const long words = (long)H * a.Wd;
  if (form == 1) {
    const int lds = (int)(2 * words * 4);
    if (lds > 64 * 1024) {
      const hipError_t e = hipFuncSetAttribute((const void*)clean_lds_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
      if (e != hipSuccess) return (int)e;
    }
    clean_lds_kernel<<<B, kCleanThreads, lds, s>>>(a);
    return RS_LAUNCH_RESULT();
  }
  if (!workspace) return RS_EINVAL;
  const int chunks = (W + 63) / 64;
  const long items = (long)H * chunks;
  clean_select_kernel<<<dim3(rs_cdiv(items, 4) < 1024 ? rs_cdiv(items, 4) : 1024, B), 256, 0, s>>>(a);
  int from = 0;
  const dim3 grid(rs_cdiv(words, 256), B);
  for (int pass = 0; pass < 4; ++pass) {
    const Disc& d = pass < 2 ? a.open : a.close;
    if (d.eps <= 1) continue;
    if (pass == 0 || pass == 3)
      clean_pass_kernel<true><<<grid, 256, 0, s>>>(a, d, from);
    else
      clean_pass_kernel<false><<<grid, 256, 0, s>>>(a, d, from);
    from ^= 1;
  }
  clean_unpack_kernel<<<dim3(rs_cdiv((long)H * W, 256), B), 256, 0, s>>>(a, from);
  return RS_LAUNCH_RESULT();
}

extern "C" int rs_features_label(const uint8_t* masks, int32_t* labels, int32_t* err, int B, int H, int W, rs_stream_t stream) {
  if (!masks || !labels || !err || !shape_ok(B, H, W)) return RS_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const long P = (long)B * H * W;
  const long items = (long)B * H * ((W + 63) / 64);
  label_init_kernel<<<rs_cdiv(items, 4) < 8192 ? rs_cdiv(items, 4) : 8192, 256, 0, s>>>(masks, labels, B, H, W);
  label_merge_kernel<<<rs_cdiv(P, 256), 256, 0, s>>>(masks, labels, err, B, H, W);
  label_flatten_kernel<<<rs_cdiv(P, 256), 256, 0, s>>>(labels, err, B, H, W);
  return RS_LAUNCH_RESULT();
}

extern "C" int rs_features_components(const int32_t* labels, int32_t* slotmap, int32_t* raw, int32_t* table, int32_t* counters,
                                      long capacity, int B, int H, int W, int min_area, rs_stream_t stream) {
  if (!labels || !slotmap || !counters || capacity < 0 || (capacity > 0 && (!raw || !table)) || !shape_ok(B, H, W)) return RS_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const long P = (long)B * H * W;
  const int grid = rs_cdiv(P, 256);
  const hipError_t e = hipMemsetAsync(counters, 0, 2 * sizeof(int32_t), s);
  if (e != hipSuccess) return (int)e;
  comp_roots_kernel<false><<<grid, 256, 0, s>>>(labels, slotmap, raw, counters, capacity, B, H, W);
  comp_stats_kernel<false><<<grid, 256, 0, s>>>(labels, slotmap, raw, capacity, B, H, W, nullptr);
  comp_filter_kernel<false><<<grid, 256, 0, s>>>(labels, slotmap, raw, table, counters, capacity, B, H, W, min_area);
  return RS_LAUNCH_RESULT();
}

extern "C" int rs_features_edges(const int32_t* labels, const int32_t* table, long rows, uint8_t* keep, int32_t* edges, long capacity,
                                 int32_t* counter, int B, int H, int W, rs_stream_t stream) {
  if (!labels || !keep || !counter || rows < 0 || (rows > 0 && !table) || capacity < 0 || (capacity > 0 && !edges) || !shape_ok(B, H, W))
    return RS_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const long P = (long)B * H * W;
  hipError_t e = hipMemsetAsync(keep, 0, P, s);
  if (e == hipSuccess) e = hipMemsetAsync(counter, 0, sizeof(int32_t), s);
  if (e != hipSuccess) return (int)e;
  if (rows > 0) edges_mark_kernel<false><<<rs_cdiv(rows, 256), 256, 0, s>>>(table, rows, keep, B, (long)H * W);
  edges_emit_kernel<false><<<rs_cdiv(P, 256), 256, 0, s>>>(labels, keep, edges, capacity, reinterpret_cast<unsigned int*>(counter), B, H, W,
                                                            nullptr, nullptr);
  return RS_LAUNCH_RESULT();
}

extern "C" int rs_features_halo(const uint8_t* src, uint8_t* dst, const int32_t* nbr, int T, int H, int W, int A, int fill, int crop,
                                rs_stream_t stream) {
  if (!src || !dst || (!crop && !nbr) || !halo_ok(T, H, W, A) || fill < 0 || fill > 255) return RS_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  if (crop)
    halo_kernel<false><<<rs_cdiv((long)T * H * W, 256), 256, 0, s>>>(src, dst, nbr, T, H, W, A, fill);
  else
    halo_kernel<true><<<rs_cdiv((long)T * (H + 2 * A) * (W + 2 * A), 256), 256, 0, s>>>(src, dst, nbr, T, H, W, A, fill);
  return RS_LAUNCH_RESULT();
}

extern "C" int rs_features_stitch_labels(int32_t* labels, const int32_t* nbr, int32_t* err, int T, int H, int W, rs_stream_t stream) {
  if (!labels || !nbr || !err || !shape_ok(T, H, W)) return RS_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const long P = (long)T * H * W;
  stitch_global_kernel<<<rs_cdiv(P, 256), 256, 0, s>>>(labels, P, (long)H * W);
  stitch_seam_kernel<<<rs_cdiv((long)T * (H + W), 256), 256, 0, s>>>(labels, nbr, err, T, H, W);
  stitch_flatten_kernel<<<rs_cdiv(P, 256), 256, 0, s>>>(labels, err, P);
  return RS_LAUNCH_RESULT();
}

extern "C" int rs_features_components_stitched(const int32_t* labels, const int32_t* origin, int32_t* slotmap, int32_t* raw, int32_t* table,
                                               int32_t* counters, long capacity, int T, int H, int W, int min_area, rs_stream_t stream) {
  if (!labels || !origin || !slotmap || !counters || capacity < 0 || (capacity > 0 && (!raw || !table)) || !shape_ok(T, H, W))
    return RS_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const long P = (long)T * H * W;
  const int grid = rs_cdiv(P, 256);
  const hipError_t e = hipMemsetAsync(counters, 0, 2 * sizeof(int32_t), s);
  if (e != hipSuccess) return (int)e;
  comp_roots_kernel<true><<<grid, 256, 0, s>>>(labels, slotmap, raw, counters, capacity, T, H, W);
  comp_stats_kernel<true><<<grid, 256, 0, s>>>(labels, slotmap, raw, capacity, T, H, W, origin);
  comp_filter_kernel<true><<<grid, 256, 0, s>>>(labels, slotmap, raw, table, counters, capacity, T, H, W, min_area);
  return RS_LAUNCH_RESULT();
}

extern "C" int rs_features_edges_stitched(const int32_t* labels, const int32_t* nbr, const int32_t* origin, const int32_t* table, long rows,
                                          uint8_t* keep, int32_t* edges, long capacity, int32_t* counter, int T, int H, int W,
                                          rs_stream_t stream) {
  if (!labels || !nbr || !origin || !keep || !counter || rows < 0 || (rows > 0 && !table) || capacity < 0 || (capacity > 0 && !edges) ||
      !shape_ok(T, H, W))
    return RS_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const long P = (long)T * H * W;
  hipError_t e = hipMemsetAsync(keep, 0, P, s);
  if (e == hipSuccess) e = hipMemsetAsync(counter, 0, sizeof(int32_t), s);
  if (e != hipSuccess) return (int)e;
  if (rows > 0) edges_mark_kernel<true><<<rs_cdiv(rows, 256), 256, 0, s>>>(table, rows, keep, T, (long)H * W);
  edges_emit_kernel<true><<<rs_cdiv(P, 256), 256, 0, s>>>(labels, keep, edges, capacity, reinterpret_cast<unsigned int*>(counter), T, H, W,
                                                           nbr, origin);
  return RS_LAUNCH_RESULT();
}

extern "C" int rs_features_thin(const uint8_t* masks, uint8_t* out, void* workspace, const int32_t* nbr, int32_t* counters, int B, int H,
                                int W, int pairs, int resume, rs_stream_t stream) {
  if ((!masks && !resume) || !out || !workspace || !counters || !shape_ok(B, H, W) || pairs < 1 || pairs > (1 << 20)) return RS_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  ThinArgs a;
  a.ws = static_cast<uint32_t*>(workspace);
  a.nbr = nbr;
  a.B = B, a.H = H, a.W = W, a.Wd = (W + 31) / 32;
  const long words = (long)H * a.Wd;
  hipError_t e = hipMemsetAsync(counters + 1, 0, sizeof(int32_t), s);
  if (e == hipSuccess && !resume) e = hipMemsetAsync(counters, 0, sizeof(int32_t), s);
  if (e != hipSuccess) return (int)e;
  if (!resume) {
    const long items = (long)H * ((W + 63) / 64);
    thin_pack_kernel<<<dim3(rs_cdiv(items, 4) < 1024 ? rs_cdiv(items, 4) : 1024, B), 256, 0, s>>>(masks, a);
  }
  const dim3 grid(rs_cdiv(words, 256), B);
  for (int pair = 0; pair < pairs; ++pair) {  // (a pair leaves its result where it found its input: plane 0)
    int* last = pair == pairs - 1 ? counters + 1 : nullptr;
    if (nbr) {
      thin_pass_kernel<true, false><<<grid, 256, 0, s>>>(a, 0, counters, last);
      thin_pass_kernel<true, true><<<grid, 256, 0, s>>>(a, 1, counters, last);
    } else {
      thin_pass_kernel<false, false><<<grid, 256, 0, s>>>(a, 0, counters, last);
      thin_pass_kernel<false, true><<<grid, 256, 0, s>>>(a, 1, counters, last);
    }
  }
  CleanArgs u = {};
  u.out = out;
  u.ws = a.ws;
  u.B = B, u.H = H, u.W = W, u.Wd = a.Wd;
  clean_unpack_kernel<<<dim3(rs_cdiv((long)H * W, 256), B), 256, 0, s>>>(u, 0);
  return RS_LAUNCH_RESULT();
}

extern "C" int rs_features_skeleton_links(const uint8_t* skeleton, const int32_t* labels, const int32_t* nbr, const int32_t* origin,
                                          const int32_t* table, long rows, uint8_t* keep, int32_t* links, long capacity, int32_t* counter,
                                          int B, int H, int W, rs_stream_t stream) {
  if (!skeleton || !labels || (nbr == nullptr) != (origin == nullptr) || !keep || !counter || rows < 0 || (rows > 0 && !table) ||
      capacity < 0 || (capacity > 0 && !links) || !shape_ok(B, H, W))
    return RS_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const long P = (long)B * H * W;
  hipError_t e = hipMemsetAsync(keep, 0, P, s);
  if (e == hipSuccess) e = hipMemsetAsync(counter, 0, sizeof(int32_t), s);
  if (e != hipSuccess) return (int)e;
  unsigned int* c = reinterpret_cast<unsigned int*>(counter);
  if (nbr) {
    if (rows > 0) edges_mark_kernel<true><<<rs_cdiv(rows, 256), 256, 0, s>>>(table, rows, keep, B, (long)H * W);
    links_emit_kernel<true><<<rs_cdiv(P, 256), 256, 0, s>>>(skeleton, labels, keep, links, capacity, c, B, H, W, nbr, origin);
  } else {
    if (rows > 0) edges_mark_kernel<false><<<rs_cdiv(rows, 256), 256, 0, s>>>(table, rows, keep, B, (long)H * W);
    links_emit_kernel<false><<<rs_cdiv(P, 256), 256, 0, s>>>(skeleton, labels, keep, links, capacity, c, B, H, W, nullptr, nullptr);
  }
  return RS_LAUNCH_RESULT();
}

extern "C" long rs_features_overlaps_workspace_bytes(long capacity) {
  if (capacity < 0 || capacity > (1l << 29)) return RS_EINVAL;
  return overlap_slots(capacity) * (long)(sizeof(unsigned long long) + sizeof(int32_t));
}

extern "C" int rs_features_overlaps(const int32_t* labels_a, const int32_t* labels_b, void* workspace, int32_t* rows, long capacity,
                                    int32_t* counters, long pixels, long group, rs_stream_t stream) {
  if (!labels_a || !labels_b || !workspace || ((uintptr_t)workspace & 7) || !counters || capacity < 0 || capacity > (1l << 29) ||
      (capacity > 0 && !rows) || pixels <= 0 || pixels >= (1l << 29) || group <= 0 || pixels % group != 0)
    return RS_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const long slots = overlap_slots(capacity);
  unsigned long long* keys = static_cast<unsigned long long*>(workspace);
  int* counts = reinterpret_cast<int*>(keys + slots);
  hipError_t e = hipMemsetAsync(workspace, 0, slots * (sizeof(unsigned long long) + sizeof(int32_t)), s);
  if (e == hipSuccess) e = hipMemsetAsync(counters, 0, 2 * sizeof(int32_t), s);
  if (e != hipSuccess) return (int)e;
  const int vec = (((uintptr_t)labels_a | (uintptr_t)labels_b) & 15) == 0;
  overlaps_count_kernel<<<rs_cdiv(pixels, 256 * kOvRun), 256, 0, s>>>(labels_a, labels_b, keys, counts, counters,
                                                                       (unsigned long long)(slots - 1),
                                                                       (int)(slots < kOvMaxProbe ? slots : kOvMaxProbe), pixels, group, vec);
  overlaps_rows_kernel<<<rs_cdiv(slots, 256 * kOvRowsRun), 256, 0, s>>>(keys, counts, rows, capacity, counters, slots, group);
  return RS_LAUNCH_RESULT();
}

extern "C" int rs_features_scores(const int32_t* labels, const uint8_t* q, const int32_t* table, long rows, int stitched,
                                  int32_t* rowmap, uint64_t* sums, long pixels, long group, int K, rs_stream_t stream) {
  if (!labels || !q || !rowmap || rows < 0 || rows > pixels || (rows > 0 && (!table || !sums || ((uintptr_t)sums & 7))) || pixels <= 0 ||
      pixels >= (1l << 29) || group <= 0 || pixels % group != 0 || K < 1 || K > kScoreMaxK)
    return RS_EINVAL;
  if (rows == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  hipError_t e = hipMemsetAsync(rowmap, 0xff, pixels * sizeof(int32_t), s);
  if (e == hipSuccess) e = hipMemsetAsync(sums, 0, rows * K * sizeof(uint64_t), s);
  if (e != hipSuccess) return (int)e;
  score_rows_kernel<<<rs_cdiv(rows, 256), 256, 0, s>>>(table, rows, stitched ? 6 : 7, rowmap, pixels, group);
  score_sum_kernel<<<rs_cdiv(pixels, 256), 256, 0, s>>>(labels, q, rowmap, reinterpret_cast<unsigned long long*>(sums), pixels, group, K);
  return RS_LAUNCH_RESULT();
}

extern "C" int rs_features_edt(const uint8_t* masks, const int32_t* nbr, uint8_t* g, int32_t* d2, int B, int H, int W, int R,
                               rs_stream_t stream) {
  if (!masks || !g || !d2 || !shape_ok(B, H, W) || R < 1 || R > kEdtMaxR) return RS_EINVAL;
  if (nbr && R > (H < W ? H : W)) return RS_EINVAL;  // (one step in the table must reach every pixel within R)
  hipStream_t s = (hipStream_t)stream;
  const long items = (long)B * H * ((W + 63) / 64);
  const int row_grid = rs_cdiv(items, 4) < 16384 ? rs_cdiv(items, 4) : 16384;
  const dim3 col_grid(rs_cdiv(W, 64), rs_cdiv(H, kEdtRows), B);
  const int lds = (kEdtRows + 2 * R) * 64;
  if (nbr) {
    edt_row_kernel<true><<<row_grid, 256, 0, s>>>(masks, nbr, g, B, H, W, R);
    edt_col_kernel<true><<<col_grid, 256, lds, s>>>(g, nbr, d2, B, H, W, R);
  } else {
    edt_row_kernel<false><<<row_grid, 256, 0, s>>>(masks, nullptr, g, B, H, W, R);
    edt_col_kernel<false><<<col_grid, 256, lds, s>>>(g, nullptr, d2, B, H, W, R);
  }
  return RS_LAUNCH_RESULT();
}

extern "C" int rs_features_split_cores(const int32_t* d2, uint8_t* cores, long pixels, int R, rs_stream_t stream) {
  if (!d2 || !cores || pixels <= 0 || pixels >= (1l << 29) || R < 1 || R > kEdtMaxR) return RS_EINVAL;
  split_cores_kernel<<<rs_cdiv(pixels, 256), 256, 0, (hipStream_t)stream>>>(d2, cores, pixels, R * R);
  return RS_LAUNCH_RESULT();
}

extern "C" int rs_features_split_seeds(const int32_t* labels, const int32_t* seed_labels, uint8_t* has, int32_t* out, long pixels,
                                       long group, rs_stream_t stream) {
  if (!labels || !seed_labels || !has || !out || pixels <= 0 || pixels >= (1l << 29) || group <= 0 || pixels % group != 0) return RS_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const hipError_t e = hipMemsetAsync(has, 0, pixels, s);
  if (e != hipSuccess) return (int)e;
  split_mark_kernel<<<rs_cdiv(pixels, 256), 256, 0, s>>>(labels, seed_labels, has, pixels, group);
  split_start_kernel<<<rs_cdiv(pixels, 256), 256, 0, s>>>(labels, seed_labels, has, out, pixels, group);
  return RS_LAUNCH_RESULT();
}

extern "C" long rs_features_grow_workspace_bytes(int B, int H, int W) {
  if (!shape_ok(B, H, W)) return RS_EINVAL;
  return (long)B * H * W * 4 + 2 * grow_blocks(B, H, W);
}

extern "C" int rs_features_grow_config(int* block_h, int* block_w, int* fused) {
  if (!block_h || !block_w || !fused) return RS_EINVAL;
  *block_h = kGrowH;
  *block_w = kGrowW;
  *fused = grow_fused();
  return 0;
}

extern "C" int rs_features_grow(int32_t* labels, void* workspace, const int32_t* nbr, int32_t* counters, int B, int H, int W, int steps,
                                rs_stream_t stream) {
  if (!labels || !workspace || ((uintptr_t)workspace & 3) || !counters || !shape_ok(B, H, W) || steps < 1 || steps > (1 << 20))
    return RS_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const long P = (long)B * H * W, blocks = grow_blocks(B, H, W);
  int* other = static_cast<int*>(workspace);
  GrowArgs a;
  a.nbr = nbr;
  a.done = reinterpret_cast<uint8_t*>(other + P);
  a.counters = counters;
  a.B = B, a.H = H, a.W = W;
  a.K = grow_fused();
  if (a.K > (H < W ? H : W)) a.K = H < W ? H : W;
  hipError_t e = hipMemsetAsync(counters, 0, 2 * sizeof(int32_t), s);
  if (e == hipSuccess) e = hipMemsetAsync(a.done, 0, 2 * blocks, s);
  if (e != hipSuccess) return (int)e;
  const dim3 grid(rs_cdiv(W, kGrowW), rs_cdiv(H, kGrowH), B);
  const int lds = (kGrowH + 2 * a.K) * (kGrowW + 2 * a.K) * 4;  // at most 24 KB
  int to = 0;
  for (int left = steps; left > 0; left -= a.K) {
    to ^= 1;  // 1: labels -> workspace
    a.src = to ? labels : other;
    a.dst = to ? other : labels;
    a.to = to;
    a.steps = left < a.K ? left : a.K;
    a.last = left <= a.K;
    if (nbr)
      grow_kernel<true><<<grid, 256, lds, s>>>(a);
    else
      grow_kernel<false><<<grid, 256, lds, s>>>(a);
  }
  if (to) {
    e = hipMemcpyAsync(labels, other, P * sizeof(int32_t), hipMemcpyDeviceToDevice, s);
    if (e != hipSuccess) return (int)e;
  }
  return RS_LAUNCH_RESULT();
}
