// The optimiser step of `rs train` (robosat_amd/optim.py): AdamW with the learning-rate schedule, the clipping
// coefficient and the EMA shadow riding in ONE pass over the parameters, and the global gradient norm as one extra read of the gradients.
//
// Both entry points work on a list of ITEMS (rs_optim_item: one parameter tensor's p, g, m, v, optional shadow s, numel, decay flag), a HOST
// array read at call time: gradient addresses change every step (a fresh arena per backward), so the items travel BY VALUE in the launch
// arguments, RS_OPTIM_ITEMS per launch -- no device-side pointer table the host would have to rewrite (and order against the stream),
// no allocation, no synchronisation, every call capturable (under capture the addresses are the graph pool's and never change).
//
// Work split: an item is cut into chunks of RS_OPTIM_CHUNK elements and one 256-thread block walks one chunk: four 16-byte accesses per
// lane and stream (p, g, m, v, s), every wave-instruction 1 KiB contiguous.  The grid is the chunk count of the launch's items; a block
// finds its (item, chunk) by a binary search over the items' first-chunk numbers in the launch arguments (at most 6 scalar loads).
// Purely element-wise: no LDS, no cross-block dependency in the step; the norm writes one fp64 partial per chunk and a single block adds
// them in a fixed order -- no float atomics, the same bits in every run.
//
// Sizes (profiles/optimizer/README.md): 4096 elements per chunk = 16 KiB per stream and block; the U-Net's 37 M parameters are ~9 000
// blocks over 4 launches, and the small tensors (BatchNorm vectors of 64..2048 floats) cost one mostly idle block each, as they would in
// any form that keeps items apart.  48 items: 48 x 56 bytes + 49 + 48 ints = 3.1 KB of the 4 KB a launch may carry.
#include "common.h"

#include <math.h>

// (overridable for A/B builds of the sizes: `make EXTRA=-DRS_OPTIM_CHUNK=8192`)
#ifndef RS_OPTIM_CHUNK
#define RS_OPTIM_CHUNK 4096
#endif
#ifndef RS_OPTIM_ITEMS
#define RS_OPTIM_ITEMS 48
#endif
#define OPT_THREADS 256
#define OPT_VEC_ITERS (RS_OPTIM_CHUNK / (OPT_THREADS * 4))

static_assert(RS_OPTIM_CHUNK % (OPT_THREADS * 4) == 0, "a chunk is a whole number of 16-byte sweeps of the block");

namespace {

// `ctl` as the kernels see it (include/robosat_hip.h: rs_optim_* "state on the device")
struct OptCtl {
  long long step;
  double sumsq;
  float coef;
  float pad;
};

struct OptBlock {
  rs_optim_item it[RS_OPTIM_ITEMS];
  int cbegin[RS_OPTIM_ITEMS + 1];  // first block of item i in this launch; cbegin[cnt] = the grid
  int vec[RS_OPTIM_ITEMS];         // every pointer of the item 16-byte aligned
  int cnt;
  int chunk0;  // (norm) the launch's first chunk in the workspace
};

static_assert(sizeof(OptBlock) <= 3584, "the items travel in the launch arguments (4 KB)");

// item of block b: the last i with cbegin[i] <= b
__device__ __forceinline__ int opt_find(const OptBlock& a, int b) {
  int lo = 0, hi = a.cnt - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (a.cbegin[mid] <= b)
      lo = mid;
    else
      hi = mid - 1;
  }
  return lo;
}

struct OptRow {
  float a, b, c, d;  // lr_t / (1 - beta1^(t+1)),  1 / sqrt(1 - beta2^(t+1)),  1 - lr_t wd,  EMA decay of the step
};

// One element.  Every product and sum is written out (no contraction left to the compiler): the vector and the scalar path, and an item
// alone or in a long list, give the same bits.
//   m' = beta1 m + (1 - beta1) g^          one rounding for the sum (fma), the addend rounded once
//   v' = beta2 v + ((1 - beta2) g^) g^     likewise, the square inside the fma
//   u  = a m' / (sqrt(v') b + eps);  p' = (decay ? c p : p) - u;  s' = d s + (1 - d) p'
#pragma clang fp contract(off)
__device__ __forceinline__ void opt_element(float& p, float g, float& m, float& v, float& s, bool has_s, bool decay, const OptRow r,
                                            float beta1, float omb1, float beta2, float omb2, float eps, float coef, bool use_coef) {
  const float gh = use_coef ? coef * g : g;
  const float m1 = __builtin_fmaf(beta1, m, omb1 * gh);
  const float v1 = __builtin_fmaf(omb2 * gh, gh, beta2 * v);
  const float den = __builtin_sqrtf(v1) * r.b + eps;
  const float u = (r.a * m1) / den;
  const float p1 = (decay ? r.c * p : p) - u;
  m = m1;
  v = v1;
  p = p1;
  if (has_s) s = __builtin_fmaf(r.d, s, (1.0f - r.d) * p1);
}

__global__ __launch_bounds__(OPT_THREADS) void optim_step_kernel(const OptBlock a, const float* __restrict__ table, int T,
                                                                  const OptCtl* __restrict__ ctl, float beta1, float beta2, float eps,
                                                                  int use_coef) {
  const int b = blockIdx.x;
  const int i = opt_find(a, b);
  const rs_optim_item it = a.it[i];
  const long base = (long)(b - a.cbegin[i]) * RS_OPTIM_CHUNK;
  const long left = it.numel - base;
  const int n = left < RS_OPTIM_CHUNK ? (int)left : RS_OPTIM_CHUNK;

  long long t = ctl->step;
  t = t < 0 ? 0 : (t > T - 1 ? T - 1 : t);
  const f32x4 row4 = *reinterpret_cast<const f32x4*>(table + 4 * t);
  const OptRow r = {row4[0], row4[1], row4[2], row4[3]};
  const float coef = use_coef ? ctl->coef : 1.0f;
  const float omb1 = 1.0f - beta1, omb2 = 1.0f - beta2;
  const bool has_s = it.s != nullptr, decay = it.decay != 0, uc = use_coef != 0;

  float* __restrict__ p = it.p + base;
  const float* __restrict__ g = it.g + base;
  float* __restrict__ m = it.m + base;
  float* __restrict__ v = it.v + base;
  float* __restrict__ s = has_s ? it.s + base : nullptr;

  int done = 0;
  if (a.vec[i]) {
    const int nv = n >> 2;  // (base is a multiple of the chunk: the alignment of the item's pointers holds for the chunk's)
#pragma unroll
    for (int k = 0; k < OPT_VEC_ITERS; ++k) {
      const int q = k * OPT_THREADS + threadIdx.x;
      if (q < nv) {
        f32x4 pp = rs_ld4(p + 4 * q), mm = rs_ld4(m + 4 * q), vv = rs_ld4(v + 4 * q);
        const f32x4 gg = rs_ld4(g + 4 * q);
        f32x4 ss = {0.0f, 0.0f, 0.0f, 0.0f};
        if (has_s) ss = rs_ld4(s + 4 * q);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float pe = pp[e], me = mm[e], ve = vv[e], se = ss[e];
          opt_element(pe, gg[e], me, ve, se, has_s, decay, r, beta1, omb1, beta2, omb2, eps, coef, uc);
          pp[e] = pe, mm[e] = me, vv[e] = ve, ss[e] = se;
        }
        rs_st4(p + 4 * q, pp);
        rs_st4(m + 4 * q, mm);
        rs_st4(v + 4 * q, vv);
        if (has_s) rs_st4(s + 4 * q, ss);
      }
    }
    done = nv << 2;
  }
  // the scalar path: items that are only 4-byte aligned, and the <= 3 elements behind the last whole 16 bytes
  for (int q = done + threadIdx.x; q < n; q += OPT_THREADS) {
    float pe = p[q], me = m[q], ve = v[q], se = has_s ? s[q] : 0.0f;
    opt_element(pe, g[q], me, ve, se, has_s, decay, r, beta1, omb1, beta2, omb2, eps, coef, uc);
    p[q] = pe, m[q] = me, v[q] = ve;
    if (has_s) s[q] = se;
  }
}

// stream-ordered behind the element pass of the step: the counter must not move while blocks still read it
__global__ void optim_advance_kernel(OptCtl* ctl) { ctl->step += 1; }

// sum of the 256 threads' values in thread 0, a fixed tree: xor shuffles inside a wave, the four waves in order
__device__ __forceinline__ double opt_block_sum(double x, double* lds) {
  x = rs_wave_sum(x);
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = x;
  rs_lds_writes_done();
  __syncthreads();
  return ((lds[0] + lds[1]) + lds[2]) + lds[3];
}

__global__ __launch_bounds__(OPT_THREADS) void optim_norm_kernel(const OptBlock a, double* __restrict__ partial) {
  __shared__ double lds[OPT_THREADS / 64];
  const int b = blockIdx.x;
  const int i = opt_find(a, b);
  const long base = (long)(b - a.cbegin[i]) * RS_OPTIM_CHUNK;
  const long left = a.it[i].numel - base;
  const int n = left < RS_OPTIM_CHUNK ? (int)left : RS_OPTIM_CHUNK;
  const float* __restrict__ g = a.it[i].g + base;

  double acc = 0.0;
  int done = 0;
  if (a.vec[i]) {
    const int nv = n >> 2;
#pragma unroll
    for (int k = 0; k < OPT_VEC_ITERS; ++k) {
      const int q = k * OPT_THREADS + threadIdx.x;
      if (q < nv) {
        const f32x4 gg = rs_ld4(g + 4 * q);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc += (double)gg[e] * (double)gg[e];
      }
    }
    done = nv << 2;
  }
  for (int q = done + threadIdx.x; q < n; q += OPT_THREADS) acc += (double)g[q] * (double)g[q];
  const double sum = opt_block_sum(acc, lds);
  if (threadIdx.x == 0) partial[(long)a.chunk0 + b] = sum;
}

// one block: thread t adds the partials t, t + 256, ... in ascending order, then the fixed tree
__global__ __launch_bounds__(OPT_THREADS) void optim_norm_finish_kernel(const double* __restrict__ partial, long chunks, float clip,
                                                                         OptCtl* ctl) {
  __shared__ double lds[OPT_THREADS / 64];
  double acc = 0.0;
  for (long q = threadIdx.x; q < chunks; q += OPT_THREADS) acc += partial[q];
  const double sum = opt_block_sum(acc, lds);
  if (threadIdx.x == 0) {
    // torch.nn.utils.clip_grad_norm_(error_if_nonfinite=False): clamp(max_norm / (norm + 1e-6), max=1); a NaN stays a NaN
    const double c = (double)clip / (sqrt(sum) + 1e-6);
    ctl->sumsq = sum;
    ctl->coef = (float)(c > 1.0 ? 1.0 : c);
  }
}

bool opt_aligned(const void* p, uintptr_t mask) { return ((uintptr_t)p & mask) == 0; }

// RS_EINVAL conditions of the items, shared by both entry points (`norm`: only g and numel are read)
bool opt_items_ok(const rs_optim_item* items, int n, bool norm) {
  if (!items || n <= 0) return false;
  for (int i = 0; i < n; ++i) {
    const rs_optim_item& it = items[i];
    if (!it.g || !opt_aligned(it.g, 3) || it.numel <= 0) return false;
    if ((it.numel + RS_OPTIM_CHUNK - 1) / RS_OPTIM_CHUNK > 0x40000000L) return false;
    if (norm) continue;
    if (!it.p || !it.m || !it.v || !opt_aligned(it.p, 3) || !opt_aligned(it.m, 3) || !opt_aligned(it.v, 3) || !opt_aligned(it.s, 3))
      return false;
  }
  return true;
}

// The items in launches of at most RS_OPTIM_ITEMS (and fewer where the grid would pass 2^30 blocks); `launch(block, grid)` per group.
template <typename F>
int opt_for_groups(const rs_optim_item* items, int n, bool norm, F launch) {
  OptBlock a;
  long chunk0 = 0;
  int at = 0;
  while (at < n) {
    int cnt = 0;
    long blocks = 0;
    while (at + cnt < n && cnt < RS_OPTIM_ITEMS) {
      const rs_optim_item& it = items[at + cnt];
      const long c = (it.numel + RS_OPTIM_CHUNK - 1) / RS_OPTIM_CHUNK;
      if (cnt > 0 && blocks + c > 0x40000000L) break;
      a.it[cnt] = it;
      a.cbegin[cnt] = (int)blocks;
      a.vec[cnt] = norm ? opt_aligned(it.g, 15)
                        : opt_aligned(it.p, 15) && opt_aligned(it.g, 15) && opt_aligned(it.m, 15) && opt_aligned(it.v, 15) &&
                              opt_aligned(it.s, 15);
      blocks += c;
      ++cnt;
    }
    for (int i = cnt; i < RS_OPTIM_ITEMS; ++i) {
      a.it[i] = rs_optim_item{nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0, 0};
      a.vec[i] = 0;
    }
    for (int i = cnt; i <= RS_OPTIM_ITEMS; ++i) a.cbegin[i] = (int)blocks;
    a.cnt = cnt;
    if (chunk0 > 0x7fffffffL - blocks) return RS_EINVAL;
    a.chunk0 = (int)chunk0;
    const int rc = launch(a, (int)blocks);
    if (rc) return rc;
    chunk0 += blocks;
    at += cnt;
  }
  return 0;
}

}  // namespace

extern "C" int rs_optim_limits(int* chunk, int* items) {
  if (!chunk || !items) return RS_EINVAL;
  *chunk = RS_OPTIM_CHUNK;
  *items = RS_OPTIM_ITEMS;
  return 0;
}

extern "C" long rs_optim_workspace_bytes(long total_chunks) {
  if (total_chunks <= 0 || total_chunks > 0x7fffffffL) return RS_EINVAL;
  return total_chunks * (long)sizeof(double);
}

extern "C" int rs_optim_grad_norm(const rs_optim_item* items, int n, float clip, void* ctl, void* workspace, rs_stream_t stream) {
  if (!opt_items_ok(items, n, true) || !ctl || !workspace || !opt_aligned(ctl, 7) || !opt_aligned(workspace, 7)) return RS_EINVAL;
  if (!isfinite(clip) || clip < 0.0f) return RS_EINVAL;
  long chunks = 0;
  for (int i = 0; i < n; ++i) chunks += (items[i].numel + RS_OPTIM_CHUNK - 1) / RS_OPTIM_CHUNK;
  if (chunks > 0x7fffffffL) return RS_EINVAL;
  double* partial = static_cast<double*>(workspace);
  const int rc = opt_for_groups(items, n, true, [&](const OptBlock& a, int blocks) {
    optim_norm_kernel<<<blocks, OPT_THREADS, 0, (hipStream_t)stream>>>(a, partial);
    return RS_LAUNCH_RESULT();
  });
  if (rc) return rc;
  optim_norm_finish_kernel<<<1, OPT_THREADS, 0, (hipStream_t)stream>>>(partial, chunks, clip, static_cast<OptCtl*>(ctl));
  return RS_LAUNCH_RESULT();
}

extern "C" int rs_optim_step(const rs_optim_item* items, int n, const float* table, int T, void* ctl, float beta1, float beta2,
                             float eps, int use_coef, rs_stream_t stream) {
  if (!opt_items_ok(items, n, false) || !table || !opt_aligned(table, 15) || T <= 0 || !ctl || !opt_aligned(ctl, 7)) return RS_EINVAL;
  if (!(beta1 >= 0.0f && beta1 < 1.0f) || !(beta2 >= 0.0f && beta2 < 1.0f) || !isfinite(eps) || eps < 0.0f) return RS_EINVAL;
  const OptCtl* c = static_cast<const OptCtl*>(ctl);
  const int rc = opt_for_groups(items, n, false, [&](const OptBlock& a, int blocks) {
    optim_step_kernel<<<blocks, OPT_THREADS, 0, (hipStream_t)stream>>>(a, table, T, c, beta1, beta2, eps, use_coef ? 1 : 0);
    return RS_LAUNCH_RESULT();
  });
  if (rc) return rc;
  optim_advance_kernel<<<1, 1, 0, (hipStream_t)stream>>>(static_cast<OptCtl*>(ctl));
  return RS_LAUNCH_RESULT();
}
