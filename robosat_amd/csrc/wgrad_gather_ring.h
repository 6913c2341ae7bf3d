// wgrad_gather_ring.h -- the HBM -> LDS pipeline the two fp32 Winograd-domain weight gradients share (conv_wgrad_wino_f32.hip,
// conv_wgrad_wino33_f32.hip; DESIGN.md 4, "common skeleton"): a ring of RING stages, each one chunk of NRA rows of the gradient
// (A: BM couts per row) and NRB rows of the source (B: BN cins per row), copied by LDS-DMA (lds_dma.h) through a gather table of
// pixel indices (-1 = a row of zeros), the pieces of chunk c + RING - 1 issued between the MFMAs of chunk c.  The kernel brings
// what is its own: how a chunk's table is filled, how a k-step's fragments are read and what its MFMAs are.  Everything is
// __forceinline__ and leaves no symbol behind.
//
// THE COUNTED WAIT.  rs_dma_wait_n<N> ("all but my N youngest pieces have landed") publishes chunk c + 1 at the barrier that ends
// iteration c while the pieces of chunk c + 2 .. c + RING - 1 are still in flight.  It is sound only if N is what THIS wave issued
// for those RING - 2 chunks.  Instruction ii of a chunk (ii < IA + IB) belongs to wave ii % NW, so wave w issues
//     n(w) = (IA + IB - w + NW - 1) / NW
// pieces per chunk, while the wait below is written with NI = n(0) = ceil((IA + IB) / NW) for every wave.  Where NW does not
// divide IA + IB the higher waves issue n(w) = NI - 1 and their wait leaves (RING - 2) more of chunk c + 1's pieces uncovered
// than it says.  Today that is the case in three of the four instantiations:
//     conv_wgrad_wino_f32<2, 2, 8, 3>   IA + IB = 8 + 18, NW = 4, NI = 7:   waves 2, 3 issue 6
//     conv_wgrad_wino33_f32<2, 2>       IA + IB = 8 + 18, NW = 8, NI = 4:   waves 2 .. 7 issue 3
//     conv_wgrad_wino33_f32<1, 1>       IA + IB = 4 + 9,  NW = 2, NI = 7:   wave 1 issues 6
// (conv_wgrad_wino_f32<1, 2, 8, 3>: 4 + 18 over two waves, 11 each: exact).  ADVICE.md's high finding describes the defect and
// two ways out (wait on n(w), or rebalance so that NW divides IA + IB and assert it, as conv_wgrad_bf16.hip does).  The immediate
// is deliberately left as it was when this header was cut out of the two kernels: the move changes nothing a wave issues or waits
// for, and the fix now has one place to go -- `ring` below.
#pragma once
#include "lds_dma.h"

// BM, BN: channels per A / B row; NRA, NRB: rows per chunk; NW: waves per block; RING: stages.
template <int BM, int BN, int NRA, int NRB, int NW, int RING>
struct WgradGatherRing {
  static constexpr int ROWA = BM * 4, ROWB = BN * 4;          // bytes per LDS row (one pixel)
  static constexpr int PPA = ROWA / 16, PPB = ROWB / 16;      // 16-byte pieces per row
  static constexpr int RIA = 1024 / ROWA, RIB = 1024 / ROWB;  // rows per DMA instruction
  static constexpr int IA = NRA / RIA, IB = NRB / RIB;        // DMA instructions per chunk
  static_assert(IA * RIA == NRA && IB * RIB == NRB, "whole instructions");
  static constexpr int NI = (IA + IB + NW - 1) / NW;  // per wave, rounded up (see the note on the counted wait)
  static constexpr int ABYTES = NRA * ROWA, BBYTES = NRB * ROWB;
  static constexpr int BUF = ABYTES + BBYTES;
  static constexpr int NT = NRA + NRB;  // table entries per chunk: A rows, then B rows
  static_assert(NT <= 64 * NW, "one table entry per thread");
  static constexpr int LDS_BYTES = RING * BUF + RING * NT * 4;  // [RING][BUF] stages, then [RING][NT] tables

  static __device__ __forceinline__ int* tables(unsigned char* smem) { return reinterpret_cast<int*>(smem + RING * BUF); }

  // The DMA role of a wave: instruction ii = wave + NW j; ii < IA copies A rows RIA ii.., else B rows RIB (ii - IA)..
  struct Dma {
    const __amdgpu_buffer_rsrc_t rsrc_a, rsrc_b;
    const int* const tabs;
    const int wave;
    const int ra_a, ra_b;      // this lane's row inside an instruction
    const int cola, colb;      // ... and its byte offset inside a pixel
    const int pixa4, pixb4;    // bytes per pixel of the two tensors
    const unsigned int lds0;
    unsigned int fL;
    int voff[NI];

    // cha, chb: the block's first channel in the two tensors; pixa4, pixb4: their pixel strides in bytes
    __device__ __forceinline__ Dma(__amdgpu_buffer_rsrc_t rsrc_a, __amdgpu_buffer_rsrc_t rsrc_b, unsigned char* smem, int wave, int lane,
                                   int pixa4, int pixb4, int cha, int chb)
        : rsrc_a(rsrc_a), rsrc_b(rsrc_b), tabs(tables(smem)), wave(wave), ra_a(lane / PPA), ra_b(lane / PPB),
          cola((cha + lane % PPA * 4) * 4), colb((chb + lane % PPB * 4) * 4), pixa4(pixa4), pixb4(pixb4),
          lds0(__builtin_amdgcn_readfirstlane(rs_lds_addr(smem))), fL(lds0) {}

    // table `which` -> this lane's byte offsets of the chunk that goes to stage `buf` (-1 stays -1: out of range, zeros)
    __device__ __forceinline__ void prepare(int buf, int which) {
      fL = lds0 + buf * BUF;
#pragma unroll
      for (int j = 0; j < NI; ++j) {
        const int ii = wave + NW * j;  // wave-uniform
        if (ii < IA) {
          const int pix = tabs[which * NT + RIA * ii + ra_a];
          voff[j] = pix >= 0 ? pix * pixa4 + cola : -1;
        } else if (ii < IA + IB) {
          const int pix = tabs[which * NT + NRA + RIB * (ii - IA) + ra_b];
          voff[j] = pix >= 0 ? pix * pixb4 + colb : -1;
        }
      }
    }
    __device__ __forceinline__ void issue(int j) const {
      const int ii = wave + NW * j;
#if defined(RS_WW_KO) && (RS_WW_KO & 1)
      return;  // (knock-out build: no DMA in the steady state -- wrong results by construction)
#endif
      if (ii < IA) rs_dma16(rsrc_a, fL + ii * 1024, voff[j]);
      else if (ii < IA + IB) rs_dma16(rsrc_b, fL + ABYTES + (ii - IA) * 1024, voff[j]);
    }
  };

  // One chunk out of stage L: NS k-steps of MPS MFMAs each, fragment s + 1 read ahead of k-step s.  kstep(frag, issue, s) calls
  // issue(q) in front of its MFMA q = s MPS + x; with `fetch` that places the wave's pieces front-loaded, every PSTEP MFMAs over
  // the chunk's first half, so that the chunk's tail covers their latency.
  template <int NS, int MPS, class Frag, class ReadFrag, class Kstep>
  static __device__ __forceinline__ void chunk_mma(const Dma& dma, const unsigned char* L, bool fetch, const ReadFrag& read_frag,
                                                   const Kstep& kstep) {
    constexpr int NMMA = NS * MPS;
    constexpr int PSTEP = NMMA / (2 * NI) >= 1 ? NMMA / (2 * NI) : 1;
    Frag f[2];
    read_frag(L, 0, f[0]);
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      if (s + 1 < NS) read_frag(L, s + 1, f[(s + 1) & 1]);
      kstep(f[s & 1], [&](int q) __attribute__((always_inline)) {
        if (fetch && q % PSTEP == 0 && q / PSTEP < NI) dma.issue(q / PSTEP);
      }, s);
    }
    if (fetch) {
#pragma unroll
      for (int q = (NMMA + PSTEP - 1) / PSTEP; q < NI; ++q) dma.issue(q);
    }
  }

  // Chunks [chunk0, chunk1) of a block.  fill_table(chunk, which) writes table `which` (every thread calls it; chunks past the
  // end give -1 rows) and ends in rs_lds_writes_done().
  // Chunk c lives in stage / table (c - chunk0) % RING.  Iteration c runs chunk c's MFMAs with the pieces of chunk c + RING - 1
  // issued between them (into the stage chunk c - 1 left at the last barrier), writes the table of chunk c + RING (over chunk c's,
  // read RING - 1 barriers ago) and waits for chunk c + 1's pieces: all but this wave's (RING - 2) NI youngest.
  template <int NS, int MPS, class Frag, class FillTable, class ReadFrag, class Kstep>
  static __device__ __forceinline__ void ring(Dma& dma, const unsigned char* smem, int chunk0, int chunk1, const FillTable& fill_table,
                                              const ReadFrag& read_frag, const Kstep& kstep) {
    if (chunk0 >= chunk1) return;
#pragma unroll
    for (int r = 0; r < RING; ++r) fill_table(chunk0 + r, r);
    __syncthreads();
#pragma unroll
    for (int r = 0; r < RING - 1; ++r) {
      if (chunk0 + r < chunk1) {
        dma.prepare(r, r);
#pragma unroll
        for (int q = 0; q < NI; ++q) dma.issue(q);
      }
    }
    rs_dma_wait();
    __syncthreads();
    int st = 0;  // (c - chunk0) % RING
    for (int c = chunk0; c < chunk1; ++c) {
      const int stf = st == 0 ? RING - 1 : st - 1;  // stage / table of chunk c + RING - 1
      const bool fetch = c + RING - 1 < chunk1;     // (block-uniform)
      if (fetch) dma.prepare(stf, stf);
      chunk_mma<NS, MPS, Frag>(dma, smem + st * BUF, fetch, read_frag, kstep);
      if (fetch) {
        fill_table(c + RING, st);
        rs_dma_wait_n<(RING - 2) * NI>();
      } else {
        rs_dma_wait();
      }
      __syncthreads();
      st = st == RING - 1 ? 0 : st + 1;
    }
  }
};

// NX accumulators of v_mfma_f32_32x32x2_f32 -> out[x][co][ci] (planes of Cout x Cin).  D[i][j]: i = cout (tile-local) =
// (r & 3) + 8 (r >> 2) + 4 (lane >> 5), j = cin (tile-local) = lane & 31; co, ci: the wave's sub-tile origin.
template <int NX>
__device__ __forceinline__ void rs_wgrad_store_acc(float* out, const f32x16 (&acc)[NX], int Cout, int Cin, int co, int ci, int lane) {
  ci += lane & 31;
#pragma unroll
  for (int x = 0; x < NX; ++x)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int c = co + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
      out[((long)x * Cout + c) * Cin + ci] = acc[x][r];
    }
}
