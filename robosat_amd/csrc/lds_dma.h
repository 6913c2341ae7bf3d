// lds_dma.h -- the HBM -> LDS primitives every fast convolution kernel of the library is built from ("common
// skeleton"): a buffer descriptor, one LDS-DMA wave instruction, the waits for it, the LDS byte address of a pointer and
// the transposing LDS read of the bf16 weight gradients.  The only place in csrc/ where they are defined.  Everything is
// __forceinline__ and leaves no symbol behind.
#pragma once
#include "common.h"

// ---- buffer descriptors ---------------------------------------------------------------------------------------------
// `bytes` from `base` on are addressable; a lane offset at or beyond that is out of range (loads return zeros, LDS-DMA
// writes zeros).  CLAMP caps num_records: a kernel that marks padding / past-the-end rows with a sentinel offset picks a
// clamp BELOW its sentinel, so that the sentinel is out of range for every descriptor it builds, and says so in a
// static_assert next to the sentinel.
//
// rs_dma_rsrc: the form for descriptors that feed rs_dma16.  The inputs are wave-uniform (kernel arguments and blockIdx
// arithmetic) but 64-bit multiplies, integer divisions and the clamp run on the VALU: hipcc then carries the descriptor in
// VGPRs and only sometimes moves it back (it did not once a select between two descriptors was itself lowered to
// v_cndmask: "invalid operand" in the LDS-DMA asm, whose SRSRC must be SGPRs).  readfirstlane on the descriptor's INPUTS
// makes the uniformity provable (cdna_hip_programming.md T20).
template <unsigned int CLAMP>
__device__ __forceinline__ __amdgpu_buffer_rsrc_t rs_dma_rsrc(const void* base, long bytes) {
  const unsigned int n = bytes > (long)CLAMP ? CLAMP : (unsigned int)(bytes < 0 ? 0 : bytes);
  const unsigned long b = (unsigned long)base;
  const unsigned int lo = __builtin_amdgcn_readfirstlane((unsigned int)b), hi = __builtin_amdgcn_readfirstlane((unsigned int)(b >> 32));
  const unsigned int nn = __builtin_amdgcn_readfirstlane(n);
  return __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<void*>(((unsigned long)hi << 32) | lo), 0, (int)nn, 0x00020000);
}
// rs_buf_rsrc: the plain form, for kernels where hipcc proves the uniformity itself.  The two forms are NOT interchangeable
// for free: the readfirstlanes change the register allocation of the whole kernel.
template <unsigned int CLAMP>
__device__ __forceinline__ __amdgpu_buffer_rsrc_t rs_buf_rsrc(const void* base, long bytes) {
  const unsigned int n = bytes > (long)CLAMP ? CLAMP : (unsigned int)(bytes < 0 ? 0 : bytes);
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, (int)n, 0x00020000);
}

// ---- one LDS-DMA wave instruction (buffer_load_dwordx4 ... lds) ------------------------------------------------------
// Lane l's 16 bytes at buffer offset `voff` (+ `soff`) land at LDS byte `lds_dst` + 16*l (lds_dst wave-uniform, in M0); an
// out-of-range offset => zeros (scripts/probes/probe_glds.hip).
// Inline asm on purpose: through the builtin hipcc cannot tell that the DMA's destination (the OTHER pipeline buffer) is
// disjoint from the fragment reads that follow and drains the queue (s_waitcnt vmcnt(0)) before the first ds_read of
// every chunk, serialising copy and MFMA.  As asm the copy is invisible to its counters, so the kernel waits itself
// (rs_dma_wait / rs_dma_wait_n) ahead of the barrier that publishes the buffer.
// `soff` is a wave-uniform byte offset added to the address (the SOFFSET operand): the per-lane offsets of a
// (tap, source) stay in registers and the K loop advances through the channels with one SGPR.
// m0 is declared clobbered rather than saved and restored (two SALU per piece, eight pieces per chunk per wave): the
// compiler itself only touches m0 for M0-operand LDS builtins and dynamically indexed register arrays, and no kernel that
// calls rs_dma16 may have either (every register array of theirs is indexed by unrolled constants) -- check `grep m0`
// of the ISA after touching such a kernel.  hipcc warns that m0 is a reserved register: those objects are built
// with -Wno-inline-asm (Makefile).
__device__ __forceinline__ void rs_dma16(__amdgpu_buffer_rsrc_t r, unsigned int lds_dst, int voff) {
  asm volatile(
      "s_mov_b32 m0, %1\n\t"
      "s_nop 0\n\t"
      "buffer_load_dwordx4 %0, %2, 0 offen lds"
      :
      : "v"(voff), "s"(lds_dst), "s"(r)
      : "memory", "m0");
}
__device__ __forceinline__ void rs_dma16(__amdgpu_buffer_rsrc_t r, unsigned int lds_dst, int voff, int soff) {
  asm volatile(
      "s_mov_b32 m0, %1\n\t"
      "s_nop 0\n\t"
      "buffer_load_dwordx4 %0, %2, %3 offen lds"
      :
      : "v"(voff), "s"(lds_dst), "s"(r), "s"(soff)
      : "memory", "m0");
}

// ---- waits ----------------------------------------------------------------------------------------------------------
// every vector-memory operation of this wave, its LDS-DMA pieces among them, has completed
__device__ __forceinline__ void rs_dma_wait() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
// ... all but the N youngest.  Sound as "the older pieces have landed" because LDS-DMA pieces retire IN ORDER whatever
// their lanes address, out of range included (scripts/probes/probe_dma_order.hip, profiles/r06/dma_order.txt)
// -- and only if every wave issues the same count of pieces between two such waits.
template <int N>
__device__ __forceinline__ void rs_dma_wait_n() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// ---- LDS addressing -------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned int rs_lds_addr(const void* p) {
  return (unsigned int)(unsigned long)(__attribute__((address_space(3))) const void*)p;
}

// two ds_read_b64_tr_b16 = one bf16 MFMA operand fragment, transposed by the hardware on the way out of the LDS
__device__ __forceinline__ bf16x8 rs_tr_read8(const unsigned char* p0, const unsigned char* p1) {
  typedef __attribute__((address_space(3))) s16x4* lds_ptr;
  const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_ptr)p0);
  const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_ptr)p1);
  s16x8 v;
  v[0] = lo[0];
  v[1] = lo[1];
  v[2] = lo[2];
  v[3] = lo[3];
  v[4] = hi[0];
  v[5] = hi[1];
  v[6] = hi[2];
  v[7] = hi[3];
  return __builtin_bit_cast(bf16x8, v);
}
