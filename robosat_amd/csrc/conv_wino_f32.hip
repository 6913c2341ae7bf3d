// conv_wino_f32.hip -- DecoderBlock (reference robosat/unet.py:63-73: conv3x3(pad 1) over a nearest-x2 upsample of
// cat[skip, prev]) in fp32 as a WINOGRAD F(2x2, 2x2) convolution on the phase form.
//
// The phase form (conv_igemm_dma_kernel.h, PHASE = true) already turns the 3x3 convolution over the upsampled tensor into
// four 2x2 convolutions on the SOURCE grid, one per output parity (py, px), with pre-summed taps: 16 multiply-adds per source
// pixel, channel and cout instead of 36.  A 2x2 correlation producing a 2x2 block of outputs from a 3x3 block of inputs
// needs only 9 multiplies with the minimal-filtering transforms (all coefficients are 0 / +-1, so nothing is lost in fp32):
//     Y = A^T [ (G g G^T) (.) (B^T d B) ] A,   B^T = [1 -1 0; 0 1 0; 0 -1 1],  G = [1 0; 1 1; 0 1],  A^T = [1 1 0; 0 1 1]
// i.e. 9 GEMMs [tiles x Cin] . [Cin x Cout] per parity instead of 16: 9/16 of the phase form's MFMA work, 1/4 of the
// reference-shape count.  That trade only pays where the matrix cores are the bottleneck and the vector ALU / LDS have
// slack: exactly the fp32 path (v_mfma_f32_32x32x2_f32: 157 TFLOP/s, 64 cycles per instruction per SIMD), where the four
// generic phase layers are 48 % of a predict pass at 0.87-0.91 of the MFMA peak.  In bf16 the same layers are bound by the
// LDS-DMA stream, not by MFMA, and the transform would only add bytes: bf16 keeps the phase form.
//
// Mapping.  GEMM rows = TILES (2x2 blocks of source positions -> 4x4 output pixels over the four parities; each parity is
// its own set of work items), columns = couts, K = input channels of cat[skip, prev] in 16-channel chunks (64-byte rows).
//   block  = 8 waves, persistent: one block per CU walks work items (16*TG tiles x 32*CG couts x parity; TG x CG = 4 x 2, or
//            8 x 1 for the 32-cout layer).  A wave owns 16 tiles x 32 couts and keeps 9 x 2 accumulators of
//            v_mfma_f32_16x16x4_f32 (one pair per transformed position xi): 72 registers, two waves per SIMD -- while one
//            wave reads its patch and runs the transform's vector ops, the other's MFMAs keep the matrix core busy.
//   LDS    = per K-chunk the block's source HALO -- every source pixel any of its tiles touches, once: (2 PB + 1)^2 pixels
//            per PB x PB patch of tiles, 64 bytes each -- plus the transformed filters U[xi][cout][16 ch], both by LDS-DMA
//            (buffer_load ... lds; out-of-image pixels arrive as zeros), double buffered, one barrier per chunk.  A source
//            pixel is fetched ONCE per block and chunk (the generic phase kernel fetches it once per tap: 4x).  The fetch side
//            runs one chunk ahead ACROSS work items: the next item's first chunk streams in while this item's outputs are
//            stored (its halo table is built an item ahead, double buffered).
//   reads  = each lane reads the 3x3 patch of its tile (9 ds_read_b128: 4 channels of each of the 9 pixels), forms B^T d B
//            with 12 vector subtractions, reads the filter pieces one position ahead of their use (sched_barrier keeps hipcc
//            from sinking them in front of every MFMA group) and issues 72 MFMAs per chunk.  Halo rows are stored
//            even-x-first, sub-blocks padded to 8 rows, pieces XOR-swizzled with (row ^ row >> 1) & 3, lanes mapped to tiles
//            by a bit permutation: found by exhaustive search against ds_read_b128's four 16-lane groups, all 27 reads per
//            chunk are bank-conflict free (scripts/probes/wino_lds.py re-derives and checks it; SQ_LDS_BANK_CONFLICT = 0).
//   store  = A^T M A on the accumulators (3 adds per output element), ReLU, 16-byte stores straight from registers: a lane
//            holds 4 consecutive couts of its tile's pixels; no LDS staging, nothing to wait for.
//
// Two arrangements of the same arithmetic.  The TILE form above (the data gradient, the p4 blocks, rs_conv2d_fwd_phase_wino -- any
// phase pack's filters --, and rs_conv2d_fwd_upsampled_wino behind ROBOSAT_WINO_PIXEL=0) makes every parity its own work item: the four items of an m block run on four CUs, each fetches the same
// source region shifted by one pixel, each carries a (2 * 8 + 1)^2 = 289-pixel halo per 64 rows.  The PIXEL form (PIX = true: the p8
// forward blocks of rs_conv2d_fwd_upsampled_wino, whose filters are ONE 3x3 filter's) arranges it on source pixels.  In one dimension, taps w0 w1 w2 over the x2-nearest upsample, x[-1] = x[W] = 0:
//     out[2i] = w0 (x[i-1] - x[i]) + (w0+w1+w2) x[i],     out[2i+1] = (w0+w1+w2) x[i] + w2 (x[i+1] - x[i])
// so per source pixel the 3x3 patch AROUND it, through the same input transform [d0 - d1, d1, d2 - d1] along each axis, times nine
// filters gives all four parity outputs of the pixel: the same 2.25 multiplies per output, the same output transform with (u, v) the
// output PARITY instead of the pixel inside the tile, stored to (2y + u, 2x + v).  The nine filters are already in the pack:
// position (r, c) is slab [2 (r == 2) + (c == 2)][3r + c] of U [4][9][Cout][Cin] (G g G^T of parity 0 is [w0, w0+w1+w2, ..] along an
// axis, of parity 1 [.., w0+w1+w2, w2]).
//   rows   = source pixels; a sub-block is an 8 x 8 patch of pixels with a 10 x 10 halo at origin (8 bby - 1, 8 bbx - 1), a wave's 16
//            rows one 4 x 4 block of it; items are (m block, cout block), nsub = N ceil(Hs / 8) ceil(Ws / 8); pixels past Hs / Ws of a
//            ragged patch are masked per pixel in the epilogue.
//   LDS    = halo lines in x order at pitch 10 (100 rows, padded to 104 per sub-block), the same swizzle, lane l -> pixel (l & 3,
//            l >> 2): all nine unit-stride patch reads conflict free (scripts/probes/wino_lds.py --search).  Filter rows as above.
//   DMA    = rows per 16-channel chunk, halo + filters: 128 x 64 block 592 + 576 -> 208 + 576 (-33 %), 128 x 32 592 + 288 -> 208 + 288
//            (-44 %), 64 x 64 296 + 576 -> 112 + 576 (-21 %: seven 16-row pieces over 104 rows); halo pieces per wave 5 -> 2, gather-table rows per thread 2 -> 1, LDS per
//            block 158 -> 104 KB; a launch reads 9 of the 36 filter slabs, and a source pixel's halo is fetched by one CU, not four.
//   One descriptor spans the four filter sets (4 * 9 * Cout * Cin * 4 bytes < 2^31: wino_plan); a filter piece's 16 rows lie in one
//   position, so the position's slab is one scalar offset per piece of the wave, formed once per block.
// MFMA count and order, accumulators, fragment reads and transform VALU per MFMA are the tile form's; outputs differ from it in fp32
// summation order (both within 2e-5 of float64: tests/test_gpu_wino_pixel.py, tests/test_wino_pixel_cpu.py).  Measured
// (profiles/wino_pixel): dec1 711 -> 694, dec2 434 -> 423, dec3 1 481 -> 1 437, dec4 690 -> 661 us per launch, dec0 340 -> 338.
// Weights: rs_pack_wino_phase_weight turns the phase pack [4][Cout][2][2][Cin] into U = G g G^T, [4][9][Cout][Cin].
// Which layers: decided on the layer's GEOMETRY alone (>= 8 tiles per image side), never on the batch size -- the two forms
// differ in fp32 summation order, and a tile's probabilities must not depend on the batch it travels in.
//
// Measured (MI355X, bs 16 at 512^2, scripts/bench_wino.py; generic phase kernel -> this kernel): dec0 0.68 -> 0.40 ms, dec1
// 1.24 -> 0.79, dec2 0.76 -> 0.48, dec3 2.39 -> 1.68, dec4 1.21 -> 0.79: 1.43-1.7x for 9/16 of the MFMA work, i.e. the matrix
// cores are 72-78 % busy here against 90 % in the generic kernel (SQ_VALU_MFMA_BUSY_CYCLES, profiles/r03).  What the rest is:
// the CU's LDS-DMA path (~23 B/clk) carries 12 B/clk here -- 55 KB per chunk, two thirds of it filters -- and the waves that
// issue those pieces stall on it in phase with each other (one barrier per chunk).  Variants measured on the way
// (profiles/r03/wino_variants.txt): 32x32x2 MFMAs with 144 accumulator registers at one wave per SIMD (104 TFLOP/s executed
// on dec3), the same with two dedicated DMA-producer waves and persistent blocks (101), with wave pairs splitting each
// chunk's channels and an LDS reduction at the end (110), this one (116); front-loading the DMA pieces: no change.
#define RS_CONV_INSTANTIATE  // (for kDmaOOB / kDmaClamp and the small helpers of the header; no kernel of it is instantiated here)
#include "conv_igemm_dma_kernel.h"

namespace {

struct WinoArgs {
  const float* src1;
  const float* src2;
  const float* u;  // [4][9][Cout][C1 + C2]
  float* out;      // [N][2 Hs][2 Ws][Cout]
  int N, Hs, Ws, C1, C2, Cout;
  int TY, TX;    // tiles per image: ceil(Hs / 2), ceil(Ws / 2)
  int BBY, BBX;  // PB x PB tile patches ("sub-blocks") per image
  int nsub;      // N * BBY * BBX
  int ncb;       // cout blocks: Cout / BN
  int relu;
  // DG instantiations only -- the DecoderBlock's DATA gradient (autograd of unet.py:63-73 under tools/train.py:186): `src1` is dz
  // [N][2 Hs][2 Ws][C1] (C2 = 0), `u` the transformed data-gradient filters [4][9][Cout][C1] (rs_pack_wino_dgrad_weight), the output
  // d cat[skip, prev] at SOURCE resolution [N][Hs][Ws][Cout], optionally split at cout `csplit` into out / out2 (torch.cat's backward
  // fused into the store) with a ReLU mask each (the tensor whose sign decides: the forward activation; null = none)
  float* out2;
  const float* mask1;
  const float* mask2;
  int csplit;
};

template <int PB, bool PIX = false>
struct WinoGeom {
  // halo width of a sub-block: a PB x PB patch of tiles (2 PB + 1), or, pixel form, an 8 x 8 patch of source pixels (10)
  static constexpr int HW = PIX ? 10 : 2 * PB + 1;
  static constexpr int PITCH = HW;     // LDS rows per halo line
  static constexpr int HALF = PB + 1;  // tile form: even x first, then odd x (the pixel form stores a line in x order)
  // rows per sub-block, padded to a multiple of 8: the swizzle reads row bits 0..2, so every sub-block sees the pattern the
  // conflict-free search was run on
  static constexpr int SBROWS = (HW * PITCH + 7) / 8 * 8;
};

// lane (0..15) -> tile of the wave's 16: the bit permutation that belongs to the conflict-free LDS layout (found by exhaustive
// search over pitch / row order / swizzle / permutation against ds_read_b128's four 16-lane groups; scripts/probes/wino_lds.py)
template <int PB>
__device__ __forceinline__ int wino_lane_tile(int l) {
  if constexpr (PB == 8) return ((l & 1) << 1) | (((l >> 1) & 1) << 2) | ((l >> 2) & 1) | (l & 8);
  return ((l & 1) << 1) | (((l >> 1) & 1) << 3) | ((l >> 2) & 1) | (((l >> 3) & 1) << 2);
}
// pixel form: lane (0..15) -> pixel (ly, lx) of the wave's 4 x 4 block.  With halo lines in x order at pitch 10 and the same
// swizzle, this transposed order makes all nine patch reads conflict free (scripts/probes/wino_lds.py searches and checks it).
__device__ __forceinline__ int wino_lane_pixel_y(int l) { return l & 3; }
__device__ __forceinline__ int wino_lane_pixel_x(int l) { return (l >> 2) & 3; }
typedef float f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f32x2 pk_sub(f32x2 a, f32x2 b) {  // a - b on two floats: v_pk_add_f32 with the second operand negated
  f32x2 d;
  asm("v_pk_add_f32 %0, %1, %2 neg_lo:[0,1] neg_hi:[0,1]" : "=v"(d) : "v"(a), "v"(b));
  return d;
}
// the lane index computed where it is used (volatile: not hoisted out of the item loop).  Carried from the kernel's entry across the
// MFMA loops, the thread index behind the gather table's addresses cost the 128 x 64 block a scratch slot and a reload per item.
__device__ __forceinline__ int wino_lane_now() {
  int l;
  asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
  return l;
}
__device__ __forceinline__ int wino_swz(int row) { return (row ^ (row >> 1)) & 3; }  // 16-byte piece c of a row is stored at c ^ swz(row)

// TG tile groups (16 tiles each) x CG cout groups (32 couts each) = 8 waves per block
// NM = MFMA tiles of 16 couts per wave (a wave owns 16 tiles x 16*NM couts)
// DG (round 6): the 4x4 / stride-2 data gradient of the phase form in the same machinery.  d src(a, b) = sum over the four parity
// planes of dz, plane(pa, pb)(u, v) = dz(2 u + pa, 2 v + pb), of a 2x2 correlation with taps w4[2 r + 1 - pa][2 s + 1 - pb] at origin
// (a - pa, b - pb): exactly the forward's parity (py, px) = (1 - pa, 1 - pb) item on that plane -- same halo origin, same 3x3 patches,
// same transforms -- except that the four parities ACCUMULATE into one output tile instead of interleaving into four.  So a block
// owns an output item for four consecutive "units" (one per plane: its own halo table, source offsets and filter set, as for a
// forward item), keeps the accumulators across them and writes A^T M A once: 9/16 of the generic 4x4 kernel's multiply-adds.
// PIX: the forward's pixel form -- GEMM rows are SOURCE PIXELS, all four parities of a pixel from one 3x3 patch around it (see the
// header).  Same pipeline, same transforms and MFMA order; a sub-block is an 8 x 8 patch of pixels, an item has no parity.
template <int PB, int TG, int CG, int NM = 2, bool DG = false, bool PIX = false>
__global__ __launch_bounds__(512, 1) void conv_wino_f32_kernel(const WinoArgs p) {
  using G = WinoGeom<PB, PIX>;
  constexpr int NW = TG * CG;
  static_assert(NW == 8, "8 waves");
  static_assert(!PIX || (PB == 8 && !DG), "the pixel form: forward, 64-row sub-blocks");
  constexpr bool PAR = !DG && !PIX;  // the output parity is part of the item index
  constexpr int BMT = 16 * TG, BN = 16 * NM * CG;
  constexpr int SB = BMT / (PB * PB);
  static_assert(SB * PB * PB == BMT, "whole sub-blocks per block");
  constexpr int AROWS = SB * G::SBROWS;
  constexpr int IA = (AROWS + 15) / 16, IB = 9 * BN / 16;
  constexpr int AROWS_PAD = IA * 16;
  constexpr int JA = (IA + NW - 1) / NW, JB = (IB + NW - 1) / NW;  // halo / filter pieces per wave and chunk (the last of either: some waves)
  constexpr int NI = JA + JB;                                     // DMA instructions per wave and chunk
  constexpr int STAGE = (AROWS_PAD + 9 * BN) * 64;
  constexpr int KC = 16;  // channels per chunk (64-byte rows)

  constexpr int NTR = (AROWS_PAD + 64 * NW - 1) / (64 * NW);  // gather-table rows per thread
  __shared__ __attribute__((aligned(16))) unsigned char smem[2 * STAGE + 2 * AROWS_PAD * 4 + NTR * 64 * NW * 4];
  int* tabs = reinterpret_cast<int*>(smem + 2 * STAGE);  // [2][AROWS_PAD]: halo row -> source pixel relative to the item's first image, -1 = zeros

  int* trows = tabs + 2 * AROWS_PAD;                     // [NTR][512]: what a thread knows about its table rows, see build_table
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int tg = wave % TG, cg = wave / TG;
  const int per_img = p.BBY * p.BBX;
  const int Cin = p.C1 + p.C2;
  const int nk = Cin / KC;
  const int ntiles = ((p.nsub + SB - 1) / SB) * p.ncb * (PAR ? 4 : 1);  // work items: (m block, cout block[, parity]); DG: output items
  const int first = rs_xcd_remap(blockIdx.x, gridDim.x);
  // this block walks items first, first + grid, ...; DG: each output item as four consecutive units (the parity planes of dz)
  const int nitems = (ntiles - first + (int)gridDim.x - 1) / (int)gridDim.x * (DG ? 4 : 1);
  const unsigned int lds0 = __builtin_amdgcn_readfirstlane(rs_lds_addr(smem));
  const long img1 = (long)p.Hs * p.Ws * p.C1 * (DG ? 4 : 1), img2 = (long)p.Hs * p.Ws * p.C2;  // (DG: dz images are 2 Hs x 2 Ws)

  // ---- an item, decoded once: wave-uniform, kept in scalar registers -------------------------------------------------------------
  // The block's items advance by gridDim.x: parity, and quotient and remainder of the rest by ncb, are carried from item to item, so
  // the item index is never divided.  Sub-block sb of the item: image n[sb], parity-less halo origin (y0, x0) = (2 PB bby - 1,
  // 2 PB bbx - 1); the sub-blocks of an item follow each other in (n, bby, bbx) order and may lie in different images.  The table
  // builder and the fetch side run one item ahead (`nxt`), the epilogue reads the item in the accumulators (`cur`).  The p4 blocks
  // (4 / 8 sub-blocks of 16 tiles: the small layers, none of them in the benchmark) keep only the first sub-block's index and divide
  // per sub-block where they need one -- that many scalars would live in memory.
  constexpr int SBS = SB <= 2 ? SB : 1;
  struct Item {
    int py, px, nblk, nfirst, sub0;
    int n[SBS], y0[SBS], x0[SBS];
    bool live[SBS];
  };
  const int uni_first = __builtin_amdgcn_readfirstlane(first), uni_grid = __builtin_amdgcn_readfirstlane((int)gridDim.x);
  // forward: item = 4 rest + parity, + gridDim.x per item; DG: rest = the output item, + gridDim.x once its four planes are through
  // pixel form: item = rest, + gridDim.x per item, no parity and no carry
  const int d_step = PAR ? uni_grid >> 2 : uni_grid, d_parstep = DG ? 1 : uni_grid & 3;
  int d_par = PAR ? uni_first & 3 : 0;
  int d_mblk = (PAR ? uni_first >> 2 : uni_first) / p.ncb, d_nblk = (PAR ? uni_first >> 2 : uni_first) - d_mblk * p.ncb;
  const int dq = d_step / p.ncb, dr = d_step - dq * p.ncb;
  auto decode_next = [&](Item& s) __attribute__((always_inline)) {
    s.py = PIX ? 0 : d_par >> 1;
    s.px = PIX ? 0 : d_par & 1;
    if (!DG || d_par == 0) {  // (DG: the four units of an output item share everything but the plane)
      s.nblk = d_nblk;
      const int sub0 = s.sub0 = d_mblk * SB;
      int n = __builtin_amdgcn_readfirstlane(sub0 / per_img);
      const int r2 = sub0 - n * per_img;
      int bby = __builtin_amdgcn_readfirstlane(r2 / p.BBX);
      int bbx = r2 - bby * p.BBX;
      s.nfirst = n;
#pragma unroll
      for (int sb = 0; sb < SBS; ++sb) {
        s.live[sb] = sub0 + sb < p.nsub;
        s.n[sb] = n;
        s.y0[sb] = (PIX ? 8 : 2 * PB) * bby - 1;
        s.x0[sb] = (PIX ? 8 : 2 * PB) * bbx - 1;
        if (++bbx == p.BBX) {
          bbx = 0;
          if (++bby == p.BBY) {
            bby = 0;
            ++n;
          }
        }
      }
    }
    int carry = 0;
    if constexpr (!PIX) {
      d_par += d_parstep;
      carry = d_par >> 2;
      d_par &= 3;
    }
    if (!DG || carry) {
      d_mblk += dq;
      d_nblk += dr + (PAR ? carry : 0);
      if (d_nblk >= p.ncb) {
        d_nblk -= p.ncb;
        ++d_mblk;
      }
    }
  };
  Item cur, nxt;
  decode_next(cur);
  nxt = cur;
  // sub-block sb of item s: image, halo origin, liveness
  auto sub_block = [&](const Item& s, int sb, int& n, int& y0, int& x0, bool& live) __attribute__((always_inline)) {
    if constexpr (SB <= 2) {
      const bool one = SB > 1 && sb > 0;
      n = one ? s.n[SBS - 1] : s.n[0];
      y0 = one ? s.y0[SBS - 1] : s.y0[0];
      x0 = one ? s.x0[SBS - 1] : s.x0[0];
      live = one ? s.live[SBS - 1] : s.live[0];
    } else {
      const int sub = s.sub0 + sb;
      n = sub / per_img;
      const int r2 = sub - n * per_img, bby = r2 / p.BBX, bbx = r2 - bby * p.BBX;
      y0 = 2 * bby * PB - 1;
      x0 = 2 * bbx * PB - 1;
      live = sub < p.nsub;
    }
  };

  // this thread's rows of the gather table: sub-block and halo position (hy, hx) of row rho = tid + 512 e -- item-independent.  Rows
  // of the padding (no halo pixel) get an hy far outside every image: the bounds test below turns them into -1 like the pixels past
  // the border.  One word per row, hy << 16 | hx << 8 | sb, parked in LDS (each thread reads back its own): the 128 x 64 block has
  // no register left for it between two items.
#pragma unroll
  for (int e = 0; e < NTR; ++e) {
    const int rho = tid + 64 * NW * e;
    const int sb = rho / G::SBROWS, rem = rho - sb * G::SBROWS;
    const int hy = rem / G::PITCH, xs = rem - hy * G::PITCH;
    const int hx = PIX ? xs : xs < G::HALF ? 2 * xs : 2 * (xs - G::HALF) + 1;
    trows[rho] = ((rho < AROWS && hy < G::HW) ? hy << 16 : -(1 << 28)) | (hx << 8) | sb;
  }
  auto build_table = [&](const Item& s, int seq) __attribute__((always_inline)) {  // all threads; visible after the next barrier
    int* tab = tabs + (seq & 1) * AROWS_PAD;
    const int tnow = 64 * wave + wino_lane_now();
#pragma unroll
    for (int e = 0; e < NTR; ++e) {
      const int rho = tnow + 64 * NW * e;
      if (rho < AROWS_PAD) {
        int n, y0, x0;
        bool live;
        const int row = trows[rho];
        sub_block(s, row & 255, n, y0, x0, live);
        const int y = y0 + (PIX ? 0 : s.py) + (row >> 16), x = x0 + (PIX ? 0 : s.px) + ((row >> 8) & 255);
        const bool in = live && (unsigned)y < (unsigned)p.Hs && (unsigned)x < (unsigned)p.Ws;
        const int v = DG ? ((n - s.nfirst) * 2 * p.Hs + 2 * y + 1 - s.py) * (2 * p.Ws) + 2 * x + 1 - s.px  // plane (1 - py, 1 - px) of dz, pixel (y, x)
                         : ((n - s.nfirst) * p.Hs + y) * p.Ws + x;
        tab[rho] = in ? v : -1;
      }
    }
    rs_lds_writes_done();  // (read by every wave behind a later barrier, which hipcc emits bare: common.h)
  };

  // ---- fetch side: runs ONE chunk ahead of the MFMAs, across item boundaries (the next item's first chunk streams in while
  //      this item's outputs are stored).  A piece copies 16 rows of 64 bytes (4 lanes per row).  Piece j of a wave is of the same
  //      kind in every wave: j < JA halo rows 16 (wave + NW j) .., then filter rows 16 (wave + NW (j - JA)) ..; only the last piece of
  //      either kind asks whether the wave still has one.  Per lane and halo piece ONE register: the row's byte offset for the
  //      current item and source (from the gather table).  The filter pieces share one register, the offset of row 16 wave + (lane >> 2)
  //      = xi * BN + cout for every item: piece j - JA lies 128 rows = 128 / BN positions xi further (same cout, same swizzle), which
  //      goes into the DMA's scalar offset with the item's cout block and the chunk; the parity's filter set is the descriptor's base.
  const int ra = lane >> 2, pp = lane & 3;
  static_assert(128 % BN == 0, "a wave's filter pieces: the same cout, whole positions apart");
  //      Pixel form: one descriptor spans all four filter sets, and position xi = 3 r + c takes its rows from set 2 (r == 2) + (c == 2)
  //      (G g G^T of parity 0 is [w0, w0 + w1 + w2, ..] along an axis, of parity 1 [.., w0 + w1 + w2, w2]).  A piece's 16 rows lie in
  //      one position (BN is a multiple of 16), so that is one scalar per piece of the wave, formed once per block.
  int doff[JA], doffu, upos[JB];
  {
    const int w = 16 * wave + ra, xi = PIX ? 0 : w / BN, co = w - (w / BN) * BN;
    doffu = ((xi * p.Cout + co) * Cin) * 4 + ((pp ^ wino_swz(w)) & 3) * 16;
  }
  const int ustep = (128 / BN) * p.Cout * Cin * 4;
#pragma unroll
  for (int j = 0; j < JB; ++j) {
    const int fi = wave + NW * j, xi = fi < IB ? 16 * fi / BN : 8, r = xi / 3, c = xi - 3 * r;
    upos[j] = PIX ? __builtin_amdgcn_readfirstlane(((2 * (r == 2) + (c == 2)) * 9 + xi) * p.Cout * Cin * 4) : 0;
  }
  int f_seq = 0, f_kc = 0, f_g = 0;  // item / chunk / global chunk being fetched
  int f_nb = 0, f_nfirst = 0;        // of item f_seq: byte offset of its cout block's filter rows, first image
  __amdgpu_buffer_rsrc_t rsrcs = rs_dma_rsrc<kDmaClamp>(p.src1, 0);
  __amdgpu_buffer_rsrc_t rsrcu = PIX ? rs_dma_rsrc<kDmaClamp>(p.u, (long)36 * p.Cout * Cin * 4) : rsrcs;
  auto fetch_item = [&](const Item& s) __attribute__((always_inline)) {  // f_seq changed: what the new item's pieces need
    f_nfirst = s.nfirst;
    f_nb = s.nblk * BN * Cin * 4;
    if constexpr (!PIX) rsrcu = rs_dma_rsrc<kDmaClamp>(p.u + (long)(2 * s.py + s.px) * 9 * p.Cout * Cin, (long)9 * p.Cout * Cin * 4);
  };
  auto set_source = [&](bool src_first) __attribute__((always_inline)) {
    const int cb = (src_first ? p.C1 : p.C2) * 4;
    rsrcs = rs_dma_rsrc<kDmaClamp>(src_first ? p.src1 + f_nfirst * img1 : p.src2 + f_nfirst * img2,
                                   (long)(p.N - f_nfirst) * (src_first ? img1 : img2) * 4);
    const int* tab = tabs + (f_seq & 1) * AROWS_PAD;
    // every table read of the wave first (a row past the wave's share clamped: read, its piece never issued), then the offsets
    int pix[JA];
#pragma unroll
    for (int j = 0; j < JA; ++j) {
      const int ii = wave + NW * j;
      pix[j] = tab[16 * (ii < IA ? ii : IA - 1) + ra];
    }
#pragma unroll
    for (int j = 0; j < JA; ++j) {
      const int ii = wave + NW * j;
      const int rho = 16 * (ii < IA ? ii : IA - 1) + ra;
      doff[j] = pix[j] < 0 ? kDmaOOB : pix[j] * cb + ((pp ^ wino_swz(rho)) & 3) * 16;
    }
  };
  // issue chunk (f_seq, f_kc) into stage f_g & 1, then advance.  Past the block's last chunk (`past`: once, during its very
  // last MFMAs) the previous chunk's pieces are simply issued again into the free stage -- nobody reads them, and the MFMA
  // loop needs no second, fetch-less copy of itself (which cost registers: hipcc kept the two copies' live ranges apart).
  auto fetch_chunk = [&](auto interleave, bool past) __attribute__((always_inline)) {
    const int c0 = f_kc * KC;
    const bool src_first = c0 < p.C1;
    if (!past) {
      if (f_kc == 0) fetch_item(nxt);
      if (c0 == 0 || c0 == p.C1) set_source(src_first);
    }
    const unsigned int fL = lds0 + (f_g & 1) * STAGE;
    // (readfirstlane: the DMA's scalar offset must be provably uniform -- lds_dma.h)
    const int fsa = __builtin_amdgcn_readfirstlane((src_first ? c0 : c0 - p.C1) * 4), fsu = __builtin_amdgcn_readfirstlane(c0 * 4 + f_nb);
    interleave([&](int j) __attribute__((always_inline)) {
      if (j < JA) {
        const int ii = wave + NW * j;  // wave-uniform
        if (j < JA - 1 || JA * NW == IA || ii < IA) rs_dma16(rsrcs, fL + ii * 1024, doff[j], fsa);
      } else {
        const int fi = wave + NW * (j - JA);
        if (j < NI - 1 || JB * NW == IB || fi < IB) rs_dma16(rsrcu, fL + (IA + fi) * 1024, doffu, fsu + (PIX ? upos[j - JA] : (j - JA) * ustep));
      }
    });
    ++f_g;
    if (!past && ++f_kc == nk) {
      f_kc = 0;
      ++f_seq;
    }
  };

  // ---- fragment addressing (item-independent): lane = tile (lane & 15) of the wave's 16, 16-byte piece (lane >> 4) --------
  const int l15 = lane & 15, pc = lane >> 4;
  const int t = 16 * tg + wino_lane_tile<PB>(l15);
  const int tsb = 16 * tg / (PB * PB), tq = t - tsb * (PB * PB);  // (the wave's 16 tiles lie in one sub-block: wave-uniform)
  const int tty = tq / PB, ttx = tq - tty * PB;
  // pixel form: the wave's 4 x 4 pixel block (wby, wbx) of the sub-block's 2 x 2
  const int wby = (tg >> 1) & 1, wbx = tg & 1;
  int addrA[3][3];
  {
    const int rho0 = PIX ? tsb * G::SBROWS + (4 * wby + wino_lane_pixel_y(l15)) * G::PITCH + 4 * wbx + wino_lane_pixel_x(l15)
                         : tsb * G::SBROWS + 2 * tty * G::PITCH + ttx;
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const int rho = rho0 + r * G::PITCH + (PIX ? c : c == 0 ? 0 : (c == 1 ? G::HALF : 1));
        addrA[r][c] = rho * 64 + ((pc ^ wino_swz(rho)) & 3) * 16;
      }
  }
  // filter rows xi * BN + 32 cg + 16 m + l15: BN and 16 are multiples of 8, so the swizzle only sees l15
  const int addrB = AROWS_PAD * 64 + (16 * NM * cg + l15) * 64 + ((pc ^ wino_swz(l15)) & 3) * 16;  // + (xi * BN + 16 m) * 64

  build_table(cur, 0);
  __syncthreads();
  fetch_chunk([&](auto issue) __attribute__((always_inline)) {
#pragma unroll
    for (int j = 0; j < NI; ++j) issue(j);
  }, false);
  const int total = nitems * nk;
  const int Ho = 2 * p.Hs, Wo = 2 * p.Ws;

  // ---- the chunk loop, software-pipelined across its one barrier per chunk.  Chunk g runs as
  //        HEAD  positions 0 .. 8 - TAIL: 4 NM MFMAs each, the filter pieces one position ahead (the TAIL positions' all at once
  //              at the last one), chunk g + 1's LDS-DMA pieces spread over the first two thirds of the chunk's MFMAs
  //        -- the wave's LDS reads of stage g & 1 have returned, chunk g + 1 has landed: barrier --
  //        TAIL  the last TAIL positions' MFMAs, with chunk g + 1's patch reads and B^T d B transform in between them
  //      so a chunk opens straight into MFMAs: the barrier, the patch reads and the transform no longer stand between two chunks'
  //      MFMA streams.  Stage g & 1 is free for chunk g + 2 once every wave has passed chunk g's barrier (its last reads of the
  //      stage are waited for in front of it), and chunk g + 2 is issued in chunk g + 1's head.  Every accumulator receives the
  //      same MFMAs in the same order from the same transforms as in the unpipelined loop: only issue times moved.
  // positions behind the barrier (0: the unpipelined loop -- barrier, patch reads and transform between two chunks' MFMAs).  The
  // 128 x 64 block needs one: 16 MFMAs cover every wave's nine patch reads.  The NM = 2 forms, 8 MFMAs per position, each keep what
  // measured fastest (profiles/wino_items/ab_steps.txt): none for 128 x 32 (dec4) and the data gradient, one for 64 x 64 (dec0); the p4
  // blocks were not measured and keep their two.  The pixel forms, with fewer DMA pieces to spread and two fewer offset registers, all
  // run fastest without (profiles/wino_pixel/ab_tail.txt: 128 x 64 -1.0 .. -1.6 % against one position, 64 x 64 -0.7 %; 128 x 32 +0.5 %
  // with one).  (RS_WINO_TAIL2 / RS_WINO_TAIL4: a measurement build's value for all NM = 2 / NM = 4 forms.)
#if defined(RS_WINO_TAIL2) || defined(RS_WINO_TAIL4)  // (measurement builds: a value for all NM = 2 forms / for the NM = 4 forms)
#ifndef RS_WINO_TAIL2
#define RS_WINO_TAIL2 (PIX ? 0 : PB == 4 ? 2 : (DG || TG == 8) ? 0 : 1)
#endif
#ifndef RS_WINO_TAIL4
#define RS_WINO_TAIL4 (PIX ? 0 : 1)
#endif
  constexpr int TAIL = NM >= 4 ? RS_WINO_TAIL4 : RS_WINO_TAIL2;
#else
  constexpr int TAIL = PIX ? 0 : NM >= 4 ? 1 : PB == 4 ? 2 : (DG || TG == 8) ? 0 : 1;
#endif
  static_assert(TAIL >= 0 && TAIL <= 2, "positions behind the barrier");
  constexpr int NMMA = 36 * NM, NHEAD = (9 - TAIL) * 4 * NM, NT = TAIL * 4 * NM;
  constexpr int PSTEP = 2 * NMMA / 3 / NI >= 1 ? 2 * NMMA / 3 / NI : 1;
  static_assert((NI - 1) * PSTEP < NHEAD, "the DMA pieces go out in the chunk's head");
  f32x4 V[9], Bq[9][NM];  // the chunk's transformed patch and filter pieces; V and Bq[0] are formed in the previous chunk's tail
  // chunk head: the lane's 3x3 patch from stage L, V' = B^T d B (along x, then along y: [d0 - d1, d1, d2 - d1] each way, on 2-float
  // halves with v_pk_add_f32: two fp32 subtractions per instruction; as 4-float vector code hipcc emits scalar v_sub_f32: measured
  // -4 % on the 3x3 form) and the first filter pair B0, between the MFMAs tail(0 .. nt - 1) of the previous chunk: half of them
  // first (the reads' latency), then one of the transform's six steps per slice of the rest, the filter pair before the last ones
  auto chunk_head = [&](const unsigned char* L, f32x4(&Vn)[9], f32x4(&B0)[NM], auto tail, auto nt) __attribute__((always_inline)) {
    constexpr int N = decltype(nt)::value, LEAD = N / 2;
    f32x4 P[3][3];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 3; ++c) P[r][c] = *reinterpret_cast<const f32x4*>(L + addrA[r][c]);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = 0; i < LEAD; ++i) tail(i);
    __builtin_amdgcn_sched_barrier(0);
    f32x2 Tl[3][3], Th[3][3];
#pragma unroll
    for (int s = 0; s < 6; ++s) {
      if (s < 3) {
        const int r = s;
        const f32x2 l0 = {P[r][0][0], P[r][0][1]}, h0 = {P[r][0][2], P[r][0][3]};
        const f32x2 l1 = {P[r][1][0], P[r][1][1]}, h1 = {P[r][1][2], P[r][1][3]};
        const f32x2 l2 = {P[r][2][0], P[r][2][1]}, h2 = {P[r][2][2], P[r][2][3]};
        Tl[r][0] = pk_sub(l0, l1);
        Tl[r][1] = l1;
        Tl[r][2] = pk_sub(l2, l1);
        Th[r][0] = pk_sub(h0, h1);
        Th[r][1] = h1;
        Th[r][2] = pk_sub(h2, h1);
      } else {
        const int c = s - 3;
        const f32x2 a = pk_sub(Tl[0][c], Tl[1][c]), b = pk_sub(Tl[2][c], Tl[1][c]);
        const f32x2 d = pk_sub(Th[0][c], Th[1][c]), e = pk_sub(Th[2][c], Th[1][c]);
        Vn[0 * 3 + c] = f32x4{a[0], a[1], d[0], d[1]};
        Vn[1 * 3 + c] = f32x4{Tl[1][c][0], Tl[1][c][1], Th[1][c][0], Th[1][c][1]};
        Vn[2 * 3 + c] = f32x4{b[0], b[1], e[0], e[1]};
      }
#pragma unroll
      for (int i = LEAD + (N - LEAD) * s / 7; i < LEAD + (N - LEAD) * (s + 1) / 7; ++i) tail(i);
      __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int m = 0; m < NM; ++m) B0[m] = *reinterpret_cast<const f32x4*>(L + addrB + (16 * m) * 64);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = LEAD + (N - LEAD) * 6 / 7; i < N; ++i) tail(i);
    __builtin_amdgcn_sched_barrier(0);
  };
  // MFMA q of the chunk (q = (x * 4 + k) * NM + m: position x, k-step k, cout tile m -- the unpipelined loop's order)
  int g = 0;
  f32x4 acc[9][NM];
  auto mfma = [&](int q) __attribute__((always_inline)) {
    const int x = q / (4 * NM), k = (q / NM) % 4, m = q % NM;
    acc[x][m] = __builtin_amdgcn_mfma_f32_16x16x4f32(Bq[x][m][k], V[x][k], acc[x][m], 0, 0, 0);
  };
  rs_dma_wait();
  __syncthreads();  // chunk 0 is in stage 0
  chunk_head(smem, V, Bq[0], [](int) {}, std::integral_constant<int, 0>());

  for (int seq = 0; seq < nitems; ++seq) {
    if (!DG || (seq & 3) == 0) {  // (DG: the four parity planes of an output item accumulate)
#pragma unroll
      for (int x = 0; x < 9; ++x)
#pragma unroll
        for (int m = 0; m < NM; ++m) acc[x][m] = f32x4{0.f, 0.f, 0.f, 0.f};
    }

    for (int kc = 0; kc < nk; ++kc, ++g) {
      const unsigned char* L = smem + (g & 1) * STAGE;
      const bool more = g + 1 < total;
      // head: filter pieces one position ahead of the MFMAs that use them (sched_barrier keeps hipcc from sinking the reads in
      // front of every group of 8 MFMAs); chunk g + 1's DMA pieces spread evenly over the first two thirds of the chunk's MFMAs:
      // the CU's DMA path moves ~23 B/clk and this kernel needs ~12 B/clk of it; issued in a burst the pieces queue up and hold
      // the issuing waves (measured: -26 %), and the last ones need a third of a chunk to land before the barrier
      fetch_chunk([&](auto issue) __attribute__((always_inline)) {
#pragma unroll
        for (int x = 0; x < 9 - TAIL; ++x) {
#pragma unroll
          for (int xr = x + 1; xr < (x + 1 == 9 - TAIL ? 9 : x + 2); ++xr)
#pragma unroll
            for (int m = 0; m < NM; ++m) Bq[xr][m] = *reinterpret_cast<const f32x4*>(L + addrB + (xr * BN + 16 * m) * 64);
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int i = 0; i < 4 * NM; ++i) {
            const int q = x * 4 * NM + i;
            if (q % PSTEP == 0 && q / PSTEP < NI) issue(q / PSTEP);
            mfma(q);
          }
        }
      }, !more);
      // the next item's gather table (its buffer held item seq - 1's, whose last reader, the fetch of that item's C2 switch, was
      // two barriers ago at the latest); published by the barrier below and first read by the fetch of item seq + 1's chunk 0,
      // in item seq's last chunk -- a later one, since nk >= 2 (wino_plan)
      if (kc == 0 && seq + 1 < nitems) {
        decode_next(nxt);
        build_table(nxt, seq + 1);
      }
      rs_lds_writes_done();  // (and every LDS read of stage g & 1 by this wave has returned: other waves refill it behind the barrier)
      rs_dma_wait();
      __syncthreads();  // chunk g + 1 is in stage (g + 1) & 1; no wave reads stage g & 1 any more
      // tail: chunk g's last TAIL positions around chunk g + 1's head (past the block's last chunk: the re-issued pieces, unused)
      f32x4 Vn[9], B0[NM];
      chunk_head(smem + ((g + 1) & 1) * STAGE, Vn, B0, [&](int i) __attribute__((always_inline)) { mfma(NHEAD + i); },
                 std::integral_constant<int, NT>());
#pragma unroll
      for (int x = 0; x < 9; ++x) V[x] = Vn[x];
#pragma unroll
      for (int m = 0; m < NM; ++m) Bq[0][m] = B0[m];
    }

    // ---- Y = A^T M A, ReLU, store: lane = tile l15, couts 32 cg + 16 m + 4 pc + (0..3) -------------------------------------
    // (reads `cur`, the item decoded when its table was built: no decode, and at one or two sub-blocks per block no division)
    int e_n, e_y0, e_x0;
    bool e_live;
    sub_block(cur, tsb, e_n, e_y0, e_x0, e_live);
    // (the lane's tile and cout piece afresh, a few VALU per item: see wino_lane_now)
    const int e_lane = wino_lane_now(), e_pc = e_lane >> 4;
    const int e_tq = 16 * tg + wino_lane_tile<PB>(e_lane & 15) - tsb * (PB * PB), e_ty = e_tq / PB, e_tx = e_tq - e_ty * PB;
    const int a0 = e_y0 + 1 + 2 * e_ty, b0 = e_x0 + 1 + 2 * e_tx;
    if constexpr (DG) {
      if ((seq & 3) == 3 && e_live) {
        // destination of this wave's couts (block-uniform: a cout block never straddles csplit)
        const int co = cur.nblk * BN + 16 * NM * cg + 4 * e_pc;
        const bool second = p.out2 != nullptr && cur.nblk * BN >= p.csplit;
        float* ob = second ? p.out2 : p.out;
        const float* mb = second ? p.mask2 : p.mask1;
        const int ostride = p.out2 ? (second ? p.Cout - p.csplit : p.csplit) : p.Cout;
        const int ocol = second ? co - p.csplit : co;
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
          for (int v = 0; v < 2; ++v) {
            const int a = a0 + u, b = b0 + v;
            if (a >= p.Hs || b >= p.Ws) continue;
            const long o = ((long)(e_n * p.Hs + a) * p.Ws + b) * ostride + ocol;
#pragma unroll
            for (int m = 0; m < NM; ++m) {
              f32x4 y = (acc[u * 3 + v][m] + acc[u * 3 + v + 1][m]) + (acc[(u + 1) * 3 + v][m] + acc[(u + 1) * 3 + v + 1][m]);
              if (mb) {
                const f32x4 z = *reinterpret_cast<const f32x4*>(mb + o + 16 * m);
#pragma unroll
                for (int e = 0; e < 4; ++e) y[e] = z[e] > 0.f ? y[e] : 0.f;
              }
              *reinterpret_cast<f32x4*>(ob + o + 16 * m) = y;
            }
          }
      }
    } else if constexpr (PIX) {
      // the lane's pixel (a, b): rows past Hs / Ws of a ragged patch are masked per pixel; its four parities go to (2 a + u, 2 b + v)
      const int a = e_y0 + 1 + 4 * wby + wino_lane_pixel_y(e_lane & 15), b = e_x0 + 1 + 4 * wbx + wino_lane_pixel_x(e_lane & 15);
      if (e_live && a < p.Hs && b < p.Ws) {
        float* obase = p.out + cur.nblk * BN + 16 * NM * cg + 4 * e_pc + ((long)(e_n * Ho + 2 * a) * Wo + 2 * b) * p.Cout;
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
          for (int v = 0; v < 2; ++v) {
            float* o = obase + ((long)u * Wo + v) * p.Cout;
#pragma unroll
            for (int m = 0; m < NM; ++m) {
              f32x4 y = (acc[u * 3 + v][m] + acc[u * 3 + v + 1][m]) + (acc[(u + 1) * 3 + v][m] + acc[(u + 1) * 3 + v + 1][m]);
              if (p.relu) {
#pragma unroll
                for (int e = 0; e < 4; ++e) y[e] = fmaxf(y[e], 0.f);
              }
              *reinterpret_cast<f32x4*>(o + 16 * m) = y;
            }
          }
      }
    } else if (e_live) {
      float* obase = p.out + cur.nblk * BN + 16 * NM * cg + 4 * e_pc;
#pragma unroll
      for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int v = 0; v < 2; ++v) {
          const int a = a0 + u, b = b0 + v;
          if (a >= p.Hs || b >= p.Ws) continue;
          float* o = obase + ((long)(e_n * Ho + 2 * a + cur.py) * Wo + 2 * b + cur.px) * p.Cout;
#pragma unroll
          for (int m = 0; m < NM; ++m) {
            f32x4 y = (acc[u * 3 + v][m] + acc[u * 3 + v + 1][m]) + (acc[(u + 1) * 3 + v][m] + acc[(u + 1) * 3 + v + 1][m]);
            if (p.relu) {
#pragma unroll
              for (int e = 0; e < 4; ++e) y[e] = fmaxf(y[e], 0.f);
            }
            *reinterpret_cast<f32x4*>(o + 16 * m) = y;
          }
        }
    }
    cur = nxt;
  }
  rs_dma_wait();  // (the re-issued pieces of the last chunk: landed before this block's LDS is handed to the next one)
}

// U = G g G^T per (parity, cout, cin): phase pack [4][Cout][2][2][Cin] -> [4][9][Cout][Cin]
__global__ void pack_wino_phase_weight_kernel(const float* __restrict__ w, float* __restrict__ u, int Cout, int Cin, long total) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;  // over [4][Cout][Cin]
  if (i >= total) return;
  const int ci = (int)(i % Cin);
  const long r = i / Cin;
  const int co = (int)(r % Cout), ph = (int)(r / Cout);
  const float* g = w + (((long)ph * Cout + co) * 4) * Cin + ci;  // [2][2][Cin]
  const float g00 = g[0], g01 = g[Cin], g10 = g[2 * (long)Cin], g11 = g[3 * (long)Cin];
  const float v[9] = {g00, g00 + g01, g01, g00 + g10, (g00 + g01) + (g10 + g11), g01 + g11, g10, g10 + g11, g11};
#pragma unroll
  for (int x = 0; x < 9; ++x) u[(((long)ph * 9 + x) * Cout + co) * Cin + ci] = v[x];
}

// Data-gradient filters: wd [Cin][4][4][Cout] (rs_pack_dgrad_phase_weight_dt: the 4x4 / stride-2 taps over dz) -> U [4][9][Cin][Cout].
// Unit (py, px) of an output item reads plane (1 - py, 1 - px) of dz with the 2x2 taps g[r][s] = wd[ci][2 r + py][2 s + px][co]
// (= w4[2 r + 1 - pa][2 s + 1 - pb]); U = G g G^T as in the forward pack.
__global__ void pack_wino_dgrad_weight_kernel(const float* __restrict__ wd, float* __restrict__ u, int Cin, int Cout, long total) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;  // over [4][Cin][Cout]
  if (i >= total) return;
  const int co = (int)(i % Cout);
  const long r = i / Cout;
  const int ci = (int)(r % Cin), ph = (int)(r / Cin), py = ph >> 1, px = ph & 1;
  const float* g = wd + (long)ci * 16 * Cout + co;  // [4][4][Cout]
  const float g00 = g[(long)(py * 4 + px) * Cout], g01 = g[(long)(py * 4 + 2 + px) * Cout];
  const float g10 = g[(long)((2 + py) * 4 + px) * Cout], g11 = g[(long)((2 + py) * 4 + 2 + px) * Cout];
  const float v[9] = {g00, g00 + g01, g01, g00 + g10, (g00 + g01) + (g10 + g11), g01 + g11, g10, g10 + g11, g11};
#pragma unroll
  for (int x = 0; x < 9; ++x) u[(((long)ph * 9 + x) * Cin + ci) * Cout + co] = v[x];
}

bool wino_wide() {  // (A/B knob while the wide block is being measured: ROBOSAT_WINO_WIDE=0 keeps 64 tiles x 64 couts)
  return rs_knobs().wino_wide != 0;
}

// The forward's pixel form (ROBOSAT_WINO_PIXEL=0: the tile form everywhere, for the A/B), decided per cout width of the p8 blocks at
// compile time from what measured faster (profiles/wino_pixel).  The two 64-cout blocks go together: `wide` may depend on the batch
// size, and the two forms differ in fp32 summation order, so a layer's form must not follow its block shape.
constexpr bool kWinoPixel64 = true, kWinoPixel32 = true;
bool wino_pixel(int wgn) { return (wgn == 2 ? kWinoPixel64 : kWinoPixel32) && rs_knobs().wino_pixel != 0; }

// The 128-row block instead of the 64-row one where that still leaves two work items per CU.  Counted in REGIONS of 16 x 16 source
// pixels (an 8 x 8 patch of tiles = four 8 x 8 pixel sub-blocks), two per wide block; `units` work items per region pair and cout
// block: 4 on the forward side (the tile form's parities = the pixel form's four sub-blocks of a region), 1 for the data gradient
// (an output item accumulates its four planes).  One rule for the name queries and the launches.
bool wino_wide_rule(long regions, int ncb, int units) {
  return wino_wide() && (regions + 1) / 2 * ncb * units >= 2L * rs_cu_count();
}

struct WinoPlan {
  int pb, wgn;  // 8 | 4; 2 (64 couts per block) | 1 (32)
  int sb;       // sub-blocks per block
  bool pix;     // pixel form (p8 forward only)
  bool worth;   // enough work items to fill the chip (else the generic phase kernel is the faster choice)
  bool wide;    // 128 tiles x 64 couts per block instead of 64 x 64 (see wino_plan)
};

// `upsampled`: the launch's parity filters come from ONE 3x3 filter over the nearest-x2 upsample (rs_conv2d_fwd_upsampled_wino), which
// is what the pixel form's slab mapping needs; the plan's other answers (ok, names, `wide`) do not depend on it.
bool wino_plan(const rs_conv_desc* d, WinoPlan* pl, bool fwd = true, bool upsampled = false) {
  if (!d || d->N <= 0 || d->Hs <= 0 || d->Ws <= 0 || d->C1 <= 0 || (d->C1 % 16) || d->C2 < 0 || (d->C2 % 16) || d->Cout <= 0 ||
      (d->Cout % 32))
    return false;
  if (!(d->ups == 1 && d->kh == 3 && d->kw == 3 && d->stride == 1 && d->pad == 1 && d->Ho == 2 * d->Hs && d->Wo == 2 * d->Ws)) return false;
  const int ty = (d->Hs + 1) / 2, tx = (d->Ws + 1) / 2;
  if (ty < 4 || tx < 4) return false;  // (tiny layers: the halo of a 64-tile block would not fit; the generic kernel runs them)
  pl->pb = (ty >= 8 && tx >= 8) ? 8 : 4;
  pl->wgn = (d->Cout % 64 == 0) ? 2 : 1;
  pl->sb = 16 * (8 / pl->wgn) / (pl->pb * pl->pb);
  if (d->C1 + d->C2 < 32) return false;  // (the table of the next item is built during an item's first chunk: two chunks at least)
  const long cmax = d->C1 > d->C2 ? d->C1 : d->C2;
  if ((long)(pl->sb + 1) * d->Hs * d->Ws * cmax * 4 >= (1L << 31)) return false;  // 32-bit byte offsets within a block's images
  if ((long)9 * d->Cout * (d->C1 + d->C2) * 4 >= (1L << 31)) return false;
  if ((long)d->N * d->Ho * d->Wo >= (1L << 31)) return false;
  // (pixel form: one descriptor spans the four filter sets, and the position's set goes into a 32-bit scalar offset; a layer whose
  // four sets do not fit keeps the tile form)
  pl->pix = fwd && upsampled && pl->pb == 8 && wino_pixel(pl->wgn) && (long)4 * 9 * d->Cout * (d->C1 + d->C2) * 4 < (1L << 31);
  // one block per CU and no other block to hide behind: a launch with fewer work items than ~half the CUs (the `center`
  // block at small batches) is faster on the generic phase kernel's 4-blocks-per-CU grid
  // Worth it -- a decision on the layer's GEOMETRY alone, never on the batch size: a tile's probabilities must not depend on
  // its batch neighbours (the two forms differ in fp32 summation order), so the same kernel runs a layer at every N.  One
  // full 8x8 patch of tiles per image side at least (Hs, Ws >= 15): with fewer, a block's tiles straddle images and the
  // persistent one-block-per-CU grid is short of work items at any batch size (`center` at 512^2: 0.32 vs 0.21 ms).
  pl->worth = pl->pb == 8;
  // Block shape for the 64-cout layers: 128 tiles x 64 couts (a wave = 16 tiles x 64 couts: twice the MFMAs per transformed
  // patch and per filter byte; +3-5 % on dec1-dec3) when that still leaves two work items per CU, else 64 tiles x 64 couts
  // (dec0 at bs 16: 128 wide items on 256 CUs would halve the chip).  Either shape accumulates every output in the same order
  // -- they differ in which wave computes what --, so the choice may depend on the batch size without making a tile's
  // output depend on it.
  pl->wide = pl->pb == 8 && pl->wgn == 2 && wino_wide_rule((long)d->N * rs_cdiv(d->Hs, 16) * rs_cdiv(d->Ws, 16), d->Cout / 64, 4);
  if (pl->wide) pl->sb = 2;
  return true;
}

}  // namespace

extern "C" int rs_conv2d_phase_wino_ok(const rs_conv_desc* d) {
  WinoPlan pl;
  if (!wino_plan(d, &pl)) return 0;
  return pl.worth ? 1 : 2;
}

extern "C" const char* rs_conv2d_phase_wino_name(const rs_conv_desc* d) {
  WinoPlan pl;
  if (!wino_plan(d, &pl)) return "";
  if (pl.pb == 8) return pl.wide ? "conv_wino_f32<phase,p8,128x64>" : (pl.wgn == 2 ? "conv_wino_f32<phase,p8,64x64>" : "conv_wino_f32<phase,p8,128x32>");
  return pl.wgn == 2 ? "conv_wino_f32<phase,p4,64x64>" : "conv_wino_f32<phase,p4,128x32>";
}

extern "C" int rs_pack_wino_phase_weight(const float* w_phase, float* u, int Cout, int Cin, rs_stream_t stream) {
  if (!w_phase || !u || Cout <= 0 || Cin <= 0) return RS_EINVAL;
  const long total = 4L * Cout * Cin;
  pack_wino_phase_weight_kernel<<<rs_cdiv(total, 256), 256, 0, (hipStream_t)stream>>>(w_phase, u, Cout, Cin, total);
  return RS_LAUNCH_RESULT();
}

namespace {
int wino_fwd_launch(const rs_conv_desc* d, const float* src1, const float* src2, const float* u, float* out, rs_stream_t stream,
                    bool upsampled) {
  WinoPlan pl;
  if (!wino_plan(d, &pl, true, upsampled) || !src1 || !u || !out || (d->C2 > 0 && !src2)) return RS_EINVAL;
  WinoArgs a;
  a.src1 = src1;
  a.src2 = src2;
  a.u = u;
  a.out = out;
  a.N = d->N;
  a.Hs = d->Hs;
  a.Ws = d->Ws;
  a.C1 = d->C1;
  a.C2 = d->C2;
  a.Cout = d->Cout;
  a.TY = (d->Hs + 1) / 2;
  a.TX = (d->Ws + 1) / 2;
  // sub-blocks: PB x PB patches of tiles, each parity an item of its own; pixel form: 8 x 8 patches of source pixels
  a.BBY = pl.pix ? rs_cdiv(d->Hs, 8) : rs_cdiv(a.TY, pl.pb);
  a.BBX = pl.pix ? rs_cdiv(d->Ws, 8) : rs_cdiv(a.TX, pl.pb);
  if ((long)d->N * a.BBY * a.BBX >= (1L << 31)) return RS_EINVAL;
  a.nsub = d->N * a.BBY * a.BBX;
  a.ncb = d->Cout / (32 * pl.wgn);
  a.relu = d->relu;
  a.out2 = nullptr;
  a.mask1 = a.mask2 = nullptr;
  a.csplit = 0;
  const long items = (long)rs_cdiv(a.nsub, pl.sb) * a.ncb * (pl.pix ? 1 : 4);
  if (items >= (1L << 31)) return RS_EINVAL;
  // persistent: one block per CU (its LDS stages fill the CU), items dealt round-robin
  const int grid = (int)(items < rs_cu_count() ? items : rs_cu_count());
  hipStream_t s = (hipStream_t)stream;
  if (pl.pix && pl.wide) conv_wino_f32_kernel<8, 8, 1, 4, false, true><<<grid, 512, 0, s>>>(a);  // 128 pixels x 64 couts
  else if (pl.pix && pl.wgn == 2) conv_wino_f32_kernel<8, 4, 2, 2, false, true><<<grid, 512, 0, s>>>(a);
  else if (pl.pix) conv_wino_f32_kernel<8, 8, 1, 2, false, true><<<grid, 512, 0, s>>>(a);
  else if (pl.wide) conv_wino_f32_kernel<8, 8, 1, 4><<<grid, 512, 0, s>>>(a);  // 128 tiles x 64 couts
  else if (pl.pb == 8 && pl.wgn == 2) conv_wino_f32_kernel<8, 4, 2><<<grid, 512, 0, s>>>(a);
  else if (pl.pb == 8) conv_wino_f32_kernel<8, 8, 1><<<grid, 512, 0, s>>>(a);
  else if (pl.wgn == 2) conv_wino_f32_kernel<4, 4, 2><<<grid, 512, 0, s>>>(a);
  else conv_wino_f32_kernel<4, 8, 1><<<grid, 512, 0, s>>>(a);
  return RS_LAUNCH_RESULT();
}
}  // namespace

// Any phase pack's four 2x2 parity filter sets (the DecoderBlock's, or the 3x3 / stride-2 data gradient's over dy): the tile form.
extern "C" int rs_conv2d_fwd_phase_wino(const rs_conv_desc* d, const float* src1, const float* src2, const float* u, float* out,
                                        rs_stream_t stream) {
  return wino_fwd_launch(d, src1, src2, u, out, stream, false);
}

// The DecoderBlock itself: `u` packed from ONE 3x3 filter over the upsample (rs_pack_phase_weight_dt -> rs_pack_wino_phase_weight), so
// the p8 blocks may take the pixel form.  Other filters give wrong results here: they go through rs_conv2d_fwd_phase_wino.
extern "C" int rs_conv2d_fwd_upsampled_wino(const rs_conv_desc* d, const float* src1, const float* src2, const float* u, float* out,
                                            rs_stream_t stream) {
  return wino_fwd_launch(d, src1, src2, u, out, stream, true);
}

// ---- the DecoderBlock's data gradient in the same form (round 6) ---------------------------------------------------------------------
// `d` is the FORWARD layer's descriptor (DecoderBlock: ups = 1, 3x3, pad 1; Hs x Ws the source grid, C1 + C2 the concatenated input
// channels, Cout the block's output channels): the gradient has Cout INPUT channels (dz, at 2 Hs x 2 Ws) and C1 + C2 OUTPUT channels.
namespace {
bool wino_dgrad_plan(const rs_conv_desc* d, rs_conv_desc* g, WinoPlan* pl) {
  if (!d || d->C1 <= 0 || d->C2 < 0 || d->Cout <= 0) return false;
  *g = *d;
  g->C1 = d->Cout;
  g->C2 = 0;
  g->Cout = d->C1 + d->C2;
  if (!wino_plan(g, pl, false) || !pl->worth) return false;
  // (dz images are four times the plan's: 32-bit byte offsets within a block's images)
  if ((long)(pl->sb + 1) * 4 * d->Hs * d->Ws * g->C1 * 4 >= (1L << 31)) return false;
  if (g->Cout % 64) return false;  // (64-cout blocks only: every DecoderBlock input of the U-Net is a multiple of 64 channels)
  // (the wide block where that leaves two OUTPUT items per CU: there is no parity factor in the item count here)
  pl->wide = wino_wide_rule((long)d->N * rs_cdiv(d->Hs, 16) * rs_cdiv(d->Ws, 16), g->Cout / 64, 1);
  pl->sb = pl->wide ? 2 : 1;
  return true;
}
}  // namespace

extern "C" int rs_conv2d_dgrad_phase_wino_ok(const rs_conv_desc* d) {
  rs_conv_desc g;
  WinoPlan pl;
  return wino_dgrad_plan(d, &g, &pl) ? 1 : 0;
}

extern "C" const char* rs_conv2d_dgrad_phase_wino_name(const rs_conv_desc* d) {
  rs_conv_desc g;
  WinoPlan pl;
  if (!wino_dgrad_plan(d, &g, &pl)) return "";
  return pl.wide ? "conv_wino_f32<dgrad4x4,p8,128x64>" : "conv_wino_f32<dgrad4x4,p8,64x64>";
}

extern "C" int rs_pack_wino_dgrad_weight(const float* wd4x4, float* u, int Cin, int Cout, rs_stream_t stream) {
  if (!wd4x4 || !u || Cin <= 0 || Cout <= 0) return RS_EINVAL;
  const long total = 4L * Cin * Cout;
  pack_wino_dgrad_weight_kernel<<<rs_cdiv(total, 256), 256, 0, (hipStream_t)stream>>>(wd4x4, u, Cin, Cout, total);
  return RS_LAUNCH_RESULT();
}

extern "C" int rs_conv2d_dgrad_phase_wino(const rs_conv_desc* d, const float* dz, const float* u, float* out, const float* mask,
                                          float* out2, const float* mask2, int csplit, rs_stream_t stream) {
  rs_conv_desc g;
  WinoPlan pl;
  if (!wino_dgrad_plan(d, &g, &pl) || !dz || !u || !out) return RS_EINVAL;
  if (out2 ? (csplit <= 0 || csplit >= g.Cout || (csplit % 64) != 0) : (csplit != 0 || mask2 != nullptr)) return RS_EINVAL;
  WinoArgs a;
  a.src1 = dz;
  a.src2 = nullptr;
  a.u = u;
  a.out = out;
  a.out2 = out2;
  a.mask1 = mask;
  a.mask2 = mask2;
  a.csplit = csplit;
  a.N = d->N;
  a.Hs = d->Hs;
  a.Ws = d->Ws;
  a.C1 = g.C1;
  a.C2 = 0;
  a.Cout = g.Cout;
  a.TY = (d->Hs + 1) / 2;
  a.TX = (d->Ws + 1) / 2;
  a.BBY = rs_cdiv(a.TY, pl.pb);
  a.BBX = rs_cdiv(a.TX, pl.pb);
  a.nsub = d->N * a.BBY * a.BBX;
  a.ncb = g.Cout / 64;
  a.relu = 0;
  const bool wide = pl.wide;
  const long items = (long)rs_cdiv(a.nsub, pl.sb) * a.ncb;
  if (items >= (1L << 29)) return RS_EINVAL;
  const int grid = (int)(items < rs_cu_count() ? items : rs_cu_count());
  hipStream_t s = (hipStream_t)stream;
  if (wide) conv_wino_f32_kernel<8, 8, 1, 4, true><<<grid, 512, 0, s>>>(a);
  else conv_wino_f32_kernel<8, 4, 2, 2, true><<<grid, 512, 0, s>>>(a);
  return RS_LAUNCH_RESULT();
}
