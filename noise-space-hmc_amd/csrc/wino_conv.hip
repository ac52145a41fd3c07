// 3x3 stride-1 padding-1 convolution of the score network as Winograd F(2x2, 3x3) in ONE launch, with the sixteen
// per-frequency products on the fp32 matrix cores (v_mfma_f32_32x32x2_f32: exact k-ascending fp32 FMA chains).
//
//   y[n,k,h,w] = sum_c sum_rs x[n,c,h+r-1,w+s-1] w[k,c,r,s]      NCHW fp32
//   U = G w G^T   [C][K][16], built once per weight tensor by k_wino_weights (forward, or backward-data: the flipped,
//                 transposed filter, so that dx = conv(dy, w') runs on the same kernel)
//   V = B^T d B   from a halo patch of x, zero padding by predicate, staged in LDS per chunk of 8 channels (never in HBM)
//   M_f[k, tile] += U_f[c, k] V_f[c, tile]   for f = 0..15, c ascending, no atomics: two runs give the same bits
//   Y = A^T M A   in registers, stored as 256-byte row segments; optional epilogue (acc + bias[k]) + add, k_bias_add2's order
//
// Frequency index: f = 4 b + a, a the vertical and b the horizontal frequency, innermost in U and in both LDS operands.
//
// Workgroup: 256 threads own 64 output channels x 64 tiles (2 tile rows x 32 tile columns = 4 x 64 outputs) x 16 frequencies.
// Wave (kh, th) holds channels 32 kh .. + 31 of tile row th for all 16 frequencies: 16 accumulator tiles = 256 registers,
// one wave per SIMD; every lane has all 16 frequencies of its outputs, so the output transform needs no exchange.
// The 64 tiles are 32 / TC pairs of tile rows x TC tile columns, TC a template parameter: 32 is the 4 x 64 block above,
// 16 an 8 x 32 block (images 32 wide), 8 a 16 x 16 block (images 16 wide).  Tile t = 32 th + lr of the workgroup is tile row
// 2 (lr / TC) + th, column lr % TC; only the loader's patch origin, the block origin and the epilogue's output origin
// know TC, the LDS layout, the main loop and the accumulation order do not.
// LDS: two buffers of U[8][64][16] + V[8][64][16] = 128 KB: a row (c, k or tile) is the 16 frequencies = 64 bytes, so a
// lane fetches the eight A or B values of one MFMA group with two ds_read_b128.  Rows of 64 bytes alone would put the 16
// lanes of a b128 group on 4 of the 16 slots of a bank row; the 16-byte granule g of row R is stored at granule
// g ^ wc_swz(R), which spreads every group of the read over all 16 and every 8-lane group of the stores (32 banks: the four
// rows of one parity) over all 8 (tests/test_wino_swizzle_cpu.py enumerates both).  While chunk i is multiplied, chunk
// i + 1 is loaded into registers, transformed and written to the other buffer.
// K that is a multiple of 32 but not of 64 (template parameter TAIL, entry nhmc_conv3x3_wino_k32): ceil(K / 64) K blocks, the
// last one half empty.  U keeps nhmc_wino_weights' layout [C][K][16] with K as it is; the tail block's loads of the upper
// 32 rows are predicated off and zeros go to LDS instead, so nothing outside U is read.  A channel's MFMA chain is the same
// A row against the same B rows in the same order whatever K is, so its bits do not depend on K.
// Two workgroup geometries: k_conv3x3_wino, the four waves described above, for every instantiation; and k_conv3x3_wino8,
// eight waves, two per SIMD, for the wide geometry without a tail block (TC = 32, K % 64 == 0), the default there.  Its wave
// (fh, kh, th) holds the 8 frequencies 8 fh .. + 7 of wave (kh, th)'s outputs, 128 accumulators, so that the two halves of a
// (kh, th) share a SIMD; before the output transform the pair exchanges accumulator halves through LDS, lane by lane, and
// each wave transforms 8 of the lane's 16 channel rows.  Same LDS layout, same MFMA chains, same transform expressions: the
// same bits.  NHMC_WINO_WAVES = 4 | 8, read per call, chooses (wc_waves); the comment above k_conv3x3_wino8 has the details.
// Nearest 2x upsample (template parameters of k_conv3x3_wino8, entry nhmc_conv3x3_wino_up; the up-sampling ResBlocks, whose
// upsampled tensors then never reach memory).  IN_UP: x is [n][C][H / 2][W / 2] and stands for its nearest 2x upsample.  The
// tiles are even-aligned, so rows 1 and 2 of every 4 x 4 patch are one low-res row and columns 1 and 2 one low-res column, at
// the zero-padded borders too.  Column b = 2 of the transform is d(r, 2) - d(r, 1) and entry a = 2 is e[2] - e[1]: every V
// entry with a == 2 or b == 2 is exactly +0.0f, the frequencies f = 2, 6, 8, 9, 10, 11, 14, and their accumulators stay +0
// (u * (+0) = +-0, +0 + (-0) = +0; tests/test_wino_up_cpu.py).  The loader fetches three rows of one dword instead of four
// of two, column 2 of V is neither formed nor stored nor read, and no MFMA is issued for the seven frequencies: 6 per unit in
// the lower frequency half, 3 in the upper, whose j < 4 is one uniform branch.  The accumulators of the skipped frequencies
// keep their zero state and the exchange and Y = A^T M A run unchanged, adding the same +0 terms in the same order: for
// finite inputs the bits are those of the kernel on the materialised tensor.  With +-inf or NaN in x the skipped products held
// inf - inf = NaN, so the values at non-finite outputs may differ; the set of non-finite output positions is the same.
// ADD_UP: add is [n][K][H / 2][W / 2]; the epilogue loads the two low-res values under the lane's four output columns and
// adds {l.x, l.x, l.y, l.y} where it adds the float4 otherwise.  OUT_POOL: y is [n][K][H / 2][W / 2]; a lane's 2 x 2 patch
// is one low-res pixel, stored as ((((0 + o00) + o01) + o10) + o11) * 0.25f * 4.0f, the chain of k_sr<2, 1> followed by the
// multiplication by 4 of the upsample's backward (denormals round as there), with no exchange between lanes.
// Skip bias (template parameter ADD_BIAS of k_conv3x3_wino8, entry nhmc_conv3x3_wino_skip; the ResBlocks whose skip path is a
// 1x1 convolution): add is that convolution's output WITHOUT its bias and add_bias [K] the bias; the epilogue stores
// (acc + bias[k]) + (add + add_bias[k]).  The inner add is the fp32 add of the broadcast pass that would otherwise have run
// over add before this kernel, so every output bit is that sequence's, and the pass (one read and one write of add) is gone.
#include "nhmc_common.h"

#include <cstdlib>
#include <type_traits>

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float wc_v2f __attribute__((ext_vector_type(2)));

constexpr int WC_KBLK = 64;                      // output channels per workgroup
constexpr int WC_ROWS = 4, WC_COLS = 64;         // output block of the wide geometry (TC = 32): 2 x 32 tiles
constexpr int WC_CHUNK = 8;                      // input channels per LDS stage
constexpr int WC_OPER = 16 * WC_CHUNK * 64;      // floats of one operand (U or V) of one stage
constexpr int WC_LDS_BYTES = 4 * WC_OPER * 4;    // 2 stages x (U + V)

// granule swizzle of operand row R, linear in the row's bits: bit 1 -> 01, bit 2 -> 10, bit 3 -> 11.  A bijection on the rows
// {0, 12, 20, 24} + r and {4, 8, 16, 28} + r that share a quarter of the 64 banks in a ds_read_b128 lane group, and on the
// four rows of one parity among 8 contiguous ones, which share a half of the 32 banks in a ds_write_b128 lane group
__device__ __forceinline__ constexpr int wc_swz(int R) { return ((R >> 1) & 3) ^ (((R >> 3) & 1) ? 3 : 0); }

// Phase stamps, in the diagnostic build of tools/wino_stamps.hip only (NHMC_WINO_STAMPS; libnhmc.so holds none): every wave
// keeps the shader clock of its phase boundaries in scalar registers and lane 0 writes them behind the epilogue, 24 values
// per wave, into a buffer of their own.  WC_T64: 0 kernel start, 1 behind the prologue barrier, 2 loop start, 3 loop end,
// 4 kernel end; 5, 6 the constant-rate clock at loop start and end.  WC_T32 (low words, of chunk nhmc_wino_stamp_chunk
// only): 0 .. 6 the head of unit u, 7 / 8 around the wait for the patch, 9 / 10 around the chunk's barrier, 11 the head
// of unit 7 (10 -> 11 held all loads of a chunk while they were issued in one piece), 12 the chunk's end, 13 .. 16 the
// heads of MFMAs 1, 3, 5, 7 of unit 4: behind the reads, the arithmetic, the V stores, the U stores of a staging unit
#ifdef NHMC_WINO_STAMPS
__device__ unsigned long long* nhmc_wino_stamps;
__device__ int nhmc_wino_stamp_chunk;
#define WC_FENCE() __builtin_amdgcn_sched_barrier(0)
#define WC_T64(i) do { WC_FENCE(); t64[i] = __builtin_amdgcn_s_memtime(); WC_FENCE(); } while (0)
#define WC_R64(i) do { WC_FENCE(); t64[i] = __builtin_amdgcn_s_memrealtime(); WC_FENCE(); } while (0)
#define WC_T32(i) do { WC_FENCE(); const unsigned now_ = (unsigned)__builtin_amdgcn_s_memtime(); \
                       t32[i] = ch == stamp_ch ? now_ : t32[i]; WC_FENCE(); } while (0)
#else
#define WC_T64(i)
#define WC_R64(i)
#define WC_T32(i)
#endif

struct WinoArgs {
  const float* x; const float* U; const float* bias; const float* add; float* y;
  int C, K, H, W, row_blocks, col_blocks;
  const float* add_bias;                           // ADD_BIAS only; last, so that every other field keeps its offset
};

template <int TC, bool TAIL>
__global__ __launch_bounds__(256, 1) void k_conv3x3_wino(const WinoArgs a) {
  static_assert(TC == 32 || TC == 16 || TC == 8, "64 tiles as 32 / TC row pairs x TC columns");
  constexpr int BLK_ROWS = 128 / TC, BLK_COLS = 2 * TC;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 31, lh = lane >> 5;
  const int kh = wave & 1, th = wave >> 1;
  const int C = a.C, K = a.K, H = a.H, W = a.W, HW = H * W;
#ifdef NHMC_WINO_STAMPS
  unsigned long long t64[7] = {};
  unsigned t32[17] = {};
  const int stamp_ch = nhmc_wino_stamp_chunk < C / WC_CHUNK ? nhmc_wino_stamp_chunk : C / WC_CHUNK - 1;
#endif
  WC_T64(0);

  // the K blocks of one spatial block, then the next spatial block, follow each other on one XCD (they share the input)
  const int total = gridDim.x;
  int logical = blockIdx.x;
  if ((total & 7) == 0) logical = (logical & 7) * (total >> 3) + (logical >> 3);
  const int kblocks = TAIL ? (K + WC_KBLK - 1) / WC_KBLK : K / WC_KBLK;
  const int kb = logical % kblocks, sp = logical / kblocks;
  // TAIL (K % 64 == 32): the last K block owns its lower 32 channels only.  Its kh = 1 waves keep their loader and barrier
  // roles, issue no MFMA (a scalar branch: the condition goes through readfirstlane) and leave before the epilogue; rows
  // 32 .. 63 of its U stage are never read from U (they would be the next input channel's, or past the end) and are zeros
  // in LDS.  A second copy of the loop for those waves cost the other waves 212 bytes of scratch; the branch costs none
  const bool tail_block = TAIL && kb == kblocks - 1;
  const bool idle = tail_block && __builtin_amdgcn_readfirstlane(kh) == 1;
  const bool u_row_ok = !(tail_block && tid >= 128);
  const int cb = sp % a.col_blocks, rb = (sp / a.col_blocks) % a.row_blocks, n = sp / (a.col_blocks * a.row_blocks);
  const int h0 = rb * BLK_ROWS, w0 = cb * BLK_COLS;

  // ---- loader roles: thread (lc, ltx) transforms channel lc of the chunk for the two tiles of tile column ltx % TC of
  // row pair ltx / TC
  // The 6 x 4 patch of the thread has its origin at column w0 + 2 t - 1, t = ltx % TC.  Its two middle columns, 2 t and
  // 2 t + 1 of the block, are one 8-byte load per row: w0 + 2 t is even and W a multiple of 16, so the load is aligned and
  // never leaves the row.  The outer columns are the neighbouring lanes' (the 32 lanes of one lc are contiguous in a wave):
  // column 2 t - 1 is the .y of lane - 1 and column 2 t + 2 the .x of lane + 1, moved by DPP once the patch has arrived.
  // Lanes t = 0 and t = TC - 1 have no such neighbour.  In the narrow geometries the block is the whole width and the
  // missing column is the zero padding (okmask).  In the wide one it is the padding in the first / last column block and
  // column w0 - 1 / w0 + 64 of the image otherwise: one 4-byte load per row, EDGE, whose address is that column in the two
  // edge lanes and the lane's own column 2 t (in range, the line the 8-byte load fetches) in all the others
  constexpr bool EDGE = TC == 32;
  constexpr int NP = EDGE ? 12 : 6;                      // patch loads per thread and chunk
  const int lc = tid >> 5, ltx = tid & 31, lt = ltx % TC;
  unsigned voff[6], eoff[6];                             // bytes from the chunk's first channel: the load's 32-bit offset
  unsigned okmask = 0;
  const int ecol = lt == 0 ? w0 - 1 : w0 + 2 * TC;       // meaningful in the edge lanes only
  const bool eok = EDGE && (lt == 0 || lt == TC - 1) && (unsigned)ecol < (unsigned)W;
#pragma unroll
  for (int r = 0; r < 6; ++r) {
    const int row = h0 + 4 * (ltx / TC) - 1 + r;
    const bool rok = (unsigned)row < (unsigned)H;
    voff[r] = rok ? 4u * (unsigned)(lc * HW + row * W + w0 + 2 * lt) : 0u;
    eoff[r] = rok ? 4u * (unsigned)(lc * HW + row * W + (eok ? ecol : w0 + 2 * lt)) : 0u;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int col = w0 + 2 * lt - 1 + s;
      const bool ok = rok && (unsigned)col < (unsigned)W;
      okmask |= ok ? 1u << (r * 4 + s) : 0u;
    }
  }
  const float* xn = a.x + (int64_t)n * C * HW;
  // U stage: the chunk's 8 x 64 rows of this K block are 8 contiguous pieces of 4 KB; thread takes float4 tid of piece i
  const char* un = reinterpret_cast<const char*>(a.U + (int64_t)kb * WC_KBLK * 16);
  const unsigned uoff = 16u * tid;
  const int uw = (tid & ~3) * 4 + (((tid & 3) ^ wc_swz(tid >> 2)) << 2);            // row tid >> 2, swizzled granule
  const int vw = (lc * 64 + ltx) * 16, vswz = wc_swz(ltx);                          // rows lc * 64 + 32 ty + ltx

  // A chunk's NP + 8 loads per thread, numbered in the order they are issued and consumed: 0 .. NP - 1 the patch (row by row;
  // with EDGE the row's 8-byte load, then its edge load; all of it is needed at unit 3), then the 8 U pieces (piece 2 b,
  // 2 b + 1 at unit 3 + b).  Scalar base + 32-bit lane offset, no address arithmetic per load.  The offset passes through an
  // empty asm next to its load: hoisted out of the loop, its zero extension became a register pair per load and a 64-bit
  // add in front of every load
  wc_v2f xm[6];                                          // columns 1, 2 of the patch
  float xl[6], xq[6], xe[6];                             // columns 0 and 3 (behind exchange_patch), the edge loads
  nhmc_v4f ur[8];
  auto load_one = [&](int ch, int i) {
    if (i < NP) {
      const char* xs = reinterpret_cast<const char*>(xn + (int64_t)ch * WC_CHUNK * HW);
      const int r = EDGE ? i >> 1 : i;
      unsigned off = EDGE && (i & 1) ? eoff[r] : voff[r];
      asm volatile("" : "+v"(off));
      if (EDGE && (i & 1)) xe[r] = *reinterpret_cast<const float*>(xs + off);
      else xm[r] = *reinterpret_cast<const wc_v2f*>(xs + off);
    } else {
      const char* us = un + (int64_t)ch * WC_CHUNK * K * 64 + (int64_t)(i - NP) * K * 64;
      unsigned off = uoff;
      asm volatile("" : "+v"(off));
      if (!TAIL || u_row_ok) ur[i - NP] = *reinterpret_cast<const nhmc_v4f*>(us + off);
      else ur[i - NP] = nhmc_v4f{0.0f, 0.0f, 0.0f, 0.0f};
    }
  };
  auto issue_loads = [&](int ch, int first, int last) {
#pragma unroll
    for (int i = first; i < last; ++i) load_one(ch, i);
  };
  // the loaded patch is first touched here, three units after its loads were issued: without the pin the selects and the
  // first-level differences of all four columns move to the head of the chunk, and the chunk starts with a wait on the loads
  auto pin_patch = [&]() {
#pragma unroll
    for (int r = 0; r < 6; ++r) {
      asm volatile("" : "+v"(xm[r]));
      if (EDGE) asm volatile("" : "+v"(xe[r]));
    }
  };
  // the outer columns from the neighbouring lanes: wave_shr:1 gives lane l the value of lane l - 1, wave_shl:1 that of lane
  // l + 1 (values are moved, not computed).  What a lane at t = 0 / t = TC - 1 receives is another tile row's or channel's
  // and is never used: with EDGE the edge load takes its place, and where that column is outside the image, here as in the
  // narrow geometries, okmask selects the padding's 0.0f
  auto exchange_patch = [&]() {
#pragma unroll
    for (int r = 0; r < 6; ++r) {
      xl[r] = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(xm[r].y), 0x138, 0xF, 0xF, false));
      xq[r] = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(xm[r].x), 0x130, 0xF, 0xF, false));
      if (EDGE) {
        xl[r] = lt == 0 ? xe[r] : xl[r];
        xq[r] = lt == TC - 1 ? xe[r] : xq[r];
      }
    }
  };
  auto d = [&](int r, int s) {
    const float v = s == 0 ? xl[r] : s == 1 ? xm[r].x : s == 2 ? xm[r].y : xq[r];
    return (okmask >> (r * 4 + s)) & 1u ? v : 0.0f;
  };
  // column b of V = B^T d B for both tiles of the thread (one granule each), and a quarter of the U stage -> LDS stage `st`
  // in pieces, so that the staging units can place each between two MFMAs: the row differences e[r] of column b, the
  // granule of tile ty from them with its store, and the store of one U piece
  float e[6];
  auto stage_rows = [&](int b, int first, int last) {
#pragma unroll
    for (int r = first; r < last; ++r)
      e[r] = b == 0 ? d(r, 0) - d(r, 2) : b == 1 ? d(r, 1) + d(r, 2) : b == 2 ? d(r, 2) - d(r, 1) : d(r, 1) - d(r, 3);
  };
  nhmc_v4f vt[2];                                        // one granule per tile: both are formed before the first is stored,
  auto stage_cols = [&]() {                              // so the second is not written into registers a store still reads
#pragma unroll
    for (int ty = 0; ty < 2; ++ty) {
      const int r0 = 2 * ty;
      vt[ty].x = e[r0] - e[r0 + 2]; vt[ty].y = e[r0 + 1] + e[r0 + 2]; vt[ty].z = e[r0 + 2] - e[r0 + 1]; vt[ty].w = e[r0 + 1] - e[r0 + 3];
    }
  };
  auto stage_v = [&](int st, int b, int ty) {
    float* Vs = lds + st * 2 * WC_OPER + WC_OPER;
    *reinterpret_cast<nhmc_v4f*>(Vs + vw + ty * 32 * 16 + ((b ^ vswz) << 2)) = vt[ty];
  };
  auto stage_u = [&](int st, int i) { *reinterpret_cast<nhmc_v4f*>(lds + st * 2 * WC_OPER + uw + 1024 * i) = ur[i]; };
  auto stage_part = [&](int st, int b) {
    stage_rows(b, 0, 6);
    stage_cols();
    stage_v(st, b, 0);
    stage_v(st, b, 1);
    stage_u(st, 2 * b);
    stage_u(st, 2 * b + 1);
  };

  const int chunks = C / WC_CHUNK;
  f32x16 acc[16];
#pragma unroll
  for (int f = 0; f < 16; ++f)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[f][r] = 0.0f;

  // one chunk: 8 units of 8 MFMAs (k-step u / 2, frequencies 8 (u & 1) .. + 7 = granules 2 (u & 1), + 1 of the lane's A and B
  // rows); the operands of unit u + 1 are read from LDS before the MFMAs of unit u issue (units 0 .. 2, 7) or behind its
  // first two (units 3 .. 6).  The following chunk is staged between the MFMAs of units 3 .. 6; the workgroup meets between units 6 and 7, when unit 7's operands are in registers, so that the
  // first operands of the following chunk are read behind the MFMAs of unit 7 and no MFMA waits on the read before it
  const int swz = wc_swz(lr);
  const int arow = (lh * 64 + kh * 32 + lr) * 16, brow = WC_OPER + (lh * 64 + th * 32 + lr) * 16;
  float av[2][8], bv[2][8];
  auto fetch_half = [&](int st, int u, int g, float (&fa)[8], float (&fb)[8]) {       // MFMAs 4 g .. 4 g + 3 of unit u
    const float* S = lds + st * 2 * WC_OPER + (u >> 1) * 2 * 64 * 16;
    const int go = ((2 * (u & 1) + g) ^ swz) << 2;
    const nhmc_v4f va = *reinterpret_cast<const nhmc_v4f*>(S + arow + go);
    const nhmc_v4f vb = *reinterpret_cast<const nhmc_v4f*>(S + brow + go);
    fa[4 * g + 0] = va.x; fa[4 * g + 1] = va.y; fa[4 * g + 2] = va.z; fa[4 * g + 3] = va.w;
    fb[4 * g + 0] = vb.x; fb[4 * g + 1] = vb.y; fb[4 * g + 2] = vb.z; fb[4 * g + 3] = vb.w;
  };
  auto fetch = [&](int st, int u, float (&fa)[8], float (&fb)[8]) {
    fetch_half(st, u, 0, fa, fb);
    fetch_half(st, u, 1, fa, fb);
  };
  // The loads of chunk `cl` are spread over the gaps between the MFMAs of the four units that follow the barrier, at most two
  // per gap, instead of all of them behind the barrier (where the four waves of the CU, released together, queued them on
  // the one address path and no MFMA issued until the last was accepted): unit 7 the patch's rows 0 - 2, unit 0 of the next
  // body its rows 3 - 5 and U pieces 0, 1, unit 1 pieces 2 - 5, unit 2 pieces 6, 7.  Every gap is fenced, so the placement
  // is the scheduler's too
  auto unit_loading = [&](int u, int cl) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int f = 8 * (u & 1) + j;
      if (!TAIL || !idle) acc[f] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[u & 1][j], bv[u & 1][j], acc[f], 0, 0, 0);
      if (u == 7) issue_loads(cl, (NP / 2 * j) / 8, (NP / 2 * (j + 1)) / 8);         // rows 0 - 2: 6 or 3 loads over 8 gaps
      if (u == 0 && j < 6) issue_loads(cl, NP / 2 + (NP / 2 * j) / 6, NP / 2 + (NP / 2 * (j + 1)) / 6);   // rows 3 - 5
      if (u == 0 && j >= 6) issue_loads(cl, NP - 6 + j, NP - 5 + j);                 // pieces 0, 1
      if (u == 1 && (j & 1) == 0) issue_loads(cl, NP + 2 + j / 2, NP + 3 + j / 2);   // pieces 2 .. 5
      if (u == 2 && (j == 0 || j == 2)) issue_loads(cl, NP + 6 + j / 2, NP + 7 + j / 2);   // pieces 6, 7
      __builtin_amdgcn_sched_barrier(0);
    }
  };

  // Units 3 .. 6 stage column u - 3 of V and U pieces 2 (u - 3), + 1 of the following chunk into stage st ^ 1 and read the
  // operands of unit u + 1, every gap fenced as above.  Left to the scheduler, the four stores, the four reads and the
  // arithmetic all went into the unit's first four gaps, and the four waves, released by one barrier, met on the LDS
  // store-data path (13 cycles per ds_write_b128, shared by two SIMDs).  Here a gap holds at most one store, with the
  // arithmetic that feeds it in front, and the reads sit in the two gaps that hold none: gap 0 (behind the exchange of the
  // patch, in unit 3) and gap 1, the row differences in gaps 1 and 2, the V stores in gaps 3 and 4, the U stores in 5 and 6
  auto unit_staging = [&](int u, int st, int ch) {
    const int b = u - 3;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int f = 8 * (u & 1) + j;
      if (u == 4 && (j & 1)) WC_T32(13 + j / 2);
      if (!TAIL || !idle) acc[f] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[u & 1][j], bv[u & 1][j], acc[f], 0, 0, 0);
      if (j == 0 && u == 3) {
        WC_T32(7);
        pin_patch();
        exchange_patch();
        WC_T32(8);
      }
      if (j < 2) fetch_half(st, u + 1, j, av[(u + 1) & 1], bv[(u + 1) & 1]);
      if (j == 1) stage_rows(b, 0, 3);
      if (j == 2) stage_rows(b, 3, 6);
      if (j == 3) stage_cols();
      if (j == 3 || j == 4) stage_v(st ^ 1, b, j - 3);
      if (j == 5 || j == 6) stage_u(st ^ 1, 2 * b + j - 5);
      __builtin_amdgcn_sched_barrier(0);
    }
  };

  issue_loads(0, 0, NP + 8);
  exchange_patch();
#pragma unroll
  for (int b = 0; b < 4; ++b) stage_part(0, b);
  __syncthreads();
  WC_T64(1);
  int cl = 1 < chunks ? 1 : 0;                      // the chunk being loaded
  issue_loads(cl, 0, NP / 2);
  fetch(0, 0, av[0], bv[0]);
  // ONE instance of the chunk body (a second one behind the loop made the register allocator shuffle the 256 accumulators
  // through scratch): the last chunk stages itself once more into the idle buffer and reads unit 0 of it, which nobody
  // uses.  do-while: the accumulators reach the epilogue from the loop only (C >= 8), not merged with their zero state
  int ch = 0, st = 0;
  WC_T64(2);
  WC_R64(5);
  do {
#pragma unroll
    for (int u = 0; u < 7; ++u) {
      WC_T32(u);
      if (u < 3) {
        fetch(st, u + 1, av[(u + 1) & 1], bv[(u + 1) & 1]);
        __builtin_amdgcn_sched_barrier(0);
        unit_loading(u, cl);
      } else {
        unit_staging(u, st, ch);
      }
    }
    WC_T32(9);
    __syncthreads();                                // stage st ^ 1 is complete, and every wave is done reading stage st
    WC_T32(10);
    st ^= 1;
    cl = ch + 2 < chunks ? ch + 2 : chunks - 1;
    WC_T32(11);
    fetch(st, 0, av[0], bv[0]);
    __builtin_amdgcn_sched_barrier(0);
    unit_loading(7, cl);
    WC_T32(12);
  } while (++ch < chunks);
  WC_T64(3);
  WC_R64(6);

  // ---- Y = A^T M A per (channel, tile), epilogue, row segments of 8 TC bytes (TC / 2 lanes x float4).  bias and add are loaded
  // for all 16 channels of the lane before the transform (the loaders' registers are free), behind one wait
  if (TAIL && idle) return;
  const int oh = h0 + 4 * (lr / TC) + 2 * th, ow = w0 + 2 * (lr % TC);
  const bool has_bias = a.bias != nullptr, has_add = a.add != nullptr;
  const int k0 = kb * WC_KBLK + kh * 32 + 4 * lh;
  // the lane's 2 x 2 patch and that of lane lr ^ 1, two columns further, are exchanged by halves (DPP, within the quad): the
  // even lane stores row 0 and the odd lane row 1 of both, four adjacent columns = one 16-byte store per channel
  const bool odd = lr & 1;
  const int64_t at0 = (((int64_t)n * K + k0) * H + oh) * W + ow + (odd ? W - 2 : 0);
  float bc[16];
  nhmc_v4f ad[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    bc[r] = 0.0f;
    ad[r] = nhmc_v4f{0.0f, 0.0f, 0.0f, 0.0f};
  }
  if (has_bias) {
#pragma unroll
    for (int r = 0; r < 16; ++r) bc[r] = a.bias[k0 + (r & 3) + 8 * (r >> 2)];
  }
  if (has_add) {
#pragma unroll
    for (int r = 0; r < 16; ++r)
      ad[r] = *reinterpret_cast<const nhmc_v4f*>(a.add + at0 + (int64_t)((r & 3) + 8 * (r >> 2)) * HW);
  }
  auto neighbour = [](float v) {                    // lane ^ 1's value: quad_perm [1, 0, 3, 2]
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xB1, 0xF, 0xF, false));
  };
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    float t[2][4];
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      t[0][b] = (acc[4 * b + 0][r] + acc[4 * b + 1][r]) + acc[4 * b + 2][r];
      t[1][b] = (acc[4 * b + 1][r] - acc[4 * b + 2][r]) - acc[4 * b + 3][r];
    }
    wc_v2f o[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      o[i].x = (t[i][0] + t[i][1]) + t[i][2];
      o[i].y = (t[i][1] - t[i][2]) - t[i][3];
      o[i].x = has_bias ? o[i].x + bc[r] : o[i].x;
      o[i].y = has_bias ? o[i].y + bc[r] : o[i].y;
    }
    const wc_v2f keep = odd ? o[1] : o[0], send = odd ? o[0] : o[1];
    const wc_v2f got = {neighbour(send.x), neighbour(send.y)};
    nhmc_v4f v;
    v.x = odd ? got.x : keep.x; v.y = odd ? got.y : keep.y; v.z = odd ? keep.x : got.x; v.w = odd ? keep.y : got.y;
    if (has_add) v += ad[r];
    __builtin_nontemporal_store(v, reinterpret_cast<nhmc_v4f*>(a.y + at0 + (int64_t)((r & 3) + 8 * (r >> 2)) * HW));
  }
  WC_T64(4);
#ifdef NHMC_WINO_STAMPS
  if (nhmc_wino_stamps && lane == 0) {
    unsigned long long* out = nhmc_wino_stamps + ((size_t)blockIdx.x * 4 + wave) * 24;
#pragma unroll
    for (int i = 0; i < 7; ++i) out[i] = t64[i];
#pragma unroll
    for (int i = 0; i < 17; ++i) out[7 + i] = t32[i];
  }
#endif
}

// ---- the eight-wave geometry of the wide kernel (TC = 32, K % 64 == 0): 512 threads, two waves per SIMD ----------------------
// Wave (fh, kh, th), fh = wave >> 2, holds the same 32 channels x 32 tiles as wave (kh, th) above, for the 8 frequencies
// 8 fh .. 8 fh + 7 only: acc[8], 128 registers, so that waves w and w + 4, the two frequency halves of one (kh, th), are
// resident on one SIMD and each issues into the waits, the transform arithmetic and the load issue of the other.  A chunk is
// 4 units of 8 MFMAs per wave: unit v is k-step v at the wave's frequency half (granules 2 fh, 2 fh + 1 of the operand
// rows).  The LDS layout, the swizzle, the MFMA and every per-frequency chain over the channels are those of the four-wave
// kernel, so every M_f has its bits.
// Loader: thread (lc, lt, ty = tid >> 8) transforms channel lc of the chunk for the ONE tile of tile column lt in tile row
// ty: rows 2 ty .. 2 ty + 3 of the column's 6 x 4 patch (rows 2 and 3 are loaded by both threads of a column), one V granule
// per column b with the expressions of the four-wave loader, and U pieces 2 i + ty, i = 0 .. 3.
// Epilogue: Y = A^T M A needs all 16 frequencies of a channel row in one lane.  The two waves of a pair hold the same
// (channel rows, tile) in the same lane, so they exchange halves through LDS lane by lane: wave fh = 0 keeps accumulator
// registers r = 0 .. 7 (channel rows (r & 3) + 8 (r >> 2) of the lane) and sends r = 8 .. 15, wave fh = 1 the reverse.  A wave
// writes the float4 (frequency j of its half, registers 4 q .. + 3 of the half it sends) at float4 index
// (16 wave + 2 j + q) * 64 + lane and reads its partner's at (16 (wave ^ 4) + 2 j + q) * 64 + lane: 8 x 16 x 64 float4 are
// the 128 KB of the operand stages, every ds_write_b128 / ds_read_b128 lane group is contiguous
// (tests/test_wino_exchange_cpu.py).  Each wave then runs the four-wave transform expression on its 8 channel rows.
constexpr int WC8_XSLOTS = 16;                   // float4 per lane and wave in the exchange: 8 frequencies x 2 register quads

// ADD_BIAS: add arrives without its per-channel bias a.add_bias (file header, "Skip bias").
// IN_UP, ADD_UP, OUT_POOL: the forms next to a nearest 2x upsample (file header, "Nearest 2x upsample"): x, add or y at half
// the resolution.  All false is the kernel described above, instruction for instruction.
template <bool IN_UP = false, bool ADD_UP = false, bool OUT_POOL = false, bool ADD_BIAS = false>
__global__ __launch_bounds__(512, 2) void k_conv3x3_wino8(const WinoArgs a) {
  static_assert(!(OUT_POOL && ADD_UP), "the pooled epilogue takes no add");
  static_assert(!ADD_BIAS || !(IN_UP || ADD_UP || OUT_POOL), "the skip bias goes with a full-resolution add");
  constexpr int TC = 32, BLK_ROWS = 128 / TC, BLK_COLS = 2 * TC;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 31, lh = lane >> 5;
  const int kh = wave & 1, th = (wave >> 1) & 1;
  const int fh = __builtin_amdgcn_readfirstlane(wave >> 2);
  const int C = a.C, K = a.K, H = a.H, W = a.W, HW = H * W;
  const int XW = IN_UP ? W >> 1 : W, XHW = IN_UP ? HW >> 2 : HW;      // row and plane of x: IN_UP reads the low-res tensor
#ifdef NHMC_WINO_STAMPS
  unsigned long long t64[7] = {};
  unsigned t32[17] = {};
  const int stamp_ch = nhmc_wino_stamp_chunk < C / WC_CHUNK ? nhmc_wino_stamp_chunk : C / WC_CHUNK - 1;
#endif
  WC_T64(0);

  const int total = gridDim.x;
  int logical = blockIdx.x;
  if ((total & 7) == 0) logical = (logical & 7) * (total >> 3) + (logical >> 3);
  const int kblocks = K / WC_KBLK;
  const int kb = logical % kblocks, sp = logical / kblocks;
  const int cb = sp % a.col_blocks, rb = (sp / a.col_blocks) % a.row_blocks, n = sp / (a.col_blocks * a.row_blocks);
  const int h0 = rb * BLK_ROWS, w0 = cb * BLK_COLS;

  // ---- loader roles.  The patch's columns and the lane exchange are the four-wave loader's; q = 0 .. 3 is row 2 ty + q of
  // the column's patch, image row h0 - 1 + 2 ty + q
  const int ty = tid >> 8, t8 = tid & 255, lc = t8 >> 5, lt = tid & 31;
  unsigned voff[4], eoff[4];
  unsigned okmask = 0;
  const int ecol = lt == 0 ? w0 - 1 : w0 + 2 * TC;
  const bool eok = (lt == 0 || lt == TC - 1) && (unsigned)ecol < (unsigned)W;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int row = h0 + 2 * ty - 1 + q;
    const bool rok = (unsigned)row < (unsigned)H;
    if (IN_UP) {                                         // row >> 1, column >> 1 of the low-res tensor; one dword per row
      voff[q] = rok ? 4u * (unsigned)(lc * XHW + (row >> 1) * XW + (w0 >> 1) + lt) : 0u;
      eoff[q] = rok ? 4u * (unsigned)(lc * XHW + (row >> 1) * XW + (eok ? ecol >> 1 : (w0 >> 1) + lt)) : 0u;
    } else {
      voff[q] = rok ? 4u * (unsigned)(lc * HW + row * W + w0 + 2 * lt) : 0u;
      eoff[q] = rok ? 4u * (unsigned)(lc * HW + row * W + (eok ? ecol : w0 + 2 * lt)) : 0u;
    }
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int col = w0 + 2 * lt - 1 + s;
      const bool ok = rok && (unsigned)col < (unsigned)W;
      okmask |= ok ? 1u << (q * 4 + s) : 0u;
    }
  }
  const float* xn = a.x + (int64_t)n * C * XHW;
  const char* un = reinterpret_cast<const char*>(a.U + (int64_t)kb * WC_KBLK * 16);
  const unsigned uoff = 16u * t8 + (unsigned)ty * (unsigned)K * 64u;                // float4 t8 of piece 2 i + ty
  const int uw = (t8 & ~3) * 4 + (((t8 & 3) ^ wc_swz(t8 >> 2)) << 2) + 1024 * ty;
  const int vw = (lc * 64 + 32 * ty + lt) * 16, vswz = wc_swz(lt);                  // row lc * 64 + 32 ty + lt

  // A chunk's 12 loads per thread: 0 .. 7 the patch (row q = i >> 1: its 8-byte load, then its edge load), 8 .. 11 U pieces
  wc_v2f xm[4];
  float xl[4], xq[4], xe[4], xu[4];                      // xu: IN_UP's one dword per row, both middle columns
  nhmc_v4f ur[4];
  auto load_one = [&](int ch, int i) {
    if (i < 8) {
      const char* xs = reinterpret_cast<const char*>(xn + (int64_t)ch * WC_CHUNK * XHW);
      const int q = i >> 1;
      if (IN_UP && q == 2) return;                       // rows 1 and 2 of the patch are one low-res row
      unsigned off = (i & 1) ? eoff[q] : voff[q];
      asm volatile("" : "+v"(off));
      if (i & 1) xe[q] = *reinterpret_cast<const float*>(xs + off);
      else if (IN_UP) xu[q] = *reinterpret_cast<const float*>(xs + off);
      else xm[q] = *reinterpret_cast<const wc_v2f*>(xs + off);
    } else {
      const char* us = un + (int64_t)ch * WC_CHUNK * K * 64 + (int64_t)(2 * (i - 8)) * K * 64;
      unsigned off = uoff;
      asm volatile("" : "+v"(off));
      ur[i - 8] = *reinterpret_cast<const nhmc_v4f*>(us + off);
    }
  };
  auto issue_loads = [&](int ch, int first, int last) {
#pragma unroll
    for (int i = first; i < last; ++i) load_one(ch, i);
  };
  auto pin_patch = [&]() {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if (IN_UP && q == 2) continue;
      if (IN_UP) asm volatile("" : "+v"(xu[q]));
      else asm volatile("" : "+v"(xm[q]));
      asm volatile("" : "+v"(xe[q]));
    }
  };
  auto exchange_patch = [&]() {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if (IN_UP && q == 2) continue;
      if (IN_UP) xm[q] = wc_v2f{xu[q], xu[q]};
      xl[q] = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(xm[q].y), 0x138, 0xF, 0xF, false));
      xq[q] = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(xm[q].x), 0x130, 0xF, 0xF, false));
      xl[q] = lt == 0 ? xe[q] : xl[q];
      xq[q] = lt == TC - 1 ? xe[q] : xq[q];
    }
  };
  auto d = [&](int q0, int s) {
    const int q = IN_UP && q0 == 2 ? 1 : q0;             // IN_UP: row 2 IS row 1, values and padding mask
    const float v = s == 0 ? xl[q] : s == 1 ? xm[q].x : s == 2 ? xm[q].y : xq[q];
    return (okmask >> (q * 4 + s)) & 1u ? v : 0.0f;
  };
  float e[4];
  auto stage_rows = [&](int b) {
    if (IN_UP && b == 2) return;
#pragma unroll
    for (int q = 0; q < 4; ++q)
      e[q] = b == 0 ? d(q, 0) - d(q, 2) : b == 1 ? d(q, 1) + d(q, 2) : b == 2 ? d(q, 2) - d(q, 1) : d(q, 1) - d(q, 3);
  };
  nhmc_v4f vt;
  auto stage_cols = [&](int b = 0) {
    if (IN_UP && b == 2) return;
    vt.x = e[0] - e[2]; vt.y = e[1] + e[2]; vt.z = e[2] - e[1]; vt.w = e[1] - e[3];
  };
  auto stage_v = [&](int st, int b) {
    if (IN_UP && b == 2) return;                         // column 2 of V is +0 throughout: neither formed, stored nor read
    *reinterpret_cast<nhmc_v4f*>(lds + st * 2 * WC_OPER + WC_OPER + vw + ((b ^ vswz) << 2)) = vt;
  };
  auto stage_u = [&](int st, int i) { *reinterpret_cast<nhmc_v4f*>(lds + st * 2 * WC_OPER + uw + 2048 * i) = ur[i]; };

  const int chunks = C / WC_CHUNK;
  f32x16 acc[8];
#pragma unroll
  for (int j = 0; j < 8; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[j][r] = 0.0f;

  const int swz = wc_swz(lr);
  const int arow = (lh * 64 + kh * 32 + lr) * 16, brow = WC_OPER + (lh * 64 + th * 32 + lr) * 16;
  const int go[2] = {((2 * fh) ^ swz) << 2, ((2 * fh + 1) ^ swz) << 2};              // the wave's two granules of a row
  float av[2][8], bv[2][8];
  auto fetch_half = [&](int st, int v, int g, float (&fa)[8], float (&fb)[8]) {      // MFMAs 4 g .. 4 g + 3 of unit v
    const float* S = lds + st * 2 * WC_OPER + v * 2 * 64 * 16;
    const nhmc_v4f va = *reinterpret_cast<const nhmc_v4f*>(S + arow + go[g]);
    const nhmc_v4f vb = *reinterpret_cast<const nhmc_v4f*>(S + brow + go[g]);
    fa[4 * g + 0] = va.x; fa[4 * g + 1] = va.y; fa[4 * g + 2] = va.z; fa[4 * g + 3] = va.w;
    fb[4 * g + 0] = vb.x; fb[4 * g + 1] = vb.y; fb[4 * g + 2] = vb.z; fb[4 * g + 3] = vb.w;
  };
  // One unit: 8 MFMAs, every gap fenced.  Gaps 0 and 1 read the operands of the following unit (unit 3: unit 0 of stage
  // `st`, which the caller has flipped behind the barrier) and hold no store.  Units 1 and 2 stage columns 2 (v - 1), + 1 of
  // V and U pieces v - 1, v + 1 of the following chunk into stage st ^ 1, at most one store per gap with the arithmetic that
  // feeds it in front: the exchange of the patch in gap 0 of unit 1, row differences in gaps 1 and 4, the V stores in gaps 3
  // and 5, the U stores in gaps 6 and 7.  The patch of chunk `cl`, two chunks ahead, is loaded as soon as the staging has
  // read the last one: rows 0 - 2 in gaps 5 - 7 of unit 2, in front of the barrier (which waits for LDS only, so they stay in
  // flight across it), row 3 in gaps 0 and 1 of unit 3; its 4 U pieces follow in gaps 1, 3, 5, 7 of unit 0.  Issued behind
  // the barrier, one per gap of unit 3, the patch cost 2 % of the kernel (with the priority below; without it, nothing)
  int ch = 0;                                       // the chunk being multiplied
  auto unit = [&](int v, int st, int cl) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      // IN_UP: the frequencies with a == 2 (j = 2, 6) or b == 2 (j = 0 .. 3 of the upper half) have V = +0: no MFMA; fh is
      // a scalar, so the upper half's j < 4 is one uniform branch, and that half never reads granule 2
      if constexpr (IN_UP) {
        if (j != 2 && j != 6 && (j >= 4 || fh == 0))
          acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[v & 1][j], bv[v & 1][j], acc[j], 0, 0, 0);
      } else {
        acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[v & 1][j], bv[v & 1][j], acc[j], 0, 0, 0);
      }
      if (j == 0 && v == 1) {
        WC_T32(7);
        pin_patch();
        exchange_patch();
        WC_T32(8);
      }
      if constexpr (IN_UP) {
        if (j == 1 || (j == 0 && fh == 0)) fetch_half(st, (v + 1) & 3, j, av[(v + 1) & 1], bv[(v + 1) & 1]);
      } else {
        if (j < 2) fetch_half(st, (v + 1) & 3, j, av[(v + 1) & 1], bv[(v + 1) & 1]);
      }
      if (v == 2 && j >= 5) issue_loads(cl, 2 * (j - 5), 2 * (j - 5) + 2);
      if (v == 3 && j < 2) issue_loads(cl, 6 + j, 7 + j);
      if (v == 0 && (j & 1)) issue_loads(cl, 8 + j / 2, 9 + j / 2);
      if (v == 1 || v == 2) {
        const int b = 2 * (v - 1);
        if (j == 1) stage_rows(b);
        if (j == 2) stage_cols(b);
        if (j == 3) stage_v(st ^ 1, b);
        if (j == 4) { stage_rows(b + 1); stage_cols(); }
        if (j == 5) stage_v(st ^ 1, b + 1);
        if (j == 6) stage_u(st ^ 1, v - 1);
        if (j == 7) stage_u(st ^ 1, v + 1);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
  };

  issue_loads(0, 0, 12);
  exchange_patch();
#pragma unroll
  for (int b = 0; b < 4; ++b) {
    stage_rows(b);
    stage_cols(b);
    stage_v(0, b);
    stage_u(0, b);
  }
  __syncthreads();
  WC_T64(1);
  int cl = 1 < chunks ? 1 : 0;
  issue_loads(cl, 0, 8);
  if constexpr (IN_UP) {
    if (fh == 0) fetch_half(0, 0, 0, av[0], bv[0]);
  } else {
    fetch_half(0, 0, 0, av[0], bv[0]);
  }
  fetch_half(0, 0, 1, av[0], bv[0]);
  // ONE instance of the chunk body, as in the four-wave kernel: the last chunk stages itself once more into the idle buffer.
  // One barrier per chunk, between units 2 and 3, when unit 3's operands are in registers: the first operands of the
  // following chunk are read behind the first MFMAs of unit 3.
  // The two waves of a SIMD run the same stream in lockstep.  Waves 4 - 7, dispatched second, lose every arbitration of the
  // SIMD's issue to their partners; one static s_setprio 1 for them in front of the loop, with the early patch loads above,
  // is worth 2 % of the kernel (neither alone is outside the run-to-run spread; profiles/r12_wino_waves_ab.txt)
  int st = 0;
  if (fh) __builtin_amdgcn_s_setprio(1);
  WC_T64(2);
  WC_R64(5);
  do {
#pragma unroll
    for (int v = 0; v < 3; ++v) {
      WC_T32(v);
      if (v == 2) cl = ch + 2 < chunks ? ch + 2 : chunks - 1;
      unit(v, st, cl);
    }
    WC_T32(9);
    __syncthreads();                                // stage st ^ 1 is complete, and every wave is done reading stage st
    WC_T32(10);
    st ^= 1;
    WC_T32(3);
    unit(3, st, cl);
    WC_T32(12);
  } while (++ch < chunks);
  WC_T64(3);
  WC_R64(6);

  // ---- the exchange, then Y = A^T M A for the wave's 8 channel rows per lane: rows (r & 3) + 8 (r >> 2), r = 8 fh + rr
  const int oh = h0 + 2 * th, ow = w0 + 2 * lr;
  const bool has_bias = a.bias != nullptr, has_add = a.add != nullptr;
  const int k0 = kb * WC_KBLK + kh * 32 + 4 * lh + 16 * fh;
  const bool odd = lr & 1;
  const int64_t at0 = (((int64_t)n * K + k0) * H + oh) * W + ow + (odd ? W - 2 : 0);
  // ADD_UP: add is [n][K][H / 2][W / 2]; the two low-res values under the lane's four output columns.  OUT_POOL: y is
  // [n][K][H / 2][W / 2]; the lane's 2 x 2 patch is its pixel (oh / 2, ow / 2)
  const int64_t lt0 = !(ADD_UP || OUT_POOL) ? 0 : (((int64_t)n * K + k0) * (H >> 1) + (oh >> 1)) * (W >> 1) + (OUT_POOL ? ow >> 1 : (ow >> 1) - (odd ? 1 : 0));
  float bc[8];
  nhmc_v4f ad[8];
  wc_v2f al[8];
#pragma unroll
  for (int rr = 0; rr < 8; ++rr) {
    bc[rr] = 0.0f;
    ad[rr] = nhmc_v4f{0.0f, 0.0f, 0.0f, 0.0f};
    al[rr] = wc_v2f{0.0f, 0.0f};
  }
  if (has_bias) {
#pragma unroll
    for (int rr = 0; rr < 8; ++rr) bc[rr] = a.bias[k0 + (rr & 3) + 8 * (rr >> 2)];
  }
  // ADD_BIAS: the wave's 16 channels k0 - 4 lh .. + 15 at a wave-uniform address, so they sit in scalar registers (the
  // epilogue has no eight vector registers to spare); a lane's row rr is entry 4 lh + (rr & 3) + 8 (rr >> 2)
  // (read through the constant address space, which nothing writes while the kernel runs: scalar loads)
  typedef const __attribute__((address_space(4))) float* wc_cptr;
  const wc_cptr sbp = (wc_cptr)(uintptr_t)a.add_bias + (kb * WC_KBLK + __builtin_amdgcn_readfirstlane(kh) * 32 + 16 * fh);
  float sb[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) sb[j] = ADD_BIAS ? sbp[j] : 0.0f;
  if (has_add) {
#pragma unroll
    for (int rr = 0; rr < 8; ++rr) {
      if (ADD_UP) al[rr] = *reinterpret_cast<const wc_v2f*>(a.add + lt0 + (int64_t)((rr & 3) + 8 * (rr >> 2)) * (HW >> 2));
      else ad[rr] = *reinterpret_cast<const nhmc_v4f*>(a.add + at0 + (int64_t)((rr & 3) + 8 * (rr >> 2)) * HW);
    }
  }
  nhmc_v4f* xch = reinterpret_cast<nhmc_v4f*>(lds);
  const int xw = wave * WC8_XSLOTS * 64 + lane, xr = (wave ^ 4) * WC8_XSLOTS * 64 + lane;
  __syncthreads();                                  // every wave has left the loop: the operand stages are free
  auto send = [&](auto half) {                      // the 8 registers of each frequency that the partner transforms
    constexpr int RS = decltype(half)::value ? 0 : 8;
#pragma unroll
    for (int j = 0; j < 8; ++j)
#pragma unroll
      for (int q = 0; q < 2; ++q)
        xch[xw + (2 * j + q) * 64] = nhmc_v4f{acc[j][RS + 4 * q], acc[j][RS + 4 * q + 1], acc[j][RS + 4 * q + 2], acc[j][RS + 4 * q + 3]};
  };
  if (fh == 0) send(std::integral_constant<int, 0>{});
  else send(std::integral_constant<int, 1>{});
  __syncthreads();
  nhmc_v4f got[8][2];                               // the partner's frequencies, registers 8 fh + 4 q .. + 3
#pragma unroll
  for (int j = 0; j < 8; ++j)
#pragma unroll
    for (int q = 0; q < 2; ++q) got[j][q] = xch[xr + (2 * j + q) * 64];
  auto neighbour = [](float v) {                    // lane ^ 1's value: quad_perm [1, 0, 3, 2]
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xB1, 0xF, 0xF, false));
  };
  auto finish = [&](auto half) {
    constexpr int F = decltype(half)::value, RK = 8 * F;
    auto M = [&](int f, int rr) { return (f >> 3) == F ? acc[f & 7][RK + rr] : got[f & 7][rr >> 2][rr & 3]; };
#pragma unroll
    for (int rr = 0; rr < 8; ++rr) {
      float t[2][4];
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        t[0][b] = (M(4 * b + 0, rr) + M(4 * b + 1, rr)) + M(4 * b + 2, rr);
        t[1][b] = (M(4 * b + 1, rr) - M(4 * b + 2, rr)) - M(4 * b + 3, rr);
      }
      wc_v2f o[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        o[i].x = (t[i][0] + t[i][1]) + t[i][2];
        o[i].y = (t[i][1] - t[i][2]) - t[i][3];
        o[i].x = has_bias ? o[i].x + bc[rr] : o[i].x;
        o[i].y = has_bias ? o[i].y + bc[rr] : o[i].y;
      }
      if (OUT_POOL) {                                  // k_sr<2, 1>'s block mean, then _Resample2x.backward's mul_(4.0)
        const float pooled = ((((0.0f + o[0].x) + o[0].y) + o[1].x) + o[1].y) * 0.25f * 4.0f;
        __builtin_nontemporal_store(pooled, a.y + lt0 + (int64_t)((rr & 3) + 8 * (rr >> 2)) * (HW >> 2));
        continue;
      }
      const wc_v2f keep = odd ? o[1] : o[0], give = odd ? o[0] : o[1];
      const wc_v2f recv = {neighbour(give.x), neighbour(give.y)};
      nhmc_v4f v;
      v.x = odd ? recv.x : keep.x; v.y = odd ? recv.y : keep.y; v.z = odd ? keep.x : recv.x; v.w = odd ? keep.y : recv.y;
      if (ADD_BIAS) v += ad[rr] + (lh ? sb[4 + (rr & 3) + 8 * (rr >> 2)] : sb[(rr & 3) + 8 * (rr >> 2)]);            // (acc + bias) + (add + add_bias): the bias pass's own add, then today's
      else if (has_add) v += ADD_UP ? nhmc_v4f{al[rr].x, al[rr].x, al[rr].y, al[rr].y} : ad[rr];
      __builtin_nontemporal_store(v, reinterpret_cast<nhmc_v4f*>(a.y + at0 + (int64_t)((rr & 3) + 8 * (rr >> 2)) * HW));
    }
  };
  __builtin_amdgcn_sched_barrier(0);
  if (fh == 0) finish(std::integral_constant<int, 0>{});
  else finish(std::integral_constant<int, 1>{});
  WC_T64(4);
#ifdef NHMC_WINO_STAMPS
  if (nhmc_wino_stamps && lane == 0) {
    unsigned long long* out = nhmc_wino_stamps + ((size_t)blockIdx.x * 8 + wave) * 24;
#pragma unroll
    for (int i = 0; i < 7; ++i) out[i] = t64[i];
#pragma unroll
    for (int i = 0; i < 17; ++i) out[7 + i] = t32[i];
  }
#endif
}

// U[ci][ko][f = 4 b + a] = (G g G^T)[a][b], G = [1 0 0; 1/2 1/2 1/2; 1/2 -1/2 1/2; 0 0 1].
// forward: (ci, ko) = (c, k), g = w[k][c];  backward-data: (ci, ko) = (k, c), g[r][s] = w[k][c][2 - r][2 - s].
__global__ __launch_bounds__(NHMC_BLOCK) void k_wino_weights(const float* __restrict__ w, float* __restrict__ U, int C, int K,
                                                             int backward) {
  const int CI = backward ? K : C, KO = backward ? C : K;
  const int idx = blockIdx.x * NHMC_BLOCK + threadIdx.x;
  if (idx >= CI * KO) return;
  const int ci = idx / KO, ko = idx % KO;
  const float* g = w + (int64_t)(backward ? ci * C + ko : ko * C + ci) * 9;
  float t[4][3];
#pragma unroll
  for (int s = 0; s < 3; ++s) {
    const float g0 = g[backward ? 8 - s : s], g1 = g[backward ? 5 - s : 3 + s], g2 = g[backward ? 2 - s : 6 + s];
    t[0][s] = g0; t[1][s] = 0.5f * ((g0 + g1) + g2); t[2][s] = 0.5f * ((g0 - g1) + g2); t[3][s] = g2;
  }
  nhmc_v4f u[4];                                     // u[b] = the four vertical frequencies a of horizontal frequency b
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    u[0][r] = t[r][0];
    u[1][r] = 0.5f * ((t[r][0] + t[r][1]) + t[r][2]);
    u[2][r] = 0.5f * ((t[r][0] - t[r][1]) + t[r][2]);
    u[3][r] = t[r][2];
  }
#pragma unroll
  for (int b = 0; b < 4; ++b) reinterpret_cast<nhmc_v4f*>(U + (int64_t)idx * 16)[b] = u[b];
}

// Geometry by tile-column count: TC = 32 serves every width that is a multiple of 64 (the wide entries), 16 the width 32
// and 8 the width 16 (the narrow entries), one column block each; H must be a multiple of the block's 128 / TC rows.
// KM: what K must be a multiple of, 64 (the entries without a tail block) or 32 (nhmc_conv3x3_wino_k32).
template <int TC, int KM = WC_KBLK>
int wc_covers_tc(int64_t n, int64_t c, int64_t k, int64_t h, int64_t w) {
  constexpr int ROWS = 128 / TC, COLS = 2 * TC;
  if (n <= 0 || c < WC_CHUNK || c % WC_CHUNK || k < KM || k % KM || h < ROWS || h % ROWS || w < COLS || w % COLS)
    return 0;
  if (TC != 32 && w != COLS) return 0;
  if (c > 65536 || k > 65536 || h * w > (1 << 24)) return 0;                     // 32-bit offsets inside a chunk / the weights
  return n * (h / ROWS) * (w / COLS) * ((k + WC_KBLK - 1) / WC_KBLK) < (int64_t)1 << 31;
}

int wc_covers(int64_t n, int64_t c, int64_t k, int64_t h, int64_t w) { return wc_covers_tc<32>(n, c, k, h, w); }

int wc_narrow_covers(int64_t n, int64_t c, int64_t k, int64_t h, int64_t w) {
  return w == 32 ? wc_covers_tc<16>(n, c, k, h, w) : w == 16 ? wc_covers_tc<8>(n, c, k, h, w) : 0;
}

int wc_k32_covers(int64_t n, int64_t c, int64_t k, int64_t h, int64_t w) {
  return w == 32 ? wc_covers_tc<16, 32>(n, c, k, h, w) : w == 16 ? wc_covers_tc<8, 32>(n, c, k, h, w)
                                                                 : wc_covers_tc<32, 32>(n, c, k, h, w);
}

static_assert(WC_ROWS == 128 / 32 && WC_COLS == 2 * 32, "the wide geometry");

struct WcRow { int backward, c, k, res; };

template <int N>
int wc_listed(const WcRow (&table)[N], int backward, int c, int k, int h) {
  for (const WcRow& r : table)
    if (r.backward == (backward != 0) && r.c == c && r.k == k && r.res == h) return 1;
  return 0;
}

// Waves per workgroup, read per call (as NHMC_WINO is in Python): NHMC_WINO_WAVES = 4 or 8, unset = WC_DEFAULT_WAVES.  The
// eight-wave kernel exists for the wide geometry without a tail block; every other instantiation runs on four waves whatever
// the variable says.  -1: the variable holds something else.  Eight waves are the default because they were faster than four
// at 128->128 @ 256^2, 256->256 @ 128^2 and 512->256 @ 64^2, forward and backward-data, by 3.8 - 4.8 % against a
// run-to-run spread of at most 1.1 % (profiles/r12_wino_waves_ab.txt).
constexpr int WC_DEFAULT_WAVES = 8;

int wc_waves() {
  const char* v = std::getenv("NHMC_WINO_WAVES");
  if (!v || !*v) return WC_DEFAULT_WAVES;
  if (v[0] == '4' && !v[1]) return 4;
  if (v[0] == '8' && !v[1]) return 8;
  return -1;
}

template <bool IN_UP = false, bool ADD_UP = false, bool OUT_POOL = false, bool ADD_BIAS = false>
int wc_launch8(const float* x, const float* u, const float* bias, const float* add, float* y, int n, int c, int k, int h, int w,
               nhmc_stream_t stream, const float* add_bias = nullptr) {
  static bool attr_set[64] = {};
  int dev = 0;
  (void)hipGetDevice(&dev);
  if (dev < 0 || dev >= 64 || !attr_set[dev]) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(&k_conv3x3_wino8<IN_UP, ADD_UP, OUT_POOL, ADD_BIAS>),
                            hipFuncAttributeMaxDynamicSharedMemorySize, WC_LDS_BYTES) != hipSuccess)
      return NHMC_ERR_LAUNCH;
    if (dev >= 0 && dev < 64) attr_set[dev] = true;
  }
  const WinoArgs a{x, u, bias, add, y, c, k, h, w, h / WC_ROWS, w / WC_COLS, add_bias};
  const int64_t blocks = (int64_t)n * a.row_blocks * a.col_blocks * (k / WC_KBLK);
  NHMC_LAUNCH((k_conv3x3_wino8<IN_UP, ADD_UP, OUT_POOL, ADD_BIAS>), dim3((unsigned)blocks), dim3(512), WC_LDS_BYTES, nhmc_s(stream), a);
  return nhmc_launch_status();
}

template <int TC, bool TAIL = false>
int wc_launch(const float* x, const float* u, const float* bias, const float* add, float* y, int n, int c, int k, int h, int w,
              nhmc_stream_t stream) {
  const int waves = wc_waves();
  if (waves < 0) return NHMC_ERR_ARG;
  if (TC == 32 && !TAIL && waves == 8) return wc_launch8(x, u, bias, add, y, n, c, k, h, w, stream);
  static bool attr_set[64] = {};                             // raise the dynamic-LDS limit once per device
  int dev = 0;
  (void)hipGetDevice(&dev);
  if (dev < 0 || dev >= 64 || !attr_set[dev]) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(&k_conv3x3_wino<TC, TAIL>), hipFuncAttributeMaxDynamicSharedMemorySize,
                            WC_LDS_BYTES) != hipSuccess)
      return NHMC_ERR_LAUNCH;
    if (dev >= 0 && dev < 64) attr_set[dev] = true;
  }
  const WinoArgs a{x, u, bias, add, y, c, k, h, w, h / (128 / TC), w / (2 * TC)};
  const int64_t blocks = (int64_t)n * a.row_blocks * a.col_blocks * ((k + WC_KBLK - 1) / WC_KBLK);
  NHMC_LAUNCH((k_conv3x3_wino<TC, TAIL>), dim3((unsigned)blocks), dim3(256), WC_LDS_BYTES, nhmc_s(stream), a);
  return nhmc_launch_status();
}

}  // namespace

extern "C" int nhmc_conv3x3_wino_covers(int n, int c, int k, int h, int w) { return wc_covers(n, c, k, h, w); }
extern "C" int nhmc_conv3x3_wino_narrow_covers(int n, int c, int k, int h, int w) { return wc_narrow_covers(n, c, k, h, w); }

// Routing rule: (c, k, h, w) of the convolution that runs (backward-data: c = the gradient's channels, k = the layer's input
// channels).  A (shape, direction) pair is listed only where tools/conv_bench.py measured this kernel at <= 0.90 of
// F.conv2d's time at 64 chains on MI355X in the same process (the figure behind each row is the larger of the median and
// the best-of-rounds ratio): a tie is never routed.  Other batch sizes follow the same rows; only n = 64 was measured.
// The first table holds the 3x3 convolutions of unet.FFHQ_CONFIG (unet.conv3x3_shapes()) with widths that are multiples of
// 64, all measured in one run: profiles/r10_wino_conv_routing.txt.  The second holds shapes that FFHQ_CONFIG never runs;
// they are kept because they are real measurements (profiles/r05_wino_conv_roofline.txt) and serve other channel multipliers.
extern "C" int nhmc_conv3x3_wino_prefers(int backward, int n, int c, int k, int h, int w) {
  if (!wc_covers(n, c, k, h, w) || h != w) return 0;
  static const WcRow network[] = {
      {0, 128, 128, 256},   // 128->128 forward: 0.513
      {1, 128, 128, 256},   // 128->128 backward-data: 0.499
      {0, 256, 128, 256},   // 256->128 forward: 0.503
      {1, 128, 256, 256},   // 256->128 backward-data: 0.500
      {0, 128, 128, 128},   // 128->128 forward: 0.524
      {1, 128, 128, 128},   // 128->128 backward-data: 0.517
      {0, 256, 128, 128},   // 256->128 forward: 0.512
      {1, 128, 256, 128},   // 256->128 backward-data: 0.504
      {0, 256, 256, 128},   // 256->256 forward: 0.527
      {1, 256, 256, 128},   // 256->256 backward-data: 0.516
      {0, 384, 128, 128},   // 384->128 forward: 0.506
      {1, 128, 384, 128},   // 384->128 backward-data: 0.504
      {0, 128, 128, 64},   // 128->128 forward: 0.535
      {1, 128, 128, 64},   // 128->128 backward-data: 0.509
      {0, 128, 256, 64},   // 128->256 forward: 0.526
      {1, 256, 128, 64},   // 128->256 backward-data: 0.507
      {0, 256, 256, 64},   // 256->256 forward: 0.533
      {1, 256, 256, 64},   // 256->256 backward-data: 0.519
      {0, 384, 256, 64},   // 384->256 forward: 0.533
      {1, 256, 384, 64},   // 384->256 backward-data: 0.527
      {0, 512, 256, 64},   // 512->256 forward: 0.532
      {1, 256, 512, 64},   // 512->256 backward-data: 0.533
  };
  static const WcRow elsewhere[] = {           // not in FFHQ_CONFIG
      {0, 384, 128, 256},   // 384->128 forward: 0.696
      {1, 128, 384, 256},   // 384->128 backward-data: 0.684
      {0, 128, 256, 128},   // 128->256 forward: 0.706
      {1, 256, 128, 128},   // 128->256 backward-data: 0.678
      {0, 384, 256, 128},   // 384->256 forward: 0.718
      {1, 256, 384, 128},   // 384->256 backward-data: 0.704
      {0, 512, 256, 128},   // 512->256 forward: 0.722
      {1, 256, 512, 128},   // 512->256 backward-data: 0.716
      {0, 256, 512, 64},   // 256->512 forward: 0.725
      {1, 512, 256, 64},   // 256->512 backward-data: 0.704
      {0, 512, 512, 64},   // 512->512 forward: 0.731
      {1, 512, 512, 64},   // 512->512 backward-data: 0.726
      {0, 768, 256, 64},   // 768->256 forward: 0.715
      {1, 256, 768, 64},   // 768->256 backward-data: 0.709
      {0, 1024, 512, 64},   // 1024->512 forward: 0.734
      {1, 512, 1024, 64},   // 1024->512 backward-data: 0.742
  };
  // latent networks, measured at 16 chains (tools/conv_bench.py --latent, profiles/r10_wino_conv_latent.txt): the shapes of
  // ldm.conv3x3_shapes with K % 64 == 0 that no row above holds.  The score network runs without gradient: forward only
  static const WcRow latent[] = {
      {0, 448, 448, 64},    // U-Net 448->448 forward: 0.505
      {0, 256, 256, 256},   // decoder 256->256 forward: 0.526
      {1, 256, 256, 256},   // decoder 256->256 backward-data: 0.512
      {0, 512, 512, 128},   // decoder 512->512 forward: 0.544
      {1, 512, 512, 128},   // decoder 512->512 backward-data: 0.537
  };
  return wc_listed(network, backward, c, k, h) || wc_listed(elsewhere, backward, c, k, h) || wc_listed(latent, backward, c, k, h);
}

// The narrow geometries (w = 32 and w = 16) under the same rule and from the same run: the network's nine shapes at 32 and 16.
extern "C" int nhmc_conv3x3_wino_narrow_prefers(int backward, int n, int c, int k, int h, int w) {
  if (!wc_narrow_covers(n, c, k, h, w) || h != w) return 0;
  static const WcRow network[] = {
      {0, 256, 256, 32},   // 256->256 forward: 0.491
      {1, 256, 256, 32},   // 256->256 backward-data: 0.490
      {0, 512, 256, 32},   // 512->256 forward: 0.488
      {1, 256, 512, 32},   // 512->256 backward-data: 0.485
      {0, 512, 512, 32},   // 512->512 forward: 0.527
      {1, 512, 512, 32},   // 512->512 backward-data: 0.515
      {0, 768, 256, 32},   // 768->256 forward: 0.487
      {1, 256, 768, 32},   // 768->256 backward-data: 0.510
      {0, 256, 256, 16},   // 256->256 forward: 0.484
      {1, 256, 256, 16},   // 256->256 backward-data: 0.463
      {0, 256, 512, 16},   // 256->512 forward: 0.488
      {1, 512, 256, 16},   // 256->512 backward-data: 0.470
      {0, 512, 512, 16},   // 512->512 forward: 0.484
      {1, 512, 512, 16},   // 512->512 backward-data: 0.475
      {0, 768, 512, 16},   // 768->512 forward: 0.484
      {1, 512, 768, 16},   // 768->512 backward-data: 0.506
      {0, 1024, 512, 16},   // 1024->512 forward: 0.482
      {1, 512, 1024, 16},   // 1024->512 backward-data: 0.518
  };
  // latent networks, measured at 16 chains (profiles/r10_wino_conv_latent.txt): the LDM U-Net's K = 448 / 896 layers, forward
  static const WcRow latent[] = {
      {0, 224, 448, 32},    // 224->448 forward: 0.561
      {0, 448, 448, 32},    // 448->448 forward: 0.544
      {0, 672, 448, 32},    // 672->448 forward: 0.544
      {0, 896, 448, 32},    // 896->448 forward: 0.544
      {0, 1120, 448, 32},   // 1120->448 forward: 0.550
      {0, 896, 896, 16},    // 896->896 forward: 0.470
  };
  return wc_listed(network, backward, c, k, h) || wc_listed(latent, backward, c, k, h);
}

// K % 64 == 32 only; same rule, measured at 16 chains (the latent sampler's chain count) by tools/conv_bench.py --latent:
// profiles/r10_wino_conv_latent.txt.  The rows are the LDM U-Net's K = 224 / 672 layers, forward only (it runs without
// gradient).  At 16 x 16 a tail launch has 16 x 11 = 176 workgroups on 256 CUs, one in eleven of them half empty.
extern "C" int nhmc_conv3x3_wino_k32_covers(int n, int c, int k, int h, int w) { return wc_k32_covers(n, c, k, h, w); }

extern "C" int nhmc_conv3x3_wino_k32_prefers(int backward, int n, int c, int k, int h, int w) {
  if (!wc_k32_covers(n, c, k, h, w) || h != w || k % WC_KBLK == 0) return 0;
  static const WcRow latent[] = {
      {0, 224, 224, 64},    // 224->224 forward: 0.669
      {0, 448, 224, 64},    // 448->224 forward: 0.671
      {0, 672, 224, 64},    // 672->224 forward: 0.669
      {0, 672, 672, 32},    // 672->672 forward: 0.609
      {0, 448, 672, 16},    // 448->672 forward: 0.724
      {0, 672, 672, 16},    // 672->672 forward: 0.728
      {0, 1120, 672, 16},   // 1120->672 forward: 0.718
      {0, 1344, 672, 16},   // 1344->672 forward: 0.722
      {0, 1568, 672, 16},   // 1568->672 forward: 0.727
  };
  return wc_listed(latent, backward, c, k, h);
}

extern "C" int nhmc_wino_weights(const float* weight, float* u, int backward, int channels_in, int channels_out,
                                 nhmc_stream_t stream) {
  if (!weight || !u || (backward != 0 && backward != 1) || channels_in <= 0 || channels_out <= 0) return NHMC_ERR_ARG;
  if (channels_in > 65536 || channels_out > 65536) return NHMC_ERR_SHAPE;
  if (!nhmc_aligned16(u)) return NHMC_ERR_ALIGN;
  const int pairs = channels_in * channels_out;
  NHMC_LAUNCH(k_wino_weights, dim3((unsigned)((pairs + NHMC_BLOCK - 1) / NHMC_BLOCK)), dim3(NHMC_BLOCK), 0, nhmc_s(stream), weight,
              u, channels_in, channels_out, backward);
  return nhmc_launch_status();
}

extern "C" int nhmc_conv3x3_wino(const float* x, const float* u, const float* bias, const float* add, float* y, int n, int c,
                                 int k, int h, int w, int stride, int padding, nhmc_stream_t stream) {
  if (!x || !u || !y || y == x || (add && add == x)) return NHMC_ERR_ARG;
  if (stride != 1 || padding != 1 || !wc_covers(n, c, k, h, w)) return NHMC_ERR_SHAPE;
  if (!nhmc_aligned16(x) || !nhmc_aligned16(u) || !nhmc_aligned16(y) || !nhmc_aligned16(add)) return NHMC_ERR_ALIGN;
  return wc_launch<32>(x, u, bias, add, y, n, c, k, h, w, stream);
}

// The upsample forms of the eight-wave kernel (the paragraph "Nearest 2x upsample" of the file header).  h, w are the
// convolution's own resolution; mode names which tensor is at half of it.
extern "C" int nhmc_conv3x3_wino_up_covers(int n, int c, int k, int h, int w) {
  return wc_covers(n, c, k, h, w) && wc_waves() == 8;
}

extern "C" int nhmc_conv3x3_wino_up(const float* x, const float* u, const float* bias, const float* add, float* y, int n, int c,
                                    int k, int h, int w, int mode, nhmc_stream_t stream) {
  if (!x || !u || !y || y == x || (add && add == x)) return NHMC_ERR_ARG;
  if (mode != NHMC_WINO_IN_UP && mode != NHMC_WINO_ADD_UP && mode != NHMC_WINO_OUT_POOL) return NHMC_ERR_ARG;
  if ((mode == NHMC_WINO_ADD_UP) != (add != nullptr) || (mode == NHMC_WINO_ADD_UP && add == y)) return NHMC_ERR_ARG;
  if (mode == NHMC_WINO_OUT_POOL && bias) return NHMC_ERR_ARG;
  if (wc_waves() < 0) return NHMC_ERR_ARG;
  if (!wc_covers(n, c, k, h, w) || wc_waves() != 8) return NHMC_ERR_SHAPE;
  if (!nhmc_aligned16(x) || !nhmc_aligned16(u) || !nhmc_aligned16(y) || !nhmc_aligned16(add)) return NHMC_ERR_ALIGN;
  return mode == NHMC_WINO_IN_UP    ? wc_launch8<true, false, false>(x, u, bias, add, y, n, c, k, h, w, stream)
         : mode == NHMC_WINO_ADD_UP ? wc_launch8<false, true, false>(x, u, bias, add, y, n, c, k, h, w, stream)
                                    : wc_launch8<false, false, true>(x, u, bias, add, y, n, c, k, h, w, stream);
}

// The skip-bias form of the eight-wave kernel (the paragraph "Skip bias" of the file header): add and add_bias are required.
extern "C" int nhmc_conv3x3_wino_skip_covers(int n, int c, int k, int h, int w) {
  return wc_covers(n, c, k, h, w) && wc_waves() == 8;
}

extern "C" int nhmc_conv3x3_wino_skip(const float* x, const float* u, const float* bias, const float* add, const float* add_bias,
                                      float* y, int n, int c, int k, int h, int w, nhmc_stream_t stream) {
  if (!x || !u || !y || !add || !add_bias || y == x || add == x) return NHMC_ERR_ARG;
  if (wc_waves() < 0) return NHMC_ERR_ARG;
  if (!wc_covers(n, c, k, h, w) || wc_waves() != 8) return NHMC_ERR_SHAPE;
  if (!nhmc_aligned16(x) || !nhmc_aligned16(u) || !nhmc_aligned16(y) || !nhmc_aligned16(add)) return NHMC_ERR_ALIGN;
  return wc_launch8<false, false, false, true>(x, u, bias, add, y, n, c, k, h, w, stream, add_bias);
}

extern "C" int nhmc_conv3x3_wino_narrow(const float* x, const float* u, const float* bias, const float* add, float* y, int n,
                                        int c, int k, int h, int w, int stride, int padding, nhmc_stream_t stream) {
  if (!x || !u || !y || y == x || (add && add == x)) return NHMC_ERR_ARG;
  if (stride != 1 || padding != 1 || !wc_narrow_covers(n, c, k, h, w)) return NHMC_ERR_SHAPE;
  if (!nhmc_aligned16(x) || !nhmc_aligned16(u) || !nhmc_aligned16(y) || !nhmc_aligned16(add)) return NHMC_ERR_ALIGN;
  return w == 32 ? wc_launch<16>(x, u, bias, add, y, n, c, k, h, w, stream)
                 : wc_launch<8>(x, u, bias, add, y, n, c, k, h, w, stream);
}

// Output-channel counts that are multiples of 32, all three geometries, chosen by w.  K % 64 == 0 runs the instantiations of
// the two entries above (their bits); K % 64 == 32 the TAIL ones.
extern "C" int nhmc_conv3x3_wino_k32(const float* x, const float* u, const float* bias, const float* add, float* y, int n, int c,
                                     int k, int h, int w, int stride, int padding, nhmc_stream_t stream) {
  if (!x || !u || !y || y == x || (add && add == x)) return NHMC_ERR_ARG;
  if (stride != 1 || padding != 1 || !wc_k32_covers(n, c, k, h, w)) return NHMC_ERR_SHAPE;
  if (!nhmc_aligned16(x) || !nhmc_aligned16(u) || !nhmc_aligned16(y) || !nhmc_aligned16(add)) return NHMC_ERR_ALIGN;
  if (k % WC_KBLK == 0)
    return w == 32   ? wc_launch<16>(x, u, bias, add, y, n, c, k, h, w, stream)
           : w == 16 ? wc_launch<8>(x, u, bias, add, y, n, c, k, h, w, stream)
                     : wc_launch<32>(x, u, bias, add, y, n, c, k, h, w, stream);
  return w == 32   ? wc_launch<16, true>(x, u, bias, add, y, n, c, k, h, w, stream)
         : w == 16 ? wc_launch<8, true>(x, u, bias, add, y, n, c, k, h, w, stream)
                   : wc_launch<32, true>(x, u, bias, add, y, n, c, k, h, w, stream);
}
