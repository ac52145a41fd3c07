// Principal components of the posterior samples (nhmc.h "Principal components of the posterior samples"): the Gram matrix
// of an image's pooled draws about the first one, and the projection that turns coefficients back into images.
//
// k_sample_gram<RB>: a tall-skinny U U^T on the fp64 MFMA, v_mfma_f64_16x16x4_f64.  The n operand rows (u_1 ... u_n)
// are cut into RB = 2, 4, 8 or 16 blocks of 16, rows from n up being zero.  A workgroup owns one slab (PCS_SLAB elements)
// of one group and walks it in tiles of E elements: all threads load the raw fp32 rows d_1 ... d_n and t of the next tile
// with 16-byte non-temporal loads into registers, the current tile sits in LDS as [row][E + 4] fp32.  For D = U U^T a lane's
// A operand and B operand of block b are the same value, u[16 b + (lane & 15)][k = lane >> 4], so a wave converts each
// block it needs once per k-step and feeds every block pair it owns from those registers.  A lane reads 8 bytes per row:
// elements 8 s + 2 k and 8 s + 2 k + 1 are its operands of two consecutive k-steps (which element is "k" is free as long as
// all rows agree); with a row stride of E + 4 dwords that ds_read_b64 is bank-conflict free (bank = 4 row + 2 k + {0, 1}
// mod 64 over a 32-lane half; 36 row for E = 32, a permutation of the same multiples of 4).
// Block pairs: with rb = ceil(n / 16) <= RB blocks in use, the unordered pairs {x, y} of Z_rb are (bi, (bi + d) mod rb),
// d = 0 ... rb / 2, those with 2 d = rb taken for bi < rb / 2 only.  Wave w owns bi = BPW w ... BPW w + BPW - 1 (those below
// rb) with all their d, so it needs the BPW + RB / 2 consecutive (cyclic) blocks from BPW w on and every register index is a
// constant; taking the pairs modulo rb, not RB, keeps every pair a wave holds inside the blocks in use.
// The accumulators stay in registers over the whole slab; the workgroup writes its 16 x 16 tiles to ws, and
// k_sample_gram_final adds the slabs in ascending order, reading (a, b) and (b, a) from the same addresses: exactly
// symmetric, no atomics.
// The f64 C/D layout is col = lane & 15, row = (lane >> 4) + 4 reg -- not the f32 one.
//
// k_sample_project<J>: thread = one element, lanes hold consecutive elements, draws loaded in batches ahead of the
// arithmetic as k_calibration does; J fp64 fma chains in ascending draw order, rounded once.
#include <math.h>
#include "nhmc_common.h"

namespace {

typedef double pcs_v4d __attribute__((ext_vector_type(4)));
typedef float pcs_v2f __attribute__((ext_vector_type(2)));

constexpr int PCS_SLAB = 1024;       // elements per workgroup: a multiple of every E
constexpr int PCS_MAX_N = 256;
constexpr int PCS_MAX_OUT = 8;
constexpr int PCS_BATCH = 16;        // projection: draws in flight per batch
constexpr int PCS_FINAL_BATCH = 16;  // second Gram kernel: slab partials in flight per thread

template <int RB> struct PcsCfg;
template <> struct PcsCfg<2>  { static constexpr int NW = 2, E = 128; };
template <> struct PcsCfg<4>  { static constexpr int NW = 4, E = 128; };
template <> struct PcsCfg<8>  { static constexpr int NW = 4, E = 64; };
template <> struct PcsCfg<16> { static constexpr int NW = 8, E = 32; };

static inline int pcs_rb(int n) { return n <= 32 ? 2 : n <= 64 ? 4 : n <= 128 ? 8 : 16; }
// doubles one slab of one group leaves in ws: rb = ceil(n / 16) block rows x (rb / 2 + 1) offsets x 256
static inline int64_t pcs_slab_doubles(int n) { const int rb = (n + 15) / 16; return (int64_t)rb * (rb / 2 + 1) * 256; }

// u = d - d_1 in fp64; a non-finite draw or d_1 gives NaN (x * 0 is 0 for a finite x and NaN otherwise).  A row from n up
// reads d_1 itself (its LDS offset points at row 0): 0 exactly, or NaN in a row that is never written out.
__device__ __forceinline__ double pcs_u(float x, double d1, float z1) {
  const double u = (double)x - d1;
  const float z = fmaf(x, 0.0f, z1);
  return z == 0.0f ? u : (double)NAN;
}

template <int RB>
__global__ __launch_bounds__(PcsCfg<RB>::NW * 64) void k_sample_gram(const float* __restrict__ samples,
                                                                     const float* __restrict__ x_orig,
                                                                     double* __restrict__ ws, int n, int64_t n_elem,
                                                                     int slabs) {
  constexpr int NW = PcsCfg<RB>::NW, NT = NW * 64, E = PcsCfg<RB>::E, E4 = E / 4, S = E + 4;
  constexpr int BPW = RB / NW, H = RB / 2, D = H + 1, NV = BPW + H;
  constexpr int ROWS = 16 * RB + 1;                       // d_1 ... d_n in rows 0 ... n - 1, t in row n
  constexpr int LPT = (ROWS * E4 + NT - 1) / NT;
  __shared__ __attribute__((aligned(16))) float tile[ROWS * S];
  const int g = blockIdx.y, slab = blockIdx.x, tid = threadIdx.x;
  const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r16 = lane & 15, kk = lane >> 4;
  const int rb = (n + 15) >> 4;
  const int64_t e_begin = (int64_t)slab * PCS_SLAB;
  const int64_t e_end = e_begin + PCS_SLAB < n_elem ? e_begin + PCS_SLAB : n_elem;
  const int tiles = (int)((e_end - e_begin + E - 1) / E);
  const float* base = samples + (int64_t)g * n * n_elem;
  const float* orig = x_orig ? x_orig + (int64_t)g * n_elem : nullptr;

  nhmc_v4f pre[LPT];
  auto fetch = [&](int64_t e0) {
#pragma unroll
    for (int i = 0; i < LPT; ++i) {
      const int f = tid + i * NT, row = f / E4, c4 = f % E4;
      const int64_t e = e0 + 4 * c4;
      nhmc_v4f v = {0.0f, 0.0f, 0.0f, 0.0f};                                   // the tail and the rows past t are zero
      if (row <= n && e < e_end) {
        if (row < n) v = __builtin_nontemporal_load(reinterpret_cast<const nhmc_v4f*>(base + (int64_t)row * n_elem + e));
        else if (orig) v = __builtin_nontemporal_load(reinterpret_cast<const nhmc_v4f*>(orig + e));
        else v = nhmc_v4f{NAN, NAN, NAN, NAN};
      }
      pre[i] = v;
    }
  };

  const int da = rb / 2 + 1;                                                   // offsets in use: d = 0 ... rb / 2
  int off[NV];
  bool blk_on[NV], pair_on[BPW * D];
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int b = (BPW * wave + i) % rb;
    blk_on[i] = false;
    off[i] = (16 * b + r16 < n ? (16 * b + r16 + 1) * S : 0) + 2 * kk;
  }
#pragma unroll
  for (int c = 0; c < BPW; ++c) {
    const int bi = BPW * wave + c;
#pragma unroll
    for (int d = 0; d < D; ++d) {
      const bool on = bi < rb && d < da && (2 * d < rb || bi < rb / 2);
      pair_on[c * D + d] = on;
      blk_on[c] = blk_on[c] || on;                                             // a block is read and converted only where
      blk_on[c + d] = blk_on[c + d] || on;                                     // one of this wave's pairs uses it
    }
  }

  pcs_v4d acc[BPW * D];
#pragma unroll
  for (int p = 0; p < BPW * D; ++p) acc[p] = pcs_v4d{0.0, 0.0, 0.0, 0.0};

  fetch(e_begin);
  for (int t = 0; t < tiles; ++t) {
    __syncthreads();                                                           // the last tile has been read
#pragma unroll
    for (int i = 0; i < LPT; ++i) {
      const int f = tid + i * NT, row = f / E4, c4 = f % E4;
      if (row < ROWS) *reinterpret_cast<nhmc_v4f*>(&tile[row * S + 4 * c4]) = pre[i];
    }
    __syncthreads();
    if (t + 1 < tiles) fetch(e_begin + (int64_t)(t + 1) * E);                  // in flight under this tile's arithmetic
#pragma unroll 2
    for (int s = 0; s < E / 8; ++s) {
      const pcs_v2f f1 = *reinterpret_cast<const pcs_v2f*>(&tile[2 * kk + 8 * s]);
      const double d1x = (double)f1.x, d1y = (double)f1.y;
      const float z1x = f1.x * 0.0f, z1y = f1.y * 0.0f;
      double ux[NV], uy[NV];
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        ux[i] = 0.0; uy[i] = 0.0;
        if (blk_on[i]) {
          const pcs_v2f r = *reinterpret_cast<const pcs_v2f*>(&tile[off[i] + 8 * s]);
          ux[i] = pcs_u(r.x, d1x, z1x);
          uy[i] = pcs_u(r.y, d1y, z1y);
        }
      }
#pragma unroll
      for (int c = 0; c < BPW; ++c) {
#pragma unroll
        for (int d = 0; d < D; ++d) {
          if (pair_on[c * D + d]) {
            acc[c * D + d] = __builtin_amdgcn_mfma_f64_16x16x4f64(ux[c], ux[c + d], acc[c * D + d], 0, 0, 0);
            acc[c * D + d] = __builtin_amdgcn_mfma_f64_16x16x4f64(uy[c], uy[c + d], acc[c * D + d], 0, 0, 0);
          }
        }
      }
    }
  }

  // tile (bi, d) = rows of block bi x columns of block (bi + d) mod rb, stored [row][col]
  double* out = ws + ((int64_t)g * slabs + slab) * ((int64_t)rb * da * 256);
#pragma unroll
  for (int c = 0; c < BPW; ++c) {
#pragma unroll
    for (int d = 0; d < D; ++d) {
      if (pair_on[c * D + d]) {
        double* o = out + ((BPW * wave + c) * da + d) * 256 + r16;
#pragma unroll
        for (int q = 0; q < 4; ++q) o[(kk + 4 * q) * 16] = acc[c * D + d][q];
      }
    }
  }
}

// gram[a][b] = the slabs' partials in ascending order; (a, b) and (b, a) read the same addresses.
__global__ void k_sample_gram_final(const double* __restrict__ ws, double* __restrict__ gram, int n, int slabs) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x, g = blockIdx.y;
  if (idx >= n * n) return;
  const int a = idx / n, b = idx - a * n;
  const int lo = a < b ? a : b, hi = a < b ? b : a;
  const int x = lo >> 4, y = hi >> 4, dd = y - x, rb = (n + 15) >> 4, D = rb / 2 + 1;
  const int at = 2 * dd <= rb ? (x * D + dd) * 256 + (lo & 15) * 16 + (hi & 15)
                              : (y * D + (rb - dd)) * 256 + (hi & 15) * 16 + (lo & 15);
  const int64_t stride = (int64_t)rb * D * 256;
  const double* p = ws + (int64_t)g * slabs * stride + at;
  double sum = 0.0;
  int s = 0;
  for (; s + PCS_FINAL_BATCH <= slabs; s += PCS_FINAL_BATCH) {                 // the loads of a batch in flight together,
    double v[PCS_FINAL_BATCH];                                                 // the additions still one ascending chain
#pragma unroll
    for (int j = 0; j < PCS_FINAL_BATCH; ++j) v[j] = p[(int64_t)(s + j) * stride];
#pragma unroll
    for (int j = 0; j < PCS_FINAL_BATCH; ++j) sum += v[j];
  }
  for (; s < slabs; ++s) sum += p[(int64_t)s * stride];
  gram[(int64_t)g * n * n + idx] = sum;
}

__device__ __forceinline__ void prj_load(float (&x)[PCS_BATCH], const float* __restrict__ p, int64_t stride) {
#pragma unroll
  for (int j = 0; j < PCS_BATCH; ++j) x[j] = __builtin_nontemporal_load(p + (int64_t)j * stride);
}

__device__ __forceinline__ void prj_load_tail(float (&x)[PCS_BATCH - 1], const float* __restrict__ p, int cnt, int64_t stride) {
#pragma unroll
  for (int j = 0; j < PCS_BATCH - 1; ++j) x[j] = j < cnt ? __builtin_nontemporal_load(p + (int64_t)j * stride) : 0.0f;
}

template <int J>
__device__ __forceinline__ void prj_step(double (&acc)[J], const double* __restrict__ coef, int n, int i, float x, double d1) {
  const double d = (double)x - d1;
#pragma unroll
  for (int j = 0; j < J; ++j) acc[j] = fma(coef[j * n + i], d, acc[j]);
}

template <int J>
__global__ __launch_bounds__(NHMC_BLOCK) void k_sample_project(const float* __restrict__ samples,
                                                               const double* __restrict__ coef, float* __restrict__ out,
                                                               int n, int64_t n_elem) {
  const int g = blockIdx.y;
  const int64_t e = (int64_t)blockIdx.x * NHMC_BLOCK + threadIdx.x;
  if (e >= n_elem) return;
  const float* p = samples + (int64_t)g * n * n_elem + e;
  const double* c = coef + (int64_t)g * J * n;                                 // uniform: scalar loads
  const int full = n / PCS_BATCH, rem = n - full * PCS_BATCH;
  double acc[J];
#pragma unroll
  for (int j = 0; j < J; ++j) acc[j] = 0.0;
  float cur[PCS_BATCH], nxt[PCS_BATCH], tail[PCS_BATCH - 1];
  prj_load_tail(tail, p + (int64_t)full * PCS_BATCH * n_elem, rem, n_elem);   // the last rem < 16 draws, used last
  if (full > 0) prj_load(cur, p, n_elem);
  const double d1 = (double)(full > 0 ? cur[0] : tail[0]);
  for (int bi = 0; bi < full; ++bi) {
    const bool more = bi + 1 < full;
    if (more) prj_load(nxt, p + (int64_t)(bi + 1) * PCS_BATCH * n_elem, n_elem);
#pragma unroll
    for (int j = 0; j < PCS_BATCH; ++j) prj_step<J>(acc, c, n, bi * PCS_BATCH + j, cur[j], d1);
    if (more) {
#pragma unroll
      for (int j = 0; j < PCS_BATCH; ++j) cur[j] = nxt[j];
    }
  }
#pragma unroll
  for (int j = 0; j < PCS_BATCH - 1; ++j)
    if (j < rem) prj_step<J>(acc, c, n, full * PCS_BATCH + j, tail[j], d1);
#pragma unroll
  for (int j = 0; j < J; ++j) __builtin_nontemporal_store((float)acc[j], out + ((int64_t)g * J + j) * n_elem + e);
}

template <int RB>
void pcs_launch_gram(const float* samples, const float* x_orig, double* ws, int n_groups, int n, int64_t n_elem, int slabs,
                     hipStream_t stream) {
  NHMC_LAUNCH(k_sample_gram<RB>, dim3((unsigned)slabs, (unsigned)n_groups), dim3(PcsCfg<RB>::NW * 64), 0, stream, samples,
              x_orig, ws, n, n_elem, slabs);
}

template <int J>
void pcs_launch_project(const float* samples, const double* coef, float* out, int n_groups, int n, int64_t n_elem,
                        hipStream_t stream) {
  NHMC_LAUNCH(k_sample_project<J>, dim3((unsigned)((n_elem + NHMC_BLOCK - 1) / NHMC_BLOCK), (unsigned)n_groups),
              dim3(NHMC_BLOCK), 0, stream, samples, coef, out, n, n_elem);
}

}  // namespace

extern "C" int nhmc_sample_gram_slabs(int64_t n_elem) {
  if (n_elem <= 0) return 0;
  const int64_t s = (n_elem + PCS_SLAB - 1) / PCS_SLAB;
  return s > INT32_MAX ? 0 : (int)s;
}

extern "C" size_t nhmc_sample_gram_ws_bytes(int n_groups, int n, int64_t n_elem) {
  if (n_groups <= 0 || n < 2 || n > PCS_MAX_N || n_elem <= 0) return 0;
  return (size_t)n_groups * (size_t)nhmc_sample_gram_slabs(n_elem) * (size_t)pcs_slab_doubles(n) * sizeof(double);
}

extern "C" int nhmc_sample_gram(const float* samples, const float* x_orig, double* gram, double* ws, int n_groups,
                                int n_replicas, int n_samples, int64_t n_elem, nhmc_stream_t stream) {
  if (!samples || !gram || !ws || n_groups <= 0 || n_replicas <= 0 || n_samples <= 0 || n_elem <= 0) return NHMC_ERR_ARG;
  if ((n_elem & 3) || !nhmc_aligned16(samples) || !nhmc_aligned16(x_orig) || !nhmc_aligned16(gram)) return NHMC_ERR_ALIGN;
  const int64_t n64 = (int64_t)n_replicas * n_samples;
  const int slabs = nhmc_sample_gram_slabs(n_elem);
  if (n64 < 2 || n64 > PCS_MAX_N || n_groups > 65535 || slabs <= 0) return NHMC_ERR_SHAPE;
  const int n = (int)n64, RB = pcs_rb(n);
  hipStream_t s = nhmc_s(stream);
  switch (RB) {
    case 2: pcs_launch_gram<2>(samples, x_orig, ws, n_groups, n, n_elem, slabs, s); break;
    case 4: pcs_launch_gram<4>(samples, x_orig, ws, n_groups, n, n_elem, slabs, s); break;
    case 8: pcs_launch_gram<8>(samples, x_orig, ws, n_groups, n, n_elem, slabs, s); break;
    default: pcs_launch_gram<16>(samples, x_orig, ws, n_groups, n, n_elem, slabs, s); break;
  }
  NHMC_LAUNCH(k_sample_gram_final, dim3((unsigned)((n * n + 255) / 256), (unsigned)n_groups), dim3(256), 0, s, ws, gram, n,
              slabs);
  return nhmc_launch_status();
}

extern "C" int nhmc_sample_project(const float* samples, const double* coef, float* out, int n_groups, int n_replicas,
                                   int n_samples, int n_out, int64_t n_elem, nhmc_stream_t stream) {
  if (!samples || !coef || !out || n_groups <= 0 || n_replicas <= 0 || n_samples <= 0 || n_elem <= 0) return NHMC_ERR_ARG;
  if ((n_elem & 3) || !nhmc_aligned16(samples) || !nhmc_aligned16(coef) || !nhmc_aligned16(out)) return NHMC_ERR_ALIGN;
  const int64_t n64 = (int64_t)n_replicas * n_samples;
  if (n64 < 2 || n64 > PCS_MAX_N || n_groups > 65535 || n_out < 1 || n_out > PCS_MAX_OUT ||
      (n_elem + NHMC_BLOCK - 1) / NHMC_BLOCK > INT32_MAX)
    return NHMC_ERR_SHAPE;
  const int n = (int)n64;
  hipStream_t s = nhmc_s(stream);
  switch (n_out) {
    case 1: pcs_launch_project<1>(samples, coef, out, n_groups, n, n_elem, s); break;
    case 2: pcs_launch_project<2>(samples, coef, out, n_groups, n, n_elem, s); break;
    case 3: pcs_launch_project<3>(samples, coef, out, n_groups, n, n_elem, s); break;
    case 4: pcs_launch_project<4>(samples, coef, out, n_groups, n, n_elem, s); break;
    case 5: pcs_launch_project<5>(samples, coef, out, n_groups, n, n_elem, s); break;
    case 6: pcs_launch_project<6>(samples, coef, out, n_groups, n, n_elem, s); break;
    case 7: pcs_launch_project<7>(samples, coef, out, n_groups, n, n_elem, s); break;
    default: pcs_launch_project<8>(samples, coef, out, n_groups, n, n_elem, s); break;
  }
  return nhmc_launch_status();
}
