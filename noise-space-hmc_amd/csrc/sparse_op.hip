// Sparse linear operators (operators.SparseLinear, --deg ct<V>): A x, the exact adjoint A^T w on the transposed list, and
// the data term with the last DDIM step's VJP as the epilogue of the adjoint pass.  The definition (canonical CSR pair,
// summation, limits) is in include/nhmc.h.
//
// The batch is the dense side of a sparse-times-dense product: P = n_chains * C planes see the same matrix.  In NCHW a
// plane is contiguous, so x[p][col] over the planes would be P scattered dwords per entry.  The operand is therefore staged
// plane-minor, Xt[col][P]: one entry costs one contiguous row of 4 P bytes.  Four passes:
//   1. k_sparse_tin : [P][n] -> Xt[n][P], a 64 x 64 tile transpose through LDS (stride 65: conflict-free both ways); the
//                     data term clips here.
//   2. k_sparse_mm  : the product.  A wave owns one matrix row and 64 planes, lane = plane: the row's entries are one
//                     serial fmaf chain per lane in list order from 0.0f, whatever P, n_chains or the plane's place in
//                     the batch are -- no atomics, nothing to reduce.  The wave reads 64 (col, val) pairs with one
//                     coalesced load, then hands them out lane by lane as scalars (v_readlane), eight gathers in flight.
//                     A workgroup (4 waves) owns SP_ROWS = 16 consecutive rows, four per wave.  The data term's forward
//                     pass stages its 16 x 64 tile of y (plane-major in memory: 64-byte runs) through LDS and writes the
//                     residual plane-minor and the fp64 partial of its fp32 squares per (plane, row tile).
//   3. k_sparse_mm on the transposed list over the residual, each gathered value scaled by -2 (exact).
//   4. k_sparse_tout: [n][P] -> [P][n]; the store side applies the clamp mask or nhmc_mix_vjp.
// Lanes past P (P % 64 != 0) gather plane P - 1 again and store nothing.
//
// The entries cannot read the device lists: nhmc_sparse_check validates the host copy, and the kernel clamps the row
// bounds into [0, nnz] and every column into [0, cols), so no read leaves a buffer whatever the device lists hold.
#include "nhmc_common.h"

namespace {

constexpr int SP_ROWS = 16;                    // matrix rows per workgroup: 4 per wave
constexpr int SP_RW = SP_ROWS / 4;
constexpr int SP_T = 64;                       // transpose tile
constexpr int SP_UN = 8;                       // gathers in flight per wave

enum { SP_PLAIN = 0, SP_NEG2 = 1, SP_RESID = 2 };
enum { SP_OUT = 0, SP_MASK = 1, SP_VJP = 2 };

struct SparseVjp {
  const float* e;
  float* g_e;
  const float* at;
  const float* at_next;
  int e_channels, fill_sigma;
};

__global__ __launch_bounds__(NHMC_BLOCK) void k_sparse_tin(const float* __restrict__ src, float* __restrict__ dst, int n,
                                                           int P, int clip) {
  __shared__ float t[SP_T][SP_T + 1];
  const int lane = threadIdx.x & (NHMC_WAVE - 1), wave = threadIdx.x >> 6;
  const int j0 = blockIdx.x * SP_T, p0 = blockIdx.y * SP_T;
  for (int rr = wave; rr < SP_T; rr += 4) {
    const int p = p0 + rr, j = j0 + lane;
    if (p < P && j < n) {
      const float v = src[(int64_t)p * n + j];
      t[rr][lane] = clip ? nhmc_clip1(v) : v;
    }
  }
  __syncthreads();
  for (int rr = wave; rr < SP_T; rr += 4) {
    const int j = j0 + rr, p = p0 + lane;
    if (j < n && p < P) dst[(int64_t)j * P + p] = t[lane][rr];
  }
}

// MODE SP_OUT : out = src^T
//      SP_MASK: out = masked(src^T, 1[|aux| <= 1])                 (aux = xt)
//      SP_VJP : (out, g_e) = nhmc_mix_vjp(src^T, aux, e)           (aux = xt, the last step's input)
template <int MODE>
__global__ __launch_bounds__(NHMC_BLOCK) void k_sparse_tout(const float* __restrict__ src, const float* __restrict__ aux,
                                                            float* __restrict__ out, SparseVjp vjp, int n, int P, int C) {
  __shared__ float t[SP_T][SP_T + 1];
  const int lane = threadIdx.x & (NHMC_WAVE - 1), wave = threadIdx.x >> 6;
  const int j0 = blockIdx.x * SP_T, p0 = blockIdx.y * SP_T;
  for (int rr = wave; rr < SP_T; rr += 4) {
    const int j = j0 + rr, p = p0 + lane;
    if (j < n && p < P) t[rr][lane] = src[(int64_t)j * P + p];
  }
  __syncthreads();
  for (int rr = wave; rr < SP_T; rr += 4) {
    const int p = p0 + rr, j = j0 + lane;
    if (p >= P || j >= n) continue;
    const float g = t[lane][rr];
    const int64_t o = (int64_t)p * n + j;
    if (MODE == SP_OUT) {
      out[o] = g;
    } else if (MODE == SP_MASK) {
      out[o] = nhmc_masked(g, nhmc_in1(aux[o]));
    } else {
      const int chain = p / C, ch = p - chain * C;
      const NhmcMix k = nhmc_mix_coef(vjp.at, vjp.at_next, chain);
      const int64_t eo = ((int64_t)chain * vjp.e_channels + ch) * n + j;
      float gx, ge;
      nhmc_mix_vjp(k, g, aux[o], vjp.e[eo], gx, ge);
      out[o] = gx;
      vjp.g_e[eo] = ge;
      if (vjp.fill_sigma && vjp.e_channels > C) vjp.g_e[eo + (int64_t)C * n] = 0.0f;      // learned-sigma half
    }
  }
}

// Xt [cols][P] -> Ot [rows][P].
// SP_PLAIN: Ot = A Xt
// SP_NEG2 : Ot = A (-2 Xt)
// SP_RESID: Ot = y - A Xt (y [P][rows], plane-major), loss_ws[p][tile] = sum of the tile's fp32 squares in fp64
template <int MODE>
__global__ __launch_bounds__(NHMC_BLOCK) void k_sparse_mm(const float* __restrict__ Xt, const int* __restrict__ row_ptr,
                                                          const int* __restrict__ col, const float* __restrict__ val,
                                                          int rows, int cols, int nnz, int P, const float* __restrict__ y,
                                                          float* __restrict__ Ot, double* __restrict__ loss_ws) {
  __shared__ float ys[MODE == SP_RESID ? SP_ROWS : 1][NHMC_WAVE + 1];
  __shared__ double red[MODE == SP_RESID ? 4 : 1][NHMC_WAVE];
  const int lane = threadIdx.x & (NHMC_WAVE - 1);
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int tile = blockIdx.x, i0 = tile * SP_ROWS, p0 = blockIdx.y * NHMC_WAVE;
  const int p = p0 + lane;
  const bool p_in = p < P;
  const float* __restrict__ xp = Xt + (p_in ? p : P - 1);

  if (MODE == SP_RESID) {
    for (int idx = threadIdx.x; idx < SP_ROWS * NHMC_WAVE; idx += NHMC_BLOCK) {
      const int r = idx & (SP_ROWS - 1), pl = idx >> 4;
      if (i0 + r < rows && p0 + pl < P) ys[r][pl] = y[(int64_t)(p0 + pl) * rows + i0 + r];
    }
    __syncthreads();
  }

  double sq = 0.0;                                           // fp32 squares summed in fp64, as the other data terms
  for (int r = 0; r < SP_RW; ++r) {
    const int row = i0 + wave * SP_RW + r;                   // wave-uniform
    if (row >= rows) break;
    const int beg = min(max(row_ptr[row], 0), nnz);
    const int end = min(max(row_ptr[row + 1], beg), nnz);
    float acc = 0.0f;
    for (int k0 = beg; k0 < end; k0 += NHMC_WAVE) {
      const int kk = k0 + lane;
      int cv = 0, wv = 0;
      if (kk < end) {
        cv = min(max(col[kk], 0), cols - 1);
        wv = __float_as_int(val[kk]);
      }
      const int cnt = min(NHMC_WAVE, end - k0);
      int j = 0;
      for (; j + SP_UN <= cnt; j += SP_UN) {
        float xv[SP_UN];
#pragma unroll
        for (int u = 0; u < SP_UN; ++u) xv[u] = xp[(int64_t)__builtin_amdgcn_readlane(cv, j + u) * P];
#pragma unroll
        for (int u = 0; u < SP_UN; ++u) {
          const float w = __int_as_float(__builtin_amdgcn_readlane(wv, j + u));
          acc = fmaf(w, MODE == SP_NEG2 ? -(2.0f * xv[u]) : xv[u], acc);
        }
      }
      for (; j < cnt; ++j) {
        const float v = xp[(int64_t)__builtin_amdgcn_readlane(cv, j) * P];
        const float w = __int_as_float(__builtin_amdgcn_readlane(wv, j));
        acc = fmaf(w, MODE == SP_NEG2 ? -(2.0f * v) : v, acc);
      }
    }
    if (MODE == SP_RESID) {
      const float res = ys[wave * SP_RW + r][lane] - acc;
      sq += (double)(res * res);
      acc = res;
    }
    if (p_in) Ot[(int64_t)row * P + p] = acc;
  }
  if (MODE == SP_RESID) {
    red[wave][lane] = sq;
    __syncthreads();
    if (wave == 0 && p_in) loss_ws[(int64_t)p * gridDim.x + tile] = (red[0][lane] + red[1][lane]) + (red[2][lane] + red[3][lane]);
  }
}

int sp_ceil(int64_t a, int b) { return (int)((a + b - 1) / b); }

// NHMC_OK, or the code the entries return for a shape they do not cover.
int sparse_geom(int rows, int cols, int nnz, int n_chains, int channels) {
  if (rows < 1 || cols < 1 || nnz < 1) return NHMC_ERR_SHAPE;
  if (n_chains <= 0 || n_chains > 65535 || channels <= 0 || channels > 65535) return NHMC_ERR_SHAPE;
  if ((int64_t)n_chains * channels > (int64_t)65535 * NHMC_WAVE) return NHMC_ERR_SHAPE;      // plane chunks ride grid.y
  return NHMC_OK;
}

int sparse_tin(const float* src, float* dst, int n, int P, int clip, nhmc_stream_t stream) {
  dim3 grid((unsigned)sp_ceil(n, SP_T), (unsigned)sp_ceil(P, SP_T));
  NHMC_LAUNCH(k_sparse_tin, grid, dim3(NHMC_BLOCK), 0, nhmc_s(stream), src, dst, n, P, clip);
  return nhmc_launch_status();
}

template <int MODE>
int sparse_tout(const float* src, const float* aux, float* out, const SparseVjp& vjp, int n, int P, int C,
                nhmc_stream_t stream) {
  dim3 grid((unsigned)sp_ceil(n, SP_T), (unsigned)sp_ceil(P, SP_T));
  NHMC_LAUNCH(k_sparse_tout<MODE>, grid, dim3(NHMC_BLOCK), 0, nhmc_s(stream), src, aux, out, vjp, n, P, C);
  return nhmc_launch_status();
}

template <int MODE>
int sparse_mm(const float* Xt, const int32_t* row_ptr, const int32_t* col, const float* val, int rows, int cols, int nnz,
              int P, const float* y, float* Ot, double* loss_ws, nhmc_stream_t stream) {
  dim3 grid((unsigned)sp_ceil(rows, SP_ROWS), (unsigned)sp_ceil(P, NHMC_WAVE));
  NHMC_LAUNCH(k_sparse_mm<MODE>, grid, dim3(NHMC_BLOCK), 0, nhmc_s(stream), Xt, row_ptr, col, val, rows, cols, nnz, P, y, Ot,
              loss_ws);
  return nhmc_launch_status();
}

bool sp_aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }

// passes 1-3 of the two data terms: tmp = [Xt | Gt : n * P][r : m * P]
int sparse_data_passes(const float* x, int clip, const float* y, const int32_t* row_ptr, const int32_t* col,
                       const float* val, const int32_t* t_row_ptr, const int32_t* t_col, const float* t_val, int m, int n,
                       int nnz, double* loss_ws, float* tmp, int P, nhmc_stream_t stream) {
  float* Xt = tmp;
  float* Rt = tmp + (int64_t)n * P;
  if (const int rc = sparse_tin(x, Xt, n, P, clip, stream)) return rc;
  if (const int rc = sparse_mm<SP_RESID>(Xt, row_ptr, col, val, m, n, nnz, P, y, Rt, loss_ws, stream)) return rc;
  return sparse_mm<SP_NEG2>(Rt, t_row_ptr, t_col, t_val, n, m, nnz, P, nullptr, Xt, nullptr, stream);
}

}  // namespace

extern "C" int nhmc_sparse_check(const int32_t* host_row_ptr, const int32_t* host_col, int m, int n, int nnz) {
  if (!host_row_ptr || !host_col) return NHMC_ERR_ARG;
  if (m < 1 || n < 1 || nnz < 1) return NHMC_ERR_SHAPE;
  if (host_row_ptr[0] != 0 || host_row_ptr[m] != nnz) return NHMC_ERR_SHAPE;
  for (int i = 0; i < m; ++i)
    if (host_row_ptr[i + 1] < host_row_ptr[i]) return NHMC_ERR_SHAPE;
  for (int k = 0; k < nnz; ++k)
    if (host_col[k] < 0 || host_col[k] >= n) return NHMC_ERR_SHAPE;
  return NHMC_OK;
}

extern "C" int nhmc_sparse_tiles(int channels, int m) { return channels * sp_ceil(m, SP_ROWS); }

extern "C" size_t nhmc_sparse_tmp_floats(int n_chains, int channels, int m, int n) {
  return (size_t)n_chains * (size_t)channels * ((size_t)m + (size_t)n);
}

extern "C" int nhmc_sparse_apply(const float* x, const int32_t* row_ptr, const int32_t* col, const float* val, int rows,
                                 int cols, int nnz, float* out, float* tmp, int n_chains, int channels,
                                 nhmc_stream_t stream) {
  if (!x || !row_ptr || !col || !val || !out || !tmp || x == out || tmp == x || tmp == out) return NHMC_ERR_ARG;
  if (const int rc = sparse_geom(rows, cols, nnz, n_chains, channels)) return rc;
  if (!nhmc_aligned16(x) || !nhmc_aligned16(out) || !nhmc_aligned16(tmp) || !sp_aligned4(row_ptr) || !sp_aligned4(col) ||
      !sp_aligned4(val))
    return NHMC_ERR_ALIGN;
  const int P = n_chains * channels;
  float* Xt = tmp;
  float* Ot = tmp + (int64_t)cols * P;
  if (const int rc = sparse_tin(x, Xt, cols, P, 0, stream)) return rc;
  if (const int rc = sparse_mm<SP_PLAIN>(Xt, row_ptr, col, val, rows, cols, nnz, P, nullptr, Ot, nullptr, stream)) return rc;
  return sparse_tout<SP_OUT>(Ot, nullptr, out, SparseVjp{}, rows, P, channels, stream);
}

extern "C" int nhmc_data_sparse(const float* xt, const float* y, const int32_t* row_ptr, const int32_t* col,
                                const float* val, const int32_t* t_row_ptr, const int32_t* t_col, const float* t_val, int m,
                                int nnz, int apply_clip, float* g_xt, double* loss_ws, float* tmp, int n_chains,
                                int channels, int dim, nhmc_stream_t stream) {
  if (!xt || !y || !row_ptr || !col || !val || !t_row_ptr || !t_col || !t_val || !g_xt || !loss_ws || !tmp || tmp == g_xt ||
      tmp == xt)
    return NHMC_ERR_ARG;
  if (dim <= 0 || dim > 32768) return NHMC_ERR_SHAPE;
  if (const int rc = sparse_geom(m, dim * dim, nnz, n_chains, channels)) return rc;
  if (dim & 3) return NHMC_ERR_ALIGN;
  if (!nhmc_aligned16(xt) || !nhmc_aligned16(y) || !nhmc_aligned16(g_xt) || !nhmc_aligned16(tmp) || !sp_aligned4(row_ptr) ||
      !sp_aligned4(col) || !sp_aligned4(val) || !sp_aligned4(t_row_ptr) || !sp_aligned4(t_col) || !sp_aligned4(t_val))
    return NHMC_ERR_ALIGN;
  const int P = n_chains * channels, n = dim * dim;
  if (const int rc = sparse_data_passes(xt, apply_clip != 0, y, row_ptr, col, val, t_row_ptr, t_col, t_val, m, n, nnz,
                                        loss_ws, tmp, P, stream))
    return rc;
  if (apply_clip) return sparse_tout<SP_MASK>(tmp, xt, g_xt, SparseVjp{}, n, P, channels, stream);
  return sparse_tout<SP_OUT>(tmp, nullptr, g_xt, SparseVjp{}, n, P, channels, stream);
}

extern "C" int nhmc_data_sparse_vjp(const float* xt_next, const float* y, const int32_t* row_ptr, const int32_t* col,
                                    const float* val, const int32_t* t_row_ptr, const int32_t* t_col, const float* t_val,
                                    int m, int nnz, const float* xt_in, const float* e, int e_channels, const float* at,
                                    const float* at_next, float* g_xt, float* g_e, int fill_sigma, double* loss_ws,
                                    float* tmp, int n_chains, int channels, int dim, nhmc_stream_t stream) {
  if (!xt_next || !y || !row_ptr || !col || !val || !t_row_ptr || !t_col || !t_val || !xt_in || !e || !at || !at_next ||
      !g_xt || !g_e || !loss_ws || !tmp || tmp == g_xt || tmp == xt_next)
    return NHMC_ERR_ARG;
  if (dim <= 0 || dim > 32768) return NHMC_ERR_SHAPE;
  if (const int rc = sparse_geom(m, dim * dim, nnz, n_chains, channels)) return rc;
  if (e_channels != channels && e_channels != 2 * channels) return NHMC_ERR_SHAPE;
  if (dim & 3) return NHMC_ERR_ALIGN;
  if (!nhmc_aligned16(xt_next) || !nhmc_aligned16(y) || !nhmc_aligned16(xt_in) || !nhmc_aligned16(e) ||
      !nhmc_aligned16(g_xt) || !nhmc_aligned16(g_e) || !nhmc_aligned16(tmp) || !sp_aligned4(row_ptr) || !sp_aligned4(col) ||
      !sp_aligned4(val) || !sp_aligned4(t_row_ptr) || !sp_aligned4(t_col) || !sp_aligned4(t_val))
    return NHMC_ERR_ALIGN;
  const int P = n_chains * channels, n = dim * dim;
  if (const int rc = sparse_data_passes(xt_next, 0, y, row_ptr, col, val, t_row_ptr, t_col, t_val, m, n, nnz, loss_ws, tmp,
                                        P, stream))
    return rc;
  const SparseVjp vjp{e, g_e, at, at_next, e_channels, fill_sigma};
  return sparse_tout<SP_VJP>(tmp, xt_in, g_xt, vjp, n, P, channels, stream);
}
