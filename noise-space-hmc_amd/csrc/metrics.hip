// Report stage on the device: what `sample_image` computes from the collected samples (main_sampling.py:488-561) --
// every sample's data range and SSIM (:520, skimage's structural_similarity at its defaults), the posterior-mean image and
// the per-pixel standard deviation across a chain's samples with its min-max normalised picture (:494-507).  The PSNR of
// the block (:517-519) is nhmc_psnr_samples in sampler_state.hip, next to the kernels it shares with nhmc_psnr.
// The reference does this on the host, one sample at a time (numpy + skimage + matplotlib); here it is per (tile, channel,
// sample) and stays on the stream.  Every image passes through inverse_data_transform, clamp((v+1)/2, 0, 1) in fp32, as in
// k_psnr_partial.  Reductions: per-tile fp64 partials, then one wave per sample / chain in a fixed order.
#include <math.h>
#include "nhmc_common.h"

namespace {

constexpr int SSIM_WIN = 7;                      // skimage's default win_size
constexpr int SSIM_TH = 16, SSIM_TW = 32;        // window positions per block: 16 rows x 32 columns
constexpr int SSIM_RH = SSIM_TH + SSIM_WIN - 1;  // staged rows: the tile plus the 6 pixels its windows reach below it
constexpr int SSIM_RW = SSIM_TW + SSIM_WIN - 1;

__device__ __forceinline__ float unit_range(float v) { return fminf(fmaxf((v + 1.0f) / 2.0f, 0.0f), 1.0f); }

// Block-level min / max of one value pair per thread (256 threads); result valid in thread 0.
__device__ __forceinline__ void block_minmax(float& lo, float& hi, float* lds /* [8] */) {
  const int lane = threadIdx.x & (NHMC_WAVE - 1), wave = threadIdx.x >> 6;
#pragma unroll
  for (int off = NHMC_WAVE / 2; off > 0; off >>= 1) {
    lo = fminf(lo, __shfl_down(lo, off, NHMC_WAVE));
    hi = fmaxf(hi, __shfl_down(hi, off, NHMC_WAVE));
  }
  if (lane == 0) { lds[wave * 2] = lo; lds[wave * 2 + 1] = hi; }
  __syncthreads();
  if (threadIdx.x == 0) {
    lo = fminf(fminf(lds[0], lds[2]), fminf(lds[4], lds[6]));
    hi = fmaxf(fmaxf(lds[1], lds[3]), fmaxf(lds[5], lds[7]));
  }
}

// One wave: min / max over `tiles` (lo, hi) pairs of doubles holding fp32 values; result valid in every lane.
__device__ __forceinline__ void wave_minmax_pairs(const double* __restrict__ pairs, int tiles, float& lo, float& hi) {
  const int lane = threadIdx.x & (NHMC_WAVE - 1);
  lo = INFINITY; hi = -INFINITY;
  for (int t = lane; t < tiles; t += NHMC_WAVE) {
    lo = fminf(lo, (float)pairs[2 * t]);
    hi = fmaxf(hi, (float)pairs[2 * t + 1]);
  }
#pragma unroll
  for (int off = NHMC_WAVE / 2; off > 0; off >>= 1) {
    lo = fminf(lo, __shfl_xor(lo, off, NHMC_WAVE));
    hi = fmaxf(hi, __shfl_xor(hi, off, NHMC_WAVE));
  }
}

// ---- data range of every sample ---------------------------------------------------------------
__global__ __launch_bounds__(NHMC_BLOCK) void k_sample_range_partial(const float4* __restrict__ x,
                                                                     double* __restrict__ ws, int64_t n4) {
  const int row = blockIdx.y;
  const int64_t base = (int64_t)row * n4;
  const int64_t t0 = (int64_t)blockIdx.x * (NHMC_BLOCK * NHMC_VEC_PER_THREAD) + threadIdx.x;
  float lo = INFINITY, hi = -INFINITY;
#pragma unroll
  for (int i = 0; i < NHMC_VEC_PER_THREAD; ++i) {
    const int64_t q = t0 + (int64_t)i * NHMC_BLOCK;
    if (q >= n4) continue;
    const float4 a = nhmc_ldnt(&x[base + q]);
    const float* ae = reinterpret_cast<const float*>(&a);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const float u = unit_range(ae[c]);
      lo = fminf(lo, u);
      hi = fmaxf(hi, u);
    }
  }
  __shared__ float red[8];
  block_minmax(lo, hi, red);
  if (threadIdx.x == 0) {
    double* out = ws + ((int64_t)row * gridDim.x + blockIdx.x) * 2;
    out[0] = (double)lo;
    out[1] = (double)hi;
  }
}

__global__ void k_sample_range(const double* __restrict__ ws, int tiles, float* __restrict__ range, int rows) {
  const int row = blockIdx.x * (blockDim.x / NHMC_WAVE) + (threadIdx.x >> 6);
  if (row >= rows) return;
  float lo, hi;
  wave_minmax_pairs(ws + (int64_t)row * tiles * 2, tiles, lo, hi);
  if ((threadIdx.x & 63) == 0) range[row] = hi - lo;      // x[j].max() - x[j].min() on float32, :520
}

// ---- SSIM -------------------------------------------------------------------------------------
// Block = one 16 x 32 tile of window positions of one channel plane of one sample.  The tile and the 6 rows / columns its
// 7 x 7 windows reach past it are staged in LDS for both images (each staged pixel is used by up to 49 windows); the five
// window sums are formed separably -- 7 along the row, then 7 down the column -- in fp64 from the products on.
__global__ __launch_bounds__(NHMC_BLOCK) void k_ssim_partial(const float* __restrict__ x, const float* __restrict__ xo,
                                                             const float* __restrict__ range, double* __restrict__ ws,
                                                             int n_samples, int C, int H, int W, int tiles_x) {
  __shared__ float rx[SSIM_RH][SSIM_RW], ry[SSIM_RH][SSIM_RW];
  __shared__ double hs[5][SSIM_RH][SSIM_TW];
  __shared__ double red[4];
  const int tile = blockIdx.x, c = blockIdx.y, row = blockIdx.z;
  const int y0 = (tile / tiles_x) * SSIM_TH, x0 = (tile % tiles_x) * SSIM_TW;
  const int64_t hw = (int64_t)H * W;
  const float* px = x + ((int64_t)row * C + c) * hw;
  const float* py = xo + ((int64_t)(row / n_samples) * C + c) * hw;     // sample b * S + j against x_orig[b]

  for (int i = threadIdx.x; i < SSIM_RH * SSIM_RW; i += NHMC_BLOCK) {
    const int r = i / SSIM_RW, q = i - r * SSIM_RW;
    const int gy = y0 + r, gx = x0 + q;
    const bool in = gy < H && gx < W;                                   // past the image: zeros no counted window reads
    rx[r][q] = in ? unit_range(px[(int64_t)gy * W + gx]) : 0.0f;
    ry[r][q] = in ? unit_range(py[(int64_t)gy * W + gx]) : 0.0f;
  }
  __syncthreads();

  for (int i = threadIdx.x; i < SSIM_RH * SSIM_TW; i += NHMC_BLOCK) {
    const int r = i / SSIM_TW, q = i - r * SSIM_TW;
    double sx = 0.0, sy = 0.0, sxx = 0.0, syy = 0.0, sxy = 0.0;
#pragma unroll
    for (int j = 0; j < SSIM_WIN; ++j) {
      const double a = (double)rx[r][q + j], b = (double)ry[r][q + j];
      sx += a; sy += b; sxx += a * a; syy += b * b; sxy += a * b;
    }
    hs[0][r][q] = sx; hs[1][r][q] = sy; hs[2][r][q] = sxx; hs[3][r][q] = syy; hs[4][r][q] = sxy;
  }
  __syncthreads();

  const double R = (double)range[row];
  const double C1 = (0.01 * R) * (0.01 * R), C2 = (0.03 * R) * (0.03 * R);
  const double NP = (double)(SSIM_WIN * SSIM_WIN), cov_norm = NP / (NP - 1.0);
  double acc = 0.0;
  for (int i = threadIdx.x; i < SSIM_TH * SSIM_TW; i += NHMC_BLOCK) {
    const int r = i / SSIM_TW, q = i - r * SSIM_TW;
    if (y0 + r > H - SSIM_WIN || x0 + q > W - SSIM_WIN) continue;       // the window must lie inside the image
    double s[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      double v = 0.0;
#pragma unroll
      for (int j = 0; j < SSIM_WIN; ++j) v += hs[k][r + j][q];
      s[k] = v / NP;
    }
    const double ux = s[0], uy = s[1];
    const double vx = cov_norm * (s[2] - ux * ux), vy = cov_norm * (s[3] - uy * uy), vxy = cov_norm * (s[4] - ux * uy);
    const double A1 = 2.0 * ux * uy + C1, A2 = 2.0 * vxy + C2, B1 = ux * ux + uy * uy + C1, B2 = vx + vy + C2;
    acc += (A1 * A2) / (B1 * B2);
  }
  double v[1] = {acc};
  nhmc_block_sum<1>(v, red);
  if (threadIdx.x == 0) ws[((int64_t)row * C + c) * gridDim.x + tile] = v[0];
}

// One wave per sample: each plane's mean over its window positions, then the mean over the planes.
__global__ void k_ssim_final(const double* __restrict__ ws, int tiles, int C, int64_t n_windows, double* __restrict__ ssim,
                             int rows) {
  const int row = blockIdx.x * (blockDim.x / NHMC_WAVE) + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int lane = threadIdx.x & 63;
  double total = 0.0;
  for (int c = 0; c < C; ++c) {
    const double* part = ws + ((int64_t)row * C + c) * tiles;
    double acc = 0.0;
    for (int t = lane; t < tiles; t += NHMC_WAVE) acc += part[t];
    acc = nhmc_wave_sum(acc);
    total += acc / (double)n_windows;                                   // valid in lane 0
  }
  if (lane == 0) ssim[row] = total / (double)C;
}

// ---- posterior mean and the std map -------------------------------------------------------------
// Thread = one pixel of one chain; per channel the chain's S values of that pixel are read twice (mean, then squared
// deviations about it -- the second read comes from cache), both passes in fp64.
__global__ __launch_bounds__(NHMC_BLOCK) void k_sample_moments(const float* __restrict__ samples, float* __restrict__ mean,
                                                               float* __restrict__ std_map, double* __restrict__ ws,
                                                               int S, int C, int64_t hw) {
  const int chain = blockIdx.y;
  const int64_t p = (int64_t)blockIdx.x * NHMC_BLOCK + threadIdx.x;
  const int64_t n_elem = (int64_t)C * hw;
  float lo = INFINITY, hi = -INFINITY;
  if (p < hw) {
    double std_sum = 0.0;
    for (int c = 0; c < C; ++c) {
      const float* v = samples + (int64_t)chain * S * n_elem + (int64_t)c * hw + p;
      double sr = 0.0, st = 0.0;
      for (int s = 0; s < S; ++s) {
        const float raw = v[(int64_t)s * n_elem];
        sr += (double)raw;
        st += (double)unit_range(raw);
      }
      mean[(int64_t)chain * n_elem + (int64_t)c * hw + p] = (float)(sr / (double)S);
      const double mt = st / (double)S;
      double ss = 0.0;
      for (int s = 0; s < S; ++s) {
        const double d = (double)unit_range(v[(int64_t)s * n_elem]) - mt;
        ss += d * d;
      }
      std_sum += sqrt(ss / (double)(S - 1));                             // x.std(dim=0): unbiased
    }
    const float m = (float)(std_sum / (double)C);                       // .mean(dim=0) over the channels
    std_map[(int64_t)chain * hw + p] = m;
    lo = hi = m;
  }
  __shared__ float red[8];
  block_minmax(lo, hi, red);
  if (threadIdx.x == 0) {
    double* out = ws + ((int64_t)chain * gridDim.x + blockIdx.x) * 2;
    out[0] = (double)lo;
    out[1] = (double)hi;
  }
}

__global__ void k_std_map_minmax(const double* __restrict__ ws, int tiles, float* __restrict__ minmax, int n_chains) {
  const int chain = blockIdx.x * (blockDim.x / NHMC_WAVE) + (threadIdx.x >> 6);
  if (chain >= n_chains) return;
  float lo, hi;
  wave_minmax_pairs(ws + (int64_t)chain * tiles * 2, tiles, lo, hi);
  if ((threadIdx.x & 63) == 0) { minmax[chain * 2] = lo; minmax[chain * 2 + 1] = hi; }
}

__global__ __launch_bounds__(NHMC_BLOCK) void k_std_map_normalise(const float* __restrict__ std_map,
                                                                  const float* __restrict__ minmax,
                                                                  float* __restrict__ out, int64_t hw) {
  const int chain = blockIdx.y;
  const int64_t p = (int64_t)blockIdx.x * NHMC_BLOCK + threadIdx.x;
  if (p >= hw) return;
  const float lo = minmax[chain * 2], hi = minmax[chain * 2 + 1];
  out[(int64_t)chain * hw + p] = (std_map[(int64_t)chain * hw + p] - lo) / (hi - lo);     // :497
}

inline dim3 wave_grid(int n) { return dim3((unsigned)((n + 3) / 4)); }
inline int64_t max64(int64_t a, int64_t b) { return a > b ? a : b; }

}  // namespace

extern "C" int nhmc_ssim_tiles(int h, int w) {
  if (h < SSIM_WIN || w < SSIM_WIN) return 0;
  const int64_t t = (int64_t)((h - SSIM_WIN + 1 + SSIM_TH - 1) / SSIM_TH) * ((w - SSIM_WIN + 1 + SSIM_TW - 1) / SSIM_TW);
  return t > INT32_MAX ? 0 : (int)t;
}

extern "C" size_t nhmc_ssim_ws_bytes(int n_total_samples, int c, int h, int w) {
  if (n_total_samples <= 0 || c <= 0 || h <= 0 || w <= 0) return 0;
  const int64_t ssim = (int64_t)c * nhmc_ssim_tiles(h, w);
  const int64_t range = 2 * (int64_t)nhmc_data_tiles((int64_t)c * h * w);
  return (size_t)n_total_samples * (size_t)max64(ssim, range) * sizeof(double);
}

extern "C" int nhmc_moments_tiles(int64_t hw) { return hw <= 0 ? 0 : (int)((hw + NHMC_BLOCK - 1) / NHMC_BLOCK); }

extern "C" int nhmc_sample_range(const float* samples, float* range, double* ws, int n_total_samples, int64_t n_elem,
                                 nhmc_stream_t stream) {
  if (!samples || !range || !ws || n_total_samples <= 0 || n_elem <= 0) return NHMC_ERR_ARG;
  if ((n_elem & 3) || !nhmc_aligned16(samples)) return NHMC_ERR_ALIGN;
  if (n_total_samples > 65535) return NHMC_ERR_SHAPE;
  const int tiles = nhmc_data_tiles(n_elem);
  NHMC_LAUNCH(k_sample_range_partial, dim3((unsigned)tiles, (unsigned)n_total_samples), dim3(NHMC_BLOCK), 0, nhmc_s(stream),
              (const float4*)samples, ws, n_elem / 4);
  NHMC_LAUNCH(k_sample_range, wave_grid(n_total_samples), dim3(256), 0, nhmc_s(stream), ws, tiles, range, n_total_samples);
  return nhmc_launch_status();
}

extern "C" int nhmc_ssim(const float* samples, const float* x_orig, const float* range, double* ssim, double* ws,
                         int n_chains, int n_samples, int c, int h, int w, nhmc_stream_t stream) {
  if (!samples || !x_orig || !range || !ssim || !ws || n_chains <= 0 || n_samples <= 0 || c <= 0 || h <= 0 || w <= 0)
    return NHMC_ERR_ARG;
  if ((((int64_t)c * h * w) & 3) || !nhmc_aligned16(samples) || !nhmc_aligned16(x_orig)) return NHMC_ERR_ALIGN;
  const int tiles = nhmc_ssim_tiles(h, w);
  if (tiles <= 0 || c > 65535 || (int64_t)n_chains * n_samples > 65535) return NHMC_ERR_SHAPE;
  const int rows = n_chains * n_samples;
  NHMC_LAUNCH(k_ssim_partial, dim3((unsigned)tiles, (unsigned)c, (unsigned)rows), dim3(NHMC_BLOCK), 0, nhmc_s(stream),
              samples, x_orig, range, ws, n_samples, c, h, w, (w - SSIM_WIN + 1 + SSIM_TW - 1) / SSIM_TW);
  NHMC_LAUNCH(k_ssim_final, wave_grid(rows), dim3(256), 0, nhmc_s(stream), ws, tiles, c,
              (int64_t)(h - SSIM_WIN + 1) * (w - SSIM_WIN + 1), ssim, rows);
  return nhmc_launch_status();
}

extern "C" int nhmc_sample_moments(const float* samples, float* mean, float* std_map, float* minmax, double* ws,
                                   int n_chains, int n_samples, int c, int h, int w, nhmc_stream_t stream) {
  if (!samples || !mean || !std_map || !minmax || !ws || n_chains <= 0 || n_samples <= 0 || c <= 0 || h <= 0 || w <= 0)
    return NHMC_ERR_ARG;
  if ((((int64_t)c * h * w) & 3) || !nhmc_aligned16(samples) || !nhmc_aligned16(mean) || !nhmc_aligned16(std_map))
    return NHMC_ERR_ALIGN;
  if (n_samples < 2 || n_chains > 65535) return NHMC_ERR_SHAPE;
  const int64_t hw = (int64_t)h * w;
  const int tiles = nhmc_moments_tiles(hw);
  NHMC_LAUNCH(k_sample_moments, dim3((unsigned)tiles, (unsigned)n_chains), dim3(NHMC_BLOCK), 0, nhmc_s(stream), samples,
              mean, std_map, ws, n_samples, c, hw);
  NHMC_LAUNCH(k_std_map_minmax, wave_grid(n_chains), dim3(256), 0, nhmc_s(stream), ws, tiles, minmax, n_chains);
  return nhmc_launch_status();
}

extern "C" int nhmc_std_map_normalise(const float* std_map, const float* minmax, float* out, int n_chains, int64_t hw,
                                      nhmc_stream_t stream) {
  if (!std_map || !minmax || !out || n_chains <= 0 || hw <= 0) return NHMC_ERR_ARG;
  if (!nhmc_aligned16(std_map) || !nhmc_aligned16(out)) return NHMC_ERR_ALIGN;
  if (n_chains > 65535) return NHMC_ERR_SHAPE;
  NHMC_LAUNCH(k_std_map_normalise, dim3((unsigned)nhmc_moments_tiles(hw), (unsigned)n_chains), dim3(NHMC_BLOCK), 0,
              nhmc_s(stream), std_map, minmax, out, hw);
  return nhmc_launch_status();
}
