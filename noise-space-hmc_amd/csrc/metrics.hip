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

__device__ __forceinline__ float unit_range(float v) { return nhmc_unit_range(v); }   // NaN stays NaN (nhmc_common.h)

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

// ---- split R-hat and ESS of K replica chains per element (nhmc.h "Convergence of replica chains") ----------------------
// Thread = one element of one image; lanes hold consecutive elements, so every (replica, draw) load of a wave is one
// contiguous 256-byte row and each sample value leaves HBM once.  The n draws of the current split chain sit in registers
// (NMAX is a compile-time bound on n: every index below is a constant after unrolling, nothing goes to scratch), the next
// split chain's draws are already in flight while this one's autocovariances are summed.  acc[t] = sum over the split
// chains of sum_i d_i d_{i+t} (the 1/n is applied once at the end); the means enter as offsets from the first split
// chain's mean, so chains stuck at one common value give Bn = 0 exactly whatever that value is.
constexpr int DIAG_WS = 8;       // per-tile partials: rhat max, sum, finite count, count above; ess min, sum, count; constant

template <int NMAX>
__device__ __forceinline__ void diag_load(float (&x)[NMAX], const float* __restrict__ p, int n, int64_t stride) {
#pragma unroll
  for (int i = 0; i < NMAX; ++i) x[i] = i < n ? __builtin_nontemporal_load(p + (int64_t)i * stride) : 0.0f;
}

__device__ __forceinline__ const float* diag_split(const float* base, int m, int S, int n, int64_t n_elem) {
  return base + ((int64_t)(m >> 1) * S + ((m & 1) ? S - n : 0)) * n_elem;      // split 2r: draws [0, n); 2r+1: [S-n, S)
}

// Block-level min of lo and max of hi (256 threads, doubles); result valid in thread 0.
__device__ __forceinline__ void block_minmax_f64(double& lo, double& hi, double* lds /* [8] */) {
  const int lane = threadIdx.x & (NHMC_WAVE - 1), wave = threadIdx.x >> 6;
#pragma unroll
  for (int off = NHMC_WAVE / 2; off > 0; off >>= 1) {
    lo = fmin(lo, __shfl_down(lo, off, NHMC_WAVE));
    hi = fmax(hi, __shfl_down(hi, off, NHMC_WAVE));
  }
  if (lane == 0) { lds[wave * 2] = lo; lds[wave * 2 + 1] = hi; }
  __syncthreads();
  if (threadIdx.x == 0) {
    lo = fmin(fmin(lds[0], lds[2]), fmin(lds[4], lds[6]));
    hi = fmax(fmax(lds[1], lds[3]), fmax(lds[5], lds[7]));
  }
}

template <int NMAX>
__global__ __launch_bounds__(NHMC_BLOCK) void k_chain_diag(const float* __restrict__ samples, float* __restrict__ rhat,
                                                           float* __restrict__ ess, double* __restrict__ ws, int K, int S,
                                                           int n, int64_t n_elem, double threshold) {
  const int g = blockIdx.y;
  const int64_t e = (int64_t)blockIdx.x * NHMC_BLOCK + threadIdx.x;
  const int M = 2 * K;
  double part[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};   // rhat sum, finite rhats, rhats above, ess sum, ess count, constant
  double r_max = -INFINITY, e_min = INFINITY;
  if (e < n_elem) {
    const float* base = samples + (int64_t)g * K * S * n_elem + e;
    double acc[NMAX - 1];
#pragma unroll
    for (int t = 0; t < NMAX - 1; ++t) acc[t] = 0.0;
    double mu0 = 0.0, sm = 0.0, sq = 0.0;
    float cur[NMAX], nxt[NMAX];
    diag_load<NMAX>(cur, diag_split(base, 0, S, n, n_elem), n, n_elem);
    for (int m = 0; m < M; ++m) {
      if (m + 1 < M) diag_load<NMAX>(nxt, diag_split(base, m + 1, S, n, n_elem), n, n_elem);
      double sum = 0.0;
#pragma unroll
      for (int i = 0; i < NMAX; ++i) sum += (double)cur[i];               // entries past n are zero
      const double mu = sum / (double)n;
      double d[NMAX];
#pragma unroll
      for (int i = 0; i < NMAX; ++i) d[i] = i < n ? (double)cur[i] - mu : 0.0;
#pragma unroll
      for (int t = 0; t < NMAX - 1; ++t) {
        if (t <= n - 2 || t == 0) {                                       // wave-uniform
          double s = 0.0;
#pragma unroll
          for (int i = 0; i + t < NMAX; ++i) s = fma(d[i], d[i + t], s);
          acc[t] += s;
        }
      }
      if (m == 0) mu0 = mu;
      const double dm = mu - mu0;
      sm += dm;
      sq = fma(dm, dm, sq);
      if (m + 1 < M) {
#pragma unroll
        for (int i = 0; i < NMAX; ++i) cur[i] = nxt[i];
      }
    }
    const double dn = (double)n, dM = (double)M;
    const double W = (acc[0] / dn / dM) * (dn / (dn - 1.0));
    const double Bn = fmax((sq - sm * sm / dM) / (dM - 1.0), 0.0);
    const double V = W * (dn - 1.0) / dn + Bn;
    double r = NAN, es = NAN;
    if (V == 0.0) {
      part[5] = 1.0;
    } else if (W == 0.0) {
      r = INFINITY;
    } else {
      r = sqrt(V / W);
      double sum_p = 0.0, prev = INFINITY;
      bool go = true;
#pragma unroll
      for (int k = 0; 2 * k + 1 <= NMAX - 2; ++k) {
        if (2 * k + 1 <= n - 2) {                                         // wave-uniform
          const double rho0 = k == 0 ? 1.0 : 1.0 - (W - acc[2 * k] / dn / dM) / V;
          const double rho1 = 1.0 - (W - acc[2 * k + 1] / dn / dM) / V;
          double p = rho0 + rho1;
          go = go && p > 0.0;
          if (go) {
            p = fmin(p, prev);
            prev = p;
            sum_p += p;
          }
        }
      }
      const double tau = fmax(-1.0 + 2.0 * sum_p, 1.0 / log10(dM * dn));
      es = dM * dn / tau;
    }
    rhat[(int64_t)g * n_elem + e] = (float)r;
    ess[(int64_t)g * n_elem + e] = (float)es;
    if (r == r) {
      r_max = r;
      if (r < INFINITY) { part[0] = r; part[1] = 1.0; }
      if (r > threshold) part[2] = 1.0;
    }
    if (es == es) { e_min = es; part[3] = es; part[4] = 1.0; }
  }
  __shared__ double red[24], red_mm[8];
  nhmc_block_sum<6>(part, red);
  block_minmax_f64(e_min, r_max, red_mm);
  if (threadIdx.x == 0) {
    double* out = ws + ((int64_t)g * gridDim.x + blockIdx.x) * DIAG_WS;
    out[0] = r_max; out[1] = part[0]; out[2] = part[1]; out[3] = part[2];
    out[4] = e_min; out[5] = part[3]; out[6] = part[4]; out[7] = part[5];
  }
}

// One wave per image: the tiles' partials in a fixed order -> the six summaries.
__global__ void k_chain_diag_final(const double* __restrict__ ws, int tiles, int64_t n_elem, double* __restrict__ summary,
                                   int n_groups) {
  const int g = blockIdx.x * (blockDim.x / NHMC_WAVE) + (threadIdx.x >> 6);
  if (g >= n_groups) return;
  const int lane = threadIdx.x & 63;
  const double* part = ws + (int64_t)g * tiles * DIAG_WS;
  double r_max = -INFINITY, e_min = INFINITY, s[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int t = lane; t < tiles; t += NHMC_WAVE) {
    const double* p = part + (int64_t)t * DIAG_WS;
    r_max = fmax(r_max, p[0]);
    e_min = fmin(e_min, p[4]);
    s[0] += p[1]; s[1] += p[2]; s[2] += p[3]; s[3] += p[5]; s[4] += p[6]; s[5] += p[7];
  }
#pragma unroll
  for (int off = NHMC_WAVE / 2; off > 0; off >>= 1) {
    r_max = fmax(r_max, __shfl_down(r_max, off, NHMC_WAVE));
    e_min = fmin(e_min, __shfl_down(e_min, off, NHMC_WAVE));
  }
#pragma unroll
  for (int i = 0; i < 6; ++i) s[i] = nhmc_wave_sum(s[i]);
  if (lane == 0) {
    const double varying = (double)n_elem - s[5];
    double* out = summary + (int64_t)g * 6;
    out[0] = varying > 0.0 ? r_max : NAN;
    out[1] = s[0] / s[1];
    out[2] = s[2] / varying;
    out[3] = s[4] > 0.0 ? e_min : NAN;
    out[4] = s[3] / s[4];
    out[5] = s[5];
  }
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

extern "C" int nhmc_chain_diag_tiles(int64_t n_elem) {
  if (n_elem <= 0) return 0;
  const int64_t t = (n_elem + NHMC_BLOCK - 1) / NHMC_BLOCK;
  return t > INT32_MAX ? 0 : (int)t;
}

extern "C" size_t nhmc_chain_diag_ws_bytes(int n_groups, int64_t n_elem) {
  if (n_groups <= 0 || n_elem <= 0) return 0;
  return (size_t)n_groups * (size_t)nhmc_chain_diag_tiles(n_elem) * DIAG_WS * sizeof(double);
}

extern "C" int nhmc_chain_diag(const float* samples, float* rhat, float* ess, double* summary, double* ws, int n_groups,
                               int n_replicas, int n_samples, int64_t n_elem, double rhat_threshold, nhmc_stream_t stream) {
  if (!samples || !rhat || !ess || !summary || !ws || n_groups <= 0 || n_replicas <= 0 || n_samples <= 0 || n_elem <= 0)
    return NHMC_ERR_ARG;
  if ((n_elem & 3) || !nhmc_aligned16(samples) || !nhmc_aligned16(rhat) || !nhmc_aligned16(ess)) return NHMC_ERR_ALIGN;
  const int n = n_samples / 2;
  const int tiles = nhmc_chain_diag_tiles(n_elem);
  if (n_samples < 4 || n > 32 || (int64_t)n_replicas * n_samples > 4096 || n_groups > 65535 || tiles <= 0)
    return NHMC_ERR_SHAPE;
  const dim3 grid((unsigned)tiles, (unsigned)n_groups);
#define NHMC_DIAG(NMAX)                                                                                             \
  NHMC_LAUNCH(k_chain_diag<NMAX>, grid, dim3(NHMC_BLOCK), 0, nhmc_s(stream), samples, rhat, ess, ws, n_replicas, \
              n_samples, n, n_elem, rhat_threshold)
  if (n <= 4) NHMC_DIAG(4);
  else if (n <= 10) NHMC_DIAG(10);
  else if (n <= 16) NHMC_DIAG(16);
  else NHMC_DIAG(32);
#undef NHMC_DIAG
  NHMC_LAUNCH(k_chain_diag_final, wave_grid(n_groups), dim3(256), 0, nhmc_s(stream), ws, tiles, n_elem, summary, n_groups);
  return nhmc_launch_status();
}
