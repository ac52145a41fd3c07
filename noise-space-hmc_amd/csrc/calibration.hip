// Calibration of the posterior samples against the original image (nhmc.h "Calibration of the posterior samples"): per
// element the rank of the original among an image's pooled draws, the z-score of the original against their mean and
// standard deviation, and per image six fp64 sums, two counts and the rank histogram.
// Thread = one element of one image; lanes hold consecutive elements, so a wave's load of one draw is one contiguous
// 256-byte row and every sample value leaves HBM once.  The loop over the n draws has a run-time trip count, which the
// compiler does not pipeline: the draws are loaded in batches of CAL_BATCH, the next batch issued before the current one's
// arithmetic; the last n % CAL_BATCH draws are requested first and used last.  Every index into the three
// register batches is a constant after unrolling, nothing goes to scratch.  A block walks `tpb` consecutive tiles of 256 elements: each tile leaves its own fp64 partials (summed by k_calibration_final in a fixed
// order), while the block's LDS histogram is added to the image's once at the end, with integer atomics.
#include <math.h>
#include "nhmc_common.h"

namespace {

constexpr int CAL_WS = 8;            // per-tile partials: the six sums, n_tied, n_flat
constexpr int CAL_BATCH = 16;        // draws in flight per batch; two batches are live
constexpr int CAL_MAX_N = 1024;      // bins: n + 1 <= 1025
constexpr int CAL_BLOCKS = 4096;     // blocks aimed at per launch; more tiles than that are walked tpb per block

__device__ __forceinline__ void cal_load(float (&x)[CAL_BATCH], const float* __restrict__ p, int64_t stride) {
#pragma unroll
  for (int j = 0; j < CAL_BATCH; ++j) x[j] = __builtin_nontemporal_load(p + (int64_t)j * stride);
}

__device__ __forceinline__ void cal_load_tail(float (&x)[CAL_BATCH], const float* __restrict__ p, int cnt, int64_t stride) {
#pragma unroll
  for (int j = 0; j < CAL_BATCH - 1; ++j) x[j] = j < cnt ? __builtin_nontemporal_load(p + (int64_t)j * stride) : 0.0f;
}

struct CalAcc {
  double d1, sum, sq;
  float t;
  int below, equal;
  __device__ __forceinline__ void step(float x) {
    const double d = (double)x - d1;
    sum += d;
    sq = fma(d, d, sq);
    below += x < t ? 1 : 0;
    equal += x == t ? 1 : 0;
  }
};

__global__ void k_calibration_zero(unsigned long long* __restrict__ hist, int64_t count) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < count) hist[i] = 0ull;
}

__global__ __launch_bounds__(NHMC_BLOCK) void k_calibration(const float* __restrict__ samples,
                                                            const float* __restrict__ x_orig, float* __restrict__ z,
                                                            int* __restrict__ counts, unsigned long long* __restrict__ hist,
                                                            double* __restrict__ ws, int n, int64_t n_elem, int tiles,
                                                            int tpb) {
  __shared__ unsigned int bins[CAL_MAX_N + 1];
  __shared__ double red[4 * CAL_WS];
  const int g = blockIdx.y;
  for (int b = threadIdx.x; b <= n; b += NHMC_BLOCK) bins[b] = 0u;
  __syncthreads();
  const double dn = (double)n;
  for (int k = 0; k < tpb; ++k) {
    const int64_t tile = (int64_t)blockIdx.x * tpb + k;
    if (tile >= tiles) break;                                              // block-uniform
    const int64_t e = tile * NHMC_BLOCK + threadIdx.x;
    double part[CAL_WS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (e < n_elem) {
      const float* p = samples + (int64_t)g * n * n_elem + e;            // draw i of the pooled n: row g * n + i
      const int full = n / CAL_BATCH, rem = n - full * CAL_BATCH;         // wave-uniform
      CalAcc acc;
      acc.t = __builtin_nontemporal_load(x_orig + (int64_t)g * n_elem + e);
      acc.sum = 0.0; acc.sq = 0.0; acc.below = 0; acc.equal = 0;
      float cur[CAL_BATCH], nxt[CAL_BATCH], tail[CAL_BATCH];
      cal_load_tail(tail, p + (int64_t)full * CAL_BATCH * n_elem, rem, n_elem);   // the last rem < 16 draws, used last
      if (full > 0) cal_load(cur, p, n_elem);
      acc.d1 = (double)(full > 0 ? cur[0] : tail[0]);
      for (int bi = 0; bi < full; ++bi) {
        const bool more = bi + 1 < full;
        if (more) cal_load(nxt, p + (int64_t)(bi + 1) * CAL_BATCH * n_elem, n_elem);
#pragma unroll
        for (int j = 0; j < CAL_BATCH; ++j) acc.step(cur[j]);
        if (more) {
#pragma unroll
          for (int j = 0; j < CAL_BATCH; ++j) cur[j] = nxt[j];
        }
      }
#pragma unroll
      for (int j = 0; j < CAL_BATCH - 1; ++j)
        if (j < rem) acc.step(tail[j]);
      const double t = (double)acc.t;
      const double mu = acc.d1 + acc.sum / dn;
      const double v = fmax(0.0, (acc.sq - acc.sum * acc.sum / dn) / (dn - 1.0));
      const double s = sqrt(v);
      const double err = t - mu, aerr = fabs(err);
      const double zz = err / s;                                           // s == 0: +-inf, or NaN where t == mu
      __builtin_nontemporal_store((float)zz, z + (int64_t)g * n_elem + e);
      __builtin_nontemporal_store(acc.below + 65536 * acc.equal, counts + (int64_t)g * n_elem + e);
      part[0] = err * err; part[1] = v; part[2] = aerr; part[3] = s; part[4] = aerr * s;
      if (s > 0.0) part[5] = zz * zz; else part[7] = 1.0;
      if (acc.equal > 0) part[6] = 1.0; else atomicAdd(&bins[acc.below], 1u);
    }
    nhmc_block_sum<CAL_WS>(part, red);
    if (threadIdx.x == 0) {
      double* out = ws + ((int64_t)g * tiles + tile) * CAL_WS;
#pragma unroll
      for (int i = 0; i < CAL_WS; ++i) out[i] = part[i];
    }
    __syncthreads();                                                       // red is reused by the next tile
  }
  unsigned long long* h = hist + (int64_t)g * (n + 1);
  for (int b = threadIdx.x; b <= n; b += NHMC_BLOCK) {
    const unsigned int c = bins[b];
    if (c) atomicAdd(&h[b], (unsigned long long)c);
  }
}

// One wave per image: the tiles' partials in a fixed order -> the eight summaries.
__global__ void k_calibration_final(const double* __restrict__ ws, int tiles, double* __restrict__ summary, int n_groups) {
  const int g = blockIdx.x * (blockDim.x / NHMC_WAVE) + (threadIdx.x >> 6);
  if (g >= n_groups) return;
  const int lane = threadIdx.x & 63;
  const double* part = ws + (int64_t)g * tiles * CAL_WS;
  double s[CAL_WS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int t = lane; t < tiles; t += NHMC_WAVE) {
#pragma unroll
    for (int i = 0; i < CAL_WS; ++i) s[i] += part[(int64_t)t * CAL_WS + i];
  }
#pragma unroll
  for (int i = 0; i < CAL_WS; ++i) s[i] = nhmc_wave_sum(s[i]);
  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < CAL_WS; ++i) summary[(int64_t)g * CAL_WS + i] = s[i];
  }
}

}  // namespace

extern "C" int nhmc_calibration_tiles(int64_t n_elem) {
  if (n_elem <= 0) return 0;
  const int64_t t = (n_elem + NHMC_BLOCK - 1) / NHMC_BLOCK;
  return t > INT32_MAX ? 0 : (int)t;
}

extern "C" size_t nhmc_calibration_ws_bytes(int n_groups, int64_t n_elem) {
  if (n_groups <= 0 || n_elem <= 0) return 0;
  return (size_t)n_groups * (size_t)nhmc_calibration_tiles(n_elem) * CAL_WS * sizeof(double);
}

extern "C" int nhmc_calibration(const float* samples, const float* x_orig, float* z, int32_t* counts, int64_t* hist,
                                double* summary, double* ws, int n_groups, int n_replicas, int n_samples, int64_t n_elem,
                                nhmc_stream_t stream) {
  if (!samples || !x_orig || !z || !counts || !hist || !summary || !ws || n_groups <= 0 || n_replicas <= 0 ||
      n_samples <= 0 || n_elem <= 0)
    return NHMC_ERR_ARG;
  if ((n_elem & 3) || !nhmc_aligned16(samples) || !nhmc_aligned16(x_orig) || !nhmc_aligned16(z) || !nhmc_aligned16(counts))
    return NHMC_ERR_ALIGN;
  const int64_t n64 = (int64_t)n_replicas * n_samples;
  const int tiles = nhmc_calibration_tiles(n_elem);
  if (n64 < 2 || n64 > CAL_MAX_N || n_groups > 65535 || tiles <= 0) return NHMC_ERR_SHAPE;
  const int n = (int)n64;
  const int64_t bins = (int64_t)n_groups * (n + 1);
  unsigned long long* h = reinterpret_cast<unsigned long long*>(hist);
  NHMC_LAUNCH(k_calibration_zero, dim3((unsigned)((bins + 255) / 256)), dim3(256), 0, nhmc_s(stream), h, bins);
  const int64_t want = ((int64_t)tiles * n_groups + CAL_BLOCKS - 1) / CAL_BLOCKS;
  const int tpb = (int)(want < 1 ? 1 : want > tiles ? tiles : want);
  NHMC_LAUNCH(k_calibration, dim3((unsigned)((tiles + tpb - 1) / tpb), (unsigned)n_groups), dim3(NHMC_BLOCK), 0,
              nhmc_s(stream), samples, x_orig, z, counts, h, ws, n, n_elem, tiles, tpb);
  NHMC_LAUNCH(k_calibration_final, dim3((unsigned)((n_groups + 3) / 4)), dim3(256), 0, nhmc_s(stream), ws, tiles, summary,
              n_groups);
  return nhmc_launch_status();
}
