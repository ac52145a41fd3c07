// Credible interval and median of the posterior samples (nhmc.h "Credible interval and median of the posterior samples"):
// per element the order statistics d_(k), the median and d_(n+1-k) of an image's n pooled draws, and per image six fp64
// summaries.  Selecting an order statistic involves no arithmetic, so the maps are exact.
// k_calibration's frame: thread = one element of one image, lanes hold consecutive elements, so a wave's load of one draw
// is one contiguous 256-byte row; grid.y = image, a block walks `tpb` consecutive tiles of 256 elements and every tile
// leaves its own fp64 partials, which k_credible_final sums in a fixed order.
// The draws become order-preserving unsigned keys (cr_key): every NaN is first made the one positive quiet pattern, then
// the sign flip, so that unsigned order is torch.sort's -- ascending, -0.0 just below +0.0, every NaN above +inf -- and a
// compare-exchange is one unsigned min and one unsigned max with no special case.
// Two paths, chosen on the host from n (NHMC_CREDIBLE_PATH=general, read per call, forces the second: the A/B switch of the
// tests).  Both return the same keys, hence the same bits.
//   register path, n <= NMAX in {8, 16, 32, 64}: all draws are requested at once with non-temporal loads (each value
//     leaves HBM once), unused slots hold the largest key, a bitonic network with compile-time indices sorts the NMAX
//     registers and the three (four) wanted ranks are picked by selects over constant indices -- no register is indexed at
//     run time, nothing goes to scratch.
//   general path, n <= 1024: MSB-first radix select on the keys for the four wanted ranks at once, two bits per pass with
//     three named cumulative counters per rank, 16 passes; each pass reads the tile's draws again (from cache where they
//     still are), in batches of CR_BATCH loads ahead of their arithmetic.
#include <math.h>
#include "nhmc_common.h"

#include <cstdlib>
#include <cstring>

namespace {

constexpr int CR_WS = 8;             // per-tile partials: sum_width, max_width, sum_err2, n_inside, n_point, n_nan, n_nan_width, -
constexpr int CR_SUMMARY = 6;
constexpr int CR_BATCH = 16;         // general path: draws in flight per batch
constexpr int CR_MAX_N = 1024;
constexpr int CR_REG_MAX = 64;       // the widest register-path instantiation (128: DESIGN.md section 3)
constexpr int CR_BLOCKS = 4096;      // blocks aimed at per launch; more tiles than that are walked tpb per block
constexpr uint32_t CR_PAD = 0xFFFFFFFFu;   // above every key of a value: the NaN key is 0xFFC00000

__device__ __forceinline__ uint32_t cr_key(float x) {
  uint32_t b = __float_as_uint(x);
  b = x != x ? 0x7FC00000u : b;
  return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}

__device__ __forceinline__ float cr_value(uint32_t key) {
  return __uint_as_float(key ^ ((key >> 31) ? 0x80000000u : 0xFFFFFFFFu));
}

// A wave-uniform value, placed in scalar registers at this point of the program.
__device__ __forceinline__ uint32_t cr_uniform(uint32_t v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ int64_t cr_uniform64(int64_t v) {
  return (int64_t)(((uint64_t)cr_uniform((uint32_t)((uint64_t)v >> 32)) << 32) | cr_uniform((uint32_t)v));
}

__device__ __forceinline__ uint32_t cr_min(uint32_t a, uint32_t b) { return a < b ? a : b; }
__device__ __forceinline__ uint32_t cr_max(uint32_t a, uint32_t b) { return a < b ? b : a; }

// Bitonic sorting network, ascending, on N = 2^LOG registers; every index is a constant after unrolling.
template <int LOG>
__device__ __forceinline__ void cr_sort(uint32_t (&a)[1 << LOG]) {
  constexpr int N = 1 << LOG;
#pragma unroll
  for (int lk = 1; lk <= LOG; ++lk) {
#pragma unroll
    for (int lj = lk - 1; lj >= 0; --lj) {
#pragma unroll
      for (int i = 0; i < N; ++i) {
        const int l = i ^ (1 << lj);
        if (l > i) {
          const uint32_t lo = cr_min(a[i], a[l]), hi = cr_max(a[i], a[l]);
          const bool up = ((i >> lk) & 1) == 0;
          a[i] = up ? lo : hi;
          a[l] = up ? hi : lo;
        }
      }
    }
  }
}

// The three values of one element from its selected keys, and its contribution to the tile's partials.
struct CrOut {
  float lower, median, upper;
};

__device__ __forceinline__ CrOut cr_finish(uint32_t k_lo, uint32_t k_m0, uint32_t k_m1, uint32_t k_hi, bool odd) {
  CrOut o;
  o.lower = cr_value(k_lo);
  o.upper = cr_value(k_hi);
  const float m0 = cr_value(k_m0), m1 = cr_value(k_m1);
  o.median = odd ? m0 : (m0 + m1) * 0.5f;
  return o;
}

__device__ __forceinline__ void cr_partials(const CrOut& o, bool has_t, float t, double (&part)[CR_WS]) {
  const double w = (double)o.upper - (double)o.lower;
  const bool wnan = w != w;
  part[0] = w;
  part[1] = wnan ? 0.0 : w;                                                // the NaN widths are counted in part[6]
  if (has_t) {
    const double err = (double)t - (double)o.median;
    part[2] = err * err;
    part[3] = (o.lower <= t && t <= o.upper) ? 1.0 : 0.0;
  }
  part[4] = o.upper == o.lower ? 1.0 : 0.0;
  part[5] = o.upper != o.upper ? 1.0 : 0.0;
  part[6] = wnan ? 1.0 : 0.0;
}

// Block sums of the partials (fixed order) with the block maximum of part[1]; the result is valid in thread 0.
__device__ __forceinline__ void cr_block_reduce(double (&part)[CR_WS], double* red /* [4 * CR_WS] */, double* redmax /* [4] */) {
  double m = part[1];
#pragma unroll
  for (int off = NHMC_WAVE / 2; off > 0; off >>= 1) m = fmax(m, __shfl_down(m, off, NHMC_WAVE));
  if ((threadIdx.x & (NHMC_WAVE - 1)) == 0) redmax[threadIdx.x >> 6] = m;
  nhmc_block_sum<CR_WS>(part, red);                                        // holds the __syncthreads that publishes redmax
  if (threadIdx.x == 0) part[1] = fmax(fmax(redmax[0], redmax[1]), fmax(redmax[2], redmax[3]));
}

__device__ __forceinline__ void cr_store(const CrOut& o, float* __restrict__ lower, float* __restrict__ median,
                                         float* __restrict__ upper, int64_t at) {
  __builtin_nontemporal_store(o.lower, lower + at);
  __builtin_nontemporal_store(o.median, median + at);
  __builtin_nontemporal_store(o.upper, upper + at);
}

template <int LOG>
__global__ __launch_bounds__(NHMC_BLOCK) void k_credible_reg(const float* __restrict__ samples,
                                                             const float* __restrict__ x_orig, float* __restrict__ lower,
                                                             float* __restrict__ median, float* __restrict__ upper,
                                                             double* __restrict__ ws, int n_arg, int k_arg,
                                                             int64_t n_elem, int tiles, int tpb) {
  constexpr int NMAX = 1 << LOG;
  __shared__ double red[4 * CR_WS];
  __shared__ double redmax[4];
  const int g = blockIdx.y;
  const bool has_t = x_orig != nullptr;
  for (int b = 0; b < tpb; ++b) {
    const int64_t tile = (int64_t)blockIdx.x * tpb + b;
    if (tile >= tiles) break;                                              // block-uniform
    const int64_t e = tile * NHMC_BLOCK + threadIdx.x;
    double part[CR_WS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (e < n_elem) {
      // Everything the unrolled code below derives from n, k and the tile's base goes through cr_uniform inside the tile
      // loop: left loop-invariant, the NMAX row addresses (a vector pair each) and the 5 NMAX comparisons with j are hoisted
      // out of the loop and held across it, which cost 256 VGPRs at NMAX = 64.
      const int n = (int)cr_uniform(n_arg), k = (int)cr_uniform(k_arg);
      const int i_lo = k - 1, i_hi = n - k, i_m0 = (n - 1) >> 1, i_m1 = n >> 1;  // 0-based ranks; i_m0 == i_m1 for odd n
      // draw i of the pooled n: row g * n + i.  The row's base is wave-uniform and walks on by n_elem in scalar registers;
      // the lane adds threadIdx.x
      const float* row = samples + cr_uniform64((int64_t)g * n * n_elem + tile * NHMC_BLOCK);
      float x[NMAX];
#pragma unroll
      for (int j = 0; j < NMAX; ++j) {
        x[j] = j < n ? __builtin_nontemporal_load(row + threadIdx.x) : 0.0f;
        row += n_elem;
      }
      const float t = has_t ? __builtin_nontemporal_load(x_orig + (int64_t)g * n_elem + e) : 0.0f;
      uint32_t a[NMAX];
#pragma unroll
      for (int j = 0; j < NMAX; ++j) a[j] = j < n ? cr_key(x[j]) : CR_PAD;
      cr_sort<LOG>(a);
      uint32_t k_lo = 0u, k_hi = 0u, k_m0 = 0u, k_m1 = 0u;
#pragma unroll
      for (int j = 0; j < NMAX; ++j) {
        if (j < NMAX / 2) k_lo = j == i_lo ? a[j] : k_lo;                 // k - 1 < n / 2 <= NMAX / 2
        if (j < NMAX / 2) k_m0 = j == i_m0 ? a[j] : k_m0;
        if (j <= NMAX / 2) k_m1 = j == i_m1 ? a[j] : k_m1;
        k_hi = j == i_hi ? a[j] : k_hi;
      }
      const CrOut o = cr_finish(k_lo, k_m0, k_m1, k_hi, (n & 1) != 0);
      cr_store(o, lower, median, upper, (int64_t)g * n_elem + e);
      cr_partials(o, has_t, t, part);
    }
    cr_block_reduce(part, red, redmax);
    if (threadIdx.x == 0) {
      double* out = ws + ((int64_t)g * tiles + tile) * CR_WS;
#pragma unroll
      for (int i = 0; i < CR_WS; ++i) out[i] = part[i];
    }
    __syncthreads();                                                       // red and redmax are reused by the next tile
  }
}

// One rank of the radix select: `prefix` holds the bits decided so far (zeros below), `r` the rank among the draws that
// match them; c0 <= c1 <= c2 count the matching draws whose next two bits are <= 0, <= 1, <= 2.
struct CrRank {
  uint32_t prefix;
  int r, c0, c1, c2;
  __device__ __forceinline__ void count(uint32_t key, int shift) {
    const uint32_t v = (key ^ prefix) >> shift;                            // < 4 exactly when the decided bits match
    c0 += v == 0u ? 1 : 0;
    c1 += v <= 1u ? 1 : 0;
    c2 += v <= 2u ? 1 : 0;
  }
  __device__ __forceinline__ void decide(int shift) {
    const uint32_t d = (r >= c0 ? 1u : 0u) + (r >= c1 ? 1u : 0u) + (r >= c2 ? 1u : 0u);
    r -= d == 0u ? 0 : d == 1u ? c0 : d == 2u ? c1 : c2;
    prefix |= d << shift;
    c0 = 0; c1 = 0; c2 = 0;
  }
};

__global__ __launch_bounds__(NHMC_BLOCK) void k_credible_radix(const float* __restrict__ samples,
                                                               const float* __restrict__ x_orig, float* __restrict__ lower,
                                                               float* __restrict__ median, float* __restrict__ upper,
                                                               double* __restrict__ ws, int n, int k, int64_t n_elem,
                                                               int tiles, int tpb) {
  __shared__ double red[4 * CR_WS];
  __shared__ double redmax[4];
  const int g = blockIdx.y;
  const bool has_t = x_orig != nullptr;
  for (int b = 0; b < tpb; ++b) {
    const int64_t tile = (int64_t)blockIdx.x * tpb + b;
    if (tile >= tiles) break;                                              // block-uniform
    const int64_t e = tile * NHMC_BLOCK + threadIdx.x;
    double part[CR_WS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (e < n_elem) {
      const float* p = samples + (int64_t)g * n * n_elem + tile * NHMC_BLOCK;   // wave-uniform; the lane adds threadIdx.x
      CrRank lo = {0u, k - 1, 0, 0, 0}, m0 = {0u, (n - 1) >> 1, 0, 0, 0}, m1 = {0u, n >> 1, 0, 0, 0},
             hi = {0u, n - k, 0, 0, 0};
      for (int shift = 30; shift >= 0; shift -= 2) {
        for (int base = 0; base < n; base += CR_BATCH) {
          const int cnt = n - base;                                        // wave-uniform
          float x[CR_BATCH];
#pragma unroll
          for (int j = 0; j < CR_BATCH; ++j) x[j] = j < cnt ? p[(int64_t)(base + j) * n_elem + threadIdx.x] : 0.0f;
#pragma unroll
          for (int j = 0; j < CR_BATCH; ++j) {
            if (j < cnt) {
              const uint32_t key = cr_key(x[j]);
              lo.count(key, shift); m0.count(key, shift); m1.count(key, shift); hi.count(key, shift);
            }
          }
        }
        lo.decide(shift); m0.decide(shift); m1.decide(shift); hi.decide(shift);
      }
      const float t = has_t ? __builtin_nontemporal_load(x_orig + (int64_t)g * n_elem + e) : 0.0f;
      const CrOut o = cr_finish(lo.prefix, m0.prefix, m1.prefix, hi.prefix, (n & 1) != 0);
      cr_store(o, lower, median, upper, (int64_t)g * n_elem + e);
      cr_partials(o, has_t, t, part);
    }
    cr_block_reduce(part, red, redmax);
    if (threadIdx.x == 0) {
      double* out = ws + ((int64_t)g * tiles + tile) * CR_WS;
#pragma unroll
      for (int i = 0; i < CR_WS; ++i) out[i] = part[i];
    }
    __syncthreads();
  }
}

// One wave per image: the tiles' partials in a fixed order -> the six summaries.
__global__ void k_credible_final(const double* __restrict__ ws, int tiles, double* __restrict__ summary, int n_groups,
                                 int has_t) {
  const int g = blockIdx.x * (blockDim.x / NHMC_WAVE) + (threadIdx.x >> 6);
  if (g >= n_groups) return;
  const int lane = threadIdx.x & 63;
  const double* part = ws + (int64_t)g * tiles * CR_WS;
  double s[CR_WS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  double m = 0.0;
  for (int t = lane; t < tiles; t += NHMC_WAVE) {
#pragma unroll
    for (int i = 0; i < CR_WS; ++i) s[i] += part[(int64_t)t * CR_WS + i];
    m = fmax(m, part[(int64_t)t * CR_WS + 1]);
  }
#pragma unroll
  for (int i = 0; i < CR_WS; ++i) s[i] = nhmc_wave_sum(s[i]);
#pragma unroll
  for (int off = NHMC_WAVE / 2; off > 0; off >>= 1) m = fmax(m, __shfl_down(m, off, NHMC_WAVE));
  if (lane == 0) {
    double* out = summary + (int64_t)g * CR_SUMMARY;
    const double nan = __longlong_as_double(0x7FF8000000000000ll);
    out[0] = s[0];
    out[1] = s[6] > 0.0 ? nan : m;                                         // a NaN width is never turned into a number
    out[2] = has_t ? s[2] : nan;
    out[3] = has_t ? s[3] : nan;
    out[4] = s[4];
    out[5] = s[5];
  }
}

// NHMC_CREDIBLE_PATH, read per call: "general" sends every n through the radix select; unset, empty or "register" leaves
// the choice to n.  -1: the variable holds something else.
int cr_forced_general() {
  const char* v = std::getenv("NHMC_CREDIBLE_PATH");
  if (!v || !*v || !std::strcmp(v, "register")) return 0;
  if (!std::strcmp(v, "general")) return 1;
  return -1;
}

}  // namespace

extern "C" int nhmc_credible_tiles(int64_t n_elem) {
  if (n_elem <= 0) return 0;
  const int64_t t = (n_elem + NHMC_BLOCK - 1) / NHMC_BLOCK;
  return t > INT32_MAX ? 0 : (int)t;
}

extern "C" size_t nhmc_credible_ws_bytes(int n_groups, int64_t n_elem) {
  if (n_groups <= 0 || n_elem <= 0) return 0;
  return (size_t)n_groups * (size_t)nhmc_credible_tiles(n_elem) * CR_WS * sizeof(double);
}

extern "C" int nhmc_credible(const float* samples, const float* x_orig, float* lower, float* median, float* upper,
                             double* summary, double* ws, int n_groups, int n_replicas, int n_samples, int64_t n_elem, int k,
                             nhmc_stream_t stream) {
  if (!samples || !lower || !median || !upper || !summary || !ws || n_groups <= 0 || n_replicas <= 0 || n_samples <= 0 ||
      n_elem <= 0)
    return NHMC_ERR_ARG;
  if ((n_elem & 3) || !nhmc_aligned16(samples) || !nhmc_aligned16(x_orig) || !nhmc_aligned16(lower) ||
      !nhmc_aligned16(median) || !nhmc_aligned16(upper))
    return NHMC_ERR_ALIGN;
  const int64_t n64 = (int64_t)n_replicas * n_samples;
  const int tiles = nhmc_credible_tiles(n_elem);
  if (n64 < 2 || n64 > CR_MAX_N || n_groups > 65535 || tiles <= 0 || k < 1 || k > n64 / 2) return NHMC_ERR_SHAPE;
  const int forced = cr_forced_general();
  if (forced < 0) return NHMC_ERR_ARG;
  const int n = (int)n64;
  const int64_t want = ((int64_t)tiles * n_groups + CR_BLOCKS - 1) / CR_BLOCKS;
  const int tpb = (int)(want < 1 ? 1 : want > tiles ? tiles : want);
  const dim3 grid((unsigned)((tiles + tpb - 1) / tpb), (unsigned)n_groups), block(NHMC_BLOCK);
#define CR_REG(LOG)                                                                                                     \
  NHMC_LAUNCH(k_credible_reg<LOG>, grid, block, 0, nhmc_s(stream), samples, x_orig, lower, median, upper, ws, n, k, n_elem, \
              tiles, tpb)
  if (forced || n > CR_REG_MAX)
    NHMC_LAUNCH(k_credible_radix, grid, block, 0, nhmc_s(stream), samples, x_orig, lower, median, upper, ws, n, k, n_elem,
                tiles, tpb);
  else if (n <= 8) CR_REG(3);
  else if (n <= 16) CR_REG(4);
  else if (n <= 32) CR_REG(5);
  else CR_REG(6);
#undef CR_REG
  NHMC_LAUNCH(k_credible_final, dim3((unsigned)((n_groups + 3) / 4)), dim3(256), 0, nhmc_s(stream), ws, tiles, summary,
              n_groups, x_orig ? 1 : 0);
  return nhmc_launch_status();
}
