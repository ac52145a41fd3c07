// Shared device/host helpers for libnhmc (gfx950 / CDNA4 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/nhmc.h"

#define NHMC_WAVE 64
#define NHMC_BLOCK 256            // 4 waves, one per SIMD of a CU
#define NHMC_VEC_PER_THREAD 2     // float4 per thread per stream -> 2048 elements per tile (measured best: see DESIGN.md)
#define NHMC_TILE (NHMC_BLOCK * NHMC_VEC_PER_THREAD * 4)

static inline bool nhmc_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
static inline hipStream_t nhmc_s(nhmc_stream_t s) { return reinterpret_cast<hipStream_t>(s); }
inline thread_local hipError_t nhmc_last_hip_error = hipSuccess;   // last launch error of this thread (diagnostics)
static inline int nhmc_launch_status() {
  const hipError_t e = hipGetLastError();
  if (e == hipSuccess) return NHMC_OK;
  nhmc_last_hip_error = e;
  return NHMC_ERR_LAUNCH;
}
// hipGetLastError() is per-thread and sticky: the host framework around us leaves benign codes behind
// (e.g. hipErrorNotReady from event polling).  Clear it right before every launch so that
// nhmc_launch_status() reports this launch only.
#define NHMC_LAUNCH(...) do { (void)hipGetLastError(); hipLaunchKernelGGL(__VA_ARGS__); } while (0)

// Wave-level sum over 64 lanes with shuffles; result valid in lane 0.
__device__ __forceinline__ double nhmc_wave_sum(double v) {
#pragma unroll
  for (int off = NHMC_WAVE / 2; off > 0; off >>= 1) v += __shfl_down(v, off, NHMC_WAVE);
  return v;
}

// Block-level sum of up to NV values per thread (256 threads = 4 waves): shuffle inside the
// wave, 4 x NV doubles through LDS, fixed order -> deterministic.  Result valid in thread 0.
template <int NV>
__device__ __forceinline__ void nhmc_block_sum(double (&v)[NV], double* lds /* [4*NV] */) {
  const int lane = threadIdx.x & (NHMC_WAVE - 1), wave = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < NV; ++i) v[i] = nhmc_wave_sum(v[i]);
  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < NV; ++i) lds[wave * NV + i] = v[i];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int i = 0; i < NV; ++i) v[i] = (lds[0 * NV + i] + lds[1 * NV + i]) + (lds[2 * NV + i] + lds[3 * NV + i]);
  }
}

// Sum of an R x R block of pixels held as R float4 strips per lane by LANES = R / 4 adjacent, LANES-aligned lanes of a
// wave, in the REFERENCE'S ORDER: row by row, left to right, one running fp32 sum (SuperResolution.H is a matmul of the
// unfolded patch -- index kh * R + kw -- with a column of +-1/R, Hfuncs.py:188-200: a k-ascending FMA chain with a power-
// of-two weight, i.e. exactly this sequential sum times 1/R^2; so is avg_pool2d).  The running sum is handed from lane to
// lane with shuffles: R * LANES steps.  A pairwise tree over the lanes (round 2) adds the same numbers in another order
// and was 1e-7 off per evaluation, 4.7e-6 after a whole sr16 run.  Returns the block sum in every lane of the group.
template <int R, int LANES>
__device__ __forceinline__ float nhmc_block_sum_rowmajor(const float4 (&v)[R], int lane_in_group) {
  const int lane = threadIdx.x & (NHMC_WAVE - 1), base = lane - lane_in_group;
  float acc = 0.0f;
#pragma unroll
  for (int rr = 0; rr < R; ++rr) {
#pragma unroll
    for (int ln = 0; ln < LANES; ++ln) {
      const float prev = __shfl(acc, base + (ln == 0 ? LANES - 1 : ln - 1), NHMC_WAVE);
      if (lane_in_group == ln) {
        acc = (rr == 0 && ln == 0) ? 0.0f : prev;
        acc += v[rr].x; acc += v[rr].y; acc += v[rr].z; acc += v[rr].w;
      }
    }
  }
  return __shfl(acc, base + LANES - 1, NHMC_WAVE);
}

// Streaming (non-temporal) 16-byte accesses: every image element on this path is touched once per kernel, so
// loads and stores carry the nt hint (measured on MI355X, fused update at B = 64: 49.5 -> 41.8 us).
typedef float nhmc_v4f __attribute__((ext_vector_type(4)));
__device__ __forceinline__ float4 nhmc_ldnt(const float4* p) {
  const nhmc_v4f v = __builtin_nontemporal_load(reinterpret_cast<const nhmc_v4f*>(p));
  return make_float4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ void nhmc_stnt(float4* p, const float4& v) {
  nhmc_v4f w;
  w.x = v.x; w.y = v.y; w.z = v.z; w.w = v.w;
  __builtin_nontemporal_store(w, reinterpret_cast<nhmc_v4f*>(p));
}

// Clamps as torch.clamp: two compares and two selects, so a NaN passes through (fminf / fmaxf -- v_max_f32, v_med3_f32 --
// return a bound for a NaN operand, which would turn a diverged chain's decode into a finite pixel).  Every other input,
// -0.0 included, gets the bits of the min/max form.
__device__ __forceinline__ float nhmc_clamp(float v, float lo, float hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ float nhmc_clip1(float v) { return nhmc_clamp(v, -1.0f, 1.0f); }
__device__ __forceinline__ float nhmc_unit_range(float v) { return nhmc_clamp((v + 1.0f) / 2.0f, 0.0f, 1.0f); }   // inverse_data_transform
__device__ __forceinline__ float nhmc_in1(float v) { return (v >= -1.0f && v <= 1.0f) ? 1.0f : 0.0f; }
// torch's clamp backward SELECTS: the gradient where the mask (nhmc_in1) is set, zero elsewhere, even when the gradient
// is inf or NaN -- g * mask would give inf * 0 = NaN there.  For finite g the two forms are equal.
__device__ __forceinline__ float nhmc_masked(float g, float mask) { return mask != 0.0f ? g : 0.0f; }

// Square roots: plain sqrtf.  hipcc's default -fhip-fp32-correctly-rounded-divide-sqrt makes sqrtf and the fp32 division
// IEEE correctly rounded on gfx950 (no fast-math flag is set in build.py); tests/test_hygiene_gpu.py sweeps all 1001
// alpha-bar table entries through the kernels against numpy's correctly rounded root.

// ---- the forward epilogue of the fused GroupNorm kernels (gn_act.hip, gn_onepass.hip): one definition, the same bits ----
//   u = (x + pre - mean) rstd gamma (1 + scale) + beta (1 + scale) + shift ;   y = act ? u sigmoid(u) : u
// evaluated in fp64 per element and rounded to fp32 once, so an output element is within 1 ulp of the float64
// definition whatever the slab's mean / std is: a chain of fp32 roundings (centring, rstd, FiLM, exp, 1 + e, the
// division, the product) is 3 ulp off on some elements, which a slab of 8 elements does not average out
// (tests/test_gn_conditioning_gpu.py).  The kernels are bandwidth bound and gfx950 issues fp64 FMAs at half the fp32 rate.
struct NhmcGnAffine { double ga, be; };           // gamma (1 + scale), beta (1 + scale) + shift of one (sample, channel)
struct NhmcGnOut { double c, a, b; };             // u = (x + c) a + b
__device__ __forceinline__ NhmcGnAffine nhmc_gn_affine(const float* gamma, const float* beta, const float* film,
                                                       int64_t film_stride, int C, int b, int ch) {
  NhmcGnAffine f{(double)gamma[ch], (double)beta[ch]};
  if (film) {
    const double sc = 1.0 + (double)film[(int64_t)b * film_stride + ch];
    f.ga = f.ga * sc; f.be = fma(f.be, sc, (double)film[(int64_t)b * film_stride + C + ch]);
  }
  return f;
}
__device__ __forceinline__ NhmcGnOut nhmc_gn_out_terms(const NhmcGnAffine& f, float pb, double mean, double rstd) {
  return NhmcGnOut{(double)pb - mean, rstd * f.ga, f.be};
}
// SiLU: exp(-u) is expf at u rounded to fp32 (<= 1 ulp, which 1 / (1 + e) damps to u s (1 - s) 2^-23 <= 0.23 2^-23 of
// the output) times exp(fl(u) - u) = 1 + (fl(u) - u); the reciprocal is the fp32 approximation and one Newton step.
// Below u = -80 the result is u 0 as in fp32, where exp(-u) overflows: -0 for a finite u (|u sigmoid(u)| < 2e-33 there),
// NaN for -inf as torch's SiLU gives; the exponent is held at 80 so that no inf enters the Newton step.  A NaN stays
// one; +inf gives +inf (tests/test_nonfinite_gpu.py::test_group_norm_silu_at_the_ends).
__device__ __forceinline__ float nhmc_gn_out(const NhmcGnOut& k, float x, int act) {
  const double u = fma((double)x + k.c, k.a, k.b);
  if (!act) return (float)u;
  const float uf = (float)u;
  const double du = (uf - uf == 0.0f) ? (double)uf - u : 0.0;
  const double e = (double)expf(fminf(-uf, 80.0f)) * (1.0 + du);
  const double d = 1.0 + e;
  const double s = (double)__builtin_amdgcn_rcpf((float)d);
  return (float)(uf < -80.0f ? u * 0.0 : u * fma(s, fma(-d, s, 1.0), s));
}

// ---- the last DDIM step and its VJP: the one definition every fused "data term + last-step VJP" kernel calls ----------
//   u   = (x - e*c1) / c2         x0 = clip(u)
//   pre = c3*x0 + c4*e            xt_next = clip(pre)  (final_clip)
// The per-chain coefficients are the fp32 roots the reference takes on its [n,1,1,1] tensors.
struct NhmcMix { float c1, c2, c3, c4; };

__device__ __forceinline__ NhmcMix nhmc_mix_coef(const float* at, const float* at_next, int64_t chain) {
  const float a = at[chain], an = at_next[chain];
  NhmcMix k;
  k.c1 = sqrtf(1.0f - a);    // (1 - at).sqrt()
  k.c2 = sqrtf(a);           // at.sqrt()
  k.c3 = sqrtf(an);          // at_next.sqrt()
  k.c4 = sqrtf(1.0f - an);   // (1 - at_next).sqrt()
  return k;
}

// decode: (x, e) -> u (x0 before its clip) and pre (the step's output before the final clip)
__device__ __forceinline__ float nhmc_mix_u(const NhmcMix& k, float x, float e) { return (x - e * k.c1) / k.c2; }
__device__ __forceinline__ float nhmc_mix_pre(const NhmcMix& k, float u, float e) { return k.c3 * nhmc_clip1(u) + k.c4 * e; }
__device__ __forceinline__ void nhmc_mix_decode(const NhmcMix& k, float x, float e, float& u, float& pre) {
  u = nhmc_mix_u(k, x, e);
  pre = nhmc_mix_pre(k, u, e);
}

// The VJP's body, in autograd's rounding order: `gin` is the gradient w.r.t. the step's output (after the final clip's
// mask), `g0` the gradient reaching x0 -- gin*c3 through map_back, except in k_mix_bwd's split form, which is handed it --
// and `mu` = 1[-1 <= u <= 1] the x0 clip's mask.  Every product and the division are rounded separately
// (-ffp-contract=off), the masks select (nhmc_masked): g_xt = (mu ? g0 : 0)/c2, g_e = c4*gin + (-g_xt)*c1.
__device__ __forceinline__ void nhmc_mix_vjp_body(const NhmcMix& k, float gin, float g0, float mu, float& g_xt, float& g_e) {
  const float gu = nhmc_masked(g0, mu) / k.c2;
  g_xt = gu;
  g_e = k.c4 * gin + (-gu) * k.c1;
}

// Entry for kernels that keep u / pre, or only their mask bits mp = 1[-1 <= pre <= 1] and mu, between two passes.
// `gin`: the data term's gradient w.r.t. the clipped decode.
__device__ __forceinline__ void nhmc_mix_vjp_masked(const NhmcMix& k, float gin, float mp, float mu, float& g_xt, float& g_e) {
  gin = nhmc_masked(gin, mp);                                // final clip mask
  nhmc_mix_vjp_body(k, gin, gin * k.c3, mu, g_xt, g_e);
}

// Entry for epilogues that recompute everything from (x, e).
__device__ __forceinline__ void nhmc_mix_vjp(const NhmcMix& k, float gin, float x, float e, float& g_xt, float& g_e) {
  float u, pre;
  nhmc_mix_decode(k, x, e, u, pre);
  nhmc_mix_vjp_masked(k, gin, nhmc_in1(pre), nhmc_in1(u), g_xt, g_e);
}

// Learned-sigma channels of the score gradient are zero (the forward slices them away): the tail of the streaming kernels
// whose tile index t0 runs over [0, n4) float4 per chain.  A caller that keeps a persistent, pre-zeroed g_e buffer passes
// fill = 0 and saves this T of writes.
__device__ __forceinline__ void nhmc_zero_sigma_half(float4* g_e, int64_t ebase, int64_t n4, int64_t e_stride4, int64_t t0, bool fill) {
  const int64_t extra = fill ? e_stride4 - n4 : 0;
  if (extra > 0) {
    const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int i = 0; i < NHMC_VEC_PER_THREAD; ++i) {
      const int64_t q = t0 + (int64_t)i * NHMC_BLOCK;
      if (q < extra) nhmc_stnt(&g_e[ebase + n4 + q], z);
    }
  }
}
