// One-pass GroupNorm (+ FiLM scale/shift) (+ SiLU), forward and input gradient: every activation crosses HBM once per call.
//
// Pass arithmetic.  The two-pass kernels of gn_act.hip read x (and dy) twice, because the statistics of a (sample, group)
// slab must be complete before any element of it can be normalised and the two halves are separate launches over a
// tensor far larger than the Infinity Cache:
//     forward   k_gn_stats (R x)     -> k_gn_apply (R x, W y)                   2 reads + 1 write
//     backward  k_gn_stats (R x, dy) -> k_gn_apply (R x, dy [, acc], W dx)      4 (5) reads + 1 write
// Here a slab is spread over `splits` workgroups of one launch, each of which loads its share (256 threads x 8 float4 of x,
// in the backward also of dy) into registers ONCE, reduces it, exchanges the 16-byte partial with the other workgroups
// of its slab and then normalises / differentiates its share from registers:
//     forward   k_gn_onepass<false, *> (R x, W y)                               1 read  + 1 write
//     backward  k_gn_onepass<true, *>  (R x, dy [, acc], W dx)                  2 (3) reads + 1 write
// The formulas, the fp64 partial sums, their fixed summation order k = 0 .. splits - 1 and the workspace layout
// ws[(bg * splits + split) * 2 ..] are those of gn_act.hip, so a forward workspace of either path feeds either backward.
// As there, the forward's sums of v = x + pre and v^2 are fp64 from the element on (widened, added and squared per
// float4, per thread, per workgroup in fp64): var = E[v^2] - mean^2 cancels and tolerates no square rounded to fp32;
// the forward's output is evaluated in fp64 per element and rounded once (nhmc_gn_out of nhmc_common.h, the one
// definition both files call); the backward centres x + pre - mean from the fp64 mean (op_centre) and goes on in fp32.
// The backward's sums are fp32 inside a float4, fp64 across.
//
// The wait protocol (agent scope, placement independent; "the data is the flag").  The entry point fills the workspace
// with the byte 0xFF by a small launch of its own (k_gn_ws_fill) on the same stream ahead of every launch; no partial sum can have
// that bit pattern.  Thread 0 of a workgroup stores its two fp64 partials with relaxed agent-scope atomic stores (8-byte, write-
// through, vector path).  The lanes of its first wave then poll one slot of the slab each -- relaxed agent-scope atomic
// loads, which bypass this CU's L1, s_sleep between sweeps -- until no word of the slab holds the fill pattern any more;
// what they have loaded then IS the data, and thread 0 adds it in the fixed order.  (A first version with a ticket
// counter -- drain, fetch_add, polls of one word, then one lane reading all partials in a loop -- measured 3-4 x the
// two-pass time at the 256x256 level.)
// No other load of this kernel touches bytes that another workgroup writes in the same launch.
//
// Why the result does not depend on scheduling.  Dispatch order and co-residency are not guaranteed, so the wait is
// bounded: when the poll limit expires the workgroup stops waiting and computes the partials of the other shares of its
// slab itself, from memory, split by split, with the thread-to-element mapping and the reduction order of the owning
// workgroup -- the same numbers bit for bit (the file is built without fp contraction, one code path forms a partial).
// That is the two-pass cost for that one workgroup and nothing worse; no workgroup can spin without end, and the bits of
// the output do not tell whether the fallback ran (flag NHMC_GN_ONEPASS_NOWAIT forces it everywhere, for the tests).
// A slab that fits one workgroup (splits == 1) takes no fill and no wait.
//
// Behind the partials the forward leaves the slab totals, ws[n * groups * splits * 2 + bg * 2 ..] (a workspace of one
// split): a backward that reads those needs one pair of loads per workgroup whatever the forward's split count was.
//
// The per-channel terms (pre, gamma, beta, FiLM) of a slab's channels are formed once per workgroup into LDS (groups of up
// to 64 channels; wider groups read them from memory per float4): per float4 they cost an LDS read instead of up to five
// dependent global loads, each of which the compiler follows with a full s_waitcnt.  The backward's table also holds the
// centre (op_centre), which it can form per channel because it knows the mean before it loads its share.
//
// Instruction issue, not HBM, bounds these kernels (profiles/README.md, round 17), so each element's work is done once:
// the backward's statistics loop leaves xh and dxh = du * ga in the registers that held x and dy, and the output is
// rstd * ((dxh - m0) - xh * m1) from those -- no second sigmoid, no channel terms, no plane index in the last loop.
// Where a channel plane is a whole multiple of the 256 float4 of one float4 index of a share (every FFHQ level from
// 32 x 32 up), plane, channel and source / destination side are the workgroup's and live in scalar registers
// (template parameter UNI, OpWalk below); the general path finds them per lane by a division.
//
// Concatenated input (the U-Net's output blocks): the forward may take the logical input as two tensors
// x1 [n][C1][hw] | x2 [n][C - C1][hw] and then also writes their concatenation x_cat from the same load; the backward
// may write dx as two contiguous tensors of those shapes.  The source / destination is chosen per channel plane
// (hw % 4 == 0 keeps a float4 inside one plane); a group may straddle C1.
#include <cstdlib>

#include "nhmc_common.h"

namespace {

constexpr int OP_K = 8;                          // float4 per thread held in registers (32 VGPRs of x, 32 of dy)
constexpr int OP_SHARE = NHMC_BLOCK * OP_K;      // float4 per workgroup
constexpr int OP_MAX_SPLITS = 64;
constexpr unsigned OP_POLLS = 2048;              // bounded wait: a few milliseconds, then the fallback
// what k_gn_ws_fill leaves ahead of a launch in every word of the partials: no sum of fp32-derived values has this bit pattern (a NaN
// whose payload is all ones down to the last bit; fp32 -> fp64 conversion leaves the low 29 bits zero)
constexpr unsigned long long OP_EMPTY = ~0ull;

struct OpArgs {
  const float* gamma; const float* beta;          // [C]
  const float* film; int64_t film_stride;         // nullable, as in gn_act.hip
  const float* pre; int64_t pre_stride;           // nullable, as in gn_act.hip
  int C, G, C1;                                   // C1: channels of the first source / destination (== C without a second)
  int hw4, n4;                                    // float4 per channel plane, per (sample, group) slab
  float eps; int act; int splits, fwd_splits; unsigned polls;
};

__device__ __forceinline__ float op_sigmoid(float u) { return 1.0f / (1.0f + expf(-u)); }

// float4 index of slab element q (plane pl of the group, offset p4 inside it) in a tensor of `ch_total` channels
__device__ __forceinline__ int64_t op_index(int b, int ch_total, int ch, int hw4, int p4) {
  return ((int64_t)b * ch_total + ch) * hw4 + p4;
}

// nhmc_block_sum<2> in its arithmetic ((wave 0 + wave 1) + (wave 2 + wave 3), result in thread 0), with the two values
// summed one after the other: thread 0 then holds 4 doubles of LDS data at a time instead of 8, which matters where the
// backward's 64 data registers are live around it.  lds: double[8].
__device__ __forceinline__ void op_block_sum(double (&v)[2], double* lds) {
  const int lane = threadIdx.x & (NHMC_WAVE - 1), wave = threadIdx.x >> 6;
  v[0] = nhmc_wave_sum(v[0]); v[1] = nhmc_wave_sum(v[1]);
  if (lane == 0) { lds[wave] = v[0]; lds[4 + wave] = v[1]; }
  __syncthreads();
  if (threadIdx.x == 0) {
    v[0] = (lds[0] + lds[1]) + (lds[2] + lds[3]);
    __builtin_amdgcn_sched_barrier(0);
    v[1] = (lds[4] + lds[5]) + (lds[6] + lds[7]);
  }
}

constexpr int OP_CHAN_LDS = 64;                  // channels per group whose terms are staged in LDS
struct OpChan { float pb, ga, be, hi, lo; };       // hi + lo = pb - mean (op_centre), where the mean is known
// the terms of one (sample, channel) from memory
template <bool AFFINE>
__device__ __forceinline__ OpChan op_chan(const OpArgs& a, int b, int ch) {
  OpChan c;
  c.hi = c.lo = 0.0f;
  c.pb = a.pre ? a.pre[(int64_t)b * a.pre_stride + ch] : 0.0f;
  c.ga = c.be = 0.0f;
  if (AFFINE) {
    c.ga = a.gamma[ch]; c.be = a.beta[ch];
    if (a.film) { const float sc = 1.0f + a.film[(int64_t)b * a.film_stride + ch]; c.ga *= sc; c.be = c.be * sc + a.film[(int64_t)b * a.film_stride + a.C + ch]; }
  }
  return c;
}

// x + pre - mean is (x + hi) + lo, hi + lo split from fp64: gn_centre of gn_act.hip
__device__ __forceinline__ OpChan op_centre(OpChan c, double mean) {
  const double d = (double)c.pb - mean;
  c.hi = (float)d; c.lo = (float)(d - (double)c.hi);
  return c;
}

// The terms of channel ch as the loops over a share use them.  tab (nullable): the row of the group's LDS table, first
// channel ch0, which the thread that filled it formed once per workgroup -- forward {pb, ga, be, -}; backward
// {hi, lo, ga, be}, the centre included (the backward knows the mean before it loads its share).  Without a table (groups
// of more than OP_CHAN_LDS channels): from memory, the centre per float4.
template <bool BWD>
__device__ __forceinline__ OpChan op_terms(const OpArgs& a, int b, int ch, double mean, const float4* tab, int ch0) {
  if (tab) {
    const float4 t = tab[ch - ch0];
    return BWD ? OpChan{0.0f, t.z, t.w, t.x, t.y} : OpChan{t.x, t.y, t.z, 0.0f, 0.0f};
  }
  const OpChan c = op_chan<BWD>(a, b, ch);
  return BWD ? op_centre(c, mean) : c;
}

// One element's contribution to the partial sums of its share: the one place where it is formed (the register path
// calls these four times per float4, the fallback element by element).
// OpAcc: what the four elements of a float4 are added up in before the sum joins the fp64 partial.  Forward: fp64, as
// in gn_act.hip -- v = x + pre and v^2 never exist rounded to fp32, or E[v^2] - mean^2 would cancel against
// mean^2 2^-24 per square.  Backward: fp32; its two sums do not cancel.
template <bool BWD> struct OpAccT { using type = double; };
template <> struct OpAccT<true> { using type = float; };
template <bool BWD> using OpAcc = typename OpAccT<BWD>::type;

// the backward's element: x, d = dy  ->  xh = the normalised input, dxh = the gradient that reaches it.  Everything the
// activation costs (expf, a correctly rounded division) is in here and runs once per element: the register path keeps
// xh and dxh where x and dy were, and the output needs nothing else of the element.
__device__ __forceinline__ void op_bwd1(const OpArgs& a, const OpChan& c, float x, float d, float rstd, float& xh, float& dxh) {
  xh = ((x + c.hi) + c.lo) * rstd;
  float du = d;
  if (a.act) { const float u = xh * c.ga + c.be, sg = op_sigmoid(u); du = du * (sg * (1.0f + u * (1.0f - sg))); }
  dxh = du * c.ga;
}

// forward: d is unused.  backward: x <- xh, d <- dxh.
template <bool BWD>
__device__ __forceinline__ void op_stat1(const OpArgs& a, const OpChan& c, float& x, float& d, float rstd,
                                         OpAcc<BWD>& t0, OpAcc<BWD>& t1) {
  if constexpr (!BWD) {
    const double v = (double)x + (double)c.pb;
    t0 += v; t1 = fma(v, v, t1);
  } else {
    float xh, dxh;
    op_bwd1(a, c, x, d, rstd, xh, dxh);
    t0 += dxh; t1 += dxh * xh;
    x = xh; d = dxh;
  }
}
// (the backward's output element from xh and dxh; the forward's is nhmc_gn_out of nhmc_common.h, shared with gn_act.hip)
__device__ __forceinline__ float op_apply1(float xh, float dxh, float rstd, float m0, float m1) {
  return rstd * ((dxh - m0) - xh * m1);
}

// one float4 of the share into the partial sums; the backward leaves xh in xv and dxh in dv
template <bool BWD>
__device__ __forceinline__ void op_stat(const OpArgs& a, const OpChan& c, float4& xv, float4& dv, float rstd, double& s0, double& s1) {
  float* xe = reinterpret_cast<float*>(&xv);
  float* de = reinterpret_cast<float*>(&dv);
  OpAcc<BWD> t0 = 0, t1 = 0;
#pragma unroll
  for (int e = 0; e < 4; ++e) op_stat1<BWD>(a, c, xe[e], de[e], rstd, t0, t1);
  s0 += (double)t0; s1 += (double)t1;
}

// One float4 of slab (b, g): where it lives.  q: float4 index inside the slab.
struct OpAt { int ch, p4; };
__device__ __forceinline__ OpAt op_at(const OpArgs& a, int g, int q) {
  const int pl = q / a.hw4;
  return OpAt{g * (a.C / a.G) + pl, q - pl * a.hw4};
}

// The uniform-plane path (template parameter UNI; hw4 % NHMC_BLOCK == 0 and a group that has the LDS table): float4 index
// i of a share starts at a multiple of 256 float4, so its 256 threads are in ONE channel plane.  Plane, channel, the
// side of C1 and the "inside the slab" test are then the workgroup's, not the lane's: one division per workgroup, a
// walk in scalar registers from i to i + 1, a broadcast LDS read of the channel's row, and no per-lane select between
// two sources / destinations.  The values are those of op_at.
struct OpWalk { int pl, r; };                     // plane inside the group, float4 offset of thread 0 inside the plane
__device__ __forceinline__ OpWalk op_walk0(const OpArgs& a, int split) {
  const unsigned q = (unsigned)split * OP_SHARE, pl = q / (unsigned)a.hw4;
  return OpWalk{(int)pl, (int)(q - pl * (unsigned)a.hw4)};
}
__device__ __forceinline__ void op_walk_next(const OpArgs& a, OpWalk& w) {
  w.r += NHMC_BLOCK;
  if (w.r >= a.hw4) { w.r -= a.hw4; ++w.pl; }     // hw4 >= 256: one plane further at the most
}

// where float4 q of the slab is read from (forward: one of the two sources) / written to (backward: one of the two
// destinations); p1 serves the channels below C1, p2 (nullable: p1 is then the whole [n][C][hw] tensor) the rest
template <typename T>
__device__ __forceinline__ T* op_side(const OpArgs& a, T* p1, T* p2, int b, int64_t base, int q, const OpAt& at) {
  if (!p2) return p1 + (base + q);
  return at.ch < a.C1 ? p1 + op_index(b, a.C1, at.ch, a.hw4, at.p4) : p2 + op_index(b, a.C - a.C1, at.ch - a.C1, a.hw4, at.p4);
}

// normalise (forward) / differentiate (backward: xv = xh, dv = dxh) one float4 held in registers and write it
// accv (nullable): acc[base + q] where the kernel has loaded it already
template <bool BWD>
__device__ __forceinline__ void op_apply(const OpArgs& a, int b, int64_t base, int q, const OpAt& at, const float4& xv,
                                         const float4& dv, double mean, float rstd, double rstd64, float m0, float m1,
                                         float4* __restrict__ out1, float4* __restrict__ out2, float4* __restrict__ xcat,
                                         const float4* __restrict__ acc, const float4* tab, const NhmcGnAffine* tab64, int ch0,
                                         const float4* accv = nullptr) {
  const float* xe = reinterpret_cast<const float*>(&xv);
  const float* de = reinterpret_cast<const float*>(&dv);
  float4 o;
  float* oe = reinterpret_cast<float*>(&o);
  if constexpr (!BWD) {
    // the output in fp64 per element, rounded once: the arithmetic of gn_act.hip's forward, the same bits
    const NhmcGnAffine f = tab64 ? tab64[at.ch - ch0] : nhmc_gn_affine(a.gamma, a.beta, a.film, a.film_stride, a.C, b, at.ch);
    const NhmcGnOut k = nhmc_gn_out_terms(f, op_terms<false>(a, b, at.ch, mean, tab, ch0).pb, mean, rstd64);
#pragma unroll
    for (int e = 0; e < 4; ++e) oe[e] = nhmc_gn_out(k, xe[e], a.act);
    out1[base + q] = o;
    if (xcat) xcat[base + q] = xv;
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) oe[e] = op_apply1(xe[e], de[e], rstd, m0, m1);
    if (acc) {
      const float4 av = accv ? *accv : acc[base + q];
      o.x = o.x + av.x; o.y = o.y + av.y; o.z = o.z + av.z; o.w = o.w + av.w;
    }
    *op_side(a, out1, out2, b, base, q, at) = o;
  }
}

// thread 0: the slab's totals -> st64[0..1] = mean, rstd (fp64), st[1] = rstd (forward) / st[2..3] = the two means of the backward
template <bool BWD>
__device__ __forceinline__ void op_totals(const OpArgs& a, double n, double t0, double t1, float* st, double* st64) {
  if (!BWD) {
    const double m = t0 / n;
    st64[0] = m;
    st64[1] = 1.0 / sqrt(fmax(t1 / n - m * m, 0.0) + (double)a.eps);
    st[1] = (float)st64[1];
  } else {
    st[2] = (float)(t0 / n);
    st[3] = (float)(t1 / n);
  }
}

// x: two sources in the forward (x2 nullable), one in the backward.  `ws` is written and read by several workgroups
// of this launch: agent-scope atomics only, no const / __restrict__ on it.
// UNI: the uniform-plane path (OpWalk above); the entry points choose it, the general path serves every shape.
// AHEAD (backward with a second gradient, acc != nullptr): all of the share's `acc` loads are issued ahead of the first
// store instead of pair by pair between the stores.  The last loop is four instructions per element, so nothing hides
// a load's latency inside it; the 32 registers fit (113 / 122 VGPRs, UNI / general).  Without `acc` the instantiation
// that has no such loads keeps the schedule that measured faster for that form.
template <bool BWD, bool UNI, bool AHEAD>
__global__ __launch_bounds__(NHMC_BLOCK) void k_gn_onepass(const float4* __restrict__ x1, const float4* __restrict__ x2,
                                                           const float4* __restrict__ dy, const double* __restrict__ fwd_ws,
                                                           OpArgs a, double* ws, float4* __restrict__ out1,
                                                           float4* __restrict__ out2, float4* __restrict__ xcat,
                                                           const float4* __restrict__ acc) {
  const int bg = blockIdx.y, split = blockIdx.x, tid = threadIdx.x;
  const int b = bg / a.G, g = bg % a.G;
  const int64_t base = (int64_t)bg * a.n4;
  const double n = (double)(a.C / a.G) * (double)a.hw4 * 4.0;
  __shared__ double red[8];
  __shared__ float st[4];
  __shared__ double st64[2];
  __shared__ int arrived;
  __shared__ double part[2 * OP_MAX_SPLITS];        // the partials of a slab, one lane loads one
  __shared__ float4 chan[OP_CHAN_LDS];              // op_terms' rows
  __shared__ NhmcGnAffine chan64[BWD ? 1 : OP_CHAN_LDS];   // forward: the affine terms in fp64, for its output
  const int cpg = a.C / a.G, ch0 = g * cpg;
  const float4* tab = UNI || cpg <= OP_CHAN_LDS ? chan : nullptr;
  const NhmcGnAffine* tab64 = !BWD && tab ? chan64 : nullptr;
  OpChan crow{};                                   // thread tid < cpg: its row of the table, loaded ahead of the waits below
  if (tab && tid < cpg) {
    crow = op_chan<true>(a, b, ch0 + tid);
    if (!BWD) { chan[tid] = make_float4(crow.pb, crow.ga, crow.be, 0.0f); chan64[tid] = nhmc_gn_affine(a.gamma, a.beta, a.film, a.film_stride, a.C, b, ch0 + tid); }
  }
  double mean = 0.0;
  float rstd = 0.f;
  if (BWD) {
    // the forward's partials: one lane each (a serial chain of dependent loads costs more than the share itself), then
    // thread 0 adds them in the order k = 0 .. fwd_splits - 1
    if (tid < a.fwd_splits) { part[2 * tid] = fwd_ws[((int64_t)bg * a.fwd_splits + tid) * 2]; part[2 * tid + 1] = fwd_ws[((int64_t)bg * a.fwd_splits + tid) * 2 + 1]; }
    __syncthreads();
    if (tid == 0) {
      double s = 0.0, ss = 0.0;
#pragma unroll 2
      for (int k = 0; k < a.fwd_splits; ++k) { s += part[2 * k]; ss += part[2 * k + 1]; }
      op_totals<false>(a, n, s, ss, st, st64);
    }
    __syncthreads();
    mean = st64[0]; rstd = st[1];
    if (tab && tid < cpg) {                        // the centre once per channel
      crow = op_centre(crow, mean);
      chan[tid] = make_float4(crow.hi, crow.lo, crow.ga, crow.be);
    }
  }
  const int q0 = split * OP_SHARE;
  const OpWalk w0 = UNI ? op_walk0(a, split) : OpWalk{0, 0};

  // ---- the share of this workgroup, once, into registers
  float4 xv[OP_K], dv[OP_K];
  OpWalk w = w0;
#pragma unroll
  for (int i = 0; i < OP_K; ++i) {
    const int q = q0 + i * NHMC_BLOCK + tid;
    xv[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    dv[i] = xv[i];
    if (UNI ? q0 + i * NHMC_BLOCK < a.n4 : q < a.n4) {
      xv[i] = *op_side(a, x1, BWD ? nullptr : x2, b, base, q, UNI ? OpAt{ch0 + w.pl, w.r + tid} : op_at(a, g, q));
      if (BWD) dv[i] = dy[base + q];
    }
    if (UNI) op_walk_next(a, w);
  }
  __syncthreads();                                 // `chan` is complete
  double v[2] = {0.0, 0.0};
  w = w0;
#pragma unroll
  for (int i = 0; i < OP_K; ++i) {
    if (i % 2 == 0) __builtin_amdgcn_sched_barrier(0);      // as in the last loop of this kernel
    const int q = q0 + i * NHMC_BLOCK + tid;
    if (UNI ? q0 + i * NHMC_BLOCK < a.n4 : q < a.n4)
      op_stat<BWD>(a, op_terms<BWD>(a, b, UNI ? ch0 + w.pl : op_at(a, g, q).ch, mean, tab, ch0), xv[i], dv[i], rstd, v[0], v[1]);
    if (UNI) op_walk_next(a, w);
  }
  op_block_sum(v, red);                       // thread 0 holds the partial of this share

  // ---- the sums of the whole slab
  double* slab_ws = ws + (int64_t)bg * a.splits * 2;
  double t0 = 0.0, t1 = 0.0;                       // thread 0: totals in the order k = 0 .. splits - 1
  if (a.splits == 1) {
    if (tid == 0) { slab_ws[0] = v[0]; slab_ws[1] = v[1]; t0 = v[0]; t1 = v[1]; }
  } else {
    if (tid < NHMC_WAVE) {                         // wave 0: lane 0 publishes, then one lane per partial of the slab
      if (tid == 0) {
        __hip_atomic_store(slab_ws + split * 2, v[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(slab_ws + split * 2 + 1, v[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      // the data is the flag: a word is there when it no longer holds the pattern the launch's memset left
      unsigned long long* slot = reinterpret_cast<unsigned long long*>(slab_ws) + 2 * (tid < a.splits ? tid : 0);
      unsigned long long w0 = OP_EMPTY, w1 = OP_EMPTY;
      int ok = 0;
      for (unsigned spin = 0; spin < a.polls; ++spin) {
        w0 = __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        w1 = __hip_atomic_load(slot + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        ok = __all(w0 != OP_EMPTY && w1 != OP_EMPTY);
        if (ok) break;
        __builtin_amdgcn_s_sleep(8);
      }
      if (ok && tid < a.splits) { part[2 * tid] = __longlong_as_double((long long)w0); part[2 * tid + 1] = __longlong_as_double((long long)w1); }
      if (tid == 0) arrived = ok;
    }
    __syncthreads();
    if (tid == 0 && arrived) {
#pragma unroll 2                                   // (an 8-fold unrolled LDS read here would set the register count)
      for (int k = 0; k < a.splits; ++k) { t0 += part[2 * k]; t1 += part[2 * k + 1]; }
    }
    if (__builtin_expect(!__builtin_amdgcn_readfirstlane(arrived), 0)) {   // a scalar: a uniform branch to the compiler too
      // Bounded wait expired: the other shares of the slab from memory, as their owners reduce them.  Element by element
      // in rolled loops: the share in registers stays live across this branch, which is rarely taken and must not set
      // the kernel's register count; the arithmetic per element and its order are those of the register path.
      for (int k = 0; k < a.splits; ++k) {
        double p[2] = {0.0, 0.0};
        if (k != split) {
#pragma unroll 1
          for (int i = 0; i < OP_K; ++i) {
            const int q = k * OP_SHARE + i * NHMC_BLOCK + tid;
            if (q >= a.n4) continue;
            const OpAt at = op_at(a, g, q);
            const OpChan c = op_terms<BWD>(a, b, at.ch, mean, tab, ch0);
            const float* xs = reinterpret_cast<const float*>(op_side(a, x1, BWD ? nullptr : x2, b, base, q, at));
            const float* ds = reinterpret_cast<const float*>(dy + (base + q));
            OpAcc<BWD> u0 = 0, u1 = 0;
#pragma unroll 1
            for (int e = 0; e < 4; ++e) { float xe = xs[e], de = BWD ? ds[e] : 0.0f; op_stat1<BWD>(a, c, xe, de, rstd, u0, u1); }
            p[0] += (double)u0; p[1] += (double)u1;
          }
          op_block_sum(p, red);
        }
        if (tid == 0) { t0 += k == split ? v[0] : p[0]; t1 += k == split ? v[1] : p[1]; }
        __syncthreads();                           // `red` is free again
      }
    }
  }
  if (tid == 0) op_totals<BWD>(a, n, t0, t1, st, st64);
  if (!BWD && tid == 0 && split == 0) {            // the slab totals behind the partials: a one-split workspace
    double* tot = ws + ((int64_t)gridDim.y * a.splits + bg) * 2;
    tot[0] = t0; tot[1] = t1;
  }
  __syncthreads();
  mean = st64[0]; rstd = st[1];
  const double rstd64 = st64[1];
  const float m0 = st[2], m1 = st[3];

  // ---- normalise / differentiate the share from registers
  float4 av[OP_K];
  if (AHEAD && acc) {
#pragma unroll
    for (int i = 0; i < OP_K; ++i) {
      const int q = q0 + i * NHMC_BLOCK + tid;
      av[i] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (UNI ? q0 + i * NHMC_BLOCK < a.n4 : q < a.n4) av[i] = acc[base + q];
    }
  }
  w = w0;
#pragma unroll
  for (int i = 0; i < OP_K; ++i) {
    // the share fills 32 / 64 VGPRs: keep the scheduler from hoisting all eight `acc` loads on top of them, and (general
    // path) from carrying the plane index and channel terms of all eight float4 over from the statistics: q is opaque
    // here, they are formed again
    if (i % 2 == 0) __builtin_amdgcn_sched_barrier(0);
    int q = q0 + i * NHMC_BLOCK + tid;
    if constexpr (UNI) {
      if (q0 + i * NHMC_BLOCK < a.n4)
        op_apply<BWD>(a, b, base, q, OpAt{ch0 + w.pl, w.r + tid}, xv[i], dv[i], mean, rstd, rstd64, m0, m1, out1, out2, xcat, acc, tab, tab64, ch0, AHEAD ? &av[i] : nullptr);
      op_walk_next(a, w);
    } else {
      asm volatile("" : "+v"(q));
      // (the backward needs the plane only where the gradient goes to two tensors)
      if (q < a.n4) op_apply<BWD>(a, b, base, q, !BWD || out2 ? op_at(a, g, q) : OpAt{0, 0}, xv[i], dv[i], mean, rstd, rstd64, m0, m1, out1, out2, xcat, acc, tab, tab64, ch0, AHEAD ? &av[i] : nullptr);
    }
  }
}

int op_splits(int n, int C, int G, int64_t hw) {
  if (n <= 0 || C <= 0 || G <= 0 || hw <= 0 || C % G || hw % 4 || (int64_t)n * G > 65535) return 0;
  const int64_t n4 = (int64_t)(C / G) * hw / 4, s = (n4 + OP_SHARE - 1) / OP_SHARE;
  return s > OP_MAX_SPLITS ? 0 : (int)s;
}

int op_check(const void* x, const void* gamma, const void* beta, const void* ws, int n, int C, int G, int64_t hw, int flags,
             int* splits) {
  if (!x || !gamma || !beta || !ws || n <= 0 || C <= 0 || G <= 0 || hw <= 0 || (flags & ~NHMC_GN_ONEPASS_NOWAIT)) return NHMC_ERR_ARG;
  if (!(*splits = op_splits(n, C, G, hw))) return NHMC_ERR_SHAPE;
  if (!nhmc_aligned16(x) || !nhmc_aligned16(ws)) return NHMC_ERR_ALIGN;
  return NHMC_OK;
}

// The uniform-plane path serves a shape whose planes are whole multiples of a workgroup's 256 float4 and whose groups have
// the LDS table.  NHMC_GN_UNIFORM=0, read per call, keeps the general path everywhere (the A/B switch of tools/gn_bench.py).
bool op_uniform(int C, int G, int64_t hw) {
  const char* v = std::getenv("NHMC_GN_UNIFORM");
  return !(v && v[0] == '0') && (hw / 4) % NHMC_BLOCK == 0 && C / G <= OP_CHAN_LDS;
}

// every word of the workspace <- the "not yet published" pattern, by a launch of its own ahead of the one-pass kernel on
// the same stream (a kernel node under capture, ordered like every other launch of the stream).  A kernel and not
// hipMemsetAsync as a workaround: observed on ROCm 7.2, with the memset captured into a graph the second replay of
// tests/test_gn_onepass_gpu.py::test_graph_capture_replays_the_eager_bits read leftovers of the first replay as
// published partials; with this kernel it does not.  The cause inside the runtime was not looked for.
__global__ __launch_bounds__(NHMC_BLOCK) void k_gn_ws_fill(unsigned long long* ws, int64_t words) {
  const int64_t i = (int64_t)blockIdx.x * NHMC_BLOCK + threadIdx.x;
  if (i < words) ws[i] = OP_EMPTY;
}
int op_fill_ws(double* ws, int n, int G, int splits, hipStream_t st) {
  const int64_t words = (int64_t)n * G * splits * 2;
  NHMC_LAUNCH(k_gn_ws_fill, dim3((unsigned)((words + NHMC_BLOCK - 1) / NHMC_BLOCK)), dim3(NHMC_BLOCK), 0, st,
              reinterpret_cast<unsigned long long*>(ws), words);
  return nhmc_launch_status();
}

}  // namespace

extern "C" int nhmc_gn_onepass_splits(int n, int channels, int groups, int64_t hw) { return op_splits(n, channels, groups, hw); }

// Routing rule, from tools/gn_bench.py at 64 chains on MI355X (one-pass time / two-pass time, same run, nine FFHQ U-Net
// shapes; profiles/r17_gn_onepass_roofline.txt, median and min-over-rounds ratio, two runs, spread of a ratio between
// the runs <= 0.02).  Forward: 0.72 - 0.90 from 2 splits up, 0.97 - 0.98 at 1 split -> one-pass wherever it is covered.
// Backward: 0.64 - 0.69 at 4 to 32 splits per slab, 0.75 at 64 splits (256 channels at 256x256, the longest wait for the
// slowest share), 0.78 at 2 splits and 0.80 - 0.81 at 1 split; with a second gradient added 0.66 - 0.78 likewise.
// By the convention of round 4 (a class moves where median and min ratio are both below 1 by more than the spread)
// every class would now take the one-pass backward.  The classes at 1, 2 and 64 splits stay on the two-pass kernels all
// the same: the two kinds of kernel split a slab differently, so moving a class changes the last bits of every
// gradient that passes through it, and those classes are 3.9 ms of a 64-chain step (profiles/README.md, round 4), of
// which the move would save about a fifth.  -> one-pass from 4 to 32 splits, two-pass otherwise, unless the caller
// needs what only the one-pass backward offers (the gradient split into two contiguous tensors).
extern "C" int nhmc_gn_onepass_prefers(int backward, int n, int channels, int groups, int64_t hw) {
  const int s = op_splits(n, channels, groups, hw);
  return backward ? (s >= 4 && s <= 32) : s > 0;
}

extern "C" int nhmc_gn_onepass_fwd(const float* x1, const float* x2, int c1, const float* gamma, const float* beta,
                                   const float* film, int64_t film_stride, const float* pre, int64_t pre_stride, float eps,
                                   int act, float* y, float* x_cat, double* ws, int flags, int n,
                                   int channels, int groups, int64_t hw, nhmc_stream_t stream) {
  int splits = 0;
  int rc = op_check(x1, gamma, beta, ws, n, channels, groups, hw, flags, &splits);
  if (rc) return rc;
  if (!y || (x2 && !x_cat) || (!x2 && x_cat)) return NHMC_ERR_ARG;
  if (x2 ? (c1 <= 0 || c1 >= channels) : c1 != channels) return NHMC_ERR_SHAPE;
  if (!nhmc_aligned16(y) || !nhmc_aligned16(x2) || !nhmc_aligned16(x_cat)) return NHMC_ERR_ALIGN;
  if (y == x1 || y == x2 || y == x_cat || x_cat == x1 || (x2 && x_cat == x2)) return NHMC_ERR_ARG;
  const OpArgs a{gamma, beta, film, film_stride, pre, pre_stride, channels, groups, c1, (int)(hw / 4),
                 (int)((int64_t)(channels / groups) * hw / 4), eps, act, splits, splits,
                 (flags & NHMC_GN_ONEPASS_NOWAIT) ? 0u : OP_POLLS};
  hipStream_t st = nhmc_s(stream);
  if (splits > 1 && (rc = op_fill_ws(ws, n, groups, splits, st))) return rc;
  const auto kern = op_uniform(channels, groups, hw) ? k_gn_onepass<false, true, false> : k_gn_onepass<false, false, false>;
  NHMC_LAUNCH(kern, dim3((unsigned)splits, (unsigned)(n * groups)), dim3(NHMC_BLOCK), 0, st, (const float4*)x1,
              (const float4*)x2, (const float4*)nullptr, (const double*)nullptr, a, ws, (float4*)y,
              (float4*)nullptr, (float4*)x_cat, (const float4*)nullptr);
  return nhmc_launch_status();
}

extern "C" int nhmc_gn_onepass_bwd(const float* x, const float* dy, const float* gamma, const float* beta, const float* film,
                                   int64_t film_stride, const float* pre, int64_t pre_stride, float eps, int act,
                                   const double* fwd_ws, int fwd_splits, const float* dx_add, float* dx1, float* dx2, int c1,
                                   double* ws, int flags, int n, int channels, int groups, int64_t hw, nhmc_stream_t stream) {
  int splits = 0;
  int rc = op_check(x, gamma, beta, ws, n, channels, groups, hw, flags, &splits);
  if (rc) return rc;
  if (!dy || !fwd_ws || !dx1 || fwd_splits <= 0 || fwd_splits > OP_MAX_SPLITS || fwd_ws == ws) return NHMC_ERR_ARG;
  if (dx_add == dx1 || (dx2 && (dx_add == dx2 || dx1 == dx2))) return NHMC_ERR_ARG;
  // not in place: a workgroup whose wait expired reads the other shares of x and dy again
  if (dx1 == x || dx1 == dy || (dx2 && (dx2 == x || dx2 == dy))) return NHMC_ERR_ARG;
  if (dx2 ? (c1 <= 0 || c1 >= channels) : c1 != channels) return NHMC_ERR_SHAPE;
  if (!nhmc_aligned16(dy) || !nhmc_aligned16(dx1) || !nhmc_aligned16(dx2) || !nhmc_aligned16(dx_add)) return NHMC_ERR_ALIGN;
  const OpArgs a{gamma, beta, film, film_stride, pre, pre_stride, channels, groups, c1, (int)(hw / 4),
                 (int)((int64_t)(channels / groups) * hw / 4), eps, act, splits, fwd_splits,
                 (flags & NHMC_GN_ONEPASS_NOWAIT) ? 0u : OP_POLLS};
  hipStream_t st = nhmc_s(stream);
  if (splits > 1 && (rc = op_fill_ws(ws, n, groups, splits, st))) return rc;
  const bool uni = op_uniform(channels, groups, hw);
  const auto kern = dx_add ? (uni ? k_gn_onepass<true, true, true> : k_gn_onepass<true, false, true>)
                           : (uni ? k_gn_onepass<true, true, false> : k_gn_onepass<true, false, false>);
  NHMC_LAUNCH(kern, dim3((unsigned)splits, (unsigned)(n * groups)), dim3(NHMC_BLOCK), 0, st, (const float4*)x,
              (const float4*)nullptr, (const float4*)dy, fwd_ws, a, ws, (float4*)dx1, (float4*)dx2,
              (float4*)nullptr, (const float4*)dx_add);
  return nhmc_launch_status();
}
