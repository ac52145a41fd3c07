// Modulated Fourier operators (include/nhmc.h): multi-coil MRI (--deg mcmri<R>) and coded diffraction (--deg cdp<K>).
//     y_k = post(F (S_k o x) F^T),  k = 0 .. K-1,  S_k = Sre_k + i Sim_k known complex maps, F the centred orthonormal DFT,
// post a weighting (linear) or a weighted modulus.  The spectral chain of csrc/spectral_gemm.hip serves real planes, so a
// complex plane S_k o x goes through it as its two real planes A = Sre_k o x and B = Sim_k o x:
//     Y = Y_A + i Y_B   ->   Re Y = Re Y_A - Im Y_B,   Im Y = Im Y_A + Re Y_B,
// and the adjoint of a complex q as the two real adjoints U = adj(q_re, q_im) = Re[F^H q conj(F)] and
// V = adj(q_im, -q_re) = Im[F^H q conj(F)], the gradient being sum_k (Sre_k o U_k + Sim_k o V_k) = Re[conj(S_k) (U_k + i V_k)].
// Three streaming kernels around the exported chain entries (nhmc_phase_H mode 1 and nhmc_phase_adjoint at pad 0, on
// n_chains * C * 2K planes; nothing in spectral_gemm.hip changes):
//   k_modulate   x [plane][d][d] -> [plane][K][2][d][d] (A, B), the clip applied on the fly when asked
//   k_combine    the four spectra of a pair [pair][4][d][d] = (Re Y_A, Im Y_A, Re Y_B, Im Y_B) -> H, or in place the two
//                adjoint inputs (q_re, q_im), (q_im, -q_re) with the loss partial; or (H^T) the same from w o v
//   k_demodulate (U_k, V_k) [plane][K][2][d][d] and the maps -> sum over k ascending, then one of three epilogues
// Every thread owns one float4 of one plane (d % 32 == 0, so d^2 % 1024 == 0: no tails), every element has one writer, no
// atomics.  48 d^3 FLOP per (plane, map) in the chain; a complex-input chain would need 32 d^3 (not tried).
#include "nhmc_common.h"

namespace {

constexpr int MF_BLOCK = 256;
constexpr int MF_TILE = MF_BLOCK * 4;                 // elements of a plane per workgroup
constexpr int MF_SLAB_PLANES = 1024;                  // modulated planes (A and B count as two) per pass over the chain

__device__ __forceinline__ nhmc_v4f mf_ld(const float* p) { return *reinterpret_cast<const nhmc_v4f*>(p); }
__device__ __forceinline__ nhmc_v4f mf_ldnt(const float* p) { return __builtin_nontemporal_load(reinterpret_cast<const nhmc_v4f*>(p)); }
__device__ __forceinline__ void mf_st(float* p, const nhmc_v4f& v) { *reinterpret_cast<nhmc_v4f*>(p) = v; }
__device__ __forceinline__ void mf_stnt(float* p, const nhmc_v4f& v) { __builtin_nontemporal_store(v, reinterpret_cast<nhmc_v4f*>(p)); }

// grid: (d^2 / MF_TILE, planes = chains * C).  ab: [plane][K][2][d][d].
template <bool CLIP>
__global__ __launch_bounds__(MF_BLOCK) void k_modulate(const float* __restrict__ x, const float* __restrict__ maps,
                                                       float* __restrict__ ab, int n_maps, int dd) {
  const int64_t plane = blockIdx.y;
  const int off = ((int)blockIdx.x * MF_BLOCK + (int)threadIdx.x) * 4;
  nhmc_v4f v = mf_ldnt(&x[plane * dd + off]);
  if (CLIP) {
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = nhmc_clip1(v[j]);
  }
  float* __restrict__ out = ab + plane * n_maps * 2 * dd + off;
  for (int k = 0; k < n_maps; ++k) {
    const nhmc_v4f sre = mf_ld(&maps[(int64_t)(2 * k) * dd + off]);
    const nhmc_v4f sim = mf_ld(&maps[(int64_t)(2 * k + 1) * dd + off]);
    mf_st(&out[(int64_t)(2 * k) * dd], sre * v);
    mf_st(&out[(int64_t)(2 * k + 1) * dd], sim * v);
  }
}

// What k_combine does with the spectrum of a pair.
enum { MF_H = 0, MF_RESID = 1, MF_HT = 2 };

// grid: (d^2 / MF_TILE, pairs = chains * C * K).  spec: [pair][4][d][d].
//   MF_H    : io = out, [pair][2][d][d] (linear) or [pair][d][d] (modulus)
//   MF_RESID: io = y in the same layouts; spec is overwritten by (q_re, q_im, q_im, -q_re); ws[pair * tiles + tile] = the
//             workgroup's sum of r^2.  y and w are read once per element; y under w = 0 ends in a select.
//   MF_HT   : io = v [pair][2][d][d] (linear only); spec is WRITTEN from q = w o v, nothing of it is read.
template <int MODULUS, int OP>
__global__ __launch_bounds__(MF_BLOCK) void k_combine(float* __restrict__ spec, const float* __restrict__ w,
                                                      const float* __restrict__ io_in, float* __restrict__ io_out,
                                                      double* __restrict__ ws, int dd) {
  const int64_t pair = blockIdx.y;
  const int off = ((int)blockIdx.x * MF_BLOCK + (int)threadIdx.x) * 4;
  float* __restrict__ s = spec + pair * 4 * dd + off;
  const nhmc_v4f wv = mf_ld(&w[off]);
  nhmc_v4f re, im;
  if (OP != MF_HT) {
    const nhmc_v4f ra = mf_ldnt(&s[0]), ia = mf_ldnt(&s[dd]), rb = mf_ldnt(&s[2 * (int64_t)dd]), ib = mf_ldnt(&s[3 * (int64_t)dd]);
    re = ra - ib;
    im = ia + rb;
  }
  if (OP == MF_H) {
    if (MODULUS) {
      nhmc_v4f a;
#pragma unroll
      for (int j = 0; j < 4; ++j) a[j] = sqrtf(re[j] * re[j] + im[j] * im[j]);
      mf_stnt(&io_out[pair * dd + off], wv * a);
    } else {
      mf_stnt(&io_out[pair * 2 * dd + off], wv * re);
      mf_stnt(&io_out[pair * 2 * dd + dd + off], wv * im);
    }
    return;
  }
  nhmc_v4f qre, qim;
  double lsum[1] = {0.0};                                // fp32 squares summed in fp64
  if (OP == MF_HT) {
    qre = wv * mf_ldnt(&io_in[pair * 2 * dd + off]);
    qim = wv * mf_ldnt(&io_in[pair * 2 * dd + dd + off]);
  } else if (MODULUS) {
    const nhmc_v4f yv = mf_ldnt(&io_in[pair * dd + off]);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float a = sqrtf(re[j] * re[j] + im[j] * im[j]);
      const float r = wv[j] > 0.0f ? yv[j] - wv[j] * a : 0.0f;            // selected, not multiplied: a NaN or inf in an
      lsum[0] += (double)(r * r);                                         // unmeasured entry of y ends here
      const float wr = wv[j] * r;
      qre[j] = a == 0.0f ? 0.0f : wr * (re[j] / a);       // d|Y| = Y / |Y|, sgn(0) = 0; a NaN |Y| stays NaN, as torch.sgn's
      qim[j] = a == 0.0f ? 0.0f : wr * (im[j] / a);
    }
  } else {
    const nhmc_v4f yre = mf_ldnt(&io_in[pair * 2 * dd + off]);
    const nhmc_v4f yim = mf_ldnt(&io_in[pair * 2 * dd + dd + off]);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const bool measured = wv[j] > 0.0f;
      const float rp = measured ? yre[j] - wv[j] * re[j] : 0.0f;
      const float rq = measured ? yim[j] - wv[j] * im[j] : 0.0f;
      lsum[0] += (double)(rp * rp);
      lsum[0] += (double)(rq * rq);
      qre[j] = measured ? wv[j] * rp : 0.0f;
      qim[j] = measured ? wv[j] * rq : 0.0f;
    }
  }
  mf_st(&s[0], qre);                                      // U = adj(q_re, q_im)
  mf_st(&s[dd], qim);
  mf_st(&s[2 * (int64_t)dd], qim);                        // V = adj(q_im, -q_re)
  mf_st(&s[3 * (int64_t)dd], -qre);
  if (OP == MF_RESID) {
    __shared__ double red[4];
    nhmc_block_sum<1>(lsum, red);
    if (threadIdx.x == 0) ws[pair * gridDim.x + blockIdx.x] = lsum[0];   // the tiles of a chain are contiguous
  }
}

// The one accumulation H^T, the data term and the fused form share: sum over k ascending from 0.0f of
// Sre_k o U_k + Sim_k o V_k, every product and sum rounded on its own (-ffp-contract=off).  uv: [plane][K][2][d][d].
__device__ __forceinline__ nhmc_v4f mf_demodulate(const float* __restrict__ uv, const float* __restrict__ maps, int64_t plane,
                                                  int off, int n_maps, int dd) {
  const float* __restrict__ in = uv + plane * n_maps * 2 * dd + off;
  nhmc_v4f acc = {0.0f, 0.0f, 0.0f, 0.0f};
  for (int k = 0; k < n_maps; ++k) {
    const nhmc_v4f u = mf_ldnt(&in[(int64_t)(2 * k) * dd]);
    const nhmc_v4f v = mf_ldnt(&in[(int64_t)(2 * k + 1) * dd]);
    const nhmc_v4f sre = mf_ld(&maps[(int64_t)(2 * k) * dd + off]);
    const nhmc_v4f sim = mf_ld(&maps[(int64_t)(2 * k + 1) * dd + off]);
    acc = acc + (sre * u + sim * v);
  }
  return acc;
}

enum { MF_PLAIN = 0, MF_GRAD = 1, MF_VJP = 2 };
struct MfVjp { const float* e; float* g_e; const float* at; const float* at_next; int e_channels; int channels; };

// grid: (d^2 / MF_TILE, planes = chains * C).
//   MF_PLAIN: out = the sum (H^T)
//   MF_GRAD : out = -2 sum, selected by the clip mask of xt where xt is given
//   MF_VJP  : -2 sum through the VJP of the last DDIM step (inputs xt, e): out = g_xt, and channels [0, C) of g_e
template <int EPI>
__global__ __launch_bounds__(MF_BLOCK) void k_demodulate(const float* __restrict__ uv, const float* __restrict__ maps,
                                                         float* __restrict__ out, const float* __restrict__ xt, MfVjp vj,
                                                         int n_maps, int dd) {
  const int64_t plane = blockIdx.y;
  const int off = ((int)blockIdx.x * MF_BLOCK + (int)threadIdx.x) * 4;
  nhmc_v4f g = mf_demodulate(uv, maps, plane, off, n_maps, dd);
  if (EPI == MF_GRAD) {
    g = -(2.0f * g);
    if (xt) {
      const nhmc_v4f xv = mf_ldnt(&xt[plane * dd + off]);
#pragma unroll
      for (int j = 0; j < 4; ++j) g[j] = nhmc_masked(g[j], nhmc_in1(xv[j]));
    }
  }
  if (EPI == MF_VJP) {
    const int64_t chain = plane / vj.channels, c = plane % vj.channels;
    const int64_t eoff = (chain * vj.e_channels + c) * dd + off;
    const NhmcMix kc = nhmc_mix_coef(vj.at, vj.at_next, chain);
    const nhmc_v4f xv = mf_ldnt(&xt[plane * dd + off]);
    const nhmc_v4f ev = mf_ldnt(&vj.e[eoff]);
    nhmc_v4f ge;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float gx, gee;
      nhmc_mix_vjp(kc, -(2.0f * g[j]), xv[j], ev[j], gx, gee);
      ge[j] = gee; g[j] = gx;
    }
    mf_stnt(&vj.g_e[eoff], ge);
  }
  mf_stnt(&out[plane * dd + off], g);
}

bool mf_bad(int n_chains, int channels, int n_maps, int dim) {
  return n_chains <= 0 || channels <= 0 || dim <= 0 || (dim % 32) || dim > 8192 || n_maps < 1 || n_maps > 32 ||
         (int64_t)n_chains * channels * 2 * n_maps > 65535;
}

bool mf_aligned(const void* a, const void* b, const void* c, const void* d, const void* e, const void* f = nullptr,
                const void* g = nullptr, const void* h = nullptr, const void* i = nullptr, const void* j = nullptr) {
  return nhmc_aligned16(a) && nhmc_aligned16(b) && nhmc_aligned16(c) && nhmc_aligned16(d) && nhmc_aligned16(e) &&
         nhmc_aligned16(f) && nhmc_aligned16(g) && nhmc_aligned16(h) && nhmc_aligned16(i) && nhmc_aligned16(j);
}

// Chains per pass: as many as fit MF_SLAB_PLANES modulated planes, one at least.
int mf_slab_chains(int n_chains, int channels, int n_maps) {
  const int per_chain = channels * 2 * n_maps;
  const int fit = MF_SLAB_PLANES / per_chain;
  return fit < 1 ? 1 : (fit < n_chains ? fit : n_chains);
}

// The scratch of one pass over `nb` chains: the planes A, B (later U, V), the chain's own scratch, the spectra.
struct MfTmp { float *ab, *chain, *spec; };
MfTmp mf_tmp(float* tmp, int nb, int channels, int n_maps, int dim) {
  const size_t planes = (size_t)nb * channels * 2 * n_maps, dd = (size_t)dim * dim;
  float* chain = tmp + planes * dd;
  return MfTmp{tmp, chain, chain + nhmc_phase_tmp_floats(nb, channels * 2 * n_maps, dim, 0)};
}

struct MfDims { int channels, n_maps, dim, dd; unsigned tiles; };
MfDims mf_dims(int channels, int n_maps, int dim) {
  return MfDims{channels, n_maps, dim, dim * dim, (unsigned)(dim * dim / MF_TILE)};
}

// x -> the spectra of the pairs of `nb` chains, in t.spec
int mf_forward(const float* x, bool clip, const float* maps, const float* fac, const MfTmp& t, int nb, const MfDims& m,
               nhmc_stream_t stream) {
  const dim3 grid(m.tiles, (unsigned)(nb * m.channels));
  if (clip) NHMC_LAUNCH((k_modulate<true>), grid, dim3(MF_BLOCK), 0, nhmc_s(stream), x, maps, t.ab, m.n_maps, m.dd);
  else      NHMC_LAUNCH((k_modulate<false>), grid, dim3(MF_BLOCK), 0, nhmc_s(stream), x, maps, t.ab, m.n_maps, m.dd);
  const int rc = nhmc_launch_status();
  if (rc) return rc;
  return nhmc_phase_H(t.ab, fac, 1, t.spec, t.chain, nb, m.channels * 2 * m.n_maps, m.dim, 0, stream);
}

template <int MODULUS, int OP>
int mf_combine(const MfTmp& t, const float* w, const float* io_in, float* io_out, double* ws, int nb, const MfDims& m,
               nhmc_stream_t stream) {
  const dim3 grid(m.tiles, (unsigned)(nb * m.channels * m.n_maps));
  NHMC_LAUNCH((k_combine<MODULUS, OP>), grid, dim3(MF_BLOCK), 0, nhmc_s(stream), t.spec, w, io_in, io_out, ws, m.dd);
  return nhmc_launch_status();
}

// the adjoint inputs in t.spec -> (U_k, V_k) in t.ab -> the epilogue EPI
template <int EPI>
int mf_backward(const MfTmp& t, const float* maps, const float* fac, float* out, const float* xt, const MfVjp& vj, int nb,
                const MfDims& m, nhmc_stream_t stream) {
  const int rc = nhmc_phase_adjoint(t.spec, fac, t.ab, t.chain, nb, m.channels * 2 * m.n_maps, m.dim, 0, stream);
  if (rc) return rc;
  const dim3 grid(m.tiles, (unsigned)(nb * m.channels));
  NHMC_LAUNCH((k_demodulate<EPI>), grid, dim3(MF_BLOCK), 0, nhmc_s(stream), t.ab, maps, out, xt, vj, m.n_maps, m.dd);
  return nhmc_launch_status();
}

// Loss partials and the adjoint inputs of `nb` chains from xt (clipped on the fly when asked).
int mf_residual(const float* xt, bool clip, const float* y, const float* maps, const float* fac, const float* w, int modulus,
                double* ws, const MfTmp& t, int nb, const MfDims& m, nhmc_stream_t stream) {
  const int rc = mf_forward(xt, clip, maps, fac, t, nb, m, stream);
  if (rc) return rc;
  return modulus ? mf_combine<1, MF_RESID>(t, w, y, nullptr, ws, nb, m, stream)
                 : mf_combine<0, MF_RESID>(t, w, y, nullptr, ws, nb, m, stream);
}

}  // namespace

// Loss partials per chain: one per workgroup of k_combine.
extern "C" int nhmc_modfourier_tiles(int channels, int n_maps, int dim) {
  return channels * n_maps * (dim * dim / MF_TILE);
}

extern "C" size_t nhmc_modfourier_tmp_floats(int n_chains, int channels, int n_maps, int dim) {
  if (mf_bad(n_chains, channels, n_maps, dim)) return 0;
  const int nb = mf_slab_chains(n_chains, channels, n_maps);
  const size_t planes = (size_t)nb * channels * 2 * n_maps, dd = (size_t)dim * dim;
  return planes * dd + nhmc_phase_tmp_floats(nb, channels * 2 * n_maps, dim, 0) + planes * 2 * dd;    // 1 + 4 + 2 = 7 d^2 per plane
}

extern "C" int nhmc_modfourier_H(const float* x, const float* maps, const float* fac, const float* w, int modulus, float* out,
                                 float* tmp, int n_chains, int channels, int n_maps, int dim, nhmc_stream_t stream) {
  if (!x || !maps || !fac || !w || !out || !tmp || (modulus != 0 && modulus != 1)) return NHMC_ERR_ARG;
  if (mf_bad(n_chains, channels, n_maps, dim)) return NHMC_ERR_SHAPE;
  if (!mf_aligned(x, maps, fac, w, out, tmp)) return NHMC_ERR_ALIGN;
  const MfDims m = mf_dims(channels, n_maps, dim);
  const int slab = mf_slab_chains(n_chains, channels, n_maps);
  const int64_t in_chain = (int64_t)channels * m.dd, out_chain = in_chain * n_maps * (modulus ? 1 : 2);
  for (int c0 = 0; c0 < n_chains; c0 += slab) {
    const int nb = n_chains - c0 < slab ? n_chains - c0 : slab;
    const MfTmp t = mf_tmp(tmp, nb, channels, n_maps, dim);
    int rc;
    if ((rc = mf_forward(x + c0 * in_chain, false, maps, fac, t, nb, m, stream))) return rc;
    float* o = out + c0 * out_chain;
    if ((rc = modulus ? mf_combine<1, MF_H>(t, w, nullptr, o, nullptr, nb, m, stream)
                      : mf_combine<0, MF_H>(t, w, nullptr, o, nullptr, nb, m, stream))) return rc;
  }
  return NHMC_OK;
}

extern "C" int nhmc_modfourier_Ht(const float* v, const float* maps, const float* fac, const float* w, float* out, float* tmp,
                                  int n_chains, int channels, int n_maps, int dim, nhmc_stream_t stream) {
  if (!v || !maps || !fac || !w || !out || !tmp) return NHMC_ERR_ARG;
  if (mf_bad(n_chains, channels, n_maps, dim)) return NHMC_ERR_SHAPE;
  if (!mf_aligned(v, maps, fac, w, out, tmp)) return NHMC_ERR_ALIGN;
  const MfDims m = mf_dims(channels, n_maps, dim);
  const int slab = mf_slab_chains(n_chains, channels, n_maps);
  const int64_t out_chain = (int64_t)channels * m.dd, in_chain = out_chain * n_maps * 2;
  for (int c0 = 0; c0 < n_chains; c0 += slab) {
    const int nb = n_chains - c0 < slab ? n_chains - c0 : slab;
    const MfTmp t = mf_tmp(tmp, nb, channels, n_maps, dim);
    int rc;
    if ((rc = mf_combine<0, MF_HT>(t, w, v + c0 * in_chain, nullptr, nullptr, nb, m, stream))) return rc;
    if ((rc = mf_backward<MF_PLAIN>(t, maps, fac, out + c0 * out_chain, nullptr, MfVjp{}, nb, m, stream))) return rc;
  }
  return NHMC_OK;
}

extern "C" int nhmc_data_modfourier(const float* xt, const float* y, const float* maps, const float* fac, const float* w,
                                    int modulus, int apply_clip, float* g_xt, double* loss_ws, float* tmp, int n_chains,
                                    int channels, int n_maps, int dim, nhmc_stream_t stream) {
  if (!xt || !y || !maps || !fac || !w || !g_xt || !loss_ws || !tmp || (modulus != 0 && modulus != 1)) return NHMC_ERR_ARG;
  if (mf_bad(n_chains, channels, n_maps, dim)) return NHMC_ERR_SHAPE;
  if (!mf_aligned(xt, y, maps, fac, w, g_xt, tmp)) return NHMC_ERR_ALIGN;
  const MfDims m = mf_dims(channels, n_maps, dim);
  const int slab = mf_slab_chains(n_chains, channels, n_maps);
  const int64_t x_chain = (int64_t)channels * m.dd, y_chain = x_chain * n_maps * (modulus ? 1 : 2);
  const int64_t ws_chain = nhmc_modfourier_tiles(channels, n_maps, dim);
  for (int c0 = 0; c0 < n_chains; c0 += slab) {
    const int nb = n_chains - c0 < slab ? n_chains - c0 : slab;
    const MfTmp t = mf_tmp(tmp, nb, channels, n_maps, dim);
    const float* x = xt + c0 * x_chain;
    int rc;
    if ((rc = mf_residual(x, apply_clip != 0, y + c0 * y_chain, maps, fac, w, modulus, loss_ws + c0 * ws_chain, t, nb, m, stream)))
      return rc;
    if ((rc = mf_backward<MF_GRAD>(t, maps, fac, g_xt + c0 * x_chain, apply_clip ? x : nullptr, MfVjp{}, nb, m, stream))) return rc;
  }
  return NHMC_OK;
}

extern "C" int nhmc_data_modfourier_vjp(const float* xt_next, const float* y, const float* maps, const float* fac,
                                        const float* w, int modulus, const float* xt, const float* e, int e_channels,
                                        const float* at, const float* at_next, float* g_xt, float* g_e, double* loss_ws,
                                        float* tmp, int n_chains, int channels, int n_maps, int dim, nhmc_stream_t stream) {
  if (!xt_next || !y || !maps || !fac || !w || !xt || !e || !at || !at_next || !g_xt || !g_e || !loss_ws || !tmp ||
      (modulus != 0 && modulus != 1))
    return NHMC_ERR_ARG;
  if (mf_bad(n_chains, channels, n_maps, dim) || (e_channels != channels && e_channels != 2 * channels)) return NHMC_ERR_SHAPE;
  if (!mf_aligned(xt_next, y, maps, fac, w, xt, e, g_xt, g_e, tmp)) return NHMC_ERR_ALIGN;
  const MfDims m = mf_dims(channels, n_maps, dim);
  const int slab = mf_slab_chains(n_chains, channels, n_maps);
  const int64_t x_chain = (int64_t)channels * m.dd, y_chain = x_chain * n_maps * (modulus ? 1 : 2);
  const int64_t e_chain = (int64_t)e_channels * m.dd, ws_chain = nhmc_modfourier_tiles(channels, n_maps, dim);
  for (int c0 = 0; c0 < n_chains; c0 += slab) {
    const int nb = n_chains - c0 < slab ? n_chains - c0 : slab;
    const MfTmp t = mf_tmp(tmp, nb, channels, n_maps, dim);
    int rc;
    if ((rc = mf_residual(xt_next + c0 * x_chain, false, y + c0 * y_chain, maps, fac, w, modulus, loss_ws + c0 * ws_chain, t,
                          nb, m, stream)))
      return rc;
    const MfVjp vj{e + c0 * e_chain, g_e + c0 * e_chain, at + c0, at_next + c0, e_channels, channels};
    if ((rc = mf_backward<MF_VJP>(t, maps, fac, g_xt + c0 * x_chain, xt + c0 * x_chain, vj, nb, m, stream))) return rc;
  }
  return NHMC_OK;
}
