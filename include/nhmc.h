/* nhmc.h -- C ABI of the MI355X-native noise-space HMC hot path (libnhmc.so).
 *
 * Every entry point
 *   - takes raw DEVICE pointers, sizes, per-chain scalar arrays and a hipStream_t
 *     (passed as void*; NULL = the null stream);
 *   - is asynchronous on that stream, allocates nothing, never synchronises;
 *   - returns an int status (NHMC_OK = 0); no C++ exception crosses the boundary;
 *   - may be called concurrently on different streams / devices.
 *
 * "Reference" below is Sunsett5/Noise-space-HMC; file:line are relative to its root.
 * The reference has no FFI: its hot path is Python issuing ATen ops.  Each function
 * names the reference lines whose arithmetic it replaces; INTEGRATION.md shows the
 * ctypes binding a maintainer adds on the reference side.
 *
 * Layout conventions
 *   images   : fp32, [n_chains][C][H][W] contiguous (NCHW), n_elem = C*H*W per chain,
 *              n_elem % 4 == 0 and base pointers 16-byte aligned (NHMC_ERR_ALIGN otherwise)
 *   score    : fp32, [n_chains][e_channels][H][W], e_channels in {C, 2C}; only the first
 *              C channels are read (learned-sigma channels ignored, algos/unconditional.py:17-18)
 *   y        : fp32, [n_chains][M]
 *   per-chain scalars : device arrays of length n_chains (double for the sampler's
 *              Python-float quantities eps / sigma_y, float for alpha-bar)
 *   partial-sum workspaces : double, sized by the matching *_ws_bytes(); reductions are
 *              two-pass and deterministic (no float atomics)
 */
#ifndef NHMC_H
#define NHMC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* nhmc_stream_t; /* hipStream_t */

enum {
  NHMC_OK = 0,
  NHMC_ERR_ARG = 1,    /* null pointer / non-positive size / unknown mode */
  NHMC_ERR_ALIGN = 2,  /* pointer not 16-byte aligned or n_elem % 4 != 0 */
  NHMC_ERR_SHAPE = 3,  /* shape combination the kernel does not cover */
  NHMC_ERR_LAUNCH = 4  /* hipGetLastError() after launch != hipSuccess */
};

#define NHMC_ABI_VERSION 2
int nhmc_abi_version(void);
const char* nhmc_status_string(int status);
/* HIP's message for the last NHMC_ERR_LAUNCH raised on the calling thread (diagnostics only). */
const char* nhmc_last_launch_error(void);

/* ------------------------------------------------------------------------------------
 * a1-a4  Fused leapfrog update            main_sampling.py:702,706-707,713,715
 *
 *   G  = x + (1/(2 sigma_y^2)) * (g [+ g2])
 *   NHMC_LF_FIRST : Sx,Sp partials of (x,p) BEFORE the update (for H at :697);
 *                   p -= (eps/2) G ; x += (eps/m) p
 *   NHMC_LF_MID   : p -= eps G     ; x += (eps/m) p          <- the north-star kernel, 5T/chain
 *   NHMC_LF_LAST  : p -= eps G ; p += (eps/2) G ; x unchanged;
 *                   Sx,Sp partials AFTER the update (for H at :717)
 * fp32 op order and scalar rounding follow the reference (scalars are fp64 products
 * rounded once to fp32).  g2 (nullable) is a second gradient contribution added to g
 * before use (the U-Net input-gradient of the first DDIM step), saving a separate add pass.
 * sums_ws: double[n_chains][nhmc_leapfrog_tiles(n_elem)][2]; written in FIRST/LAST, may be
 * NULL in MID.
 * ---------------------------------------------------------------------------------- */
enum { NHMC_LF_FIRST = 0, NHMC_LF_MID = 1, NHMC_LF_LAST = 2 };
int nhmc_leapfrog_tiles(int64_t n_elem);
size_t nhmc_leapfrog_ws_bytes(int n_chains, int64_t n_elem);
int nhmc_leapfrog_fused(int mode, float* x, float* p, const float* g, const float* g2,
                        const double* eps, const double* sigma_y, double m_inv,
                        int n_chains, int64_t n_elem, double* sums_ws, nhmc_stream_t stream);

/* NHMC_LF_FIRST out of place in x: reads x_in, writes the proposal to x_out (x_in != x_out) and updates p in place.
 * The caller's accepted position survives the trajectory, so a reject needs no saved copy (main_sampling.py:699
 * clones x for that).  Same traffic as the in-place form. */
int nhmc_leapfrog_first(const float* x_in, float* x_out, float* p, const float* g, const float* g2,
                        const double* eps, const double* sigma_y, double m_inv,
                        int n_chains, int64_t n_elem, double* sums_ws, nhmc_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Gradient cache: one decode + gradient per leapfrog step, none for the first half step.
 *
 * The reference evaluates the decode, loss and gradient at the accepted position x at the top of every outer
 * iteration (main_sampling.py:693-695), although that point was already evaluated: by the previous iteration's last
 * leapfrog step if its proposal was accepted (x is that proposal, :709-711,731), by the previous iteration's own
 * :693-695 if it was rejected (x did not move).  Loss and gradient do not depend on sigma_y / eps (those enter inside
 * the update), so the values are identical and reusing them changes no bit while removing 1 of L+1 score-network
 * ladders per trajectory.
 *
 * Layout: g_pair = float[2][pair_stride] (pair_stride >= n_chains_total * n_elem, % 4 == 0), slot s of chain c at
 * g_pair + s*pair_stride + c*n_elem, holding the SUMMED gradient g + g2 (the fp32 add the update kernels perform
 * first anyway); loss_pair = double[2][loss_stride]; sel = int32[n_chains], the slot that belongs to the accepted
 * position.  All pointers are those of the launch's first chain (chunk views just offset them).
 *   nhmc_grad_cache_store        slot (sel ^ flip) <- (g + g2, loss)          (the once-per-run evaluation at x0)
 *   nhmc_leapfrog_first_cached   NHMC_LF_FIRST (out of place) with g read from slot sel
 *   nhmc_leapfrog_last_cached    NHMC_LF_LAST, and slot 1 - sel <- (g + g2, loss) of the end point
 *   nhmc_hamiltonian_cached      nhmc_hamiltonian with loss = loss_pair[sel]
 *   nhmc_grad_cache_flip         sel ^= accept                                 (after the Metropolis test)
 * ---------------------------------------------------------------------------------- */
int nhmc_grad_cache_store(const float* g, const float* g2, const double* loss, float* g_pair, double* loss_pair,
                          const int32_t* sel, int flip, int64_t pair_stride, int64_t loss_stride,
                          int n_chains, int64_t n_elem, nhmc_stream_t stream);
int nhmc_leapfrog_first_cached(const float* x_in, float* x_out, float* p, const float* g_pair, const int32_t* sel,
                               int64_t pair_stride, const double* eps, const double* sigma_y, double m_inv,
                               int n_chains, int64_t n_elem, double* sums_ws, nhmc_stream_t stream);
int nhmc_leapfrog_last_cached(float* x, float* p, const float* g, const float* g2, float* g_pair, const int32_t* sel,
                              int64_t pair_stride, const double* loss, double* loss_pair, int64_t loss_stride,
                              const double* eps, const double* sigma_y, double m_inv,
                              int n_chains, int64_t n_elem, double* sums_ws, nhmc_stream_t stream);
int nhmc_grad_cache_flip(const int32_t* accept, int32_t* sel, int n_chains, nhmc_stream_t stream);

/* ------------------------------------------------------------------------------------
 * a9-a10  DDIM mix, forward               algos/unconditional.py:17-28, main_sampling.py:709
 *   u = (xt - e*sqrt(1-at)) / sqrt(at);  x0 = clip(u,-1,1);  add = sqrt(1-at_next)*e;
 *   xt_next = sqrt(at_next)*x0 + add;    if final_clip: xt_next = clip(xt_next,-1,1)
 * Any of xt_next / x0_t / add_up may be NULL (not written): the fused sampler writes only
 * xt_next (3T), the plugin surface's cal_x0 writes x0_t and add_up.
 * at / at_next: float[n_chains] (the reference's [n,1,1,1] alpha-bar tensors).
 * ---------------------------------------------------------------------------------- */
int nhmc_ddim_mix_fwd(const float* xt, const float* e, int e_channels,
                      const float* at, const float* at_next, int final_clip,
                      float* xt_next, float* x0_t, float* add_up,
                      int n_chains, int channels, int64_t hw, nhmc_stream_t stream);

/* map_back alone: xt_next = sqrt(at_next)*x0_t + add_up      algos/unconditional.py:26-28 */
int nhmc_ddim_map_back(const float* x0_t, const float* add_up, const float* at_next,
                       float* xt_next, int n_chains, int64_t n_elem, nhmc_stream_t stream);

/* ------------------------------------------------------------------------------------
 * a11  DDIM mix, backward (the VJP autograd builds at main_sampling.py:695,711)
 *   gin = gout (+ gout2);  if final_clip: gin *= 1[-1 <= xt_next <= 1]
 *   g_xt = ((gin*sqrt(at_next)) * 1[-1<=u<=1]) / sqrt(at)
 *   g_e[:, :C] = sqrt(1-at_next)*gin + (-g_xt)*sqrt(1-at);   g_e[:, C:] = 0
 * g_e has e_channels channels (what the score network's backward consumes).  fill_sigma = 1 writes the zero
 * sigma-channels; fill_sigma = 0 leaves channels [C, e_channels) untouched (caller keeps a pre-zeroed buffer: -T).
 * g_e may be NULL: the score-path gradient is then not formed (a score evaluated without gradient, as the latent
 * model's apply_model is: ldm/models/diffusion/ddpm.py:892), -T of writes.
 * g_x0 (nullable; then gout2 == NULL and final_clip == 0): split form for the plugin surface,
 * where cal_x0 and map_back are differentiated separately -- gout is then d/d add_up and g_x0
 * replaces gin*sqrt(at_next) as the gradient reaching x0_t.
 * ---------------------------------------------------------------------------------- */
int nhmc_ddim_mix_bwd(const float* gout, const float* gout2, const float* g_x0, const float* xt,
                      const float* e, int e_channels, const float* at, const float* at_next, int final_clip,
                      float* g_xt, float* g_e, int fill_sigma,
                      int n_chains, int channels, int64_t hw, nhmc_stream_t stream);

/* a11 + a12/a13 fused: VJP of the LAST DDIM step (final clip included) with the inpainting data term computed on the
 * fly from (xt, e): r = y[slot] - clip(xt_next), loss partials (nhmc_leapfrog_tiles(n_elem) per chain), gin = -2 r.
 * Replaces nhmc_data_inpaint + nhmc_ddim_mix_bwd(final_clip = 1) for deg = inpaint_* (same bits, -3T of traffic). */
int nhmc_ddim_mix_bwd_inpaint(const float* xt, const float* e, int e_channels, const float* at,
                              const float* at_next, const float* y, const int32_t* slot, int64_t m,
                              float* g_xt, float* g_e, int fill_sigma, double* loss_ws, int n_chains,
                              int channels, int64_t hw, nhmc_stream_t stream);

/* The same for a WHOLE-PIXEL mask (every pixel keeps all its channels or none, as main_sampling.py:290-305 builds them):
 * mask_words[hw/32] has bit (p % 32) of word p / 32 set when pixel p (row-major) is kept, prefix[hw/32] is the number of
 * kept pixels before each word, and y index = channels * rank(p) + channel.  Replaces the T-per-chain slot stream by
 * 16 KB of tables; hw % 32 == 0.  Same bits as nhmc_ddim_mix_bwd_inpaint (g_xt, g_e; the loss to fp64 rounding).
 * loss_ws: nhmc_inpaint_px_tiles(channels, hw) partials per chain (one per tile of a channel plane). */
int nhmc_inpaint_px_tiles(int channels, int64_t hw);
int nhmc_ddim_mix_bwd_inpaint_px(const float* xt, const float* e, int e_channels, const float* at,
                                 const float* at_next, const float* y, const uint32_t* mask_words,
                                 const int32_t* prefix, int64_t m, float* g_xt, float* g_e, int fill_sigma,
                                 double* loss_ws, int n_chains, int channels, int64_t hw, nhmc_stream_t stream);

/* a11 + a12/a14 fused: the same for the super-resolution operator (obs_functions/Hfuncs.py:180-234), ratio in
 * {2,4,8,16}: r = y - blockmean(clip(xt_next)), loss partials (nhmc_sr_vjp_tiles(channels, dim, ratio) per chain),
 * gin = -2 r / ratio^2.  Replaces nhmc_data_sr + nhmc_ddim_mix_bwd(final_clip = 1) (same bits, -3T of traffic).
 * Writes channels [0, channels) of g_e only: the caller keeps the sigma-channels of g_e zero.
 * ratio 4 runs one float4 per thread and stream with the four rows of a block of pixels on the four waves of a
 * workgroup (nhmc_sr_vjp_tiles partials per chain: more, smaller tiles than nhmc_sr_tiles). */
int nhmc_sr_vjp_tiles(int channels, int dim, int ratio);
int nhmc_ddim_mix_bwd_sr(const float* xt, const float* e, int e_channels, const float* at, const float* at_next,
                         const float* y, int ratio, float* g_xt, float* g_e, double* loss_ws, int n_chains,
                         int channels, int dim, nhmc_stream_t stream);

/* ------------------------------------------------------------------------------------
 * a12-a14  Data term: loss_b = sum (y_b - H clip(xt_b))^2 and d loss / d xt
 *                                          main_sampling.py:693-695,709-711
 * All write g_xt = -2 H^T r (masked by 1[-1<=xt<=1] when apply_clip) densely (no memset
 * needed) and per-tile fp64 partials of sum r^2 into loss_ws; finish with
 * nhmc_sum_partials(loss_ws, tiles, n_chains, loss).
 *
 * inpaint (obs_functions/Hfuncs.py:119-154): slot[j], j in CHW order, is the index into y of
 *   pixel-element j, or -1 if that element is masked out.
 * sr (Hfuncs.py:180-234): ratio r in {2,4,8,16,32}, W % 4 == 0, y laid out [C][H/r][W/r].
 * ---------------------------------------------------------------------------------- */
int nhmc_data_tiles(int64_t n_elem);                 /* tiles written by nhmc_data_inpaint / nhmc_psnr */
int nhmc_sr_tiles(int channels, int dim, int ratio); /* tiles written by nhmc_data_sr */
size_t nhmc_data_ws_bytes(int n_chains, int64_t n_elem);
int nhmc_data_inpaint(const float* xt, const float* y, const int32_t* slot, int apply_clip,
                      float* g_xt, double* loss_ws,
                      int n_chains, int64_t n_elem, int64_t m, nhmc_stream_t stream);
int nhmc_data_sr(const float* xt, const float* y, int ratio, int apply_clip,
                 float* g_xt, double* loss_ws,
                 int n_chains, int channels, int dim, nhmc_stream_t stream);
int nhmc_sum_partials(const double* ws, int tiles, int stride, int offset, int n_chains,
                      double* out, nhmc_stream_t stream);

/* Operator surface H / H^T / H^+ (Hfuncs.py:65-90) for the same two operators.
 * inpaint: kept_chw[k] = CHW address of y entry k.  scale: 1/r^2 for H^T, 1 for H^+. */
int nhmc_inpaint_H(const float* x, const int32_t* kept_chw, float* y,
                   int n_chains, int64_t n_elem, int64_t m, nhmc_stream_t stream);
int nhmc_inpaint_Ht(const float* y, const int32_t* slot, float* x,
                    int n_chains, int64_t n_elem, int64_t m, nhmc_stream_t stream);
int nhmc_sr_H(const float* x, float* y, int ratio, int n_chains, int channels, int dim,
              nhmc_stream_t stream);
int nhmc_sr_Ht(const float* y, float* x, int ratio, float scale, int n_chains, int channels,
               int dim, nhmc_stream_t stream);

/* Colorization (Hfuncs.py:655-695).  w: HOST array of channels + 2 floats (channels <= 4; passed by value to the
 * kernel): the SVD (u, s, V) of the 1 x C grey row as the reference holds it -- V[0,0] .. V[C-1,0], s, U[0,0].
 *   H x = u * (s * ((v_0 x_0 + v_1 x_1) + v_2 x_2)),  H^T y = v_c * (s * (u * y)),  H^+ y = v_c * ((u * y) * (1 / s)),
 * each product and sum rounded in this order (torch's CPU ops on the reference's composition: same bits).
 * loss partials: nhmc_color_tiles(hw) per chain. */
int nhmc_color_tiles(int64_t hw);
int nhmc_data_color(const float* xt, const float* y, const float* w, int apply_clip, float* g_xt,
                    double* loss_ws, int n_chains, int channels, int64_t hw, nhmc_stream_t stream);
/* nhmc_data_color fused with the VJP of the LAST DDIM step (as nhmc_ddim_mix_bwd_inpaint / _sr): writes g_xt and
 * channels [0, channels) of g_e. */
int nhmc_ddim_mix_bwd_color(const float* xt, const float* e, int e_channels, const float* at, const float* at_next,
                            const float* y, const float* w, float* g_xt, float* g_e, double* loss_ws, int n_chains,
                            int channels, int64_t hw, nhmc_stream_t stream);
int nhmc_color_H(const float* x, const float* w, float* y, int n_chains, int channels, int64_t hw,
                 nhmc_stream_t stream);
int nhmc_color_Ht(const float* y, const float* w, int pinv, float* x, int n_chains, int channels, int64_t hw,
                  nhmc_stream_t stream);                                    /* pinv: 0 = H^T, 1 = H^+ */

/* Walsh-Hadamard compressive sensing (Hfuncs.py:611-651): y[k*C + c] = (FWHT(x_c) / d)[perm[k]], k < d*d/ratio;
 * H^T = H^+.  kslot: int32[d*d], position -> k or -1 (inverse of perm restricted to the kept rows).  m = row length
 * of y (= C*d*d/ratio).  dim: power of two, 16..256.  tmp: float[n_chains*C*d*d].
 * loss partials: nhmc_cs_tiles(channels, dim) per chain.
 * The data term takes the observation in SPECTRUM layout: y_spec = float[n_chains][C][d*d] with
 * y_spec[chain][c][perm[k]] = y[chain][k*C + c] and NaN at the positions that are not observed -- constant over a run,
 * scattered once by the host -- so that the residual is a coalesced read instead of a gather per element, and at d = 256
 * the forward column pass, the residual and the adjoint's column pass run as ONE kernel on a register-resident panel
 * (three passes over the image instead of four).  tmp for the data term: float[n_chains*C*d*d] at d = 256, twice that
 * otherwise. */
int nhmc_cs_tiles(int channels, int dim);
int nhmc_cs_H(const float* x, const int32_t* kslot, float* y, float* tmp, int n_chains, int channels, int dim,
              int64_t m, nhmc_stream_t stream);
int nhmc_cs_Ht(const float* y, const int32_t* kslot, float* x, float* tmp, int n_chains, int channels, int dim,
               int64_t m, nhmc_stream_t stream);
int nhmc_data_cs(const float* xt, const float* y_spec, int apply_clip, float* g_xt, double* loss_ws, float* tmp,
                 int n_chains, int channels, int dim, nhmc_stream_t stream);
/* nhmc_data_cs on xt_next (the clipped decode of the LAST DDIM step) with that step's VJP applied in the last row
 * pass: writes g_xt and channels [0, channels) of g_e (the caller keeps the sigma-channels zero). */
int nhmc_data_cs_vjp(const float* xt_next, const float* y_spec, const float* xt, const float* e, int e_channels,
                     const float* at, const float* at_next, float* g_xt, float* g_e, double* loss_ws, float* tmp,
                     int n_chains, int channels, int dim, nhmc_stream_t stream);

/* ------------------------------------------------------------------------------------
 * a15  Spectral (anisotropic-blur) operator   Hfuncs.py:448-523
 *   out_c = Lo (D_c o (L^T X_c R)) Ro^T      (H: L,R = V1,V2, Lo,Ro = U1,U2; H^T swaps them)
 * as a chain of fp32-MFMA GEMMs against the four shared d x d factor matrices; d % 64 == 0.
 * "Multiply by M from the left" consumes M^T's memory and "from the right" M's memory (k-major
 * tiles for the MFMA fragments), so the host keeps both orientations of the factors resident.
 * nhmc_spectral_apply   : one sandwich; L, R as stored, LoT = Lo^T, RoT = Ro^T as stored.
 *                         tmp: float[n_chains*C*d*d] scratch.
 * nhmc_data_spectral    : r = y - H clip(xt); loss partials (nhmc_spectral_tiles per chain);
 *                         g_xt = -2 H^T r (masked).  factors: packed [8][d][d] =
 *                         U1,U2,V1,V2,U1^T,U2^T,V1^T,V2^T.  tmp: float[2*n_chains*C*d*d] scratch.
 *                         The forward multiplies by the left factor first (Hfuncs.py:493-509), the adjoint by the
 *                         RIGHT factor first -- the order autograd differentiates those matmuls in at
 *                         main_sampling.py:695,711 -- and every product is an exact k-ascending FMA chain, as
 *                         torch's CPU sgemm is: the data term is the reference's bits.  The right-first order runs on
 *                         transposed operands, hence two constant inputs in transposed form:
 *                         yT = the observation with every channel plane transposed ([n_chains][C][d][d]),
 *                         DmapT = Dmap with every channel plane transposed.
 * ---------------------------------------------------------------------------------- */
int nhmc_spectral_apply(const float* x, const float* L, const float* R, const float* Dmap,
                        const float* LoT, const float* RoT, float* out, float* tmp,
                        int n_chains, int channels, int dim, nhmc_stream_t stream);
int nhmc_spectral_tiles(int channels, int dim);
int nhmc_data_spectral(const float* xt, const float* yT, const float* factors, const float* Dmap,
                       const float* DmapT, int apply_clip, float* g_xt, double* loss_ws, float* tmp,
                       int n_chains, int channels, int dim, nhmc_stream_t stream);
/* a11 + a12/a15 fused: data term on xt_next (the clipped decode of the LAST DDIM step, as nhmc_ddim_mix_fwd wrote it)
 * with the step's VJP applied in the last product's epilogue: writes g_xt and channels [0, channels) of g_e (the caller
 * keeps its sigma-channels zero).  Replaces nhmc_data_spectral(apply_clip = 0) + nhmc_ddim_mix_bwd(final_clip = 1). */
int nhmc_data_spectral_vjp(const float* xt_next, const float* yT, const float* factors, const float* Dmap,
                           const float* DmapT, const float* xt, const float* e, int e_channels, const float* at,
                           const float* at_next,
                           float* g_xt, float* g_e, double* loss_ws, float* tmp, int n_chains, int channels, int dim,
                           nhmc_stream_t stream);

/* The same data term with the residual taken in the operator's left singular basis (U1, U2 orthogonal: full SVDs,
 * Hfuncs.py:473-474):  y - H x = U1 (y^ - D o (V1^T x V2)) U2^T  with  y^ = U1^T y U2, so
 *   |y - H x|^2 = |y^ - D o S|^2   and   H^T (y - H x) = V1 (D o (y^ - D o S)) V2^T      (S = V1^T x V2):
 * four d^3 products per evaluation instead of eight.  y^ is constant over a run (main_sampling.py:694-695,710-711 use
 * the same y_0 in every leapfrog step): compute it once with nhmc_spectral_project.
 * nhmc_spectral_project      : out = L^T Y R per channel image (L = U1, R = U2 as stored); tmp: float[n_chains*C*d*d].
 * nhmc_data_spectral_proj    : as nhmc_data_spectral with y_proj in place of y; tmp: float[n_chains*C*d*d].
 * nhmc_data_spectral_proj_vjp: as nhmc_data_spectral_vjp with y_proj in place of y; same tmp. */
int nhmc_spectral_project(const float* y, const float* L, const float* R, float* out, float* tmp, int n_chains,
                          int channels, int dim, nhmc_stream_t stream);
int nhmc_data_spectral_proj(const float* xt, const float* y_proj, const float* factors, const float* Dmap,
                            int apply_clip, float* g_xt, double* loss_ws, float* tmp, int n_chains, int channels,
                            int dim, nhmc_stream_t stream);
int nhmc_data_spectral_proj_vjp(const float* xt_next, const float* y_proj, const float* factors, const float* Dmap,
                                const float* xt, const float* e, int e_channels, const float* at,
                                const float* at_next, float* g_xt, float* g_e, double* loss_ws, float* tmp,
                                int n_chains, int channels, int dim, nhmc_stream_t stream);

/* Separable strided convolution (SRConv / sr_bicubic, Hfuncs.py:527-607), in the reference's stage order: with
 * V1 = V_small[:, :sd] ([d][sd]), U = U_small ([sd][sd]), S[i][j] = fl(s_i * s_j) ([sd][sd], thresholded singular values):
 *   H(X) = U (S o (V1^T X V1)) U^T,  H^T(Y) = V1 (S o (U^T Y U)) V1^T,  H^+(Y) = V1 (S+ o (U^T Y U)) V1^T  (S+ = 1/S where != 0)
 * every product and the multiplication by S a rounded fp32 stage (H at Hfuncs.py:65-71).  Same MFMA kernel, rectangular.
 * nhmc_sandwich_rect: out = (S1^T in S2) o mul per image, as t = in^T S1, out = (t^T S2) o mul, with in [K1][R1],
 *   S1 [K1][C1], S2 [R1][C2], mul [C1][C2] (nullable: no multiplication), out [C1][C2] (all dims % 32 == 0);
 *   tmp: float[n_img*R1*C1].   V1^T X V1: in = X, S1 = S2 = V1, mul = S;   U Z U^T: in = Z, S1 = S2 = U^T.
 * nhmc_data_srconv: r = y - H(clip(xt)), loss partials (nhmc_srconv_tiles per chain), g = -2 H^T r (masked): eight
 *   products, the adjoint right factor first as in nhmc_data_spectral (autograd's order), so `y` is the observation
 *   with every channel plane TRANSPOSED ([n_chains][C][sd][sd]).  V1T = V1^T as stored [sd][d], UT = U^T [sd][sd];
 *   tmp: float[n_chains*C*(d*sd + 3*sd*sd)]. */
int nhmc_sandwich_rect(const float* in, const float* S1, const float* S2, const float* mul, float* out, float* tmp,
                       int n_img, int K1, int R1, int C1, int C2, nhmc_stream_t stream);
int nhmc_srconv_tiles(int channels, int small_dim);
int nhmc_data_srconv(const float* xt, const float* y, const float* V1, const float* V1T, const float* U, const float* UT,
                     const float* S, int apply_clip, float* g_xt, double* loss_ws, float* tmp, int n_chains,
                     int channels, int dim, int small_dim, nhmc_stream_t stream);
/* nhmc_data_srconv on xt_next (the clipped decode of the LAST DDIM step) with that step's VJP applied in the final
 * product's epilogue (as nhmc_data_spectral_vjp): writes g_xt and channels [0, channels) of g_e. */
int nhmc_data_srconv_vjp(const float* xt_next, const float* y, const float* V1, const float* V1T, const float* U,
                         const float* UT, const float* S, const float* xt, const float* e, int e_channels,
                         const float* at, const float* at_next, float* g_xt, float* g_e, double* loss_ws, float* tmp,
                         int n_chains, int channels, int dim, int small_dim, nhmc_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Nonlinear operators of --algo hmc           main_sampling.py:315-322, :693-695 / :709-711
 *
 * HDR (obs_functions/Hfuncs.py:406-445): H(x) = clip(x / 0.5, -1, 1) elementwise, M = N, y dense [n_chains][N].
 * x / 0.5 is exactly 2 x in fp32, so all elementwise outputs are the reference's bits.  Gradient masks follow torch's
 * clamp backward (the gradient passes where the argument lies inside OR ON the bounds):
 *   nhmc_hdr_H       : y = clip(2 x) over n_total elements (n_total % 4 == 0).
 *   nhmc_data_hdr    : loss partials of sum (y - clip(2 v))^2 (nhmc_data_tiles(n_elem) per chain), v = clip(xt) when
 *                      apply_clip, and g_xt = ((-2 r) 1[|2 v| <= 1]) 2 [1[|xt| <= 1]]   -- autograd of :694-695.
 *   nhmc_mix_bwd_hdr : nhmc_data_hdr on the clipped decode of the LAST DDIM step fused with that step's VJP
 *                      (as nhmc_ddim_mix_bwd_inpaint: R xt, e, y; W g_xt, g_e; nhmc_leapfrog_tiles(n_elem) partials).
 * ---------------------------------------------------------------------------------- */
int nhmc_hdr_H(const float* x, float* y, int64_t n_total, nhmc_stream_t stream);
int nhmc_data_hdr(const float* xt, const float* y, int apply_clip, float* g_xt, double* loss_ws, int n_chains,
                  int64_t n_elem, nhmc_stream_t stream);
int nhmc_mix_bwd_hdr(const float* xt, const float* e, int e_channels, const float* at, const float* at_next,
                     const float* y, float* g_xt, float* g_e, int fill_sigma, double* loss_ws, int n_chains,
                     int channels, int64_t hw, nhmc_stream_t stream);

/* Phase retrieval (obs_functions/Hfuncs.py:318-366, fft2_m / ifft2_m :8-19): H(x) = |fft2c(pad(x, pad))| per channel
 * plane, centred, norm = 'ortho', n = dim + 2 pad; y natural [n_chains][C][n][n], M = C n n.  The zero padding makes the
 * padded centred DFT two rectangular real sandwiches: with F the centred ortho DFT matrix of size n and
 * Fc = F[:, pad:pad+dim] = Cm + i Sm ([n][dim]),
 *     Re Y = Cm X Cm^T - Sm X Sm^T,   Im Y = Cm X Sm^T + Sm X Cm^T,   H(x) = sqrt(Re^2 + Im^2),
 * run on the fp32 MFMA (dim % 32 == 0, (2 pad) % 32 == 0; any such n, no power of two needed).
 * fac: float[6 n dim], packed  [Cm^T | Sm^T] ([dim][2n]),  [Cm | Sm] ([n][2 dim]),  [Sm ; Cm] ([2n][dim]).
 * tmp: float[nhmc_phase_tmp_floats(...)] for every entry below.
 *   nhmc_phase_H       : mode 0: out = H(x) [n_chains][C][n][n];  mode 1: out = [Re Y ; Im Y] [n_chains][C][2][n][n].
 *   nhmc_phase_pinv    : H^+(y) = crop(|ifft2c(y)|) -> [n_chains][C][dim][dim] (the factors conjugated).
 *   nhmc_phase_adjoint : the exact adjoint of x -> [Re Y ; Im Y]: w [n_chains][C][2][n][n] -> [n_chains][C][dim][dim].
 *   nhmc_data_phase    : loss partials of sum (y - |Y(v)|)^2 (nhmc_phase_tiles per chain) and its gradient, the adjoint
 *                        applied to -2 (y - |Y|) Y / |Y| (0 where |Y| = 0, torch's sgn(0)), times the clip mask of xt when
 *                        apply_clip -- autograd of :694-695 through the FFT, as four MFMA launches.
 *   nhmc_data_phase_vjp: the same on xt_next (the clipped decode of the LAST DDIM step) with that step's VJP in the
 *                        last product's epilogue (as nhmc_data_spectral_vjp): writes g_xt and channels [0, C) of g_e. */
int nhmc_phase_tiles(int channels, int dim, int pad);
size_t nhmc_phase_tmp_floats(int n_chains, int channels, int dim, int pad);
int nhmc_phase_H(const float* x, const float* fac, int mode, float* out, float* tmp, int n_chains, int channels, int dim,
                 int pad, nhmc_stream_t stream);
int nhmc_phase_pinv(const float* y, const float* fac, float* out, float* tmp, int n_chains, int channels, int dim, int pad,
                    nhmc_stream_t stream);
int nhmc_phase_adjoint(const float* w, const float* fac, float* out, float* tmp, int n_chains, int channels, int dim,
                       int pad, nhmc_stream_t stream);
int nhmc_data_phase(const float* xt, const float* y, const float* fac, int apply_clip, float* g_xt, double* loss_ws,
                    float* tmp, int n_chains, int channels, int dim, int pad, nhmc_stream_t stream);
int nhmc_data_phase_vjp(const float* xt_next, const float* y, const float* fac, const float* xt, const float* e,
                        int e_channels, const float* at, const float* at_next, float* g_xt, float* g_e, double* loss_ws,
                        float* tmp, int n_chains, int channels, int dim, int pad, nhmc_stream_t stream);

/* Fourier sampling (--deg mri<R>, --deg fourier): undersampled k-space, partial Fourier, band-limited optics.  Not in the
 * reference.  The linear, weighted use of the spectrum above at pad = 0: with F = Cm + i Sm the centred orthonormal DFT
 * matrix of size dim (dim % 32 == 0) and Y_c = F X_c F^T per channel plane,
 *     H(x)   = [w o Re Y ; w o Im Y]                      [n_chains][C][2][dim][dim],  M = 2 C dim^2,
 *     H^T(v) = Re[F^H (w o (v_re + i v_im)) conj(F)]       = nhmc_phase_adjoint(w o v, pad = 0),
 * w: float[dim][dim], every entry >= 0 and finite (the caller checks), centred layout (DC at [dim/2][dim/2]), one map for
 * all channels and chains; a binary mask is the common case.  fac, tmp and the loss partials are those of the phase
 * entries at pad = 0: float[6 dim dim], nhmc_phase_tmp_floats(n_chains, C, dim, 0), nhmc_phase_tiles(C, dim, 0).
 *   nhmc_fourier_H       : out = H(x).
 *   nhmc_data_fourier    : r = y - H(v) where w > 0 and EXACTLY 0 where w = 0 -- a selection, not a product, so that the
 *                          unmeasured entries of y (noise, NaN, inf) reach neither the loss nor the gradient; a NaN in a
 *                          measured entry propagates.  Loss partials of sum r^2 (fp32 squares summed in fp64), and
 *                          g_xt = -2 H^T r, times the clip mask of xt when apply_clip (v = clip(xt) then).
 *   nhmc_data_fourier_vjp: the same on xt_next (the clipped decode of the LAST DDIM step) with that step's VJP in the
 *                          last product's epilogue (as nhmc_data_phase_vjp): writes g_xt and channels [0, C) of g_e.
 * Return codes as everywhere: NHMC_ERR_ARG for a null pointer, NHMC_ERR_SHAPE (dim % 32, e_channels), NHMC_ERR_ALIGN. */
int nhmc_fourier_H(const float* x, const float* fac, const float* w, float* out, float* tmp, int n_chains, int channels,
                   int dim, nhmc_stream_t stream);
int nhmc_data_fourier(const float* xt, const float* y, const float* fac, const float* w, int apply_clip, float* g_xt,
                      double* loss_ws, float* tmp, int n_chains, int channels, int dim, nhmc_stream_t stream);
int nhmc_data_fourier_vjp(const float* xt_next, const float* y, const float* fac, const float* w, const float* xt,
                          const float* e, int e_channels, const float* at, const float* at_next, float* g_xt, float* g_e,
                          double* loss_ws, float* tmp, int n_chains, int channels, int dim, nhmc_stream_t stream);

/* Modulated Fourier operators (--deg mcmri<R>: multi-coil MRI, SENSE; --deg cdp<K>: coded diffraction patterns).  Not in
 * the reference.  The centred DFT of the image times K known complex maps, y_k = post(F (S_k o x) F^T):
 *   d = dim, d % 32 == 0;  F = Cm + i Sm = centred_dft_factors(d, 0, d), fac the phase factors at pad = 0 (float[6 d d]);
 *   maps: float[K][2][d][d], S_k = Sre_k + i Sim_k (a real and an imaginary plane per map), 1 <= K <= 32, every entry
 *         finite, not all zero (the caller checks); the maps are shared by all channels and chains;
 *   w   : float[d][d], real, >= 0 and finite, at least one entry > 0, centred layout (DC at [d/2][d/2]); all ones = no
 *         weighting.
 * Per chain b, channel c and map k, with v = x, or v = clip(x, -1, 1) under apply_clip:
 *     A = Sre_k o v,  B = Sim_k o v                        one fp32 product each
 *     Re Y = Re Y_A - Im Y_B,   Im Y = Im Y_A + Re Y_B     Y_A, Y_B: what nhmc_phase_H(mode 1, pad 0) gives for A and B
 *   linear  (modulus = 0):  H(x) = [w o Re Y ; w o Im Y]      [n_chains][C][K][2][d][d],  M = 2 C K d^2
 *                           r = y - w o Y where w > 0, EXACTLY 0 elsewhere (a selection, as nhmc_data_fourier);  q = w o r
 *   modulus (modulus = 1):  a = sqrtf(Re^2 + Im^2),  H(x) = w o a      [n_chains][C][K][d][d],  M = C K d^2
 *                           r = y - w a where w > 0, else 0;  q = a == 0 ? 0 : (w r) (Y / a)   (nhmc_data_phase's rule: a
 *                           NaN |Y| stays NaN)
 *     loss_b = sum r^2   (fp32 squares, fp64 partials: nhmc_modfourier_tiles per chain, summed in a fixed order)
 *     U_k = Re[F^H q_k conj(F)] = adj(q_re, q_im),   V_k = Im[F^H q_k conj(F)] = adj(q_im, -q_re)
 *                                                          adj = nhmc_phase_adjoint at pad 0
 *     g   = -2 sum_k (Sre_k o U_k + Sim_k o V_k)   [o clip mask of x, selected as everywhere]
 *     H^T(v) (linear only) = sum_k (Sre_k o U_k + Sim_k o V_k) with q = w o v
 * The sum over k ascends from 0.0f; one fixed expression serves H^T, the data term and the fused form, so the fused form
 * is the split path bit for bit, and a chain's bits do not depend on the batch it sits in.
 * Three streaming kernels (csrc/mod_fourier.hip: modulate, combine, demodulate) around the phase chain, which runs on
 * n_chains * C * 2K planes at pad 0: 48 d^3 FLOP per (plane, map).  n_chains * C * 2K <= 65535 (the chain's plane limit).
 * tmp: float[nhmc_modfourier_tmp_floats(...)]: 7 d^2 floats per modulated plane (the planes A and B, their spectra, the
 * chain's own scratch), at most 8 d^2.  The entries walk the chains in slabs of at most 1024 modulated planes (chains are
 * independent), which caps the scratch: 64 chains x 3 channels x 8 maps at 256^2 are 3072 planes, 6.4 GB at 8 d^2 floats
 * each if taken at once, 1.9 GB in slabs.
 *   nhmc_modfourier_H       : out = H(x).
 *   nhmc_modfourier_Ht      : out = H^T(v) [n_chains][C][d][d], v [n_chains][C][K][2][d][d]; linear only, so `modulus` is
 *                             no parameter.
 *   nhmc_data_modfourier    : loss partials and g_xt as above.  The entries of y under w = 0 are loaded and dropped by a
 *                             select: noise, NaN or inf there changes no bit; a NaN in a measured entry propagates.
 *   nhmc_data_modfourier_vjp: the same on xt_next (the clipped decode of the LAST DDIM step) with that step's VJP in the
 *                             demodulating kernel's epilogue: writes g_xt and channels [0, C) of g_e.
 * Return codes: NHMC_ERR_ARG for a null pointer or modulus outside {0, 1}; NHMC_ERR_SHAPE for dim % 32, n_maps outside
 * 1...32, n_chains * channels * 2 * n_maps > 65535, e_channels outside {C, 2C}; NHMC_ERR_ALIGN for a pointer that is not
 * 16-byte aligned.  Shape is checked before alignment. */
int nhmc_modfourier_tiles(int channels, int n_maps, int dim);
size_t nhmc_modfourier_tmp_floats(int n_chains, int channels, int n_maps, int dim);
int nhmc_modfourier_H(const float* x, const float* maps, const float* fac, const float* w, int modulus, float* out,
                      float* tmp, int n_chains, int channels, int n_maps, int dim, nhmc_stream_t stream);
int nhmc_modfourier_Ht(const float* v, const float* maps, const float* fac, const float* w, float* out, float* tmp,
                       int n_chains, int channels, int n_maps, int dim, nhmc_stream_t stream);
int nhmc_data_modfourier(const float* xt, const float* y, const float* maps, const float* fac, const float* w, int modulus,
                         int apply_clip, float* g_xt, double* loss_ws, float* tmp, int n_chains, int channels, int n_maps,
                         int dim, nhmc_stream_t stream);
int nhmc_data_modfourier_vjp(const float* xt_next, const float* y, const float* maps, const float* fac, const float* w,
                             int modulus, const float* xt, const float* e, int e_channels, const float* at,
                             const float* at_next, float* g_xt, float* g_e, double* loss_ws, float* tmp, int n_chains,
                             int channels, int n_maps, int dim, nhmc_stream_t stream);

/* ------------------------------------------------------------------------------------
 * General 2-D PSF blur (--deg deblur_motion): camera shake, defocus, any measured PSF.  Not in the reference's
 * prepare_measurement (its README names an external motion-blur generator that is never wired); the two blurs it has
 * are separable and run through the spectral chain above.
 *
 * PSF: k[K][K] fp32, K odd, 1 <= K <= 63, R = (K - 1) / 2; one PSF for every channel (depthwise), any sign.  M = N and
 * y has the image's shape [n_chains][C][dim][dim].
 * Tap list: the host compacts the PSF's NON-ZERO entries in row-major order (i ascending, then j) into n_taps taps
 * (dy, dx, w) with dy = i - R, dx = j - R.  A zero entry is not a tap: a PSF with a rim of zeros added has the same list
 * and gives the same bits, and an inf under a zero entry stays out (no 0 * inf = NaN).  Everything is defined on the list:
 *   (H x)[c][r][s]   = sum_t w_t x[c][r + dy_t][s + dx_t]      correlation form, terms outside the image omitted
 *                      (zero boundary) -- F.conv2d(x, k, padding = R) per plane
 *   (H^T w)[c][r][s] = sum_t w_t w[c][r - dy_t][s - dx_t]      the exact adjoint: the same list, offsets negated
 * Both accumulate the taps in list order from 0.0f, one fmaf per tap; where the zero boundary applies the term is a
 * +0 * w_t product of a finite weight, which changes no bit of a finite sum.
 * taps_off: DEVICE int32[n_taps][2] = (dy, dx), 8-byte aligned; taps_w: DEVICE float[n_taps]; ksize = K, or any smaller
 * odd size that still holds every offset (the kernels stage a halo of (ksize - 1) / 2 pixels, so the list's own extent
 * 2 max(|dy|, |dx|) + 1 is the cheapest; the result does not depend on it).
 * The entries reject an even K, K > 63, n_taps < 1 or > K^2 (NHMC_ERR_SHAPE) and dim % 4 != 0 (NHMC_ERR_ALIGN).  They
 * cannot read the device list: nhmc_blur2d_check_taps does the same checks and the offset range [-R, R] on the HOST copy
 * (the Python front end calls it when it builds a list), and the kernels clamp an offset into that range (no read leaves the
 * staged halo whatever the device list holds).
 *   nhmc_blur2d_apply    : out = H x, or H^T x when transpose != 0 (out != x).
 *   nhmc_blur2d_tiles    : loss partials per chain of the two data terms.
 *   nhmc_data_blur2d     : loss partials of sum (y - H v)^2, v = clip(xt) when apply_clip else xt (fp32 squares, fp64 tile
 *                          partials, nhmc_sum_partials adds them in a fixed order), and autograd's gradient
 *                          g_xt = H^T(-2 r) [1[|xt| <= 1] when apply_clip, selected as nhmc_masked does].  Two passes;
 *                          the residual r lives in tmp (float[n_chains * C * dim * dim], not aliasing xt or g_xt).
 *   nhmc_data_blur2d_vjp : the same on xt_next (the clipped decode of the LAST DDIM step, no further clip) with that
 *                          step's VJP (inputs xt_in, e) as the epilogue of the adjoint pass: writes g_xt and channels
 *                          [0, C) of g_e, and zeros channels [C, 2C) when fill_sigma and e_channels == 2C
 *                          (as nhmc_mix_bwd_hdr).
 * ---------------------------------------------------------------------------------- */
int nhmc_blur2d_check_taps(const int32_t* host_off, int n_taps, int ksize);
int nhmc_blur2d_tiles(int channels, int dim);
int nhmc_blur2d_apply(const float* x, const int32_t* taps_off, const float* taps_w, int n_taps, int ksize, int transpose,
                      float* out, int n_chains, int channels, int dim, nhmc_stream_t stream);
int nhmc_data_blur2d(const float* xt, const float* y, const int32_t* taps_off, const float* taps_w, int n_taps, int ksize,
                     int apply_clip, float* g_xt, double* loss_ws, float* tmp, int n_chains, int channels, int dim,
                     nhmc_stream_t stream);
int nhmc_data_blur2d_vjp(const float* xt_next, const float* y, const int32_t* taps_off, const float* taps_w, int n_taps,
                         int ksize, const float* xt_in, const float* e, int e_channels, const float* at,
                         const float* at_next, float* g_xt, float* g_e, int fill_sigma, double* loss_ws, float* tmp,
                         int n_chains, int channels, int dim, nhmc_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Sparse linear operators (operators.SparseLinear; --deg ct<V>, --deg sparse --operator FILE.npz): tomography,
 * spatially varying blur, irregular sampling, mosaics -- any linear forward model given as a sparse matrix.  Not in the
 * reference.  The general form of "operator as data": the 2-D blur above carries a tap list, this carries a matrix.
 *
 * One matrix A in R^{m x n}, n = dim * dim, applied to every channel plane alike (depthwise).  M = C * m and
 * y is [n_chains][C][m].
 * Canonical form, built once on the host (nhmc.kernels.SparseMatrix): entries sorted by (row, column); duplicate entries
 * summed in float64, then rounded to fp32; an entry whose fp32 value is 0 is dropped -- a zero is not an entry, so an inf
 * or NaN under it stays out (no 0 * inf = NaN), as for a zero tap.  A is stored as CSR: row_ptr int32[m + 1],
 * col int32[nnz], val float[nnz].  A^T is stored as CSR too, built by a stable transpose: within a row of A^T the
 * entries ascend by their row in A, with the same fp32 values.  Both lists stay resident on the DEVICE.
 *   (A x)[c][i]   = sum_k val_k x[c][col_k]  over the entries k of row i
 *   (A^T w)[c][j] = the same sum on the transposed list: the exact adjoint, both lists hold the same fp32 numbers.
 * Summation: the entries of a row in list order from 0.0f, one fmaf per entry.  The same inputs give the same bits; a
 * plane's result does not depend on n_chains, on channels or on where the plane sits in the batch.
 * An empty row gives +0.  A NaN in x reaches exactly the outputs that have an entry on it.
 * Limits: dim % 4 == 0 (NHMC_ERR_ALIGN, the data terms); 1 <= m, 1 <= nnz < 2^31, n_chains <= 65535, channels <= 65535,
 * n_chains * channels <= 65535 * 64 (NHMC_ERR_SHAPE).  Image pointers and tmp 16-byte aligned.
 * The entries cannot read the device lists: nhmc_sparse_check validates a HOST copy (row_ptr[0] = 0, row_ptr monotone,
 * row_ptr[m] = nnz, every column in [0, n); the Python front end calls it for both lists), and the kernels clamp the row
 * bounds into [0, nnz] and a column into [0, n), so no read leaves a buffer whatever the device lists hold.
 *   nhmc_sparse_tiles      : loss partials per chain of the two data terms.
 *   nhmc_sparse_tmp_floats : floats of tmp for every entry below (the plane-minor operand and result).
 *   nhmc_sparse_apply      : out [n_chains][C][rows] = A x for x [n_chains][C][cols]; given the transposed list (rows = n,
 *                            cols = m) the same entry computes A^T w.  out, x and tmp do not alias.
 *   nhmc_data_sparse       : loss partials of sum (y - A v)^2, v = clip(xt) when apply_clip else xt (fp32 squares, fp64 tile
 *                            partials, nhmc_sum_partials adds them in a fixed order), and autograd's gradient
 *                            g_xt = A^T(-2 r) [1[|xt| <= 1] when apply_clip, selected as nhmc_masked does].  (row_ptr, col,
 *                            val) is A, (t_row_ptr, t_col, t_val) is A^T, both with nnz entries.  The residual r lives in
 *                            tmp (not aliasing xt or g_xt).
 *   nhmc_data_sparse_vjp   : the same on xt_next (the clipped decode of the LAST DDIM step, no further clip) with that
 *                            step's VJP (inputs xt_in, e) as the epilogue of the adjoint pass: writes g_xt and channels
 *                            [0, C) of g_e, and zeros channels [C, 2C) when fill_sigma and e_channels == 2C
 *                            (as nhmc_data_blur2d_vjp).
 * ---------------------------------------------------------------------------------- */
int nhmc_sparse_check(const int32_t* host_row_ptr, const int32_t* host_col, int m, int n, int nnz);
int nhmc_sparse_tiles(int channels, int m);
size_t nhmc_sparse_tmp_floats(int n_chains, int channels, int m, int n);
int nhmc_sparse_apply(const float* x, const int32_t* row_ptr, const int32_t* col, const float* val, int rows, int cols,
                      int nnz, float* out, float* tmp, int n_chains, int channels, nhmc_stream_t stream);
int nhmc_data_sparse(const float* xt, const float* y, const int32_t* row_ptr, const int32_t* col, const float* val,
                     const int32_t* t_row_ptr, const int32_t* t_col, const float* t_val, int m, int nnz, int apply_clip,
                     float* g_xt, double* loss_ws, float* tmp, int n_chains, int channels, int dim, nhmc_stream_t stream);
int nhmc_data_sparse_vjp(const float* xt_next, const float* y, const int32_t* row_ptr, const int32_t* col,
                         const float* val, const int32_t* t_row_ptr, const int32_t* t_col, const float* t_val, int m,
                         int nnz, const float* xt_in, const float* e, int e_channels, const float* at,
                         const float* at_next, float* g_xt, float* g_e, int fill_sigma, double* loss_ws, float* tmp,
                         int n_chains, int channels, int dim, nhmc_stream_t stream);

/* ------------------------------------------------------------------------------------
 * a5  Hamiltonian                          main_sampling.py:697,717-718
 *   H = (0.5*Sx + (1/(2 sigma_y^2))*loss) + (0.5*Sp)*m^-1, per chain, in the reference's fp32
 *   op order on fp32-rounded sums; Sx,Sp summed (fixed order, fp64) from the leapfrog partials.
 * terms (nullable): double[n_chains][3] = Sx, Sp, loss as summed.
 * ---------------------------------------------------------------------------------- */
int nhmc_hamiltonian(const double* sums_ws, int tiles, const double* loss, const double* sigma_y,
                     double m_inv, float* H_out, double* terms, int n_chains,
                     nhmc_stream_t stream);
/* the same with the loss taken from the gradient cache: loss_pair[sel[chain]*loss_stride + chain] */
int nhmc_hamiltonian_cached(const double* sums_ws, int tiles, const double* loss_pair, const int32_t* sel,
                            int64_t loss_stride, const double* sigma_y, double m_inv, float* H_out, double* terms,
                            int n_chains, nhmc_stream_t stream);

/* ------------------------------------------------------------------------------------
 * a6  Metropolis test, per chain, on the device (no host sync)   main_sampling.py:718-720
 *   dH = H1 - H0;  accept = active && (u < min(1, exp(-dH)))
 * ---------------------------------------------------------------------------------- */
int nhmc_metropolis(const float* H0, const float* H1, const float* u, const int32_t* active,
                    int32_t* accept, float* dH, int n_chains, nhmc_stream_t stream);

/* ------------------------------------------------------------------------------------
 * a7  Accept/reject bookkeeping and schedules   main_sampling.py:683-689,721-749
 * nhmc_schedule_begin: per chain, active = epoch < epochs+2*sampling; sigma_y(epoch) anneal;
 *   at epoch == epochs: sigma_y = sigma_0 and (tau > 0.1 -> tau = 0.1, eps = 0.01).
 *   Inactive chains get eps_eff = 0 (frozen), active ones eps_eff = eps.
 * nhmc_accept_commit: accepted chains copy x_prop -> x and, when epoch >= epochs+sampling,
 *   xt_prop -> samples[chain][epoch-(epochs+sampling)] (samples: [n_chains][sampling][n_elem]).
 *   Uses the PRE-increment epoch (:724-727); call before nhmc_schedule_end.
 * nhmc_schedule_end: accept -> epoch += 1, rejected = 0; reject -> rejected += 1 and, from the
 *   second consecutive reject on, tau *= 0.95, eps *= 0.95.
 * ---------------------------------------------------------------------------------- */
int nhmc_schedule_begin(const int32_t* epoch, double* tau, double* eps, double* sigma_y,
                        double* eps_eff, int32_t* active, double sigma_0, int epochs, int sampling,
                        int n_chains, nhmc_stream_t stream);
int nhmc_accept_commit(const int32_t* accept, const int32_t* epoch, float* x, const float* x_prop,
                       const float* xt_prop, float* samples, int epochs, int sampling,
                       int n_chains, int64_t n_elem, nhmc_stream_t stream);
int nhmc_schedule_end(const int32_t* accept, const int32_t* active, int32_t* epoch,
                      int32_t* rejected, double* tau, double* eps, int32_t* n_accept,
                      int32_t* n_reject, int n_chains, nhmc_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Latent variant (hmc_latent)                   main_sampling_latent.py:691-733
 * The epoch index is the shared loop counter there (a reject consumes its epoch), so the host passes
 * what depends on it: final_phase = (epoch >= epochs) and sigma_y_on_accept =
 * sigma_y0*(sigma_0/sigma_y0)**(epoch/epochs) (annealing) or sigma_0 (final phase).
 * nhmc_latent_commit: accepted chains push their PREVIOUS accepted decode xt_last into a ring of the last
 *   `keep` samples when final_phase && has_prev (samples: [n_chains][keep][n_elem], slot count % keep;
 *   :709 runs before :713), then xt_last <- xt_prop, x <- x_prop.  Call before nhmc_schedule_end_latent.
 * nhmc_schedule_end_latent: accept -> rejected = 0, sigma_y = sigma_y_on_accept, final phase also tau = 0.1,
 *   eps = 0.01 and count += has_prev; has_prev = 1.  reject -> rejected += 1; at 2: tau *= 0.9, eps *= 0.9,
 *   rejected = 0.
 * ---------------------------------------------------------------------------------- */
int nhmc_latent_commit(const int32_t* accept, const int32_t* has_prev, const int32_t* count,
                       int final_phase, int keep, float* x, const float* x_prop, float* xt_last,
                       const float* xt_prop, float* samples, int n_chains, int64_t n_elem,
                       nhmc_stream_t stream);
int nhmc_schedule_end_latent(const int32_t* accept, int32_t* rejected, double* tau, double* eps,
                             double* sigma_y, int32_t* count, int32_t* has_prev, int32_t* n_accept,
                             double sigma_y_on_accept, int final_phase, int n_chains,
                             nhmc_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Diagonal-mass variant (hmc_test_conditioning)     main_sampling.py:776-894
 * nhmc_leapfrog_mass: the fused update with a per-element mass (inv_m = 1/M, std_m = sqrt(M), [n_chains][n_elem]):
 *   FIRST: p = z*std_m (z: raw N(0,1) draw, :819); partials Sx = sum x^2, Sp = sum inv_m p^2 (:824);
 *          p -= (eps/2) G; x += (eps p) inv_m (:834)
 *   MID  : p -= eps G (:841); [Welford]; x += (eps p) inv_m
 *   LAST : p -= eps G; p += (eps/2) G (:849); [Welford]; partials of the outputs (:852)
 *   [Welford] (:843-847), for chains with welford_on: delta = x - mean; mean += delta/(l+1); M2 += delta (x - mean),
 *   l = 0-based leapfrog index; at l = 0 mean and M2 are taken as zero (not read).  H = nhmc_hamiltonian with m_inv = 1.
 * nhmc_mass_from_variance (:857-870): variance = M2/(L-1); ascending sort per chain, ties by index (a stable sort:
 *   the reference's default torch.sort leaves the order of equal variances to the sort implementation); the element
 *   of rank r gets std_m = std_table[r], inv_m = inv_table[r], the host-evaluated sqrt(M_r) and 1/M_r of
 *   M_r = exp(2 r/(N-1) - 1) (float[n_elem] device arrays: the transcendental is the reference host's, :863-868);
 *   written for the chains whose flag is set.  ws: nhmc_mass_sort_ws_bytes(n_chains, n_elem) bytes.
 * nhmc_schedule_begin_mass (:808-816): sigma_table[e], e = 0..epochs, are the host-evaluated sigma_y values;
 *   active = epoch < burn+epochs+4*sampling; welford_on = active && (epoch-burn) > epochs/3.
 * ---------------------------------------------------------------------------------- */
int nhmc_leapfrog_mass(int mode, float* x, float* p, const float* z, const float* g, const float* g2,
                       const float* inv_m, const float* std_m, const double* eps, const double* sigma_y,
                       const int32_t* welford_on, float* mean, float* m2, int l, int n_chains,
                       int64_t n_elem, double* sums_ws, nhmc_stream_t stream);
size_t nhmc_mass_sort_ws_bytes(int n_chains, int64_t n_elem);
int nhmc_mass_from_variance(const float* m2, int L, const int32_t* flags, const float* std_table,
                            const float* inv_table, float* inv_m, float* std_m,
                            void* ws, size_t ws_bytes, int n_chains, int64_t n_elem, nhmc_stream_t stream);
int nhmc_schedule_begin_mass(const int32_t* epoch, double* tau, double* eps, double* sigma_y, double* eps_eff,
                             int32_t* active, int32_t* welford_on, const double* sigma_table, int burn, int epochs,
                             int sampling, int n_chains, nhmc_stream_t stream);

/* ------------------------------------------------------------------------------------
 * f.1  Codebook lookup of the VQ first stage on decode (latent variant)
 *      ldm/models/autoencoder.py:274-279 -> taming VectorQuantizer2.forward (not vendored; taming-transformers==0.0.1)
 *   per latent pixel: k* = argmin_k (|z|^2 + |e_k|^2) - 2 z.e_k (first minimum), z_q = z + (e_k* - z)
 * z, z_q: [n_chains][channels][hw] (channels = embed_dim in {3, 4}); codebook: [n_embed][channels];
 * idx (nullable): int32 [n_chains][hw].  The backward of this step is the identity (straight-through).
 * ---------------------------------------------------------------------------------- */
int nhmc_vq_nearest(const float* z, const float* codebook, float* z_q, int32_t* idx, int n_chains,
                    int channels, int64_t hw, int n_embed, nhmc_stream_t stream);

/* ------------------------------------------------------------------------------------
 * a16 glue  Fused GroupNorm (+ FiLM scale/shift) (+ SiLU) of the score networks, forward and input gradient
 *      guided_diffusion/unet_ffhq.py:310-321 (GroupNorm32, scale-shift norm, SiLU); ldm/modules/diffusionmodules/model.py:38-39
 *   u = ((x - mean_g) rstd_g gamma_c + beta_c) (1 + scale_bc) + shift_bc ;   y = act ? u sigmoid(u) : u
 * x, y, dy, dx: [n][channels][hw] contiguous fp32 (hw % 4 == 0); gamma, beta: [channels];
 * film (nullable): [n][film_stride] with scale at [c] and shift at [channels + c] (the reference's emb_out.chunk(2)).
 * pre (nullable): x + pre[b * pre_stride + c] is what gets normalised -- the bias of the convolution that produced x
 *   (pre_stride = 0) or bias + a per-sample embedding term ([n][pre_stride], openaimodel.py:257 `h = h + emb_out`), so the
 *   producer runs without its broadcast add pass.
 * ws: double[n * groups][splits][2] partial sums (splits = nhmc_gn_splits(...)); the forward's ws is an input of the
 * backward (mean / rstd are re-derived from it; nothing else is saved).  Only dx is produced: the networks are frozen.
 * ---------------------------------------------------------------------------------- */
int nhmc_gn_splits(int n, int channels, int groups, int64_t hw);
int nhmc_gn_act_fwd(const float* x, const float* gamma, const float* beta, const float* film, int64_t film_stride,
                    const float* pre, int64_t pre_stride, float eps, int act, float* y, double* ws, int splits,
                    int n, int channels, int groups, int64_t hw, nhmc_stream_t stream);
/* dx_add (optional, same shape as x, must not alias dx): a second gradient of x -- in a ResBlock the block input feeds the
 * GroupNorm AND the skip path -- added to the result in the same pass: dx = fl(dx_groupnorm) + dx_add, the bits of
 * autograd's separate accumulation add. */
int nhmc_gn_act_bwd(const float* x, const float* dy, const float* gamma, const float* beta, const float* film,
                    int64_t film_stride, const float* pre, int64_t pre_stride, float eps, int act,
                    const double* fwd_ws, const float* dx_add, float* dx, double* ws, int splits, int n, int channels,
                    int groups, int64_t hw, nhmc_stream_t stream);
/* nhmc_gn_act_bwd with the forward's workspace at a split count of its own (fwd_splits, 1..64): what a forward of the
 * one-pass entries below leaves.  nhmc_gn_act_bwd(..., splits, ...) == nhmc_gn_act_bwd_fs(..., fwd_splits = splits, ...). */
int nhmc_gn_act_bwd_fs(const float* x, const float* dy, const float* gamma, const float* beta, const float* film,
                       int64_t film_stride, const float* pre, int64_t pre_stride, float eps, int act,
                       const double* fwd_ws, int fwd_splits, const float* dx_add, float* dx, double* ws, int splits, int n,
                       int channels, int groups, int64_t hw, nhmc_stream_t stream);
/* One-pass forms of the two entries above (csrc/gn_onepass.hip): one launch each, in which every workgroup keeps its share
 * of a (sample, group) slab in registers while the slab's statistics are exchanged between the workgroups, so x (and dy) is
 * read once.  Same formulas, same ws layout: double[n * groups][splits][2] with splits = nhmc_gn_onepass_splits(...), which
 * (the forward writes n * groups more pairs behind them, the slab totals: ws is double[n * groups * (splits + 1) * 2], and
 * ws + n * groups * splits * 2 is a workspace of one split, which a backward may be given with fwd_splits = 1)
 * is 0 for a shape these entries do not cover (the caller then keeps the two-pass entries; the one-pass entries themselves
 * answer NHMC_ERR_SHAPE).  fwd_splits: the split count of the workspace the forward wrote (either path's).
 * ws (16-byte aligned, a buffer of its own) is also what the workgroups of a slab exchange their partial sums through:
 *   when splits > 1 the entry fills it with the byte 0xFF on `stream` ahead of its launch (a node of its own under
 *   graph capture), and a word that no longer holds that pattern has been published.
 * nhmc_gn_onepass_prefers(backward, ...): 1 when the one-pass entry is the faster one for this shape and direction (the
 *   measured rule is next to its definition), 0 when the caller should keep the two-pass entry.
 * flags: 0, or NHMC_GN_ONEPASS_NOWAIT (tests only): no workgroup waits for the others, each computes the whole slab's
 *   statistics itself -- the path a workgroup takes when its bounded wait expires; the results are the same bits.
 * Two sources / destinations (the concatenated input of a U-Net output block):
 *   forward: x2 != NULL -> the logical input is cat(x1 [n][c1][hw], x2 [n][channels - c1][hw]) along the channels,
 *     0 < c1 < channels (NHMC_ERR_SHAPE otherwise), and x_cat [n][channels][hw] (required then, NHMC_ERR_ARG without it)
 *     receives the concatenation; x2 == NULL -> c1 == channels and x_cat == NULL.  y is always [n][channels][hw].
 *   backward: x, dy, dx_add are [n][channels][hw]; dx2 != NULL -> dx is written as dx1 [n][c1][hw] and
 *     dx2 [n][channels - c1][hw]; dx2 == NULL -> c1 == channels.  dx_add must alias neither, and neither may alias x or
 *     dy (NHMC_ERR_ARG): the one-pass backward is not in place.
 * Null pointers / unknown flags: NHMC_ERR_ARG; a pointer off 16 bytes: NHMC_ERR_ALIGN; all before any device work. */
#define NHMC_GN_ONEPASS_NOWAIT 1
int nhmc_gn_onepass_splits(int n, int channels, int groups, int64_t hw);
int nhmc_gn_onepass_prefers(int backward, int n, int channels, int groups, int64_t hw);
int nhmc_gn_onepass_fwd(const float* x1, const float* x2, int c1, const float* gamma, const float* beta, const float* film,
                        int64_t film_stride, const float* pre, int64_t pre_stride, float eps, int act, float* y,
                        float* x_cat, double* ws, int flags, int n, int channels, int groups, int64_t hw,
                        nhmc_stream_t stream);
int nhmc_gn_onepass_bwd(const float* x, const float* dy, const float* gamma, const float* beta, const float* film,
                        int64_t film_stride, const float* pre, int64_t pre_stride, float eps, int act,
                        const double* fwd_ws, int fwd_splits, const float* dx_add, float* dx1, float* dx2, int c1,
                        double* ws, int flags, int n, int channels, int groups, int64_t hw, nhmc_stream_t stream);
/* out = (h + bias_c) + other, [n][channels][hw]: a convolution's bias folded into the residual add that follows it
 * (unet_ffhq.py:321).  Its backward is the identity towards both h and other. */
int nhmc_bias_add2(const float* h, const float* bias, const float* other, float* out, int n, int channels,
                   int64_t hw, nhmc_stream_t stream);

/* ------------------------------------------------------------------------------------
 * a16 conv  3x3 stride-1 padding-1 convolution of the score network as Winograd F(2x2, 3x3) on the fp32 matrix cores
 *      (csrc/wino_conv.hip), forward and backward-data; fp32 NCHW, one launch, no transformed tensor in HBM.
 *   y[n][k][h][w] = sum_c sum_rs x[n][c][h + r - 1][w + s - 1] weight[k][c][r][s]   (+ bias[k]) (+ add[n][k][h][w])
 * nhmc_wino_weights: u[16][c'][k'] = G g G^T of weight [channels_out][channels_in][3][3] (contiguous).
 *   backward = 0: (c', k') = (channels_in, channels_out), g = weight[k'][c'] -- the forward convolution;
 *   backward = 1: (c', k') = (channels_out, channels_in), g[r][s] = weight[c'][k'][2 - r][2 - s] -- the filter of the
 *   backward-data pass, dx = conv(dy, g), which then runs through nhmc_conv3x3_wino like a forward one.
 *   u holds 16 * channels_in * channels_out floats; it is a function of the weights alone (build once, reuse).
 * nhmc_conv3x3_wino: x [n][c][h][w], u from nhmc_wino_weights with (c', k') = (c, k), y [n][k][h][w];
 *   bias (nullable) [k], add (nullable) [n][k][h][w]: y = (acc + bias[k]) + add, the order of nhmc_bias_add2 (add may be y).
 *   Accumulation runs over c ascending with no atomics: equal inputs give equal bits.
 *   Covered (nhmc_conv3x3_wino_covers = 1): c % 8 == 0, k % 64 == 0, h % 4 == 0, w % 64 == 0, h * w <= 2^24; stride and
 *   padding must both be 1.  Anything else: NHMC_ERR_SHAPE; null x / u / y or y == x: NHMC_ERR_ARG; a pointer off 16
 *   bytes: NHMC_ERR_ALIGN; all before any device work.
 * nhmc_conv3x3_wino_prefers(backward, n, c, k, h, w): 1 when this entry measured at most 0.90 of the vendor library's time
 *   for the shape and direction (c, k: the channels of the convolution that runs, i.e. of dy and dx for backward = 1);
 *   the table is next to its definition and says which rows are convolutions of unet.FFHQ_CONFIG (unet.conv3x3_shapes()).
 *   Only n = 64 was measured; other batch sizes follow the same (c, k, h, w) rows.
 * nhmc_conv3x3_wino_narrow, _narrow_covers, _narrow_prefers: the same kernel, arguments, validation order and results for
 *   images 32 and 16 wide, which the entries above refuse: the workgroup's 64 tiles are 4 x 16 (w = 32, h % 8 == 0) or
 *   8 x 8 (w = 16, h % 16 == 0) instead of 2 x 32.  Every other width is NHMC_ERR_SHAPE here.  u is shared with the wide entry.
 * nhmc_conv3x3_wino_k32, _k32_covers, _k32_prefers: the same kernel, arguments, validation order and results for k % 32 == 0
 *   (k >= 32) in all three geometries, chosen by w; _k32_covers is 1 wherever _covers or _narrow_covers is.  With k % 64 == 32
 *   the last block of 64 output channels is half empty: its upper 32 rows of u are not read and nothing is stored for them.
 *   u is nhmc_wino_weights' with the same (c', k'), no padding.  An output channel's bits do not depend on k, so k % 64 == 0
 *   gives what the entries above give.  _k32_prefers lists shapes with k % 64 == 32 only, measured at n = 16.
 * ---------------------------------------------------------------------------------- */
int nhmc_wino_weights(const float* weight, float* u, int backward, int channels_in, int channels_out, nhmc_stream_t stream);
int nhmc_conv3x3_wino(const float* x, const float* u, const float* bias, const float* add, float* y, int n, int c, int k,
                      int h, int w, int stride, int padding, nhmc_stream_t stream);
int nhmc_conv3x3_wino_covers(int n, int c, int k, int h, int w);
int nhmc_conv3x3_wino_prefers(int backward, int n, int c, int k, int h, int w);
int nhmc_conv3x3_wino_narrow(const float* x, const float* u, const float* bias, const float* add, float* y, int n, int c,
                             int k, int h, int w, int stride, int padding, nhmc_stream_t stream);
int nhmc_conv3x3_wino_narrow_covers(int n, int c, int k, int h, int w);
int nhmc_conv3x3_wino_narrow_prefers(int backward, int n, int c, int k, int h, int w);
int nhmc_conv3x3_wino_k32(const float* x, const float* u, const float* bias, const float* add, float* y, int n, int c, int k,
                          int h, int w, int stride, int padding, nhmc_stream_t stream);
int nhmc_conv3x3_wino_k32_covers(int n, int c, int k, int h, int w);
int nhmc_conv3x3_wino_k32_prefers(int backward, int n, int c, int k, int h, int w);
/* nhmc_conv3x3_wino_up: nhmc_conv3x3_wino next to a nearest 2x upsample (unet_ffhq.py:299-321, the up-sampling ResBlock),
 *   with the upsampled or pooled tensor never in memory.  n, c, k, h, w are the convolution's own; `mode` is ONE of
 *   NHMC_WINO_IN_UP:    x is [n][c][h / 2][w / 2] and stands for its nearest 2x upsample; add must be null.  The seven
 *                       Winograd frequencies that are +0 for such an input are not multiplied.
 *   NHMC_WINO_ADD_UP:   add (required, not y) is [n][k][h / 2][w / 2] and stands for its nearest 2x upsample.
 *   NHMC_WINO_OUT_POOL: y is [n][k][h / 2][w / 2], the sum over each 2 x 2 block of the convolution's output, formed as
 *                       ((((0 + y00) + y01) + y10) + y11) * 0.25f * 4.0f; bias and add must be null.
 *   For finite inputs each gives the bits of nhmc_conv3x3_wino composed with nhmc_sr_Ht (scale 1) / nhmc_sr_H and a
 *   multiplication by 4 on the materialised tensor.  With non-finite inputs the non-finite output positions are the same,
 *   their values may differ (the skipped products held inf - inf).  Runs on the eight-wave kernel only:
 *   nhmc_conv3x3_wino_up_covers = nhmc_conv3x3_wino_covers and NHMC_WINO_WAVES unset or 8; anything else is
 *   NHMC_ERR_SHAPE.  Validation order as nhmc_conv3x3_wino, a mode / pointer mismatch is NHMC_ERR_ARG. */
#define NHMC_WINO_IN_UP 1
#define NHMC_WINO_ADD_UP 2
#define NHMC_WINO_OUT_POOL 4
int nhmc_conv3x3_wino_up(const float* x, const float* u, const float* bias, const float* add, float* y, int n, int c, int k,
                         int h, int w, int mode, nhmc_stream_t stream);
int nhmc_conv3x3_wino_up_covers(int n, int c, int k, int h, int w);
/* nhmc_conv3x3_wino_skip: nhmc_conv3x3_wino whose `add` arrives without its per-channel bias (the ResBlock whose skip path
 *   is a 1x1 convolution: that convolution runs without its bias and the broadcast pass over its output never does).
 *   add [n][k][h][w] and add_bias [k] are both required; y = (acc + bias[k]) + (add + add_bias[k]), bias nullable: the bits
 *   of nhmc_conv3x3_wino on an `add` to which add_bias was added in fp32 beforehand, NaN and inf included.  add may be y.
 *   Runs on the eight-wave kernel only: nhmc_conv3x3_wino_skip_covers = nhmc_conv3x3_wino_covers and NHMC_WINO_WAVES unset
 *   or 8; anything else is NHMC_ERR_SHAPE.  Validation order as nhmc_conv3x3_wino; a null add or add_bias is NHMC_ERR_ARG. */
int nhmc_conv3x3_wino_skip(const float* x, const float* u, const float* bias, const float* add, const float* add_bias, float* y,
                           int n, int c, int k, int h, int w, nhmc_stream_t stream);
int nhmc_conv3x3_wino_skip_covers(int n, int c, int k, int h, int w);

/* ------------------------------------------------------------------------------------
 * a16 thin conv  direct 3x3 stride-1 padding-1 convolution from a thin input (c <= 8 channels) to a wide output (k a multiple
 *      of 32) on packed fp32 FMA (csrc/thin_conv.hip): the score network's first layer and the backward-data pass of its
 *      last one; fp32 NCHW, one launch, no workspace.
 *   y[n][k][h][w] = sum_c sum_rs x[n][c][h + r - 1][w + s - 1] g[k][c][r][s]   (+ bias[k])
 * nhmc_thin_in_weights: wp[wide / 2][9 thin][2], the filter re-laid-out by output-channel pairs; thin * wide * 9 floats,
 *   a function of the weights alone (build once, reuse).
 *   backward = 0: weight is [wide][thin][3][3] and g = weight -- the forward convolution of a thin input;
 *   backward = 1: weight is [thin][wide][3][3] and g[k][c][r][s] = weight[c][k][2 - r][2 - s] -- the backward-data pass of
 *   a convolution with a thin OUTPUT, dx = conv(dy, g), dy thin.
 * nhmc_conv3x3_thin_in: x [n][c][h][w], wp from nhmc_thin_in_weights with (thin, wide) = (c, k), bias (nullable) [k],
 *   y [n][k][h][w].  One FMA chain per output (c, then r, then s ascending; zero padding by predicate), the bias added
 *   last; no atomics: equal inputs give equal bits.
 *   Covered (nhmc_conv3x3_thin_in_covers = 1): n >= 1, 1 <= c <= 8, k % 32 == 0, w % 4 == 0, h * w <= 2^24; stride and
 *   padding must both be 1.  Anything else: NHMC_ERR_SHAPE; null x / wp / y, y == x or y == wp: NHMC_ERR_ARG; x, wp or y
 *   off 16 bytes: NHMC_ERR_ALIGN; all before any device work.
 * nhmc_conv3x3_thin_in_prefers(backward, n, c, k, h, w): 1 when this entry measured at most 0.90 of the vendor library's
 *   sequence for the shape and direction (c, k: the channels of the convolution that runs); the table is next to its
 *   definition.  Only n = 64 was measured; other batch sizes follow the same rows.
 * nhmc_thin_out_weights, nhmc_conv3x3_thin_out, _covers, _prefers: the mirror image, a wide input (c % 32 == 0) to a thin
 *   output (k <= 8): the network's last layer and the backward-data pass of its first one.  gp[wide][9][2 ceil(thin / 2)]
 *   (wide * 9 * 2 ceil(thin / 2) floats); backward = 0: weight is [thin][wide][3][3]; backward = 1: weight is
 *   [wide][thin][3][3] and g[k][c][r][s] = weight[c][k][2 - r][2 - s].  x [n][c][h][w], bias (nullable) [k], y [n][k][h][w];
 *   the same summation order, coverage conditions (with c and k exchanged), error codes and validation order.
 * ---------------------------------------------------------------------------------- */
int nhmc_thin_in_weights(const float* weight, float* wp, int backward, int thin, int wide, nhmc_stream_t stream);
int nhmc_conv3x3_thin_in(const float* x, const float* wp, const float* bias, float* y, int n, int c, int k, int h, int w,
                         int stride, int padding, nhmc_stream_t stream);
int nhmc_conv3x3_thin_in_covers(int n, int c, int k, int h, int w);
int nhmc_conv3x3_thin_in_prefers(int backward, int n, int c, int k, int h, int w);
int nhmc_thin_out_weights(const float* weight, float* gp, int backward, int thin, int wide, nhmc_stream_t stream);
int nhmc_conv3x3_thin_out(const float* x, const float* gp, const float* bias, float* y, int n, int c, int k, int h, int w,
                          int stride, int padding, nhmc_stream_t stream);
int nhmc_conv3x3_thin_out_covers(int n, int c, int k, int h, int w);
int nhmc_conv3x3_thin_out_prefers(int backward, int n, int c, int k, int h, int w);

/* PSNR of clamp((xt+1)/2,0,1) against clamp((x_orig+1)/2,0,1)   main_sampling.py:738-739
 * ws: double[n_chains][nhmc_data_tiles(n_elem)]. */
int nhmc_psnr(const float* xt, const float* x_orig, float* psnr, double* ws,
              int n_chains, int64_t n_elem, nhmc_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Report stage: the metrics `sample_image` takes of the collected samples      main_sampling.py:488-561
 *
 *   samples : fp32 [n_chains][n_samples][C][H][W] in [-1,1], as the sampler returns them; x_orig : fp32 [n_chains][C][H][W].
 *   Sample j of chain b (row b * n_samples + j) is compared against x_orig[b]; x_orig is indexed, never expanded.
 *   Both images pass through the reference's inverse_data_transform, clamp((v+1)/2, 0, 1) in fp32, inside the kernels.
 *   n_elem = C*H*W with n_elem % 4 == 0, 16-byte aligned image bases, n_chains * n_samples <= 65535, C <= 65535.
 *   Reductions: per-tile fp64 partials in the caller's workspace plus a fixed-order second pass; equal inputs, equal bits.
 *   Validation, before any launch: null pointer / non-positive size -> ARG, alignment or n_elem % 4 -> ALIGN, then SHAPE.
 *
 * nhmc_psnr_samples: PSNR of every sample against its chain's original (:517-519), one launch pair for the whole block;
 *   the arithmetic is nhmc_psnr's (same kernels), so psnr[b * n_samples + j] has the bits nhmc_psnr gives for that pair.
 *   ws: double[n_chains * n_samples][nhmc_data_tiles(n_elem)].
 * nhmc_sample_range: range[i] = max - min of transformed sample i over all channels, the fp32 difference the reference
 *   passes as `data_range` (:520: the SAMPLE's range, not the original's).
 *   ws: double[n_chains * n_samples][nhmc_data_tiles(n_elem)][2]; nhmc_ssim_ws_bytes covers it.
 * nhmc_ssim: skimage.metrics.structural_similarity(sample, orig, data_range=range[i], channel_axis=0) at its defaults
 *   (:520): 7x7 uniform window, NP = 49, sample covariance (cov_norm = 49/48), K1 = 0.01, K2 = 0.03,
 *   C1 = (K1 R)^2, C2 = (K2 R)^2; per channel plane, with ux, uy, uxx, uyy, uxy the window means of x, y, xx, yy, xy:
 *     vx = cov_norm (uxx - ux^2), vy = cov_norm (uyy - uy^2), vxy = cov_norm (uxy - ux uy),
 *     S = ((2 ux uy + C1)(2 vxy + C2)) / ((ux^2 + uy^2 + C1)(vx + vy + C2)),
 *   the plane's value is the mean of S over the plane cropped by 3 pixels on every side (only windows wholly inside the
 *   image count, so no border mode enters) and a sample's SSIM is the mean of its planes' values.  fp64 from the products
 *   on (fp32 inputs: the products are exact); ssim is double[n_chains * n_samples].  range[i] = 0 is not special-cased.
 *   One block per (tile, channel, sample): nhmc_ssim_tiles(h, w) tiles of 16 x 32 window positions per plane.
 *   H < 7 or W < 7: NHMC_ERR_SHAPE (nhmc_ssim_tiles returns 0).
 *   ws: double[n_chains * n_samples][C][nhmc_ssim_tiles(h, w)]; nhmc_ssim_ws_bytes(n, c, h, w) is the larger of this and
 *   nhmc_sample_range's need for n = n_chains * n_samples samples, so one workspace serves both calls in turn.
 * nhmc_sample_moments: per chain, over its n_samples >= 2 samples (:494 guards with len(xt) > 1; fewer: NHMC_ERR_SHAPE):
 *     mean    [n_chains][C][H][W]  mean of the RAW samples (the posterior-mean image), fp64 sum rounded once to fp32;
 *     std_map [n_chains][H][W]     x.std(dim=0).mean(dim=0) of the TRANSFORMED samples (:495-496): per pixel and channel
 *                                  the two-pass unbiased std in fp64 (mean, then squared deviations), averaged over the
 *                                  channels, rounded once to fp32;
 *     minmax  [n_chains][2]        the map's minimum and maximum (:497), fp32.
 *   ws: double[n_chains][nhmc_moments_tiles(h * w)][2].
 * nhmc_std_map_normalise: out = (std_map - min) / (max - min) in fp32 (:497), the picture saved as std_dev_map_{idx}.png.
 * Not served: LPIPS (:521) needs the lpips package and its VGG weights.
 * ---------------------------------------------------------------------------------- */
int nhmc_psnr_samples(const float* samples, const float* x_orig, float* psnr, double* ws, int n_chains, int n_samples,
                      int64_t n_elem, nhmc_stream_t stream);
int nhmc_ssim_tiles(int h, int w);
size_t nhmc_ssim_ws_bytes(int n_total_samples, int c, int h, int w);
int nhmc_sample_range(const float* samples, float* range, double* ws, int n_total_samples, int64_t n_elem,
                      nhmc_stream_t stream);
int nhmc_ssim(const float* samples, const float* x_orig, const float* range, double* ssim, double* ws, int n_chains,
              int n_samples, int c, int h, int w, nhmc_stream_t stream);
int nhmc_moments_tiles(int64_t hw);
int nhmc_sample_moments(const float* samples, float* mean, float* std_map, float* minmax, double* ws, int n_chains,
                        int n_samples, int c, int h, int w, nhmc_stream_t stream);
int nhmc_std_map_normalise(const float* std_map, const float* minmax, float* out, int n_chains, int64_t hw,
                           nhmc_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Convergence of replica chains: split R-hat and effective sample size per element, on the device.
 *
 *   samples : fp32 [n_groups * n_replicas][n_samples][n_elem], the block the sampler returns; chain g * n_replicas + r is
 *             replica r of image (group) g.  rhat, ess : fp32 [n_groups][n_elem], each rounded once from fp64.
 *   summary : fp64 [n_groups][6].  ws : double, nhmc_chain_diag_ws_bytes(n_groups, n_elem) bytes: 8 partials for each of
 *             the nhmc_chain_diag_tiles(n_elem) tiles (256 elements each) of every group.
 *   Validation, before any launch: null pointer / non-positive size -> ARG; samples, rhat or ess not 16-byte aligned or
 *   n_elem % 4 != 0 -> ALIGN; n_samples < 4, n_samples / 2 > 32, n_replicas * n_samples > 4096 or n_groups > 65535 -> SHAPE.
 *   n_replicas = 1 is allowed: split R-hat of one chain is defined.
 *
 * Definition, per element e of group g, with S = n_samples and K = n_replicas.  All arithmetic is fp64 on the fp32 inputs.
 *   Split chains.  n = S / 2 (integer division) and M = 2K.  Split chain 2r is draws [0, n) of replica r, split chain
 *     2r+1 is draws [S - n, S); for odd S the middle draw is dropped.
 *   Per split chain m.  Mean mu_m: a sum over n divided once.  Deviations d = x - mu_m.  Biased autocovariances
 *     a_m[t] = (1/n) sum_{i=0}^{n-1-t} d_i d_{i+t}  for t = 0 and for 1 <= t <= n - 2.
 *   Variances.  W = (1/M) sum_m a_m[0] * n/(n-1).  Bn = the ddof = 1 variance of the M means (taken about the first split
 *     chain's mean, which leaves the value unchanged and makes chains that sit at one common value give exactly 0).
 *     V = W (n-1)/n + Bn.
 *   R-hat.  V == 0: the element is *constant* (clipped pixels make this common): rhat = ess = NaN.
 *     V > 0 and W == 0 (chains stuck at different constants): rhat = +inf, ess = NaN.  Otherwise rhat = sqrt(V / W).
 *   Autocorrelations.  rho_0 = 1 and rho_t = 1 - (W - (1/M) sum_m a_m[t]) / V for t >= 1.
 *   ESS: Geyer's initial monotone sequence as in the Stan reference manual, on the raw draws (no rank normalisation).
 *     For k = 0, 1, ... while 2k + 1 <= n - 2: P_k = rho_{2k} + rho_{2k+1}; stop at the first k with P_k <= 0; each kept
 *     P_k is replaced by min(P_k, P_{k-1}).  tau = -1 + 2 sum of the kept P_k, tau = max(tau, 1 / log10(M n)),
 *     ess = M n / tau.  So S < 6 (n = 2: no P_k exists) always yields the cap M n log10(M n).
 *   Summary per group, from the fp64 values before rounding:
 *     [0] rhat_max         over the non-constant elements; may be +inf; NaN when every element is constant
 *     [1] rhat_mean        over the finite values
 *     [2] rhat_frac_above  share of the non-constant elements with rhat > rhat_threshold (+inf counts)
 *     [3] ess_min, [4] ess_mean   over the non-NaN values
 *     [5] n_constant       number of constant elements
 *     A mean or share over no element is NaN.
 *   Reductions: per-tile fp64 partials in ws and a fixed-order second pass; equal inputs give equal bits, no atomics.
 *   Every sample value is read once: K S 4 bytes per element read, 8 written.
 * ---------------------------------------------------------------------------------- */
int nhmc_chain_diag_tiles(int64_t n_elem);
size_t nhmc_chain_diag_ws_bytes(int n_groups, int64_t n_elem);
int nhmc_chain_diag(const float* samples, float* rhat, float* ess, double* summary, double* ws, int n_groups,
                    int n_replicas, int n_samples, int64_t n_elem, double rhat_threshold, nhmc_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Calibration of the posterior samples against the original image, on the device.
 *
 *   samples : fp32 [n_groups * n_replicas][n_samples][n_elem], the block the sampler returns; chain g * n_replicas + r is
 *             replica r of image (group) g.  x_orig : fp32 [n_groups][n_elem].  Raw values in [-1, 1], finite.
 *   z       : fp32 [n_groups][n_elem];  counts : int32 [n_groups][n_elem] = below + 65536 * equal.
 *   hist    : int64 [n_groups][n + 1], zeroed by the entry on the stream;  summary : fp64 [n_groups][8].
 *   ws      : double, nhmc_calibration_ws_bytes(n_groups, n_elem) bytes: 8 partials for each of the
 *             nhmc_calibration_tiles(n_elem) tiles (256 elements each) of every group.
 *   Validation, before any launch: null pointer / non-positive size -> ARG; samples, x_orig, z or counts not 16-byte
 *   aligned or n_elem % 4 != 0 -> ALIGN; n < 2, n > 1024 or n_groups > 65535 -> SHAPE, with n = n_replicas * n_samples.
 *
 * Definition, per element of group g.  The n = n_replicas * n_samples draws of the element are pooled: d_1 ... d_n, d_1
 * being the first sample of replica 0 (draw i is row g * n + i - 1 of the block); t is the original's value.
 *   below = #{i : d_i < t},  equal = #{i : d_i == t}            fp32 comparisons, hence exact
 *   mu = d_1 + sum(d_i - d_1) / n                                fp64; the shift by a draw keeps the one-pass form benign
 *   v  = max(0, (sum (d_i - d_1)^2 - (sum(d_i - d_1))^2 / n) / (n - 1)),  s = sqrt(v)
 *        All draws equal gives s = 0 exactly: the element is *flat*.
 *   z  = (t - mu) / s  in fp64, rounded once to fp32; for s = 0 it is +-inf when t != mu and NaN when t == mu.
 * Summary per group, fp64 sums over its n_elem elements:
 *     [0] sum_err2 = sum (t - mu)^2      [1] sum_var = sum v             [2] sum_abs_err = sum |t - mu|
 *     [3] sum_std  = sum s               [4] sum_abs_err_std = sum |t - mu| s
 *     [5] sum_z2   = sum over s > 0 of z^2 (z before rounding)
 *     [6] n_tied   = #{equal > 0}        [7] n_flat = #{s == 0}
 * Rank histogram: hist[b], b = 0 ... n, counts the elements with equal == 0 and below == b.  A tied element (a clipped
 *   pixel, say) has no rank: it is left out of the histogram and counted in n_tied.
 * Reductions: the sums go through per-tile fp64 partials in ws and a fixed-order second pass; the histogram is summed per
 *   block in LDS and added to hist with integer atomics, which no order of arrival changes.  Equal inputs give equal bits.
 * Every sample value is read once, and t once: n * 4 + 4 bytes per element read, 8 written.
 * ---------------------------------------------------------------------------------- */
int nhmc_calibration_tiles(int64_t n_elem);
size_t nhmc_calibration_ws_bytes(int n_groups, int64_t n_elem);
int nhmc_calibration(const float* samples, const float* x_orig, float* z, int32_t* counts, int64_t* hist, double* summary,
                     double* ws, int n_groups, int n_replicas, int n_samples, int64_t n_elem, nhmc_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Credible interval and median of the posterior samples, on the device: the interval "Calibration" speaks of.
 *
 *   samples : fp32 [n_groups * n_replicas][n_samples][n_elem], laid out and pooled as for nhmc_calibration: draw i of
 *             group g is row g * n + i - 1 of the block, n = n_replicas * n_samples.  Any value, NaN and +-inf included.
 *   x_orig  : fp32 [n_groups][n_elem], or NULL.    lower, median, upper : fp32 [n_groups][n_elem].
 *   summary : fp64 [n_groups][6].  ws : double, nhmc_credible_ws_bytes(n_groups, n_elem) bytes: 8 partials for each of the
 *             nhmc_credible_tiles(n_elem) tiles (256 elements each) of every group.
 *   Validation, before any launch: null pointer (x_orig excepted) / non-positive size -> ARG; samples, x_orig, lower, median
 *   or upper not 16-byte aligned or n_elem % 4 != 0 -> ALIGN; n < 2, n > 1024, n_groups > 65535, k < 1 or k > n / 2 -> SHAPE.
 *
 * Definition, per element of group g.  Its n pooled draws are sorted in torch.sort's order -- ascending, every NaN above
 * +inf -- into d_(1) <= ... <= d_(n).
 *   lower  = d_(k),  upper = d_(n+1-k)
 *   median = d_((n+1)/2) for odd n;  (d_(n/2) + d_(n/2+1)) * 0.5f for even n: one fp32 add and one fp32 multiply, which
 *            is np.median of a float32 array.
 *   Selection is exact: lower and upper are values among the draws, and so is median for odd n.  A NaN that is selected
 *   comes back as a quiet NaN.  -0.0 and +0.0 compare equal and either sign may come back.
 * Summary per group, over its n_elem elements, t being the original's value:
 *     [0] sum_width       = sum ((double)upper - (double)lower)
 *     [1] max_width       = the largest such width
 *     [2] sum_err2_median = sum ((double)t - (double)median)^2
 *     [3] n_inside        = #{lower <= t <= upper}     fp32 comparisons
 *     [4] n_point         = #{upper == lower}
 *     [5] n_nan           = #{upper is NaN}
 *   x_orig == NULL: [2] and [3] are NaN.  NaN is never turned into a number: a NaN width (a NaN bound, or inf - inf) makes
 *   [0] NaN and [1] NaN, so [1] is NaN whenever [5] > 0; [3] and [4] count only what compares true.  What one group holds
 *   never changes a bit of another group's outputs or summary.
 * Reductions: per-tile fp64 partials in ws and a fixed-order second pass by one wave per group; no float atomics, equal
 *   inputs give equal bits.
 * Two kernels, chosen from n, return the same bits: for n <= 64 a sorting network over registers that reads every sample
 *   value once -- n * 4 + 4 bytes per element read, 12 written -- and for larger n a radix select that reads the draws 16
 *   times.  NHMC_CREDIBLE_PATH=general in the environment, read per call, sends every n through the second (register or
 *   unset: the choice above; anything else -> ARG).
 * ---------------------------------------------------------------------------------- */
int nhmc_credible_tiles(int64_t n_elem);
size_t nhmc_credible_ws_bytes(int n_groups, int64_t n_elem);
int nhmc_credible(const float* samples, const float* x_orig, float* lower, float* median, float* upper, double* summary,
                  double* ws, int n_groups, int n_replicas, int n_samples, int64_t n_elem, int k, nhmc_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Principal components of the posterior samples, on the device: the Gram matrix of an image's pooled draws about the
 * first one (the N x N covariance's eigenvectors follow from it on the host, nothing of size N x N is formed), and the
 * projection that turns coefficients over the draws back into images.
 *
 *   samples : fp32 [n_groups * n_replicas][n_samples][n_elem], laid out and pooled as for nhmc_calibration: draw i of
 *             group g is row g * n + i - 1 of the block, n = n_replicas * n_samples.
 *   x_orig  : fp32 [n_groups][n_elem], or NULL.    gram : fp64 [n_groups][n][n].
 *   ws      : double, nhmc_sample_gram_ws_bytes(n_groups, n, n_elem) bytes: one set of 16 x 16 partial tiles for each of
 *             the nhmc_sample_gram_slabs(n_elem) slabs (1024 elements each) of every group.  The slab count is a function
 *             of n_elem alone, never of the device.
 *   Validation, before any launch: null pointer (x_orig excepted) / non-positive size -> ARG; samples, x_orig or gram not
 *   16-byte aligned or n_elem % 4 != 0 -> ALIGN; n < 2, n > 256 or n_groups > 65535 -> SHAPE.
 *
 * Definition, per group, t being the original:
 *   u_i = (double)d_{i+1} - (double)d_1   for i = 1 ... n - 1     the subtraction in fp64: the shift costs no fp32 rounding
 *   u_n = (double)t - (double)d_1
 *   gram[a][b] = sum over the n_elem elements of u_a u_b          a, b = 1 ... n (stored from 0); products and sums in fp64
 *   The matrix is written exactly symmetric: [a][b] and [b][a] hold the same bits.  x_orig == NULL: row and column n - 1
 *   are NaN.  A non-finite draw (NaN or +-inf) makes its own row and column NaN, a non-finite d_1 the whole matrix: it is
 *   never turned into a number.  What one group holds never changes a bit of another group's matrix.
 * Reductions: a workgroup owns one slab of one group, keeps its accumulators in registers over the whole slab and writes
 *   one fp64 partial tile set to ws; a second kernel adds the slabs in ascending order.  No atomics: equal inputs give equal
 *   bits.  The products run on the fp64 MFMA (16 x 16 x 4), so the order of the additions inside a slab is the hardware's.
 * Every sample value and t leave HBM once: n * 4 + 4 bytes per element read.  On top of that the slabs' partial tiles
 *   are written once and read once: nhmc_sample_gram_ws_bytes each way (189 MB at n = 160 and 8 groups of 3 x 256^2
 *   elements, against the 1.0 GB block; 453 MB at n = 256).
 *
 * nhmc_sample_project:  coef : fp64 [n_groups][n_out][n], 1 <= n_out <= 8;  out : fp32 [n_groups][n_out][n_elem]
 *   out[g][j][e] = fp32( sum_{i = 1 ... n} coef[g][j][i] ((double)d_i[e] - (double)d_1[e]) )
 *   explicit fp64 fmas in ascending i from 0, rounded once to fp32.  Every sample value is read once.
 *   Validation as above (samples, coef, out aligned); n_out outside 1 ... 8 -> SHAPE.  The kernel takes one element per
 *   thread and needs neither the alignment nor n_elem % 4 == 0: both are asked for so that whatever nhmc_sample_gram
 *   accepts this entry accepts, and nothing else.
 * ---------------------------------------------------------------------------------- */
int nhmc_sample_gram_slabs(int64_t n_elem);
size_t nhmc_sample_gram_ws_bytes(int n_groups, int n, int64_t n_elem);
int nhmc_sample_gram(const float* samples, const float* x_orig, double* gram, double* ws, int n_groups, int n_replicas,
                     int n_samples, int64_t n_elem, nhmc_stream_t stream);
int nhmc_sample_project(const float* samples, const double* coef, float* out, int n_groups, int n_replicas, int n_samples,
                        int n_out, int64_t n_elem, nhmc_stream_t stream);

/* ------------------------------------------------------------------------------------
 * a1  Momentum / accept noise: Philox4x32-10 keyed by seed, counted by
 *     (element quad, chain_id0 + chain, draw, tag) -- independent of how chains are sharded.
 *     Replaces torch.randn_like (main_sampling.py:692) and torch.rand(1) (:720).
 * ---------------------------------------------------------------------------------- */
int nhmc_randn_philox(float* out, uint64_t seed, uint32_t chain_id0, uint32_t draw, float scale,
                      int n_chains, int64_t n_elem, nhmc_stream_t stream);
int nhmc_uniform_philox(float* out, uint64_t seed, uint32_t chain_id0, uint32_t draw,
                        int n_chains, nhmc_stream_t stream);

/* ------------------------------------------------------------------------------------
 * (d) Measurement aid: a streaming copy dst = src with the access pattern of the fused update (256-thread blocks,
 *     one non-temporal float4 per thread): the "copy ceiling" bench.py quotes beside the 8 TB/s HBM peak
 *     (SURVEY.md section 8d).  n_elem % 4 == 0, 16-byte aligned.
 * ---------------------------------------------------------------------------------- */
int nhmc_copy_probe(const float* src, float* dst, int64_t n_elem, nhmc_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* NHMC_H */
