// General 2-D PSF blur (deblur_motion): H, its exact adjoint, and the data term with the last DDIM step's VJP as the
// epilogue of the adjoint pass.  The definition (tap list, correlation form, zero boundary) is in include/nhmc.h.
//
// One workgroup (256 threads, 4 waves) owns a BL_TH x BL_TW = 32 x 64 output tile of one (chain, channel) plane.  It stages
// the (32 + 2R) x (64 + 2R) input patch in LDS (zeros outside the image by predicate; pass 1 clips while staging, pass 2
// scales the residual by -2, which is exact), then every wave walks the tap list for its 8 rows: lane = column, 8 rows in
// registers.  The tap list is staged beside the patch BL_TAPC = 512 taps at a time as (LDS offset, weight); per tap the
// two are read as wave-uniform LDS broadcasts (the scalar path was tried first: s_load and ds_read share one counter, and
// every tap drained both), one address add, then 8 ds_read_b32 on immediate offsets (the LDS row stride is the compile-
// time BL_PW, whatever R is) and 8 fmaf.  The 64 lanes of a read hit 64 consecutive dwords: conflict-free for every (dy, dx).
//
// LDS: ((32 + 2R) * 128 + 1024) * 4 bytes -- 51 KB at R = 31, below the 64 KB that needs no per-function attribute, and
// three workgroups per CU in gfx950's 160 KB.  A 64 x 64 tile would need 67 KB there: the attribute, and two per CU.
// The inner loop moves one LDS dword per FMA: ds_read_b32 runs at 128 B/clk/CU = 32 lanes/clk against the VALU's 64, so
// the LDS read rate is the bound (see DESIGN).
//
// A tap whose offset lies outside [-R, R] would read outside the staged patch; the device arrays cannot be inspected by the
// host entry, so the kernel clamps offsets into the halo while it stages them (no read leaves the patch whatever the list
// holds) and nhmc_blur2d_check_taps rejects such a list on the host copy.
#include "nhmc_common.h"

namespace {

constexpr int BL_TH = 32, BL_TW = 64;          // output tile
constexpr int BL_ROWS = BL_TH / 4;             // rows per wave = accumulators per lane
constexpr int BL_KMAX = 63, BL_RMAX = (BL_KMAX - 1) / 2;
constexpr int BL_PW = 128;                     // LDS row stride in floats
constexpr int BL_TAPC = 512;                   // taps staged in LDS at a time (4 KB)
static_assert(BL_PW >= BL_TW + 2 * BL_RMAX, "a patch row must hold the tile and both halos");
static_assert(((BL_TH + 2 * BL_RMAX) * BL_PW + 2 * BL_TAPC) * sizeof(float) <= 65536, "the patch stays below the 64 KB static limit");

enum { BL_APPLY = 0, BL_RESID = 1, BL_GRAD = 2, BL_VJP = 3 };

struct BlurVjp {
  const float* e;
  float* g_e;
  const float* at;
  const float* at_next;
  int e_channels, fill_sigma;
};

// src   : the plane set that is blurred (x; xt / xt_next; the residual in `tmp`)
// sign  : +1 H, -1 H^T (the same list, offsets negated)
// BL_APPLY: out = blur(src)
// BL_RESID: out = y - blur(clip? src), loss partial of its squares
// BL_GRAD : out = blur(-2 src) [masked by 1[|aux| <= 1] when aux]         (aux = xt)
// BL_VJP  : (out, g_e) = nhmc_mix_vjp(blur(-2 src), aux, e)               (aux = xt, the last step's input)
template <int MODE>
__global__ __launch_bounds__(NHMC_BLOCK) void k_blur2d(
    const float* __restrict__ src, const int2* __restrict__ taps_off, const float* __restrict__ taps_w, int n_taps, int R,
    int sign, int clip, const float* __restrict__ y, const float* __restrict__ aux, float* __restrict__ out,
    double* __restrict__ loss_ws, BlurVjp vjp, int dim, int tiles_x) {
  extern __shared__ float patch[];             // [(BL_TH + 2R)][BL_PW]
  const int lane = threadIdx.x & (NHMC_WAVE - 1), wave = threadIdx.x >> 6;
  const int tile = blockIdx.x, ch = blockIdx.y, chain = blockIdx.z, C = gridDim.y;
  const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
  const int r0 = ty * BL_TH, c0 = tx * BL_TW;
  const int hw = dim * dim;
  const int64_t plane = ((int64_t)chain * C + ch) * hw;
  const float* __restrict__ sp = src + plane;

  const int ph = BL_TH + 2 * R, pw = BL_TW + 2 * R;
  for (int pr = wave; pr < ph; pr += 4) {
    const int r = r0 + pr - R;
    const bool row_in = r >= 0 && r < dim;
    for (int pc = lane; pc < pw; pc += NHMC_WAVE) {
      const int c = c0 + pc - R;
      float v = 0.0f;
      if (row_in && c >= 0 && c < dim) {
        v = sp[r * dim + c];
        if (MODE == BL_RESID) { if (clip) v = nhmc_clip1(v); }
        if (MODE == BL_GRAD || MODE == BL_VJP) v = -(2.0f * v);
      }
      patch[pr * BL_PW + pc] = v;
    }
  }

  float acc[BL_ROWS];
#pragma unroll
  for (int i = 0; i < BL_ROWS; ++i) acc[i] = 0.0f;
  int* __restrict__ s_off = reinterpret_cast<int*>(patch + ph * BL_PW);          // [BL_TAPC] LDS offset of the tap
  float* __restrict__ s_w = reinterpret_cast<float*>(s_off + BL_TAPC);           // [BL_TAPC] its weight
  const float* base = patch + (wave * BL_ROWS + R) * BL_PW + lane + R;
  for (int t0 = 0; t0 < n_taps; t0 += BL_TAPC) {
    const int n = min(BL_TAPC, n_taps - t0);
    if (t0) __syncthreads();                                 // the previous chunk has been read by every wave
    for (int t = threadIdx.x; t < n; t += NHMC_BLOCK) {
      const int2 o = taps_off[t0 + t];                       // x = dy, y = dx; clamped into the staged halo
      s_off[t] = sign * (min(max(o.x, -R), R) * BL_PW + min(max(o.y, -R), R));
      s_w[t] = taps_w[t0 + t];
    }
    __syncthreads();                                         // (the first one also publishes the patch)
#pragma unroll 4
    for (int t = 0; t < n; ++t) {
      const float* p = base + s_off[t];                      // wave-uniform LDS reads: broadcasts
      const float w = s_w[t];
#pragma unroll
      for (int i = 0; i < BL_ROWS; ++i) acc[i] = fmaf(w, p[i * BL_PW], acc[i]);
    }
  }

  const int col = c0 + lane;
  const bool col_in = col < dim;
  double sq = 0.0;                                           // fp32 squares summed in fp64, as the other data terms
  NhmcMix k;
  if (MODE == BL_VJP) k = nhmc_mix_coef(vjp.at, vjp.at_next, chain);
#pragma unroll
  for (int i = 0; i < BL_ROWS; ++i) {
    const int row = r0 + wave * BL_ROWS + i;
    if (!col_in || row >= dim) continue;
    const int pix = row * dim + col;
    if (MODE == BL_APPLY) {
      out[plane + pix] = acc[i];
    } else if (MODE == BL_RESID) {
      const float r = y[plane + pix] - acc[i];
      sq += (double)(r * r);
      out[plane + pix] = r;
    } else if (MODE == BL_GRAD) {
      out[plane + pix] = aux ? nhmc_masked(acc[i], nhmc_in1(aux[plane + pix])) : acc[i];
    } else {
      const int64_t eo = ((int64_t)chain * vjp.e_channels + ch) * hw + pix;
      float gx, ge;
      nhmc_mix_vjp(k, acc[i], aux[plane + pix], vjp.e[eo], gx, ge);
      out[plane + pix] = gx;
      vjp.g_e[eo] = ge;
      if (vjp.fill_sigma && vjp.e_channels > C) vjp.g_e[eo + (int64_t)C * hw] = 0.0f;      // learned-sigma half
    }
  }
  if (MODE == BL_RESID) {
    __shared__ double red[4];
    double v[1] = {sq};
    nhmc_block_sum<1>(v, red);
    if (threadIdx.x == 0) loss_ws[((int64_t)chain * C + ch) * gridDim.x + tile] = v[0];
  }
}

struct BlurGeom { int R, tiles_x, tiles; size_t lds; };

int blur_tiles_1d(int dim, int t) { return (dim + t - 1) / t; }

// NHMC_OK, or the code the entries return for a shape they do not cover.
int blur_geom(int n_taps, int ksize, int n_chains, int channels, int dim, BlurGeom& g) {
  if (ksize < 1 || ksize > BL_KMAX || !(ksize & 1) || n_taps < 1 || n_taps > ksize * ksize) return NHMC_ERR_SHAPE;
  if (n_chains <= 0 || n_chains > 65535 || channels <= 0 || channels > 65535 || dim <= 0 || dim > 32768) return NHMC_ERR_SHAPE;
  if (dim & 3) return NHMC_ERR_ALIGN;
  g.R = (ksize - 1) / 2;
  g.tiles_x = blur_tiles_1d(dim, BL_TW);
  g.tiles = g.tiles_x * blur_tiles_1d(dim, BL_TH);
  g.lds = ((size_t)(BL_TH + 2 * g.R) * BL_PW + 2 * BL_TAPC) * sizeof(float);
  return NHMC_OK;
}

template <int MODE>
int blur_launch(const float* src, const int32_t* taps_off, const float* taps_w, int n_taps, const BlurGeom& g, int sign,
                int clip, const float* y, const float* aux, float* out, double* loss_ws, const BlurVjp& vjp, int n_chains,
                int channels, int dim, nhmc_stream_t stream) {
  dim3 grid((unsigned)g.tiles, (unsigned)channels, (unsigned)n_chains);
  NHMC_LAUNCH(k_blur2d<MODE>, grid, dim3(NHMC_BLOCK), g.lds, nhmc_s(stream), src, (const int2*)taps_off, taps_w, n_taps,
              g.R, sign, clip, y, aux, out, loss_ws, vjp, dim, g.tiles_x);
  return nhmc_launch_status();
}

}  // namespace

extern "C" int nhmc_blur2d_check_taps(const int32_t* host_off, int n_taps, int ksize) {
  if (!host_off) return NHMC_ERR_ARG;
  if (ksize < 1 || ksize > BL_KMAX || !(ksize & 1) || n_taps < 1 || n_taps > ksize * ksize) return NHMC_ERR_SHAPE;
  const int R = (ksize - 1) / 2;
  for (int t = 0; t < 2 * n_taps; ++t)
    if (host_off[t] < -R || host_off[t] > R) return NHMC_ERR_SHAPE;
  return NHMC_OK;
}

extern "C" int nhmc_blur2d_tiles(int channels, int dim) {
  return channels * blur_tiles_1d(dim, BL_TW) * blur_tiles_1d(dim, BL_TH);
}

extern "C" int nhmc_blur2d_apply(const float* x, const int32_t* taps_off, const float* taps_w, int n_taps, int ksize,
                                 int transpose, float* out, int n_chains, int channels, int dim, nhmc_stream_t stream) {
  if (!x || !taps_off || !taps_w || !out || x == out) return NHMC_ERR_ARG;
  BlurGeom g;
  if (const int rc = blur_geom(n_taps, ksize, n_chains, channels, dim, g)) return rc;
  if (!nhmc_aligned16(x) || !nhmc_aligned16(out) || (reinterpret_cast<uintptr_t>(taps_off) & 7u)) return NHMC_ERR_ALIGN;
  return blur_launch<BL_APPLY>(x, taps_off, taps_w, n_taps, g, transpose ? -1 : 1, 0, nullptr, nullptr, out, nullptr,
                               BlurVjp{}, n_chains, channels, dim, stream);
}

extern "C" int nhmc_data_blur2d(const float* xt, const float* y, const int32_t* taps_off, const float* taps_w, int n_taps,
                                int ksize, int apply_clip, float* g_xt, double* loss_ws, float* tmp, int n_chains,
                                int channels, int dim, nhmc_stream_t stream) {
  if (!xt || !y || !taps_off || !taps_w || !g_xt || !loss_ws || !tmp || tmp == g_xt || tmp == xt) return NHMC_ERR_ARG;
  BlurGeom g;
  if (const int rc = blur_geom(n_taps, ksize, n_chains, channels, dim, g)) return rc;
  if (!nhmc_aligned16(xt) || !nhmc_aligned16(y) || !nhmc_aligned16(g_xt) || !nhmc_aligned16(tmp) ||
      (reinterpret_cast<uintptr_t>(taps_off) & 7u))
    return NHMC_ERR_ALIGN;
  if (const int rc = blur_launch<BL_RESID>(xt, taps_off, taps_w, n_taps, g, 1, apply_clip != 0, y, nullptr, tmp, loss_ws,
                                           BlurVjp{}, n_chains, channels, dim, stream))
    return rc;
  return blur_launch<BL_GRAD>(tmp, taps_off, taps_w, n_taps, g, -1, 0, nullptr, apply_clip ? xt : nullptr, g_xt, nullptr,
                              BlurVjp{}, n_chains, channels, dim, stream);
}

extern "C" int nhmc_data_blur2d_vjp(const float* xt_next, const float* y, const int32_t* taps_off, const float* taps_w,
                                    int n_taps, int ksize, const float* xt_in, const float* e, int e_channels,
                                    const float* at, const float* at_next, float* g_xt, float* g_e, int fill_sigma,
                                    double* loss_ws, float* tmp, int n_chains, int channels, int dim,
                                    nhmc_stream_t stream) {
  if (!xt_next || !y || !taps_off || !taps_w || !xt_in || !e || !at || !at_next || !g_xt || !g_e || !loss_ws || !tmp ||
      tmp == g_xt || tmp == xt_next)
    return NHMC_ERR_ARG;
  BlurGeom g;
  if (const int rc = blur_geom(n_taps, ksize, n_chains, channels, dim, g)) return rc;
  if (e_channels != channels && e_channels != 2 * channels) return NHMC_ERR_SHAPE;
  if (!nhmc_aligned16(xt_next) || !nhmc_aligned16(y) || !nhmc_aligned16(xt_in) || !nhmc_aligned16(e) ||
      !nhmc_aligned16(g_xt) || !nhmc_aligned16(g_e) || !nhmc_aligned16(tmp) || (reinterpret_cast<uintptr_t>(taps_off) & 7u))
    return NHMC_ERR_ALIGN;
  if (const int rc = blur_launch<BL_RESID>(xt_next, taps_off, taps_w, n_taps, g, 1, 0, y, nullptr, tmp, loss_ws, BlurVjp{},
                                           n_chains, channels, dim, stream))
    return rc;
  const BlurVjp vjp{e, g_e, at, at_next, e_channels, fill_sigma};
  return blur_launch<BL_VJP>(tmp, taps_off, taps_w, n_taps, g, -1, 0, nullptr, xt_in, g_xt, nullptr, vjp, n_chains,
                             channels, dim, stream);
}
