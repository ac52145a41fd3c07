// Direct (non-Winograd) 3x3 stride-1 padding-1 convolution from a THIN input to a wide output, NCHW fp32: the score
// network's first layer (3 -> 128, with its bias in the store) and the backward-data pass of its last one (6 -> 128: the
// flipped, transposed filter, built by nhmc_thin_in_weights, through the same kernel).
//
//   y[n,k,h,w] = sum_c sum_rs x[n,c,h+r-1,w+s-1] g[k,c,r,s] (+ bias[k])      c < CT <= 8, K a multiple of 32
//
// The pass is store-bound: the input is CT / K of the output's bytes, so the floor is one crossing of y.  A lane owns four adjacent pixels of one image row.  It loads their 3 x 6 halo patch of every
// input channel once, straight into registers (zero padding by predicate; the input is thin, its re-reads by the rows above
// and below are served by the caches and are 3 * CT / K of the store traffic at most), then walks over the output channels
// two at a time: the 9 CT taps of a channel pair sit interleaved in the re-laid-out filter wp[K / 2][9 CT][2], at a
// wave-uniform address, so they arrive by scalar loads and every v_pk_fma_f32 takes one pixel (broadcast) against the
// (k, k + 1) weight pair from scalar registers: no LDS, no exchange, no register shuffles, 9 CT * 4 packed FMAs per pair of
// float4 stores.  A wave stores 1 KB of one output row per channel where the row is at least 256 pixels long.
// Arithmetic: 9 CT * K FMAs per pixel on packed FMA is 0.19 ms (3 -> 128) and 0.37 ms (6 -> 128) at 64 x 256 x 256 against
// a store floor of 0.4 ms; plain v_fma_f32 would be twice that and bound the second.  The fp32 matrix cores have the same
// peak as packed FMA and would need the im2col operand staged through LDS.
// Summation: one FMA chain per output, c ascending, then r, then s, bias added last; no atomics, two runs give the same bits.
//
// THIN OUTPUT (k_conv3x3_thin_out, nhmc_conv3x3_thin_out): the network's last layer (128 -> 6, with its bias) and the
// backward-data pass of its first one (128 -> 3).  The pass is read-bound: the floor is one crossing of x.  The same lane
// geometry: four adjacent pixels of a row per lane, which keeps their KT <= 8 running sums (as KT / 2 channel pairs) in
// registers and walks over the input channels, loading the 3 x 6 halo patch of one channel at a time (three 16-byte loads
// and six edge dwords that hit the lines its neighbours load; zero padding by predicate) against the 9 taps x KT weights of
// that channel from scalar registers (gp[C][9][2 ceil(KT / 2)], an odd KT padded with a zero channel that is never
// stored).  Rows h - 1 and h + 1 are loaded again by the lanes of those rows: a workgroup of 256 lanes covers whole
// neighbouring rows, so the re-reads meet in the caches and x crosses HBM about once.  9 * 4 * ceil(KT / 2) packed FMAs
// per channel; c ascending, then r, then s, the bias added last; no atomics.
#include "nhmc_common.h"

namespace {

typedef float tc_v2f __attribute__((ext_vector_type(2)));
typedef const __attribute__((address_space(4))) float* tc_cptr;      // read-only for the kernel's lifetime: scalar loads

template <int CT>
__global__ __launch_bounds__(NHMC_BLOCK) void k_conv3x3_thin_in(const float* __restrict__ x, const float* wp, const float* bias,
                                                                float* __restrict__ y, int K, int H, int W, int64_t items) {
  const int64_t item = (int64_t)blockIdx.x * NHMC_BLOCK + threadIdx.x;
  if (item >= items) return;
  const int W4 = W >> 2;
  const int w0 = (int)(item % W4) * 4;
  const int64_t t = item / W4;
  const int h = (int)(t % H);
  const int64_t n = t / H, HW = (int64_t)H * W;
  const float* xn = x + n * CT * HW + w0;
  const bool left = w0 > 0, right = w0 + 4 < W;
  float p[CT][3][6];
#pragma unroll
  for (int c = 0; c < CT; ++c)
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      const int hh = h + r - 1;
      const bool rok = (unsigned)hh < (unsigned)H;
      const float* row = xn + c * HW + (int64_t)(rok ? hh : h) * W;          // a row of the image whatever rok is
      const nhmc_v4f m = *reinterpret_cast<const nhmc_v4f*>(row);
      const float l = row[left ? -1 : 0], rr = row[right ? 4 : 3];
      p[c][r][0] = rok && left ? l : 0.0f;
      p[c][r][1] = rok ? m.x : 0.0f; p[c][r][2] = rok ? m.y : 0.0f; p[c][r][3] = rok ? m.z : 0.0f; p[c][r][4] = rok ? m.w : 0.0f;
      p[c][r][5] = rok && right ? rr : 0.0f;
    }
  float* yp = y + (n * K * H + h) * W + w0;
  const tc_cptr wc = (tc_cptr)(uintptr_t)wp, bc = (tc_cptr)(uintptr_t)bias;
  for (int kp = 0; kp < (K >> 1); ++kp) {
    const tc_cptr wk = wc + (int64_t)kp * (18 * CT);
    tc_v2f acc[4] = {{0.0f, 0.0f}, {0.0f, 0.0f}, {0.0f, 0.0f}, {0.0f, 0.0f}};
#pragma unroll
    for (int c = 0; c < CT; ++c)
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int s = 0; s < 3; ++s) {
          const int tap = (c * 3 + r) * 3 + s;
          const tc_v2f wv = {wk[2 * tap], wk[2 * tap + 1]};
#pragma unroll
          for (int px = 0; px < 4; ++px)
            acc[px] = __builtin_elementwise_fma(tc_v2f{p[c][r][px + s], p[c][r][px + s]}, wv, acc[px]);
        }
    const float b0 = bias ? bc[2 * kp] : 0.0f, b1 = bias ? bc[2 * kp + 1] : 0.0f;
    nhmc_v4f o0 = {acc[0].x, acc[1].x, acc[2].x, acc[3].x}, o1 = {acc[0].y, acc[1].y, acc[2].y, acc[3].y};
    if (bias) { o0 += b0; o1 += b1; }
    __builtin_nontemporal_store(o0, reinterpret_cast<nhmc_v4f*>(yp + (int64_t)(2 * kp) * HW));
    __builtin_nontemporal_store(o1, reinterpret_cast<nhmc_v4f*>(yp + (int64_t)(2 * kp + 1) * HW));
  }
}

template <int KT>
__global__ __launch_bounds__(NHMC_BLOCK) void k_conv3x3_thin_out(const float* __restrict__ x, const float* gp, const float* bias,
                                                                 float* __restrict__ y, int C, int H, int W, int64_t items) {
  constexpr int KP = (KT + 1) / 2;
  const int64_t item = (int64_t)blockIdx.x * NHMC_BLOCK + threadIdx.x;
  if (item >= items) return;
  const int W4 = W >> 2;
  const int w0 = (int)(item % W4) * 4;
  const int64_t t = item / W4;
  const int h = (int)(t % H);
  const int64_t n = t / H, HW = (int64_t)H * W;
  const bool left = w0 > 0, right = w0 + 4 < W;
  bool rok[3];
  const float* row[3];                                               // rows h - 1, h, h + 1 of channel 0: a row of the image whatever rok is
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const int hh = h + r - 1;
    rok[r] = (unsigned)hh < (unsigned)H;
    row[r] = x + n * C * HW + (int64_t)(rok[r] ? hh : h) * W + w0;
  }
  const tc_cptr gc = (tc_cptr)(uintptr_t)gp, bc = (tc_cptr)(uintptr_t)bias;
  tc_v2f acc[KP][4];
#pragma unroll
  for (int q = 0; q < KP; ++q)
#pragma unroll
    for (int px = 0; px < 4; ++px) acc[q][px] = tc_v2f{0.0f, 0.0f};
  for (int c = 0; c < C; ++c) {
    const tc_cptr gk = gc + (int64_t)c * (18 * KP);
    float p[3][6];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      const float* src = row[r] + c * HW;
      const nhmc_v4f m = *reinterpret_cast<const nhmc_v4f*>(src);
      const float l = src[left ? -1 : 0], rr = src[right ? 4 : 3];
      p[r][0] = rok[r] && left ? l : 0.0f;
      p[r][1] = rok[r] ? m.x : 0.0f; p[r][2] = rok[r] ? m.y : 0.0f; p[r][3] = rok[r] ? m.z : 0.0f; p[r][4] = rok[r] ? m.w : 0.0f;
      p[r][5] = rok[r] && right ? rr : 0.0f;
    }
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int s = 0; s < 3; ++s)
#pragma unroll
        for (int q = 0; q < KP; ++q) {
          const tc_v2f gv = {gk[((r * 3 + s) * KP + q) * 2], gk[((r * 3 + s) * KP + q) * 2 + 1]};
#pragma unroll
          for (int px = 0; px < 4; ++px)
            acc[q][px] = __builtin_elementwise_fma(tc_v2f{p[r][px + s], p[r][px + s]}, gv, acc[q][px]);
        }
  }
  float* yp = y + (n * KT * H + h) * W + w0;
#pragma unroll
  for (int k = 0; k < KT; ++k) {
    nhmc_v4f o = (k & 1) ? nhmc_v4f{acc[k >> 1][0].y, acc[k >> 1][1].y, acc[k >> 1][2].y, acc[k >> 1][3].y}
                         : nhmc_v4f{acc[k >> 1][0].x, acc[k >> 1][1].x, acc[k >> 1][2].x, acc[k >> 1][3].x};
    if (bias) o += bc[k];
    __builtin_nontemporal_store(o, reinterpret_cast<nhmc_v4f*>(yp + k * HW));
  }
}

// wp[ko / 2][ci * 9 + r * 3 + s][ko % 2] = g[ko][ci][r][s], ko < wide, ci < thin.
// forward: g = weight [wide][thin][3][3];  backward-data: weight is [thin][wide][3][3] and g[ko][ci][r][s] = weight[ci][ko][2 - r][2 - s].
__global__ __launch_bounds__(NHMC_BLOCK) void k_thin_in_weights(const float* __restrict__ w, float* __restrict__ wp, int thin, int wide,
                                                                int backward) {
  const int idx = blockIdx.x * NHMC_BLOCK + threadIdx.x;
  if (idx >= thin * wide * 9) return;
  const int rs = idx % 9, ci = (idx / 9) % thin, ko = idx / (9 * thin);
  const float v = backward ? w[((int64_t)ci * wide + ko) * 9 + (8 - rs)] : w[((int64_t)ko * thin + ci) * 9 + rs];
  wp[((int64_t)(ko >> 1) * (9 * thin) + ci * 9 + rs) * 2 + (ko & 1)] = v;
}

// gp[ci][r * 3 + s][2 ceil(thin / 2)] = g[ko][ci][r][s], ko < thin, ci < wide; the entry of a padding channel ko = thin is 0.
// forward: g = weight [thin][wide][3][3];  backward-data: weight is [wide][thin][3][3] and g[ko][ci][r][s] = weight[ci][ko][2 - r][2 - s].
__global__ __launch_bounds__(NHMC_BLOCK) void k_thin_out_weights(const float* __restrict__ w, float* __restrict__ gp, int thin, int wide,
                                                                 int backward) {
  const int kpad = (thin + 1) & ~1;
  const int idx = blockIdx.x * NHMC_BLOCK + threadIdx.x;
  if (idx >= wide * 9 * kpad) return;
  const int ko = idx % kpad, rs = (idx / kpad) % 9, ci = idx / (9 * kpad);
  float v = 0.0f;
  if (ko < thin) v = backward ? w[((int64_t)ci * thin + ko) * 9 + (8 - rs)] : w[((int64_t)ko * wide + ci) * 9 + rs];
  gp[idx] = v;
}

int tc_out_covers(int64_t n, int64_t c, int64_t k, int64_t h, int64_t w) {
  if (n <= 0 || k < 1 || k > 8 || c < 32 || c % 32 || h < 1 || w < 4 || w % 4) return 0;
  if (c > 65536 || h * w > (1 << 24)) return 0;
  return (n * h * (w / 4) + NHMC_BLOCK - 1) / NHMC_BLOCK < (int64_t)1 << 31;
}

template <int KT>
int tc_out_launch(const float* x, const float* gp, const float* bias, float* y, int n, int c, int h, int w, nhmc_stream_t stream) {
  const int64_t items = (int64_t)n * h * (w / 4);
  NHMC_LAUNCH(k_conv3x3_thin_out<KT>, dim3((unsigned)((items + NHMC_BLOCK - 1) / NHMC_BLOCK)), dim3(NHMC_BLOCK), 0, nhmc_s(stream), x,
              gp, bias, y, c, h, w, items);
  return nhmc_launch_status();
}

int tc_in_covers(int64_t n, int64_t c, int64_t k, int64_t h, int64_t w) {
  if (n <= 0 || c < 1 || c > 8 || k < 32 || k % 32 || h < 1 || w < 4 || w % 4) return 0;
  if (k > 65536 || h * w > (1 << 24)) return 0;
  return (n * h * (w / 4) + NHMC_BLOCK - 1) / NHMC_BLOCK < (int64_t)1 << 31;
}

template <int CT>
int tc_in_launch(const float* x, const float* wp, const float* bias, float* y, int n, int k, int h, int w, nhmc_stream_t stream) {
  const int64_t items = (int64_t)n * h * (w / 4);
  NHMC_LAUNCH(k_conv3x3_thin_in<CT>, dim3((unsigned)((items + NHMC_BLOCK - 1) / NHMC_BLOCK)), dim3(NHMC_BLOCK), 0, nhmc_s(stream), x,
              wp, bias, y, k, h, w, items);
  return nhmc_launch_status();
}

}  // namespace

extern "C" int nhmc_conv3x3_thin_in_covers(int n, int c, int k, int h, int w) { return tc_in_covers(n, c, k, h, w); }

// Routing rule, as nhmc_conv3x3_wino_prefers': a (shape, direction) pair is listed only where tools/thin_conv_bench.py
// measured this kernel at <= 0.90 of the vendor sequence's time at 64 chains on MI355X in the same process
// (profiles/r19_thin_conv.txt).  backward = 0: F.conv2d with its bias; backward = 1: conv2d_input.
extern "C" int nhmc_conv3x3_thin_in_prefers(int backward, int n, int c, int k, int h, int w) {
  if (!tc_in_covers(n, c, k, h, w) || h != w) return 0;
  struct Row { int backward, c, k, res; };
  static const Row network[] = {
      {0, 3, 128, 256},   // input_blocks[0] forward, with bias: 0.290
      {1, 6, 128, 256},   // out[2] backward-data: 0.453
  };
  for (const Row& r : network)
    if (r.backward == (backward != 0) && r.c == c && r.k == k && r.res == h) return 1;
  return 0;
}

extern "C" int nhmc_thin_in_weights(const float* weight, float* wp, int backward, int thin, int wide, nhmc_stream_t stream) {
  if (!weight || !wp || weight == wp || (backward != 0 && backward != 1)) return NHMC_ERR_ARG;
  if (thin < 1 || thin > 8 || wide < 32 || wide % 32 || wide > 65536) return NHMC_ERR_SHAPE;
  if (!nhmc_aligned16(wp)) return NHMC_ERR_ALIGN;
  const int total = thin * wide * 9;
  NHMC_LAUNCH(k_thin_in_weights, dim3((unsigned)((total + NHMC_BLOCK - 1) / NHMC_BLOCK)), dim3(NHMC_BLOCK), 0, nhmc_s(stream), weight,
              wp, thin, wide, backward);
  return nhmc_launch_status();
}

extern "C" int nhmc_conv3x3_thin_in(const float* x, const float* wp, const float* bias, float* y, int n, int c, int k, int h, int w,
                                    int stride, int padding, nhmc_stream_t stream) {
  if (!x || !wp || !y || y == x || y == wp) return NHMC_ERR_ARG;
  if (stride != 1 || padding != 1 || !tc_in_covers(n, c, k, h, w)) return NHMC_ERR_SHAPE;
  if (!nhmc_aligned16(x) || !nhmc_aligned16(wp) || !nhmc_aligned16(y)) return NHMC_ERR_ALIGN;
  switch (c) {
    case 1: return tc_in_launch<1>(x, wp, bias, y, n, k, h, w, stream);
    case 2: return tc_in_launch<2>(x, wp, bias, y, n, k, h, w, stream);
    case 3: return tc_in_launch<3>(x, wp, bias, y, n, k, h, w, stream);
    case 4: return tc_in_launch<4>(x, wp, bias, y, n, k, h, w, stream);
    case 5: return tc_in_launch<5>(x, wp, bias, y, n, k, h, w, stream);
    case 6: return tc_in_launch<6>(x, wp, bias, y, n, k, h, w, stream);
    case 7: return tc_in_launch<7>(x, wp, bias, y, n, k, h, w, stream);
    default: return tc_in_launch<8>(x, wp, bias, y, n, k, h, w, stream);
  }
}

extern "C" int nhmc_conv3x3_thin_out_covers(int n, int c, int k, int h, int w) { return tc_out_covers(n, c, k, h, w); }

// The same rule for the thin-output kernel.  backward = 0: F.conv2d with its bias; backward = 1: conv2d_input.
extern "C" int nhmc_conv3x3_thin_out_prefers(int backward, int n, int c, int k, int h, int w) {
  if (!tc_out_covers(n, c, k, h, w) || h != w) return 0;
  struct Row { int backward, c, k, res; };
  static const Row network[] = {
      {0, 128, 6, 256},   // out[2] forward, with bias: 0.417
      {1, 128, 3, 256},   // input_blocks[0] backward-data: 0.603
  };
  for (const Row& r : network)
    if (r.backward == (backward != 0) && r.c == c && r.k == k && r.res == h) return 1;
  return 0;
}

extern "C" int nhmc_thin_out_weights(const float* weight, float* gp, int backward, int thin, int wide, nhmc_stream_t stream) {
  if (!weight || !gp || weight == gp || (backward != 0 && backward != 1)) return NHMC_ERR_ARG;
  if (thin < 1 || thin > 8 || wide < 32 || wide % 32 || wide > 65536) return NHMC_ERR_SHAPE;
  if (!nhmc_aligned16(gp)) return NHMC_ERR_ALIGN;
  const int total = wide * 9 * ((thin + 1) & ~1);
  NHMC_LAUNCH(k_thin_out_weights, dim3((unsigned)((total + NHMC_BLOCK - 1) / NHMC_BLOCK)), dim3(NHMC_BLOCK), 0, nhmc_s(stream), weight,
              gp, thin, wide, backward);
  return nhmc_launch_status();
}

extern "C" int nhmc_conv3x3_thin_out(const float* x, const float* gp, const float* bias, float* y, int n, int c, int k, int h, int w,
                                     int stride, int padding, nhmc_stream_t stream) {
  if (!x || !gp || !y || y == x || y == gp) return NHMC_ERR_ARG;
  if (stride != 1 || padding != 1 || !tc_out_covers(n, c, k, h, w)) return NHMC_ERR_SHAPE;
  if (!nhmc_aligned16(x) || !nhmc_aligned16(gp) || !nhmc_aligned16(y)) return NHMC_ERR_ALIGN;
  switch (k) {
    case 1: return tc_out_launch<1>(x, gp, bias, y, n, c, h, w, stream);
    case 2: return tc_out_launch<2>(x, gp, bias, y, n, c, h, w, stream);
    case 3: return tc_out_launch<3>(x, gp, bias, y, n, c, h, w, stream);
    case 4: return tc_out_launch<4>(x, gp, bias, y, n, c, h, w, stream);
    case 5: return tc_out_launch<5>(x, gp, bias, y, n, c, h, w, stream);
    case 6: return tc_out_launch<6>(x, gp, bias, y, n, c, h, w, stream);
    case 7: return tc_out_launch<7>(x, gp, bias, y, n, c, h, w, stream);
    default: return tc_out_launch<8>(x, gp, bias, y, n, c, h, w, stream);
  }
}
