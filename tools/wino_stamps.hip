// Per-phase timing of k_conv3x3_wino (the Winograd 3x3 convolution): the product kernel file compiled with
// NHMC_WINO_STAMPS, every wave keeping the shader clock (s_memtime) of its phase boundaries in scalar registers and lane 0
// writing them out behind the epilogue.  The constant-rate clock (s_memrealtime, 100 MHz) around the loop gives the
// in-kernel shader clock.
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 -ffp-contract=off tools/wino_stamps.hip -o tools/wino_stamps
//   tools/wino_stamps [n c k h w]        (default: 64 128 128 256 256, then 64 512 256 64 64)
//   NHMC_WINO_WAVES=4|8 chooses the geometry as in the library (k_conv3x3_wino or k_conv3x3_wino8, which keeps the same
//   stamp slots: 8 x 24 values per workgroup)
// Random data; >= 2 s of back-to-back unstamped launches first; then one stamped launch each for the first, the middle and
// the last chunk of every workgroup.  Prints the median over all waves, in shader cycles, per phase, and unit 4, one of the
// four units that stage the following chunk, split at its MFMAs 1, 3, 5 and 7 (reads, arithmetic, V stores, U stores).
#define NHMC_WINO_STAMPS 1
#include "../noise-space-hmc_amd/csrc/wino_conv.hip"

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { std::printf("HIP error %s at line %d\n", hipGetErrorString(e_), __LINE__); return 1; } } while (0)

__global__ void k_fill(float* p, size_t n, unsigned seed, float scale) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    unsigned v = (unsigned)i * 2654435761u + seed;
    v ^= v >> 15; v *= 2246822519u; v ^= v >> 13; v *= 3266489917u; v ^= v >> 16;
    p[i] = ((v >> 8) * (1.0f / 8388608.0f) - 1.0f) * scale;
  }
}

static double median(std::vector<double>& v) {
  std::nth_element(v.begin(), v.begin() + v.size() / 2, v.end());
  return v[v.size() / 2];
}

static int run_shape(int n, int c, int k, int h, int w) {
  if (!wc_covers(n, c, k, h, w)) { std::printf("[%d,%d->%d,%dx%d] is not a shape of the wide geometry\n", n, c, k, h, w); return 1; }
  const size_t nx = (size_t)n * c * h * w, ny = (size_t)n * k * h * w, nw = (size_t)k * c * 9, nu = (size_t)k * c * 16;
  const int chunks = c / WC_CHUNK;
  const int geometry = wc_waves();                    // NHMC_WINO_WAVES, as the library reads it
  if (geometry < 0) { std::printf("NHMC_WINO_WAVES must be 4 or 8\n"); return 1; }
  const size_t waves = (size_t)n * (h / WC_ROWS) * (w / WC_COLS) * (k / WC_KBLK) * geometry;
  float *X, *Wt, *U, *Y;
  unsigned long long* ST;
  CK(hipMalloc(&X, nx * 4)); CK(hipMalloc(&Y, ny * 4)); CK(hipMalloc(&Wt, nw * 4)); CK(hipMalloc(&U, nu * 4));
  CK(hipMalloc(&ST, waves * 24 * 8));
  k_fill<<<4096, 256>>>(X, nx, 1u, 1.0f);
  k_fill<<<256, 256>>>(Wt, nw, 2u, 1.0f / 32.0f);
  CK(hipGetLastError());
  if (nhmc_wino_weights(Wt, U, 0, c, k, nullptr)) { std::printf("nhmc_wino_weights failed\n"); return 1; }
  unsigned long long* none = nullptr;
  CK(hipMemcpyToSymbol(HIP_SYMBOL(nhmc_wino_stamps), &none, sizeof(none)));
  CK(hipDeviceSynchronize());
  int warm = 0;
  const auto t0 = std::chrono::steady_clock::now();
  while (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() < 2.0) {
    for (int it = 0; it < 8; ++it, ++warm)
      if (nhmc_conv3x3_wino(X, U, nullptr, nullptr, Y, n, c, k, h, w, 1, 1, nullptr)) { std::printf("launch failed\n"); return 1; }
    CK(hipDeviceSynchronize());
  }
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
  CK(hipEventRecord(e0, nullptr));
  for (int it = 0; it < 10; ++it)
    if (nhmc_conv3x3_wino(X, U, nullptr, nullptr, Y, n, c, k, h, w, 1, 1, nullptr)) { std::printf("launch failed\n"); return 1; }
  CK(hipEventRecord(e1, nullptr));
  CK(hipEventSynchronize(e1));
  float ms = 0.f;
  CK(hipEventElapsedTime(&ms, e0, e1));
  std::printf("[%d,%d->%d,%dx%d] forward, %d chunks, %zu waves, after %d warm-up launches: %.0f us per launch of the stamped build "
              "(same buffers)\n", n, c, k, h, w, chunks, waves, warm, ms * 100.f);
  const int sel[3] = {0, chunks / 2, chunks - 1};
  const char* sel_name[3] = {"first", "middle", "last"};
  std::vector<unsigned long long> st(waves * 24);
  for (int s = 0; s < 3; ++s) {
    CK(hipMemset(ST, 0, waves * 24 * 8));
    CK(hipMemcpyToSymbol(HIP_SYMBOL(nhmc_wino_stamp_chunk), &sel[s], sizeof(int)));
    CK(hipMemcpyToSymbol(HIP_SYMBOL(nhmc_wino_stamps), &ST, sizeof(ST)));
    if (nhmc_conv3x3_wino(X, U, nullptr, nullptr, Y, n, c, k, h, w, 1, 1, nullptr)) { std::printf("launch failed\n"); return 1; }
    CK(hipDeviceSynchronize());
    CK(hipMemcpyToSymbol(HIP_SYMBOL(nhmc_wino_stamps), &none, sizeof(none)));
    CK(hipMemcpy(st.data(), ST, waves * 24 * 8, hipMemcpyDeviceToHost));
    auto col = [&](auto f) {
      std::vector<double> d(waves);
      for (size_t i = 0; i < waves; ++i) d[i] = f(&st[i * 24]);
      return median(d);
    };
    auto d64 = [&](int a, int b) { return col([=](const unsigned long long* r) { return (double)(long long)(r[b] - r[a]); }); };
    auto d32 = [&](int a, int b) { return col([=](const unsigned long long* r) { return (double)(unsigned)((unsigned)r[7 + b] - (unsigned)r[7 + a]); }); };
    if (s == 0) {
      const double ghz = col([](const unsigned long long* r) { return (double)(r[3] - r[2]) / (double)(r[6] - r[5]) * 0.1; });
      std::printf("   in-kernel shader clock (loop cycles / loop time on the 100 MHz clock): %.3f GHz\n", ghz);
      std::printf("   workgroup, median cycles: prologue %.0f | loop %.0f = %.0f per chunk (64 MFMAs = 4096) | epilogue %.0f | whole %.0f\n",
                  d64(0, 1) + d64(1, 2), d64(2, 3), d64(2, 3) / chunks, d64(3, 4), d64(0, 4));
    }
    if (geometry == 8) {
      // eight waves: a wave's chunk is 4 units of 8 MFMAs; two waves share the pipe, so a unit is 1024 cycles of it.  Stamps 0,
      // 1, 2: the heads of units 0 - 2; 9 / 10 around the barrier; 3 the head of unit 3; 12 the chunk's end; 7 / 8 around the
      // wait for the patch and its exchange, in unit 1
      std::printf("   %-6s chunk (%2d): units 0-2 %.0f %.0f %.0f (to the barrier) | of unit 1, patch wait and exchange %.0f | barrier %.0f | "
                  "unit 3 %.0f | chunk %.0f\n", sel_name[s], sel[s], d32(0, 1), d32(1, 2), d32(2, 9), d32(7, 8), d32(9, 10), d32(3, 12),
                  d32(0, 12));
      continue;
    }
    std::printf("   %-6s chunk (%2d): units 0-6", sel_name[s], sel[s]);
    for (int u = 0; u < 6; ++u) std::printf(" %.0f", d32(u, u + 1));
    std::printf(" %.0f (to the barrier) | of unit 3, patch wait %.0f | barrier %.0f | behind it, to unit 7 %.0f | unit 7 %.0f | chunk %.0f\n",
                d32(6, 9), d32(7, 8), d32(9, 10), d32(10, 11), d32(11, 12), d32(0, 12));
    // a staging unit by its gaps (two MFMAs = 128 cycles each): head of unit 4 -> its MFMA 1 (64) -> 3 -> 5 -> 7
    std::printf("          unit 4 (staging): to MFMA 1, the operand reads %.0f | to MFMA 3, the row differences %.0f | to MFMA 5, the V stores "
                "%.0f | to MFMA 7, the U stores and their waits %.0f\n", d32(4, 13), d32(13, 14), d32(14, 15), d32(15, 16));
  }
  CK(hipFree(X)); CK(hipFree(Y)); CK(hipFree(Wt)); CK(hipFree(U)); CK(hipFree(ST));
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 6) return run_shape(std::atoi(argv[1]), std::atoi(argv[2]), std::atoi(argv[3]), std::atoi(argv[4]), std::atoi(argv[5]));
  if (run_shape(64, 128, 128, 256, 256)) return 1;
  return run_shape(64, 512, 256, 64, 64);
}
