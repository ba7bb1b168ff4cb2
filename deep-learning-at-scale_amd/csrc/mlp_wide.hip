// wellflow — fused scoring forward of the F -> 256 -> 256 -> 1 MLP for WIDE inputs: 8 <= Fp <= 512
// padded features (the engine routes 64 < Fp <= 512 here; mlp_fused.hip serves Fp <= 64).
//
// Why: past 64 features NativeMLP.forward ran two generic GEMM launches and head_fwd, with H1
// and H2 ([B][256] bf16 each) written to HBM and read back: ~2.3 KB per row at Fp = 128 where
// the input itself is 256 B. A table with one real categorical column is past 64 features, and
// every scoring job (predict, importance, response, explain, setpoint, interval) is a loop of
// these forwards. Here ONE launch reads X once and writes 4 B of prediction per row.
//
// Why not a third KT1 instantiation of mlp2_fwd_kernel: that kernel keeps the wave's W1 slice
// in registers (64 KB per wave at Fp = 512) and stages the whole X tile in LDS (128 KB at
// 128 rows x 512 features). Layer 1 is a real K loop here, both operands streaming.
//
// Split: one workgroup of 512 threads (8 waves, two per SIMD) per CU, grid-stride over
// 128-row tiles (kMlpWideRows). Wave w owns hidden units [32w, 32w + 32) of BOTH layers and
// all 128 rows: 2 M tiles x 8 N tiles of v_mfma_f32_16x16x32_bf16, transposed products as in
// mlp_fused.hip (A = weights, lane = unit; B = activations, lane = row), so a lane's result
// is 4 consecutive units of one row. 128 rows: a K step's W1 fragments (16 KB per workgroup,
// from L2) serve 8 KB of X — at 64 rows L2 would carry 4 B of W1 per byte of X.
//
// Data movement per tile:
//  * X: K slabs of 128 rows x 32 features (8 KB: one 16-B load per thread), global -> register
//    ring (4 slabs in flight per thread) -> 2-slot LDS ring -> B fragments. Slab k + 1 is
//    written to LDS during step k, slab k + 5 is requested during step k; one barrier per
//    step. Rows >= B and features >= Fp are zero-filled in registers, never loaded.
//  * W1: the A fragments of a K step (2 x 16 B per lane) arrive from L2 in a 4-deep register
//    ring, requested four steps ahead; with Fp <= 128 the ring holds all of W1 and it is
//    loaded once per launch. K-tail fragments are zero-filled.
//  * W2: stationary, 2 x 8 fragments = 64 VGPRs per lane, loaded once.
//  * H1 = bf16(relu(acc + b1)) exists only as the [128][256] LDS tile in mlp_tiles.h's swizzled
//    tile_off image; layer 2 reads it as 16-B B fragments.
//  * H2 has no tile at all: bf16(relu(acc + b2)) is multiplied by w3 in the accumulators'
//    lanes; only the per-row head partials (8 waves x 128 rows fp32) cross waves through LDS.
//  * the next tile's first four slabs (and W1 steps, when Fp > 128) are requested before the
//    layer-1 epilogue, so they fly under layer 2.
// Nothing is written but pred[0 .. B); no atomics, no scratch buffer. A row's arithmetic
// (k order, unit order, wave order of the head sum) does not depend on its tile, its position
// in the tile or B: predictions are row-independent bit for bit.
//
// Budget: LDS 64 KB H1 tile + 16 KB X ring + 4 KB head partials + 3 KB b1 / b2 / w3 = 87 KB of
// the CU's 160 KB. Registers per lane: 64 accumulators, 64 W2, 32 W1 ring, 16 X ring, the B
// fragments of a step; the compiler's report is in profiles/r8/mlp_wide_forward/README.md
// (no scratch). _build.py SOURCE_FLAGS compiles this file with the packed fp32 VALU forms
// (v_pk_add / mul / fma_f32) switched off: the bit-for-bit contract above must not hang on
// them; the current compiler emits none with or without the flag (same resource report).
#include "common.h"
#include "kernels.h"
#include "mlp_tiles.h"

namespace wf {

namespace {
constexpr int MW_ROWS = kMlpWideRows;  // rows per tile
constexpr int MW_NT = MW_ROWS / 16;    // N tiles (16 rows) per wave
constexpr int MW_THREADS = 512;
constexpr int MW_WAVES = MW_THREADS / kWave;
constexpr int MW_MT = MF_H / MW_WAVES / 16;  // M tiles (16 units) per wave: 2
constexpr int MW_SLAB = MW_ROWS * 64;        // bytes of a 128-row x 32-feature slab
constexpr int MW_RING = 4;                   // register ring depth (slabs / W1 steps in flight)
static_assert(MW_ROWS * 4 == MW_THREADS, "a slab is one 16-B load per thread");

// [128 rows][32 features] bf16 slab, 64-B rows of four 16-B chunks: rows r and r + 4 share
// banks, so chunk c of row r sits at c ^ ((r >> 2) & 3) — a B-fragment read (16 rows x one
// chunk per lane group) covers each 16-B bank group once, as does the row-wise staging write
__device__ __forceinline__ int slab_off(int row, int chunk) { return row * 64 + ((chunk ^ ((row >> 2) & 3)) << 4); }
}  // namespace

__global__ __launch_bounds__(MW_THREADS, 1) void mlp2_fwd_wide_kernel(
    const bf16_t* __restrict__ X, int Fp, const bf16_t* __restrict__ W1, const float* __restrict__ b1,
    const bf16_t* __restrict__ W2, const float* __restrict__ b2, const float* __restrict__ w3,
    const float* __restrict__ b3, float* __restrict__ pred, int B) {
  __shared__ __attribute__((aligned(16))) char h1s[MW_ROWS * MF_H * 2];
  __shared__ __attribute__((aligned(16))) char xs[2][MW_SLAB];
  __shared__ __attribute__((aligned(16))) float prm[3][MF_H];  // b1, b2, w3
  __shared__ float red[MW_WAVES][MW_ROWS];

  const int lane = threadIdx.x & 63, l15 = lane & 15, g = lane >> 4;
  const int wid = threadIdx.x >> 6;
  const int u0 = wid * (16 * MW_MT);  // first unit of this wave

  if (threadIdx.x < MF_H) {  // read after the K loop's first barrier
    prm[0][threadIdx.x] = b1[threadIdx.x];
    prm[1][threadIdx.x] = b2[threadIdx.x];
    prm[2][threadIdx.x] = w3[threadIdx.x];
  }
  // ---- stationary W2 (A operand: lane = unit l15 of M tile m, k 8g .. 8g + 7)
  bf16x8 w2f[MW_MT][8];
#pragma unroll
  for (int m = 0; m < MW_MT; ++m)
#pragma unroll
    for (int kt = 0; kt < 8; ++kt)
      w2f[m][kt] = *reinterpret_cast<const bf16x8*>(W2 + (size_t)(u0 + 16 * m + l15) * MF_H + 32 * kt + 8 * g);
  const float bias3 = b3[0];

  const int nk = (Fp + 31) >> 5;  // K steps of 32 features (the last one zero-filled past Fp)
  const int ntiles = (B + MW_ROWS - 1) / MW_ROWS;

  // staging: thread -> row t >> 2, chunk t & 3 of every slab
  const int sr = threadIdx.x >> 2, sc = threadIdx.x & 3;
  const int soff = slab_off(sr, sc);
  auto load_x = [&](int row0, int k) -> uint4 {
    const int gr = row0 + sr, f0 = 32 * k + 8 * sc;
    return (gr < B && f0 + 8 <= Fp) ? *reinterpret_cast<const uint4*>(X + (size_t)gr * Fp + f0) : make_uint4(0, 0, 0, 0);
  };
  auto load_w1 = [&](int k, int m) -> bf16x8 {
    const int f0 = 32 * k + 8 * g;
    return f0 + 8 <= Fp ? *reinterpret_cast<const bf16x8*>(W1 + (size_t)(u0 + 16 * m + l15) * Fp + f0)
                        : bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
  };

  // register rings: slab s of the tile in xr[s & 3], the W1 fragments of step s in wr[s & 3]
  uint4 xr[MW_RING];
  bf16x8 wr[MW_RING][MW_MT];
  int tile = blockIdx.x;
#pragma unroll
  for (int j = 0; j < MW_RING; ++j) {
    xr[j] = j < nk ? load_x(tile * MW_ROWS, j) : make_uint4(0, 0, 0, 0);
#pragma unroll
    for (int m = 0; m < MW_MT; ++m) wr[j][m] = load_w1(j, m);  // zero past Fp
  }

  for (; tile < ntiles; tile += gridDim.x) {
    const int row0 = tile * MW_ROWS;
    f32x4 acc[MW_MT][MW_NT];
#pragma unroll
    for (int m = 0; m < MW_MT; ++m)
#pragma unroll
      for (int n = 0; n < MW_NT; ++n) acc[m][n] = f32x4{0.f, 0.f, 0.f, 0.f};

    // ---- layer 1: Z1^T (32 units x 128 rows per wave) = W1 x X^T, K = 32 nk
    // slot 0 was last read before the previous tile's barriers
    *reinterpret_cast<uint4*>(xs[0] + soff) = xr[0];
    if (MW_RING < nk) xr[0] = load_x(row0, MW_RING);
    for (int k0 = 0; k0 < nk; k0 += MW_RING) {
#pragma unroll
      for (int j = 0; j < MW_RING; ++j) {
        const int k = k0 + j;
        if (k < nk) {  // uniform
          // slab k is in slot k & 1; every read of slot (k + 1) & 1 (step k - 1) is done
          __syncthreads();
          if (k + 1 < nk) {
            *reinterpret_cast<uint4*>(xs[(j + 1) & 1] + soff) = xr[(j + 1) & 3];
            if (k + 1 + MW_RING < nk) xr[(j + 1) & 3] = load_x(row0, k + 1 + MW_RING);
          }
          const char* xb = xs[j & 1];
#pragma unroll
          for (int n = 0; n < MW_NT; ++n) {
            const bf16x8 xf = *reinterpret_cast<const bf16x8*>(xb + slab_off(16 * n + l15, g));
#pragma unroll
            for (int m = 0; m < MW_MT; ++m)
              acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wr[j][m], xf, acc[m][n], 0, 0, 0);
          }
          if (k + MW_RING < nk) {
#pragma unroll
            for (int m = 0; m < MW_MT; ++m) wr[j][m] = load_w1(k + MW_RING, m);
          }
        }
      }
    }
    // the next tile's first slabs (and W1 steps, unless the ring holds all of W1): in flight
    // under the epilogue and layer 2
    const int ntile = tile + (int)gridDim.x;
    if (ntile < ntiles) {
#pragma unroll
      for (int j = 0; j < MW_RING; ++j) {
        if (j < nk) xr[j] = load_x(ntile * MW_ROWS, j);
        if (nk > MW_RING) {
#pragma unroll
          for (int m = 0; m < MW_MT; ++m) wr[j][m] = load_w1(j, m);
        }
      }
    }
    // epilogue 1: + b1, relu, bf16 (RNE); 4 units -> 8 B into the H1 tile
#pragma unroll
    for (int m = 0; m < MW_MT; ++m) {
      const f32x4 bv = *reinterpret_cast<const f32x4*>(&prm[0][u0 + 16 * m + 4 * g]);
#pragma unroll
      for (int n = 0; n < MW_NT; ++n) {
        const unsigned p0 = pk_bf16(fmaxf(acc[m][n][0] + bv[0], 0.f), fmaxf(acc[m][n][1] + bv[1], 0.f));
        const unsigned p1 = pk_bf16(fmaxf(acc[m][n][2] + bv[2], 0.f), fmaxf(acc[m][n][3] + bv[3], 0.f));
        *reinterpret_cast<uint2*>(h1s + tile_off(16 * n + l15, u0 + 16 * m + 4 * g)) = make_uint2(p0, p1);
      }
    }
    __syncthreads();

    // ---- layer 2: Z2^T = W2 x H1^T, K = 256 (8 k-tiles)
#pragma unroll
    for (int m = 0; m < MW_MT; ++m)
#pragma unroll
      for (int n = 0; n < MW_NT; ++n) acc[m][n] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kt = 0; kt < 8; ++kt)
#pragma unroll
      for (int n = 0; n < MW_NT; ++n) {
        const bf16x8 hb = *reinterpret_cast<const bf16x8*>(h1s + tile_off(16 * n + l15, 32 * kt + 8 * g));
#pragma unroll
        for (int m = 0; m < MW_MT; ++m)
          acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w2f[m][kt], hb, acc[m][n], 0, 0, 0);
      }
    // epilogue 2 + head: H2 = bf16(relu(acc + b2)) times w3, summed over this lane's 8 units
    float hp[MW_NT];
#pragma unroll
    for (int n = 0; n < MW_NT; ++n) hp[n] = 0.f;
#pragma unroll
    for (int m = 0; m < MW_MT; ++m) {
      const f32x4 bv = *reinterpret_cast<const f32x4*>(&prm[1][u0 + 16 * m + 4 * g]);
      const f32x4 wv = *reinterpret_cast<const f32x4*>(&prm[2][u0 + 16 * m + 4 * g]);
#pragma unroll
      for (int n = 0; n < MW_NT; ++n)
#pragma unroll
        for (int r = 0; r < 4; ++r) hp[n] += bf2f(f2bf(fmaxf(acc[m][n][r] + bv[r], 0.f))) * wv[r];
    }
    // the row's 4 lane groups (lanes l15, + 16, + 32, + 48), then the 8 waves through LDS
#pragma unroll
    for (int n = 0; n < MW_NT; ++n) {
      hp[n] += __shfl_xor(hp[n], 16, 64);
      hp[n] += __shfl_xor(hp[n], 32, 64);
    }
    if (g == 0) {
#pragma unroll
      for (int n = 0; n < MW_NT; ++n) red[wid][16 * n + l15] = hp[n];
    }
    __syncthreads();
    if (threadIdx.x < MW_ROWS) {
      const int gr = row0 + (int)threadIdx.x;
      if (gr < B) {
        float p = red[0][threadIdx.x];
#pragma unroll
        for (int w = 1; w < MW_WAVES; ++w) p += red[w][threadIdx.x];
        pred[gr] = p + bias3;
      }
    }
    // red, h1s and the X ring are rewritten only after the next tile's first barrier
  }
}

bool launch_mlp2_fwd_wide(const bf16_t* X, int Fp, const bf16_t* W1, const float* b1, const bf16_t* W2,
                          const float* b2, const float* w3, const float* b3, float* pred, int B, hipStream_t s) {
  if (Fp % 8 != 0 || Fp < 8 || Fp > kMlpWideMaxFp || B <= 0) return false;
  for (const void* p : {(const void*)X, (const void*)W1, (const void*)W2})
    if (reinterpret_cast<uintptr_t>(p) % 16 != 0) return false;
  const int ntiles = (B + MW_ROWS - 1) / MW_ROWS;
  int dev = 0, cus = 0;
  if (hipGetDevice(&dev) != hipSuccess ||
      hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0)
    cus = 256;
  const int grid = ntiles < cus ? ntiles : cus;
  hipLaunchKernelGGL(mlp2_fwd_wide_kernel, dim3(grid), dim3(MW_THREADS), 0, s, X, Fp, W1, b1, W2, b2, w3, b3, pred, B);
  return true;
}

}  // namespace wf
