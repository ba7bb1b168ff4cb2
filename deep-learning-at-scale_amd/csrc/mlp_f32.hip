// wellflow — fused fp32 scoring forward of the F -> 256 -> 256 -> 1 MLP: 1 <= F, Fp <= 512 padded
// features, fp32 operands and fp32 accumulation on v_mfma_f32_32x32x2_f32. No bf16 anywhere.
//
// Why: the bf16 forwards (mlp_fused.hip, mlp_wide.hip) round X, the weights, H1 and H2 to 8
// significant bits; a job that needs its band or set point at the accuracy of the float32 weights
// the .mdl stores had to leave the device for the PyTorch oracle. This kernel reads the fp32 rows
// that assemble_features_kernel<float> writes ([B][ldx], stride n_features, rows 4-B aligned
// only) and the fp32 master weights (NativeMLP.params) in place and writes 4 B of prediction per
// row; every reduction kernel behind it already takes an fp32 prediction vector.
//
// Split: one workgroup of 512 threads (8 waves, two per SIMD) per CU, grid-stride over 64-row
// tiles (kMlpF32Rows). Wave w owns hidden units [32w, 32w + 32) of BOTH layers and all 64 rows:
// 1 M tile x 2 N tiles of 32x32x2, transposed products as in mlp_wide.hip (A = weights, lane =
// unit; B = activations, lane = row): 32 accumulators, a lane's register quad is 4 consecutive
// units of one row.
//
// K order: one 16-B load per lane feeds 4 MFMAs. In K step s (8 features) lane half g = lane / 32
// holds k = 8s + 4g + e, e = 0 .. 3, of its unit (A) and of its row (B); MFMA e multiplies the
// e-th elements, i.e. k = 8s + e and 8s + 4 + e. The order is permuted but fixed, and the same
// for both operands, for every row, tile and B.
//
// Data movement per tile:
//  * X: K slabs of 64 rows x 32 features (8 KB fp32), 4-B loads (consecutive lanes = consecutive
//    features of a row: 128-B segments; the rows have no wider alignment), global -> register
//    ring (4 slabs in flight, 4 values per thread each) -> 2-slot LDS ring -> 16-B B fragments.
//    Slab k + 1 is written to LDS during slab k, slab k + 5 is requested; one barrier per slab.
//    Rows >= B and features >= F are zero-filled in registers, never loaded (the gap may be NaN).
//  * W1 and W2 cannot be stationary (W2 alone is 256 KB): a K step's A fragment (16 B per lane,
//    1 KB per wave) comes from L2 straight into a 4-deep register ring, requested four steps
//    (32 MFMAs per wave) ahead. W1 columns >= F are zeroed in registers, steps >= Fp / 8 are not
//    run. The W2 ring wraps: the next tile's first four steps are requested by the last four.
//  * H1 = relu(acc + b1) exists only as the fp32 [64][256] LDS tile (64 KB); a row's 16-B chunk c
//    sits at c ^ (row & 15), so the 16 lanes of a fragment read (16 rows, one chunk) and of an
//    epilogue write cover each 16-B bank group once. The X slab swizzles c ^ ((row >> 1) & 7).
//  * H2 has no tile: relu(acc + b2) is multiplied by w3 in the accumulators' lanes, the two lane
//    halves are added by one shuffle, the 8 waves through LDS (8 x 64 fp32), in wave order.
//  * the next tile's first four slabs (and W1 steps, when Fp > 32) are requested before the
//    layer-1 epilogue, so they fly under layer 2.
// Nothing is written but pred[0 .. B); no atomics, no scratch buffer. A row's arithmetic does not
// depend on its tile, its position in the tile or B.
//
// Tile choice: 64 rows. Weight traffic is (Fp + 256) KB of L2 reads per tile (320 KB at Fp = 64)
// against 512 (Fp + 256) / 8 MFMAs of 64 cycles per SIMD; the timings in
// profiles/r9/mlp_f32_forward/README.md say which of the two bounds the kernel. A 128-row tile
// would halve the weight traffic but its H1 tile alone is 128 KB: with the X ring it passes the
// CU's 160 KB.
//
// Budget: LDS 64 KB H1 tile + 16 KB X ring + 3 KB b1 / b2 / w3 + 2 KB head partials = 85 KB of
// 160 KB. Registers per lane: 32 accumulators, 16 W1 ring, 16 W2 ring, 16 X ring, 8 B-fragment
// values; the compiler's report (no scratch, no spills) is in the profile README. _build.py
// SOURCE_FLAGS compiles this file with the packed fp32 VALU forms switched off.
#include "common.h"
#include "kernels.h"

namespace wf {

namespace {
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int FW_H = 256;
constexpr int FW_ROWS = kMlpF32Rows;    // rows per tile
constexpr int FW_NT = FW_ROWS / 32;     // N tiles (32 rows) per wave
constexpr int FW_THREADS = 512;
constexpr int FW_WAVES = FW_THREADS / kWave;
constexpr int FW_SLAB = FW_ROWS * 128;  // bytes of a 64-row x 32-feature slab
constexpr int FW_XE = FW_ROWS * 32 / FW_THREADS;  // values per thread and slab
constexpr int FW_RING = 4;              // register ring depth (X slabs, W1 / W2 steps in flight)
static_assert(FW_H == 32 * FW_WAVES, "a wave owns 32 units");
static_assert(FW_XE * FW_THREADS == FW_ROWS * 32 && FW_THREADS / 32 == 16, "staging: 16 rows per pass");

// byte offset of 16-B chunk `chunk` of a row: the H1 tile (64 chunks per row) and an X slab (8)
__device__ __forceinline__ int h1_off(int row, int chunk) { return row * (FW_H * 4) + ((chunk ^ (row & 15)) << 4); }
__device__ __forceinline__ int xs_off(int row, int chunk) { return row * 128 + ((chunk ^ ((row >> 1) & 7)) << 4); }
}  // namespace

__global__ __launch_bounds__(FW_THREADS, 1) void mlp2_fwd_f32_kernel(
    const float* __restrict__ X, long ldx, int F, int Fp, const float* __restrict__ W1, const float* __restrict__ b1,
    const float* __restrict__ W2, const float* __restrict__ b2, const float* __restrict__ w3,
    const float* __restrict__ b3, float* __restrict__ pred, int B) {
  __shared__ __attribute__((aligned(16))) char h1s[FW_ROWS * FW_H * 4];
  __shared__ __attribute__((aligned(16))) char xs[2][FW_SLAB];
  __shared__ __attribute__((aligned(16))) float prm[3][FW_H];  // b1, b2, w3
  __shared__ float red[FW_WAVES][FW_ROWS];

  const int lane = threadIdx.x & 63, l31 = lane & 31, g = lane >> 5;
  const int wid = threadIdx.x >> 6;
  const int u0 = 32 * wid;  // first unit of this wave

  if (threadIdx.x < FW_H) {  // read after the K loop's first barrier
    prm[0][threadIdx.x] = b1[threadIdx.x];
    prm[1][threadIdx.x] = b2[threadIdx.x];
    prm[2][threadIdx.x] = w3[threadIdx.x];
  }
  const float bias3 = b3[0];

  const int nk = (Fp + 31) >> 5;  // X slabs of 32 features (the last one zero-filled past F)
  const int nsteps = Fp >> 3;     // K steps of 8 features in layer 1
  const int ntiles = (B + FW_ROWS - 1) / FW_ROWS;

  // staging: value j of a slab is row 16 j + (t >> 5), feature t & 31
  const int sr = threadIdx.x >> 5, sf = threadIdx.x & 31;
  auto load_x = [&](int row0, int k, int j) -> float {
    const int gr = row0 + 16 * j + sr, f = 32 * k + sf;
    return (gr < B && f < F) ? X[(size_t)gr * (size_t)ldx + f] : 0.f;
  };
  auto stage = [&](int slot, const float (&v)[FW_XE]) {
#pragma unroll
    for (int j = 0; j < FW_XE; ++j)
      *reinterpret_cast<float*>(xs[slot] + xs_off(16 * j + sr, sf >> 2) + 4 * (sf & 3)) = v[j];
  };
  // A fragments: unit u0 + l31, k = 8 s + 4 g .. + 3 (s < nsteps: inside the padded row)
  const float* w1p = W1 + (size_t)(u0 + l31) * Fp + 4 * g;
  const float* w2p = W2 + (size_t)(u0 + l31) * FW_H + 4 * g;
  auto load_w1 = [&](int s) -> f32x4 {
    f32x4 v = *reinterpret_cast<const f32x4*>(w1p + 8 * s);
    const int k0 = 8 * s + 4 * g;
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = k0 + e < F ? v[e] : 0.f;
    return v;
  };
  auto load_w2 = [&](int s) -> f32x4 { return *reinterpret_cast<const f32x4*>(w2p + 8 * s); };

  // register rings: slab k of the tile in xr[k & 3], the W1 fragment of step s in wr[s & 3],
  // the W2 fragment of step s in w2r[s & 3]
  float xr[FW_RING][FW_XE];
  f32x4 wr[FW_RING], w2r[FW_RING];
  int tile = blockIdx.x;
#pragma unroll
  for (int j = 0; j < FW_RING; ++j) {
#pragma unroll
    for (int e = 0; e < FW_XE; ++e) xr[j][e] = j < nk ? load_x(tile * FW_ROWS, j, e) : 0.f;
    wr[j] = j < nsteps ? load_w1(j) : f32x4{0.f, 0.f, 0.f, 0.f};
    w2r[j] = load_w2(j);
  }

  for (; tile < ntiles; tile += gridDim.x) {
    const int row0 = tile * FW_ROWS;
    f32x16 acc[FW_NT];
#pragma unroll
    for (int n = 0; n < FW_NT; ++n)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[n][i] = 0.f;

    // ---- layer 1: Z1^T (32 units x 64 rows per wave) = W1 x X^T, K = Fp
    // slot 0 was last read before the previous tile's barriers
    stage(0, xr[0]);
    if (FW_RING < nk) {
#pragma unroll
      for (int e = 0; e < FW_XE; ++e) xr[0][e] = load_x(row0, FW_RING, e);
    }
    for (int k0 = 0; k0 < nk; k0 += FW_RING) {
#pragma unroll
      for (int j = 0; j < FW_RING; ++j) {
        const int k = k0 + j;
        if (k < nk) {  // uniform
          // slab k is in slot k & 1; every read of slot (k + 1) & 1 (slab k - 1) is done
          __syncthreads();
          if (k + 1 < nk) {
            stage((j + 1) & 1, xr[(j + 1) & 3]);
            if (k + 1 + FW_RING < nk) {
#pragma unroll
              for (int e = 0; e < FW_XE; ++e) xr[(j + 1) & 3][e] = load_x(row0, k + 1 + FW_RING, e);
            }
          }
          const char* xb = xs[j & 1];
#pragma unroll
          for (int jj = 0; jj < 4; ++jj) {
            const int s = 4 * k + jj;
            if (s < nsteps) {  // uniform
              f32x4 xf[FW_NT];
#pragma unroll
              for (int n = 0; n < FW_NT; ++n)
                xf[n] = *reinterpret_cast<const f32x4*>(xb + xs_off(32 * n + l31, 2 * jj + g));
#pragma unroll
              for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int n = 0; n < FW_NT; ++n)
                  acc[n] = __builtin_amdgcn_mfma_f32_32x32x2f32(wr[jj][e], xf[n][e], acc[n], 0, 0, 0);
              if (s + FW_RING < nsteps) wr[jj] = load_w1(s + FW_RING);
            }
          }
        }
      }
    }
    // the next tile's first slabs (and W1 steps, unless the ring holds all of W1): in flight
    // under the epilogue and layer 2
    const int ntile = tile + (int)gridDim.x;
    if (ntile < ntiles) {
#pragma unroll
      for (int j = 0; j < FW_RING; ++j) {
        if (j < nk) {
#pragma unroll
          for (int e = 0; e < FW_XE; ++e) xr[j][e] = load_x(ntile * FW_ROWS, j, e);
        }
        if (nsteps > FW_RING) wr[j] = load_w1(j);
      }
    }
    // epilogue 1: + b1, relu; a register quad is 4 consecutive units of one row -> 16 B of the H1 tile
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int u = u0 + 8 * q + 4 * g;
      const f32x4 bv = *reinterpret_cast<const f32x4*>(&prm[0][u]);
#pragma unroll
      for (int n = 0; n < FW_NT; ++n) {
        f32x4 h;
#pragma unroll
        for (int r = 0; r < 4; ++r) h[r] = fmaxf(acc[n][4 * q + r] + bv[r], 0.f);
        *reinterpret_cast<f32x4*>(h1s + h1_off(32 * n + l31, u >> 2)) = h;
      }
    }
    __syncthreads();

    // ---- layer 2: Z2^T = W2 x H1^T, K = 256 (32 steps)
#pragma unroll
    for (int n = 0; n < FW_NT; ++n)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[n][i] = 0.f;
#pragma unroll 2
    for (int s0 = 0; s0 < FW_H / 8; s0 += FW_RING) {
#pragma unroll
      for (int j = 0; j < FW_RING; ++j) {
        const int s = s0 + j;
        f32x4 hf[FW_NT];
#pragma unroll
        for (int n = 0; n < FW_NT; ++n)
          hf[n] = *reinterpret_cast<const f32x4*>(h1s + h1_off(32 * n + l31, 2 * s + g));
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
          for (int n = 0; n < FW_NT; ++n)
            acc[n] = __builtin_amdgcn_mfma_f32_32x32x2f32(w2r[j][e], hf[n][e], acc[n], 0, 0, 0);
        w2r[j] = load_w2((s + FW_RING) & (FW_H / 8 - 1));  // wraps: the next tile's first steps
      }
    }
    // epilogue 2 + head: relu(acc + b2) times w3, summed over this lane's 16 units in unit order
    float hp[FW_NT];
#pragma unroll
    for (int n = 0; n < FW_NT; ++n) hp[n] = 0.f;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int u = u0 + 8 * q + 4 * g;
      const f32x4 bv = *reinterpret_cast<const f32x4*>(&prm[1][u]);
      const f32x4 wv = *reinterpret_cast<const f32x4*>(&prm[2][u]);
#pragma unroll
      for (int n = 0; n < FW_NT; ++n)
#pragma unroll
        for (int r = 0; r < 4; ++r) hp[n] += fmaxf(acc[n][4 * q + r] + bv[r], 0.f) * wv[r];
    }
    // the row's two lane halves, then the 8 waves through LDS
#pragma unroll
    for (int n = 0; n < FW_NT; ++n) hp[n] += __shfl_xor(hp[n], 32, 64);
    if (g == 0) {
#pragma unroll
      for (int n = 0; n < FW_NT; ++n) red[wid][32 * n + l31] = hp[n];
    }
    __syncthreads();
    if (threadIdx.x < FW_ROWS) {
      const int gr = row0 + (int)threadIdx.x;
      if (gr < B) {
        float p = red[0][threadIdx.x];
#pragma unroll
        for (int w = 1; w < FW_WAVES; ++w) p += red[w][threadIdx.x];
        pred[gr] = p + bias3;
      }
    }
    // red, h1s and the X ring are rewritten only after the next tile's first barrier
  }
}

bool launch_mlp2_fwd_f32(const float* X, long ldx, int F, const float* W1, const float* b1, const float* W2,
                         const float* b2, const float* w3, const float* b3, float* pred, int B, hipStream_t s) {
  const int Fp = (F + 7) / 8 * 8;
  if (F < 1 || Fp > kMlpF32MaxFp || ldx < F || B <= 0) return false;
  for (const void* p : {(const void*)W1, (const void*)W2, (const void*)b1, (const void*)b2, (const void*)w3})
    if (reinterpret_cast<uintptr_t>(p) % 16 != 0) return false;
  for (const void* p : {(const void*)X, (const void*)b3, (const void*)pred})
    if (p == nullptr || reinterpret_cast<uintptr_t>(p) % 4 != 0) return false;
  if (B > INT32_MAX - FW_ROWS) return false;  // row indices of the last tile stay in an int
  const int ntiles = (B + FW_ROWS - 1) / FW_ROWS;
  int dev = 0, cus = 0;
  if (hipGetDevice(&dev) != hipSuccess ||
      hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0)
    cus = 256;
  hipLaunchKernelGGL(mlp2_fwd_f32_kernel, dim3(ntiles < cus ? ntiles : cus), dim3(FW_THREADS), 0, s, X, ldx, F, Fp, W1,
                     b1, W2, b2, w3, b3, pred, B);
  return true;
}

}  // namespace wf
