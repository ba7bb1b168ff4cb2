// wellflow — fused fp32 path-averaged input gradient of the F -> 256 -> 256 -> 1 MLP (integrated
// gradients): per row r and feature f
//   avg[r][f] = (1/m) sum_{j<m} df/dx_f (x' + alpha_j (x_r - x')),  alpha_j = (2j + 1) / (2m)
// for ONE baseline row x' shared by all rows, 1 <= m <= 1024 midpoint steps, 1 <= F, Fp <= 512
// padded features; fp32 operands and fp32 accumulation on v_mfma_f32_32x32x2_f32, fp32 master
// weights, no bf16 anywhere. The ReLU derivative at exactly 0 is 0.
//
// Why a kernel of its own: along the straight path layer 1 is affine in alpha,
//   z1(alpha) = (W1 x' + b1) + alpha W1 (x - x') = zb + alpha D,
// so the F-deep layer-1 GEMM runs ONCE per tile (on x - x'), and the F-wide dX = G1 x W1 GEMM is
// linear in G1, so it runs once too, on S = sum_j G1_j. Only the two 256 x 256 products depend on
// alpha. m launches of mlp_f32_grad.hip on m interpolated tables would run all four GEMMs m times
// and write m [rows][F] gradients; here nothing leaves the CU between the first read of X and the
// one write of avg.
//
// Split, tile, swizzles, K order and the dealing of stage 4's feature blocks are
// mlp_f32_grad.hip's: one workgroup of 512 threads (8 waves, two per SIMD) per CU, grid-stride
// over 64-row tiles; wave w owns units [32w, 32w + 32) of BOTH hidden layers and all 64 rows in
// stages 1 - 3 (A = weights, lane = unit; B = activations, lane = row); in K step s lane half
// g = lane / 32 holds k = 8s + 4g + e and MFMA e multiplies k = 8s + e and 8s + 4 + e.
//
// Stages:
//  0. once per workgroup: x' -> LDS (zero past F); zb[u] = b1[u] + sum_f W1[u][f] x'[f], an fp32
//     fmaf chain in feature order by thread u, into the LDS parameter block next to b2 and w3.
//  1. once per tile: D^T = W1 x (X - x')^T, K = Fp. The subtraction is one fp32 operation made
//     while the X slab is staged from the register ring into LDS. D is never written anywhere:
//     it stays in 32 accumulator registers per lane through the whole step loop.
//  Step j = 0 .. m - 1, all on chip:
//     a. H1 = relu(fmaf(alpha_j, D, zb)) -> the 64-row LDS tile; bit (H1 > 0) of each of the
//        lane's 32 values -> ONE register m1.
//     b. stage 2: Z2^T = W2 x H1^T (K = 256). No head reduction: only the sign of acc + b2 is
//        used. G2 = (acc + b2 > 0) ? w3 : 0 is written over H1 (after the barrier that ends the
//        reads of H1).
//     c. stage 3: G1^T = W2^T x G2^T (K = 256), W2 read in place as columns (no transposed
//        copy). The wave owns the same layer-1 units as in a., so the mask meets its own
//        accumulators in registers: S += m1 bit ? acc : 0, a second set of 32 registers, in
//        step order.
//     Both W2 rings (4 K steps deep, 16 values per lane each) wrap from one step into the next
//     (not past the last: they are filled after stage 1 and dead outside the loop),
//     so the next step's first fragments are in flight under the epilogues and barriers.
//  4. once per tile: S -> LDS tile; avg = (S x W1) * (1 / m) in blocks of 32 features with the
//     operands swapped (A = S fragment, lane = row; B = W1[j][f] in place, lane = f, zero past F
//     and never read there), so the stores cover 128-B row segments. The next tile's first X
//     slabs and W1 steps are requested before this stage and fly under it.
//
// Written: avg[row][f], row < B, f < F. Nothing else: no prediction, no atomics, no scratch
// buffer. A row's arithmetic does not depend on its tile, its position in the tile or B.
//
// Budget: LDS 64 KB tile + 16 KB X ring + 3 KB zb / b2 / w3 + 2 KB x' = 85 KB of 160 KB.
// Registers per lane: 32 (D) + 32 (S) + 32 (acc) + two 16-value W2 rings + 8 fragment values + the
// mask inside the loop; the X and W1 rings (16 each) are live only outside it, the W2 rings only
// inside. The compiler's report (no scratch, no vector spills) is in profiles/r11/mlp_f32_path/README.md. _build.py SOURCE_FLAGS compiles this file with
// the packed fp32 VALU forms switched off.
#include "common.h"
#include "kernels.h"

namespace wf {

namespace {
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int PG_H = 256;
constexpr int PG_ROWS = kMlpF32Rows;    // rows per tile
constexpr int PG_NT = PG_ROWS / 32;     // N tiles (32 rows) per wave
constexpr int PG_THREADS = 512;
constexpr int PG_WAVES = PG_THREADS / kWave;
constexpr int PG_SLAB = PG_ROWS * 128;  // bytes of a 64-row x 32-feature slab
constexpr int PG_XE = PG_ROWS * 32 / PG_THREADS;  // values per thread and slab
constexpr int PG_RING = 4;              // register ring depth
constexpr int PG_STEPS = PG_H / 8;      // K steps of a 256-deep product
static_assert(PG_H == 32 * PG_WAVES, "a wave owns 32 units");
static_assert(PG_NT == 2, "the mask is 2 x 16 bits; stage 4 splits a block into two row halves");
static_assert(PG_XE * PG_THREADS == PG_ROWS * 32 && PG_THREADS / 32 == 16, "staging: 16 rows per pass");
static_assert(kMlpF32MaxFp <= PG_THREADS, "the baseline row is staged by one thread per feature");

// byte offset of 16-B chunk `chunk` of a row: the LDS tile (64 chunks per row) and an X slab (8)
__device__ __forceinline__ int t_off(int row, int chunk) { return row * (PG_H * 4) + ((chunk ^ (row & 15)) << 4); }
__device__ __forceinline__ int xs_off(int row, int chunk) { return row * 128 + ((chunk ^ ((row >> 1) & 7)) << 4); }
}  // namespace

__global__ __launch_bounds__(PG_THREADS, 1) void mlp2_path_grad_f32_kernel(
    const float* __restrict__ X, long ldx, int F, int Fp, const float* __restrict__ xbase,
    const float* __restrict__ W1, const float* __restrict__ b1, const float* __restrict__ W2,
    const float* __restrict__ b2, const float* __restrict__ w3, int steps, float* __restrict__ avg, long ldg, int B) {
  __shared__ __attribute__((aligned(16))) char ts[PG_ROWS * PG_H * 4];  // H1 / G2 per step, then S
  __shared__ __attribute__((aligned(16))) char xs[2][PG_SLAB];
  __shared__ __attribute__((aligned(16))) float prm[3][PG_H];          // zb, b2, w3
  __shared__ __attribute__((aligned(16))) float xbs[kMlpF32MaxFp];     // the baseline row, zero past F

  const int lane = threadIdx.x & 63, l31 = lane & 31, g = lane >> 5;
  const int wid = threadIdx.x >> 6;
  const int u0 = 32 * wid;  // first unit of this wave

  const int nk = (Fp + 31) >> 5;  // X slabs / avg blocks of 32 features
  const int nsteps = Fp >> 3;     // K steps of 8 features in layer 1
  const int ntiles = (B + PG_ROWS - 1) / PG_ROWS;
  // stage 4: items of this wave are wid, wid + 8, ..: a block with both row halves, or (block, half)
  const bool halves = nk < PG_WAVES;
  const int nitems = halves ? 2 * nk : nk;

  // staging: value j of a slab is row 16 j + (t >> 5), feature t & 31
  const int sr = threadIdx.x >> 5, sf = threadIdx.x & 31;
  // made opaque at every tile's top: the row addresses are formed per tile, not kept across tiles
  const float* Xv = X;
  long ldxv = ldx;
  auto load_x = [&](int row0, int k, int j) -> float {
    const int gr = row0 + 16 * j + sr, f = 32 * k + sf;
    return (gr < B && f < F) ? Xv[(size_t)gr * (size_t)ldxv + f] : 0.f;
  };
  // slab k of the tile -> LDS slot, minus the baseline (one fp32 subtraction; 0 - 0 past F)
  auto stage = [&](int slot, int k, const float (&v)[PG_XE]) {
    const float xb = xbs[32 * k + sf];
#pragma unroll
    for (int j = 0; j < PG_XE; ++j)
      *reinterpret_cast<float*>(xs[slot] + xs_off(16 * j + sr, sf >> 2) + 4 * (sf & 3)) = v[j] - xb;
  };
  // A fragments of stages 1 and 2: unit u0 + l31, k = 8 s + 4 g .. + 3
  const float* w1p = W1 + (size_t)(u0 + l31) * Fp + 4 * g;
  const float* w2p = W2 + (size_t)(u0 + l31) * PG_H + 4 * g;
  auto load_w1 = [&](int s) -> f32x4 {
    f32x4 v = *reinterpret_cast<const f32x4*>(w1p + 8 * s);
    const int k0 = 8 * s + 4 * g;
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = k0 + e < F ? v[e] : 0.f;
    return v;
  };
  auto load_w2 = [&](int s) -> f32x4 { return *reinterpret_cast<const f32x4*>(w2p + 8 * s); };
  // stage 3's A fragment: W2[8 s + 4 g + e][u0 + l31], the column of layer-1 unit u0 + l31; stage
  // 4's B fragment: W1[8 s + 4 g + e][f0 + l31], where a column >= F is zero and is not read (the
  // lane reads column F - 1 instead and drops it). 32-bit element offsets from the uniform bases.
  unsigned w2o = (unsigned)(4 * g * PG_H + u0 + l31);
  auto load_w2t = [&](int s) -> f32x4 {
    f32x4 v;
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = W2[w2o + (unsigned)((8 * s + e) * PG_H)];
    return v;
  };
  int fpt = Fp;  // stage 4's row stride of W1: opaque per tile, so its offsets live in stage 4 only
  auto load_w1t = [&](int f0, int s) -> f32x4 {
    const int f = f0 + l31;
    const unsigned o = (unsigned)((8 * s + 4 * g) * fpt + (f < F ? f : F - 1));
    f32x4 v;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float w = W1[o + (unsigned)(e * fpt)];
      v[e] = f < F ? w : 0.f;
    }
    return v;
  };

  // register rings: slab k of the tile in xr[k & 3], the W1 fragment of step s in wr[s & 3], the
  // W2 fragment of step s in w2r[s & 3]; gr is the ring of stage 3 (W2 columns), then of stage 4.
  // The W2 rings are filled after stage 1 and are dead after the last step.
  float xr[PG_RING][PG_XE];
  f32x4 wr[PG_RING], w2r[PG_RING], gr[PG_RING];
  int tile = blockIdx.x;
#pragma unroll
  for (int j = 0; j < PG_RING; ++j) {
#pragma unroll
    for (int e = 0; e < PG_XE; ++e) xr[j][e] = j < nk ? load_x(tile * PG_ROWS, j, e) : 0.f;
    wr[j] = j < nsteps ? load_w1(j) : f32x4{0.f, 0.f, 0.f, 0.f};
  }

  // ---- stage 0: the baseline row, b2, w3, then zb = b1 + W1 x' (thread u: unit u, feature order)
  xbs[threadIdx.x] = (int)threadIdx.x < F ? xbase[threadIdx.x] : 0.f;
  if (threadIdx.x < PG_H) {
    prm[1][threadIdx.x] = b2[threadIdx.x];
    prm[2][threadIdx.x] = w3[threadIdx.x];
  }
  __syncthreads();
  if (threadIdx.x < PG_H) {  // read after the K loop's first barrier
    const float* wrow = W1 + (size_t)threadIdx.x * Fp;
    float sum = 0.f;
    for (int f = 0; f < Fp; f += 4) {
      const f32x4 w = *reinterpret_cast<const f32x4*>(wrow + f);
      const f32x4 x = *reinterpret_cast<const f32x4*>(&xbs[f]);
#pragma unroll
      for (int e = 0; e < 4; ++e) sum = __builtin_fmaf(f + e < F ? w[e] : 0.f, x[e], sum);  // past F: + 0 x 0
    }
    prm[0][threadIdx.x] = b1[threadIdx.x] + sum;
  }
  const float inv_m = 1.0f / (float)steps;
  const float two_m = (float)(2 * steps);

  for (; tile < ntiles; tile += gridDim.x) {
    const int row0 = tile * PG_ROWS;
    asm volatile("" : "+s"(ldxv), "+s"(Xv));
    f32x16 acc[PG_NT], D[PG_NT], S[PG_NT];
#pragma unroll
    for (int n = 0; n < PG_NT; ++n)
#pragma unroll
      for (int i = 0; i < 16; ++i) D[n][i] = 0.f;

    // ---- stage 1: D^T (32 units x 64 rows per wave) = W1 x (X - x')^T, K = Fp
    // slot 0 was last read before the previous tile's barriers
    stage(0, 0, xr[0]);
    if (PG_RING < nk) {
#pragma unroll
      for (int e = 0; e < PG_XE; ++e) xr[0][e] = load_x(row0, PG_RING, e);
    }
    for (int k0 = 0; k0 < nk; k0 += PG_RING) {
#pragma unroll
      for (int j = 0; j < PG_RING; ++j) {
        const int k = k0 + j;
        if (k < nk) {  // uniform
          // slab k is in slot k & 1; every read of slot (k + 1) & 1 (slab k - 1) is done
          __syncthreads();
          if (k + 1 < nk) {
            stage((j + 1) & 1, k + 1, xr[(j + 1) & 3]);
            if (k + 1 + PG_RING < nk) {
#pragma unroll
              for (int e = 0; e < PG_XE; ++e) xr[(j + 1) & 3][e] = load_x(row0, k + 1 + PG_RING, e);
            }
          }
          const char* xb = xs[j & 1];
#pragma unroll
          for (int jj = 0; jj < 4; ++jj) {
            const int s = 4 * k + jj;
            if (s < nsteps) {  // uniform
              f32x4 xf[PG_NT];
#pragma unroll
              for (int n = 0; n < PG_NT; ++n)
                xf[n] = *reinterpret_cast<const f32x4*>(xb + xs_off(32 * n + l31, 2 * jj + g));
#pragma unroll
              for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int n = 0; n < PG_NT; ++n)
                  D[n] = __builtin_amdgcn_mfma_f32_32x32x2f32(wr[jj][e], xf[n][e], D[n], 0, 0, 0);
              if (s + PG_RING < nsteps) wr[jj] = load_w1(s + PG_RING);
            }
          }
        }
      }
    }
    // the first K steps of stages 2 and 3 of step 0, requested only now so that neither ring is live
    // across stage 1; later steps find them wrapped round by the step before. The addresses are the
    // same in every tile: made opaque here, or the loads are hoisted above the tile loop and their
    // 32 values spilled around stage 1
    asm volatile("" : "+v"(w2o), "+v"(w2p));
#pragma unroll
    for (int j = 0; j < PG_RING; ++j) {
      w2r[j] = load_w2(j);
      gr[j] = load_w2t(j);
    }
#pragma unroll
    for (int n = 0; n < PG_NT; ++n)
#pragma unroll
      for (int i = 0; i < 16; ++i) S[n][i] = 0.f;

    // ---- the step loop: nothing leaves the CU
#pragma unroll 1
    for (int step = 0; step < steps; ++step) {
      const float alpha = (float)(2 * step + 1) / two_m;  // correctly rounded fp32 division
      const bool more = step + 1 < steps;  // uniform: the W2 rings wrap into the next step, not past the last
      // every read of the tile is done: the previous step's G2, or the previous tile's S
      __syncthreads();
      // a. H1 = relu(alpha D + zb) -> 16 B of the tile per register quad; the mask bits stay here
      unsigned m1 = 0u;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int u = u0 + 8 * q + 4 * g;
        const f32x4 zv = *reinterpret_cast<const f32x4*>(&prm[0][u]);
#pragma unroll
        for (int n = 0; n < PG_NT; ++n) {
          f32x4 h;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            h[r] = fmaxf(__builtin_fmaf(alpha, D[n][4 * q + r], zv[r]), 0.f);
            m1 |= (h[r] > 0.f ? 1u : 0u) << (16 * n + 4 * q + r);
          }
          *reinterpret_cast<f32x4*>(ts + t_off(32 * n + l31, u >> 2)) = h;
        }
      }
      __syncthreads();

      // b. stage 2: Z2^T = W2 x H1^T, K = 256 (32 steps)
#pragma unroll
      for (int n = 0; n < PG_NT; ++n)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[n][i] = 0.f;
#pragma unroll 2
      for (int s0 = 0; s0 < PG_STEPS; s0 += PG_RING) {
#pragma unroll
        for (int j = 0; j < PG_RING; ++j) {
          const int s = s0 + j;
          f32x4 hf[PG_NT];
#pragma unroll
          for (int n = 0; n < PG_NT; ++n)
            hf[n] = *reinterpret_cast<const f32x4*>(ts + t_off(32 * n + l31, 2 * s + g));
#pragma unroll
          for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int n = 0; n < PG_NT; ++n)
              acc[n] = __builtin_amdgcn_mfma_f32_32x32x2f32(w2r[j][e], hf[n][e], acc[n], 0, 0, 0);
          if (more || s + PG_RING < PG_STEPS) w2r[j] = load_w2((s + PG_RING) & (PG_STEPS - 1));
        }
      }
      // G2 = (acc + b2 > 0) ? w3 : 0: only the sign of z2 is used
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int u = u0 + 8 * q + 4 * g;
        const f32x4 bv = *reinterpret_cast<const f32x4*>(&prm[1][u]);
        const f32x4 wv = *reinterpret_cast<const f32x4*>(&prm[2][u]);
#pragma unroll
        for (int n = 0; n < PG_NT; ++n)
#pragma unroll
          for (int r = 0; r < 4; ++r) acc[n][4 * q + r] = acc[n][4 * q + r] + bv[r] > 0.f ? wv[r] : 0.f;
      }
      __syncthreads();  // every read of H1 is done
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int n = 0; n < PG_NT; ++n) {
          f32x4 v;
#pragma unroll
          for (int r = 0; r < 4; ++r) v[r] = acc[n][4 * q + r];
          *reinterpret_cast<f32x4*>(ts + t_off(32 * n + l31, (u0 + 8 * q + 4 * g) >> 2)) = v;
        }
      __syncthreads();

      // c. stage 3: G1^T = W2^T x G2^T, K = 256 over layer-2 units; this wave's layer-1 units
#pragma unroll
      for (int n = 0; n < PG_NT; ++n)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[n][i] = 0.f;
#pragma unroll 1
      for (int s0 = 0; s0 < PG_STEPS; s0 += PG_RING) {
#pragma unroll
        for (int j = 0; j < PG_RING; ++j) {
          const int s = s0 + j;
          f32x4 gf[PG_NT];
#pragma unroll
          for (int n = 0; n < PG_NT; ++n)
            gf[n] = *reinterpret_cast<const f32x4*>(ts + t_off(32 * n + l31, 2 * s + g));
#pragma unroll
          for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int n = 0; n < PG_NT; ++n)
              acc[n] = __builtin_amdgcn_mfma_f32_32x32x2f32(gr[j][e], gf[n][e], acc[n], 0, 0, 0);
          if (more || s + PG_RING < PG_STEPS) gr[j] = load_w2t((s + PG_RING) & (PG_STEPS - 1));
        }
      }
      // the layer-1 mask, bit by bit, and the running sum in step order
#pragma unroll
      for (int n = 0; n < PG_NT; ++n)
#pragma unroll
        for (int i = 0; i < 16; ++i) S[n][i] += (m1 >> (16 * n + i)) & 1u ? acc[n][i] : 0.f;
    }

    // the next tile's first slabs (and W1 steps, unless the ring holds all of W1): in flight
    // under stage 4; stage 4's first item: its first steps fly under the two barriers
    const int ntile = tile + (int)gridDim.x;
    const bool next = ntile < ntiles;  // uniform
#pragma unroll
    for (int j = 0; j < PG_RING; ++j) {  // every ring value is reassigned: none is live across the step loop
#pragma unroll
      for (int e = 0; e < PG_XE; ++e) xr[j][e] = next && j < nk ? load_x(ntile * PG_ROWS, j, e) : 0.f;
      wr[j] = next && j < nsteps ? load_w1(j) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
    asm volatile("" : "+s"(fpt));
    int item = __builtin_amdgcn_readfirstlane(wid);  // scalar: stage 4's branches are uniform
    int f0 = 32 * (halves ? item >> 1 : item);
    if (item < nitems) {
#pragma unroll
      for (int j = 0; j < PG_RING; ++j) gr[j] = load_w1t(f0, j);
    }
    __syncthreads();  // every read of the last G2 is done
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int n = 0; n < PG_NT; ++n) {
        f32x4 v;
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = S[n][4 * q + r];
        *reinterpret_cast<f32x4*>(ts + t_off(32 * n + l31, (u0 + 8 * q + 4 * g) >> 2)) = v;
      }
    __syncthreads();

    // ---- stage 4: avg (64 rows x 32 features per block) = (S x W1) / m, K = 256 over layer-1 units
    for (; item < nitems; item += PG_WAVES) {
      const int nlo = halves ? item & 1 : 0, nhi = halves ? nlo + 1 : PG_NT;  // uniform
#pragma unroll
      for (int n = 0; n < PG_NT; ++n)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[n][i] = 0.f;
#pragma unroll 1
      for (int s0 = 0; s0 < PG_STEPS; s0 += PG_RING) {
#pragma unroll
        for (int j = 0; j < PG_RING; ++j) {
          const int s = s0 + j;
#pragma unroll
          for (int n = 0; n < PG_NT; ++n) {
            if (n >= nlo && n < nhi) {
              const f32x4 gf = *reinterpret_cast<const f32x4*>(ts + t_off(32 * n + l31, 2 * s + g));
#pragma unroll
              for (int e = 0; e < 4; ++e)
                acc[n] = __builtin_amdgcn_mfma_f32_32x32x2f32(gf[e], gr[j][e], acc[n], 0, 0, 0);
            }
          }
          if (s + PG_RING < PG_STEPS) gr[j] = load_w1t(f0, s + PG_RING);
        }
      }
      // output epilogue: accumulator 4 q + r is row 32 n + 8 q + 4 g + r, the lane is the feature
      const int f = f0 + l31;
      const int nitem = item + PG_WAVES;
      const int nf0 = 32 * (halves ? nitem >> 1 : nitem);
      if (nitem < nitems) {
#pragma unroll
        for (int j = 0; j < PG_RING; ++j) gr[j] = load_w1t(nf0, j);
      }
      // (32-bit offsets inside the tile from its uniform base; a whole tile needs no row test)
      float* trow = avg + (size_t)row0 * (size_t)ldg;
      // (the stride is opaque here: the 32 row offsets are formed at the stores, not kept across the kernel)
      unsigned ld = (unsigned)ldg;
      asm volatile("" : "+v"(ld));
      const unsigned o = (unsigned)(4 * g) * ld + (unsigned)f;
      if (f < F) {
        if (row0 + PG_ROWS <= B) {  // uniform
#pragma unroll
          for (int n = 0; n < PG_NT; ++n) {
            if (n >= nlo && n < nhi) {
#pragma unroll
              for (int i = 0; i < 16; ++i)
                trow[o + (unsigned)(32 * n + 8 * (i >> 2) + (i & 3)) * ld] = acc[n][i] * inv_m;
            }
          }
        } else {
          int lim = B - row0 - 4 * g;  // this lane's rows 32 n + 8 q + r below lim exist
          // opaque: the 32 row tests are made here, one at a time, not hoisted above the K loop
          asm volatile("" : "+v"(lim));
#pragma unroll
          for (int n = 0; n < PG_NT; ++n) {
            if (n >= nlo && n < nhi) {
#pragma unroll
              for (int i = 0; i < 16; ++i) {
                const int ri = 32 * n + 8 * (i >> 2) + (i & 3);
                if (ri < lim) trow[o + (unsigned)ri * ld] = acc[n][i] * inv_m;
              }
            }
          }
        }
      }
      f0 = nf0;
    }
    // the tile and the X ring are rewritten only after the next tile's first barrier
  }
}

bool launch_mlp2_path_grad_f32(const float* X, long ldx, int F, const float* xb, const float* W1, const float* b1,
                               const float* W2, const float* b2, const float* w3, int steps, float* avg, long ldg,
                               int B, hipStream_t s) {
  const int Fp = (F + 7) / 8 * 8;
  if (F < 1 || Fp > kMlpF32MaxFp || ldx < F || ldg < F || ldg > (1L << 24) || B <= 0) return false;
  if (steps < 1 || steps > kMlpPathMaxSteps) return false;
  for (const void* p : {(const void*)W1, (const void*)W2, (const void*)b1, (const void*)b2, (const void*)w3})
    if (p == nullptr || reinterpret_cast<uintptr_t>(p) % 16 != 0) return false;
  for (const void* p : {(const void*)X, (const void*)xb, (const void*)avg})
    if (p == nullptr || reinterpret_cast<uintptr_t>(p) % 4 != 0) return false;
  if (B > INT32_MAX - PG_ROWS) return false;  // row indices of the last tile stay in an int
  const int ntiles = (B + PG_ROWS - 1) / PG_ROWS;
  int dev = 0, cus = 0;
  if (hipGetDevice(&dev) != hipSuccess ||
      hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0)
    cus = 256;
  hipLaunchKernelGGL(mlp2_path_grad_f32_kernel, dim3(ntiles < cus ? ntiles : cus), dim3(PG_THREADS), 0, s, X, ldx, F,
                     Fp, xb, W1, b1, W2, b2, w3, steps, avg, ldg, B);
  return true;
}

}  // namespace wf
