// wellflow — fused fp32 input gradient of the F -> 256 -> 256 -> 1 MLP: per row the prediction and
// dpred/dx = W1^T (m1 * (W2^T (m2 * w3))), m1 = (z1 > 0), m2 = (z2 > 0), 1 <= F, Fp <= 512 padded
// features, fp32 operands and fp32 accumulation on v_mfma_f32_32x32x2_f32. No bf16 anywhere.
//
// Why: the sensitivity job (sensitivity.py) wants the derivative of the prediction with respect
// to every input, row by row. The gradient depends on the activations only through the two ReLU
// masks and is otherwise a product of weights, so it is formed from the fp32 master weights
// (NativeMLP.params) in place: a bf16 route would carry three weight roundings into a quantity
// people difference. The forward half is mlp_f32.hip's, stage for stage; the two gradient GEMMs
// run over the same 64-row LDS tile, which is reused three times (H1, then G2, then G1).
//
// Split: one workgroup of 512 threads (8 waves, two per SIMD) per CU, grid-stride over 64-row
// tiles (kMlpF32Rows). Wave w owns units [32w, 32w + 32) of BOTH hidden layers and all 64 rows in
// stages 1 - 3 (1 M tile x 2 N tiles of 32x32x2, transposed products: A = weights, lane = unit;
// B = activations, lane = row; a lane's register quad is 4 consecutive units of one row). In
// stage 4 the 32-feature blocks of dX are dealt over the waves.
//
// Stages of a tile:
//  1. Z1^T = W1 x X^T (K = Fp), as the forward. Epilogue: H1 = relu(acc + b1) -> LDS tile, and
//     the bit (H1 > 0) of each of the lane's 32 accumulators -> ONE register m1 (bit 16 n + i of
//     accumulator acc[n][i]). The ReLU derivative at exactly 0 is 0.
//  2. Z2^T = W2 x H1^T (K = 256), as the forward. Epilogue: the head reduction, term for term as
//     the forward's, and G2 = (acc + b2 > 0) ? w3 : 0 in the accumulators. After the barrier that
//     ends the last read of H1, G2 is written over it (same swizzle).
//  3. G1^T = W2^T x G2^T (K = 256 over layer-2 units). The wave owns the SAME 32 layer-1 units as
//     in stage 1, so acc[n][i] meets its own mask bit: G1 = m1 bit ? acc : 0, the mask never
//     leaves its register. A operand: W2[u][j], lane = j, read from the row-major W2 in place
//     with 4-B loads (consecutive lanes = consecutive j: 128-B segments), four per K step in a
//     4-deep register ring. No transposed weight copy exists, so none can go stale. Barrier, then
//     G1 is written over G2.
//  4. dX = G1 x W1 (K = 256 over layer-1 units), in blocks of 32 features. Here the operands are
//     swapped against stages 1 - 3 (A = G1 fragment, lane = row; B = W1[j][f] read in place from
//     the [256][Fp] rows with 4-B loads, lane = f, zero past F and never loaded there): the sum
//     over k and its order are the same as in the transposed product, but an accumulator register
//     then holds 32 consecutive features of ONE row in its 32 lanes, so the output epilogue's
//     stores cover 128-B segments of dX (rows are 4-B aligned only, so the stores are 4 B each).
//     Fp >= 256: block b goes to wave b mod 8 with both 32-row halves (a W1 fragment feeds 8
//     MFMAs). Fp < 256: the items are (block, row half), item i to wave i mod 8, so the one block
//     of Fp <= 32 keeps two waves busy instead of one (see the profile README for the count).
//
// K order, stages 1 - 3 as the forward: in K step s lane half g = lane / 32 holds k = 8s + 4g + e,
// e = 0 .. 3; MFMA e multiplies k = 8s + e and 8s + 4 + e. Stage 4 the same over layer-1 units.
// The order is fixed: the same for every row, tile and B.
//
// Data movement: the X slab ring, the W1 / W2 rings from L2 and the prefetch of the next tile's
// first slabs under the later stages are the forward's. Stage 3 and stage 4 have a 4-deep
// register ring each (4 x 4 values per lane), requested four K steps ahead; stage 3's first four
// steps are requested before the head reduction, stage 4's before the stage-3 epilogue.
// Written: pred[0 .. B) and dX[row][f], row < B, f < F. Nothing else: no atomics, no scratch
// buffer. A row's arithmetic does not depend on its tile, its position in the tile or B.
//
// Budget: LDS as the forward, 64 KB tile + 16 KB X ring + 3 KB b1 / b2 / w3 + 2 KB head partials
// = 85 KB of 160 KB. Registers per lane: 32 accumulators, 16 each for the W1, W2, X, stage-3 and
// stage-4 rings, 8 fragment values, the mask; the compiler's report (no scratch, no vector spills;
// 22 scalar values are parked in lanes of a vector register, short of the goal of no spills at
// all: see there) is in profiles/r10/mlp_f32_grad/README.md. _build.py SOURCE_FLAGS compiles this file with the packed
// fp32 VALU forms switched off.
#include "common.h"
#include "kernels.h"

namespace wf {

namespace {
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int GR_H = 256;
constexpr int GR_ROWS = kMlpF32Rows;    // rows per tile
constexpr int GR_NT = GR_ROWS / 32;     // N tiles (32 rows) per wave
constexpr int GR_THREADS = 512;
constexpr int GR_WAVES = GR_THREADS / kWave;
constexpr int GR_SLAB = GR_ROWS * 128;  // bytes of a 64-row x 32-feature slab
constexpr int GR_XE = GR_ROWS * 32 / GR_THREADS;  // values per thread and slab
constexpr int GR_RING = 4;              // register ring depth
constexpr int GR_STEPS = GR_H / 8;      // K steps of a 256-deep product
static_assert(GR_H == 32 * GR_WAVES, "a wave owns 32 units");
static_assert(GR_NT == 2, "the mask is 2 x 16 bits; stage 4 splits a block into two row halves");
static_assert(GR_XE * GR_THREADS == GR_ROWS * 32 && GR_THREADS / 32 == 16, "staging: 16 rows per pass");

// byte offset of 16-B chunk `chunk` of a row: the LDS tile (64 chunks per row) and an X slab (8)
__device__ __forceinline__ int t_off(int row, int chunk) { return row * (GR_H * 4) + ((chunk ^ (row & 15)) << 4); }
__device__ __forceinline__ int xs_off(int row, int chunk) { return row * 128 + ((chunk ^ ((row >> 1) & 7)) << 4); }
}  // namespace

__global__ __launch_bounds__(GR_THREADS, 1) void mlp2_grad_f32_kernel(
    const float* __restrict__ X, long ldx, int F, int Fp, const float* __restrict__ W1, const float* __restrict__ b1,
    const float* __restrict__ W2, const float* __restrict__ b2, const float* __restrict__ w3,
    const float* __restrict__ b3, float* __restrict__ pred, float* __restrict__ dX, long ldg, int B) {
  __shared__ __attribute__((aligned(16))) char ts[GR_ROWS * GR_H * 4];  // H1, then G2, then G1
  __shared__ __attribute__((aligned(16))) char xs[2][GR_SLAB];
  __shared__ __attribute__((aligned(16))) float prm[3][GR_H];  // b1, b2, w3
  __shared__ float red[GR_WAVES][GR_ROWS];

  const int lane = threadIdx.x & 63, l31 = lane & 31, g = lane >> 5;
  const int wid = threadIdx.x >> 6;
  const int u0 = 32 * wid;  // first unit of this wave

  if (threadIdx.x < GR_H) {  // read after the K loop's first barrier
    prm[0][threadIdx.x] = b1[threadIdx.x];
    prm[1][threadIdx.x] = b2[threadIdx.x];
    prm[2][threadIdx.x] = w3[threadIdx.x];
  }
  const float bias3 = b3[0];

  const int nk = (Fp + 31) >> 5;  // X slabs / dX blocks of 32 features
  const int nsteps = Fp >> 3;     // K steps of 8 features in layer 1
  const int ntiles = (B + GR_ROWS - 1) / GR_ROWS;
  // stage 4: items of this wave are wid, wid + 8, ..: a block with both row halves, or (block, half)
  const bool halves = nk < GR_WAVES;
  const int nitems = halves ? 2 * nk : nk;

  // staging: value j of a slab is row 16 j + (t >> 5), feature t & 31
  const int sr = threadIdx.x >> 5, sf = threadIdx.x & 31;
  auto load_x = [&](int row0, int k, int j) -> float {
    const int gr = row0 + 16 * j + sr, f = 32 * k + sf;
    return (gr < B && f < F) ? X[(size_t)gr * (size_t)ldx + f] : 0.f;
  };
  auto stage = [&](int slot, const float (&v)[GR_XE]) {
#pragma unroll
    for (int j = 0; j < GR_XE; ++j)
      *reinterpret_cast<float*>(xs[slot] + xs_off(16 * j + sr, sf >> 2) + 4 * (sf & 3)) = v[j];
  };
  // A fragments of stages 1 and 2: unit u0 + l31, k = 8 s + 4 g .. + 3
  const float* w1p = W1 + (size_t)(u0 + l31) * Fp + 4 * g;
  const float* w2p = W2 + (size_t)(u0 + l31) * GR_H + 4 * g;
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
  const unsigned w2o = (unsigned)(4 * g * GR_H + u0 + l31);
  auto load_w2t = [&](int s) -> f32x4 {
    f32x4 v;
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = W2[w2o + (unsigned)((8 * s + e) * GR_H)];
    return v;
  };
  auto load_w1t = [&](int f0, int s) -> f32x4 {
    const int f = f0 + l31;
    const unsigned o = (unsigned)((8 * s + 4 * g) * Fp + (f < F ? f : F - 1));
    f32x4 v;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float w = W1[o + (unsigned)(e * Fp)];
      v[e] = f < F ? w : 0.f;
    }
    return v;
  };

  // register rings: slab k of the tile in xr[k & 3], the W1 fragment of step s in wr[s & 3],
  // the W2 fragment of step s in w2r[s & 3]; gr is the ring of stage 3, then of stage 4
  float xr[GR_RING][GR_XE];
  f32x4 wr[GR_RING], w2r[GR_RING], gr[GR_RING];
  int tile = blockIdx.x;
#pragma unroll
  for (int j = 0; j < GR_RING; ++j) {
#pragma unroll
    for (int e = 0; e < GR_XE; ++e) xr[j][e] = j < nk ? load_x(tile * GR_ROWS, j, e) : 0.f;
    wr[j] = j < nsteps ? load_w1(j) : f32x4{0.f, 0.f, 0.f, 0.f};
    w2r[j] = load_w2(j);
  }

  for (; tile < ntiles; tile += gridDim.x) {
    const int row0 = tile * GR_ROWS;
    f32x16 acc[GR_NT];
#pragma unroll
    for (int n = 0; n < GR_NT; ++n)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[n][i] = 0.f;

    // ---- stage 1: Z1^T (32 units x 64 rows per wave) = W1 x X^T, K = Fp
    // slot 0 was last read before the previous tile's barriers
    stage(0, xr[0]);
    if (GR_RING < nk) {
#pragma unroll
      for (int e = 0; e < GR_XE; ++e) xr[0][e] = load_x(row0, GR_RING, e);
    }
    for (int k0 = 0; k0 < nk; k0 += GR_RING) {
#pragma unroll
      for (int j = 0; j < GR_RING; ++j) {
        const int k = k0 + j;
        if (k < nk) {  // uniform
          // slab k is in slot k & 1; every read of slot (k + 1) & 1 (slab k - 1) is done, and so is
          // (k = 0) every read of the previous tile's G1
          __syncthreads();
          if (k + 1 < nk) {
            stage((j + 1) & 1, xr[(j + 1) & 3]);
            if (k + 1 + GR_RING < nk) {
#pragma unroll
              for (int e = 0; e < GR_XE; ++e) xr[(j + 1) & 3][e] = load_x(row0, k + 1 + GR_RING, e);
            }
          }
          const char* xb = xs[j & 1];
#pragma unroll
          for (int jj = 0; jj < 4; ++jj) {
            const int s = 4 * k + jj;
            if (s < nsteps) {  // uniform
              f32x4 xf[GR_NT];
#pragma unroll
              for (int n = 0; n < GR_NT; ++n)
                xf[n] = *reinterpret_cast<const f32x4*>(xb + xs_off(32 * n + l31, 2 * jj + g));
#pragma unroll
              for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int n = 0; n < GR_NT; ++n)
                  acc[n] = __builtin_amdgcn_mfma_f32_32x32x2f32(wr[jj][e], xf[n][e], acc[n], 0, 0, 0);
              if (s + GR_RING < nsteps) wr[jj] = load_w1(s + GR_RING);
            }
          }
        }
      }
    }
    // the next tile's first slabs (and W1 steps, unless the ring holds all of W1): in flight
    // under the later stages
    const int ntile = tile + (int)gridDim.x;
    if (ntile < ntiles) {
#pragma unroll
      for (int j = 0; j < GR_RING; ++j) {
        if (j < nk) {
#pragma unroll
          for (int e = 0; e < GR_XE; ++e) xr[j][e] = load_x(ntile * GR_ROWS, j, e);
        }
        if (nsteps > GR_RING) wr[j] = load_w1(j);
      }
    }
    // epilogue 1: + b1, relu -> 16 B of the tile per register quad; the mask bits stay here
    unsigned m1 = 0u;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int u = u0 + 8 * q + 4 * g;
      const f32x4 bv = *reinterpret_cast<const f32x4*>(&prm[0][u]);
#pragma unroll
      for (int n = 0; n < GR_NT; ++n) {
        f32x4 h;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          h[r] = fmaxf(acc[n][4 * q + r] + bv[r], 0.f);
          m1 |= (h[r] > 0.f ? 1u : 0u) << (16 * n + 4 * q + r);
        }
        *reinterpret_cast<f32x4*>(ts + t_off(32 * n + l31, u >> 2)) = h;
      }
    }
    __syncthreads();

    // ---- stage 2: Z2^T = W2 x H1^T, K = 256 (32 steps)
#pragma unroll
    for (int n = 0; n < GR_NT; ++n)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[n][i] = 0.f;
#pragma unroll 2
    for (int s0 = 0; s0 < GR_STEPS; s0 += GR_RING) {
#pragma unroll
      for (int j = 0; j < GR_RING; ++j) {
        const int s = s0 + j;
        f32x4 hf[GR_NT];
#pragma unroll
        for (int n = 0; n < GR_NT; ++n)
          hf[n] = *reinterpret_cast<const f32x4*>(ts + t_off(32 * n + l31, 2 * s + g));
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
          for (int n = 0; n < GR_NT; ++n)
            acc[n] = __builtin_amdgcn_mfma_f32_32x32x2f32(w2r[j][e], hf[n][e], acc[n], 0, 0, 0);
        w2r[j] = load_w2((s + GR_RING) & (GR_STEPS - 1));  // wraps: the next tile's first steps
      }
    }
#pragma unroll
    for (int j = 0; j < GR_RING; ++j) gr[j] = load_w2t(j);  // stage 3's first steps, under the head
    // epilogue 2 + head: relu(acc + b2) times w3, summed over this lane's 16 units in unit order
    // (the forward's terms); the accumulator becomes G2 = (acc + b2 > 0) ? w3 : 0
    float hp[GR_NT];
#pragma unroll
    for (int n = 0; n < GR_NT; ++n) hp[n] = 0.f;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int u = u0 + 8 * q + 4 * g;
      const f32x4 bv = *reinterpret_cast<const f32x4*>(&prm[1][u]);
      const f32x4 wv = *reinterpret_cast<const f32x4*>(&prm[2][u]);
#pragma unroll
      for (int n = 0; n < GR_NT; ++n)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float h = fmaxf(acc[n][4 * q + r] + bv[r], 0.f);
          hp[n] += h * wv[r];
          acc[n][4 * q + r] = h > 0.f ? wv[r] : 0.f;
        }
    }
    // the row's two lane halves, then the 8 waves through LDS
#pragma unroll
    for (int n = 0; n < GR_NT; ++n) hp[n] += __shfl_xor(hp[n], 32, 64);
    if (g == 0) {
#pragma unroll
      for (int n = 0; n < GR_NT; ++n) red[wid][32 * n + l31] = hp[n];
    }
    __syncthreads();  // the head partials are in red; every read of H1 is done
    if (threadIdx.x < GR_ROWS) {
      const int grow = row0 + (int)threadIdx.x;
      if (grow < B) {
        float p = red[0][threadIdx.x];
#pragma unroll
        for (int w = 1; w < GR_WAVES; ++w) p += red[w][threadIdx.x];
        pred[grow] = p + bias3;
      }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int n = 0; n < GR_NT; ++n) {
        f32x4 v;
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = acc[n][4 * q + r];
        *reinterpret_cast<f32x4*>(ts + t_off(32 * n + l31, (u0 + 8 * q + 4 * g) >> 2)) = v;
      }
    __syncthreads();

    // ---- stage 3: G1^T = W2^T x G2^T, K = 256 over layer-2 units; this wave's layer-1 units
#pragma unroll
    for (int n = 0; n < GR_NT; ++n)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[n][i] = 0.f;
#pragma unroll 1
    for (int s0 = 0; s0 < GR_STEPS; s0 += GR_RING) {
#pragma unroll
      for (int j = 0; j < GR_RING; ++j) {
        const int s = s0 + j;
        f32x4 gf[GR_NT];
#pragma unroll
        for (int n = 0; n < GR_NT; ++n)
          gf[n] = *reinterpret_cast<const f32x4*>(ts + t_off(32 * n + l31, 2 * s + g));
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
          for (int n = 0; n < GR_NT; ++n)
            acc[n] = __builtin_amdgcn_mfma_f32_32x32x2f32(gr[j][e], gf[n][e], acc[n], 0, 0, 0);
        if (s + GR_RING < GR_STEPS) gr[j] = load_w2t(s + GR_RING);
      }
    }
    // stage 4's first item: its first steps fly under the epilogue and the two barriers
    int item = __builtin_amdgcn_readfirstlane(wid);  // scalar: stage 4's branches are uniform
    int f0 = 32 * (halves ? item >> 1 : item);
    if (item < nitems) {
#pragma unroll
      for (int j = 0; j < GR_RING; ++j) gr[j] = load_w1t(f0, j);
    }
    __syncthreads();  // every read of G2 is done
    // epilogue 3: the layer-1 mask, bit by bit, and G1 over G2
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int n = 0; n < GR_NT; ++n) {
        f32x4 v;
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = (m1 >> (16 * n + 4 * q + r)) & 1u ? acc[n][4 * q + r] : 0.f;
        *reinterpret_cast<f32x4*>(ts + t_off(32 * n + l31, (u0 + 8 * q + 4 * g) >> 2)) = v;
      }
    __syncthreads();

    // ---- stage 4: dX (64 rows x 32 features per block) = G1 x W1, K = 256 over layer-1 units
    for (; item < nitems; item += GR_WAVES) {
      const int nlo = halves ? item & 1 : 0, nhi = halves ? nlo + 1 : GR_NT;  // uniform
#pragma unroll
      for (int n = 0; n < GR_NT; ++n)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[n][i] = 0.f;
#pragma unroll 1
      for (int s0 = 0; s0 < GR_STEPS; s0 += GR_RING) {
#pragma unroll
        for (int j = 0; j < GR_RING; ++j) {
          const int s = s0 + j;
#pragma unroll
          for (int n = 0; n < GR_NT; ++n) {
            if (n >= nlo && n < nhi) {
              const f32x4 gf = *reinterpret_cast<const f32x4*>(ts + t_off(32 * n + l31, 2 * s + g));
#pragma unroll
              for (int e = 0; e < 4; ++e)
                acc[n] = __builtin_amdgcn_mfma_f32_32x32x2f32(gf[e], gr[j][e], acc[n], 0, 0, 0);
            }
          }
          if (s + GR_RING < GR_STEPS) gr[j] = load_w1t(f0, s + GR_RING);
        }
      }
      // output epilogue: accumulator 4 q + r is row 32 n + 8 q + 4 g + r, the lane is the feature
      const int f = f0 + l31;
      const int nitem = item + GR_WAVES;
      const int nf0 = 32 * (halves ? nitem >> 1 : nitem);
      if (nitem < nitems) {
#pragma unroll
        for (int j = 0; j < GR_RING; ++j) gr[j] = load_w1t(nf0, j);
      }
      // (32-bit offsets inside the tile from its uniform base; a whole tile needs no row test)
      float* trow = dX + (size_t)row0 * (size_t)ldg;
      const unsigned ld = (unsigned)ldg, o = (unsigned)(4 * g) * ld + (unsigned)f;
      if (f < F) {
        if (row0 + GR_ROWS <= B) {  // uniform
#pragma unroll
          for (int n = 0; n < GR_NT; ++n) {
            if (n >= nlo && n < nhi) {
#pragma unroll
              for (int i = 0; i < 16; ++i) trow[o + (unsigned)(32 * n + 8 * (i >> 2) + (i & 3)) * ld] = acc[n][i];
            }
          }
        } else {
          int lim = B - row0 - 4 * g;  // this lane's rows 32 n + 8 q + r below lim exist
          // opaque: the 32 row tests are made here, one at a time, not hoisted above the K loop
          // (where their results would be live in scalar registers all through stage 4)
          asm volatile("" : "+v"(lim));
#pragma unroll
          for (int n = 0; n < GR_NT; ++n) {
            if (n >= nlo && n < nhi) {
#pragma unroll
              for (int i = 0; i < 16; ++i) {
                const int ri = 32 * n + 8 * (i >> 2) + (i & 3);
                if (ri < lim) trow[o + (unsigned)ri * ld] = acc[n][i];
              }
            }
          }
        }
      }
      f0 = nf0;
    }
    // red, the tile and the X ring are rewritten only after the next tile's first barrier
  }
}

bool launch_mlp2_grad_f32(const float* X, long ldx, int F, const float* W1, const float* b1, const float* W2,
                          const float* b2, const float* w3, const float* b3, float* pred, float* dX, long ldg, int B,
                          hipStream_t s) {
  const int Fp = (F + 7) / 8 * 8;
  if (F < 1 || Fp > kMlpF32MaxFp || ldx < F || ldg < F || ldg > (1L << 24) || B <= 0) return false;
  for (const void* p : {(const void*)W1, (const void*)W2, (const void*)b1, (const void*)b2, (const void*)w3})
    if (p == nullptr || reinterpret_cast<uintptr_t>(p) % 16 != 0) return false;
  for (const void* p : {(const void*)X, (const void*)b3, (const void*)pred, (const void*)dX})
    if (p == nullptr || reinterpret_cast<uintptr_t>(p) % 4 != 0) return false;
  if (B > INT32_MAX - GR_ROWS) return false;  // row indices of the last tile stay in an int
  const int ntiles = (B + GR_ROWS - 1) / GR_ROWS;
  int dev = 0, cus = 0;
  if (hipGetDevice(&dev) != hipSuccess ||
      hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0)
    cus = 256;
  hipLaunchKernelGGL(mlp2_grad_f32_kernel, dim3(ntiles < cus ? ntiles : cus), dim3(GR_THREADS), 0, s, X, ldx, F, Fp,
                     W1, b1, W2, b2, w3, b3, pred, dX, ldg, B);
  return true;
}

}  // namespace wf
