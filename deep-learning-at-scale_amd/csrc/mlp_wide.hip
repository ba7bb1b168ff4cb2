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
//
// mlp2_fwd_wide_train_kernel is the same tile loop (mlp2_wide_tiles<true>) as the first launch
// of a TRAINING step at these widths (NativeMLP._step_wide). Added per tile:
//  * rows (optional): tile row gr reads data row data_row(rows, gr, nrows) of X and y; every slab
//    a thread stages is then also stored (16 B) to the dense batch Xout, the dW1 GEMM's operand.
//  * the H1 tile is copied out of LDS as 16-B row segments (rows < B) after the head: dW2's
//    operand and the backward's layer-1 ReLU mask.
//  * H2 = bf16(relu(acc + b2)) stays in registers across the head barrier as the bf16 PAIRS it
//    was rounded to (32 registers; as 64 fp32 values the kernel spilled 45). The 128 row
//    threads form d = pred - y, the loss term and dy (MSE, or clipped MAE when clip > 0), write
//    pred and dy and hand dy back to all waves through the column of `red` they alone read.
//  * M2: after that barrier, bit 16m + 4g + r of wave w's word of row 16n + l15 is read off
//    the pairs, OR-ed over the row's 4 lane groups by shuffles, one word stored per row and wave.
//  * dw3 += H2^T dy per tile, reduced over the 16 row lanes by DPP (row16_sum) into the workgroup's
//    LDS sums (one owner lane per unit, no LDS atomics; in registers they spilled); the row
//    threads' loss and db3 sums likewise. At kernel end: one fp32 atomic per unit, one for the
//    loss, one for db3 per workgroup, zeros skipped.
//  * y is requested after layer 2 and lands under the layer-2 epilogue; everything the training
//    epilogue derives from the thread index (M2, dy, sums and copy-out addresses) is formed per
//    tile from one opaque copy of it, so none of it is a loop invariant held in a register
//    across the K loop and layer 2, where all 256 are taken. That is what made the kernel
//    spill-free (12 spills before).
// The prefetch of the next tile is where the scoring kernel has it. Two more barriers per tile.
// Budget of the training instantiation: 89 KB LDS, 256 VGPRs, no scratch, no spills. The scoring
// kernel's report is unchanged. Reports and timings: profiles/r8/mlp_wide_step/README.md.
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

// Sum over the 16 lanes of a DPP row (lanes 16g .. 16g + 15), left in every lane: quad swaps, then
// the half-row and row mirrors. DPP, not __shfl_xor: ds_bpermute keeps one lane-index register per
// distance alive across the whole tile loop.
template <int CTRL>
__device__ __forceinline__ float dpp_f(float x) {
  return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, x), CTRL, 0xF, 0xF, false));
}
__device__ __forceinline__ float row16_sum(float v) {
  v += dpp_f<0xB1>(v);   // quad_perm [1, 0, 3, 2]
  v += dpp_f<0x4E>(v);   // quad_perm [2, 3, 0, 1]
  v += dpp_f<0x141>(v);  // row_half_mirror
  v += dpp_f<0x140>(v);  // row_mirror
  return v;
}

// What the training forward reads and writes beyond the scoring forward (kernels.h
// launch_mlp2_fwd_wide_train); the scoring kernel is handed an empty one and never looks at it.
struct WideTrain {
  const float* y;         // targets, indexed like X's rows
  const long long* rows;  // optional dataset row per batch row (data_row clamps), nrows of them in X
  long nrows;
  bf16_t* Xout;           // with rows: the gathered batch, dense [B][Fp]
  bf16_t* H1;             // [B][256]
  unsigned* M2;           // [B][8] ReLU bits of H2
  float *dy, *dw3, *db3, *loss_sum;
  float dy_scale, clip;   // clip > 0: clipped MAE, else MSE (mlp_step.hip's convention)
};
}  // namespace

// The tile loop of both kernels. TRAIN = false is the scoring kernel, whose code every
// `if constexpr (TRAIN)` below leaves as it was; TRAIN = true adds what WideTrain describes.
template <bool TRAIN>
__device__ __forceinline__ void mlp2_wide_tiles(
    const bf16_t* __restrict__ X, int Fp, const bf16_t* __restrict__ W1, const float* __restrict__ b1,
    const bf16_t* __restrict__ W2, const float* __restrict__ b2, const float* __restrict__ w3,
    const float* __restrict__ b3, float* __restrict__ pred, int B, const WideTrain& t) {
  __shared__ __attribute__((aligned(16))) char h1s[MW_ROWS * MF_H * 2];
  __shared__ __attribute__((aligned(16))) char xs[2][MW_SLAB];
  __shared__ __attribute__((aligned(16))) float prm[3][MF_H];  // b1, b2, w3
  __shared__ float red[MW_WAVES][MW_ROWS];
  // TRAIN: the workgroup's sums over all its tiles, each slot owned by ONE thread (plain
  // read-add-write, no LDS atomics): dw3 of unit u in [u] (lane l15 == 0 of the lane group that
  // holds u), row thread r's loss terms in [256 + r] and its dy in [384 + r]. In LDS, not in
  // registers: 11 more registers live across layer 2 spilled. Unused, and dropped, when !TRAIN.
  __shared__ float sums[TRAIN ? MF_H + 2 * MW_ROWS : 1];

  const int lane = threadIdx.x & 63, l15 = lane & 15, g = lane >> 4;
  const int wid = threadIdx.x >> 6;
  const int u0 = wid * (16 * MW_MT);  // first unit of this wave

  if constexpr (TRAIN) sums[threadIdx.x] = 0.f;  // MF_H + 2 MW_ROWS == MW_THREADS
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
  // TRAIN: element offset of this thread's chunk column in its data row, of the tile whose slabs
  // are being requested (set before a tile's first request; 0 for rows >= B, never dereferenced)
  [[maybe_unused]] size_t xo = 0;
  [[maybe_unused]] auto row_off = [&](int row0) -> size_t {
    const int gr = row0 + sr;
    return gr < B ? data_row(t.rows, gr, t.nrows) * (size_t)Fp + 8 * sc : 0;
  };
  auto load_x = [&](int row0, int k) -> uint4 {
    const int gr = row0 + sr, f0 = 32 * k + 8 * sc;
    if constexpr (TRAIN)
      return (gr < B && f0 + 8 <= Fp) ? *reinterpret_cast<const uint4*>(X + xo + 32 * k) : make_uint4(0, 0, 0, 0);
    else
      return (gr < B && f0 + 8 <= Fp) ? *reinterpret_cast<const uint4*>(X + (size_t)gr * Fp + f0) : make_uint4(0, 0, 0, 0);
  };
  // slab k of the tile at row0 into its LDS slot; TRAIN with rows: also into the dense batch copy
  auto stage = [&](int slot, const uint4& v, int row0, int k) {
    *reinterpret_cast<uint4*>(xs[slot] + soff) = v;
    if constexpr (TRAIN) {
      int gr = row0 + sr;
      const int f0 = 32 * k + 8 * sc;
      // opaque: the 64-bit address is formed at each store, not kept across the K loop (a
      // register pair there spilled a W2 fragment)
      asm volatile("" : "+v"(gr));
      if (t.Xout != nullptr && gr < B && f0 + 8 <= Fp)
        *reinterpret_cast<uint4*>(t.Xout + (size_t)gr * Fp + f0) = v;
    }
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
  if constexpr (TRAIN) xo = row_off(tile * MW_ROWS);
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
    stage(0, xr[0], row0, 0);
    if (MW_RING < nk) xr[0] = load_x(row0, MW_RING);
    for (int k0 = 0; k0 < nk; k0 += MW_RING) {
#pragma unroll
      for (int j = 0; j < MW_RING; ++j) {
        const int k = k0 + j;
        if (k < nk) {  // uniform
          // slab k is in slot k & 1; every read of slot (k + 1) & 1 (step k - 1) is done
          __syncthreads();
          if (k + 1 < nk) {
            stage((j + 1) & 1, xr[(j + 1) & 3], row0, k + 1);
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
      if constexpr (TRAIN) xo = row_off(ntile * MW_ROWS);  // this tile's requests are all issued
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
    // TRAIN: H2 stays in registers (dw3 needs it once dy is known) as the bf16 pairs it was
    // rounded to, 32 registers where the fp32 accumulators are 64 (kept as fp32, the kernel
    // spilled); the mask bits are read off the pairs after the barrier, where less is live
    float hp[MW_NT];
    [[maybe_unused]] unsigned h2p[MW_MT][MW_NT][2];
    [[maybe_unused]] float yv = 0.f;  // TRAIN: the row threads' target, requested here: it lands under this epilogue
    // TRAIN: the thread index as the training epilogue sees it, opaque once per tile: what it
    // derives from it (row, unit and segment addresses of M2, dy, the sums, the H1 copy-out) is
    // formed here each tile, not kept as loop invariants across the MFMA loops, where every
    // register is taken
    [[maybe_unused]] int tt = threadIdx.x;
    if constexpr (TRAIN) {
      asm volatile("" : "+v"(tt));
      if (tt < MW_ROWS && row0 + tt < B) yv = t.y[data_row(t.rows, row0 + tt, t.nrows)];
    }
    [[maybe_unused]] const int tl15 = tt & 15, tg = (tt >> 4) & 3, tu0 = (tt >> 6) * (16 * MW_MT);
#pragma unroll
    for (int n = 0; n < MW_NT; ++n) hp[n] = 0.f;
#pragma unroll
    for (int m = 0; m < MW_MT; ++m) {
      const f32x4 bv = *reinterpret_cast<const f32x4*>(&prm[1][u0 + 16 * m + 4 * g]);
      const f32x4 wv = *reinterpret_cast<const f32x4*>(&prm[2][u0 + 16 * m + 4 * g]);
#pragma unroll
      for (int n = 0; n < MW_NT; ++n)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          if constexpr (TRAIN) {
            const bf16_t hb = f2bf(fmaxf(acc[m][n][r] + bv[r], 0.f));
            const float v = bf2f(hb);
            hp[n] += v * wv[r];
            h2p[m][n][r >> 1] = (r & 1) ? h2p[m][n][r >> 1] | ((unsigned)hb << 16) : (unsigned)hb;
            // opaque: the compiler otherwise sees through the pair and keeps 64 fp32 values
            if (r & 1) asm volatile("" : "+v"(h2p[m][n][r >> 1]));
          } else {
            hp[n] += bf2f(f2bf(fmaxf(acc[m][n][r] + bv[r], 0.f))) * wv[r];
          }
        }
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
      [[maybe_unused]] float gy = 0.f;
      if (gr < B) {
        float p = red[0][threadIdx.x];
#pragma unroll
        for (int w = 1; w < MW_WAVES; ++w) p += red[w][threadIdx.x];
        pred[gr] = p + bias3;
        if constexpr (TRAIN) {
          const float d = (p + bias3) - yv;
          float per;
          if (t.clip > 0.f) {
            per = fminf(fabsf(d), t.clip);
            gy = fabsf(d) <= t.clip ? t.dy_scale * (d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f)) : 0.f;
          } else {
            per = d * d;
            gy = t.dy_scale * d;
          }
          t.dy[row0 + tt] = gy;
          sums[MF_H + tt] += per;
          sums[MF_H + MW_ROWS + tt] += gy;
        }
      }
      // dy of the tile's rows (0 past B) back to every wave, in the column of red that only
      // this thread has read
      if constexpr (TRAIN) red[0][tt] = gy;
    }
    if constexpr (TRAIN) {
      // M2: this wave's 32 units are word wid of the row's 8 mask words. Bit 16m + 4g + r of row
      // 16n + l15 is H2 > 0 (a relu'd bf16: its 16 bits as a signed number are > 0); the row's 4
      // lane groups are OR-ed by shuffles, then group g stores the words of rows 16g + l15 and
      // 16(g + 4) + l15 (one predicated store per n: picking the word by a select chain over g
      // became an indexed stack array, i.e. scratch)
#pragma unroll
      for (int n = 0; n < MW_NT; ++n) {
        unsigned bw = 0u;
#pragma unroll
        for (int m = 0; m < MW_MT; ++m)
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if ((short)(h2p[m][n][r >> 1] >> (16 * (r & 1))) > 0) bw |= 1u << (16 * m + 4 * tg + r);
        bw |= (unsigned)__shfl_xor((int)bw, 16, 64);
        bw |= (unsigned)__shfl_xor((int)bw, 32, 64);
        const int gr = row0 + 16 * n + tl15;
        if ((n & 3) == tg && gr < B) t.M2[(size_t)gr * 8 + (tt >> 6)] = bw;
      }
      __syncthreads();
      // dw3 of this tile: H2 times dy over the lane's 8 rows, then over the 16 lanes l15
      // of the lane group, which hold the same 4 units of other rows
      float dyn[MW_NT];
#pragma unroll
      for (int n = 0; n < MW_NT; ++n) dyn[n] = red[0][16 * n + tl15];
#pragma unroll
      for (int m = 0; m < MW_MT; ++m)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float v = 0.f;
#pragma unroll
          for (int n = 0; n < MW_NT; ++n) v += bf2f((bf16_t)(h2p[m][n][r >> 1] >> (16 * (r & 1)))) * dyn[n];
          v = row16_sum(v);
          if (tl15 == 0) sums[tu0 + 16 * m + 4 * tg + r] += v;
        }
      // H1 tile -> HBM as 16-B row segments (a row's 512 B from 32 consecutive threads); the
      // accumulators are dead, and h1s is rewritten only after the next tile's K-loop barriers
#pragma unroll 2
      for (int i = 0; i < MW_ROWS * 32 / MW_THREADS; ++i) {
        const int seg = i * MW_THREADS + tt, r = seg >> 5, c = seg & 31, gr = row0 + r;
        if (gr < B)
          *reinterpret_cast<uint4*>(t.H1 + (size_t)gr * MF_H + 8 * c) =
              *reinterpret_cast<const uint4*>(h1s + tile_off(r, 8 * c));
      }
    }
    // red, h1s and the X ring are rewritten only after the next tile's first barrier
  }
  if constexpr (TRAIN) {
    // one fp32 atomic per unit, and one each for the loss and db3, per workgroup; zeros skipped
    __syncthreads();
    const float v = sums[threadIdx.x];
    if (threadIdx.x < MF_H && v != 0.f) atomicAdd(t.dw3 + threadIdx.x, v);
    // red[1] is free: its last readers (the row threads' head sum) passed a barrier since
    const float ls = block_sum<MW_THREADS>(threadIdx.x >= MF_H && threadIdx.x < MF_H + MW_ROWS ? v : 0.f, red[1]);
    if (threadIdx.x == 0 && ls != 0.f) atomicAdd(t.loss_sum, ls);
    const float t3 = block_sum<MW_THREADS>(threadIdx.x >= MF_H + MW_ROWS ? v : 0.f, red[1]);
    if (threadIdx.x == 0 && t3 != 0.f) atomicAdd(t.db3, t3);
  }
}

__global__ __launch_bounds__(MW_THREADS, 1) void mlp2_fwd_wide_kernel(
    const bf16_t* __restrict__ X, int Fp, const bf16_t* __restrict__ W1, const float* __restrict__ b1,
    const bf16_t* __restrict__ W2, const float* __restrict__ b2, const float* __restrict__ w3,
    const float* __restrict__ b3, float* __restrict__ pred, int B) {
  mlp2_wide_tiles<false>(X, Fp, W1, b1, W2, b2, w3, b3, pred, B, WideTrain{});
}

__global__ __launch_bounds__(MW_THREADS, 1) void mlp2_fwd_wide_train_kernel(
    const bf16_t* __restrict__ X, int Fp, const bf16_t* __restrict__ W1, const float* __restrict__ b1,
    const bf16_t* __restrict__ W2, const float* __restrict__ b2, const float* __restrict__ w3,
    const float* __restrict__ b3, float* __restrict__ pred, int B, WideTrain t) {
  mlp2_wide_tiles<true>(X, Fp, W1, b1, W2, b2, w3, b3, pred, B, t);
}

namespace {
int wide_grid(int B) {  // one workgroup per CU at most, one per tile at least
  const int ntiles = (B + MW_ROWS - 1) / MW_ROWS;
  int dev = 0, cus = 0;
  if (hipGetDevice(&dev) != hipSuccess ||
      hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0)
    cus = 256;
  return ntiles < cus ? ntiles : cus;
}
}  // namespace

bool launch_mlp2_fwd_wide_train(const bf16_t* X, int Fp, const bf16_t* W1, const float* b1, const bf16_t* W2,
                                const float* b2, const float* w3, const float* b3, const float* y,
                                const long long* rows, long nrows, bf16_t* Xout, bf16_t* H1, unsigned* M2, float* pred,
                                float* dy, float* dw3, float* db3, float* loss_sum, float dy_scale, float clip, int B,
                                hipStream_t s) {
  if (Fp % 8 != 0 || Fp < 8 || Fp > kMlpWideMaxFp || B <= 0) return false;
  if (rows != nullptr && (Xout == nullptr || nrows <= 0)) return false;
  for (const void* p : {(const void*)X, (const void*)W1, (const void*)W2, (const void*)H1, (const void*)Xout})
    if (reinterpret_cast<uintptr_t>(p) % 16 != 0) return false;
  for (const void* p : {(const void*)y, (const void*)H1, (const void*)M2, (const void*)pred, (const void*)dy,
                        (const void*)dw3, (const void*)db3, (const void*)loss_sum})
    if (p == nullptr) return false;
  const WideTrain t{y, rows, nrows, rows != nullptr ? Xout : nullptr, H1, M2, dy, dw3, db3, loss_sum, dy_scale, clip};
  hipLaunchKernelGGL(mlp2_fwd_wide_train_kernel, dim3(wide_grid(B)), dim3(MW_THREADS), 0, s, X, Fp, W1, b1, W2, b2, w3,
                     b3, pred, B, t);
  return true;
}

bool launch_mlp2_fwd_wide(const bf16_t* X, int Fp, const bf16_t* W1, const float* b1, const bf16_t* W2,
                          const float* b2, const float* w3, const float* b3, float* pred, int B, hipStream_t s) {
  if (Fp % 8 != 0 || Fp < 8 || Fp > kMlpWideMaxFp || B <= 0) return false;
  for (const void* p : {(const void*)X, (const void*)W1, (const void*)W2})
    if (reinterpret_cast<uintptr_t>(p) % 16 != 0) return false;
  hipLaunchKernelGGL(mlp2_fwd_wide_kernel, dim3(wide_grid(B)), dim3(MW_THREADS), 0, s, X, Fp, W1, b1, W2, b2, w3, b3,
                     pred, B);
  return true;
}

}  // namespace wf
