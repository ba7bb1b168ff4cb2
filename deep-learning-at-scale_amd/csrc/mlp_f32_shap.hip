// wellflow — fused fp32 exact Shapley attribution of the F -> 256 -> 256 -> 1 MLP: per row x and
// 1 <= K <= 12 picked input columns (feature spans), against ONE baseline row x' shared by all rows,
//   phi_c = sum over the 2^K coalitions S of  p(S) * (c in S ? w_in[|S|] : -w_out[|S|]),
//   p(S)  = f(own values on the spans of S, x' on the other picked spans, own values elsewhere),
// with 1 <= F, Fp <= 512 padded features; fp32 operands and fp32 accumulation on
// v_mfma_f32_32x32x2_f32, fp32 master weights, no bf16 anywhere; the sum over coalitions in fp64.
//
// Why a kernel of its own: layer 1 is linear, so for x~ = x with every picked span set to x'
//   z1(S) = z0 + sum_{c in S} D_c,   z0 = b1 + W1 x~,   D_c = W1[:, span_c] (x - x')[span_c],
// and the F-deep product runs K + 1 times per row, not 2^K times. A coalition then costs a few
// vector adds, the 256 x 256 layer and the head. 2^K launches of assembly + mlp_f32.hip would run
// layer 1 2^K times and keep 2^K x B predictions; here only K + 2 numbers per row leave the kernel.
//
// Split, tile, swizzles and K order are mlp_f32.hip's: one workgroup of 512 threads (8 waves, two
// per SIMD) per CU, grid-stride over 64-row tiles; wave w owns units [32w, 32w + 32) of BOTH hidden
// layers and all 64 rows of an MFMA tile (A = weights, lane = unit; B = activations, lane = row);
// in K step s lane half g = lane / 32 holds k = 8s + 4g + e and MFMA e multiplies k = 8s + e and
// 8s + 4 + e.
//
// Stages:
//  0. once per workgroup: x', b1, b2, w3, the spans and the weights -> LDS; col[f] = the picked
//     column that owns feature f, or -1.
//  1. once per 64-row tile, K + 1 passes over layer 1. Pass 0: z0 = (W1 x x~^T) + b1 over all Fp
//     features, x~ chosen per feature while the slab is staged (col[f] >= 0 ? x' : x). Pass c + 1:
//     D_c over the slabs and K steps that meet span c only, the slab staged as fl(x - x') inside
//     the span and 0 outside, so a span needs no alignment to a K step or a slab. Each pass writes
//     its 64 x 256 result to the workgroup's own slab [K + 1][64][256] of the scratch buffer.
//     K + 1 KB per row, written once and read once: no LDS or register budget holds it at K = 12
//     (64 rows x 13 KB), and against 2^K evaluations the traffic is nothing. The passes are not
//     pipelined (one LDS slot, two barriers per slab, W1 fragments loaded where they are used):
//     stage 1 is (K + 1) Fp / (2^K 256) of the coalition loop's MFMAs, 1 % at K = 9 and Fp = 128.
//  2. the coalition loop, per sub-group of 4 real rows: their z0 / D_c (4 (K + 1) KB, 52 KB at
//     K = 12) go from the slab to LDS once. An MFMA tile's 64 rows are 4 real rows x 16 coalitions
//     i = 16 t + j, virtual row 16 r + j. Building H1: thread (r, 16-B chunk, half) forms the
//     prefix z0 + D_c over the set bits of t (columns K - 1 .. 4, descending: shared by the 16
//     coalitions of the step), then adds D_3 .. D_0 by the bits of j, one fp32 add each, relu, and
//     writes 8 rows of the swizzled 64 KB tile. The values of step t + 1 are formed in 32
//     registers before the MFMAs of step t are issued, so their LDS reads and adds run under them;
//     the tile itself is single (two tiles and the resident rows pass 160 KB). Layer 2 streams W2
//     from L2 through the 4-deep register ring (it wraps from step to step), the head is taken
//     from the accumulators and summed over the waves through LDS, in wave order: p(S) per virtual
//     row, in wave 0, lane = virtual row.
//  3. the rule: lane 16 r + c of wave 0 owns phi_c of real row r, ONE fp64 register: for j = 0 ..
//     15 it takes p(16 t + j) of its row by a shuffle and adds (double)p * w, one multiply and one
//     add, never an fma, in ascending i. (One lane per row AND column, not per row: the K sums of
//     a row are independent, and one register needs no indexing.) K < 4: a step holds 2^K
//     coalitions, the other virtual rows repeat them and are dropped.
//
// The value of a coalition does not depend on the walk: every z1(S) is z0 plus its members' D_c in
// descending column index. A row's arithmetic does not depend on its tile, its position or B.
//
// Written: phi[c][row], p0[row] (coalition 0), pfull[row] (coalition 2^K - 1), row < B; p_out[i][row]
// when it is given; the workgroup's scratch slab. Nothing else, no atomics.
//
// Budget: LDS 64 KB tile + 52 KB resident rows + 8 KB X slab + 3 KB b1 / b2 / w3 + 2 KB x' + 2 KB
// head partials + spans, weights and col = 132 KB of 160 KB. Registers per lane: 32 accumulators,
// 32 values of the next H1 tile, the 16-value W2 ring, 8 fragment values, 16 of D_0 .. D_3 while a
// tile is built. The compiler's report (no scratch memory, no spills) is in
// profiles/r12/mlp_f32_shap/README.md. _build.py SOURCE_FLAGS compiles this file with the packed
// fp32 VALU forms switched off.
#include "common.h"
#include "kernels.h"

namespace wf {

namespace {
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int SH_H = 256;
constexpr int SH_ROWS = kMlpF32Rows;    // rows per tile, real (stage 1) and virtual (the coalition loop)
constexpr int SH_NT = SH_ROWS / 32;     // N tiles (32 rows) per wave
constexpr int SH_THREADS = 512;
constexpr int SH_WAVES = SH_THREADS / kWave;
constexpr int SH_XE = SH_ROWS * 32 / SH_THREADS;  // values per thread and slab
constexpr int SH_RING = 4;              // W2 register ring depth
constexpr int SH_STEPS = SH_H / 8;      // K steps of the 256-deep product
constexpr int SH_R = 4;                 // real rows per sub-group
constexpr int SH_C = SH_ROWS / SH_R;    // coalitions per step
constexpr int SH_MAXK = kMlpShapMaxCols;
static_assert(SH_H == 32 * SH_WAVES, "a wave owns 32 units");
static_assert(SH_XE * SH_THREADS == SH_ROWS * 32 && SH_THREADS / 32 == 16, "staging: 16 rows per pass");
static_assert(kMlpF32MaxFp <= SH_THREADS, "x' and col are staged by one thread per feature");
static_assert(SH_C == 16 && SH_WAVES == 2 * SH_R, "a wave builds 8 coalitions of one real row; 4 low columns");

// byte offset of 16-B chunk `chunk` of a row: the H1 tile (64 chunks per row) and the X slab (8)
__device__ __forceinline__ int t_off(int row, int chunk) { return row * (SH_H * 4) + ((chunk ^ (row & 15)) << 4); }
__device__ __forceinline__ int xs_off(int row, int chunk) { return row * 128 + ((chunk ^ ((row >> 1) & 7)) << 4); }

__device__ __forceinline__ double shap_add(double phi, float p, double w) {
#pragma clang fp contract(off)
  const double t = (double)p;
  return phi + t * w;
}

int shap_grid(int B) {
  const int ntiles = (B + SH_ROWS - 1) / SH_ROWS;
  int dev = 0, cus = 0;
  if (hipGetDevice(&dev) != hipSuccess ||
      hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0)
    cus = 256;
  return ntiles < cus ? ntiles : cus;
}
}  // namespace

__global__ __launch_bounds__(SH_THREADS, 1) void mlp2_shapley_f32_kernel(
    const float* __restrict__ X, long ldx, int F, int Fp, const float* __restrict__ xbase,
    const float* __restrict__ W1, const float* __restrict__ b1, const float* __restrict__ W2,
    const float* __restrict__ b2, const float* __restrict__ w3, const float* __restrict__ b3, const ShapleyPlan plan,
    float* scratch, double* __restrict__ phi, long ldo, float* __restrict__ p0,
    float* __restrict__ pfull, float* __restrict__ p_out, long ldp, int B) {
  __shared__ __attribute__((aligned(16))) char ts[SH_ROWS * SH_H * 4];         // H1 of 64 virtual rows
  __shared__ __attribute__((aligned(16))) char xs[SH_ROWS * 128];              // one X slab
  __shared__ __attribute__((aligned(16))) float res[SH_MAXK + 1][SH_R][SH_H];  // z0, D_0 .. of a sub-group
  __shared__ __attribute__((aligned(16))) float prm[3][SH_H];                  // b1, b2, w3
  __shared__ __attribute__((aligned(16))) float xbs[kMlpF32MaxFp];             // the baseline row, zero past F
  __shared__ float red[SH_WAVES][SH_ROWS];
  __shared__ double cf[2][SH_MAXK + 1];  // w_in, w_out
  __shared__ int soff[SH_MAXK], ssize[SH_MAXK];
  __shared__ signed char col[kMlpF32MaxFp];

  const int lane = threadIdx.x & 63, l31 = lane & 31, g = lane >> 5;
  const int wid = threadIdx.x >> 6;
  const int u0 = 32 * wid;  // first unit of this wave
  const int K = plan.K;

  const int nk = (Fp + 31) >> 5;  // X slabs of 32 features
  const int nsteps = Fp >> 3;     // K steps of 8 features in layer 1
  const int ntiles = (B + SH_ROWS - 1) / SH_ROWS;
  const int nt = K > 4 ? 1 << (K - 4) : 1;      // steps of 16 coalitions
  const int ncoal = K >= 4 ? SH_C : 1 << K;     // coalitions of a step that exist
  const int last = (1 << K) - 1;

  // ---- stage 0
  if (threadIdx.x == 0) {  // constant indices: the plan is read from the kernel arguments in place
#pragma unroll
    for (int c = 0; c < SH_MAXK; ++c) {
      soff[c] = plan.off[c];
      ssize[c] = plan.size[c];
    }
#pragma unroll
    for (int s = 0; s <= SH_MAXK; ++s) {
      cf[0][s] = plan.coef[0][s];
      cf[1][s] = plan.coef[1][s];
    }
  }
  xbs[threadIdx.x] = (int)threadIdx.x < F ? xbase[threadIdx.x] : 0.f;
  if (threadIdx.x < SH_H) {
    prm[0][threadIdx.x] = b1[threadIdx.x];
    prm[1][threadIdx.x] = b2[threadIdx.x];
    prm[2][threadIdx.x] = w3[threadIdx.x];
  }
  const float bias3 = b3[0];
  __syncthreads();
  {
    int c_of = -1;
    for (int c = 0; c < K; ++c)
      if ((int)threadIdx.x >= soff[c] && (int)threadIdx.x < soff[c] + ssize[c]) c_of = c;
    col[threadIdx.x] = (signed char)c_of;  // read after stage 1's first barrier
  }

  // staging: value j of a slab is row 16 j + (t >> 5), feature t & 31
  const int sr = threadIdx.x >> 5, sf = threadIdx.x & 31;
  // A fragments: unit u0 + l31, k = 8 s + 4 g .. + 3
  const float* w1p = W1 + (size_t)(u0 + l31) * Fp + 4 * g;
  const float* w2p = W2 + (size_t)(u0 + l31) * SH_H + 4 * g;
  auto load_w1 = [&](int s) -> f32x4 {
    f32x4 v = *reinterpret_cast<const f32x4*>(w1p + 8 * s);
    const int k0 = 8 * s + 4 * g;
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = k0 + e < F ? v[e] : 0.f;
    return v;
  };
  auto load_w2 = [&](int s) -> f32x4 { return *reinterpret_cast<const f32x4*>(w2p + 8 * s); };
  f32x4 w2r[SH_RING];  // the W2 fragment of step s in w2r[s & 3]; wraps from one coalition step into the next
#pragma unroll
  for (int j = 0; j < SH_RING; ++j) w2r[j] = load_w2(j);

  // the H1 build: this wave's real row of the sub-group and half of the step's coalitions; lane = chunk
  const int br = wid & (SH_R - 1), bh = wid >> 2;
  auto resv = [&](int c) -> f32x4 { return *reinterpret_cast<const f32x4*>(&res[c][br][4 * lane]); };
  auto build = [&](int t, f32x4 (&hv)[8]) {
    f32x4 q = resv(0);
    for (int c = K - 1; c >= 4; --c)  // the step's shared prefix, descending column index
      if ((t >> (c - 4)) & 1) q += resv(c + 1);
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    const f32x4 d0 = resv(1), d1 = K > 1 ? resv(2) : zero, d2 = K > 2 ? resv(3) : zero, d3 = K > 3 ? resv(4) : zero;
    if (K > 3 && bh) q += d3;
#pragma unroll
    for (int jj = 0; jj < 8; ++jj) {  // coalition j = 8 bh + jj of the step
      f32x4 v = q;
      if (K > 2 && (jj & 4)) v += d2;
      if (K > 1 && (jj & 2)) v += d1;
      if (jj & 1) v += d0;
#pragma unroll
      for (int e = 0; e < 4; ++e) hv[jj][e] = fmaxf(v[e], 0.f);
    }
  };

  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int row0 = tile * SH_ROWS;
    // this workgroup's slab: every read of the previous tile's values is behind a barrier
    float* slab = scratch + (size_t)blockIdx.x * (size_t)(K + 1) * (SH_ROWS * SH_H);
    f32x16 acc[SH_NT];

    // ---- stage 1: pass 0 is z0, pass c + 1 is D_c (32 units x 64 rows per wave each)
#pragma unroll 1
    for (int c = 0; c <= K; ++c) {
      const int flo = c == 0 ? 0 : soff[c - 1], fhi = c == 0 ? Fp : flo + ssize[c - 1];
      const int klo = flo >> 5, khi = (fhi + 31) >> 5;
      const int slo = flo >> 3, shi = min((fhi + 7) >> 3, nsteps);
#pragma unroll
      for (int n = 0; n < SH_NT; ++n)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[n][i] = 0.f;
#pragma unroll 1
      for (int k = klo; k < khi; ++k) {
        __syncthreads();  // every read of the slab before this one is done
        {
          const int f = 32 * k + sf;
          const float xb = xbs[f];
          const int cf_ = col[f];
#pragma unroll
          for (int j = 0; j < SH_XE; ++j) {
            const int gr = row0 + 16 * j + sr;
            const float x = (gr < B && f < F) ? X[(size_t)gr * (size_t)ldx + f] : 0.f;
            const float v = c == 0 ? (cf_ >= 0 ? xb : x) : (cf_ == c - 1 ? x - xb : 0.f);  // one fp32 subtraction
            *reinterpret_cast<float*>(xs + xs_off(16 * j + sr, sf >> 2) + 4 * (sf & 3)) = v;
          }
        }
        __syncthreads();
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
          const int s = 4 * k + jj;
          if (s >= slo && s < shi) {  // uniform
            const f32x4 wf = load_w1(s);
            f32x4 xf[SH_NT];
#pragma unroll
            for (int n = 0; n < SH_NT; ++n)
              xf[n] = *reinterpret_cast<const f32x4*>(xs + xs_off(32 * n + l31, 2 * jj + g));
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
              for (int n = 0; n < SH_NT; ++n)
                acc[n] = __builtin_amdgcn_mfma_f32_32x32x2f32(wf[e], xf[n][e], acc[n], 0, 0, 0);
          }
        }
      }
      // a register quad is 4 consecutive units of one row -> 16 B of the slab; + b1 in pass 0 only
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int u = u0 + 8 * q + 4 * g;
        const f32x4 bv = *reinterpret_cast<const f32x4*>(&prm[0][u]);
#pragma unroll
        for (int n = 0; n < SH_NT; ++n) {
          f32x4 v;
#pragma unroll
          for (int r = 0; r < 4; ++r) v[r] = c == 0 ? acc[n][4 * q + r] + bv[r] : acc[n][4 * q + r];
          *reinterpret_cast<f32x4*>(slab + (size_t)(c * SH_ROWS + 32 * n + l31) * SH_H + u) = v;
        }
      }
    }

    // ---- the coalition loop, 4 real rows at a time
#pragma unroll 1
    for (int sg = 0; sg < SH_ROWS / SH_R; ++sg) {
      const int r0 = row0 + SH_R * sg;
      if (r0 >= B) break;  // uniform
      __syncthreads();     // the slab is written (first sub-group); every read of res is done
      for (int idx = threadIdx.x; idx < (K + 1) * (SH_R * SH_H / 4); idx += SH_THREADS) {
        const int c = idx >> 8, r = (idx >> 6) & (SH_R - 1), ch = idx & 63;
        *reinterpret_cast<f32x4*>(&res[c][r][4 * ch]) =
            *reinterpret_cast<const f32x4*>(slab + (size_t)(c * SH_ROWS + SH_R * sg + r) * SH_H + 4 * ch);
      }
      __syncthreads();
      f32x4 hv[8];
      build(0, hv);
      double ph = 0.0;  // wave 0, lane 16 r + c: phi_c of real row r

#pragma unroll 1
      for (int t = 0; t < nt; ++t) {
        // every read of the tile is behind the previous step's last barrier
#pragma unroll
        for (int jj = 0; jj < 8; ++jj)
          *reinterpret_cast<f32x4*>(ts + t_off(SH_C * br + 8 * bh + jj, lane)) = hv[jj];
        __syncthreads();
        if (t + 1 < nt) build(t + 1, hv);  // under this step's MFMAs

        // layer 2: Z2^T = W2 x H1^T, K = 256 (32 steps)
#pragma unroll
        for (int n = 0; n < SH_NT; ++n)
#pragma unroll
          for (int i = 0; i < 16; ++i) acc[n][i] = 0.f;
#pragma unroll 2
        for (int s0 = 0; s0 < SH_STEPS; s0 += SH_RING) {
#pragma unroll
          for (int j = 0; j < SH_RING; ++j) {
            const int s = s0 + j;
            f32x4 hf[SH_NT];
#pragma unroll
            for (int n = 0; n < SH_NT; ++n)
              hf[n] = *reinterpret_cast<const f32x4*>(ts + t_off(32 * n + l31, 2 * s + g));
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
              for (int n = 0; n < SH_NT; ++n)
                acc[n] = __builtin_amdgcn_mfma_f32_32x32x2f32(w2r[j][e], hf[n][e], acc[n], 0, 0, 0);
            w2r[j] = load_w2((s + SH_RING) & (SH_STEPS - 1));  // wraps: the next step's first fragments
          }
        }
        // epilogue 2 + head, as mlp_f32.hip: relu(acc + b2) times w3 over this lane's 16 units in unit order
        float hp[SH_NT];
#pragma unroll
        for (int n = 0; n < SH_NT; ++n) hp[n] = 0.f;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int u = u0 + 8 * q + 4 * g;
          const f32x4 bv = *reinterpret_cast<const f32x4*>(&prm[1][u]);
          const f32x4 wv = *reinterpret_cast<const f32x4*>(&prm[2][u]);
#pragma unroll
          for (int n = 0; n < SH_NT; ++n)
#pragma unroll
            for (int r = 0; r < 4; ++r) hp[n] += fmaxf(acc[n][4 * q + r] + bv[r], 0.f) * wv[r];
        }
#pragma unroll
        for (int n = 0; n < SH_NT; ++n) hp[n] += __shfl_xor(hp[n], 32, 64);
        if (g == 0) {
#pragma unroll
          for (int n = 0; n < SH_NT; ++n) red[wid][32 * n + l31] = hp[n];
        }
        __syncthreads();

        // wave 0, lane = virtual row 16 r + j: p(S_i), i = 16 t + j, of real row r0 + r
        if (wid == 0) {  // red is rewritten only behind the next step's first barrier
          float p = red[0][lane];
#pragma unroll
          for (int w = 1; w < SH_WAVES; ++w) p += red[w][lane];
          p += bias3;
          const int jl = lane & (SH_C - 1), row = r0 + (lane >> 4), i = SH_C * t + jl;
          if (row < B && jl < ncoal) {
            if (p_out != nullptr) p_out[(size_t)i * (size_t)ldp + row] = p;
            if (i == 0) p0[row] = p;
            if (i == last) pfull[row] = p;
          }
          // the rule: this lane is column jl of its row; coalitions in ascending i
          for (int j = 0; j < ncoal; ++j) {
            const float pj = __shfl(p, (lane & ~(SH_C - 1)) + j, 64);
            const int ii = SH_C * t + j, s = __popc(ii);
            ph = shap_add(ph, pj, (ii >> jl) & 1 ? cf[0][s] : -cf[1][s]);
          }
        }
      }
      if (wid == 0) {
        const int c = lane & (SH_C - 1), row = r0 + (lane >> 4);
        if (c < K && row < B) phi[(size_t)c * (size_t)ldo + row] = ph;
      }
    }
    __syncthreads();  // every read of the slab is done before the next tile's stage 1 rewrites it
  }
}

size_t mlp2_shapley_scratch_floats(int B, int K) {
  if (B <= 0 || K < 1 || K > SH_MAXK) return 0;
  return (size_t)shap_grid(B) * (size_t)(K + 1) * (SH_ROWS * SH_H);
}

const char* launch_mlp2_shapley_f32(const float* X, long ldx, int F, const float* xb, const float* W1, const float* b1,
                                    const float* W2, const float* b2, const float* w3, const float* b3, int K,
                                    const int* off, const int* size, const double* coef, float* scratch,
                                    size_t scratch_floats, double* phi, long ldo, float* p0, float* pfull, float* p_out,
                                    long ldp, int B, hipStream_t s) {
  const int Fp = (F + 7) / 8 * 8;
  if (F < 1 || Fp > kMlpF32MaxFp) return "F outside 1 .. 512 after padding to a multiple of 8";
  if (K < 1 || K > SH_MAXK) return "the number of picked columns is outside 1 .. 12";
  if (B <= 0 || B > INT32_MAX - SH_ROWS) return "the row count is outside 1 .. 2^31 - 65";
  if (ldx < F || ldo < B || (p_out != nullptr && ldp < B)) return "a row stride is shorter than its row";
  if (off == nullptr || size == nullptr || coef == nullptr) return "the spans or the weights are missing";
  ShapleyPlan plan = {};
  plan.K = K;
  int end = 0;  // source order and disjoint: every span starts at or after the end of the one before
  for (int c = 0; c < K; ++c) {
    if (size[c] < 1 || off[c] < end || off[c] > F - size[c])
      return "a span is empty, outside [0, F), overlaps another or is out of source order";
    plan.off[c] = off[c];
    plan.size[c] = size[c];
    end = off[c] + size[c];
  }
  for (int i = 0; i <= K; ++i) {
    plan.coef[0][i] = coef[i];
    plan.coef[1][i] = coef[K + 1 + i];
  }
  for (const void* p : {(const void*)W1, (const void*)W2, (const void*)b1, (const void*)b2, (const void*)w3,
                        (const void*)scratch})
    if (p == nullptr || reinterpret_cast<uintptr_t>(p) % 16 != 0)
      return "a weight view or the scratch buffer is null or not 16-byte aligned";
  for (const void* p : {(const void*)X, (const void*)xb, (const void*)b3, (const void*)p0, (const void*)pfull})
    if (p == nullptr || reinterpret_cast<uintptr_t>(p) % 4 != 0) return "an fp32 operand is null or misaligned";
  if (phi == nullptr || reinterpret_cast<uintptr_t>(phi) % 8 != 0) return "phi is null or misaligned";
  if (p_out != nullptr && reinterpret_cast<uintptr_t>(p_out) % 4 != 0) return "p_out is misaligned";
  if (scratch_floats < mlp2_shapley_scratch_floats(B, K)) return "the scratch buffer is too small";
  hipLaunchKernelGGL(mlp2_shapley_f32_kernel, dim3(shap_grid(B)), dim3(SH_THREADS), 0, s, X, ldx, F, Fp, xb, W1, b1, W2,
                     b2, w3, b3, plan, scratch, phi, ldo, p0, pfull, p_out, ldp, B);
  return nullptr;
}

}  // namespace wf
