// wellflow — conformal scores and their exact per-group order statistics on the device (gfx950):
// what a calibration run of the prediction-interval job (wellflow/interval.py) does with the
// predictions of its one scoring pass, instead of a D2H copy, a numpy score and a sort per group.
//
// abs_scores. For predictions in standardised target units and the raw target,
//   v = (double)pred * y_scale + y_shift,  d = v - (double)y          (err_sums' d, score.hip)
//   out[i] = (float)fabs(d)                 absolute mode
//   out[i] = (float)(fabs(d) / fabs(v))     relative mode (IEEE: x / 0 is inf, 0 / 0 is NaN)
// from correctly rounded fp64 mul / add / sub / div without contraction and one round-to-nearest-
// even cast, so a score equals the numpy rule (interval.py score_host) bit for bit. One
// grid-stride elementwise launch, one thread per element, plain vector loads and stores.
//
// group_quantiles. out[g][a] = the ranks[g][a]-th smallest (0-based) score of group g, exactly: an
// order statistic, the one reduction of the scoring jobs that is not a sum. The KEY of a score is
// its 32-bit pattern, every NaN replaced by 0x7FC00000: scores are non-negative or NaN, so
// unsigned key order is value order with NaN last, numpy's sort order. The selection is a radix
// select over the key, four rounds of 8 bits, most significant byte first; per (group, level) it
// carries the key bytes found so far (the prefix) and the rank among the keys that share them.
// Each round is two plain launches on the stream, over the plan of ops/native.py QuantilePlan
// (a GroupPlan: `order`, a stable argsort of the group ids, every group's run cut into pieces of
// at most kGroupPiece positions; plus the group of every piece):
//   A. histogram: one wave per piece (grid-stride, capped grid, the shape of group_partial_kernel).
//      Lane l reads positions l, l + 64, .. of the piece through `order` and, for every level
//      whose prefix equals the key's higher bytes, adds 1 to bin (this round's byte) of the wave's
//      PRIVATE LDS histogram [A][256] with an integer LDS atomic. Then the wave adds its nonzero
//      bins to hist[g][a][.] with global integer atomic adds and clears its LDS rows. Waves share
//      no LDS and leave the loop at different trip counts: there is no workgroup barrier in it.
//   B. pick: one wave per (group, level) (grid-stride). Lane l loads bins 4 l .. 4 l + 3 (16 B a
//      lane, 1 KiB a wave), a shuffle scan gives the running count, the lane that holds the
//      first bin whose running count exceeds the rank appends the bin to the prefix, subtracts the
//      count before it from the rank and stores both in state[g][a]; every lane stores zeros over
//      the bins it read. After round four that lane stores the prefix, as a float, in out[g][a].
// B starts after A has finished and the next A after B (stream order): no fence, no ticket,
// nothing waits on another workgroup and nothing spins. Only INTEGER atomics: the adds commute, so
// hist does not depend on the order of arrival and two runs are bitwise equal. hist is zero before
// the first launch and every pick leaves it zero.
// Round 0 takes its ranks straight from `ranks` (there is no init launch): its histogram pass
// matches every key without reading state, its pick sees the group's size n_g as the histogram's
// total, clamps the rank into [0, n_g - 1] and writes state for the rounds after it. An empty group
// (total 0) gets the rank -1, which every later round passes on, and NaN in out.
// Every index read from the plan is clamped into its array, so a wrong plan gives wrong
// quantiles (or NaN: a rank that no bin reaches becomes -1), never an access outside scores /
// order / hist / state / out.
#include "common.h"
#include "kernels.h"

namespace wf {

namespace {

constexpr int kQuantWaves = 4;        // waves (pieces / (group, level) pairs in flight) per workgroup
constexpr unsigned kNanKey = 0x7FC00000u;

// one element's score: correctly rounded fp64 operations, never fused (numpy's evaluation)
__device__ __forceinline__ float abs_score(float p, float y, double y_scale, double y_shift, bool relative) {
#pragma clang fp contract(off)
  const double a = (double)p * y_scale;
  const double v = a + y_shift;
  const double d = v - (double)y;
  const double s = relative ? fabs(d) / fabs(v) : fabs(d);
  return (float)s;
}

__device__ __forceinline__ unsigned score_key(float s) { return s != s ? kNanKey : __float_as_uint(s); }

// the lanes of a wave exchange data through LDS without a workgroup barrier: LDS operations of one
// wave execute in order; this keeps the compiler from moving them across the phase boundary
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

}  // namespace

__global__ __launch_bounds__(256) void abs_scores_kernel(const float* __restrict__ pred, const float* __restrict__ y,
                                                         long M, double y_scale, double y_shift, int relative,
                                                         float* __restrict__ out) {
  const long stride = (long)gridDim.x * blockDim.x;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < M; i += stride) {
    out[i] = abs_score(pred[i], y[i], y_scale, y_shift, relative != 0);
  }
}

bool launch_abs_scores(const float* pred, const float* y, long M, double y_scale, double y_shift, bool relative,
                       float* out, hipStream_t s) {
  if (M < 1) return false;
  // capped grid, grid-stride over the rest: 8 workgroups per CU of a 256-CU device
  long blocks = (M + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(abs_scores_kernel, dim3((unsigned)blocks), dim3(256), 0, s, pred, y, M, y_scale, y_shift,
                     relative ? 1 : 0, out);
  return true;
}

// round r of 4: `shift` = 24 - 8 r is the position of this round's byte; the prefix of a level holds
// the 8 r bits above it
__global__ __launch_bounds__(64 * kQuantWaves) void quantile_hist_kernel(
    const float* __restrict__ scores, const int* __restrict__ order, const int* __restrict__ piece_first,
    const int* __restrict__ piece_len, const int* __restrict__ piece_group, long M, int pieces, int G, int A,
    int round, const int* __restrict__ state, int* __restrict__ hist) {
  __shared__ int bins[kQuantWaves][kQuantMaxLevels][256];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int shift = 24 - 8 * round;
  int(*const mine)[256] = bins[wave];
  for (int a = 0; a < A; ++a) {
#pragma unroll
    for (int u = 0; u < 4; ++u) mine[a][lane + 64 * u] = 0;
  }
  wave_lds_sync();
  for (long pc = (long)blockIdx.x * kQuantWaves + wave; pc < pieces; pc += (long)gridDim.x * kQuantWaves) {
    long first = piece_first[pc];
    int len = piece_len[pc];
    int g = piece_group[pc];
    first = first < 0 ? 0 : (first > M ? M : first);
    len = len < 0 ? 0 : (len > kGroupPiece ? kGroupPiece : len);
    if (first + len > M) len = (int)(M - first);
    g = g < 0 ? 0 : (g >= G ? G - 1 : g);
    unsigned prefix[kQuantMaxLevels];
#pragma unroll
    for (int a = 0; a < kQuantMaxLevels; ++a) {
      prefix[a] = (round > 0 && a < A) ? (unsigned)state[2 * ((long)g * A + a)] : 0u;
    }
    for (int i = lane; i < len; i += 4 * 64) {  // four strided positions per trip: the loads overlap
      float sc[4];
      bool ok[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int j = i + 64 * u;
        ok[u] = j < len;
        long r = ok[u] ? order[first + j] : 0;
        r = r < 0 ? 0 : (r >= M ? M - 1 : r);
        sc[u] = scores[r];
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (!ok[u]) continue;
        const unsigned key = score_key(sc[u]);
        const unsigned high = round > 0 ? key >> (shift + 8) : 0u;  // the bytes above this round's
        const int bin = (int)((key >> shift) & 255u);
#pragma unroll
        for (int a = 0; a < kQuantMaxLevels; ++a) {
          if (a < A && high == prefix[a]) atomicAdd(&mine[a][bin], 1);
        }
      }
    }
    wave_lds_sync();
    for (int a = 0; a < A; ++a) {
      int* const row = hist + ((long)g * A + a) * 256;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int b = lane + 64 * u;
        const int c = mine[a][b];
        if (c != 0) {
          atomicAdd(row + b, c);
          mine[a][b] = 0;
        }
      }
    }
    wave_lds_sync();
  }
}

__global__ __launch_bounds__(64 * kQuantWaves) void quantile_pick_kernel(int* __restrict__ hist, int* __restrict__ state,
                                                                         const int* __restrict__ ranks, int GA,
                                                                         int round, float* __restrict__ out) {
  typedef int int4_t __attribute__((ext_vector_type(4)));
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  for (long ga = (long)blockIdx.x * kQuantWaves + wave; ga < GA; ga += (long)gridDim.x * kQuantWaves) {
    int4_t* const row = reinterpret_cast<int4_t*>(hist + ga * 256) + lane;
    const int4_t c = *row;
    *row = int4_t{0, 0, 0, 0};
    const int own = (c.x + c.y) + (c.z + c.w);
    int incl = own;  // the running count up to and including this lane's four bins
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int up = __shfl_up(incl, o, 64);
      if (lane >= o) incl += up;
    }
    const int total = __shfl(incl, 63, 64);
    unsigned prefix = 0u;
    int rank;
    if (round == 0) {
      rank = ranks[ga];
      rank = rank < 0 ? 0 : rank;
      rank = rank > total - 1 ? total - 1 : rank;  // an empty group: -1
    } else {
      prefix = (unsigned)state[2 * ga];
      rank = state[2 * ga + 1];
    }
    const unsigned long long reach = __ballot(rank >= 0 && incl > rank);
    const int owner = reach != 0ull ? __ffsll((long long)reach) - 1 : 0;  // no bin reaches the rank: lane 0 says so
    if (lane == owner) {
      int before = incl - own, bin = 4 * lane;
      if (reach == 0ull) {
        rank = -1;
        bin = 0;
      } else if (before + c.x > rank) {
      } else if (before + c.x + c.y > rank) {
        before += c.x;
        bin += 1;
      } else if (before + c.x + c.y + c.z > rank) {
        before += c.x + c.y;
        bin += 2;
      } else {
        before += c.x + c.y + c.z;
        bin += 3;
      }
      prefix = (prefix << 8) | (unsigned)bin;
      if (rank >= 0) rank -= before;
      state[2 * ga] = (int)prefix;
      state[2 * ga + 1] = rank;
      if (round == 3) out[ga] = __uint_as_float(rank >= 0 ? prefix : kNanKey);
    }
  }
}

bool launch_group_quantiles(const float* scores, const int* order, const int* piece_first, const int* piece_len,
                            const int* piece_group, long M, int pieces, int G, int A, const int* ranks, int* hist,
                            int* state, float* out, hipStream_t s) {
  if (M < 1 || M > 2147483647L || pieces < 1 || G < 1 || A < 1 || A > kQuantMaxLevels ||
      (long)G * A > kQuantMaxCells) {
    return false;
  }
  // capped grids, grid-stride over the rest: 8 workgroups per CU of a 256-CU device
  long ba = ((long)pieces + kQuantWaves - 1) / kQuantWaves;
  if (ba > 2048) ba = 2048;
  long bb = ((long)G * A + kQuantWaves - 1) / kQuantWaves;
  if (bb > 2048) bb = 2048;
  for (int round = 0; round < 4; ++round) {
    hipLaunchKernelGGL(quantile_hist_kernel, dim3((unsigned)ba), dim3(64 * kQuantWaves), 0, s, scores, order,
                       piece_first, piece_len, piece_group, M, pieces, G, A, round, state, hist);
    hipLaunchKernelGGL(quantile_pick_kernel, dim3((unsigned)bb), dim3(64 * kQuantWaves), 0, s, hist, state, ranks,
                       G * A, round, out);
  }
  return true;
}

}  // namespace wf
