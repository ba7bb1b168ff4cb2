// wellflow — scoring reductions on the device (gfx950): the error sums of a pass (err_sums, below),
// the per-row attribution accumulation over two passes (attr_step), the grouped prediction sums
// of a pass (group_sums) and the per-row bracket search of a set-point run (solve_step, last part
// of this file).
//
// A permutation-importance run (wellflow/importance.py) scores the table 1 + columns x repeats
// times; every pass ends in this kernel instead of a D2H copy of the predictions and a host
// sync. For predictions in standardised target units and the raw target,
//   d = (double)pred * y_scale + y_shift - (double)y
// (the pipeline's inverse_target, then the error, all in fp64) and
//   out[slot] = { sum d^2, sum |d| }.
// d is built from correctly rounded fp64 mul / add / sub without contraction, so it equals a
// numpy float64 evaluation bit for bit; only the accumulation (an fma per element, a different
// order of additions) differs.
//
// Grid-stride with a capped grid; each workgroup stores ONE partial pair; the LAST workgroup to
// draw a ticket adds the partials in a fixed tree over their index and writes out[slot]. This is
// the hand-off of grad_clip_scale_kernel (elementwise.hip), fences included: agent-scope partial
// stores, __threadfence() (release) before the ticket add; the last workgroup fences (acquire)
// after its ticket, before the barrier that lets its other waves read. No float atomics, so the
// sums do not depend on the order in which workgroups finish and are bitwise repeatable for a
// given M (the grid is a function of M alone); no workgroup waits for another, nothing spins.
// The last workgroup leaves the ticket at zero for the next launch on the stream.
// A NaN prediction gives NaN sums (NaN + x and |NaN| are NaN): the job reports it.
//
// scratch (fp64, kErrSumsScratch elements): [0 .. 2 * kErrSumsMaxBlocks) the partial pairs,
// [2 * kErrSumsMaxBlocks] the ticket (its low 32 bits; zero before the first launch).
#include "common.h"
#include "kernels.h"

namespace wf {

namespace {

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// one element's error: correctly rounded mul, add, sub, never fused (numpy's evaluation)
__device__ __forceinline__ double score_err(float p, float y, double y_scale, double y_shift) {
#pragma clang fp contract(off)
  const double a = (double)p * y_scale;
  const double b = a + y_shift;
  return b - (double)y;
}

}  // namespace

__global__ __launch_bounds__(256) void err_sums_kernel(const float* __restrict__ pred, const float* __restrict__ y,
                                                       long M, double y_scale, double y_shift, double* out2,
                                                       double* scratch) {
  __shared__ double red[2][4];
  __shared__ int is_last;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const long stride = (long)gridDim.x * blockDim.x;
  double s2 = 0.0, s1 = 0.0;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < M; i += stride) {
    const double d = score_err(pred[i], y[i], y_scale, y_shift);
    s2 += d * d;
    s1 += fabs(d);
  }
  s2 = wave_sum_f64(s2);
  s1 = wave_sum_f64(s1);
  if (lane == 0) {
    red[0][wid] = s2;
    red[1][wid] = s1;
  }
  __syncthreads();
  double* const partial = scratch;
  unsigned* const ticket = reinterpret_cast<unsigned*>(scratch + 2 * kErrSumsMaxBlocks);
  if (threadIdx.x == 0) {
    const double p2 = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
    const double p1 = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
    __hip_atomic_store(partial + 2 * blockIdx.x, p2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(partial + 2 * blockIdx.x + 1, p1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __threadfence();  // release: the partials are visible device-wide before the ticket moves
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const bool last = atomicAdd(ticket, 1u) == gridDim.x - 1;
    if (last) {
      __threadfence();  // acquire: the reads below are ordered after the ticket
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    is_last = last ? 1 : 0;
  }
  __syncthreads();
  if (!is_last) return;
  // every other workgroup has published its pair: a fixed fp64 tree over partial[0 .. grid)
  const bool have = threadIdx.x < gridDim.x;
  double d2 = have ? __hip_atomic_load(partial + 2 * threadIdx.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0;
  double d1 = have ? __hip_atomic_load(partial + 2 * threadIdx.x + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0;
  d2 = wave_sum_f64(d2);
  d1 = wave_sum_f64(d1);
  if (lane == 0) {  // (red[] was last read before the barrier above)
    red[0][wid] = d2;
    red[1][wid] = d1;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    out2[0] = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
    out2[1] = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
    __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

void launch_err_sums(const float* pred, const float* y, long M, double y_scale, double y_shift, double* out2,
                     double* scratch, hipStream_t s) {
  // one ticket counter, and the last workgroup reads one pair per thread: at most
  // kErrSumsMaxBlocks (= its 256 threads) workgroups, grid-stride over the rest
  long blocks = (M + 255) / 256;
  if (blocks > kErrSumsMaxBlocks) blocks = kErrSumsMaxBlocks;
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(err_sums_kernel, dim3((unsigned)blocks), dim3(256), 0, s, pred, y, M, y_scale, y_shift, out2,
                     scratch);
}

// ---- per-row attribution accumulation (Shapley attribution, wellflow/explain.py) ----
//
// A sampling Shapley run scores the table 1 + repeats x columns times and combines two
// consecutive passes PER ROW: the column that returned to the row's own value between them is
// credited with the change of the row's prediction. One grid-stride elementwise launch per pass:
//   start (all picked columns from the background row): v = (double)p_cur * y_scale + y_shift,
//          acc[i] += v, sq[i] += v * v             (acc / sq: the base row of the job's tables)
//   step:  d = ((double)p_cur - (double)p_prev) * y_scale,
//          acc[i] += d, sq[i] += d * d             (acc / sq: the row of the returned column)
// and p_prev[i] = p_cur[i] either way. Every operation is a correctly rounded fp64 sub / mul / add,
// never fused, and cell i is read and written by ONE thread of the launch, with plain vector
// loads and stores: no atomics, no scratch, no order of additions to depend on, so the tables
// equal a numpy float64 replay bit for bit. A NaN prediction reaches its own cell only.
namespace {

__device__ __forceinline__ void attr_cell(float pc, float pp, double y_scale, double y_shift, bool start, double* acc,
                                          double* sq) {
#pragma clang fp contract(off)
  double d;
  if (start) {
    const double a = (double)pc * y_scale;
    d = a + y_shift;
  } else {
    const double a = (double)pc - (double)pp;
    d = a * y_scale;
  }
  const double dd = d * d;
  *acc = *acc + d;
  *sq = *sq + dd;
}

}  // namespace

__global__ __launch_bounds__(256) void attr_step_kernel(const float* __restrict__ p_cur, float* __restrict__ p_prev,
                                                        long M, double y_scale, double y_shift,
                                                        double* __restrict__ acc, double* __restrict__ sq, int start) {
  const long stride = (long)gridDim.x * blockDim.x;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < M; i += stride) {
    const float pc = p_cur[i];
    const float pp = start ? 0.0f : p_prev[i];  // the start of a repeat does not read the previous pass
    attr_cell(pc, pp, y_scale, y_shift, start != 0, acc + i, sq + i);
    p_prev[i] = pc;
  }
}

void launch_attr_step(const float* p_cur, float* p_prev, long M, double y_scale, double y_shift, double* acc,
                      double* sq, bool start, hipStream_t s) {
  // capped grid, grid-stride over the rest: 8 workgroups per CU of a 256-CU device
  long blocks = (M + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(attr_step_kernel, dim3((unsigned)blocks), dim3(256), 0, s, p_cur, p_prev, M, y_scale, y_shift, acc,
                     sq, start ? 1 : 0);
}

// ---- grouped prediction sums (response curves, wellflow/response.py) ----
//
// A response-curve run scores the table 1 + sum(grid sizes) times and wants, per pass, the mean
// prediction of every group (a well, say). For v = (double)pred * y_scale + y_shift (the
// pipeline's inverse_target in fp64: a correctly rounded mul and add, never fused, so v equals
// numpy's float64 value bit for bit)
//   out[g] = { n_g, sum v, sum v * v }        for every group g in [0, G).
//
// The grouping is the same for every pass, so the host builds a PLAN once (ops/native.py
// GroupPlan): `order`, a stable argsort of the group ids (pred is read through it: the identity,
// a coalesced read, when the rows are already grouped; a 4-B gather otherwise), and every group's
// run in `order` cut into pieces of at most kGroupPiece positions. Two plain launches on the stream:
//   A. one wave per piece (grid-stride, capped grid): lane l adds positions l, l + 64, .. of the
//      piece in that order, a fixed xor tree joins the lanes, lane 0 stores partial[piece];
//   B. one wave per group (grid-stride): lane l adds the group's pieces l, l + 64, .. in index
//      order, the same tree, lane 0 stores out[g] (zeros for a group without pieces).
// B starts after A has finished (stream order), so there is no fence, no ticket and no scratch
// state to leave ready; no float atomics, nothing waits or spins. The order of additions is a
// function of the plan alone (of the group layout and kGroupPiece), so the sums are bitwise
// repeatable. A NaN prediction reaches the partials of its own group only.
// Every index read from the plan is clamped into its array, so a wrong plan gives wrong sums,
// never an access outside pred / order / partial.
namespace {

constexpr int kGroupWaves = 4;  // waves (pieces / groups in flight) per workgroup

__device__ __forceinline__ double group_value(float p, double y_scale, double y_shift) {
#pragma clang fp contract(off)
  const double a = (double)p * y_scale;
  return a + y_shift;
}

}  // namespace

__global__ __launch_bounds__(64 * kGroupWaves) void group_partial_kernel(
    const float* __restrict__ pred, const int* __restrict__ order, const int* __restrict__ piece_first,
    const int* __restrict__ piece_len, long M, int pieces, double y_scale, double y_shift,
    double* __restrict__ partial) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  for (long pc = (long)blockIdx.x * kGroupWaves + wave; pc < pieces; pc += (long)gridDim.x * kGroupWaves) {
    long first = piece_first[pc];
    int len = piece_len[pc];
    first = first < 0 ? 0 : (first > M ? M : first);
    len = len < 0 ? 0 : (len > kGroupPiece ? kGroupPiece : len);
    if (first + len > M) len = (int)(M - first);
    double s1 = 0.0, s2 = 0.0;
    for (int i = lane; i < len; i += 4 * 64) {  // four strided positions per trip: the loads overlap
      float p[4];
      bool ok[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int j = i + 64 * u;
        ok[u] = j < len;
        long r = ok[u] ? order[first + j] : 0;
        r = r < 0 ? 0 : (r >= M ? M - 1 : r);
        p[u] = pred[r];
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (ok[u]) {
          const double v = group_value(p[u], y_scale, y_shift);
          s1 += v;
          s2 += v * v;
        }
      }
    }
    s1 = wave_sum_f64(s1);
    s2 = wave_sum_f64(s2);
    if (lane == 0) {
      partial[3 * pc] = (double)len;
      partial[3 * pc + 1] = s1;
      partial[3 * pc + 2] = s2;
    }
  }
}

__global__ __launch_bounds__(64 * kGroupWaves) void group_finish_kernel(const double* __restrict__ partial,
                                                                        const int* __restrict__ group_pieces,
                                                                        int pieces, int G, double* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  for (long g = (long)blockIdx.x * kGroupWaves + wave; g < G; g += (long)gridDim.x * kGroupWaves) {
    int p0 = group_pieces[g], p1 = group_pieces[g + 1];
    p0 = p0 < 0 ? 0 : (p0 > pieces ? pieces : p0);
    p1 = p1 < p0 ? p0 : (p1 > pieces ? pieces : p1);
    double n = 0.0, s1 = 0.0, s2 = 0.0;
    // four strided pieces per trip: their loads overlap (one group of a large table has thousands
    // of pieces and ONE wave to walk them); added in index order all the same
    for (int pc = p0 + lane; pc < p1; pc += 4 * 64) {
      double a[4][3];
      bool ok[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        ok[u] = pc + 64 * u < p1;
        const long q = 3 * (long)(ok[u] ? pc + 64 * u : p0);
        a[u][0] = partial[q];
        a[u][1] = partial[q + 1];
        a[u][2] = partial[q + 2];
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (ok[u]) {
          n += a[u][0];
          s1 += a[u][1];
          s2 += a[u][2];
        }
      }
    }
    n = wave_sum_f64(n);
    s1 = wave_sum_f64(s1);
    s2 = wave_sum_f64(s2);
    if (lane == 0) {
      const bool empty = p1 == p0;
      out[3 * g] = empty ? 0.0 : n;
      out[3 * g + 1] = empty ? 0.0 : s1;
      out[3 * g + 2] = empty ? 0.0 : s2;
    }
  }
}

bool launch_group_sums(const float* pred, const int* order, const int* piece_first, const int* piece_len,
                       const int* group_pieces, long M, int pieces, int G, double y_scale, double y_shift,
                       double* out, double* partial, hipStream_t s) {
  if (M < 1 || M > 2147483647L || pieces < 1 || G < 1 || G > kGroupSumsMaxGroups) return false;
  // capped grids, grid-stride over the rest: 8 workgroups per CU of a 256-CU device
  long ba = ((long)pieces + kGroupWaves - 1) / kGroupWaves;
  if (ba > 2048) ba = 2048;
  long bb = ((long)G + kGroupWaves - 1) / kGroupWaves;
  if (bb > 2048) bb = 2048;
  hipLaunchKernelGGL(group_partial_kernel, dim3((unsigned)ba), dim3(64 * kGroupWaves), 0, s, pred, order, piece_first,
                     piece_len, M, pieces, y_scale, y_shift, partial);
  hipLaunchKernelGGL(group_finish_kernel, dim3((unsigned)bb), dim3(64 * kGroupWaves), 0, s, partial, group_pieces,
                     pieces, G, out);
  return true;
}

// ---- per-row bracket search (set points, wellflow/setpoint.py) ----
//
// A set-point run asks, per row, at which value of ONE input column the prediction meets a wanted
// value: 1 + G + S passes, G over a grid of values (the same for every row), then S in which every
// bracketed row is scored at the midpoint of its own bracket. Each pass ends in one grid-stride
// elementwise launch that carries the row's state to the next pass. The residual is err_sums' d:
//   r = (double)p * y_scale + y_shift - (double)want[i]        (fp64, never contracted)
// State per prediction i: xs fp32 [4][M] = {lo, hi, best_x, xq}, fs fp64 [3][M] = {f_lo, f_hi,
// best_r}, status int32 [M] (0 open, 1 bracketed). x: the value the column had in this pass.
//   first scan (x = *grid_x): status = 0; lo = hi = best_x = x; f_lo = f_hi = best_r = r
//   scan (x = *grid_x), open rows only, in this order:
//     |r| < |best_r|, or best_r is NaN and r is not   ->  best_x = x, best_r = r   (strict: the first
//                                                         of equal misses stays)
//     (f_lo <= 0 && r >= 0) || (f_lo >= 0 && r <= 0)  ->  hi = x, f_hi = r, status = 1
//     else                                            ->  lo = hi = x, f_lo = f_hi = r
//   refine (x = xq[i]), bracketed rows only: r on f_lo's side of zero (f_lo < 0 ? r < 0 : f_lo > 0 ?
//     r > 0 : false)  ->  lo = x, f_lo = r;  else hi = x, f_hi = r
//   every pass ends with xq = status == 1 ? lo + (hi - lo) * 0.5f : best_x   (fp32)
// A comparison with a NaN is false, so a NaN residual never brackets and reaches its own row only.
// Cell i is read and written by ONE thread of the launch, with plain vector loads and stores: no
// atomics, no LDS, no scratch, no state outside the arguments, so the state equals a numpy replay
// bit for bit and two runs are bitwise equal. p / want must not overlap the state.
namespace {

__device__ __forceinline__ float solve_mid(float lo, float hi) {
#pragma clang fp contract(off)
  const float w = hi - lo;
  const float h = w * 0.5f;
  return lo + h;
}

}  // namespace

__global__ __launch_bounds__(256) void solve_step_kernel(const float* __restrict__ p, const float* __restrict__ want,
                                                         long M, double y_scale, double y_shift, int mode,
                                                         const float* __restrict__ grid_x, float* __restrict__ xs,
                                                         double* __restrict__ fs, int* __restrict__ status) {
  const long stride = (long)gridDim.x * blockDim.x;
  float* const lo_ = xs;
  float* const hi_ = xs + M;
  float* const bx_ = xs + 2 * M;
  float* const xq_ = xs + 3 * M;
  double* const flo_ = fs;
  double* const fhi_ = fs + M;
  double* const br_ = fs + 2 * M;
  const float gx = mode == kSolveRefine ? 0.0f : grid_x[0];  // uniform: one scalar for every row
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < M; i += stride) {
    const double r = score_err(p[i], want[i], y_scale, y_shift);
    if (mode == kSolveFirst) {
      lo_[i] = gx;
      hi_[i] = gx;
      bx_[i] = gx;
      xq_[i] = gx;  // open: the best value so far
      flo_[i] = r;
      fhi_[i] = r;
      br_[i] = r;
      status[i] = 0;
      continue;
    }
    const int st = status[i];
    if (mode == kSolveScan) {
      if (st != 0) continue;  // the first crossing in grid order stays (xq is the bracket's midpoint already)
      float bx = bx_[i];
      const double br = br_[i];
      const double flo = flo_[i];
      if (fabs(r) < fabs(br) || (br != br && r == r)) {
        bx = gx;
        bx_[i] = gx;
        br_[i] = r;
      }
      if ((flo <= 0.0 && r >= 0.0) || (flo >= 0.0 && r <= 0.0)) {
        hi_[i] = gx;
        fhi_[i] = r;
        status[i] = 1;
        xq_[i] = solve_mid(lo_[i], gx);
      } else {
        lo_[i] = gx;
        hi_[i] = gx;
        flo_[i] = r;
        fhi_[i] = r;
        xq_[i] = bx;
      }
    } else {
      if (st != 1) continue;  // open rows keep xq = best_x
      const float x = xq_[i];
      const double flo = flo_[i];
      const bool same = flo < 0.0 ? r < 0.0 : (flo > 0.0 ? r > 0.0 : false);
      float lo = lo_[i], hi = hi_[i];
      if (same) {
        lo = x;
        lo_[i] = x;
        flo_[i] = r;
      } else {
        hi = x;
        hi_[i] = x;
        fhi_[i] = r;
      }
      xq_[i] = solve_mid(lo, hi);
    }
  }
}

bool launch_solve_step(const float* p, const float* want, long M, double y_scale, double y_shift, int mode,
                       const float* grid_x, float* xs, double* fs, int* status, hipStream_t s) {
  if (M < 1 || mode < kSolveFirst || mode > kSolveRefine) return false;
  if (mode != kSolveRefine && grid_x == nullptr) return false;
  // capped grid, grid-stride over the rest: 8 workgroups per CU of a 256-CU device
  long blocks = (M + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(solve_step_kernel, dim3((unsigned)blocks), dim3(256), 0, s, p, want, M, y_scale, y_shift, mode,
                     grid_x, xs, fs, status);
  return true;
}

}  // namespace wf
