// wellflow — scoring-error reduction on the device (gfx950).
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

}  // namespace wf
