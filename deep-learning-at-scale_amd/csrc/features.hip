// wellflow — feature assembly on the device (gfx950): raw table columns -> engine input rows.
//
// A scoring job touches every row once, so building the engines' input on the host (numpy
// one-hot blocks + concatenate + standardise, data/features.py FeaturePipeline._assemble) and
// uploading the widened [N][F] matrix is its whole run time. This kernel takes the raw columns
// (int32 label codes [C][N], fp32 continuous values [Q][N]) and writes
//   * OutT = bf16_t, ld = round_up(F, 8): the MLP input format (NativeMLP.to_input_format),
//     columns F .. ld-1 zero;
//   * OutT = float,  ld = F: the LSTM row table that lstm_pack_x_win reads.
// Row r: one-hot blocks in pipeline order (block c has a 1 at cat_off[c] + code when
// code < cat_size[c], else stays zero: the dropped last category and unseen labels), then the Q
// continuous values (x - mean) / std: an fp32 subtract and a correctly rounded fp32 divide (the
// build passes no fast-math flag), so the result equals the host pipeline bit for bit.
//
// Shape. Source columns are column-major and the output is row-major, so a 256-thread
// workgroup transposes one 64-row tile through LDS:
//   1. zero the tile (the one-hot zeros and the padding columns);
//   2. lane = row, wave = source column: a wave reads 64 consecutive rows of one column (one
//      256-B segment, every source value read exactly once) and writes its element into the
//      tile. The tile's row stride is Dp = D | 1 dwords (D = dwords per output row), odd, so the
//      64 lanes of a continuous column hit 32 distinct banks per half-wave; the one-hot 1s land
//      at data-dependent columns;
//   3. the tile's rows are contiguous in the output (64 rows x ld x sizeof(OutT) is a multiple of
//      256 B), so it leaves as a flat copy: 16 B per lane, consecutive lanes at consecutive
//      addresses. A lane gathers its four dwords from the padded tile with ds_read_b32; the k-th
//      read of lane l takes dword (k + l / 8) & 3, so lanes l, l + 8, l + 16, l + 24 (whose four
//      dwords share four banks: 32 lanes x 4 dwords span the 32 banks four times) read four
//      different banks at once: at most 2-3 addresses per bank where the row padding shifts a
//      lane's dwords, against 4 in the unrotated order.
// No atomics; plain vector stores; any N >= 1 (the tail tile copies rows x D dwords, the last
// < 4 of them as single dwords); C = 0 or Q = 0 allowed; grid-stride over tiles.
//
// Source columns are ld_src elements apart (>= N): a piece of a larger resident table is
// assembled by pointing codes / cont at its first row, without a copy of the piece.
//
// One permuted source (permutation importance, wellflow/importance.py). With perm_src in
// [0, C + Q) (the kernel's source order: categorical columns, then continuous) output row r takes
// THAT column's value from perm_base[clamp(perm[r], 0, perm_n - 1)]: perm_base / perm_n are the
// base and length of the whole source column, so a piece gathers from all rows of the table. The
// clamp is unconditional (gather_rows_kernel, elementwise.hip): a bad index is never an
// out-of-bounds read. The wave index is the source column, so the branch is wave-uniform: one
// wave per tile gathers (64 4-B reads, a 32-B sector each), every other column is read as
// before, coalesced and once. perm_src = -1: no column matches, the launch is the plain one.
//
// One constant source (response curves, wellflow/response.py). With const_src in [0, C + Q) every
// output row takes THAT column's value from the one-element device array const_val (an int32 label
// code or an fp32 raw value: a job uploads a column's whole grid once and pass g points at element
// g). The value goes through the same code < cat_size test / the same (x - mean) / std as a value
// read from the table, so the unknown index and the dropped last category give the all-zero block.
// const_src is a kernel argument, so the branch is uniform: the column's wave reads one scalar
// instead of 64 rows, every other column is read as before. const_src = -1 (and perm_src = -1):
// the plain launch. At most one of perm_src / const_src is set (the launcher refuses both).
//
// A SET of permuted sources (Shapley attribution, wellflow/explain.py): assemble_features_set_kernel,
// below. set_mask is a device bitmask over the source columns (bit s & 31 of word s >> 5,
// ceil((C + Q) / 32) <= 16 words: a job uploads the masks of all its passes once and a pass points
// at its row); every source column s in the set takes base_column_s[clamp(perm[r], 0, perm_n - 1)],
// where base_column_s = codes0 + s * ld_src or cont0 + (s - C) * ld_src: codes0 / cont0 are row 0 of
// the resident table and perm_n the column length, so a piece gathers from all rows. The row's index
// is read and clamped once per tile row; s is wave-uniform, so the set test is one scalar word load
// per column. The value goes through the same block test / standardisation. The tile scheme is the
// one above, in a kernel of its own: assemble_features_kernel is compiled from the text it had, so
// the plain, single-perm_src and constant launches run the code they ran before (a shared body
// template was tried: inlined into the old kernel it gave other register allocation and schedule).
#include "common.h"
#include "kernels.h"

namespace wf {

namespace {

constexpr int kAsmRows = 64;      // rows per tile = one wave of lanes per source column
constexpr int kAsmThreads = 256;

template <typename OutT>
struct AsmOut;
template <>
struct AsmOut<float> {
  static __device__ __forceinline__ float cvt(float v) { return v; }
};
template <>
struct AsmOut<bf16_t> {
  static __device__ __forceinline__ bf16_t cvt(float v) { return f2bf(v); }  // RNE, as cast_bf16_kernel
};

}  // namespace

template <typename OutT>
__global__ __launch_bounds__(kAsmThreads) void assemble_features_kernel(
    const int* __restrict__ codes, const float* __restrict__ cont, const int* __restrict__ cat_off,
    const int* __restrict__ cat_size, const float* __restrict__ mean, const float* __restrict__ stdv, long N, int C,
    int Q, int F, int ld, OutT* __restrict__ out, long ld_src, int perm_src, const int* __restrict__ perm,
    const void* __restrict__ perm_base, long perm_n, int const_src, const void* __restrict__ const_val) {
  extern __shared__ unsigned asm_tile[];  // [kAsmRows][Dp] dwords
  constexpr int EPD = 4 / (int)sizeof(OutT);  // elements per dword
  const int D = ld / EPD;                     // dwords per output row (bf16: ld % 8 == 0)
  const int Dp = D | 1;
  const int Fc = F - Q;  // width of the one-hot part
  OutT* const telem = reinterpret_cast<OutT*>(asm_tile);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // wave-uniform: the column spec loads go scalar
  const long ntiles = (N + kAsmRows - 1) / kAsmRows;
  for (long tl = blockIdx.x; tl < ntiles; tl += gridDim.x) {
    const long row0 = tl * kAsmRows;
    const int rows = (int)((N - row0) < (long)kAsmRows ? (N - row0) : (long)kAsmRows);
    for (int i = tid; i < kAsmRows * Dp; i += kAsmThreads) asm_tile[i] = 0u;
    __syncthreads();
    if (lane < rows) {
      OutT* const trow = telem + (long)lane * Dp * EPD;
      for (int s = wave; s < C + Q; s += kAsmThreads / 64) {
        const bool permuted = s == perm_src;  // wave-uniform
        const bool constant = s == const_src;  // uniform: the same value for every row
        long pr = 0;
        if (permuted) {
          pr = perm[row0 + lane];
          pr = pr < 0 ? 0 : (pr >= perm_n ? perm_n - 1 : pr);
        }
        if (s < C) {
          const int code = constant   ? *static_cast<const int*>(const_val)
                           : permuted ? static_cast<const int*>(perm_base)[pr]
                                      : codes[(long)s * ld_src + row0 + lane];
          const int col = cat_off[s] + code;
          // col < Fc also when the block spec itself were wrong: never a write outside the row
          if ((unsigned)code < (unsigned)cat_size[s] && (unsigned)col < (unsigned)Fc) trow[col] = AsmOut<OutT>::cvt(1.0f);
        } else {
          const int q = s - C;
          const float x = constant   ? *static_cast<const float*>(const_val)
                          : permuted ? static_cast<const float*>(perm_base)[pr]
                                     : cont[(long)q * ld_src + row0 + lane];
          trow[Fc + q] = AsmOut<OutT>::cvt((x - mean[q]) / stdv[q]);
        }
      }
    }
    __syncthreads();
    const int tile_dw = rows * D;
    unsigned* const gout = reinterpret_cast<unsigned*>(out + row0 * ld);  // 256-B aligned: row0 % 64 == 0
    const int nchunk = tile_dw >> 2;
    const int rot = (lane >> 3) & 3;
    for (int ch = tid; ch < nchunk; ch += kAsmThreads) {
      const int d0 = ch * 4;
      const int r0 = d0 / D, c0 = d0 - r0 * D;
      unsigned v0 = 0u, v1 = 0u, v2 = 0u, v3 = 0u;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int kk = (k + rot) & 3;
        int r = r0, c = c0 + kk;
        while (c >= D) {  // a float row of F % 4 != 0 dwords: the 16 B straddle rows
          c -= D;
          ++r;
        }
        const unsigned w = asm_tile[r * Dp + c];
        v0 = kk == 0 ? w : v0;
        v1 = kk == 1 ? w : v1;
        v2 = kk == 2 ? w : v2;
        v3 = kk == 3 ? w : v3;
      }
      typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
      *reinterpret_cast<u32x4*>(gout + d0) = u32x4{v0, v1, v2, v3};
    }
    for (int d = nchunk * 4 + tid; d < tile_dw; d += kAsmThreads) {  // tail tile of a float table only
      const int r = d / D;
      gout[d] = asm_tile[r * Dp + (d - r * D)];
    }
    __syncthreads();  // the next tile's zero fill overwrites what this copy reads
  }
}

// The set launch: the tile scheme of assemble_features_kernel (zero, lane = row / wave = source
// column, flat rotated copy-out); every source column whose bit is set in set_mask is read through
// perm from the whole column (codes0 / cont0 + column * ld_src, perm_n rows), the others in place.
template <typename OutT>
__global__ __launch_bounds__(kAsmThreads) void assemble_features_set_kernel(
    const int* __restrict__ codes, const float* __restrict__ cont, const int* __restrict__ cat_off,
    const int* __restrict__ cat_size, const float* __restrict__ mean, const float* __restrict__ stdv, long N, int C,
    int Q, int F, int ld, OutT* __restrict__ out, long ld_src, const int* __restrict__ perm, long perm_n,
    const unsigned* __restrict__ set_mask, const int* __restrict__ codes0, const float* __restrict__ cont0) {
  extern __shared__ unsigned asm_tile[];  // [kAsmRows][Dp] dwords
  constexpr int EPD = 4 / (int)sizeof(OutT);
  const int D = ld / EPD;
  const int Dp = D | 1;
  const int Fc = F - Q;
  OutT* const telem = reinterpret_cast<OutT*>(asm_tile);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // wave-uniform: the mask and column spec loads go scalar
  const long ntiles = (N + kAsmRows - 1) / kAsmRows;
  for (long tl = blockIdx.x; tl < ntiles; tl += gridDim.x) {
    const long row0 = tl * kAsmRows;
    const int rows = (int)((N - row0) < (long)kAsmRows ? (N - row0) : (long)kAsmRows);
    for (int i = tid; i < kAsmRows * Dp; i += kAsmThreads) asm_tile[i] = 0u;
    __syncthreads();
    if (lane < rows) {
      OutT* const trow = telem + (long)lane * Dp * EPD;
      long pr = perm[row0 + lane];  // one index per row for every column of the set
      pr = pr < 0 ? 0 : (pr >= perm_n ? perm_n - 1 : pr);  // unconditional: a bad index is never read through
      for (int s = wave; s < C + Q; s += kAsmThreads / 64) {
        const bool permuted = ((set_mask[s >> 5] >> (s & 31)) & 1u) != 0u;  // wave-uniform
        if (s < C) {
          const int code = permuted ? codes0[(long)s * ld_src + pr] : codes[(long)s * ld_src + row0 + lane];
          const int col = cat_off[s] + code;
          if ((unsigned)code < (unsigned)cat_size[s] && (unsigned)col < (unsigned)Fc) trow[col] = AsmOut<OutT>::cvt(1.0f);
        } else {
          const int q = s - C;
          const float x = permuted ? cont0[(long)q * ld_src + pr] : cont[(long)q * ld_src + row0 + lane];
          trow[Fc + q] = AsmOut<OutT>::cvt((x - mean[q]) / stdv[q]);
        }
      }
    }
    __syncthreads();
    const int tile_dw = rows * D;
    unsigned* const gout = reinterpret_cast<unsigned*>(out + row0 * ld);  // 256-B aligned: row0 % 64 == 0
    const int nchunk = tile_dw >> 2;
    const int rot = (lane >> 3) & 3;
    for (int ch = tid; ch < nchunk; ch += kAsmThreads) {
      const int d0 = ch * 4;
      const int r0 = d0 / D, c0 = d0 - r0 * D;
      unsigned v0 = 0u, v1 = 0u, v2 = 0u, v3 = 0u;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int kk = (k + rot) & 3;
        int r = r0, c = c0 + kk;
        while (c >= D) {
          c -= D;
          ++r;
        }
        const unsigned w = asm_tile[r * Dp + c];
        v0 = kk == 0 ? w : v0;
        v1 = kk == 1 ? w : v1;
        v2 = kk == 2 ? w : v2;
        v3 = kk == 3 ? w : v3;
      }
      typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
      *reinterpret_cast<u32x4*>(gout + d0) = u32x4{v0, v1, v2, v3};
    }
    for (int d = nchunk * 4 + tid; d < tile_dw; d += kAsmThreads) {
      const int r = d / D;
      gout[d] = asm_tile[r * Dp + (d - r * D)];
    }
    __syncthreads();
  }
}

size_t assemble_features_lds_bytes(int ld, bool bf16_out) {
  const int D = bf16_out ? ld / 2 : ld;
  return (size_t)kAsmRows * (D | 1) * 4;
}

template <typename OutT>
static bool launch_assemble(const int* codes, const float* cont, const int* cat_off, const int* cat_size,
                            const float* mean, const float* stdv, long N, int C, int Q, int F, int ld, OutT* out,
                            hipStream_t s, const AssemblePerm& pm) {
  // a permuted source needs its index vector and a non-empty column to clamp into; a broadcast
  // source its one value, and no index vector (the two modes exclude each other)
  if (pm.src >= 0 && !pm.broadcast && (pm.src >= C + Q || pm.perm == nullptr || pm.base == nullptr || pm.n < 1))
    return false;
  if (pm.broadcast && (pm.src < 0 || pm.src >= C + Q || pm.value == nullptr || pm.perm != nullptr)) return false;
  if (pm.ld_src != 0 && pm.ld_src < N) return false;
  // a set of permuted sources: its mask and index vector, the table's row 0 and a non-empty column
  // of at most ld_src rows to clamp into; never together with one permuted or one constant source
  const bool set = pm.set_mask != nullptr;
  if (set && (pm.src >= 0 || pm.broadcast || pm.value != nullptr || pm.base != nullptr || pm.perm == nullptr ||
              pm.n < 1 || pm.ld_src < pm.n || (C > 0 && pm.codes0 == nullptr) || (Q > 0 && pm.cont0 == nullptr)))
    return false;
  const size_t lds = assemble_features_lds_bytes(ld, sizeof(OutT) == 2);
  if (lds > kAssembleMaxLds) return false;
  const long ntiles = (N + kAsmRows - 1) / kAsmRows;
  // capped grid: 8 workgroups per CU of a 256-CU device keep ~0.5 MB of column reads in flight
  const long grid = ntiles < 2048 ? ntiles : 2048;
  if (set) {
    auto skern = assemble_features_set_kernel<OutT>;
    if (lds > 48 * 1024 &&
        hipFuncSetAttribute(reinterpret_cast<const void*>(skern), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)lds) != hipSuccess)
      return false;
    hipLaunchKernelGGL(skern, dim3((unsigned)grid), dim3(kAsmThreads), lds, s, codes, cont, cat_off, cat_size, mean,
                       stdv, N, C, Q, F, ld, out, pm.ld_src, pm.perm, pm.n, pm.set_mask, pm.codes0, pm.cont0);
    return true;
  }
  auto kern = assemble_features_kernel<OutT>;
  if (lds > 48 * 1024 &&
      hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) !=
          hipSuccess)
    return false;
  hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(kAsmThreads), lds, s, codes, cont, cat_off, cat_size, mean, stdv,
                     N, C, Q, F, ld, out, pm.ld_src ? pm.ld_src : N, pm.src >= 0 && !pm.broadcast ? pm.src : -1, pm.perm,
                     pm.base, pm.n, pm.broadcast ? pm.src : -1, pm.value);
  return true;
}

bool launch_assemble_features_bf16(const int* codes, const float* cont, const int* cat_off, const int* cat_size,
                                   const float* mean, const float* stdv, long N, int C, int Q, int F, int ld,
                                   bf16_t* out, hipStream_t s, const AssemblePerm& pm) {
  return launch_assemble<bf16_t>(codes, cont, cat_off, cat_size, mean, stdv, N, C, Q, F, ld, out, s, pm);
}

bool launch_assemble_features_f32(const int* codes, const float* cont, const int* cat_off, const int* cat_size,
                                  const float* mean, const float* stdv, long N, int C, int Q, int F, int ld, float* out,
                                  hipStream_t s, const AssemblePerm& pm) {
  return launch_assemble<float>(codes, cont, cat_off, cat_size, mean, stdv, N, C, Q, F, ld, out, s, pm);
}

}  // namespace wf
