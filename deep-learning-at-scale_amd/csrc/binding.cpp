// wellflow — Python bindings for the HIP kernel library (pybind11 via torch/extension.h).
//
// Every entry point validates device, dtype, contiguity, alignment and the extents the
// kernel and its grid will touch BEFORE launching: a hand-written kernel indexing out of
// bounds can take the whole GPU node down, so shape errors must be caught on the host.
#include <torch/extension.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>
#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>

#include <cstdlib>
#include <map>
#include <type_traits>
#include <mutex>
#include <vector>

#include "kernels.h"

namespace {

using wf::bf16_t;

// A/B and diagnostic environment overrides are read only when the HIP objects are a WF_DIAG
// build (wf::dbg_mask() is ~0 there): a production _C.so reads exactly the documented knobs
// (README "Environment knobs"; tests/test_diag_cpu.py checks the set).
int diag_env(const char* name, int dflt) {
  if (wf::dbg_mask() != ~0) return dflt;
  const char* v = std::getenv(name);
  return v != nullptr ? std::atoi(v) : dflt;
}

bool disable_glds() {
  static const bool off = diag_env("WELLFLOW_NO_GLDS", 0) == 1;  // register-staged GEMM (A/B)
  return off;
}

hipStream_t cur_stream() { return c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream(); }

void check_t(const at::Tensor& t, at::ScalarType dt, const char* name) {
  TORCH_CHECK(t.defined(), name, ": undefined tensor");
  TORCH_CHECK(t.is_cuda(), name, ": must be a GPU tensor");
  TORCH_CHECK(t.scalar_type() == dt, name, ": expected dtype ", dt, " got ", t.scalar_type());
  TORCH_CHECK(t.is_contiguous(), name, ": must be contiguous");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0, name,
              ": data pointer must be 16-byte aligned");
}

void check_extent(const at::Tensor& t, int64_t need, const char* name) {
  TORCH_CHECK(t.numel() >= need, name, ": needs at least ", need, " elements, has ", t.numel());
}

bf16_t* bfp(const at::Tensor& t) { return reinterpret_cast<bf16_t*>(t.data_ptr()); }
float* fp(const at::Tensor& t) { return t.data_ptr<float>(); }

template <class T>
T* opt_ptr(const c10::optional<at::Tensor>& t, at::ScalarType dt, const char* name,
           int64_t need) {
  if (!t.has_value() || !t->defined()) return nullptr;
  check_t(*t, dt, name);
  check_extent(*t, need, name);
  return reinterpret_cast<T*>(t->data_ptr());
}

// CPU tensors are accepted where nothing is launched (gemm_plan): the plan only needs sizes.
void check_operand(const at::Tensor& t, at::ScalarType dt, const char* name, bool launch) {
  if (launch) return check_t(t, dt, name);
  TORCH_CHECK(t.defined(), name, ": undefined tensor");
  TORCH_CHECK(t.scalar_type() == dt, name, ": expected dtype ", dt, " got ", t.scalar_type());
  TORCH_CHECK(t.is_contiguous(), name, ": must be contiguous");
}

template <class T>
T* opt_operand(const c10::optional<at::Tensor>& t, at::ScalarType dt, const char* name, int64_t need, bool launch) {
  if (!t.has_value() || !t->defined()) return nullptr;
  check_operand(*t, dt, name, launch);
  check_extent(*t, need, name);
  return reinterpret_cast<T*>(t->data_ptr());
}

// Everything gemm checks and decides before its launch: the validated epilogue and whether the
// direct-to-LDS ring may read these operands. gemm_plan runs exactly this and launches nothing.
struct GemmCall {
  wf::GemmEpilogue e;
  bool glds_ok = false;
};

GemmCall gemm_prepare(const at::Tensor& A, bool a_mn, int64_t lda, const at::Tensor& B, bool b_mn, int64_t ldb,
                      int64_t M, int64_t N, int64_t K, int64_t ksplit, const c10::optional<at::Tensor>& outF,
                      const c10::optional<at::Tensor>& outH, int64_t ldo, const c10::optional<at::Tensor>& bias,
                      const c10::optional<at::Tensor>& mask, int64_t ldm, double mask_scale,
                      const c10::optional<at::Tensor>& colsum, double alpha, double beta, int64_t act, bool atomic,
                      double drop_p, int64_t seed, int64_t big_tile, const c10::optional<at::Tensor>& seed_dev,
                      bool launch) {
  TORCH_CHECK(wf::dw_tile_valid(big_tile), "gemm: tile ", big_tile, " does not exist; valid ids are 0 (128x128), ",
              "1 (256x128), 3 (256x192), 4 / 5 (256x192, 5- / 4-slot ring), 7 (best for N)");
  check_operand(A, at::kBFloat16, "A", launch);
  check_operand(B, at::kBFloat16, "B", launch);
  TORCH_CHECK(M > 0 && N > 0 && K > 0, "gemm: empty problem");
  TORCH_CHECK(lda % 8 == 0 && ldb % 8 == 0, "gemm: lda/ldb must be multiples of 8");
  TORCH_CHECK(a_mn ? (M % 8 == 0) : (K % 8 == 0), "gemm: A contiguous extent must be a multiple of 8");
  TORCH_CHECK(b_mn ? (N % 8 == 0) : (K % 8 == 0), "gemm: B contiguous extent must be a multiple of 8");
  TORCH_CHECK(a_mn ? lda >= M : lda >= K, "gemm: lda too small");
  TORCH_CHECK(b_mn ? ldb >= N : ldb >= K, "gemm: ldb too small");
  check_extent(A, wf::gemm_operand_extent(a_mn, M, K, lda), "A");
  check_extent(B, wf::gemm_operand_extent(b_mn, N, K, ldb), "B");
  TORCH_CHECK(ldo >= N, "gemm: ldo < N");
  // the epilogue's ranges: the kernel would take any other act as 0 and divide by 1 - drop_p
  TORCH_CHECK(act == 0 || act == 1, "gemm: act must be 0 (linear) or 1 (ReLU), got ", act);
  TORCH_CHECK(drop_p >= 0.0 && drop_p < 1.0, "gemm: drop_p must lie in [0, 1), got ", drop_p);
  const int64_t out_need = (M - 1) * ldo + N;
  GemmCall c;
  wf::GemmEpilogue& e = c.e;
  e.outF = opt_operand<float>(outF, at::kFloat, "outF", out_need, launch);
  e.outH = opt_operand<bf16_t>(outH, at::kBFloat16, "outH", out_need, launch);
  TORCH_CHECK(e.outF || e.outH, "gemm: need an output");
  TORCH_CHECK(!atomic || (e.outF && !e.outH && beta == 0.0), "gemm: atomic needs outF only, beta 0");
  TORCH_CHECK(beta == 0.0 || e.outF, "gemm: beta needs outF");
  e.ldo = ldo;
  e.bias = opt_operand<float>(bias, at::kFloat, "bias", N, launch);
  if (mask.has_value() && mask->defined()) TORCH_CHECK(ldm >= N, "gemm: ldm < N");
  e.mask = opt_operand<bf16_t>(mask, at::kBFloat16, "mask", (M - 1) * ldm + N, launch);
  e.ldm = ldm;
  e.mask_scale = (float)mask_scale;
  e.colsum = opt_operand<float>(colsum, at::kFloat, "colsum", N, launch);
  // the atomic epilogue adds alpha * acc and nothing else: refuse what it would silently drop
  TORCH_CHECK(!atomic || (!e.bias && !e.mask && !e.colsum && act == 0 && drop_p == 0.0),
              "gemm: atomic adds alpha * acc only; bias, mask, colsum, act and drop_p cannot go with it");
  e.alpha = (float)alpha;
  e.beta = (float)beta;
  e.act = (int)act;
  e.atomic = atomic ? 1 : 0;
  e.drop_p = (float)drop_p;
  e.seed = (unsigned long long)seed;
  if (seed_dev.has_value() && seed_dev->defined()) {
    TORCH_CHECK((seed_dev->is_cuda() || !launch) && seed_dev->scalar_type() == at::kLong && seed_dev->numel() >= 1,
                "gemm: seed_dev must be a GPU int64 tensor");
    e.seed_dev = reinterpret_cast<const long long*>(seed_dev->data_ptr<int64_t>());
  }
  e.big_tile = (int)big_tile;
  TORCH_CHECK(ksplit == 1 || atomic, "gemm: split-K needs atomic accumulation");
  e.stage_ok = wf::gemm_stage_ok(e.outF != nullptr, e.outH != nullptr, atomic, beta, N, ldo, e.mask != nullptr, ldm) ? 1 : 0;
  // glds (whole-tile) path: the 128x128 tiles may over-read rows/cols past M / N; allow it
  // only when that stays inside both allocations (and every K chunk is 64-aligned).
  c.glds_ok = wf::gemm_glds_ok(a_mn, b_mn, M, N, K, lda, ldb, A.numel(), B.numel()) && !disable_glds();
  return c;
}

void gemm(const at::Tensor& A, bool a_mn, int64_t lda, const at::Tensor& B, bool b_mn, int64_t ldb,
          int64_t M, int64_t N, int64_t K, int64_t ksplit, c10::optional<at::Tensor> outF,
          c10::optional<at::Tensor> outH, int64_t ldo, c10::optional<at::Tensor> bias,
          c10::optional<at::Tensor> mask, int64_t ldm, double mask_scale,
          c10::optional<at::Tensor> colsum, double alpha, double beta, int64_t act, bool atomic,
          double drop_p, int64_t seed, int64_t big_tile, c10::optional<at::Tensor> seed_dev) {
  const GemmCall c = gemm_prepare(A, a_mn, lda, B, b_mn, ldb, M, N, K, ksplit, outF, outH, ldo, bias, mask, ldm,
                                  mask_scale, colsum, alpha, beta, act, atomic, drop_p, seed, big_tile, seed_dev, true);
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(A.device());
  wf::launch_gemm(bfp(A), lda, a_mn, bfp(B), ldb, b_mn, (int)M, (int)N, (int)K, (int)ksplit, c.e,
                  cur_stream(), c.glds_ok);
}

// The route gemm takes for these arguments (kernels.h gemm_plan, the function launch_gemm itself
// calls), after the same checks; nothing is launched, so CPU tensors of the same sizes will do.
py::dict gemm_plan(const at::Tensor& A, bool a_mn, int64_t lda, const at::Tensor& B, bool b_mn, int64_t ldb,
                   int64_t M, int64_t N, int64_t K, int64_t ksplit, c10::optional<at::Tensor> outF,
                   c10::optional<at::Tensor> outH, int64_t ldo, c10::optional<at::Tensor> bias,
                   c10::optional<at::Tensor> mask, int64_t ldm, double mask_scale,
                   c10::optional<at::Tensor> colsum, double alpha, double beta, int64_t act, bool atomic,
                   double drop_p, int64_t seed, int64_t big_tile, c10::optional<at::Tensor> seed_dev) {
  const GemmCall c = gemm_prepare(A, a_mn, lda, B, b_mn, ldb, M, N, K, ksplit, outF, outH, ldo, bias, mask, ldm,
                                  mask_scale, colsum, alpha, beta, act, atomic, drop_p, seed, big_tile, seed_dev, false);
  const wf::GemmPlan p = wf::gemm_plan(a_mn, b_mn, (int)M, (int)N, (int)K, (int)ksplit, c.e, c.glds_ok);
  py::dict d;
  d["kernel"] = wf::gemm_kernel_name(p.kernel);
  d["mainloop"] = p.ring ? "ring" : "register";
  d["epilogue"] = p.staged ? "staged" : "direct";
  d["kchunk"] = p.kchunk;
  d["nsplit"] = p.nsplit;
  d["workgroups"] = p.workgroups;
  return d;
}

wf::LstmDims lstm_dims(int64_t B, int64_t T, int64_t F, int64_t KX, int64_t H) {
  TORCH_CHECK(B > 0 && T > 0 && H > 0, "lstm: bad dims");
  TORCH_CHECK(H % 128 == 0, "lstm: hidden size must be a multiple of 128");
  TORCH_CHECK(KX % 64 == 0 && F + 1 <= KX, "lstm: KX must be a multiple of 64 and > F");
  wf::LstmDims d;
  d.B = (int)B; d.T = (int)T; d.F = (int)F; d.KX = (int)KX; d.H = (int)H;
  d.xcd_map = diag_env("WELLFLOW_XCD_MAP", 1) == 0 ? 0 : 1;  // diagnostics: 0 = identity tile order
  d.nt = diag_env("WELLFLOW_NT", 1) == 0 ? 0 : 1;
  // WELLFLOW_PF_DBG: timing-only switches and A/B variants of the persistent kernels. Only a
  // WF_DIAG build of the HIP objects (WELLFLOW_DIAG_BUILD=1) honours them: dbg_mask() is the
  // mask the objects were compiled with, so a production _C.so ignores the variable
  // (tests/test_diag_cpu.py checks this call stays here; bench.py refuses to run with it set).
  const char* pd = std::getenv("WELLFLOW_PF_DBG");
  d.dbg = (pd != nullptr ? std::atoi(pd) : 0) & wf::dbg_mask();
  const char* sl = std::getenv("WELLFLOW_SPIN_LIMIT");  // tests: force the hand-off timeout path
  d.spin_limit = sl != nullptr ? (unsigned)std::strtoul(sl, nullptr, 10) : 0u;
  const char* ft = std::getenv("WELLFLOW_FORCE_TIMEOUT");  // tests: every hand-off wait trips its bound
  if (ft != nullptr && ft[0] == '1') d.dbg |= 1 << 21;  // fails the run loudly (STAT block)
  return d;
}

void check_lstm_state(const at::Tensor& XH, const at::Tensor& Cst, const at::Tensor& S,
                      const wf::LstmDims& d) {
  const int64_t KA = d.KX + d.H, G = 4 * d.H;
  const int64_t Bp = (d.B + 15) / 16 * 16;  // fragment-native state is padded to 16 rows
  check_t(XH, at::kBFloat16, "XH");
  check_t(Cst, at::kBFloat16, "Cst");  // bf16 cell-state history (lstm_layout.h)
  check_t(S, at::kBFloat16, "S");
  check_extent(XH, (int64_t)(d.T + 1) * d.B * KA, "XH");
  check_extent(Cst, (int64_t)(d.T + 1) * Bp * d.H, "Cst");
  check_extent(S, (int64_t)d.T * Bp * G, "S");
}

// full = false: only the feature chunks (the buffer's constant 1 column / zero padding were
// written by an earlier full pack of the same B)
void lstm_pack_x(const at::Tensor& x, const at::Tensor& XH, int64_t B, int64_t T, int64_t F,
                 int64_t KX, int64_t H, bool full) {
  auto d = lstm_dims(B, T, F, KX, H);
  check_t(x, at::kFloat, "x");
  check_extent(x, B * T * F, "x");
  check_t(XH, at::kBFloat16, "XH");
  check_extent(XH, (T + 1) * B * (KX + H), "XH");
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(x.device());
  wf::launch_lstm_pack_x(fp(x), bfp(XH), d, cur_stream(), full);
}

// the batch's windows read in place from the resident row table: batch row b = rows
// starts[idx[b]] .. + T - 1 of `table` (data/features.py SeriesWindows)
void lstm_pack_x_win(const at::Tensor& table, const at::Tensor& starts, const at::Tensor& idx, const at::Tensor& XH,
                     int64_t B, int64_t T, int64_t F, int64_t KX, int64_t H, bool full) {
  auto d = lstm_dims(B, T, F, KX, H);
  check_t(table, at::kFloat, "table");
  TORCH_CHECK(table.dim() == 2 && table.size(1) == F && table.size(0) >= T, "lstm_pack_x_win: table must be [>= T][F]");
  check_t(starts, at::kLong, "starts");
  check_t(idx, at::kLong, "idx");
  check_extent(idx, B, "idx");
  TORCH_CHECK(starts.numel() >= 1, "lstm_pack_x_win: no windows");
  check_t(XH, at::kBFloat16, "XH");
  check_extent(XH, (T + 1) * B * (KX + H), "XH");
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(table.device());
  wf::launch_lstm_pack_x(fp(table), bfp(XH), d, cur_stream(), full, reinterpret_cast<const long*>(starts.data_ptr<int64_t>()),
                         reinterpret_cast<const long*>(idx.data_ptr<int64_t>()), starts.numel(), table.size(0));
}

// cf32: fp32 [Bp][H] in-place state slab of the per-step path (c_{t-1} -> c_t; e.g. the
// engine's dcarry buffer, which the backward re-initialises)
void lstm_forward(const at::Tensor& XH, const at::Tensor& Wp, const at::Tensor& Cst,
                  const at::Tensor& S, const at::Tensor& cf32, int64_t B, int64_t T, int64_t F, int64_t KX,
                  int64_t H, int64_t variant) {
  auto d = lstm_dims(B, T, F, KX, H);
  d.fwd_variant = (int)variant;
  check_lstm_state(XH, Cst, S, d);
  check_t(Wp, at::kBFloat16, "Wp");
  check_extent(Wp, 4 * H * (KX + H), "Wp");
  check_t(cf32, at::kFloat, "cf32");
  check_extent(cf32, (B + 15) / 16 * 16 * H, "cf32");
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(XH.device());
  auto s = cur_stream();
  for (int t = 0; t < d.T; ++t) wf::launch_lstm_fwd_step(t, bfp(XH), bfp(Wp), bfp(Cst), bfp(S), fp(cf32), d, s);
}

// A persistent kernel's sync buffer: int32, 16-B aligned, zeroed once by its owner. No launch
// resets it (csrc/persistent_sync.h: monotonic launch epochs and arrival counters), so there is
// no memset node in a captured step at all (round 2's early exit was an unaligned per-launch
// memset node under graph replay, profiles/r3_early_exit.md).
void check_sync(const at::Tensor& sync) {
  check_t(sync, at::kInt, "sync");  // check_t: 16-B aligned data pointer
}

// Raise on a failed persistent launch (status < 0: -(hipError_t)); 0 = not supported.
bool persistent_status(int st, const char* what) {
  TORCH_CHECK(st >= 0, what, ": launch failed: ", hipGetErrorString((hipError_t)(-st)));
  return st == 1;
}

// All T steps in one persistent launch per sub-batch (lstm_persistent.hip). Returns false
// (nothing launched) when the shape or device cannot host it and raises when the launch
// fails; `sync` (int32): csrc/persistent_sync.h (hand-off words) + the STAT block at its end.
bool lstm_forward_persistent(const at::Tensor& XH, const at::Tensor& Wp, const at::Tensor& Cst,
                             const at::Tensor& S, const at::Tensor& sync, int64_t B, int64_t T, int64_t F,
                             int64_t KX, int64_t H) {
  auto d = lstm_dims(B, T, F, KX, H);
  check_lstm_state(XH, Cst, S, d);
  check_t(Wp, at::kBFloat16, "Wp");
  check_extent(Wp, 4 * H * (KX + H), "Wp");
  check_sync(sync);
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(XH.device());
  return persistent_status(wf::launch_lstm_fwd_persistent(bfp(XH), bfp(Wp), bfp(Cst), bfp(S),
                                                          reinterpret_cast<unsigned*>(sync.data_ptr<int>()),
                                                          sync.numel(), d, cur_stream()),
                           "persistent LSTM forward");
}

// Operands of the BPTT chain (lstm_backward, lstm_backward_dw) next to the forward state.
void check_lstm_bwd(const at::Tensor& WhhT, const at::Tensor& DG, const at::Tensor& dcarry, const at::Tensor& dy,
                    const at::Tensor& w_out, int64_t B, int64_t T, int64_t H) {
  check_t(WhhT, at::kBFloat16, "WhhT");
  check_extent(WhhT, H * 4 * H, "WhhT");
  check_t(DG, at::kBFloat16, "DG");
  check_extent(DG, T * B * 4 * H, "DG");
  check_t(dcarry, at::kFloat, "dcarry");
  check_extent(dcarry, (B + 15) / 16 * 16 * H, "dcarry");
  check_t(dy, at::kFloat, "dy");
  check_extent(dy, B, "dy");
  check_t(w_out, at::kFloat, "w_out");
  check_extent(w_out, H, "w_out");
}

void lstm_backward(const at::Tensor& WhhT, const at::Tensor& XH, const at::Tensor& Cst,
                   const at::Tensor& S, const at::Tensor& DG, const at::Tensor& dcarry,
                   const at::Tensor& dy, const at::Tensor& w_out, int64_t B, int64_t T, int64_t F,
                   int64_t KX, int64_t H, int64_t variant, const c10::optional<at::Tensor>& sync) {
  auto d = lstm_dims(B, T, F, KX, H);
  d.bwd_variant = (int)variant;
  check_lstm_state(XH, Cst, S, d);
  check_lstm_bwd(WhhT, DG, dcarry, dy, w_out, B, T, H);
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(XH.device());
  auto s = cur_stream();
  if (sync.has_value()) {  // step T-1, then the persistent chain (tools/pb_time.py)
    check_sync(*sync);
    wf::launch_lstm_bwd_step(d.T - 1, bfp(WhhT), bfp(Cst), bfp(S), bfp(DG), fp(dcarry), fp(dy),
                             fp(w_out), d, s);
    TORCH_CHECK(persistent_status(wf::launch_lstm_bwd_persistent(bfp(WhhT), bfp(Cst), bfp(S), bfp(DG), fp(dcarry),
                                                                 reinterpret_cast<unsigned*>(sync->data_ptr<int>()),
                                                                 sync->numel(), d, s),
                                  "persistent LSTM backward"),
                "persistent backward refused this shape");
    return;
  }
  for (int t = d.T - 1; t >= 0; --t)
    wf::launch_lstm_bwd_step(t, bfp(WhhT), bfp(Cst), bfp(S), bfp(DG), fp(dcarry), fp(dy),
                             fp(w_out), d, s);
}

// Two persistent side streams per device for the backward pass: the serial BPTT chain
// runs on a HIGH-priority stream, the weight-gradient GEMM chunks on a LOW-priority one,
// fork/joined to the caller's stream with events (capturable in a hipGraph).
struct SideStreams {
  hipStream_t hi = nullptr, lo = nullptr;
  std::vector<hipEvent_t> ev;
};

SideStreams& side_streams(int dev, size_t nev) {
  static std::mutex mu;
  static std::map<int, SideStreams> all;
  std::lock_guard<std::mutex> g(mu);
  SideStreams& ss = all[dev];
  if (ss.hi == nullptr) {
    int least = 0, greatest = 0;
    TORCH_CHECK(hipDeviceGetStreamPriorityRange(&least, &greatest) == hipSuccess, "stream priorities");
    TORCH_CHECK(hipStreamCreateWithPriority(&ss.hi, hipStreamNonBlocking, greatest) == hipSuccess,
                "hi stream");
    TORCH_CHECK(hipStreamCreateWithPriority(&ss.lo, hipStreamNonBlocking, least) == hipSuccess,
                "lo stream");
  }
  while (ss.ev.size() < nev) {
    hipEvent_t e;
    TORCH_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming) == hipSuccess, "event");
    ss.ev.push_back(e);
  }
  return ss;
}

// Full LSTM backward: BPTT chain + dWcat = sum_t DG[t]^T XH[t] into gW (fp32 [G][KA],
// accumulated with atomics, so it must be zeroed by the caller). With chunk > 0 the dW
// GEMM is cut into chunks of `chunk` timesteps, each launched on the low-priority stream
// as soon as the chain has produced its DG slabs: compute-bound dW work fills the gaps of
// the memory/latency-bound chain instead of running after it.
// Returns true when the BPTT chain ran as the persistent kernel (false: per-step kernels).
bool lstm_backward_dw(const at::Tensor& WhhT, const at::Tensor& XH, const at::Tensor& Cst,
                      const at::Tensor& S, const at::Tensor& DG, const at::Tensor& dcarry,
                      const at::Tensor& dy, const at::Tensor& w_out, const at::Tensor& gW,
                      int64_t B, int64_t T, int64_t F, int64_t KX, int64_t H, int64_t variant,
                      int64_t chunk, int64_t ksplit, const c10::optional<at::Tensor>& sync,
                      const c10::optional<at::Tensor>& dw_slab) {
  auto d = lstm_dims(B, T, F, KX, H);
  d.bwd_variant = (int)variant;
  check_lstm_state(XH, Cst, S, d);
  check_lstm_bwd(WhhT, DG, dcarry, dy, w_out, B, T, H);
  check_t(gW, at::kFloat, "gW");
  const int64_t G = 4 * H, KA = KX + H;
  check_extent(gW, G * KA, "gW");
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(XH.device());
  hipStream_t main = cur_stream();

  auto dw = [&](int t0, int t1, hipStream_t s) {
    const int64_t K = (int64_t)(t1 - t0) * B;
    wf::GemmEpilogue e;
    e.outF = fp(gW);
    e.ldo = KA;
    e.atomic = 1;
    e.big_tile = wf::kDwBest;
    if (dw_slab.has_value()) {  // split-K partials plain-stored, one reduce (gemm.hip launch_dw_288w)
      check_t(*dw_slab, at::kFloat, "dw_slab");
      e.slab = fp(*dw_slab);
      e.slab_cap = dw_slab->numel();
    }
    const bf16_t* A = bfp(DG) + (size_t)t0 * B * G;
    const bf16_t* Bm = bfp(XH) + (size_t)t0 * B * KA;
    // whole-tile over-read of XH columns 576..639 stays inside XH (its slab T follows)
    int64_t ks = std::max<int64_t>(1, ksplit);
    int64_t kchunk = ((K + ks - 1) / ks + 63) / 64 * 64;
    const bool glds_ok = (K % 64 == 0) && (kchunk % 64 == 0) && !disable_glds();
    wf::launch_gemm(A, G, 1, Bm, KA, 1, (int)G, (int)KA, (int)K, (int)ks, e, s, glds_ok);
  };

  if (chunk <= 0) {
    // step T-1 (dh from the head), then steps T-2 .. 0 in one persistent launch when a sync
    // buffer is given and the shape fits (lstm_persistent_bwd.hip), else per-step kernels
    wf::launch_lstm_bwd_step(d.T - 1, bfp(WhhT), bfp(Cst), bfp(S), bfp(DG), fp(dcarry), fp(dy),
                             fp(w_out), d, main);
    bool done = false;
    if (sync.has_value()) {
      check_sync(*sync);
      done = persistent_status(wf::launch_lstm_bwd_persistent(bfp(WhhT), bfp(Cst), bfp(S), bfp(DG), fp(dcarry),
                                                              reinterpret_cast<unsigned*>(sync->data_ptr<int>()),
                                                              sync->numel(), d, main),
                               "persistent LSTM backward");
    }
    if (!done)
      for (int t = d.T - 2; t >= 0; --t)
        wf::launch_lstm_bwd_step(t, bfp(WhhT), bfp(Cst), bfp(S), bfp(DG), fp(dcarry), fp(dy),
                                 fp(w_out), d, main);
    dw(0, d.T, main);
    return done;
  }
  const int nchunks = (int)((T + chunk - 1) / chunk);
  SideStreams& ss = side_streams(XH.device().index(), nchunks + 3);
  TORCH_CHECK(hipEventRecord(ss.ev[0], main) == hipSuccess, "event record");
  TORCH_CHECK(hipStreamWaitEvent(ss.hi, ss.ev[0], 0) == hipSuccess, "wait");
  TORCH_CHECK(hipStreamWaitEvent(ss.lo, ss.ev[0], 0) == hipSuccess, "wait");
  int t_end = d.T, k = 0;
  for (int t = d.T - 1; t >= 0; --t) {
    wf::launch_lstm_bwd_step(t, bfp(WhhT), bfp(Cst), bfp(S), bfp(DG), fp(dcarry), fp(dy),
                             fp(w_out), d, ss.hi);
    if (t % chunk == 0) {  // DG[t .. t_end) complete
      hipEvent_t e = ss.ev[3 + k++];
      TORCH_CHECK(hipEventRecord(e, ss.hi) == hipSuccess, "event record");
      TORCH_CHECK(hipStreamWaitEvent(ss.lo, e, 0) == hipSuccess, "wait");
      dw(t, t_end, ss.lo);
      t_end = t;
    }
  }
  TORCH_CHECK(hipEventRecord(ss.ev[1], ss.hi) == hipSuccess, "event record");
  TORCH_CHECK(hipEventRecord(ss.ev[2], ss.lo) == hipSuccess, "event record");
  TORCH_CHECK(hipStreamWaitEvent(main, ss.ev[1], 0) == hipSuccess, "join");
  TORCH_CHECK(hipStreamWaitEvent(main, ss.ev[2], 0) == hipSuccess, "join");
  return false;
}

// The clipnorm state block of grad_clip_scale (csrc/elementwise.hip) as the fused updates take it;
// none = no clipnorm.
const float* clip_state(const c10::optional<at::Tensor>& clip) {
  return opt_ptr<float>(clip, at::kFloat, "clip", wf::kGradClipStateFloats);
}

// Adam on the LSTM's flat parameters + Wp / WhhT (lstm_pack_weights' output) in one launch
void lstm_adam_pack(const at::Tensor& p, const at::Tensor& g, const at::Tensor& m, const at::Tensor& v,
                    const at::Tensor& step, double lr, double b1, double b2, double eps, double wd, double gscale,
                    bool zero_g, const at::Tensor& Wp, const at::Tensor& WhhT, int64_t H, int64_t KX,
                    c10::optional<at::Tensor> clip, double clipvalue) {
  for (const at::Tensor* t : {&p, &g, &m, &v}) check_t(*t, at::kFloat, "p/g/m/v");
  const int64_t n = p.numel();
  TORCH_CHECK(g.numel() == n && m.numel() == n && v.numel() == n, "lstm_adam_pack: size mismatch");
  TORCH_CHECK(KX % 32 == 0 && H % 32 == 0 && n >= 4 * H * (KX + H), "lstm_adam_pack: layout (KX, H multiples of 32)");
  for (const at::Tensor* t : {&p, &g, &m, &v})
    TORCH_CHECK(reinterpret_cast<uintptr_t>(t->data_ptr()) % 16 == 0, "lstm_adam_pack: buffers must be 16-B aligned");
  check_t(step, at::kFloat, "step");
  check_extent(step, 2, "step");
  check_t(Wp, at::kBFloat16, "Wp");
  check_t(WhhT, at::kBFloat16, "WhhT");
  check_extent(Wp, 4 * H * (KX + H), "Wp");
  check_extent(WhhT, H * 4 * H, "WhhT");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(Wp.data_ptr()) % 8 == 0, "lstm_adam_pack: Wp must be 8-B aligned");
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(p.device());
  wf::launch_lstm_adam_pack(fp(p), fp(g), fp(m), fp(v), n, fp(step), (float)lr, (float)b1, (float)b2, (float)eps,
                            (float)wd, (float)gscale, zero_g ? 1 : 0, (int)KX, (int)H, bfp(Wp), bfp(WhhT), cur_stream(),
                            clip_state(clip), (float)clipvalue);
}

void lstm_pack_weights(const at::Tensor& W, const at::Tensor& Wp, const at::Tensor& WhhT,
                       int64_t H, int64_t KX) {
  auto d = lstm_dims(1, 1, 0, KX, H);
  check_t(W, at::kFloat, "W");
  check_t(Wp, at::kBFloat16, "Wp");
  check_t(WhhT, at::kBFloat16, "WhhT");
  check_extent(W, 4 * H * (KX + H), "W");
  check_extent(Wp, 4 * H * (KX + H), "Wp");
  check_extent(WhhT, H * 4 * H, "WhhT");
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(W.device());
  wf::launch_lstm_pack_weights(fp(W), bfp(Wp), bfp(WhhT), d, cur_stream());
}

// Regression-head input H may be a strided view of a larger bf16 buffer (e.g. the last
// timestep of XH): the raw pointer is taken from the given tensor (its storage offset).
void check_head_h(const at::Tensor& Hm, int64_t ldh, int64_t B, int64_t Hd) {
  TORCH_CHECK(Hm.is_cuda() && Hm.scalar_type() == at::kBFloat16, "H: bf16 GPU tensor");
  TORCH_CHECK(Hd % 8 == 0 && ldh % 8 == 0 && Hd <= 2048, "head: Hd, ldh multiples of 8, Hd <= 2048");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(Hm.data_ptr()) % 16 == 0, "head: H must be 16-B aligned");
  TORCH_CHECK(ldh >= Hd, "head: ldh < Hd");
  TORCH_CHECK(Hm.storage().nbytes() - Hm.storage_offset() * 2 >= (size_t)(((B - 1) * ldh + Hd) * 2),
              "head: H too small");
}

void head_fwd(const at::Tensor& Hm, int64_t ldh, int64_t B, int64_t Hd, const at::Tensor& w,
              const at::Tensor& b0, c10::optional<at::Tensor> target, const at::Tensor& pred,
              c10::optional<at::Tensor> dy, c10::optional<at::Tensor> loss_sum, double dy_scale) {
  check_head_h(Hm, ldh, B, Hd);
  TORCH_CHECK(Hd % 8 == 0 && ldh % 8 == 0, "head: Hd and ldh must be multiples of 8");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(Hm.data_ptr()) % 16 == 0, "head: H must be 16-B aligned");
  check_t(w, at::kFloat, "w");
  check_extent(w, Hd, "w");
  check_t(b0, at::kFloat, "b0");
  check_t(pred, at::kFloat, "pred");
  check_extent(pred, B, "pred");
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(Hm.device());
  wf::launch_head_fwd(bfp(Hm), ldh, (int)B, (int)Hd, fp(w), fp(b0),
                      opt_ptr<float>(target, at::kFloat, "target", B), fp(pred),
                      opt_ptr<float>(dy, at::kFloat, "dy", B),
                      opt_ptr<float>(loss_sum, at::kFloat, "loss_sum", 1), (float)dy_scale,
                      cur_stream());
}

// Fused MLP backward (mlp_fused.hip) for the F -> 256 -> 256 -> 1 shape: dZ2, dZ1 and the
// bias / head gradients in one launch (the dW GEMMs stay separate).
// ReLU bitmask of the MLP's second hidden layer: int32 [B][8] (256 bits per row), 16-B aligned
static unsigned* mask_ptr(const c10::optional<at::Tensor>& M2, int64_t B) {
  if (!M2.has_value()) return nullptr;
  check_t(*M2, at::kInt, "M2");
  check_extent(*M2, B * 8, "M2");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(M2->data_ptr()) % 16 == 0, "M2 must be 16-B aligned");
  return reinterpret_cast<unsigned*>(M2->data_ptr<int>());
}

static const long long* rows_ptr(const c10::optional<at::Tensor>& rows, int64_t B) {
  if (!rows.has_value() || !rows->defined()) return nullptr;
  TORCH_CHECK(rows->is_cuda() && rows->scalar_type() == at::kLong && rows->is_contiguous(), "rows: contiguous int64 GPU tensor");
  TORCH_CHECK(rows->numel() >= B, "rows: needs ", B, " indices");
  return reinterpret_cast<const long long*>(rows->data_ptr<int64_t>());
}

// X rows read by a kernel: B rows directly, or dataset rows named by `rows`. Returns the
// dataset row count; the kernels CLAMP every index into [0, nrows) (an out-of-range index
// must never become an out-of-bounds device read, and checking here would need a host sync,
// which a captured hipGraph step cannot do).
static int64_t check_x_rows(const at::Tensor& X, int64_t Fp, int64_t B, const c10::optional<at::Tensor>& rows) {
  if (!rows.has_value() || !rows->defined()) {
    check_extent(X, B * Fp, "X");
    return B;
  }
  const int64_t nrows = X.numel() / Fp;
  TORCH_CHECK(nrows > 0, "X: empty dataset");
  return nrows;
}

bool mlp2_backward(c10::optional<at::Tensor> H1, const at::Tensor& H2, const at::Tensor& dy, const at::Tensor& w3,
                   const at::Tensor& W2, const at::Tensor& X, int64_t Fp, const at::Tensor& dZ1,
                   const at::Tensor& dZ2, c10::optional<at::Tensor> dW1, const at::Tensor& db1,
                   const at::Tensor& db2, const at::Tensor& dw3, const at::Tensor& db3, int64_t B,
                   c10::optional<at::Tensor> M2, c10::optional<at::Tensor> W1, c10::optional<at::Tensor> b1,
                   c10::optional<at::Tensor> rows, c10::optional<at::Tensor> red) {
  constexpr int64_t H = 256;
  const bool recompute = !H1.has_value() || !H1->defined();
  std::vector<const at::Tensor*> acts = {&H2, &dZ1, &dZ2};
  if (!recompute) acts.push_back(&*H1);
  for (const at::Tensor* t : acts) {
    check_t(*t, at::kBFloat16, "H/dZ");
    check_extent(*t, B * H, "H/dZ");
  }
  check_t(W2, at::kBFloat16, "W2");
  check_extent(W2, H * H, "W2");
  check_t(dy, at::kFloat, "dy");
  check_extent(dy, B, "dy");
  for (const at::Tensor* t : {&w3, &db1, &db2, &dw3}) {
    check_t(*t, at::kFloat, "w3/db");
    check_extent(*t, H, "w3/db");
  }
  check_t(db3, at::kFloat, "db3");
  check_extent(db3, 1, "db3");
  check_t(X, at::kBFloat16, "X");
  const int64_t nrows = check_x_rows(X, Fp, B, rows);
  const bf16_t* w1p = opt_ptr<bf16_t>(W1, at::kBFloat16, "W1", H * Fp);
  const float* b1p = opt_ptr<float>(b1, at::kFloat, "b1", H);
  TORCH_CHECK(!recompute || (w1p && b1p && dW1.has_value()), "mlp2_backward: H1 recompute needs W1, b1 and dW1");
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(H2.device());
  return wf::launch_mlp2_bwd(recompute ? nullptr : bfp(*H1), bfp(H2), mask_ptr(M2, B), fp(dy), fp(w3), bfp(W2), bfp(X),
                             (int)Fp, bfp(dZ1), bfp(dZ2), opt_ptr<float>(dW1, at::kFloat, "dW1", H * Fp), fp(db1),
                             fp(db2), fp(dw3), fp(db3), (int)B, w1p, b1p, rows_ptr(rows, B), nrows, cur_stream(),
                             opt_ptr<float>(red, at::kFloat, "red", wf::kMlpRedFloats));
}

// dW2 [256][256] += dZ2^T relu(X W1^T + b1), H1 recomputed (mlp_fused.hip mlp2_dw2_kernel).
bool mlp2_dw2(const at::Tensor& dZ2, const at::Tensor& X, int64_t Fp, c10::optional<at::Tensor> rows,
              const at::Tensor& W1, const at::Tensor& b1, int64_t B, int64_t nsplit, const at::Tensor& dW2,
              c10::optional<at::Tensor> red) {
  constexpr int64_t H = 256;
  check_t(dZ2, at::kBFloat16, "dZ2");
  check_extent(dZ2, B * H, "dZ2");
  check_t(X, at::kBFloat16, "X");
  const int64_t nrows = check_x_rows(X, Fp, B, rows);
  check_t(W1, at::kBFloat16, "W1");
  check_extent(W1, H * Fp, "W1");
  check_t(b1, at::kFloat, "b1");
  check_extent(b1, H, "b1");
  check_t(dW2, at::kFloat, "dW2");
  check_extent(dW2, H * H, "dW2");
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(dZ2.device());
  return wf::launch_mlp2_dw2(bfp(dZ2), bfp(X), (int)Fp, rows_ptr(rows, B), nrows, bfp(W1), fp(b1), (int)B, (int)nsplit,
                             fp(dW2), cur_stream(), opt_ptr<float>(red, at::kFloat, "red", wf::kMlpRedFloats));
}

// Sums the spread-reduction scratch of the 8-wave MLP training kernels into the gradients
// (mlp_fused.hip mlp2_reduce_kernel) and zeroes it; null destinations are skipped.
void mlp2_reduce(const at::Tensor& red, int64_t Fp, int64_t B, c10::optional<at::Tensor> loss_sum, const at::Tensor& db3,
                 const at::Tensor& dw3, const at::Tensor& db1, const at::Tensor& db2, const at::Tensor& dW1,
                 c10::optional<at::Tensor> dW2, int64_t dw2_rows) {
  constexpr int64_t H = 256;
  check_t(red, at::kFloat, "red");
  check_extent(red, wf::kMlpRedFloats, "red");
  TORCH_CHECK(Fp > 0 && Fp <= 64, "mlp2_reduce: Fp <= 64");
  for (const at::Tensor* t : {&dw3, &db1, &db2}) {
    check_t(*t, at::kFloat, "dw3/db");
    check_extent(*t, H, "dw3/db");
  }
  check_t(db3, at::kFloat, "db3");
  check_extent(db3, 1, "db3");
  check_t(dW1, at::kFloat, "dW1");
  check_extent(dW1, H * Fp, "dW1");
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(red.device());
  TORCH_CHECK(B > 0, "mlp2_reduce: B > 0");
  wf::launch_mlp2_reduce(fp(red), (int)Fp, (int)B, opt_ptr<float>(loss_sum, at::kFloat, "loss_sum", 1), fp(db3), fp(dw3),
                         fp(db1), fp(db2), fp(dW1), opt_ptr<float>(dW2, at::kFloat, "dW2", H * H), cur_stream(),
                         (int)dw2_rows);
}

// MLP training step forward + backward in one launch (mlp_step.hip); the batch sums land in
// the spread scratch `red` (mlp2_reduce adds them), dZ2 feeds mlp2_dw2. False = not covered.
bool mlp2_step(const at::Tensor& X, int64_t Fp, const at::Tensor& W1, const at::Tensor& b1, const at::Tensor& W2,
               const at::Tensor& b2, const at::Tensor& w3, const at::Tensor& b3, const at::Tensor& y, double dy_scale,
               int64_t B, c10::optional<at::Tensor> rows, const at::Tensor& dZ2, c10::optional<at::Tensor> pred,
               const at::Tensor& red, bool dz_frag, c10::optional<at::Tensor> W2T, double clip) {
  constexpr int64_t H = 256;
  check_t(X, at::kBFloat16, "X");
  const int64_t nrows = check_x_rows(X, Fp, B, rows);
  check_t(W1, at::kBFloat16, "W1");
  check_extent(W1, H * Fp, "W1");
  check_t(W2, at::kBFloat16, "W2");
  check_extent(W2, H * H, "W2");
  for (const at::Tensor* t : {&b1, &b2, &w3}) {
    check_t(*t, at::kFloat, "bias/w3");
    check_extent(*t, H, "bias/w3");
  }
  check_t(b3, at::kFloat, "b3");
  check_extent(b3, 1, "b3");
  check_t(y, at::kFloat, "y");
  check_extent(y, nrows, "y");
  check_t(dZ2, at::kBFloat16, "dZ2");
  check_extent(dZ2, B * H, "dZ2");
  check_t(red, at::kFloat, "red");
  check_extent(red, wf::kMlpRedFloats, "red");
  for (const at::Tensor* t : {&X, &W1, &W2, &dZ2})
    TORCH_CHECK(reinterpret_cast<uintptr_t>(t->data_ptr()) % 16 == 0, "mlp2_step: bf16 operands must be 16-B aligned");
  TORCH_CHECK(B > 0, "mlp2_step: B > 0");
  const bf16_t* w2t = nullptr;
  if (W2T.has_value()) {
    check_t(*W2T, at::kBFloat16, "W2T");
    check_extent(*W2T, H * H, "W2T");
    TORCH_CHECK(reinterpret_cast<uintptr_t>(W2T->data_ptr()) % 16 == 0, "mlp2_step: W2T must be 16-B aligned");
    w2t = bfp(*W2T);
  }
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(X.device());
  return wf::launch_mlp2_step(bfp(X), (int)Fp, bfp(W1), fp(b1), bfp(W2), fp(b2), fp(w3), fp(b3), fp(y), (float)dy_scale,
                              (int)B, rows_ptr(rows, B), nrows, bfp(dZ2), opt_ptr<float>(pred, at::kFloat, "pred", B),
                              fp(red), dz_frag, cur_stream(), w2t, (float)clip);
}

int64_t mlp_small_scratch_floats() { return wf::kMlpSmallScratch; }



// K small-batch MLP training steps (forward, backward, Adam) in ONE persistent launch
// (mlp_small.hip). X / Y: the dataset (bf16 [N][Fp], fp32 [N]) read through rows [K * B] (or
// contiguous from row 0); params / m / v / step: the flat parameters and FlatAdam state, updated
// in place; offs: (W1, b1, W2, b2, w3, b3) element offsets of the MlpLayout. False = not covered.
bool mlp_small_steps(const at::Tensor& X, const at::Tensor& Y, c10::optional<at::Tensor> rows, int64_t Fp, int64_t B,
                     int64_t K, const at::Tensor& params, const at::Tensor& m, const at::Tensor& v,
                     const at::Tensor& step, double lr, double b1, double b2, double eps, double wd, double dy_scale,
                     double clip, c10::optional<at::Tensor> shadow, c10::optional<at::Tensor> w2t,
                     c10::optional<at::Tensor> loss_acc, const at::Tensor& scr, const at::Tensor& sync,
                     std::vector<int64_t> offs, c10::optional<at::Tensor> stamps) {
  constexpr int64_t H = 256;
  TORCH_CHECK(offs.size() == 6, "mlp_small_steps: offs = (W1, b1, W2, b2, w3, b3)");
  TORCH_CHECK(K > 0 && B > 0, "mlp_small_steps: K, B > 0");
  check_t(X, at::kBFloat16, "X");
  check_t(Y, at::kFloat, "Y");
  int64_t nrows;
  const long long* rp = nullptr;
  if (rows.has_value() && rows->defined()) {
    rp = rows_ptr(rows, K * B);
    nrows = X.numel() / Fp;
    TORCH_CHECK(nrows > 0, "X: empty dataset");
  } else {
    check_extent(X, K * B * Fp, "X");
    nrows = K * B;
  }
  check_extent(Y, nrows, "Y");
  const int64_t n = params.numel();
  for (const at::Tensor* t : {&params, &m, &v}) {
    check_t(*t, at::kFloat, "params/m/v");
    check_extent(*t, n, "params/m/v");
  }
  TORCH_CHECK(offs[0] + H * Fp <= n && offs[2] + H * H <= n && offs[5] < n && offs[1] + H <= n && offs[3] + H <= n &&
                  offs[4] + H <= n, "mlp_small_steps: parameter offsets out of range");
  check_t(step, at::kFloat, "step");
  check_t(scr, at::kFloat, "scr");
  check_extent(scr, wf::kMlpSmallScratch, "scr");
  check_t(sync, at::kInt, "sync");
  check_extent(sync, 4, "sync");
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(X.device());
  wf::MlpSmallArgs a{};
  a.X = bfp(X);
  a.Y = fp(Y);
  a.rows = rp;
  a.nrows = (long)nrows;
  a.Fp = (int)Fp;
  a.B = (int)B;
  a.K = (int)K;
  a.p = fp(params);
  a.m = fp(m);
  a.v = fp(v);
  a.step = fp(step);
  a.lr = (float)lr;
  a.b1 = (float)b1;
  a.b2 = (float)b2;
  a.eps = (float)eps;
  a.wd = (float)wd;
  a.dy_scale = (float)dy_scale;
  a.clip = (float)clip;
  a.shadow = opt_ptr<bf16_t>(shadow, at::kBFloat16, "shadow", n);
  a.w2t = opt_ptr<bf16_t>(w2t, at::kBFloat16, "w2t", H * H);
  a.loss_acc = opt_ptr<float>(loss_acc, at::kFloat, "loss_acc", 1);
  a.scr = fp(scr);
  a.sync = reinterpret_cast<unsigned*>(sync.data_ptr<int>());
  const char* sl = std::getenv("WELLFLOW_SPIN_LIMIT");  // tests: force the hand-off timeout path
  a.spin_limit = sl != nullptr ? (unsigned)std::strtoul(sl, nullptr, 10) : (1u << 22);
  a.oW1 = (long)offs[0];
  a.ob1 = (long)offs[1];
  a.oW2 = (long)offs[2];
  a.ob2 = (long)offs[3];
  a.ow3 = (long)offs[4];
  a.ob3 = (long)offs[5];
  a.stamps = reinterpret_cast<unsigned long long*>(opt_ptr<int64_t>(stamps, at::kLong, "stamps", 16 * 64 * 16));
  return wf::launch_mlp_small(a, cur_stream());
}

// dW2 from the fragment-layout dZ2 of mlp2_step(dz_frag=True) into the spread scratch's dW2
// copies (mlp_step.hip mlp2_dw2f_kernel; mlp2_reduce adds them). False = not covered.
int64_t mlp2_dw2f(const at::Tensor& dZ2F, const at::Tensor& X, int64_t Fp, c10::optional<at::Tensor> rows,
               const at::Tensor& W1, const at::Tensor& b1, int64_t B, int64_t nsplit, const at::Tensor& red) {
  constexpr int64_t H = 256;
  check_t(dZ2F, at::kBFloat16, "dZ2F");
  check_extent(dZ2F, B * H, "dZ2F");
  check_t(X, at::kBFloat16, "X");
  const int64_t nrows = check_x_rows(X, Fp, B, rows);
  check_t(W1, at::kBFloat16, "W1");
  check_extent(W1, H * Fp, "W1");
  check_t(b1, at::kFloat, "b1");
  check_extent(b1, H, "b1");
  check_t(red, at::kFloat, "red");
  check_extent(red, wf::kMlpRedFloats, "red");
  for (const at::Tensor* t : {&dZ2F, &X, &W1})
    TORCH_CHECK(reinterpret_cast<uintptr_t>(t->data_ptr()) % 16 == 0, "mlp2_dw2f: bf16 operands must be 16-B aligned");
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(dZ2F.device());
  return wf::launch_mlp2_dw2f(bfp(dZ2F), bfp(X), (int)Fp, rows_ptr(rows, B), nrows, bfp(W1), fp(b1), (int)B, (int)nsplit,
                              fp(red), cur_stream());
}

// Fused MLP forward (mlp_fused.hip): both 256-wide hidden layers + head (+ MSE) in one launch.
// Returns false (nothing launched) when the shape is not covered; the caller then runs the
// per-layer GEMMs + head kernel.
bool mlp2_forward(const at::Tensor& X, int64_t Fp, const at::Tensor& W1, const at::Tensor& b1,
                  const at::Tensor& W2, const at::Tensor& b2, const at::Tensor& w3, const at::Tensor& b3,
                  c10::optional<at::Tensor> y, c10::optional<at::Tensor> H1, const at::Tensor& H2,
                  const at::Tensor& pred, c10::optional<at::Tensor> dy, c10::optional<at::Tensor> loss_sum,
                  double dy_scale, int64_t B, c10::optional<at::Tensor> M2,
                  c10::optional<at::Tensor> dw3, c10::optional<at::Tensor> db3, c10::optional<at::Tensor> rows,
                  c10::optional<at::Tensor> red) {
  constexpr int64_t H = 256;
  check_t(X, at::kBFloat16, "X");
  const int64_t nrows = check_x_rows(X, Fp, B, rows);
  check_t(W1, at::kBFloat16, "W1");
  check_extent(W1, H * Fp, "W1");
  check_t(W2, at::kBFloat16, "W2");
  check_extent(W2, H * H, "W2");
  for (const at::Tensor* t : {&b1, &b2, &w3}) {
    check_t(*t, at::kFloat, "bias/w3");
    check_extent(*t, H, "bias/w3");
  }
  check_t(b3, at::kFloat, "b3");
  bf16_t* h1p = opt_ptr<bf16_t>(H1, at::kBFloat16, "H1", B * H);
  check_t(H2, at::kBFloat16, "H2");
  check_extent(H2, B * H, "H2");
  check_t(pred, at::kFloat, "pred");
  check_extent(pred, B, "pred");
  for (const at::Tensor* t : {&X, &W1, &W2, &H2})
    TORCH_CHECK(reinterpret_cast<uintptr_t>(t->data_ptr()) % 16 == 0, "mlp2_forward: bf16 operands must be 16-B aligned");
  const int64_t ny = nrows;  // y is indexed like X
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(X.device());
  return wf::launch_mlp2_fwd(bfp(X), (int)Fp, bfp(W1), fp(b1), bfp(W2), fp(b2), fp(w3), fp(b3),
                             opt_ptr<float>(y, at::kFloat, "y", ny), h1p, bfp(H2), mask_ptr(M2, B),
                             opt_ptr<float>(dw3, at::kFloat, "dw3", H), opt_ptr<float>(db3, at::kFloat, "db3", 1),
                             fp(pred),
                             opt_ptr<float>(dy, at::kFloat, "dy", B),
                             opt_ptr<float>(loss_sum, at::kFloat, "loss_sum", 1), (float)dy_scale, (int)B,
                             rows_ptr(rows, B), nrows, cur_stream(),
                             opt_ptr<float>(red, at::kFloat, "red", wf::kMlpRedFloats));
}

// head forward + MSE + head weight gradient in one pass over H (elementwise.hip); false = shape
// not covered (the caller runs head_fwd + head_bwd_w)
bool head_fwd_bwd(const at::Tensor& Hm, int64_t ldh, int64_t B, int64_t Hd, const at::Tensor& w, const at::Tensor& b0,
                  const at::Tensor& target, const at::Tensor& pred, const at::Tensor& dy,
                  c10::optional<at::Tensor> loss_sum, double dy_scale, const at::Tensor& dw, c10::optional<at::Tensor> db) {
  check_head_h(Hm, ldh, B, Hd);
  TORCH_CHECK(Hd % 8 == 0 && ldh % 8 == 0, "head: Hd and ldh must be multiples of 8");
  check_t(w, at::kFloat, "w");
  check_extent(w, Hd, "w");
  check_t(b0, at::kFloat, "b0");
  check_t(target, at::kFloat, "target");
  check_extent(target, B, "target");
  check_t(pred, at::kFloat, "pred");
  check_extent(pred, B, "pred");
  check_t(dy, at::kFloat, "dy");
  check_extent(dy, B, "dy");
  check_t(dw, at::kFloat, "dw");
  check_extent(dw, Hd, "dw");
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(Hm.device());
  return wf::launch_head_fwd_bwd(bfp(Hm), ldh, (int)B, (int)Hd, fp(w), fp(b0), fp(target), fp(pred), fp(dy),
                                 opt_ptr<float>(loss_sum, at::kFloat, "loss_sum", 1), (float)dy_scale, fp(dw),
                                 opt_ptr<float>(db, at::kFloat, "db", 1), cur_stream());
}

void head_bwd_w(const at::Tensor& Hm, int64_t ldh, int64_t B, int64_t Hd, const at::Tensor& dy,
                const at::Tensor& dw, c10::optional<at::Tensor> db) {
  check_head_h(Hm, ldh, B, Hd);
  check_t(dy, at::kFloat, "dy");
  check_extent(dy, B, "dy");
  check_t(dw, at::kFloat, "dw");
  check_extent(dw, Hd, "dw");
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(Hm.device());
  wf::launch_head_bwd_w(bfp(Hm), ldh, (int)B, (int)Hd, fp(dy), fp(dw),
                        opt_ptr<float>(db, at::kFloat, "db", 1), cur_stream());
}

void head_bwd_x(const at::Tensor& Hm, int64_t ldh, int64_t B, int64_t Hd, const at::Tensor& dy,
                const at::Tensor& w, bool relu_mask, const at::Tensor& dz, int64_t ldz,
                c10::optional<at::Tensor> colsum) {
  check_head_h(Hm, ldh, B, Hd);
  check_t(dy, at::kFloat, "dy");
  check_extent(dy, B, "dy");
  check_t(w, at::kFloat, "w");
  check_extent(w, Hd, "w");
  check_t(dz, at::kBFloat16, "dz");
  check_extent(dz, (B - 1) * ldz + Hd, "dz");
  TORCH_CHECK(ldz % 8 == 0, "head_bwd_x: ldz must be a multiple of 8");
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(Hm.device());
  wf::launch_head_bwd_x(bfp(Hm), ldh, (int)B, (int)Hd, fp(dy), fp(w), relu_mask ? 1 : 0, bfp(dz),
                        ldz, opt_ptr<float>(colsum, at::kFloat, "colsum", Hd), cur_stream());
}

void loss(int64_t kind, const at::Tensor& pred, const at::Tensor& y, int64_t B, int64_t O,
          double clip, double scale, c10::optional<at::Tensor> loss_sum,
          c10::optional<at::Tensor> dpred, c10::optional<at::Tensor> dpredF,
          c10::optional<at::Tensor> colsum) {
  TORCH_CHECK(kind == 0 || kind == 1, "loss: kind 0 (mse) or 1 (mae_clip)");
  check_t(pred, at::kFloat, "pred");
  check_t(y, at::kFloat, "y");
  check_extent(pred, B * O, "pred");
  check_extent(y, B * O, "y");
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(pred.device());
  wf::launch_loss((int)kind, fp(pred), fp(y), (int)B, (int)O, (float)clip, (float)scale,
                  opt_ptr<float>(loss_sum, at::kFloat, "loss_sum", 1),
                  opt_ptr<bf16_t>(dpred, at::kBFloat16, "dpred", B * O),
                  opt_ptr<float>(dpredF, at::kFloat, "dpredF", B * O),
                  opt_ptr<float>(colsum, at::kFloat, "colsum", O), cur_stream());
}

void adam(const at::Tensor& p, const at::Tensor& g, const at::Tensor& m, const at::Tensor& v,
          double lr, double b1, double b2, double eps, double wd, double bc1, double bc2,
          double gscale) {
  check_t(p, at::kFloat, "p");
  check_t(g, at::kFloat, "g");
  check_t(m, at::kFloat, "m");
  check_t(v, at::kFloat, "v");
  const int64_t n = p.numel();
  TORCH_CHECK(g.numel() == n && m.numel() == n && v.numel() == n, "adam: size mismatch");
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(p.device());
  wf::launch_adam(fp(p), fp(g), fp(m), fp(v), n, (float)lr, (float)b1, (float)b2, (float)eps,
                  (float)wd, (float)bc1, (float)bc2, (float)gscale, cur_stream());
}

void adam_dev(const at::Tensor& p, const at::Tensor& g, const at::Tensor& m, const at::Tensor& v,
              const at::Tensor& step, double lr, double b1, double b2, double eps, double wd,
              double gscale, c10::optional<at::Tensor> shadow, bool zero_g,
              c10::optional<at::Tensor> shadow_t, int64_t t_off, int64_t t_rows, int64_t t_cols,
              c10::optional<at::Tensor> clip, double clipvalue) {
  check_t(p, at::kFloat, "p");
  check_t(g, at::kFloat, "g");
  check_t(m, at::kFloat, "m");
  check_t(v, at::kFloat, "v");
  check_t(step, at::kFloat, "step");
  check_extent(step, 2, "step");  // [0] = t, [1] = completion ticket
  const int64_t n = p.numel();
  TORCH_CHECK(g.numel() == n && m.numel() == n && v.numel() == n, "adam: size mismatch");
  for (const at::Tensor* t : {&p, &g, &m, &v})
    TORCH_CHECK(reinterpret_cast<uintptr_t>(t->data_ptr()) % 16 == 0, "adam: buffers must be 16-B aligned");
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(p.device());
  // shadow_t: a transposed bf16 copy of the [t_rows][t_cols] block at element t_off (e.g. the
  // MLP's W2^T, read by mlp2_step128_kernel) written in the same launch
  bf16_t* tdst = nullptr;
  if (shadow_t.has_value()) {
    TORCH_CHECK(t_off >= 0 && t_rows > 0 && t_cols > 0 && t_off + t_rows * t_cols <= n, "adam: shadow_t block outside p");
    tdst = opt_ptr<bf16_t>(shadow_t, at::kBFloat16, "shadow_t", t_rows * t_cols);
  }
  wf::launch_adam_dev(fp(p), fp(g), fp(m), fp(v), n, fp(step), (float)lr, (float)b1, (float)b2,
                      (float)eps, (float)wd, (float)gscale, opt_ptr<bf16_t>(shadow, at::kBFloat16, "shadow", n),
                      zero_g ? 1 : 0, cur_stream(), tdst, (long)t_off, (int)t_rows, (int)t_cols, clip_state(clip),
                      (float)clipvalue);
}

void sgd(const at::Tensor& p, const at::Tensor& g, const at::Tensor& vel, double lr,
         double momentum, bool nesterov, double gscale) {
  check_t(p, at::kFloat, "p");
  check_t(g, at::kFloat, "g");
  check_t(vel, at::kFloat, "vel");
  const int64_t n = p.numel();
  TORCH_CHECK(g.numel() == n && vel.numel() == n, "sgd: size mismatch");
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(p.device());
  wf::launch_sgd(fp(p), fp(g), fp(vel), n, (float)lr, (float)momentum, nesterov ? 1 : 0,
                 (float)gscale, cur_stream());
}

void sgd_dev(const at::Tensor& p, const at::Tensor& g, const at::Tensor& vel, const at::Tensor& step, double lr,
             double decay, double momentum, bool nesterov, double gscale, bool zero_g,
             c10::optional<at::Tensor> clip, double clipvalue) {
  check_t(p, at::kFloat, "p");
  check_t(g, at::kFloat, "g");
  check_t(vel, at::kFloat, "vel");
  check_t(step, at::kFloat, "step");
  check_extent(step, 2, "step");  // [0] = iterations, [1] = completion ticket
  const int64_t n = p.numel();
  TORCH_CHECK(g.numel() == n && vel.numel() == n, "sgd: size mismatch");
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(p.device());
  wf::launch_sgd_dev(fp(p), fp(g), fp(vel), n, fp(step), (float)lr, (float)decay, (float)momentum, nesterov ? 1 : 0,
                     (float)gscale, zero_g ? 1 : 0, cur_stream(), clip_state(clip), (float)clipvalue);
}

// clipnorm: norm of gscale * g and the factor min(1, clipnorm / norm) into `state` (device only)
void grad_clip_scale(const at::Tensor& g, double gscale, double clipnorm, const at::Tensor& partial,
                     const at::Tensor& state) {
  check_t(g, at::kFloat, "g");
  check_t(partial, at::kFloat, "partial");
  check_t(state, at::kFloat, "state");
  check_extent(partial, wf::kGradClipMaxBlocks, "partial");
  check_extent(state, wf::kGradClipStateFloats, "state");
  TORCH_CHECK(g.numel() >= 1, "grad_clip_scale: empty bucket");
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(g.device());
  wf::launch_grad_clip_scale(fp(g), g.numel(), (float)gscale, (float)clipnorm, fp(partial), fp(state), cur_stream());
}

void cast_bf16(const at::Tensor& src, const at::Tensor& dst) {
  check_t(src, at::kFloat, "src");
  check_t(dst, at::kBFloat16, "dst");
  TORCH_CHECK(dst.numel() >= src.numel(), "cast: dst too small");
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(src.device());
  wf::launch_cast_bf16(fp(src), bfp(dst), src.numel(), cur_stream());
}

// out[r] = src[idx[r]] (rows of any dtype, contiguous, row size a multiple of 4 B; ids clamped)
void gather_rows(const at::Tensor& src, const at::Tensor& idx, const at::Tensor& out) {
  TORCH_CHECK(src.is_cuda() && idx.is_cuda() && out.is_cuda(), "gather_rows: GPU tensors");
  TORCH_CHECK(src.is_contiguous() && out.is_contiguous() && idx.is_contiguous(), "gather_rows: contiguous tensors");
  TORCH_CHECK(idx.scalar_type() == at::kLong && idx.dim() == 1, "gather_rows: idx int64 [m]");
  TORCH_CHECK(src.scalar_type() == out.scalar_type() && src.dim() >= 1 && out.dim() == src.dim(), "gather_rows: dtype / rank");
  TORCH_CHECK(src.size(0) > 0 && out.size(0) == idx.size(0), "gather_rows: out rows == idx size");
  const int64_t rb = src.numel() / src.size(0) * src.element_size();
  TORCH_CHECK(rb > 0 && rb % 4 == 0 && out.numel() / std::max<int64_t>(out.size(0), 1) * out.element_size() == rb,
              "gather_rows: row bytes must match and be a multiple of 4");
  if (idx.size(0) == 0) return;
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(src.device());
  wf::launch_gather_rows(src.data_ptr(), reinterpret_cast<const long long*>(idx.data_ptr<int64_t>()), out.data_ptr(), idx.size(0), (int)rb, src.size(0),
                         cur_stream());
}

void transpose_cast_bf16(const at::Tensor& src, int64_t lds, int64_t rows, int64_t cols,
                         const at::Tensor& dst, int64_t ldd) {
  TORCH_CHECK(src.is_cuda() && src.scalar_type() == at::kFloat, "src: fp32 GPU tensor");
  check_t(dst, at::kBFloat16, "dst");
  TORCH_CHECK(lds >= cols && ldd >= rows, "transpose_cast: bad leading dims");
  TORCH_CHECK(src.storage().nbytes() - src.storage_offset() * 4 >= (size_t)(((rows - 1) * lds + cols) * 4),
              "transpose_cast: src too small");
  check_extent(dst, (cols - 1) * ldd + rows, "dst");
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(src.device());
  wf::launch_transpose_cast_bf16(src.data_ptr<float>(), lds, (int)rows, (int)cols, bfp(dst), ldd,
                                 cur_stream());
}

// Feature assembly on the device (features.hip): rows [row0, row0 + N) of the source columns codes
// int32 [C][Ntot] + cont fp32 [Q][Ntot] (read in place) -> out [N][ld], bf16 (ld = round_up(F, 8),
// the MLP input format) or fp32 (ld = F, the LSTM row table). cat_off / cat_size int32 [C], mean /
// std fp32 [Q] (device); C = 0 or Q = 0: pass None. With perm_col in [0, C + Q) (categorical columns
// first; else -1 and perm None) that source column is read through `perm` (int32 [N], indices into
// all Ntot rows; the kernel clamps them): the permutation-importance pass. With const_col in
// [0, C + Q) (else -1 and const_value None; not together with perm) that source column is the
// CONSTANT const_value[0] instead, a one-element device tensor: an int32 label code for a
// categorical column, an fp32 raw value for a continuous one: the response-curve pass.
// With set_mask (int32 [ceil((C + Q) / 32)] on the table's device, the bit pattern of the mask's
// 32-bit words: bit s & 31 of word s >> 5 is source column s; perm given, perm_col and const_col
// -1) EVERY source column of the set is read through `perm`: the Shapley-attribution pass.
// With perm_values (fp32 [Ntot] on the table's device; perm and a CONTINUOUS perm_col given, no
// set, no constant) the permuted column is read from that vector instead of the table's column:
// output row r takes perm_values[clamp(perm[r])]: the set-point pass (one value per row).
constexpr int64_t kAssembleMaxF = 512;

void assemble_features(c10::optional<at::Tensor> codes, c10::optional<at::Tensor> cont,
                       c10::optional<at::Tensor> cat_off, c10::optional<at::Tensor> cat_size,
                       c10::optional<at::Tensor> mean, c10::optional<at::Tensor> stdv, int64_t row0, int64_t N,
                       int64_t F, const at::Tensor& out, int64_t perm_col, c10::optional<at::Tensor> perm,
                       int64_t const_col, c10::optional<at::Tensor> const_value,
                       c10::optional<at::Tensor> set_mask, c10::optional<at::Tensor> perm_values) {
  const bool has_c = codes.has_value() && codes->defined() && codes->numel() > 0;
  const bool has_q = cont.has_value() && cont->defined() && cont->numel() > 0;
  int64_t Ntot = -1;
  if (has_c && codes->dim() == 2) Ntot = codes->size(1);
  else if (has_q && cont->dim() == 2) Ntot = cont->size(1);
  TORCH_CHECK(Ntot >= 1, "assemble_features: no source columns");
  TORCH_CHECK(N >= 1, "assemble_features: no rows");
  TORCH_CHECK(row0 >= 0 && row0 + N <= Ntot, "assemble_features: rows ", row0, " .. ", row0 + N, " outside the ", Ntot,
              " source rows");
  TORCH_CHECK(F >= 1 && F <= kAssembleMaxF, "assemble_features: F = ", F, " outside 1 .. ", kAssembleMaxF);
  int64_t C = 0, Q = 0;
  if (has_c) {
    check_t(*codes, at::kInt, "codes");
    TORCH_CHECK(codes->dim() == 2 && codes->size(1) == Ntot, "assemble_features: codes must be [C][N]");
    C = codes->size(0);
  }
  if (has_q) {
    check_t(*cont, at::kFloat, "cont");
    TORCH_CHECK(cont->dim() == 2 && cont->size(1) == Ntot, "assemble_features: cont must be [Q][N]");
    Q = cont->size(0);
  }
  TORCH_CHECK(Q <= F && C <= F, "assemble_features: more source columns than features");
  const int* off = opt_ptr<int>(cat_off, at::kInt, "cat_off", C);
  const int* size = opt_ptr<int>(cat_size, at::kInt, "cat_size", C);
  const float* mu = opt_ptr<float>(mean, at::kFloat, "mean", Q);
  const float* sd = opt_ptr<float>(stdv, at::kFloat, "std", Q);
  TORCH_CHECK(C == 0 || (off != nullptr && size != nullptr), "assemble_features: cat_off / cat_size missing");
  TORCH_CHECK(Q == 0 || (mu != nullptr && sd != nullptr), "assemble_features: mean / std missing");
  const bool bf = out.scalar_type() == at::kBFloat16;
  check_t(out, bf ? at::kBFloat16 : at::kFloat, "out");
  TORCH_CHECK(out.dim() == 2 && out.size(0) == N, "assemble_features: out must be [N][ld]");
  const int64_t ld = out.size(1);
  TORCH_CHECK(bf ? (ld == (F + 7) / 8 * 8) : (ld == F), "assemble_features: out width ", ld, " does not fit F = ", F,
              bf ? " (bf16: round_up(F, 8))" : " (fp32: F)");
  TORCH_CHECK(wf::assemble_features_lds_bytes((int)ld, bf) <= wf::kAssembleMaxLds, "assemble_features: LDS tile too large");
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(out.device());
  const int* cp = has_c ? codes->data_ptr<int>() : nullptr;
  const float* xp = has_q ? cont->data_ptr<float>() : nullptr;
  wf::AssemblePerm pm;
  pm.ld_src = Ntot;
  const bool has_p = perm.has_value() && perm->defined();
  const bool has_s = set_mask.has_value() && set_mask->defined();
  const bool has_v = perm_values.has_value() && perm_values->defined();
  if (has_v) {
    TORCH_CHECK(!has_s, "assemble_features: perm_values is not combined with a set of permuted columns");
    TORCH_CHECK(const_col < 0 && !(const_value.has_value() && const_value->defined()),
                "assemble_features: perm_values is not combined with a constant column");
    TORCH_CHECK(has_p && perm_col >= 0, "assemble_features: perm_values goes together with perm and perm_col");
    TORCH_CHECK(perm_col >= C && perm_col < C + Q, "assemble_features: perm_values needs a continuous perm_col (",
                C, " .. ", C + Q - 1, "), got ", perm_col);
    TORCH_CHECK(perm_values->is_cuda() && perm_values->device() == out.device() &&
                    perm_values->scalar_type() == at::kFloat && perm_values->is_contiguous() && perm_values->dim() == 1,
                "assemble_features: perm_values must be a contiguous float32 vector on the table's device");
    TORCH_CHECK(perm_values->numel() == Ntot, "assemble_features: perm_values holds ", perm_values->numel(),
                " values for the table's ", Ntot, " rows");
  }
  if (has_s) {
    TORCH_CHECK(perm_col < 0, "assemble_features: a set of permuted columns or ONE perm_col, not both");
    TORCH_CHECK(const_col < 0 && !(const_value.has_value() && const_value->defined()),
                "assemble_features: a set of permuted columns is not combined with a constant column");
    TORCH_CHECK(has_p, "assemble_features: a set of permuted columns needs perm");
    TORCH_CHECK(set_mask->is_cuda() && set_mask->device() == out.device() && set_mask->scalar_type() == at::kInt &&
                    set_mask->is_contiguous() && set_mask->dim() == 1,
                "assemble_features: set_mask must be a contiguous int32 vector on the table's device");
    TORCH_CHECK(set_mask->numel() == (C + Q + 31) / 32, "assemble_features: set_mask holds ", set_mask->numel(),
                " words for ", C + Q, " source columns (need ", (C + Q + 31) / 32, ")");
    TORCH_CHECK(perm->is_cuda() && perm->device() == out.device() && perm->scalar_type() == at::kInt &&
                    perm->is_contiguous() && perm->dim() == 1,
                "assemble_features: perm must be a contiguous int32 GPU vector");
    TORCH_CHECK(perm->numel() == N, "assemble_features: perm holds ", perm->numel(), " indices for ", N, " rows");
    TORCH_CHECK(Ntot <= INT32_MAX, "assemble_features: int32 perm cannot index ", Ntot, " rows");
    pm.perm = perm->data_ptr<int>();
    pm.n = Ntot;
    pm.set_mask = reinterpret_cast<const unsigned*>(set_mask->data_ptr<int>());
    pm.codes0 = cp;
    pm.cont0 = xp;
  } else {
    TORCH_CHECK(has_p == (perm_col >= 0), "assemble_features: perm and perm_col go together");
  }
  if (has_p && !has_s) {
    TORCH_CHECK(perm_col < C + Q, "assemble_features: perm_col ", perm_col, " outside 0 .. ", C + Q - 1);
    TORCH_CHECK(perm->is_cuda() && perm->scalar_type() == at::kInt && perm->is_contiguous() && perm->dim() == 1,
                "assemble_features: perm must be a contiguous int32 GPU vector");
    TORCH_CHECK(perm->numel() == N, "assemble_features: perm holds ", perm->numel(), " indices for ", N, " rows");
    TORCH_CHECK(Ntot <= INT32_MAX, "assemble_features: int32 perm cannot index ", Ntot, " rows");
    pm.src = (int)perm_col;
    pm.perm = perm->data_ptr<int>();
    pm.base = perm_col < C ? static_cast<const void*>(cp + perm_col * Ntot)
                           : static_cast<const void*>(xp + (perm_col - C) * Ntot);
    if (has_v) pm.base = perm_values->data_ptr<float>();  // per-row values of the column, one per table row
    pm.n = Ntot;
  }
  const bool has_k = const_value.has_value() && const_value->defined();
  TORCH_CHECK(has_k == (const_col >= 0), "assemble_features: const_col and const_value go together");
  if (has_k) {
    TORCH_CHECK(!has_p, "assemble_features: one source column is permuted or constant, not both (perm and const_col)");
    TORCH_CHECK(const_col < C + Q, "assemble_features: const_col ", const_col, " outside 0 .. ", C + Q - 1);
    TORCH_CHECK(const_value->is_cuda() && const_value->device() == out.device() && const_value->is_contiguous() &&
                    const_value->numel() == 1,
                "assemble_features: const_value must be a contiguous one-element tensor on the table's device");
    const auto want = const_col < C ? at::kInt : at::kFloat;
    TORCH_CHECK(const_value->scalar_type() == want, "assemble_features: const_value must be ",
                const_col < C ? "int32 (a label code: a categorical column)" : "float32 (a raw value: a continuous column)");
    pm.src = (int)const_col;
    pm.broadcast = true;
    pm.value = const_value->data_ptr();
  }
  if (cp != nullptr) cp += row0;
  if (xp != nullptr) xp += row0;
  const bool ok = bf ? wf::launch_assemble_features_bf16(cp, xp, off, size, mu, sd, N, (int)C, (int)Q, (int)F, (int)ld,
                                                         bfp(out), cur_stream(), pm)
                     : wf::launch_assemble_features_f32(cp, xp, off, size, mu, sd, N, (int)C, (int)Q, (int)F, (int)ld,
                                                        fp(out), cur_stream(), pm);
  TORCH_CHECK(ok, "assemble_features: the launcher refused the shape");
}

// Scoring-error sums (score.hip): out[slot] = {sum d^2, sum |d|}, d = pred * y_scale + y_shift - y
// in fp64. pred / y fp32 [M] (views of larger vectors allowed), out fp64 [S][2], scratch fp64
// [kErrSumsScratch] zeroed once by the caller. Stream-ordered; nothing is read back here.
void err_sums(const at::Tensor& pred, const at::Tensor& y, double y_scale, double y_shift, const at::Tensor& out,
              int64_t slot, const at::Tensor& scratch) {
  for (const at::Tensor* t : {&pred, &y}) {
    TORCH_CHECK(t->defined() && t->is_cuda() && t->scalar_type() == at::kFloat && t->is_contiguous() && t->dim() == 1,
                "err_sums: pred / y must be contiguous fp32 GPU vectors");
  }
  TORCH_CHECK(pred.numel() >= 1 && pred.numel() == y.numel(), "err_sums: pred holds ", pred.numel(), " elements, y ",
              y.numel(), " (need the same, >= 1)");
  check_t(out, at::kDouble, "out");
  check_t(scratch, at::kDouble, "scratch");
  TORCH_CHECK(out.dim() == 2 && out.size(1) == 2, "err_sums: out must be fp64 [S][2]");
  TORCH_CHECK(slot >= 0 && slot < out.size(0), "err_sums: slot ", slot, " outside 0 .. ", out.size(0) - 1);
  check_extent(scratch, wf::kErrSumsScratch, "scratch");
  TORCH_CHECK(pred.device() == y.device() && pred.device() == out.device() && pred.device() == scratch.device(),
              "err_sums: tensors on different devices");
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(pred.device());
  wf::launch_err_sums(pred.data_ptr<float>(), y.data_ptr<float>(), pred.numel(), y_scale, y_shift,
                      out.data_ptr<double>() + 2 * slot, scratch.data_ptr<double>(), cur_stream());
}

// Per-row attribution accumulation (score.hip): one step of a sampling Shapley run. p_cur / p_prev
// fp32 [M] (not overlapping), acc / sq contiguous fp64 [K + 1][M]; row `row` of both is updated
// (start: v = p_cur * y_scale + y_shift; else d = (p_cur - p_prev) * y_scale; acc += ., sq += .^2,
// uncontracted fp64) and p_prev = p_cur. Stream-ordered; nothing is read back here.
void attr_step(const at::Tensor& p_cur, const at::Tensor& p_prev, double y_scale, double y_shift, const at::Tensor& acc,
               const at::Tensor& sq, int64_t row, bool start) {
  for (const at::Tensor* t : {&p_cur, &p_prev}) {
    TORCH_CHECK(t->defined() && t->is_cuda() && t->scalar_type() == at::kFloat && t->is_contiguous() && t->dim() == 1,
                "attr_step: p_cur / p_prev must be contiguous fp32 GPU vectors");
  }
  const int64_t M = p_cur.numel();
  TORCH_CHECK(M >= 1 && p_prev.numel() == M, "attr_step: p_cur holds ", M, " elements, p_prev ", p_prev.numel(),
              " (need the same, >= 1)");
  const char* a0 = static_cast<const char*>(p_cur.data_ptr());
  const char* b0 = static_cast<const char*>(p_prev.data_ptr());
  TORCH_CHECK(a0 + 4 * M <= b0 || b0 + 4 * M <= a0, "attr_step: p_cur and p_prev overlap");
  for (const at::Tensor* t : {&acc, &sq}) {
    TORCH_CHECK(t->defined() && t->is_cuda() && t->scalar_type() == at::kDouble && t->is_contiguous() &&
                    t->dim() == 2 && t->size(1) == M,
                "attr_step: acc / sq must be contiguous fp64 [K + 1][", M, "] GPU tensors");
    TORCH_CHECK(t->device() == p_cur.device(), "attr_step: tensors on different devices");
  }
  TORCH_CHECK(acc.size(0) == sq.size(0) && acc.data_ptr() != sq.data_ptr(), "attr_step: acc and sq must be two tables of one shape");
  TORCH_CHECK(p_prev.device() == p_cur.device(), "attr_step: tensors on different devices");
  TORCH_CHECK(row >= 0 && row < acc.size(0), "attr_step: row ", row, " outside 0 .. ", acc.size(0) - 1);
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(p_cur.device());
  wf::launch_attr_step(p_cur.data_ptr<float>(), p_prev.data_ptr<float>(), M, y_scale, y_shift,
                       acc.data_ptr<double>() + row * M, sq.data_ptr<double>() + row * M, start, cur_stream());
}

// Per-row bracket search (score.hip): one pass of a set-point run. p / want fp32 [M]; the state xs
// fp32 [4][M] (lo, hi, best_x, xq), fs fp64 [3][M] (f_lo, f_hi, best_r), status int32 [M], all
// contiguous; mode 0 first scan, 1 scan (both read the pass's value from grid_x, a one-element fp32
// device array), 2 refine (reads xq; grid_x None). p / want must not overlap the state.
// Stream-ordered; nothing is read back here.
void solve_step(const at::Tensor& p, const at::Tensor& want, double y_scale, double y_shift, int64_t mode,
                c10::optional<at::Tensor> grid_x, const at::Tensor& xs, const at::Tensor& fs, const at::Tensor& status) {
  for (const at::Tensor* t : {&p, &want}) {
    TORCH_CHECK(t->defined() && t->is_cuda() && t->scalar_type() == at::kFloat && t->is_contiguous() && t->dim() == 1,
                "solve_step: p / want must be contiguous fp32 GPU vectors");
  }
  const int64_t M = p.numel();
  TORCH_CHECK(M >= 1 && want.numel() == M, "solve_step: p holds ", M, " elements, want ", want.numel(),
              " (need the same, >= 1)");
  TORCH_CHECK(mode >= wf::kSolveFirst && mode <= wf::kSolveRefine, "solve_step: mode ", mode, " outside 0 .. 2");
  TORCH_CHECK(xs.defined() && xs.is_cuda() && xs.scalar_type() == at::kFloat && xs.is_contiguous() && xs.dim() == 2 &&
                  xs.size(0) == 4 && xs.size(1) == M,
              "solve_step: xs must be a contiguous fp32 [4][", M, "] GPU tensor");
  TORCH_CHECK(fs.defined() && fs.is_cuda() && fs.scalar_type() == at::kDouble && fs.is_contiguous() && fs.dim() == 2 &&
                  fs.size(0) == 3 && fs.size(1) == M,
              "solve_step: fs must be a contiguous fp64 [3][", M, "] GPU tensor");
  TORCH_CHECK(status.defined() && status.is_cuda() && status.scalar_type() == at::kInt && status.is_contiguous() &&
                  status.dim() == 1 && status.numel() == M,
              "solve_step: status must be a contiguous int32 [", M, "] GPU vector");
  for (const at::Tensor* t : {&want, &xs, &fs, &status}) {
    TORCH_CHECK(t->device() == p.device(), "solve_step: tensors on different devices");
  }
  const float* gx = nullptr;
  const bool has_g = grid_x.has_value() && grid_x->defined();
  if (mode != wf::kSolveRefine) {
    TORCH_CHECK(has_g && grid_x->is_cuda() && grid_x->device() == p.device() && grid_x->scalar_type() == at::kFloat &&
                    grid_x->is_contiguous() && grid_x->numel() == 1,
                "solve_step: grid_x must be one contiguous fp32 element on the predictions' device (scan modes)");
    gx = grid_x->data_ptr<float>();
  }
  // every array of the state against p and want: a thread reads p[i] / want[i] while others store
  struct Span { const char* a; int64_t n; };
  const Span state[] = {{static_cast<const char*>(xs.data_ptr()), 16 * M},
                        {static_cast<const char*>(fs.data_ptr()), 24 * M},
                        {static_cast<const char*>(status.data_ptr()), 4 * M}};
  for (const at::Tensor* t : {&p, &want}) {
    const char* a0 = static_cast<const char*>(t->data_ptr());
    for (const Span& sp : state) {
      TORCH_CHECK(a0 + 4 * M <= sp.a || sp.a + sp.n <= a0, "solve_step: p / want overlap the state");
    }
  }
  for (int i = 0; i < 3; ++i) {
    for (int j = i + 1; j < 3; ++j) {
      TORCH_CHECK(state[i].a + state[i].n <= state[j].a || state[j].a + state[j].n <= state[i].a,
                  "solve_step: the state arrays overlap each other");
    }
  }
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(p.device());
  const bool ok = wf::launch_solve_step(p.data_ptr<float>(), want.data_ptr<float>(), M, y_scale, y_shift, (int)mode, gx,
                                        xs.data_ptr<float>(), fs.data_ptr<double>(), status.data_ptr<int>(),
                                        cur_stream());
  TORCH_CHECK(ok, "solve_step: the launcher refused the shape");
}

// Grouped prediction sums (score.hip): out[slot][g] = {n_g, sum v, sum v^2}, v = pred * y_scale +
// y_shift in fp64, from the host-built plan of ops/native.py GroupPlan: order int32 [M], pieces
// int32 [2][P] (row 0 the first position of a piece in `order`, row 1 its length), group_pieces
// int32 [G + 1], scratch fp64 [>= 3 P]. out fp64 [S][G][3]. Stream-ordered; nothing is read back.
void group_sums(const at::Tensor& pred, const at::Tensor& order, const at::Tensor& pieces,
                const at::Tensor& group_pieces, double y_scale, double y_shift, const at::Tensor& out, int64_t slot,
                const at::Tensor& scratch) {
  TORCH_CHECK(pred.defined() && pred.is_cuda() && pred.scalar_type() == at::kFloat && pred.is_contiguous() &&
                  pred.dim() == 1,
              "group_sums: pred must be a contiguous fp32 GPU vector");
  const int64_t M = pred.numel();
  TORCH_CHECK(M >= 1 && M <= INT32_MAX, "group_sums: ", M, " predictions (need 1 .. 2^31 - 1)");
  for (const at::Tensor* t : {&order, &pieces, &group_pieces}) {
    TORCH_CHECK(t->defined() && t->is_cuda() && t->scalar_type() == at::kInt && t->is_contiguous(),
                "group_sums: order / pieces / group_pieces must be contiguous int32 GPU tensors");
  }
  TORCH_CHECK(order.dim() == 1 && order.numel() == M, "group_sums: the plan orders ", order.numel(), " predictions, pred holds ",
              M);
  TORCH_CHECK(pieces.dim() == 2 && pieces.size(0) == 2 && pieces.size(1) >= 1, "group_sums: pieces must be int32 [2][P]");
  const int64_t P = pieces.size(1);
  TORCH_CHECK(group_pieces.dim() == 1 && group_pieces.numel() >= 2, "group_sums: group_pieces must be int32 [G + 1]");
  const int64_t G = group_pieces.numel() - 1;
  TORCH_CHECK(G <= wf::kGroupSumsMaxGroups, "group_sums: ", G, " groups (at most ", wf::kGroupSumsMaxGroups, ")");
  TORCH_CHECK(P <= M + G, "group_sums: ", P, " pieces for ", M, " predictions in ", G, " groups");
  check_t(out, at::kDouble, "out");
  check_t(scratch, at::kDouble, "scratch");
  TORCH_CHECK(out.is_contiguous() && out.dim() == 3 && out.size(1) == G && out.size(2) == 3,
              "group_sums: out must be contiguous fp64 [S][", G, "][3]");
  TORCH_CHECK(slot >= 0 && slot < out.size(0), "group_sums: slot ", slot, " outside 0 .. ", out.size(0) - 1);
  check_extent(scratch, 3 * P, "scratch");
  for (const at::Tensor* t : {&order, &pieces, &group_pieces, &out, &scratch}) {
    TORCH_CHECK(t->device() == pred.device(), "group_sums: tensors on different devices");
  }
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(pred.device());
  const bool ok = wf::launch_group_sums(pred.data_ptr<float>(), order.data_ptr<int>(), pieces.data_ptr<int>(),
                                        pieces.data_ptr<int>() + P, group_pieces.data_ptr<int>(), M, (int)P, (int)G,
                                        y_scale, y_shift, out.data_ptr<double>() + slot * G * 3,
                                        scratch.data_ptr<double>(), cur_stream());
  TORCH_CHECK(ok, "group_sums: the launcher refused the shape");
}

// Conformal scores (quantile.hip): out[i] = (float)|d|, or (float)(|d| / |v|) with `relative`, for
// v = pred * y_scale + y_shift and d = v - y in fp64. pred / y / out contiguous fp32 [M] (views of
// larger vectors allowed); out does not overlap pred / y. Stream-ordered; nothing is read back here.
void abs_scores(const at::Tensor& pred, const at::Tensor& y, double y_scale, double y_shift, bool relative,
                const at::Tensor& out) {
  for (const at::Tensor* t : {&pred, &y, &out}) {
    TORCH_CHECK(t->defined() && t->is_cuda() && t->scalar_type() == at::kFloat && t->is_contiguous() && t->dim() == 1,
                "abs_scores: pred / y / out must be contiguous fp32 GPU vectors");
    TORCH_CHECK(t->device() == pred.device(), "abs_scores: tensors on different devices");
  }
  const int64_t M = pred.numel();
  TORCH_CHECK(M >= 1 && y.numel() == M && out.numel() == M, "abs_scores: pred holds ", M, " elements, y ", y.numel(),
              ", out ", out.numel(), " (need the same, >= 1)");
  const char* o0 = static_cast<const char*>(out.data_ptr());
  for (const at::Tensor* t : {&pred, &y}) {
    const char* a0 = static_cast<const char*>(t->data_ptr());
    TORCH_CHECK(a0 + 4 * M <= o0 || o0 + 4 * M <= a0, "abs_scores: out overlaps pred / y");
  }
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(pred.device());
  const bool ok = wf::launch_abs_scores(pred.data_ptr<float>(), y.data_ptr<float>(), M, y_scale, y_shift, relative,
                                        out.data_ptr<float>(), cur_stream());
  TORCH_CHECK(ok, "abs_scores: the launcher refused the shape");
}

// Exact per-group order statistics (quantile.hip): out[g][a] = the ranks[g][a]-th smallest score of
// group g, from the host-built plan of ops/native.py QuantilePlan: order int32 [M], pieces int32
// [2][P], piece_group int32 [P], hist int32 [G][A][256] (zero; left zero), state int32 [G][A][2].
// ranks int32 [G][A], out fp32 [G][A]. Stream-ordered; nothing is read back here.
void group_quantiles(const at::Tensor& scores, const at::Tensor& order, const at::Tensor& pieces,
                     const at::Tensor& piece_group, const at::Tensor& ranks, const at::Tensor& hist,
                     const at::Tensor& state, const at::Tensor& out) {
  TORCH_CHECK(scores.defined() && scores.is_cuda() && scores.scalar_type() == at::kFloat && scores.is_contiguous() &&
                  scores.dim() == 1,
              "group_quantiles: scores must be a contiguous fp32 GPU vector");
  const int64_t M = scores.numel();
  TORCH_CHECK(M >= 1 && M <= INT32_MAX, "group_quantiles: ", M, " scores (need 1 .. 2^31 - 1)");
  for (const at::Tensor* t : {&order, &pieces, &piece_group, &ranks, &hist, &state}) {
    TORCH_CHECK(t->defined() && t->is_cuda() && t->scalar_type() == at::kInt && t->is_contiguous(),
                "group_quantiles: order / pieces / piece_group / ranks / hist / state must be contiguous int32 GPU tensors");
  }
  TORCH_CHECK(order.dim() == 1 && order.numel() == M, "group_quantiles: the plan orders ", order.numel(),
              " scores, scores holds ", M);
  TORCH_CHECK(pieces.dim() == 2 && pieces.size(0) == 2 && pieces.size(1) >= 1, "group_quantiles: pieces must be int32 [2][P]");
  const int64_t P = pieces.size(1);
  TORCH_CHECK(piece_group.dim() == 1 && piece_group.numel() == P, "group_quantiles: piece_group must be int32 [", P, "]");
  TORCH_CHECK(ranks.dim() == 2 && ranks.size(0) >= 1 && ranks.size(1) >= 1, "group_quantiles: ranks must be int32 [G][A]");
  const int64_t G = ranks.size(0), A = ranks.size(1);
  TORCH_CHECK(A <= wf::kQuantMaxLevels, "group_quantiles: ", A, " levels (at most ", wf::kQuantMaxLevels, ")");
  TORCH_CHECK(G * A <= wf::kQuantMaxCells, "group_quantiles: ", G, " groups x ", A, " levels (at most ",
              wf::kQuantMaxCells, " cells)");
  TORCH_CHECK(P <= M + G, "group_quantiles: ", P, " pieces for ", M, " scores in ", G, " groups");
  TORCH_CHECK(hist.dim() == 3 && hist.size(0) == G && hist.size(1) == A && hist.size(2) == 256,
              "group_quantiles: hist must be int32 [", G, "][", A, "][256]");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(hist.data_ptr()) % 16 == 0, "group_quantiles: hist must be 16-byte aligned");
  TORCH_CHECK(state.dim() == 3 && state.size(0) == G && state.size(1) == A && state.size(2) == 2,
              "group_quantiles: state must be int32 [", G, "][", A, "][2]");
  TORCH_CHECK(out.defined() && out.is_cuda() && out.scalar_type() == at::kFloat && out.is_contiguous() &&
                  out.dim() == 2 && out.size(0) == G && out.size(1) == A,
              "group_quantiles: out must be a contiguous fp32 [", G, "][", A, "] GPU tensor");
  for (const at::Tensor* t : {&order, &pieces, &piece_group, &ranks, &hist, &state, &out}) {
    TORCH_CHECK(t->device() == scores.device(), "group_quantiles: tensors on different devices");
  }
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(scores.device());
  const bool ok = wf::launch_group_quantiles(scores.data_ptr<float>(), order.data_ptr<int>(), pieces.data_ptr<int>(),
                                             pieces.data_ptr<int>() + P, piece_group.data_ptr<int>(), M, (int)P, (int)G,
                                             (int)A, ranks.data_ptr<int>(), hist.data_ptr<int>(), state.data_ptr<int>(),
                                             out.data_ptr<float>(), cur_stream());
  TORCH_CHECK(ok, "group_quantiles: the launcher refused the shape");
}

void im2col1d(const at::Tensor& x, int64_t B, int64_t L, int64_t Cin, int64_t ksz, int64_t Kp,
              const at::Tensor& col) {
  check_t(x, at::kFloat, "x");
  check_t(col, at::kBFloat16, "col");
  const int64_t Lout = L - ksz + 1;
  TORCH_CHECK(Lout > 0 && Kp >= ksz * Cin + 1, "im2col1d: bad shape");
  check_extent(x, B * L * Cin, "x");
  check_extent(col, B * Lout * Kp, "col");
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(x.device());
  wf::launch_im2col1d(fp(x), (int)B, (int)L, (int)Cin, (int)ksz, (int)Lout, (int)Kp, bfp(col),
                      cur_stream());
}

// ---- fused reference CNN (cnn_fused.hip). dims = [L, C, taps, T, Fp, Kc, O] (models/cnn.py
// CnnLayout; the dense weight has 16 rows, Op = 16).
wf::CnnDims cnn_dims(const std::vector<int64_t>& dims, double drop_p) {
  TORCH_CHECK(dims.size() == 7, "cnn: dims = [L, C, taps, T, Fp, Kc, O]");
  wf::CnnDims d;
  d.L = (int)dims[0]; d.C = (int)dims[1]; d.taps = (int)dims[2]; d.T = (int)dims[3];
  d.Fp = (int)dims[4]; d.Kc = (int)dims[5]; d.O = (int)dims[6];
  d.drop_p = (float)drop_p;
  return d;
}

bool cnn_fused_ok(const std::vector<int64_t>& dims, double drop_p) {
  return wf::cnn_fused_supported(cnn_dims(dims, drop_p));
}

std::vector<int64_t> cnn_part_sizes(int64_t B, const std::vector<int64_t>& dims) {
  auto d = cnn_dims(dims, 0.0);
  long wd = 0, wc = 0, f = 0;
  wf::cnn_part_floats((int)B, d, &wd, &wc, &f);
  return {wd, wc, f};
}

static wf::CnnDims cnn_checked(const std::vector<int64_t>& dims, double drop_p) {
  auto d = cnn_dims(dims, drop_p);
  TORCH_CHECK(wf::cnn_fused_supported(d), "cnn: shape not covered by the fused kernels");
  return d;
}

static int64_t cnn_frag_elems(const wf::CnnDims& d) { return (int64_t)d.T * (d.Fp / 16) * 64 * 4; }

int64_t cnn_small_scratch_floats() { return wf::kCnnSmallScratch; }

// K small-batch CNN training steps (forward, backward, Keras SGD) in ONE persistent launch
// (cnn_small.hip). X [N][48] / Y [N][O] fp32 through rows [K * B] (or contiguous); params / vel
// / step: flat parameters and FlatSGD state; rng: the engine's dropout step counter. False =
// not covered.
bool cnn_small_steps(const at::Tensor& X, const at::Tensor& Y, c10::optional<at::Tensor> rows, int64_t B, int64_t K,
                     std::vector<int64_t> dims, double drop_p, int64_t loss_kind, double clip, double scale,
                     int64_t seed, const at::Tensor& rng, const at::Tensor& params, const at::Tensor& vel,
                     const at::Tensor& step, double lr, double decay, double momentum, bool nesterov, double gscale,
                     c10::optional<at::Tensor> loss_acc, const at::Tensor& scr, const at::Tensor& sync,
                     int64_t filters, c10::optional<at::Tensor> stamps) {
  const wf::CnnDims d = cnn_checked(dims, drop_p);
  TORCH_CHECK(d.L == 48 && d.C == 1 && d.Fp == 112 && d.Kc == 16 && d.T == 36, "cnn_small_steps: the reference layout only");
  TORCH_CHECK(K > 0 && B > 0 && B <= 64, "cnn_small_steps: 0 < B <= 64, K > 0");
  check_t(X, at::kFloat, "X");
  check_t(Y, at::kFloat, "Y");
  int64_t nrows;
  const long long* rp = nullptr;
  if (rows.has_value() && rows->defined()) {
    rp = rows_ptr(rows, K * B);
    nrows = X.numel() / d.L;
    TORCH_CHECK(nrows > 0, "X: empty dataset");
  } else {
    nrows = K * B;
    check_extent(X, nrows * d.L, "X");
  }
  check_extent(Y, nrows * d.O, "Y");
  const int64_t n = (int64_t)d.Fp * d.Kc + 16LL * d.T * d.Fp + 16;
  for (const at::Tensor* t : {&params, &vel}) {
    check_t(*t, at::kFloat, "params/vel");
    check_extent(*t, n, "params/vel");
  }
  check_t(step, at::kFloat, "step");
  TORCH_CHECK(rng.is_cuda() && rng.scalar_type() == at::kLong && rng.numel() >= 1, "rng: int64 GPU counter");
  check_t(scr, at::kFloat, "scr");
  check_extent(scr, wf::kCnnSmallScratch, "scr");
  check_t(sync, at::kInt, "sync");
  check_extent(sync, 4, "sync");
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(X.device());
  wf::CnnSmallArgs a{};
  a.X = fp(X);
  a.Y = fp(Y);
  a.rows = rp;
  a.nrows = (long)nrows;
  a.B = (int)B;
  a.K = (int)K;
  a.O = d.O;
  a.taps = d.taps;
  a.filters = (int)filters;
  a.drop = drop_p > 0.0 ? 1 : 0;
  a.loss_kind = (int)loss_kind;
  a.keep_scale = drop_p > 0.0 ? (float)(1.0 / (1.0 - drop_p)) : 1.f;
  a.clip = (float)clip;
  a.scale = (float)scale;
  a.seed = (unsigned)seed;
  a.rng = reinterpret_cast<long long*>(rng.data_ptr<int64_t>());
  a.p = fp(params);
  a.vel = fp(vel);
  a.step = fp(step);
  a.lr = (float)lr;
  a.decay = (float)decay;
  a.momentum = (float)momentum;
  a.gscale = (float)gscale;
  a.nesterov = nesterov ? 1 : 0;
  a.loss_acc = opt_ptr<float>(loss_acc, at::kFloat, "loss_acc", 1);
  a.scr = fp(scr);
  a.sync = reinterpret_cast<unsigned*>(sync.data_ptr<int>());
  const char* sl = std::getenv("WELLFLOW_SPIN_LIMIT");  // tests: force the hand-off timeout path
  a.spin_limit = sl != nullptr ? (unsigned)std::strtoul(sl, nullptr, 10) : (1u << 22);
  a.stamps = reinterpret_cast<unsigned long long*>(opt_ptr<int64_t>(stamps, at::kLong, "stamps", 28 * 64 * 16));
  return wf::launch_cnn_small(a, cur_stream());
}

void cnn_pack(const at::Tensor& Wc, const at::Tensor& Wd, const std::vector<int64_t>& dims, const at::Tensor& WcA,
              const at::Tensor& WdF, const at::Tensor& WdB) {
  auto d = cnn_checked(dims, 0.0);
  check_t(Wc, at::kFloat, "Wc");
  check_extent(Wc, (int64_t)d.Fp * d.Kc, "Wc");
  TORCH_CHECK(Wd.is_cuda() && Wd.scalar_type() == at::kFloat && Wd.is_contiguous(), "Wd: contiguous fp32 GPU tensor");
  check_extent(Wd, (int64_t)16 * d.T * d.Fp, "Wd");
  check_t(WcA, at::kBFloat16, "WcA");
  check_extent(WcA, (int64_t)d.Fp * d.Kc, "WcA");
  for (const at::Tensor* t : {&WdF, &WdB}) {
    check_t(*t, at::kBFloat16, "WdF/WdB");
    check_extent(*t, cnn_frag_elems(d), "WdF/WdB");
  }
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(Wc.device());
  wf::launch_cnn_pack(fp(Wc), Wd.data_ptr<float>(), d, bfp(WcA), bfp(WdF), bfp(WdB), cur_stream());
}

// Keras SGD on the CNN's flat parameters + the bf16 operand images (cnn_pack's output) in one launch
void cnn_sgd_pack(const at::Tensor& p, const at::Tensor& g, const at::Tensor& vel, const at::Tensor& step, double lr,
                  double decay, double momentum, bool nesterov, double gscale, bool zero_g,
                  const std::vector<int64_t>& dims, const at::Tensor& WcA, const at::Tensor& WdF, const at::Tensor& WdB,
                  c10::optional<at::Tensor> clip, double clipvalue) {
  auto d = cnn_checked(dims, 0.0);
  for (const at::Tensor* t : {&p, &g, &vel}) check_t(*t, at::kFloat, "p/g/vel");
  const int64_t n = p.numel();
  TORCH_CHECK(g.numel() == n && vel.numel() == n, "cnn_sgd_pack: size mismatch");
  TORCH_CHECK(n >= (int64_t)d.Fp * d.Kc + (int64_t)16 * d.T * d.Fp, "cnn_sgd_pack: p shorter than the CNN layout");
  check_t(step, at::kFloat, "step");
  check_extent(step, 2, "step");
  check_t(WcA, at::kBFloat16, "WcA");
  check_extent(WcA, (int64_t)d.Fp * d.Kc, "WcA");
  for (const at::Tensor* t : {&WdF, &WdB}) {
    check_t(*t, at::kBFloat16, "WdF/WdB");
    check_extent(*t, cnn_frag_elems(d), "WdF/WdB");
  }
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(p.device());
  wf::launch_cnn_sgd_pack(fp(p), fp(g), fp(vel), n, fp(step), (float)lr, (float)decay, (float)momentum, nesterov ? 1 : 0,
                          (float)gscale, zero_g ? 1 : 0, d, bfp(WcA), bfp(WdF), bfp(WdB), cur_stream(), clip_state(clip),
                          (float)clipvalue);
}

static const long long* rng_ptr(const c10::optional<at::Tensor>& rng) {
  if (!rng.has_value() || !rng->defined()) return nullptr;
  TORCH_CHECK(rng->is_cuda() && rng->scalar_type() == at::kLong && rng->numel() >= 1, "rng: GPU int64 tensor");
  return reinterpret_cast<const long long*>(rng->data_ptr<int64_t>());
}

void cnn_forward(const at::Tensor& x, int64_t B, const std::vector<int64_t>& dims, double drop_p, const at::Tensor& WcA,
                 const at::Tensor& WdF, const at::Tensor& bd, c10::optional<at::Tensor> y, c10::optional<at::Tensor> dout,
                 c10::optional<at::Tensor> pred, c10::optional<at::Tensor> part, bool train, int64_t loss_kind,
                 double clip, double scale, int64_t seed, c10::optional<at::Tensor> rng) {
  auto d = cnn_checked(dims, drop_p);
  TORCH_CHECK(B > 0, "cnn_forward: B > 0");
  const int64_t rows = (B + 15) / 16 * 16;
  check_t(x, at::kFloat, "x");
  check_extent(x, B * d.L, "x");
  check_t(WcA, at::kBFloat16, "WcA");
  check_extent(WcA, (int64_t)d.Fp * d.Kc, "WcA");
  check_t(WdF, at::kBFloat16, "WdF");
  check_extent(WdF, cnn_frag_elems(d), "WdF");
  TORCH_CHECK(bd.is_cuda() && bd.scalar_type() == at::kFloat && bd.numel() >= 16, "bd: 16 fp32 values");
  long wd = 0, wc = 0, f = 0;
  wf::cnn_part_floats((int)B, d, &wd, &wc, &f);
  float *yp = nullptr, *dp = nullptr, *pp = nullptr, *part_p = nullptr;
  if (train) {
    TORCH_CHECK(loss_kind == 0 || loss_kind == 1, "cnn_forward: loss 0 (mse) or 1 (mae_clip)");
    yp = opt_ptr<float>(y, at::kFloat, "y", B * d.O);
    dp = opt_ptr<float>(dout, at::kFloat, "dout", rows * 16);
    part_p = opt_ptr<float>(part, at::kFloat, "part", f);
    TORCH_CHECK(yp && dp && part_p, "cnn_forward(train): y, dout and part are required");
  } else {
    pp = opt_ptr<float>(pred, at::kFloat, "pred", rows * 16);
    TORCH_CHECK(pp, "cnn_forward(eval): pred is required");
  }
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(x.device());
  wf::launch_cnn_forward(fp(x), (int)B, d, bfp(WcA), bfp(WdF), bd.data_ptr<float>(), yp, dp, pp, part_p, train ? 1 : 0,
                         (int)loss_kind, (float)clip, (float)scale, (unsigned)(seed & 0xFFFFFFFF), rng_ptr(rng),
                         cur_stream());
}

void cnn_backward(const at::Tensor& x, int64_t B, const std::vector<int64_t>& dims, double drop_p, const at::Tensor& WcA,
                  const at::Tensor& WdB, const at::Tensor& dout, int64_t seed, c10::optional<at::Tensor> rng,
                  const at::Tensor& part_wd, const at::Tensor& part_wc) {
  auto d = cnn_checked(dims, drop_p);
  TORCH_CHECK(B > 0, "cnn_backward: B > 0");
  const int64_t rows = (B + 15) / 16 * 16;
  check_t(x, at::kFloat, "x");
  check_extent(x, B * d.L, "x");
  check_t(WcA, at::kBFloat16, "WcA");
  check_extent(WcA, (int64_t)d.Fp * d.Kc, "WcA");
  check_t(WdB, at::kBFloat16, "WdB");
  check_extent(WdB, cnn_frag_elems(d), "WdB");
  check_t(dout, at::kFloat, "dout");
  check_extent(dout, rows * 16, "dout");
  long wd = 0, wc = 0, f = 0;
  wf::cnn_part_floats((int)B, d, &wd, &wc, &f);
  check_t(part_wd, at::kFloat, "part_wd");
  check_extent(part_wd, wd, "part_wd");
  check_t(part_wc, at::kFloat, "part_wc");
  check_extent(part_wc, wc, "part_wc");
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(x.device());
  wf::launch_cnn_backward(fp(x), (int)B, d, bfp(WcA), bfp(WdB), fp(dout), (unsigned)(seed & 0xFFFFFFFF), rng_ptr(rng),
                          fp(part_wd), fp(part_wc), cur_stream());
}

void cnn_reduce(const at::Tensor& part_wd, const at::Tensor& part_wc, const at::Tensor& part_f, int64_t B,
                const std::vector<int64_t>& dims, const at::Tensor& gWc, const at::Tensor& gWd, const at::Tensor& gbd,
                c10::optional<at::Tensor> loss_sum, c10::optional<at::Tensor> rng) {
  auto d = cnn_checked(dims, 0.0);
  long wd = 0, wc = 0, f = 0;
  wf::cnn_part_floats((int)B, d, &wd, &wc, &f);
  check_t(part_wd, at::kFloat, "part_wd");
  check_extent(part_wd, wd, "part_wd");
  check_t(part_wc, at::kFloat, "part_wc");
  check_extent(part_wc, wc, "part_wc");
  check_t(part_f, at::kFloat, "part_f");
  check_extent(part_f, f, "part_f");
  for (const at::Tensor* t : {&gWc, &gWd, &gbd})
    TORCH_CHECK(t->is_cuda() && t->scalar_type() == at::kFloat && t->is_contiguous(), "grads: contiguous fp32 GPU");
  check_extent(gWc, (int64_t)d.Fp * d.Kc, "gWc");
  check_extent(gWd, (int64_t)16 * d.T * d.Fp, "gWd");
  check_extent(gbd, 16, "gbd");
  long long* rp = nullptr;
  if (rng.has_value() && rng->defined()) {
    TORCH_CHECK(rng->is_cuda() && rng->scalar_type() == at::kLong && rng->numel() >= 1, "rng: GPU int64 tensor");
    rp = reinterpret_cast<long long*>(rng->data_ptr<int64_t>());
  }
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(part_wd.device());
  wf::launch_cnn_reduce(fp(part_wd), fp(part_wc), fp(part_f), (int)B, d, gWc.data_ptr<float>(), gWd.data_ptr<float>(),
                        gbd.data_ptr<float>(), opt_ptr<float>(loss_sum, at::kFloat, "loss_sum", 1), rp, cur_stream());
}

// True when the HIP objects are a WF_DIAG build (WELLFLOW_DIAG_BUILD=1): timing-only switches
// and A/B variants are live. bench.py refuses to time such a build.
bool diag_build() { return wf::dbg_mask() != (1 << 21); }

// Every binding runs behind this wrapper: a kernel launch that the runtime rejected (bad grid,
// missing code object, invalid resource) raises here instead of failing silently.
template <auto F>
struct Checked;
template <class R, class... A, R (*F)(A...)>
struct Checked<F> {
  static R call(A... a) {
    (void)hipGetLastError();  // errors of earlier, foreign launches are not ours to report
    if constexpr (std::is_void_v<R>) {
      F(a...);
      check();
    } else {
      R r = F(a...);
      check();
      return r;
    }
  }
  static void check() {
    const hipError_t e = hipGetLastError();
    TORCH_CHECK(e == hipSuccess, "wellflow kernel launch failed: ", hipGetErrorString(e));
  }
};

}  // namespace

#define WF_DEF(name) m.def(#name, &Checked<&name>::call)

PYBIND11_MODULE(_C, m) {
  m.doc() = "wellflow HIP kernel library (gfx950)";
  WF_DEF(gemm);
  WF_DEF(mlp2_forward);
  WF_DEF(mlp2_backward);
  WF_DEF(mlp2_dw2);
  WF_DEF(mlp2_reduce);
  WF_DEF(mlp2_step);
  WF_DEF(mlp2_dw2f);
  WF_DEF(mlp_small_steps);
  WF_DEF(mlp_small_scratch_floats);
  WF_DEF(cnn_small_steps);
  WF_DEF(cnn_small_scratch_floats);
  WF_DEF(lstm_pack_x);
  WF_DEF(lstm_pack_x_win);
  WF_DEF(lstm_forward);
  WF_DEF(lstm_forward_persistent);
  WF_DEF(lstm_backward);
  WF_DEF(lstm_backward_dw);
  WF_DEF(lstm_pack_weights);
  WF_DEF(lstm_adam_pack);
  WF_DEF(head_fwd);
  WF_DEF(head_bwd_w);
  WF_DEF(head_fwd_bwd);
  WF_DEF(head_bwd_x);
  WF_DEF(loss);
  WF_DEF(adam);
  WF_DEF(adam_dev);
  WF_DEF(sgd);
  WF_DEF(sgd_dev);
  WF_DEF(grad_clip_scale);
  WF_DEF(cast_bf16);
  WF_DEF(gather_rows);
  WF_DEF(transpose_cast_bf16);
  WF_DEF(im2col1d);
  // const_col / const_value / set_mask / perm_values are optional (and keywords): the twelve-argument call is the
  // launch it was
  m.def("assemble_features", &Checked<&assemble_features>::call, py::arg("codes"), py::arg("cont"), py::arg("cat_off"),
        py::arg("cat_size"), py::arg("mean"), py::arg("std"), py::arg("row0"), py::arg("N"), py::arg("F"), py::arg("out"),
        py::arg("perm_col"), py::arg("perm"), py::arg("const_col") = -1, py::arg("const_value") = py::none(),
        py::arg("set_mask") = py::none(), py::arg("perm_values") = py::none());
  WF_DEF(err_sums);
  WF_DEF(group_sums);
  WF_DEF(attr_step);
  WF_DEF(solve_step);
  WF_DEF(abs_scores);
  WF_DEF(group_quantiles);
  // host-only queries (no launch; callable without a GPU)
  m.def("diag_build", &diag_build);
  m.def("gemm_plan", &gemm_plan);
  m.def("cnn_fused_ok", &cnn_fused_ok);
  m.def("cnn_part_sizes", &cnn_part_sizes);
  WF_DEF(cnn_pack);
  WF_DEF(cnn_sgd_pack);
  WF_DEF(cnn_forward);
  WF_DEF(cnn_backward);
  WF_DEF(cnn_reduce);
}
