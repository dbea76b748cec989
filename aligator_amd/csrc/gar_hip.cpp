// gar_hip.cpp -- C-ABI implementation (include/gar_hip.h) over the HIP kernels.
// Host C++ only packs per-stage blocks into the contiguous device records,
// launches kernels on a HIP stream and copies results back; all arithmetic of
// the Riccati path runs in the kernels (gar_generic.hpp, gar_mfma.hpp).  The unit's host code is split over headers
// included in place: gar_host.hpp (what a solver is made of), gar_select.hpp (kernel families), gar_launch.hpp (the sweeps'
// launches), gar_resident.hpp (the services on a resident batch), gar_multi.hpp, gar_entry_io.hpp; the extern "C" entry
// points are here.
#include "../../include/gar_hip.h"

#include <hip/hip_runtime.h>

#include <dlfcn.h>

#include <algorithm>
#include <atomic>
#include <cfloat>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "gar_generic.hpp"
#include "gar_layout.h"
#include "gar_mfma.hpp"
#include "gar_forward_lean.hpp"
#include "gar_wave.hpp"
#include "gar_wave_leg.hpp"
#include "gar_wave_pair.hpp"
#include "gar_cyclic.hpp"
#include "gar_condensed_cr.hpp"
#include "gar_dense.hpp"
#include "gar_fold.hpp"
#include "gar_cstr_seg_api.hpp"
#include "gar_leg_seg.hpp"
#include "gar_kkt.hpp"
#include "gar_affine.hpp"
#include "gar_refine.hpp"
#include "gar_adjoint.hpp"
#include "gar_affine_multi.hpp"
#include "gar_host.hpp"
#include "gar_record_io.hpp"

namespace gar { // instantiated in gar_wave_sweep.cpp (its own translation unit, its own code-generation flags)
#define GAR_SWEEP_EXTERN(NX, NU)                                                                                        \
  extern template __global__ void gar_backward_wave<NX, NU, 0>(MfmaParams, int);                                       \
  extern template __global__ void gar_backward_wave_half<NX, NU>(MfmaParams, int);
GAR_SWEEP_SHAPES(GAR_SWEEP_EXTERN)
  extern template __global__ void gar_backward_wave<56, 24, 0>(MfmaParams, int); // gar_wave_wide.cpp
#undef GAR_SWEEP_EXTERN
} // namespace gar

namespace {

thread_local std::string g_last_error;

int fail(int code, const std::string &msg) {
  g_last_error = msg;
  return code;
}

#define HIP_TRY(expr)                                                                    \
  do {                                                                                   \
    hipError_t e_ = (expr);                                                              \
    if (e_ != hipSuccess)                                                                \
      return fail(GAR_HIP_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_)); \
  } while (0)

inline int align2(int x) { return (x + 1) & ~1; }

// Tracing hooks (the reference brackets the same places with Tracy zones: backwardImpl
// riccati-kernel.hxx:108, "factor_initial" proximal-riccati.hxx:43, forwardImpl riccati-kernel.hxx:320,
// "parallel_backward" / "parallel_forward" parallel-solver.hxx:134,213, assembleCondensedSystem :87):
// roctx ranges around the launches, visible in rocprofv3 --marker-trace.  Opt-in (GAR_HIP_ROCTX=1) and
// resolved at run time, so the library carries no link dependency on the tracer.
struct Roctx {
  int (*push)(const char *) = nullptr;
  int (*pop)() = nullptr;
  Roctx() {
    const char *e = std::getenv("GAR_HIP_ROCTX"); // (read once, when the first range opens: environment only)
    if (!e || e[0] != '1')
      return;
    if (void *h = dlopen("libroctx64.so", RTLD_NOW | RTLD_GLOBAL)) {
      push = (int (*)(const char *))dlsym(h, "roctxRangePushA");
      pop = (int (*)())dlsym(h, "roctxRangePop");
      if (!push || !pop)
        push = nullptr, pop = nullptr;
    }
  }
};
inline const Roctx &roctx() {
  static const Roctx r;
  return r;
}
struct RoctxRange {
  explicit RoctxRange(const char *name) {
    if (roctx().push)
      roctx().push(name);
  }
  ~RoctxRange() {
    if (roctx().pop)
      roctx().pop();
  }
};

// Every entry point runs on the solver's own device, whatever the caller's current device is, and
// leaves the caller's current device as it found it (two solvers on two GPUs in one process;
// torch's notion of the current device).
void pipe_autojoin(const gar_hip_solver *s);
struct DeviceGuard {
  int prev = -1, dev;
  explicit DeviceGuard(int device) : dev(device) { // device < 0 (null solver): no-op
    if (dev < 0)
      return;
    if (hipGetDevice(&prev) != hipSuccess)
      prev = -1;
    if (prev != dev)
      (void)hipSetDevice(dev);
  }
  ~DeviceGuard() {
    if (dev >= 0 && prev >= 0 && prev != dev)
      (void)hipSetDevice(prev);
  }
  DeviceGuard(const DeviceGuard &) = delete;
  DeviceGuard &operator=(const DeviceGuard &) = delete;
};
// (every entry point but the two that feed the pipelined sweep first orders the caller's stream behind the half
// streams: pipe_join, below)
#define GAR_GUARD_NOJOIN(s) DeviceGuard guard_((s) ? (s)->device : -1)
#define GAR_GUARD(s)                                                                                                   \
  GAR_GUARD_NOJOIN(s);                                                                                                 \
  pipe_autojoin(s)
// one process, several devices (gar_multi.hpp): the handle owns one ranked solver per device and serves every
// entry point by routing to them
#define GAR_MULTI(s, expr)                                                                                             \
  do {                                                                                                                 \
    if ((s) && (s)->multi)                                                                                             \
      return (expr);                                                                                                   \
  } while (0)

} // namespace

struct gar_multi;

struct gar_hip_solver : gar::HostLayout, gar::KernelBinding {
  // gar_hip_multi_create: this object holds the layout only (no device memory); `multi` owns the per-device solvers
  gar_multi *multi = nullptr;
  int device = 0, batch = 0;
  int leg_begin = 0, leg_end = 1;
  int world = 1, rank = 0; // horizon sharding: this solver owns legs [rank J / W, (rank + 1) J / W)
  // Padding onto a specialised kernel family happens HERE, behind the C ABI (riccati-base.hpp:13-37 is what
  // binds: the caller passes the knots' own dimensions).  A uniform, unconstrained, unparameterised problem whose
  // (nx, nu) has no kernel of its own runs on the smallest specialised shape (NX >= nx, NU >= nu) with DUMMY
  // controls (R = I, S = 0, B = 0, r = 0) and DUMMY states (Q = I, A = 0, f = 0, pinned to zero by extra rows
  // [0 -I] x0 = 0 of the initial constraint): both solve to exactly zero, decouple from the real variables, and
  // are stripped from every result.  user_* = what the caller passed; `ulay` = the layout of the caller-facing
  // records (packed problem, solution, gains) when they differ from the device's (caller_layout).
  std::vector<int32_t> user_dims5;
  int user_nc0 = 0;
  bool padded = false;
  int unx = 0, unu = 0, pnx = 0, pnu = 0; // caller's / device (nx, nu) of the uniform stages
  std::unique_ptr<gar::HostLayout> ulay;
  // `flay` = the layout of the folded problem (KernelBinding::fold: same knots, nc = 0) or of the segment legs'
  // scratch records (seg_bwd_kernel: same knots, serial); d_prob2 / d_fac2 / d_meta2 its device records
  std::unique_ptr<gar::HostLayout> flay;
  bool mu_divides = false; // some knot's solve divides by mueq outright (see gar_hip_backward_legs_async)
  bool any_nc = false;     // some knot carries constraints: a non-finite mueq is refused (ibid.)
  // leg mode
  int nxb = 0;
  int64_t tuple_doubles = 0, cscratch_doubles = 0;
  int legs_per_rank = 0;
  double cond_threshold = 1e-10; // parallel-solver.hpp:92
  double cond_backward_ok = GAR_CONDENSED_BACKWARD_OK; // gar_hip_set_condensed_backward_ok
  bool cond_reduced = false; // generic condensed solve: leg states eliminated leg-parallel first (GAR_HIP_CONDENSED_REDUCED=0: off)
  bool cond_cr = false;      // ... and the J remaining blocks by block cyclic reduction, a workgroup per block and level
                             // (gar_condensed_cr.hpp; GAR_HIP_CONDENSED_CR=0: the one-workgroup chain, =<k>: from k legs on)
  int max_refinement = 5;        // parallel-solver.hpp:94
  // run state (gar_host.hpp): what dies with the layout -- the buffers and what they hold right now -- and what is created
  // on first use and dies with the solver
  gar::LayoutState buf;
  gar::Current cur;
  gar::PipeState pipe;
  gar::LazyState lazy;
  Stream own_stream;            // created with the solver; `stream` is it or the caller's (gar_hip_set_stream)
  hipStream_t stream = nullptr;
  gar::LdsPlan lds{};
  gar::DensePlan dense_lds{};
  std::string lds_error;   // the generic kernels do not fit a CU's LDS (fatal unless a specialised family serves the shape)
  bool timing = false;         // gar_hip_set_timing (LazyState::ev)
  int pipe_halves = 0;         // the pipelined sweep (PipeState), 0: off
  int pipe_requested = 0;      // what the caller last asked gar_hip_set_pipeline for (a rebuild re-validates it)
  // SolverProxDDP builds the terminal knot with nx2 = 0 (solvers/proxddp/workspace.hxx:54-55); nothing of the
  // algorithm reads a terminal knot's A, f (riccati-kernel.hxx:130-193).  Such a knot is taken in as nx2 = nx -- the
  // uniform record every kernel family addresses -- with zeros for the two blocks; the gains of that knot go back
  // with the caller's row count (normalise_terminal, gar_hip_upload_stage, gar_hip_get_gains)
  bool term_grown = false;
  std::vector<double> term_zeros;
};

namespace {

// The status buffer (d_status, ints) has three regions:
//   [0, batch)                      status_words: a word per problem, 0 = the last sweep succeeded
//   [batch, batch + 4)              status_counters: MfmaParams::slow -- slow-path stages (2), constrained stages (2)
//   [batch + 4, 2 batch + 4)        status_flags: a word per problem -- MfmaParams::resume; folded solvers: "flagged, D != 0"
constexpr int kStatusCounters = 4;
inline int *status_words(const gar_hip_solver *s, int b0 = 0) { return s->buf.d_status + b0; }
inline int *status_counters(const gar_hip_solver *s) { return s->buf.d_status + s->batch; }
inline int *status_flags(const gar_hip_solver *s) { return s->buf.d_status + s->batch + kStatusCounters; }
inline size_t status_bytes(size_t b, bool flags) { return sizeof(int) * (b + kStatusCounters + (flags ? b : 0)); }

// ---- layout ---------------------------------------------------------------
int build_layout(gar::HostLayout &s) {
  const int N = s.horizon;
  s.meta.assign(N + 1, gar_stage_meta{});
  std::vector<int> leg_of(N + 1, 0), nth_eff(N + 1, 0), flags(N + 1, 0);
  for (int t = 0; t <= N; ++t) {
    const int32_t *d = &s.dims5[5 * t];
    if (d[0] < 0 || d[1] < 0 || d[2] < 0 || d[3] < 0 || d[4] < 0 || d[0] == 0)
      return fail(GAR_HIP_ERR_ARG, "negative or zero state dimension");
    nth_eff[t] = d[4];
    flags[t] = d[4] > 0 ? GAR_KNOT_HAS_PARAM : 0;
  }
  if (s.num_legs > 1) {
    // ParallelRiccatiSolver::initialize (parallel-solver.hxx:51-82)
    for (int i = 0; i < s.num_legs; ++i) {
      int i0, i1;
      gar_get_work(N, i, s.num_legs, &i0, &i1);
      if (i1 <= i0)
        return fail(GAR_HIP_ERR_ARG, "more legs than stages");
      const bool last_leg = (i == s.num_legs - 1);
      const int nth = s.dims5[5 * (i1 - 1) + 3]; // nx2 of the leg's last knot
      for (int t = i0; t < i1; ++t) {
        if (s.dims5[5 * t + 4] != 0)
          return fail(GAR_HIP_ERR_UNSUPPORTED,
                      "leg mode on a user-parameterised problem is not supported");
        leg_of[t] = i;
        nth_eff[t] = last_leg ? 0 : nth;
        flags[t] = last_leg ? 0 : (t == i1 - 1 ? GAR_KNOT_LEG_END : GAR_KNOT_LEG_PARAM);
      }
    }
  }
  s.nx0 = s.dims5[0];
  s.nth0 = nth_eff[0];
  s.n0 = s.nx0 + s.nc0;
  int64_t in = 0, fo = 0;
  s.G0_off = in;
  in += (int64_t)s.nc0 * s.nx0;
  s.g0_off = in;
  in += s.nc0;
  in = (in + 1) & ~(int64_t)1;
  int64_t x = 0, u = 0, v = 0, l = s.nc0;
  for (int t = 0; t <= N; ++t) {
    const int32_t *d = &s.dims5[5 * t];
    gar_stage_meta &m = s.meta[t];
    m.nx = d[0]; m.nu = d[1]; m.nc = d[2]; m.nx2 = d[3];
    m.nth = nth_eff[t];
    m.flags = flags[t];
    m.leg = leg_of[t];
    m.in_off = in;
    in += gar_knot_doubles(d[0], d[1], d[2], d[3], (flags[t] & GAR_KNOT_HAS_PARAM) ? d[4] : 0);
    in = (in + 1) & ~(int64_t)1; // keep records 16-byte aligned
    m.fac_off = fo;
    fo += gar_factor_doubles(d[0], d[1], d[2], s.dense ? 2 * d[3] : d[3], nth_eff[t]);
    fo = (fo + 1) & ~(int64_t)1;
    m.x_off = (int32_t)x; x += d[0];
    m.u_off = (int32_t)u; u += d[1];
    m.v_off = (int32_t)v; v += d[2];
    m.l_off = (int32_t)(t == 0 ? 0 : l);
    if (t > 0)
      l += s.dims5[5 * (t - 1) + 3];
  }
  // lbdas[t] (t>=1) has nx2 of stage t-1: recompute l offsets cleanly
  {
    int64_t lo = s.nc0;
    s.meta[0].l_off = 0;
    for (int t = 1; t <= N; ++t) {
      s.meta[t].l_off = (int32_t)lo;
      lo += s.dims5[5 * (t - 1) + 3];
    }
    l = lo;
  }
  s.prob_doubles = in;
  s.fac_doubles = fo;
  s.sol_x = 0;
  s.sol_u = x;
  s.sol_v = x + u;
  s.sol_l = x + u + v;
  for (int t = 0; t <= N; ++t) {
    s.meta[t].u_off += (int32_t)s.sol_u;
    s.meta[t].v_off += (int32_t)s.sol_v;
    s.meta[t].l_off += (int32_t)s.sol_l;
  }
  s.sol_doubles = (x + u + v + l + 1) & ~(int64_t)1;
  { // derivative buffer: header G0 | g0 | init Hxx, then one record per stage (even offsets)
    long long p = 0;
    s.d_G0 = p; p += (long long)s.nc0 * s.nx0;
    s.d_g0 = p; p += s.nc0;
    s.d_iH = p; p += (long long)s.nx0 * s.nx0;
    p = (p + 1) & ~1ll;
    s.deriv_off.assign(N + 1, 0);
    for (int t = 0; t <= N; ++t) {
      const int32_t *d = &s.dims5[5 * t];
      s.deriv_off[t] = p;
      p += gar_deriv_layout(d[0], d[1], d[2], d[3]).total;
      p = (p + 1) & ~1ll;
    }
    s.deriv_doubles = p;
  }
  {
    long long pf = 0, pb = 0;
    s.gain_off.assign(2 * (size_t)(N + 1), 0);
    for (int t = 0; t <= N; ++t) {
      const int32_t *d = &s.dims5[5 * t];
      const long long nr = (long long)d[1] + d[2] + (s.dense ? 2 * d[3] : d[3]);
      s.gain_off[2 * t] = pf;
      s.gain_off[2 * t + 1] = pb;
      pf += nr;
      pb += nr * d[0];
    }
    s.ff_all_doubles = pf;
    s.fb_all_doubles = pb;
  }
  s.init_doubles = ((int64_t)s.n0 + (int64_t)s.n0 * s.nth0 + s.nth0 + (int64_t)s.nth0 * s.nth0 + 1) & ~(int64_t)1;
  s.ring0 = 0;
  s.uni_in0 = s.meta[0].in_off;
  s.uni_in_rec = N > 1 ? s.meta[1].in_off - s.meta[0].in_off : s.meta[N].in_off - s.meta[0].in_off;
  s.uni_fac_rec = N > 1 ? s.meta[1].fac_off - s.meta[0].fac_off : s.meta[N].fac_off;
  return GAR_HIP_OK;
}

// the layout of the caller-facing records: the solver's own unless it is padded
inline const gar::HostLayout &caller_layout(const gar_hip_solver *s) {
  return s->ulay ? *s->ulay : static_cast<const gar::HostLayout &>(*s);
}

int plan_lds(gar_hip_solver *s) {
  int nxM = 0, nuM = 0, ncM = 0, nthM = 0, nwM = 0, nkM = 0;
  for (const auto &m : s->meta) {
    nxM = std::max(nxM, std::max(m.nx, m.nx2));
    nuM = std::max(nuM, m.nu);
    ncM = std::max(ncM, m.nc);
    nthM = std::max(nthM, m.nth);
    nwM = std::max(nwM, m.nx + m.nu);
    nkM = std::max(nkM, m.nu + m.nc);
  }
  gar::LdsPlan &L = s->lds;
  int p = 0;
  auto take = [&](int n) { int o = p; p += align2(std::max(n, 0)); return o; };
  L.lean = 0;
replan:
  p = 0;
  for (int k = 0; k < 2; ++k) {
    // Vxx', vx' are dead once P = V'[A B] and vplus are formed (S1), Vxx, vx are written in S5: one
    // buffer serves both (25 KB at nx = 56, what lets the Talos shape fit a CU's LDS); the
    // parameter blocks are read and written in the same phase and keep two
    L.V[k] = k == 0 ? take(nxM * nxM) : L.V[0];
    L.v[k] = k == 0 ? take(nxM) : L.v[0];
    L.Vxt[k] = (k == 1 && L.lean) ? L.Vxt[0] : take(nxM * nthM);
    L.Vtt[k] = (k == 1 && L.lean) ? L.Vtt[0] : take(nthM * nthM);
    L.vt[k] = (k == 1 && L.lean) ? L.vt[0] : take(nthM);
  }
  const int stage_begin = p;
  L.H = take(nwM * nwM);
  L.h = take(nwM);
  L.F = take(nxM * nwM);
  L.fv = take(nxM);
  L.P = take(std::max(nxM * nwM, nxM * nxM));
  L.vp = take(nxM);
  L.CD = take(ncM * nwM);
  L.dd = take(ncM);
  L.Gu = take(nuM * nthM);
  L.Guh = take(nuM * nthM);
  L.Gv = take(ncM * nthM);
  L.M = take(nkM * nkM);
  L.msub = take(nkM);
  L.piv = take(264); // 512 pivots + 8 control ints
  L.G = take(nkM * (1 + nxM + nthM));
  L.Yth = take(nxM * nthM);
  L.yff = take(nxM);
  const int stage_end = p;
  // initial-stage KKT aliases the per-stage buffers
  p = stage_begin;
  const int n0 = s->n0, nth0 = s->nth0;
  L.k0mat = take(n0 * n0);
  L.k0rhs = take(n0 * (1 + nth0));
  L.k0sub = take(n0);
  L.k0piv = take(264);
  L.total = std::max(stage_end, p);
  // panel workspace of the blocked Bunch-Kaufman, behind everything -- where there is room for it
  L.bkw = -1;
  if (nkM <= 128 && (size_t)(L.total + align2(nkM * GAR_BK_PANEL)) * sizeof(double) <= 160 * 1024) {
    L.bkw = L.total;
    L.total += align2(nkM * GAR_BK_PANEL);
  }
  if (!L.lean && nthM > 0 && (size_t)L.total * sizeof(double) > 160 * 1024) {
    L.lean = 1; // one generation of the parameter blocks in LDS, the other read back from the records
    goto replan;
  }
  // forward kernel
  p = 0;
  L.fx = take(nxM);
  L.fxn = take(nxM);
  L.fth = take(nthM);
  L.ftotal = p;
  if (s->dense) {
    int nM = 0, rldM = 0;
    for (const auto &m : s->meta) {
      nM = std::max(nM, m.nu + m.nc + 2 * m.nx2);
      rldM = std::max(rldM, 1 + m.nx + m.nth);
    }
    gar::DensePlan &D = s->dense_lds;
    p = 0;
    D.K = take(nM * (nM + 1) / 2); // packed lower triangle
    D.R = take(nM * rldM);
    D.sub = take(nM);
    D.piv = take(264);
    D.wk = -1;
    if (nM <= 128 && (int64_t)(p + nM * GAR_BK_PANEL) * 8 <= 160 * 1024)
      D.wk = take(nM * GAR_BK_PANEL);
    const int stage_total = p;
    p = 0; // the initial stage reuses the buffer from its start (gar_backward_dense)
    take(n0 * n0);
    take(n0 * (1 + nth0));
    take(n0);
    take(264);
    D.total = std::max(stage_total, p);
    if (n0 > 512 || nM > 512)
      return fail(GAR_HIP_ERR_UNSUPPORTED, "KKT dimension above 512");
    if ((int64_t)D.total * 8 > 160 * 1024)
      return fail(GAR_HIP_ERR_UNSUPPORTED,
                  "stage-dense solver: stage dimensions need " + std::to_string((int64_t)D.total * 8) +
                      " B of LDS (> 160 KiB per CU)");
    return GAR_HIP_OK;
  }
  if (n0 > 512 || nkM > 512)
    return fail(GAR_HIP_ERR_UNSUPPORTED, "KKT dimension above 512");
  s->lds_error.clear();
  if ((int64_t)L.total * 8 > 160 * 1024) // fatal only if no specialised family serves the shape (allocate)
    s->lds_error = "stage dimensions need " + std::to_string((int64_t)L.total * 8) +
                   " B of LDS (> 160 KiB per CU)";
  return GAR_HIP_OK;
}

#include "gar_select.hpp"

gar::GenericParams make_params(gar_hip_solver *s, double mueq) {
  gar::GenericParams P{};
  P.meta = s->buf.d_meta;
  P.prob = s->buf.d_prob;
  P.fac = s->buf.d_fac;
  P.sol = s->buf.d_sol;
  P.init = s->buf.d_init;
  P.status = s->buf.d_status;
  P.boundary = s->buf.d_bound_local;
  P.csol = s->buf.d_csol;
  P.theta = nullptr;
  P.prob_stride = s->prob_doubles;
  P.fac_stride = s->fac_doubles;
  P.sol_stride = s->sol_doubles;
  P.init_stride = s->init_doubles;
  P.boundary_stride = (long long)s->legs_per_rank * s->tuple_doubles;
  P.G0_off = s->G0_off;
  P.g0_off = s->g0_off;
  P.horizon = s->horizon;
  P.nc0 = s->nc0;
  P.nx0 = s->nx0;
  P.nth0 = s->nth0;
  P.num_legs = s->num_legs;
  P.leg_begin = s->leg_begin;
  P.local_legs = s->leg_end - s->leg_begin;
  P.tuple_doubles = (int)s->tuple_doubles;
  P.nxb = s->nxb;
  P.mueq = mueq;
  P.lds = s->lds;
  P.dense = s->dense_lds;
  P.init_closed = s->init_closed ? 1 : 0;
  P.vxx_packed = s->vxx_packed ? 1 : 0;
  return P;
}

void mark_dirty(gar_hip_solver *s, int b, int64_t lo, int64_t hi) {
  auto &iv = s->buf.dirty_iv[(size_t)b];
  // the common pattern is "append right after the last range" (knot after knot): O(1); gaps of
  // one double are record-alignment padding and merge as well
  if (!iv.empty() && lo >= iv.back().first && lo <= iv.back().second + 1) {
    iv.back().second = std::max(iv.back().second, hi);
  } else {
    iv.emplace_back(lo, hi);
    if (iv.size() > 1 && iv[iv.size() - 2].first > lo) { // out of order: sort and merge
      std::sort(iv.begin(), iv.end());
      size_t w = 0;
      for (size_t r = 1; r < iv.size(); ++r) {
        if (iv[r].first <= iv[w].second + 1)
          iv[w].second = std::max(iv[w].second, iv[r].second);
        else
          iv[++w] = iv[r];
      }
      iv.resize(w + 1);
    }
  }
  s->buf.dirty = true;
}

int commit(gar_hip_solver *s) {
  if (!(s->buf.staged && s->buf.dirty))
    return GAR_HIP_OK;
  stage_fence();
  const int64_t P = s->prob_doubles;
  // whole problems, back to back: one copy per run of fully rewritten problems
  int b = 0;
  while (b < s->batch) {
    auto &iv = s->buf.dirty_iv[(size_t)b];
    if (iv.empty()) {
      ++b;
      continue;
    }
    const bool whole = iv.size() == 1 && iv[0].first == 0 && iv[0].second >= P - 1;
    if (whole) {
      int e = b + 1;
      while (e < s->batch && s->buf.dirty_iv[(size_t)e].size() == 1 && s->buf.dirty_iv[(size_t)e][0].first == 0 &&
             s->buf.dirty_iv[(size_t)e][0].second >= P - 1)
        ++e;
      HIP_TRY(hipMemcpyAsync(s->buf.d_prob + (int64_t)b * P, s->buf.h_prob + (int64_t)b * P,
                             sizeof(double) * (size_t)P * (size_t)(e - b), hipMemcpyHostToDevice,
                             s->stream));
      for (int k = b; k < e; ++k)
        s->buf.dirty_iv[(size_t)k].clear();
      b = e;
      continue;
    }
    for (const auto &r : iv) {
      const int64_t hi = std::min(r.second, P);
      HIP_TRY(hipMemcpyAsync(s->buf.d_prob + (int64_t)b * P + r.first, s->buf.h_prob + (int64_t)b * P + r.first,
                             sizeof(double) * (size_t)(hi - r.first), hipMemcpyHostToDevice,
                             s->stream));
    }
    iv.clear();
    ++b;
  }
  s->buf.dirty = false;
  return GAR_HIP_OK;
}

// pipeline the upload: once the range being appended to has grown past 1 MiB it goes out
// (asynchronously, pinned -> HBM) while the caller packs the next knots -- one Newton
// iteration's 7.6 MB of knots then costs max(host packing, PCIe), not their sum
int flush_if_grown(gar_hip_solver *s, int b) {
  auto &iv = s->buf.dirty_iv[(size_t)b];
  if (!iv.empty() && iv.back().second - iv.back().first >= (int64_t)(1 << 17)) {
    stage_fence();
    const int64_t lo = iv.back().first, hi = std::min(iv.back().second, s->prob_doubles);
    HIP_TRY(hipMemcpyAsync(s->buf.d_prob + (int64_t)b * s->prob_doubles + lo,
                           s->buf.h_prob + (int64_t)b * s->prob_doubles + lo,
                           sizeof(double) * (size_t)(hi - lo), hipMemcpyHostToDevice, s->stream));
    iv.pop_back();
  }
  return GAR_HIP_OK;
}

// The n blocks `maps` (gar_record_io.hpp) of problem b, taken from `src`, into the `doubles` of its record that start at
// `base`.  Staged: straight into the pinned record, which then is ONE dirty range -- the holes that packed triangles
// leave inside their blocks included: block-by-block ranges would not merge, and a problem would go out as two small
// copies per knot instead of 1 MiB pieces.  Unstaged (a staging area beyond 1 GiB): the same put_block into per-thread
// scratch, then block by block to the device.
int write_blocks(gar_hip_solver *s, int b, int64_t base, int64_t doubles, const BlockMap *maps, const double *const *src,
                 int n) {
  if (doubles <= 0)
    return GAR_HIP_OK;
  thread_local std::vector<double> scratch;
  if (!s->buf.staged)
    scratch.resize((size_t)doubles);
  double *rec = s->buf.staged ? s->buf.h_prob + (int64_t)b * s->prob_doubles + base : scratch.data();
  for (int i = 0; i < n; ++i)
    put_block(rec, maps[i], src[i], s->buf.staged && s->buf.stage_nt);
  if (s->buf.staged) {
    mark_dirty(s, b, base, base + doubles);
    return flush_if_grown(s, b);
  }
  double *dev = s->buf.d_prob + (int64_t)b * s->prob_doubles + base;
  for (int i = 0; i < n; ++i)
    if (maps[i].doubles() > 0)
      HIP_TRY(hipMemcpyAsync(dev + maps[i].off, rec + maps[i].off, sizeof(double) * (size_t)maps[i].doubles(),
                             hipMemcpyHostToDevice, s->stream));
  return GAR_HIP_OK;
}

// the condensed solve's info slots (residual, steps, scale, resolved) in a problem's scratch: behind its blocks
inline int64_t cond_info_off(const gar_hip_solver *s) { return 4 * (int64_t)(2 * s->num_legs) * ((int64_t)s->nxb * s->nxb + s->nxb); }

// MfmaParams, what every fill shares: the knot records of layout `in` (the solver's own or the folded one), the factor
// records, the status words and counters, the horizon.  mueq and spd_accept belong to the stage sweeps (gar_launch.hpp:
// make_mfma_scratch_params); the wave-leg family's embedded block leaves them at zero.
gar::MfmaParams mfma_common(gar_hip_solver *s, const gar::HostLayout &in, const double *prob, double *fac, long long fac_stride) {
  gar::MfmaParams M{};
  M.prob = prob;
  M.fac = fac;
  M.status = status_words(s);
  M.slow = status_counters(s);
  M.prob_stride = in.prob_doubles;
  M.fac_stride = fac_stride;
  M.in_off0 = in.uni_in0;
  M.in_rec = in.uni_in_rec;
  M.in_offN = in.meta[in.horizon].in_off;
  M.horizon = in.horizon;
  return M;
}

gar::LegParams make_leg_params(gar_hip_solver *s) {
  gar::LegParams Q{};
  // folded solvers: the wave-leg family sweeps the folded knots and keeps its own (nc = 0) factor records; problems
  // with D != 0 are skipped (the generic leg kernels or the constrained segment legs take them)
  Q.M = s->fold ? mfma_common(s, *s->flay, s->buf.d_prob2, s->buf.d_fac2, s->flay->fac_doubles)
                : mfma_common(s, *s, s->buf.d_prob, s->buf.d_fac, s->fac_doubles);
  Q.M.trace = s->buf.d_trace;
  Q.meta = s->fold ? s->buf.d_meta2 : s->buf.d_meta;
  Q.skip = s->fold ? status_flags(s) : nullptr;
  Q.num_legs = s->num_legs;
  Q.leg_begin = s->leg_begin;
  Q.csol = s->buf.d_csol;
  Q.sol = s->buf.d_sol;
  Q.sol_stride = s->sol_doubles;
  Q.sol_u = (int)s->sol_u;
  Q.sol_l = (int)s->sol_l;
  Q.nc0 = s->nc0;
  Q.boundary = s->buf.d_bound_local;
  Q.boundary_stride = (long long)s->legs_per_rank * s->tuple_doubles;
  Q.tuple_doubles = (int)s->tuple_doubles;
  Q.cinfo = s->buf.d_cscratch ? s->buf.d_cscratch + cond_info_off(s) : nullptr;
  Q.cinfo_stride = s->cscratch_doubles;
  return Q;
}

// gar_fold_constraints stages C and C / mu in LDS where they fit the default dynamic allocation (0: they do not)
size_t fold_lds_bytes(const gar_hip_solver *s) {
  int nxm = 0, ncm = 0;
  for (const auto &m : s->meta)
    nxm = std::max(nxm, (int)m.nx), ncm = std::max(ncm, (int)m.nc);
  const size_t b = sizeof(double) * (size_t)gar::fold_lds_doubles(nxm, ncm);
  return b <= 48 * 1024 ? b : 0;
}
gar::FoldParams make_fold_params(gar_hip_solver *s) {
  gar::FoldParams F{};
  const gar::HostLayout &f = *s->flay;
  F.meta = s->buf.d_meta;
  F.meta2 = s->buf.d_meta2;
  F.prob = s->buf.d_prob;
  F.prob2 = s->buf.d_prob2;
  F.fac = s->buf.d_fac;
  F.fac2 = s->buf.d_fac2;
  F.sol = s->buf.d_sol;
  F.prob_stride = s->prob_doubles;
  F.prob2_stride = f.prob_doubles;
  F.fac_stride = s->fac_doubles;
  F.fac2_stride = f.fac_doubles;
  F.sol_stride = s->sol_doubles;
  F.coupled = status_flags(s);
  F.horizon = s->horizon;
  F.t2 = s->fb_t2 ? 1 : 0;
  int lo, hi, dummy;
  gar_get_work(s->horizon, s->leg_begin, s->num_legs, &lo, &dummy);
  gar_get_work(s->horizon, s->leg_end - 1, s->num_legs, &dummy, &hi);
  F.t_lo = lo;
  F.t_hi = hi;
  F.mueq = s->cur.mueq;
  F.qr_packed = s->qr_packed ? 1 : 0;
  F.lds = fold_lds_bytes(s) > 0 ? 1 : 0;
  return F;
}
// the serial twin's kernels (gar_fold_serial, gar_expand_serial): the bound family's own record formats on top
gar::SerialFoldParams make_serial_fold_params(gar_hip_solver *s) {
  gar::SerialFoldParams S{};
  S.F = make_fold_params(s);
  S.out_qr_packed = s->sf_qr_packed ? 1 : 0;
  S.src_t2 = s->sf_fb_t2 ? 1 : 0;
  S.src_vxx_packed = s->sf_vxx_packed ? 1 : 0;
  S.header = (int)std::min(s->uni_in0, s->flay->uni_in0);
  return S;
}

// Folded solvers (gar_hip_solver::fold): the caller-visible factor records are formed on first request after a
// backward (nobody who only reads the solution pays for them), and which problems the generic kernels took
// (D != 0: row-major fb in their records instead of fbT2) is read back once.
int ensure_expanded(gar_hip_solver *s) {
  if (!s->fold)
    return GAR_HIP_OK;
  if (!s->cur.expanded) {
    const dim3 grid((unsigned)(s->horizon + 1), (unsigned)s->batch);
    if (s->serial_fold)
      hipLaunchKernelGGL(gar::gar_expand_serial, grid, dim3(256), 0, s->stream, make_serial_fold_params(s));
    else
      hipLaunchKernelGGL(gar::gar_expand_constrained, grid, dim3(256), 0, s->stream, make_fold_params(s));
    HIP_TRY(hipGetLastError());
    s->cur.records_expanded();
  }
  if (!s->cur.know_coupled) {
    s->buf.h_coupled.assign((size_t)s->batch, 0);
    HIP_TRY(hipMemcpyAsync(s->buf.h_coupled.data(), status_flags(s), sizeof(int) * (size_t)s->batch,
                           hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    s->cur.coupled_read();
  }
  return GAR_HIP_OK;
}
// fb / fth of problem b in the fbT2 device order?
inline bool records_t2(const gar_hip_solver *s, int b) {
  return s->fb_t2 && !(s->fold && s->cur.coupled(s->buf.h_coupled, b));
}

// a kernel's opt-in to `doubles` of dynamic LDS (> 64 KiB needs it)
template <class K> hipError_t max_lds(K kernel, size_t doubles) {
  return hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(doubles * sizeof(double)));
}

// (defined beside prefetch_impl, which starts the read-back)
enum { kBehindStream = 1, kBehindHost = 2 };
int settle_gains_readback(gar_hip_solver *s, int behind);

#include "gar_launch.hpp"
#include "gar_resident.hpp"

int allocate(gar_hip_solver *s) {
  const size_t B = (size_t)s->batch;
  HIP_TRY(s->buf.d_meta.alloc(s->meta.size()));
  HIP_TRY(hipMemcpy(s->buf.d_meta, s->meta.data(), sizeof(gar_stage_meta) * s->meta.size(),
                    hipMemcpyHostToDevice));
  HIP_TRY(s->buf.d_prob.zalloc((size_t)s->prob_doubles * B));
  HIP_TRY(s->buf.d_fac.zalloc((size_t)s->fac_doubles * B));
  HIP_TRY(s->buf.d_sol.zalloc((size_t)s->sol_doubles * B));
  HIP_TRY(s->buf.d_init.zalloc((size_t)s->init_doubles * B));
  HIP_TRY(s->buf.d_theta.alloc((size_t)std::max(s->nth0, 1) * B));
  HIP_TRY(s->buf.d_status.zalloc(status_bytes(B, true) / sizeof(int))); // (the three regions: status_words)
  if (s->num_legs > 1) {
    const int chunk = s->legs_per_rank; // >= this rank's own leg count; equal-sized chunks for the all-gather
    const int nblk = 2 * s->num_legs;
    const size_t bs = (size_t)s->nxb * s->nxb;
    HIP_TRY(s->buf.d_bound_local.zalloc((size_t)s->tuple_doubles * chunk * B));
    if (s->world > 1) // (one rank: the local buffer is the gathered one, LayoutState::bound_all)
      HIP_TRY(s->buf.d_bound_gathered.alloc((size_t)s->tuple_doubles * chunk * s->world * B));
    HIP_TRY(s->buf.d_csol.alloc((size_t)nblk * s->nxb * B));
    s->cscratch_doubles = cond_info_off(s) + 4;
    // (the info slots behind the blocks -- residual, steps, scale, resolved -- are read by the gar_hip_condensed_*
    // getters: defined before the first solve)
    HIP_TRY(s->buf.d_cscratch.zalloc((size_t)s->cscratch_doubles * B));
    s->cond_lds_doubles = (int)(3 * bs + 4 * s->nxb + 2 + (s->nxb + 16) / 2 + 2 + (s->nxb < 9 ? 9 * s->nxb : 0));
    {
      s->cond_reduced = !option_off("GAR_HIP_CONDENSED_REDUCED") && s->nx0 == s->nxb &&
                        (size_t)gar::gar_condensed_leg_lds_doubles(s->nxb) * sizeof(double) <= 160 * 1024;
      // cyclic reduction of the reduced system: log2 J dependent steps instead of J; below 4 legs the chain is as short
      const char *cc = gar_option("GAR_HIP_CONDENSED_CR");
      const int cr_min = cc && cc[0] ? std::atoi(cc) : 4;
      s->cond_cr = s->cond_reduced && cr_min >= 1 && s->num_legs >= std::max(cr_min, 2) && s->nc0 <= s->nxb &&
                   (size_t)gar::gar_condensed_cr_back_lds_doubles(s->nxb, s->num_legs) * sizeof(double) <= 160 * 1024;
    }
  }
  if (s->seg_bwd_kernel) {
    const gar::HostLayout &f = *s->flay;
    HIP_TRY(s->buf.d_fac2.zalloc((size_t)f.fac_doubles * B));
    HIP_TRY(s->buf.d_meta2.alloc(f.meta.size()));
    HIP_TRY(hipMemcpy(s->buf.d_meta2, f.meta.data(), sizeof(gar_stage_meta) * f.meta.size(), hipMemcpyHostToDevice));
    HIP_TRY(max_lds(s->seg_bwd_kernel, s->seg_lds_doubles));
    HIP_TRY(max_lds(gar::gar_leg_param_chain, gar::leg_chain_lds_doubles(s->dims5[0])));
    HIP_TRY(max_lds(gar::gar_leg_param_stage, gar::leg_stage_lds_doubles(s->dims5[0], s->dims5[1])));
  }
  if (s->fold) {
    const gar::HostLayout &f = *s->flay;
    HIP_TRY(s->buf.d_prob2.zalloc((size_t)f.prob_doubles * B));
    HIP_TRY(s->buf.d_fac2.zalloc((size_t)f.fac_doubles * B));
    HIP_TRY(s->buf.d_meta2.alloc(f.meta.size()));
    HIP_TRY(hipMemcpy(s->buf.d_meta2, f.meta.data(), sizeof(gar_stage_meta) * f.meta.size(), hipMemcpyHostToDevice));
    if (s->cseg_on) {
      const size_t units = B * (size_t)s->legs_per_rank;
      HIP_TRY(s->buf.d_cseg_resume.alloc(units));
      HIP_TRY(hipMemset(s->buf.d_cseg_resume, 0xff, sizeof(int) * units));
      for (auto k : s->cseg.backward)
        HIP_TRY(max_lds(k, s->cseg.backward_lds_doubles));
      HIP_TRY(max_lds(s->cseg.leg_end, s->cseg.leg_end_lds_doubles));
      HIP_TRY(max_lds(s->cseg.chain, s->cseg.chain_lds_doubles));
      HIP_TRY(max_lds(s->cseg.stage, s->cseg.stage_lds_doubles));
    }
  }
  const size_t staging = sizeof(double) * (size_t)s->prob_doubles * B;
  if (staging <= ((size_t)1 << 30)) {
    HIP_TRY(s->buf.h_prob.alloc((size_t)s->prob_doubles * B, hipHostMallocDefault));
    std::memset(s->buf.h_prob, 0, staging);
    s->buf.staged = true;
    const char *nt = gar_option("GAR_HIP_STAGE_NT");
    s->buf.stage_nt = nt && nt[0] ? nt[0] == '1' : sizeof(double) * (size_t)s->prob_doubles >= ((size_t)12 << 20);
  }
  s->buf.dirty_iv.assign(B, {});
  s->buf.dirty = false;
  if (s->dense) {
    HIP_TRY(max_lds(gar::gar_backward_dense, s->dense_lds.total));
    return GAR_HIP_OK;
  }
  if (s->mfma_kernel)
    HIP_TRY(max_lds(s->mfma_kernel, s->mfma_lds_doubles));
  if (s->cyc_setup_kernel) {
    HIP_TRY(max_lds(s->cyc_setup_kernel, s->cyc_lds_doubles + s->cyc_block_doubles));
    HIP_TRY(max_lds(s->cyc_reduce_kernel, 2 * s->cyc_lds_doubles + 64 + s->cyc_block_doubles)); // (launch_condensed)
    HIP_TRY(max_lds(s->cyc_top_kernel, s->cyc_lds_doubles));
  }
  if (s->cond_wave_kernel)
    HIP_TRY(max_lds(s->cond_wave_kernel, s->cond_wave_lds_doubles));
  if (s->leg_bwd_kernel)
    HIP_TRY(max_lds(s->leg_bwd_kernel, s->leg_lds_doubles));
  if (s->wave_kernel)
    HIP_TRY(max_lds(s->wave_kernel, s->wave_lds_doubles * s->waves_per_block));
  for (auto k : {s->wave_coupled_kernel, s->wave_bk_kernel})
    if (k)
      HIP_TRY(max_lds(k, s->wave_lds_doubles * s->waves_per_block));
  if (s->lds_error.empty())
    HIP_TRY(max_lds(gar::gar_initial_generic, s->lds.total));
  if (s->n0 <= 128)
    HIP_TRY(max_lds(gar::gar_initial_wave, gar::gar_initial_wave_lds_doubles(s->n0, s->nth0)));
  // > 64 KiB of dynamic LDS needs the opt-in attribute
  if (s->lds_error.empty())
    HIP_TRY(max_lds(gar::gar_backward_generic, s->lds.total));
  if (s->num_legs > 1)
    HIP_TRY(max_lds(gar::gar_condensed_generic, s->cond_lds_doubles));
  if (s->num_legs > 1 && s->cond_reduced)
    HIP_TRY(max_lds(gar::gar_condensed_leg_eliminate, gar::gar_condensed_leg_lds_doubles(s->nxb)));
  if (s->num_legs > 1 && s->cond_cr) {
    HIP_TRY(max_lds(gar::gar_condensed_cr_eliminate, gar::gar_condensed_leg_lds_doubles(s->nxb)));
    HIP_TRY(max_lds(gar::gar_condensed_cr_update, std::min(160 * 1024 / 8, gar::gar_condensed_cr_update_lds_doubles(s->nxb, 1))));
    HIP_TRY(max_lds(gar::gar_condensed_cr_assemble, s->nxb * s->nxb));
    HIP_TRY(max_lds(gar::gar_condensed_cr_back, gar::gar_condensed_cr_back_lds_doubles(s->nxb, s->num_legs)));
  }
  return GAR_HIP_OK;
}

} // namespace

// ---- padding helpers (gar_hip_solver::padded; the block rules: gar_record_io.hpp) -------------------------------
namespace {
// the caller's solution arrays out of one device solution record
void strip_solution(const gar_hip_solver *s, const double *rec, double *xs, double *us, double *vs, double *lbdas) {
  const int N = s->horizon, nx = s->unx, nu = s->unu, nc0 = s->user_nc0;
  (void)vs; // padding applies to unconstrained problems only
  auto take = [rec](double *dst, int n, int64_t off) { take_block(dst, BlockMap{n, 1, n, 1, off, 0, 0.0, kFull}, rec); };
  for (int t = 0; t <= N; ++t) {
    const gar_stage_meta &m = s->meta[t];
    if (xs)
      take(xs + (size_t)t * nx, nx, m.x_off);
    if (us && m.nu > 0)
      take(us + (size_t)t * nu, nu, m.u_off);
    if (lbdas)
      take(t == 0 ? lbdas : lbdas + nc0 + (size_t)(t - 1) * nx, t == 0 ? nc0 : nx, m.l_off);
  }
}
// one device solution record -> the caller's record layout (ulay)
void strip_solution_rec(const gar_hip_solver *s, const double *dev, double *rec) {
  const gar::HostLayout &u = *s->ulay;
  strip_solution(s, dev, rec + u.sol_x, rec + u.sol_u, rec + u.sol_v, rec + u.sol_l);
}
} // namespace

static int fetch_results_impl(gar_hip_solver *s, int b, int what, int t_lo, int t_hi, double *gains_base, bool sync);
static int prefetch_impl(gar_hip_solver *s, int b);
// (see gar_hip_solver::term_grown) the caller's dimensions as the library keeps them
void normalise_terminal(gar_hip_solver *s) {
  const int N = s->horizon;
  if (s->dense || N < 1)
    return;
  int32_t *d = &s->user_dims5[5 * (size_t)N];
  const int32_t *prev = &s->user_dims5[5 * (size_t)(N - 1)];
  if (d[1] == 0 && d[3] == 0 && d[4] == 0 && d[0] > 0 && d[0] == prev[3]) {
    d[3] = d[0];
    s->term_grown = true;
    s->term_zeros.assign((size_t)d[0] * (size_t)d[0], 0.0);
  }
}

#include "gar_multi.hpp"

extern "C" {

const char *gar_hip_version(void) { return "gar-hip 0.1 (gfx950)"; }
const char *gar_hip_last_error(void) { return g_last_error.c_str(); }

double gar_hip_stream_ceiling_ms(int device, int batch, int horizon, int64_t in_bytes_per_stage,
                                 int64_t out_bytes_per_stage, int reps) {
  // reps < 0: the walk with TWO records requested ahead (gar_stream_sweep2), |reps| repetitions
  const bool reps_ahead2 = reps < 0;
  if (reps < 0)
    reps = -reps;
  const char *lay = std::getenv("GAR_STREAM_LAYOUT"); // "stage": the layout probe of gar_stream_sweep
  const int stage_major = (lay && std::string(lay) == "stage") ? 1 : 0;
  // (north-star records fit the compiled piece counts: <= 32 x 64 x 16 B = 32 KB in, 28 KB out per stage)
  const int in_pieces = (int)((in_bytes_per_stage + 15) / 16), out_pieces = (int)((out_bytes_per_stage + 15) / 16);
  if (batch <= 0 || horizon <= 0 || in_pieces <= 0 || out_pieces <= 0 || in_pieces > 32 * 64 || out_pieces > 28 * 64 ||
      reps <= 0)
    return -1.0;
  int prev = 0;
  if (hipGetDevice(&prev) != hipSuccess || hipSetDevice(device) != hipSuccess)
    return -1.0;
  double best = -1.0;
  const size_t nin = (size_t)batch * horizon * in_pieces, nout = (size_t)batch * horizon * out_pieces; // 16-byte pieces
  { // (the owners let go at the end of this block, with `device` still current)
    DevBuf<gar::gar_double2> in, out;
    DevBuf<double> sink;
    Event e0, e1;
    if (in.alloc(nin) == hipSuccess && out.alloc(nout) == hipSuccess && sink.alloc((size_t)batch * 64) == hipSuccess &&
        hipMemset(in, 0, nin * 16) == hipSuccess && e0.create() == hipSuccess && e1.create() == hipSuccess) {
      for (int r = 0; r < reps + 1; ++r) { // first launch: warm-up
        (void)hipEventRecord(e0, nullptr);
        if (reps_ahead2)
          hipLaunchKernelGGL((gar::gar_stream_sweep2<32, 28>), dim3((unsigned)batch), dim3(64), 0, nullptr, in.get(), out.get(),
                             sink.get(), horizon, in_pieces, out_pieces);
        else
          hipLaunchKernelGGL((gar::gar_stream_sweep<32, 28>), dim3((unsigned)batch), dim3(64), 0, nullptr, in.get(), out.get(),
                             sink.get(), horizon, in_pieces, out_pieces, stage_major);
        (void)hipEventRecord(e1, nullptr);
        float ms = 0.f;
        if (hipEventSynchronize(e1) != hipSuccess || hipEventElapsedTime(&ms, e0, e1) != hipSuccess) {
          best = -1.0;
          break;
        }
        if (r > 0 && (best < 0.0 || ms < best))
          best = ms;
      }
    }
  }
  (void)hipSetDevice(prev);
  return best;
}

double gar_hip_copy_ceiling_ms(int device, int64_t bytes_moved, int reps) {
  // bytes_moved = read + written: bytes_moved / 2 are copied
  const long long n = (long long)(bytes_moved / 2 / 16);
  if (n <= 0 || reps <= 0)
    return -1.0;
  int prev = 0;
  if (hipGetDevice(&prev) != hipSuccess || hipSetDevice(device) != hipSuccess)
    return -1.0;
  double best = -1.0;
  int cus = 256;
  (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device);
  {
    DevBuf<gar::gar_double2> src, dst;
    Event e0, e1;
    if (src.alloc((size_t)n) == hipSuccess && dst.alloc((size_t)n) == hipSuccess &&
        hipMemset(src, 0, (size_t)n * 16) == hipSuccess && e0.create() == hipSuccess && e1.create() == hipSuccess) {
      for (int r = 0; r < reps + 1; ++r) { // first launch: warm-up
        (void)hipEventRecord(e0, nullptr);
        hipLaunchKernelGGL(gar::gar_plain_copy, dim3((unsigned)(cus * 64)), dim3(256), 0, nullptr, src.get(), dst.get(), n);
        (void)hipEventRecord(e1, nullptr);
        float ms = 0.f;
        if (hipEventSynchronize(e1) != hipSuccess || hipEventElapsedTime(&ms, e0, e1) != hipSuccess) {
          best = -1.0;
          break;
        }
        if (r > 0 && (best < 0.0 || ms < best))
          best = ms;
      }
    }
  }
  (void)hipSetDevice(prev);
  return best;
}

int gar_hip_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess)
    return 0;
  return n;
}

int64_t gar_hip_knot_doubles(const int32_t d[5]) {
  return gar_knot_doubles(d[0], d[1], d[2], d[3], d[4]);
}
int64_t gar_hip_factor_doubles(const int32_t d[5]) {
  return gar_factor_doubles(d[0], d[1], d[2], d[3], d[4]);
}

namespace {
gar_hip_solver *create_impl(int device, int horizon, const int32_t *dims5, int nc0, int batch,
                            int num_legs, int rank, int world, bool dense) {
  if (horizon < 0 || !dims5 || nc0 < 0 || batch < 1 || num_legs < 1 || world < 1 || rank < 0 || rank >= world ||
      (num_legs == 1 && world != 1)) {
    fail(GAR_HIP_ERR_ARG, "gar_hip_solver_create: bad argument");
    return nullptr;
  }
  if (gar_hip_device_count() <= device) {
    fail(GAR_HIP_ERR_DEVICE, "gar_hip_solver_create: no such HIP device (the HIP "
                             "backend has no CPU fallback)");
    return nullptr;
  }
  gar_hip_solver *s = new gar_hip_solver();
  s->device = device;
  s->horizon = horizon;
  s->user_nc0 = nc0;
  s->batch = batch;
  s->num_legs = num_legs;
  s->rank = rank;
  s->world = world;
  s->dense = dense;
  s->user_dims5.assign(dims5, dims5 + 5 * (horizon + 1));
  normalise_terminal(s);
  DeviceGuard guard_(device); // the caller's current device is restored on return
  auto give_up = [s]() -> gar_hip_solver * { // the one way out on failure (g_last_error says why)
    delete s; // (inside guard_: what it owns is released with its device current)
    return nullptr;
  };
  {
    int cur = -1;
    if (hipGetDevice(&cur) != hipSuccess || cur != device) {
      fail(GAR_HIP_ERR_DEVICE, "hipSetDevice failed");
      return give_up();
    }
  }
  if (configure(s) != GAR_HIP_OK)
    return give_up();
  if (s->own_stream.create(hipStreamNonBlocking) != hipSuccess) {
    fail(GAR_HIP_ERR_DEVICE, "hipStreamCreate failed");
    return give_up();
  }
  s->stream = s->own_stream;
  if (allocate(s) != GAR_HIP_OK)
    return give_up();
  { // the default schedule is the library's own choice (GAR_HIP_PIPELINE = auto | 0 | 2; gar_hip_set_pipeline overrides)
    const char *pl = gar_option("GAR_HIP_PIPELINE");
    const int want = pl ? (pl[0] == '0' ? 0 : pl[0] == '2' ? 2 : -1) : -1;
    if (want != 0 && gar_hip_set_pipeline(s, want) != GAR_HIP_OK)
      s->pipe_halves = s->pipe_requested = 0; // (an explicit 2 on a shape without the family: plain, not an error at create)
  }
  return s;
}
} // namespace

gar_hip_solver *gar_hip_solver_create_ranked(int device, int horizon, const int32_t *dims5, int nc0, int batch,
                                             int num_legs, int rank, int world) {
  return create_impl(device, horizon, dims5, nc0, batch, num_legs, rank, world, false);
}

// legs [leg_begin, leg_end) of an EVEN split (every rank the same number of legs); any split: _ranked
gar_hip_solver *gar_hip_solver_create_sharded(int device, int horizon, const int32_t *dims5,
                                              int nc0, int batch, int num_legs, int leg_begin,
                                              int leg_end) {
  const int local = leg_end - leg_begin;
  if (num_legs < 1 || local < 1 || leg_begin < 0 || leg_end > num_legs || num_legs % local != 0 || leg_begin % local != 0) {
    fail(GAR_HIP_ERR_ARG, "gar_hip_solver_create_sharded: legs must be split evenly over ranks "
                          "(use gar_hip_solver_create_ranked for any split)");
    return nullptr;
  }
  return create_impl(device, horizon, dims5, nc0, batch, num_legs, leg_begin / local, num_legs / local, false);
}

// RiccatiSolverDense (gar/dense-riccati.hpp:19-56): serial in time, any dimensions
gar_hip_solver *gar_hip_solver_create_dense(int device, int horizon, const int32_t *dims5, int nc0,
                                            int batch) {
  return create_impl(device, horizon, dims5, nc0, batch, 1, 0, 1, true);
}

gar_hip_solver *gar_hip_solver_create(int device, int horizon, const int32_t *dims5, int nc0,
                                      int batch, int num_legs) {
  return create_impl(device, horizon, dims5, nc0, batch, num_legs, 0, 1, false);
}

void gar_hip_solver_destroy(gar_hip_solver *s) {
  if (!s)
    return;
  if (s->multi) {
    multi_destroy(s);
    return;
  }
  GAR_GUARD(s); // (encloses the delete: buffers, streams and events are released with the solver's device current)
  (void)hipStreamSynchronize(s->stream); // every stream that may hold work idle first, then the owners let go
  for (const Stream &h : s->pipe.stream)
    if (h)
      (void)hipStreamSynchronize(h);
  if (s->lazy.aux_stream)
    (void)hipStreamSynchronize(s->lazy.aux_stream);
  delete s;
}

int gar_hip_set_stream(gar_hip_solver *s, void *hip_stream) {
  GAR_GUARD(s);
  if (!s)
    return fail(GAR_HIP_ERR_ARG, "null solver");
  GAR_MULTI(s, fail(GAR_HIP_ERR_UNSUPPORTED, "a multi-device solver runs on one stream per device, its own"));
  HIP_TRY(hipStreamSynchronize(s->stream));
  s->stream = hip_stream ? (hipStream_t)hip_stream : s->own_stream;
  return GAR_HIP_OK;
}

int gar_hip_sync(gar_hip_solver *s) {
  GAR_GUARD(s);
  if (!s)
    return fail(GAR_HIP_ERR_ARG, "null solver");
  GAR_MULTI(s, multi_sync(s));
  HIP_TRY(hipStreamSynchronize(s->stream));
  return GAR_HIP_OK;
}

// (the caller's records: under padding they are laid out by the caller's dimensions, `ulay`)
int64_t gar_hip_problem_doubles(const gar_hip_solver *s) { return s ? caller_layout(s).prob_doubles : 0; }
int64_t gar_hip_factors_doubles(const gar_hip_solver *s) { return s ? s->fac_doubles : 0; }
int64_t gar_hip_solution_doubles(const gar_hip_solver *s) { return s ? caller_layout(s).sol_doubles : 0; }
int gar_hip_batch(const gar_hip_solver *s) { return s ? s->batch : 0; }
int gar_hip_horizon(const gar_hip_solver *s) { return s ? s->horizon : -1; }
const char *gar_hip_kernel_name(const gar_hip_solver *s) {
  return s ? s->kernel_name.c_str() : "";
}

int gar_hip_suggest_num_legs(int horizon, int nx, int nu) {
  (void)nu;
  if (horizon < 1)
    return 1;
  const int per_leg = nx <= 36 ? 4 : 8; // stages per leg (measured at N = 256: include/gar_hip.h)
  const int legs = (horizon + per_leg - 1) / per_leg;
  return legs < 2 ? 2 : (legs > horizon + 1 ? horizon + 1 : legs);
}

const char *gar_hip_condensed_solver_name(const gar_hip_solver *s) {
  if (!s || s->num_legs < 2)
    return "";
  GAR_MULTI(s, gar_hip_condensed_solver_name(s->multi->subs[0]));
  if (s->cyc_setup_kernel)
    return "cyclic"; // gar_cyclic.hpp (specialised leg families), the wave-scope chain gated behind it
  if (s->cond_wave_kernel)
    return "chain";
  if (s->cond_reduced)
    return s->cond_cr ? "reduced+cyclic" : "reduced+chain"; // gar_generic.hpp / gar_condensed_cr.hpp
  return "generic-chain";
}

int gar_hip_stage_offsets(const gar_hip_solver *s, int t, int64_t out[6]) {
  if (int rc = check_bt(s, 0, t))
    return rc;
  const gar_stage_meta &m = caller_layout(s).meta[t];
  out[0] = m.in_off;
  out[1] = s->meta[t].fac_off; // factor records exist on the device only
  out[2] = m.x_off;
  out[3] = m.u_off;
  out[4] = m.v_off;
  out[5] = m.l_off;
  return GAR_HIP_OK;
}

int gar_hip_init_offsets(const gar_hip_solver *s, int64_t out[2]) {
  if (!s)
    return fail(GAR_HIP_ERR_ARG, "null solver");
  out[0] = caller_layout(s).G0_off;
  out[1] = caller_layout(s).g0_off;
  return GAR_HIP_OK;
}

int gar_hip_upload_packed(gar_hip_solver *s, int b0, int nb, const double *packed) {
  GAR_GUARD(s);
  if (!s || !packed || b0 < 0 || nb < 0 || b0 + nb > s->batch)
    return fail(GAR_HIP_ERR_ARG, "gar_hip_upload_packed: bad argument");
  // The device's records differ from the caller's (padding, packed triangles of Q / R): knot by knot through
  // gar_hip_upload_stage, which routes to the stage's owner on a multi-device solver.  (A padded solver is unconstrained
  // and unparameterised; one that only packs Q / R may carry both.)
  if (s->padded || s->qr_packed) {
    const gar::HostLayout &u = caller_layout(s);
    for (int b = b0; b < b0 + nb; ++b) {
      const double *rec = packed + (int64_t)(b - b0) * u.prob_doubles;
      for (int t = 0; t <= s->horizon; ++t) {
        const gar_stage_meta &m = u.meta[t];
        const gar_knot_offsets o = gar_knot_layout(m.nx, m.nu, m.nc, m.nx2, (m.flags & GAR_KNOT_HAS_PARAM) ? m.nth : 0);
        const double *k = rec + m.in_off;
        if (int rc = gar_hip_upload_stage(s, b, t, k + o.Q, k + o.S, k + o.R, k + o.q, k + o.r, k + o.A, k + o.B, k + o.f,
                                          k + o.C, k + o.D, k + o.d, k + o.Gth, k + o.Gx, k + o.Gu, k + o.Gv, k + o.gamma))
          return rc;
      }
      if (int rc = gar_hip_set_init(s, b, rec + u.G0_off, rec + u.g0_off))
        return rc;
    }
    return GAR_HIP_OK;
  }
  GAR_MULTI(s, multi_upload_packed(s, b0, nb, packed)); // (each device its own range of the records)
  s->cur.matrices_changed("gar_hip_upload_packed");
  const size_t bytes = sizeof(double) * (size_t)s->prob_doubles * nb;
  if (s->buf.staged) {
    std::memcpy(s->buf.h_prob + (int64_t)b0 * s->prob_doubles, packed, bytes);
    for (int b = b0; b < b0 + nb; ++b) {
      s->buf.dirty_iv[(size_t)b].clear();
      mark_dirty(s, b, 0, s->prob_doubles);
    }
    return GAR_HIP_OK;
  }
  HIP_TRY(hipMemcpyAsync(s->buf.d_prob + (int64_t)b0 * s->prob_doubles, packed, bytes,
                         hipMemcpyHostToDevice, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  return GAR_HIP_OK;
}

int gar_hip_upload_packed_device(gar_hip_solver *s, int b0, int nb, const double *packed_dev) {
  GAR_GUARD(s);
  GAR_MULTI(s, fail(GAR_HIP_ERR_UNSUPPORTED, "device-resident upload into a multi-device solver: the records live on several devices"));
  if (!s || !packed_dev || b0 < 0 || nb < 0 || b0 + nb > s->batch)
    return fail(GAR_HIP_ERR_ARG, "gar_hip_upload_packed_device: bad argument");
  if (int rc = commit(s)) // staged host data first, then the device copy wins
    return rc;
  s->cur.matrices_changed("gar_hip_upload_packed_device");
  HIP_TRY(hipMemcpyAsync(s->buf.d_prob + (int64_t)b0 * s->prob_doubles, packed_dev,
                         sizeof(double) * (size_t)s->prob_doubles * nb, hipMemcpyDeviceToDevice,
                         s->stream));
  // (the staging area stays in use: commit() flushes only the ranges the host writes later)
  return GAR_HIP_OK;
}

int gar_hip_upload_packed_device_fmt(gar_hip_solver *s, int b0, int nb, const double *packed_dev, int record_format) {
  if (s && ((record_format & GAR_HIP_FMT_QR_PACKED) != 0) != s->qr_packed)
    return fail(GAR_HIP_ERR_ARG, std::string("gar_hip_upload_packed_device_fmt: the records were written with ") +
                                     ((record_format & GAR_HIP_FMT_QR_PACKED) ? "packed lower triangles" : "full blocks") +
                                     " of Q / R, this solver's sweep (" + s->kernel_name + ") reads " +
                                     (s->qr_packed ? "packed lower triangles" : "full blocks") +
                                     " (gar_hip_device_record_format)");
  return gar_hip_upload_packed_device(s, b0, nb, packed_dev);
}

int gar_hip_commit(gar_hip_solver *s) {
  GAR_GUARD(s);
  if (!s)
    return fail(GAR_HIP_ERR_ARG, "null solver");
  GAR_MULTI(s, multi_all(s, [](gar_hip_solver *q) { return gar_hip_commit(q); }));
  return commit(s);
}

double *gar_hip_device_problems(gar_hip_solver *s) {
  pipe_autojoin(s);
  return s ? s->buf.d_prob : nullptr;
}
double *gar_hip_device_factors(gar_hip_solver *s) {
  if (s && s->multi) // (the records live on several devices)
    return nullptr;
  if (s && s->fold) { // the caller-visible records of a folded solver are formed on request
    GAR_GUARD(s);
    (void)ensure_expanded(s);
  } else if (s && s->pipe.forked) { // (a pipelined sweep: the caller's stream is ordered behind it before the pointer leaves)
    GAR_GUARD(s);
  }
  return s ? s->buf.d_fac : nullptr;
}
double *gar_hip_device_solutions(gar_hip_solver *s) {
  pipe_autojoin(s); // (a pipelined sweep: the caller's stream is ordered behind it before the pointer leaves)
  return s ? s->buf.d_sol : nullptr;
}

int gar_hip_backward_legs_async(gar_hip_solver *s, double mueq) {
  GAR_GUARD(s);
  if (!s)
    return fail(GAR_HIP_ERR_ARG, "null solver");
  // A knot whose solve divides by mueq outright -- terminalSolve without controls, Z = C / mu (riccati-kernel.hxx:146-149);
  // the serial constrained chain and the constrained segment legs (gar_wave2.hpp's decoupled stage; both bind only where
  // the terminal knot is constrained) -- turns mueq = 0 into infinities that the factorisations downstream index with:
  // reported as the failed stage it is, before anything is launched.  The other fold solvers divide only on the device's
  // say-so: the fold flags mu <= 0 and hands such a problem to the generic leg kernels (gar_fold.hpp), which solve
  // [Rhat D^T; D 0] where D has full row rank and report the singular stages themselves, as the reference does
  // (:239-241).  A non-finite mueq on constrained knots is refused whatever the family.
  if (s->mu_divides && !(std::fabs(mueq) >= 1e-290))
    return fail(GAR_HIP_ERR_FACTOR, "Failed stage LDL factorization (mueq = " + std::to_string(mueq) +
                                        " on constrained knots whose solve divides by it)");
  if (s->any_nc && !(std::fabs(mueq) <= DBL_MAX))
    return fail(GAR_HIP_ERR_FACTOR, "Failed stage LDL factorization (mueq = " + std::to_string(mueq) +
                                        " on constrained knots)");
  GAR_MULTI(s, multi_backward_legs(s, mueq));
  s->cur.backward_enqueued(mueq);
  if (int rc = settle_gains_readback(s, kBehindStream))
    return rc;
  if (int rc = commit(s))
    return rc;
  HIP_TRY(hipMemsetAsync(status_words(s), 0, status_bytes((size_t)s->batch, s->fold), s->stream));
  return launch_backward(s, mueq);
}

int gar_hip_condensed_solve_async(gar_hip_solver *s) {
  GAR_GUARD(s);
  if (!s || s->num_legs < 2)
    return fail(GAR_HIP_ERR_ARG, "condensed solve needs leg mode");
  GAR_MULTI(s, multi_exchange_and_condensed(s)); // the boundary exchange happens HERE, inside the library
  return launch_condensed(s);
}

int gar_hip_forward_legs_async(gar_hip_solver *s) {
  GAR_GUARD(s);
  if (!s)
    return fail(GAR_HIP_ERR_ARG, "null solver");
  GAR_MULTI(s, multi_forward(s));
  return launch_forward(s, nullptr);
}

int gar_hip_set_option(const char *name, const char *value) {
  if (!name || !*name)
    return fail(GAR_HIP_ERR_ARG, "gar_hip_set_option: empty name");
  std::string key = name;
  if (key.rfind("GAR_HIP_", 0) != 0)
    key = "GAR_HIP_" + key;
  static const char *known[] = {"BACKWARD", "WIDE", "LEG_WAVES", "CONDENSED", "CONDENSED_REDUCED", "CONDENSED_CR", "LEGS",
                                "FOLD", "SERIAL_FOLD", "SEG_LEGS", "INIT", "FORCE_GENERIC", "PAD", "SPD_ACCEPT", "STAGE_NT", "EAGER",
                                "MULTI_EXCHANGE", "PIPE_PRIORITY", "FORWARD", "PIPELINE", "CSTR_SEG_LEGS",
                                "CSTR_SEG_LEG_END", "CSTR_SEG_FORWARD"};
  bool ok = false;
  for (const char *k : known)
    ok |= key == std::string("GAR_HIP_") + k;
  if (!ok)
    return fail(GAR_HIP_ERR_ARG, "gar_hip_set_option: unknown switch " + key + " (include/gar_hip.h lists them)");
  std::lock_guard<std::mutex> g(option_mutex());
  if (value)
    option_overrides()[key] = value;
  else
    option_overrides().erase(key);
  return GAR_HIP_OK;
}
const char *gar_hip_get_option(const char *name) {
  if (!name)
    return nullptr;
  std::string key = name;
  if (key.rfind("GAR_HIP_", 0) != 0)
    key = "GAR_HIP_" + key;
  return gar_option(key.c_str());
}

namespace {
std::string failed_stages_text(int nf) { return "Failed stage LDL factorization (" + std::to_string(nf) + " problem(s))"; }
// how a blocking entry point (`who`: its short name) ends: the host waits for the status words of the sweep it enqueued
int failure_epilogue(gar_hip_solver *s, const char *who) {
  const int nf = gar_hip_num_failed(s);
  if (nf < 0)
    return fail(GAR_HIP_ERR_DEVICE, std::string(who) + ": " + hipGetErrorString(hipGetLastError()));
  return nf > 0 ? fail(GAR_HIP_ERR_FACTOR, failed_stages_text(nf)) : GAR_HIP_OK;
}
// two of the status counters (status_counters), from `first` on
int read_counters(gar_hip_solver *s, int first, int64_t out[2]) {
  if (!s || !out)
    return fail(GAR_HIP_ERR_ARG, "bad argument");
  int c[2] = {0, 0};
  HIP_TRY(hipMemcpyAsync(c, status_counters(s) + first, sizeof(c), hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  out[0] = c[0];
  out[1] = c[1];
  return GAR_HIP_OK;
}
bool pipe_eligible(const gar_hip_solver *s) {
  return !(s->multi || s->world > 1 || s->num_legs != 1 || s->nth0 != 0 || s->batch < 2 || !s->wave_kernel || !s->lean_fwd_kernel ||
           !s->wave_half_kernel || s->wave_coupled_kernel || s->wave_block_threads != 64 || s->waves_per_block != 1 || !s->vxx_packed ||
           s->dense || s->serial_fold);
}
// The library's own choice of schedule (GAR_HIP_PIPELINE = auto, the default): the pipelined sweep pays by the tails
// it hides -- the forward sweep of one half starts while the other half's backward sweep still runs -- and only once
// EACH half fills every SIMD of the chip with a backward wave (measured, round 5: +0.4 ... +3.7 % at 4 096 problems on
// 256 CUs over four boxes, -0.2 % on one; below two full waves of problems per half the plain schedule's whole-chip
// launches win).  So: 2 halves iff the solver is eligible and batch >= 2 x (4 SIMDs x #CUs); plain otherwise.
int pipe_auto_halves(const gar_hip_solver *s) {
  if (!pipe_eligible(s))
    return 0;
  int cus = 256;
  (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, s->device);
  if (cus <= 0) // (a runtime that does not know: the MI355X's count)
    cus = 256;
  return s->batch >= 8 * cus ? 2 : 0;
}
} // namespace

int gar_hip_set_pipeline(gar_hip_solver *s, int halves) {
  GAR_GUARD(s); // (orders the caller's stream behind anything the half streams still hold)
  if (!s)
    return fail(GAR_HIP_ERR_ARG, "null solver");
  bool automatic = false;
  if (halves < 0) { // the library's choice: never an error
    automatic = true;
    halves = pipe_auto_halves(s);
    if (halves <= 1) {
      s->pipe_halves = 0;
      s->pipe_requested = -1;
      return GAR_HIP_OK;
    }
  }
  if (halves <= 1) {
    s->pipe_halves = s->pipe_requested = 0;
    return GAR_HIP_OK;
  }
  if (halves != 2)
    return fail(GAR_HIP_ERR_ARG, "gar_hip_set_pipeline: 0 (off) or 2 (two half-batches)");
  if (!pipe_eligible(s))
    return fail(GAR_HIP_ERR_UNSUPPORTED, "pipelined sweep: serial, unconstrained, unparameterised batches (>= 2 problems) "
                                         "on the one-wave-per-problem kernel family only (this solver runs " +
                                             s->kernel_name + ")");
  if (int rc = pipe_plan(s, s->lean_fwd_used))
    return rc;
  if (!s->pipe.stream[0]) { // first request served: the group is made whole or not at all
    gar::PipeState fresh;
    HIP_TRY(hipFuncSetAttribute((const void *)s->lean_fwd_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)s->lean_fwd_lds_bytes));
    HIP_TRY(hipFuncSetAttribute((const void *)s->wave_half_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)((size_t)s->wave_lds_doubles_small * sizeof(double))));
    for (int h = 0; h < 2; ++h) {
      {
        // two streams that share a hardware queue run their kernels one after the other, in submission order: the
        // runtime hands out at most GPU_MAX_HW_QUEUES (4) queues PER PRIORITY, so the halves ask for different ones
        // (with GPU_MAX_HW_QUEUES >= 8 in the environment -- bench.py sets it before the runtime starts -- plain
        // streams get queues of their own; GAR_HIP_PIPE_PRIORITY=0 / 1 forces the choice)
        const char *pp = gar_option("GAR_HIP_PIPE_PRIORITY"), *mq = std::getenv("GPU_MAX_HW_QUEUES");
        int lo = 0, hi = 0;
        (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
        const bool plain = pp ? pp[0] == '0' : (mq && std::atoi(mq) >= 8);
        if (plain)
          HIP_TRY(fresh.stream[h].create(hipStreamNonBlocking));
        else
          HIP_TRY(fresh.stream[h].create_with_priority(hipStreamNonBlocking, h == 0 ? 0 : hi));
      }
      HIP_TRY(fresh.evB[h].create(hipEventDisableTiming));
      HIP_TRY(fresh.evF[h].create(hipEventDisableTiming));
      for (Event &e : fresh.evT[h])
        HIP_TRY(e.create());
    }
    HIP_TRY(fresh.evFork.create(hipEventDisableTiming));
    s->pipe = std::move(fresh);
  }
  s->pipe_halves = 2;
  s->pipe_requested = automatic ? -1 : 2;
  return GAR_HIP_OK;
}
int gar_hip_pipeline(const gar_hip_solver *s) { return s ? s->pipe_halves : 0; }

int gar_hip_backward_async(gar_hip_solver *s, double mueq) {
  GAR_GUARD_NOJOIN(s);
  if (pipe_on(s))
    return pipe_backward(s, mueq);
  pipe_autojoin(s);
  if (int rc = gar_hip_backward_legs_async(s, mueq))
    return rc;
  GAR_MULTI(s, multi_exchange_and_condensed(s));
  if (s->num_legs > 1) {
    if (s->world > 1)
      return fail(GAR_HIP_ERR_ARG, "sharded solver: exchange boundaries, then call "
                                   "gar_hip_condensed_solve_async");
    return launch_condensed(s);
  }
  return GAR_HIP_OK;
}

// The caller's whole problem and backward(mueq) in ONE call (what the binding's backward() has in hand): the
// sequence gar_hip_upload_stage x (N+1), gar_hip_set_init, gar_hip_backward behind one crossing of the ABI (the
// staged knots go out in 1 MiB pieces while the next ones are packed, gar_hip_upload_stage).
int gar_hip_backward_blocks(gar_hip_solver *s, const double *const *blocks, const double *G0, const double *g0,
                            double mueq) {
  GAR_GUARD(s);
  if (!s || !blocks)
    return fail(GAR_HIP_ERR_ARG, "gar_hip_backward_blocks: bad argument");
  if (s->batch != 1)
    return fail(GAR_HIP_ERR_ARG, "gar_hip_backward_blocks serves one problem (batch = 1): use gar_hip_upload_stage / "
                                 "gar_hip_upload_packed + gar_hip_backward for a batch");
  const int N = s->horizon;
  auto upload = [&](int t) {
    const double *const *k = blocks + 16 * (size_t)t;
    return gar_hip_upload_stage(s, 0, t, k[0], k[1], k[2], k[3], k[4], k[5], k[6], k[7], k[8], k[9], k[10], k[11], k[12],
                                k[13], k[14], k[15]);
  };
  // (Measured and not kept, round 4: sweeping the legs chunk by chunk as their knots arrive, copies on a stream of
  // their own -- the sweep of a chunk takes as long as the sweep of all legs, a leg being a sequential chain over its
  // stages, so the critical path stays packing + one leg + condensed solve; chunks on one stream add their sweeps:
  // (56, 22), 32 legs: 2.35 -> 2.95 ms per Newton iteration.)
  // (Measured and not kept, round 4: a second host thread packing alternate 1 MiB chunks of a >= 12 MiB problem --
  // (56, 22), 32 legs: 1.53-1.57 -> 1.50 ms for this call, the link and the host's memory system are the bound, not
  // the packing core; profiles/r04_seam_two_packing_threads_not_kept.json.)
  for (int t = 0; t <= N; ++t)
    if (int rc = upload(t))
      return rc;
  if (int rc = gar_hip_set_init(s, 0, G0, g0))
    return rc;
  // Without a parameter the roll-out depends on nothing the caller still has to say: it is enqueued right behind the
  // sweep, with the solution's copy and the gains' read-back (second stream), BEFORE the host waits for the status
  // word -- the device runs sweep, roll-out and copies back to back instead of waiting for the host between them.
  // gar_hip_forward / gar_hip_prefetch_gains / the solution fetch then find their work done.
  const bool eager = !option_off("GAR_HIP_EAGER") && !s->multi && !s->fold && !s->dense &&
                     (s->nth0 == 0 || s->num_legs > 1) && s->world == 1;
  if (!eager)
    return gar_hip_backward(s, mueq);
  if (int rc = gar_hip_backward_legs_async(s, mueq))
    return rc;
  if (s->num_legs > 1) {
    // the gains are final once the leg sweeps are (the condensed solve reads the boundary tuples and writes the
    // boundary solution): their read-back starts HERE, under the condensed solve, not behind it
    if (int rc = prefetch_impl(s, 0)) // (allocates the read-back buffers on first use)
      return rc;
    if (int rc = launch_condensed(s))
      return rc;
  }
  if (!s->lazy.h_status) {
    PinnedBuf<int> h;
    Event status, sol;
    HIP_TRY(h.alloc((size_t)s->batch, hipHostMallocDefault));
    HIP_TRY(status.create(hipEventDisableTiming));
    HIP_TRY(sol.create(hipEventDisableTiming));
    s->lazy.h_status = std::move(h);
    s->lazy.ev_status = std::move(status);
    s->lazy.ev_sol = std::move(sol);
  }
  HIP_TRY(hipMemcpyAsync(s->lazy.h_status, s->buf.d_status, sizeof(int) * (size_t)s->batch, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipEventRecord(s->lazy.ev_status, s->stream));
  if (s->num_legs == 1)
    if (int rc = prefetch_impl(s, 0))
      return rc;
  if (int rc = launch_forward(s, nullptr))
    return rc;
  {
    const gar::HostLayout &u = caller_layout(s);
    const size_t nsol = (size_t)u.sol_doubles, ngain = (size_t)(u.ff_all_doubles + u.fb_all_doubles);
    // by a kernel's own stores into the pinned buffer: the copy engine is busy with the gains (3.7 / 9.4 MB) and a
    // hipMemcpyAsync would queue behind them (measured: profiles/r04_seam_eager_rollout_ab.json)
    double *dst = s->buf.h_results + (s->padded ? nsol + ngain : 0);
    const unsigned nblk = (unsigned)std::min<int64_t>((s->sol_doubles + 255) / 256, 256);
    hipLaunchKernelGGL(gar::gar_store_to_host, dim3(nblk), dim3(256), 0, s->stream, dst, s->buf.d_sol.get(), (long long)s->sol_doubles);
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(hipEventRecord(s->lazy.ev_sol, s->stream));
  HIP_TRY(hipEventSynchronize(s->lazy.ev_status));
  int nf = 0;
  for (int b = 0; b < s->batch; ++b)
    nf += (s->lazy.h_status[b] != 0);
  if (nf > 0) {
    // the roll-out, the solution's copy and the gains' read-back of the FAILED sweep are already enqueued: let them
    // finish and disarm the "already in flight" shortcuts, so that a later fetch does its own work (and nobody is
    // handed these gains as if the sweep had succeeded)
    if (int rc = settle_gains_readback(s, kBehindHost))
      return rc;
    s->cur.solution_superseded();
    return fail(GAR_HIP_ERR_FACTOR, failed_stages_text(nf));
  }
  s->cur.host_solution_enqueued();
  return GAR_HIP_OK;
}

int gar_hip_num_failed(gar_hip_solver *s) {
  GAR_GUARD(s);
  if (!s)
    return 0;
  GAR_MULTI(s, multi_num_failed(s));
  std::vector<int> st((size_t)s->batch);
  if (hipMemcpyAsync(st.data(), s->buf.d_status, sizeof(int) * st.size(), hipMemcpyDeviceToHost,
                     s->stream) != hipSuccess ||
      hipStreamSynchronize(s->stream) != hipSuccess)
    return -1;
  int n = 0;
  for (int v : st)
    n += (v != 0);
  return n;
}

int gar_hip_slow_path_stages(gar_hip_solver *s, int64_t out[2]) {
  GAR_GUARD(s);
  GAR_MULTI(s, multi_counters(s, out, gar_hip_slow_path_stages));
  return read_counters(s, 0, out);
}

int gar_hip_constrained_bk_stages(gar_hip_solver *s, int64_t out[2]) {
  GAR_GUARD(s);
  GAR_MULTI(s, multi_counters(s, out, gar_hip_constrained_bk_stages));
  return read_counters(s, 2, out);
}

int gar_hip_backward(gar_hip_solver *s, double mueq) {
  GAR_GUARD(s);
  if (int rc = gar_hip_backward_async(s, mueq))
    return rc;
  return failure_epilogue(s, "backward");
}

int gar_hip_forward_async(gar_hip_solver *s, const double *theta_device) {
  GAR_GUARD_NOJOIN(s);
  if (!s)
    return fail(GAR_HIP_ERR_ARG, "null solver");
  if (pipe_on(s))
    return pipe_forward(s);
  pipe_autojoin(s);
  GAR_MULTI(s, multi_forward(s));
  return launch_forward(s, theta_device);
}

int gar_hip_forward(gar_hip_solver *s, const double *theta) {
  GAR_GUARD(s);
  if (!s)
    return fail(GAR_HIP_ERR_ARG, "null solver");
  if (s->multi) {
    if (int rc = multi_forward(s))
      return rc;
    return multi_sync(s);
  }
  if (s->cur.host_solution) { // enqueued behind the sweep by gar_hip_backward_blocks (no parameter: theta has no say)
    HIP_TRY(hipEventSynchronize(s->lazy.ev_sol));
    return GAR_HIP_OK;
  }
  const double *th = nullptr;
  if (theta && s->nth0 > 0 && s->num_legs == 1) {
    HIP_TRY(hipMemcpyAsync(s->buf.d_theta, theta, sizeof(double) * (size_t)s->nth0 * s->batch,
                           hipMemcpyHostToDevice, s->stream));
    th = s->buf.d_theta;
  }
  if (int rc = launch_forward(s, th))
    return rc;
  HIP_TRY(hipStreamSynchronize(s->stream));
  return GAR_HIP_OK;
}

// ---- lqrComputeKktError for the whole batch, on the device (gar_kkt.hpp; launch_kkt in gar_resident.hpp) -----------
namespace {
int kkt_check(const gar_hip_solver *s, const void *theta) {
  if (!s)
    return fail(GAR_HIP_ERR_ARG, "null solver");
  if (s->multi)
    return fail(GAR_HIP_ERR_UNSUPPORTED, "device-side KKT residuals on a multi-device solver: the records live on several devices");
  if (theta && (s->num_legs > 1 || s->nth0 == 0))
    return fail(GAR_HIP_ERR_ARG, "gar_hip_kkt_error: theta on a solver without parameter (leg mode, or nth = 0)");
  if (theta) // Gx theta, Gu theta of EVERY stage: a record with another column count has no product with this theta
    for (const gar_stage_meta &m : s->meta)
      if (((m.flags & GAR_KNOT_HAS_PARAM) ? m.nth : 0) != s->nth0)
        return fail(GAR_HIP_ERR_ARG, "gar_hip_kkt_error: theta on a problem whose stages differ in nth");
  return GAR_HIP_OK;
}
} // namespace

int gar_hip_kkt_error_async(gar_hip_solver *s, double mueq, const double *theta_device) {
  GAR_GUARD(s); // (a pipelined sweep: the solver's stream is ordered behind the half streams first)
  if (int rc = kkt_check(s, theta_device))
    return rc;
  return launch_kkt(s, mueq, theta_device);
}

int gar_hip_kkt_error(gar_hip_solver *s, double mueq, const double *theta_host, double *out3, double *stage4) {
  GAR_GUARD(s);
  if (int rc = kkt_check(s, theta_host))
    return rc;
  const double *th = nullptr;
  if (theta_host) { // staged as gar_hip_forward stages it
    HIP_TRY(hipMemcpyAsync(s->buf.d_theta, theta_host, sizeof(double) * (size_t)s->nth0 * s->batch, hipMemcpyHostToDevice,
                           s->stream));
    th = s->buf.d_theta;
  }
  if (int rc = launch_kkt(s, mueq, th))
    return rc;
  int rc = d2h(s, out3, s->buf.kkt.err, (int64_t)s->batch * 3);
  rc |= d2h(s, stage4, s->buf.kkt.stage, (int64_t)s->batch * (s->horizon + 1) * 4);
  if (rc)
    return rc;
  HIP_TRY(hipStreamSynchronize(s->stream));
  return GAR_HIP_OK;
}

const double *gar_hip_device_kkt_errors(gar_hip_solver *s) {
  pipe_autojoin(s);
  return s && !s->multi ? s->buf.kkt.err.get() : nullptr;
}
const double *gar_hip_device_kkt_stage_errors(gar_hip_solver *s) {
  pipe_autojoin(s);
  return s && !s->multi ? s->buf.kkt.stage.get() : nullptr;
}

// ---- the services on a resident batch (gar_resident.hpp: work areas, launches and resident_begin, the prologue) -------
// re-solve for new affine terms from the stored factorisation (gar_affine.hpp)
int64_t gar_hip_affine_doubles(const gar_hip_solver *s) { return s && !s->user_dims5.empty() ? affine_offsets(s, nullptr) : 0; }

int gar_hip_upload_affine_device(gar_hip_solver *s, int b0, int nb, const double *affine_dev) {
  GAR_GUARD(s);
  if (int rc = resident_begin(s, "gar_hip_upload_affine_device", bad_range(s, affine_dev, b0, nb), nullptr, 0, {ensure_affine}))
    return rc;
  return launch_affine_scatter(s, b0, nb, affine_dev);
}

int gar_hip_upload_affine(gar_hip_solver *s, int b0, int nb, const double *affine_host) {
  GAR_GUARD(s);
  if (int rc = resident_begin(s, "gar_hip_upload_affine", bad_range(s, affine_host, b0, nb), nullptr, 0, {ensure_affine}))
    return rc;
  const size_t n = (size_t)affine_offsets(s, nullptr);
  if (n == 0 || nb == 0)
    return GAR_HIP_OK;
  gar::AffineArea &a = s->buf.aff;
  if (!a.staging)
    HIP_TRY(a.staging.alloc(n * (size_t)s->batch));
  if (int rc = commit(s)) // (the pinned area is free once its staged blocks are on their way)
    return rc;
  // through the pinned staging area where there is one (a problem's record is longer than its affine vector)
  const double *from = affine_host;
  if (s->buf.staged) {
    HIP_TRY(hipStreamSynchronize(s->stream));
    std::memcpy(s->buf.h_prob.get(), affine_host, sizeof(double) * n * (size_t)nb);
    from = s->buf.h_prob;
  }
  HIP_TRY(hipMemcpyAsync(a.staging.get(), from, sizeof(double) * n * (size_t)nb, hipMemcpyHostToDevice, s->stream));
  if (int rc = launch_affine_scatter(s, b0, nb, a.staging))
    return rc;
  HIP_TRY(hipStreamSynchronize(s->stream));
  return GAR_HIP_OK;
}

int gar_hip_backward_affine_async(gar_hip_solver *s) {
  GAR_GUARD(s); // (a pipelined sweep: the solver's stream is ordered behind the half streams first)
  if (int rc = resident_begin(s, "gar_hip_backward_affine", nullptr, "re-solve", 0, {ensure_affine}))
    return rc;
  return launch_backward_affine(s);
}

int gar_hip_backward_affine(gar_hip_solver *s) {
  GAR_GUARD(s);
  if (int rc = gar_hip_backward_affine_async(s))
    return rc;
  return failure_epilogue(s, "backward_affine");
}

// iterative refinement from the stored factorisation (gar_refine.hpp)
namespace {
int refine_begin(gar_hip_solver *s, int steps, double threshold, const char *who) {
  const char *bad = steps < 0 || threshold != threshold ? "the step count must be >= 0 and the threshold not NaN" : nullptr;
  return resident_begin(s, who, bad, "refine", kNeedsSolution | kSupersedesSolution | kCommits, {ensure_refine, ensure_kkt});
}
} // namespace

int gar_hip_refine_async(gar_hip_solver *s, int steps, double threshold) {
  GAR_GUARD(s); // (a pipelined sweep: the solver's stream is ordered behind the half streams first)
  if (int rc = refine_begin(s, steps, threshold, "gar_hip_refine_async"))
    return rc;
  RoctxRange range_("gar::refine");
  for (int i = 0; i < steps; ++i) {
    if (int rc = launch_refine_residual(s, threshold))
      return rc;
    if (int rc = launch_refine_correction(s))
      return rc;
  }
  return launch_refine_residual(s, threshold); // the KKT buffers describe the solution that is in HBM
}

int gar_hip_refine(gar_hip_solver *s, int max_steps, double threshold, int32_t out2[2]) {
  GAR_GUARD(s);
  if (int rc = refine_begin(s, max_steps, threshold, "gar_hip_refine"))
    return rc;
  RoctxRange range_("gar::refine");
  std::vector<int> gate((size_t)s->batch);
  int steps = 0, remaining = 0;
  for (;;) {
    if (int rc = launch_refine_residual(s, threshold))
      return rc;
    HIP_TRY(hipMemcpyAsync(gate.data(), s->buf.ref.gate.get(), sizeof(int) * gate.size(), hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    remaining = 0;
    for (int v : gate)
      remaining += (v != 0);
    if (remaining == 0 || steps == max_steps)
      break;
    if (int rc = launch_refine_correction(s))
      return rc;
    ++steps;
  }
  if (out2) {
    out2[0] = steps;
    out2[1] = remaining;
  }
  return failure_epilogue(s, "refine");
}

// gradients of a resident batch (gar_adjoint.hpp)
int gar_hip_upload_packed_user_device(gar_hip_solver *s, int b0, int nb, const double *packed_user_dev) {
  GAR_GUARD(s);
  if (int rc = resident_begin(s, "gar_hip_upload_packed_user_device", bad_range(s, packed_user_dev, b0, nb), nullptr,
                              kCommits, {ensure_user_layout})) // staged host data first, then the device copy wins
    return rc;
  s->cur.matrices_changed("gar_hip_upload_packed_user_device");
  return launch_user_upload(s, b0, nb, packed_user_dev);
}

int gar_hip_solution_vectors_device(gar_hip_solver *s, int b0, int nb, double *out_dev) {
  GAR_GUARD(s); // (a pipelined sweep: the solver's stream is ordered behind the half streams first)
  if (int rc = resident_begin(s, "gar_hip_solution_vectors_device", bad_range(s, out_dev, b0, nb), nullptr, 0,
                              {ensure_affine, ensure_user_layout}))
    return rc;
  return launch_solution_gather(s, b0, nb, s->buf.d_sol, out_dev);
}

namespace {
int adjoint_begin(gar_hip_solver *s, const void *cot, const void *grad, const char *who) {
  const char *bad = !cot ? "null cotangent" : nullptr;
  if (!bad && (reinterpret_cast<uintptr_t>(grad) & 15))
    bad = "the gradient records must start on a 16-byte boundary";
  return resident_begin(s, who, bad, "differentiate", kNeedsSolution | kCommits, {ensure_adjoint});
}
} // namespace

int gar_hip_adjoint_async(gar_hip_solver *s, const double *cot_dev, double *adj_out_dev, double *grad_out_dev) {
  GAR_GUARD(s); // (a pipelined sweep: the solver's stream is ordered behind the half streams first)
  if (int rc = adjoint_begin(s, cot_dev, grad_out_dev, "gar_hip_adjoint_async"))
    return rc;
  return launch_adjoint(s, cot_dev, adj_out_dev, grad_out_dev);
}

int gar_hip_adjoint(gar_hip_solver *s, const double *cot_host, double *adj_host, double *grad_host) {
  GAR_GUARD(s);
  if (int rc = adjoint_begin(s, cot_host, nullptr, "gar_hip_adjoint"))
    return rc;
  const size_t n = (size_t)affine_offsets(s, nullptr) * (size_t)s->batch;
  const size_t ng = (size_t)caller_layout(s).prob_doubles * (size_t)s->batch;
  gar::AdjointArea &a = s->buf.adj;
  if (!a.staging)
    HIP_TRY(a.staging.alloc(2 * n + 2));
  if (grad_host && !a.grad)
    HIP_TRY(a.grad.alloc(ng));
  double *cot = a.staging, *adj = cot + n;
  HIP_TRY(hipMemcpyAsync(cot, cot_host, sizeof(double) * n, hipMemcpyHostToDevice, s->stream));
  if (int rc = launch_adjoint(s, cot, adj_host ? adj : nullptr, grad_host ? a.grad.get() : nullptr))
    return rc;
  if (int rc = d2h(s, adj_host, adj, (int64_t)n))
    return rc;
  if (int rc = d2h(s, grad_host, a.grad, (int64_t)ng))
    return rc;
  HIP_TRY(hipStreamSynchronize(s->stream));
  return failure_epilogue(s, "adjoint");
}

const double *gar_hip_device_adjoints(gar_hip_solver *s) {
  pipe_autojoin(s);
  return s && !s->multi ? s->buf.adj.rec.get() : nullptr;
}

// many affine terms at once (gar_affine_multi.hpp): gar_hip_backward_affine's state -- no forward, the primal solution is
// not read
namespace {
int affine_multi_begin(gar_hip_solver *s, int nrhs, const void *rhs, const void *out, const char *who) {
  const char *bad = nrhs < 1 || !rhs || !out ? "nrhs must be >= 1 and neither array null" : nullptr;
  return resident_begin(s, who, bad, "solve", kCommits, {ensure_affine_multi});
}
} // namespace

int gar_hip_affine_solve_multi_async(gar_hip_solver *s, int nrhs, const double *rhs_dev, double *out_dev) {
  GAR_GUARD(s); // (a pipelined sweep: the solver's stream is ordered behind the half streams first)
  if (int rc = affine_multi_begin(s, nrhs, rhs_dev, out_dev, "gar_hip_affine_solve_multi_async"))
    return rc;
  return launch_affine_multi(s, nrhs, rhs_dev, out_dev);
}

int gar_hip_affine_solve_multi(gar_hip_solver *s, int nrhs, const double *rhs_host, double *out_host) {
  GAR_GUARD(s);
  if (int rc = affine_multi_begin(s, nrhs, rhs_host, out_host, "gar_hip_affine_solve_multi"))
    return rc;
  // one chunk of columns at a time through a device staging area of the chunk's size (columns are independent: the
  // results are those of one call on device arrays, bit for bit)
  const size_t n = (size_t)affine_offsets(s, nullptr), cols = (size_t)s->buf.am.panels * GAR_AM_COLS;
  const size_t half = ((size_t)s->batch * cols * n + 1) & ~(size_t)1;
  if (!s->buf.am.staging)
    HIP_TRY(s->buf.am.staging.alloc(2 * half + 2));
  double *in = s->buf.am.staging, *res = in + half;
  for (size_t c0 = 0; c0 < (size_t)nrhs; c0 += cols) {
    const size_t nc = std::min(cols, (size_t)nrhs - c0);
    for (size_t b = 0; b < (size_t)s->batch && n > 0; ++b)
      HIP_TRY(hipMemcpyAsync(in + b * nc * n, rhs_host + (b * (size_t)nrhs + c0) * n, sizeof(double) * nc * n,
                             hipMemcpyHostToDevice, s->stream));
    if (int rc = launch_affine_multi(s, (int)nc, in, res))
      return rc;
    for (size_t b = 0; b < (size_t)s->batch && n > 0; ++b)
      HIP_TRY(hipMemcpyAsync(out_host + (b * (size_t)nrhs + c0) * n, res + b * nc * n, sizeof(double) * nc * n,
                             hipMemcpyDeviceToHost, s->stream));
  }
  HIP_TRY(hipStreamSynchronize(s->stream));
  return failure_epilogue(s, "affine_solve_multi");
}

int gar_hip_get_status(gar_hip_solver *s, int32_t *out) {
  GAR_GUARD(s);
  if (!s || !out)
    return fail(GAR_HIP_ERR_ARG, "gar_hip_get_status: bad argument");
  GAR_MULTI(s, multi_get_status(s, out));
  static_assert(sizeof(int) == sizeof(int32_t), "the status words are 32-bit");
  HIP_TRY(hipMemcpyAsync(out, status_words(s), sizeof(int32_t) * (size_t)s->batch, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  return GAR_HIP_OK;
}

int64_t gar_hip_boundary_doubles(const gar_hip_solver *s) { return s ? s->tuple_doubles : 0; }
double *gar_hip_device_boundary_local(gar_hip_solver *s) { return s ? s->buf.d_bound_local : nullptr; }
double *gar_hip_device_boundary_all(gar_hip_solver *s) { return s ? s->buf.bound_all() : nullptr; }

int gar_hip_set_refinement(gar_hip_solver *s, double thr, int max_steps) {
  if (!s || max_steps < 0)
    return fail(GAR_HIP_ERR_ARG, "bad refinement settings");
  s->cond_threshold = thr;
  s->max_refinement = max_steps;
  GAR_MULTI(s, multi_all(s, [&](gar_hip_solver *q) { return gar_hip_set_refinement(q, thr, max_steps); }));
  return GAR_HIP_OK;
}

int gar_hip_condensed_info(gar_hip_solver *s, int b, double out[2]) {
  GAR_GUARD(s);
  if (int rc = check_bt(s, b, 0))
    return rc;
  GAR_MULTI(s, gar_hip_condensed_info(s->multi->subs[0], b, out)); // (solved redundantly on every device)
  if (s->num_legs < 2 || !out)
    return fail(GAR_HIP_ERR_ARG, "condensed info needs leg mode");
  const double *info = s->buf.d_cscratch + (int64_t)b * s->cscratch_doubles + cond_info_off(s);
  if (int rc = d2h(s, out, info, 2))
    return rc;
  HIP_TRY(hipStreamSynchronize(s->stream));
  return GAR_HIP_OK;
}

static int get_solution_dev(gar_hip_solver *s, int b, double *xs, double *us, double *vs,
                         double *lbdas) {
  const double *base = s->buf.d_sol + (int64_t)b * s->sol_doubles;
  int rc = d2h(s, xs, base + s->sol_x, s->sol_u - s->sol_x);
  rc |= d2h(s, us, base + s->sol_u, s->sol_v - s->sol_u);
  rc |= d2h(s, vs, base + s->sol_v, s->sol_l - s->sol_v);
  int64_t nl = s->nc0;
  for (int t = 0; t < s->horizon; ++t)
    nl += s->meta[t].nx2;
  rc |= d2h(s, lbdas, base + s->sol_l, nl);
  if (rc)
    return rc;
  HIP_TRY(hipStreamSynchronize(s->stream));
  return GAR_HIP_OK;
}

int gar_hip_gains_doubles(const gar_hip_solver *s, int64_t out[2]) {
  if (!s || !out)
    return fail(GAR_HIP_ERR_ARG, "bad argument");
  out[0] = caller_layout(s).ff_all_doubles;
  out[1] = caller_layout(s).fb_all_doubles;
  return GAR_HIP_OK;
}

int gar_hip_gains_offsets(const gar_hip_solver *s, int t, int64_t out[2]) {
  if (int rc = check_bt(s, 0, t))
    return rc;
  const std::vector<long long> &go = caller_layout(s).gain_off;
  out[0] = go[2 * (size_t)t];
  out[1] = go[2 * (size_t)t + 1];
  return GAR_HIP_OK;
}

// [t_lo, t_hi): the stages whose gains are gathered and copied (the whole horizon for a one-device solver; its own
// stages for each device of a multi-device solver, gar_multi.hpp); gains_base: the host buffer [.. | ff_all | fb_all]
// the gains land in (null: the solver's own); sync = false leaves the copies in flight on the solver's stream
static int fetch_results_impl(gar_hip_solver *s, int b, int what, int t_lo, int t_hi, double *gains_base, bool sync) {
  if (int rc = check_bt(s, b, 0))
    return rc;
  // the caller's records (under padding: the real rows / columns only); the device solution record is staged
  // behind them when it has to be stripped on the host
  const gar::HostLayout &u = caller_layout(s);
  const size_t nsol = (size_t)u.sol_doubles, ngain = (size_t)(u.ff_all_doubles + u.fb_all_doubles);
  const size_t nscratch = s->padded ? (size_t)s->sol_doubles : 0;
  if (!s->buf.h_results) { // first use: the buffers live as long as the solver's layout
    // all three or none: a partial failure must not leave h_results set with the device buffers missing
    PinnedBuf<double> h;
    DevBuf<double> dg;
    DevBuf<long long> dgo;
    hipError_t e = h.alloc(nsol + ngain + nscratch, hipHostMallocDefault);
    if (e == hipSuccess)
      e = dg.alloc(std::max<size_t>(ngain, 1));
    if (e == hipSuccess)
      e = dgo.alloc(u.gain_off.size());
    if (e == hipSuccess)
      e = hipMemcpyAsync(dgo, u.gain_off.data(), sizeof(long long) * u.gain_off.size(), hipMemcpyHostToDevice,
                         s->stream);
    if (e != hipSuccess)
      return fail(GAR_HIP_ERR_DEVICE, std::string("gar_hip_fetch_results: ") + hipGetErrorString(e));
    std::memset(h, 0, sizeof(double) * (nsol + ngain + nscratch)); // (alignment padding inside the records reads as zero)
    s->buf.h_results = std::move(h);
    s->buf.d_gains = std::move(dg);
    s->buf.d_gain_off = std::move(dgo);
  }
  if ((what & 2) && s->cur.gains_on_their_way(b) && !gains_base && t_lo == 0 && t_hi == s->horizon + 1) {
    // the gains are already on their way (gar_hip_prefetch_gains): wait for them; what collapseFeedback changed
    // since -- stage 0 -- comes again
    if (int rc = settle_gains_readback(s, kBehindHost))
      return rc;
    if (!s->cur.gains_collapsed)
      what &= ~2;
    else
      t_hi = 1;
  }
  if ((what & 2) && t_hi > t_lo) { // device-side gather (fbT2 -> row-major, dummy rows / columns dropped), then ONE device-to-host copy
    // a read-back started by gar_hip_prefetch_gains (of another problem, or of this one over another range) may
    // still be writing d_gains / h_results on the second stream: this gather and copy reuse both (h_results is host
    // memory: the caller may read it right after)
    if (s->cur.gains_in_flight())
      if (int rc = settle_gains_readback(s, kBehindStream | kBehindHost))
        return rc;
    if (int rc = ensure_expanded(s))
      return rc;
    const bool t2 = records_t2(s, b);
    hipLaunchKernelGGL(gar::gar_gather_gains, dim3((unsigned)(t_hi - t_lo)), dim3(256), 0, s->stream,
                       s->buf.d_meta.get(), s->buf.d_fac + (int64_t)b * s->fac_doubles, s->buf.d_gains.get(),
                       s->buf.d_gains + u.ff_all_doubles, s->buf.d_gain_off.get(), s->horizon, t2 ? 1 : 0,
                       s->dense ? 1 : 0, s->padded ? s->unx : 0, s->padded ? s->unu : 0, t_lo);
    HIP_TRY(hipGetLastError());
    double *hg = (gains_base ? gains_base : s->buf.h_results) + nsol;
    if (t_lo == 0 && t_hi == s->horizon + 1) {
      HIP_TRY(hipMemcpyAsync(hg, s->buf.d_gains, sizeof(double) * ngain, hipMemcpyDeviceToHost, s->stream));
    } else { // the two slices of this stage range
      const std::vector<long long> &go = u.gain_off;
      const long long f0 = go[2 * (size_t)t_lo], f1 = t_hi <= s->horizon ? go[2 * (size_t)t_hi] : u.ff_all_doubles;
      const long long b0 = go[2 * (size_t)t_lo + 1], b1 = t_hi <= s->horizon ? go[2 * (size_t)t_hi + 1] : u.fb_all_doubles;
      if (f1 > f0)
        HIP_TRY(hipMemcpyAsync(hg + f0, s->buf.d_gains + f0, sizeof(double) * (size_t)(f1 - f0), hipMemcpyDeviceToHost, s->stream));
      if (b1 > b0)
        HIP_TRY(hipMemcpyAsync(hg + u.ff_all_doubles + b0, s->buf.d_gains + u.ff_all_doubles + b0,
                               sizeof(double) * (size_t)(b1 - b0), hipMemcpyDeviceToHost, s->stream));
    }
  }
  const bool sol_there = (what & 1) && s->cur.host_solution && b == 0; // copied behind the eager roll-out (gar_hip_backward_blocks)
  if ((what & 1) && !sol_there)
    HIP_TRY(hipMemcpyAsync(s->buf.h_results + (s->padded ? nsol + ngain : 0), s->buf.d_sol + (int64_t)b * s->sol_doubles,
                           sizeof(double) * (size_t)s->sol_doubles, hipMemcpyDeviceToHost, s->stream));
  if (!sync)
    return GAR_HIP_OK;
  if (sol_there && what == 1)
    HIP_TRY(hipEventSynchronize(s->lazy.ev_sol));
  else
    HIP_TRY(hipStreamSynchronize(s->stream));
  if ((what & 1) && s->padded)
    strip_solution_rec(s, s->buf.h_results + nsol + ngain, s->buf.h_results);
  return GAR_HIP_OK;
}

// A read-back of the gains started by prefetch_impl may still be in flight on the second stream: the solver's stream
// (kBehindStream: it is about to rewrite the factor records or d_gains), the host (kBehindHost: it is about to read or
// release h_results) or both are ordered behind it, and the record learns that none is in flight.  The one place that
// waits on LazyState::ev_pref.
namespace {
int settle_gains_readback(gar_hip_solver *s, int behind) {
  if (s->lazy.ev_pref) {
    if (behind & kBehindStream)
      HIP_TRY(hipStreamWaitEvent(s->stream, s->lazy.ev_pref, 0));
    if (behind & kBehindHost)
      HIP_TRY(hipEventSynchronize(s->lazy.ev_pref));
  }
  s->cur.gains_settled();
  return GAR_HIP_OK;
}
} // namespace

// every stage's gains of problem b: gather + ONE device-to-host copy on the second stream, behind what the main
// stream holds now
static int prefetch_impl(gar_hip_solver *s, int b) {
  if (int rc = fetch_results_impl(s, b, 0, 0, 0, nullptr, false)) // the buffers, on first use
    return rc;
  if (!s->lazy.aux_stream) {
    Stream aux;
    Event main, pref;
    HIP_TRY(aux.create(hipStreamNonBlocking));
    HIP_TRY(main.create(hipEventDisableTiming));
    HIP_TRY(pref.create(hipEventDisableTiming));
    s->lazy.aux_stream = std::move(aux);
    s->lazy.ev_main = std::move(main);
    s->lazy.ev_pref = std::move(pref);
  }
  const gar::HostLayout &u = caller_layout(s);
  const size_t nsol = (size_t)u.sol_doubles, ngain = (size_t)(u.ff_all_doubles + u.fb_all_doubles);
  HIP_TRY(hipEventRecord(s->lazy.ev_main, s->stream));
  HIP_TRY(hipStreamWaitEvent(s->lazy.aux_stream, s->lazy.ev_main, 0));
  hipLaunchKernelGGL(gar::gar_gather_gains, dim3((unsigned)(s->horizon + 1)), dim3(256), 0, s->lazy.aux_stream, s->buf.d_meta.get(),
                     s->buf.d_fac + (int64_t)b * s->fac_doubles, s->buf.d_gains.get(), s->buf.d_gains + u.ff_all_doubles, s->buf.d_gain_off.get(),
                     s->horizon, records_t2(s, b) ? 1 : 0, s->dense ? 1 : 0, s->padded ? s->unx : 0,
                     s->padded ? s->unu : 0, 0);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(s->buf.h_results + nsol, s->buf.d_gains, sizeof(double) * ngain, hipMemcpyDeviceToHost, s->lazy.aux_stream));
  HIP_TRY(hipEventRecord(s->lazy.ev_pref, s->lazy.aux_stream));
  s->cur.gains_prefetched(b);
  return GAR_HIP_OK;
}

int gar_hip_fetch_results(gar_hip_solver *s, int b, int what) {
  GAR_GUARD(s);
  if (int rc = check_bt(s, b, 0))
    return rc;
  GAR_MULTI(s, multi_fetch_results(s, b, what));
  return fetch_results_impl(s, b, what, 0, s->horizon + 1, nullptr, true);
}

int gar_hip_prefetch_gains(gar_hip_solver *s, int b) {
  GAR_GUARD(s);
  if (int rc = check_bt(s, b, 0))
    return rc;
  // (multi-device and folded solvers: the ordinary fetch does the work -- their read-back has host-side steps)
  if (s->multi || s->fold)
    return GAR_HIP_OK;
  if (s->cur.host_solution && s->cur.gains_on_their_way(b) && !s->cur.gains_collapsed)
    return GAR_HIP_OK; // gar_hip_backward_blocks started it already
  return prefetch_impl(s, b);
}

const double *gar_hip_host_results(gar_hip_solver *s, int64_t offs[3]) {
  if (!s)
    return nullptr;
  const gar::HostLayout &u = caller_layout(s);
  if (offs) {
    offs[0] = 0;
    offs[1] = u.sol_doubles;
    offs[2] = u.sol_doubles + u.ff_all_doubles;
  }
  if (s->multi)
    return s->multi->h_results;
  return s->buf.h_results;
}

int gar_hip_get_gains_all(gar_hip_solver *s, int b, double *ff_all, double *fb_all) {
  if (int rc = gar_hip_fetch_results(s, b, 2))
    return rc;
  const gar::HostLayout &u = caller_layout(s);
  const double *h = gar_hip_host_results(s, nullptr);
  if (ff_all)
    std::memcpy(ff_all, h + u.sol_doubles, sizeof(double) * (size_t)u.ff_all_doubles);
  if (fb_all)
    std::memcpy(fb_all, h + u.sol_doubles + u.ff_all_doubles,
                sizeof(double) * (size_t)u.fb_all_doubles);
  return GAR_HIP_OK;
}

int gar_hip_debug_trace(gar_hip_solver *s, int enable, long long out[64]) {
  GAR_GUARD(s);
  if (!s)
    return fail(GAR_HIP_ERR_ARG, "null solver");
  GAR_MULTI(s, gar_hip_debug_trace(s->multi->subs[0], enable, out));
  HIP_TRY(hipStreamSynchronize(s->stream));
  if (enable && !s->buf.d_trace) {
    HIP_TRY(s->buf.d_trace.alloc(64));
    HIP_TRY(hipMemset(s->buf.d_trace, 0, sizeof(long long) * 64));
  }
  if (out && s->buf.d_trace)
    HIP_TRY(hipMemcpy(out, s->buf.d_trace, sizeof(long long) * 64, hipMemcpyDeviceToHost));
  if (!enable)
    s->buf.d_trace.reset();
  return GAR_HIP_OK;
}

// (the derivative records speak the CALLER's dimensions: under padding the layout is the caller-facing one, `ulay`)
int64_t gar_hip_deriv_doubles(const gar_hip_solver *s) { return s ? caller_layout(s).deriv_doubles : 0; }

int gar_hip_deriv_offsets(const gar_hip_solver *s, int t, int64_t out[4]) {
  if (int rc = check_bt(s, 0, t))
    return rc;
  const gar::HostLayout &u = caller_layout(s);
  out[0] = u.deriv_off[t];
  out[1] = u.d_G0;
  out[2] = u.d_g0;
  out[3] = u.d_iH;
  return GAR_HIP_OK;
}

int gar_hip_update_lq_subproblem_device(gar_hip_solver *s, const double *deriv_dev, double preg,
                                        int hess_exact) {
  GAR_GUARD(s);
  if (!s || !deriv_dev)
    return fail(GAR_HIP_ERR_ARG, "gar_hip_update_lq_subproblem_device: bad argument");
  GAR_MULTI(s, fail(GAR_HIP_ERR_UNSUPPORTED, "device-resident LQ assembly on a multi-device solver: one derivative buffer per device would be needed"));
  if (int rc = commit(s)) // pending host staging first; later host writes flush only their own ranges
    return rc;
  s->cur.matrices_changed("gar_hip_update_lq_subproblem_device");
  const gar::HostLayout &u = caller_layout(s); // the layout of the derivative buffer: the caller's dimensions
  if (!s->buf.d_deriv_off) {
    HIP_TRY(s->buf.d_deriv_off.alloc(u.deriv_off.size()));
    HIP_TRY(hipMemcpy(s->buf.d_deriv_off, u.deriv_off.data(), sizeof(long long) * u.deriv_off.size(),
                      hipMemcpyHostToDevice));
  }
  gar::UpdateParams U{};
  U.meta = s->buf.d_meta;
  U.deriv = deriv_dev;
  U.prob = s->buf.d_prob;
  U.deriv_stride = u.deriv_doubles;
  U.prob_stride = s->prob_doubles;
  U.G0_off = s->G0_off;
  U.g0_off = s->g0_off;
  U.deriv_off = s->buf.d_deriv_off;
  U.d_G0 = u.d_G0;
  U.d_g0 = u.d_g0;
  U.d_iH = u.d_iH;
  U.horizon = s->horizon;
  U.nc0 = s->nc0;
  U.nx0 = s->nx0;
  U.hess_exact = hess_exact;
  U.preg = preg;
  U.qr_packed = s->qr_packed ? 1 : 0;
  const dim3 grid((unsigned)(s->horizon + 1), (unsigned)s->batch);
  if (s->padded) // the caller's records scattered into the padded knots, dummy rows / columns written (gar_generic.hpp)
    hipLaunchKernelGGL(gar::gar_update_lq_padded, grid, dim3(256), 0, s->stream, U, s->unx, s->unu, s->user_nc0);
  else
    hipLaunchKernelGGL(gar::gar_update_lq, grid, dim3(256), 0, s->stream, U);
  HIP_TRY(hipGetLastError());
  return GAR_HIP_OK;
}

int gar_hip_download_packed(gar_hip_solver *s, int b0, int nb, double *packed) {
  GAR_GUARD(s);
  GAR_MULTI(s, multi_download_packed(s, b0, nb, packed));
  if (!s || !packed || b0 < 0 || nb < 0 || b0 + nb > s->batch)
    return fail(GAR_HIP_ERR_ARG, "gar_hip_download_packed: bad argument");
  if (int rc = commit(s))
    return rc;
  if (!(s->padded || s->qr_packed)) { // the device's records are the caller's
    HIP_TRY(hipMemcpyAsync(packed, s->buf.d_prob + (int64_t)b0 * s->prob_doubles,
                           sizeof(double) * (size_t)s->prob_doubles * nb, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    return GAR_HIP_OK;
  }
  // device records -> the caller's, block by block (gar_record_io.hpp): the real rows / columns, both triangles of Q, R
  const gar::HostLayout &u = caller_layout(s);
  std::vector<double> dev((size_t)s->prob_doubles);
  for (int b = b0; b < b0 + nb; ++b) {
    HIP_TRY(hipMemcpyAsync(dev.data(), s->buf.d_prob + (int64_t)b * s->prob_doubles, sizeof(double) * dev.size(),
                           hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    double *rec = packed + (int64_t)(b - b0) * u.prob_doubles;
    if (s->padded) // (what lies between the blocks: zeros, or what the device holds there)
      std::memset(rec, 0, sizeof(double) * (size_t)u.prob_doubles);
    else
      std::memcpy(rec, dev.data(), sizeof(double) * dev.size());
    BlockMap maps[16];
    init_block_maps(maps, u.nc0, u.nx0, s->nc0, s->nx0, s->G0_off, s->g0_off, u.G0_off, u.g0_off);
    for (int i = 0; i < 2; ++i)
      take_block(rec + maps[i].uoff, maps[i], dev.data());
    for (int t = 0; t <= s->horizon; ++t) {
      const gar_stage_meta &m = u.meta[t], &M = s->meta[t];
      knot_block_maps(maps, m, M, (M.flags & GAR_KNOT_HAS_PARAM) ? M.nth : 0, s->qr_packed && t < s->horizon);
      for (const BlockMap &blk : maps)
        take_block(rec + m.in_off + blk.uoff, blk, dev.data() + M.in_off);
    }
  }
  return GAR_HIP_OK;
}

int gar_hip_set_timing(gar_hip_solver *s, int enable) {
  GAR_GUARD(s);
  if (!s)
    return fail(GAR_HIP_ERR_ARG, "null solver");
  GAR_MULTI(s, multi_all(s, [&](gar_hip_solver *q) { return gar_hip_set_timing(q, enable); }));
  HIP_TRY(hipStreamSynchronize(s->stream));
  if (enable && !s->lazy.ev[0])
    for (Event &e : s->lazy.ev)
      HIP_TRY(e.create());
  s->timing = enable != 0;
  return GAR_HIP_OK;
}

int gar_hip_last_kernel_ms(gar_hip_solver *s, double out[3]) {
  GAR_GUARD(s);
  GAR_MULTI(s, multi_last_kernel_ms(s, out));
  if (!s || !out)
    return fail(GAR_HIP_ERR_ARG, "bad argument");
  if (!s->timing || !(s->mfma_kernel || s->wave_kernel || s->leg_bwd_kernel || s->seg_bwd_kernel))
    return fail(GAR_HIP_ERR_UNSUPPORTED, "per-kernel timing is recorded for the specialised "
                                         "kernel family after gar_hip_set_timing(s, 1)");
  HIP_TRY(hipStreamSynchronize(s->stream));
  float ms = 0.f;
  if (pipe_on(s)) { // per HALF-batch launch, the mean of the two halves; the initial stage rides inside the sweep
    out[0] = out[1] = out[2] = 0.0;
    for (int h = 0; h < 2; ++h) {
      HIP_TRY(hipEventElapsedTime(&ms, s->pipe.evT[h][0], s->pipe.evT[h][1]));
      out[0] += 0.5 * ms;
      HIP_TRY(hipEventElapsedTime(&ms, s->pipe.evT[h][2], s->pipe.evT[h][3]));
      out[2] += 0.5 * ms;
    }
    return GAR_HIP_OK;
  }
  HIP_TRY(hipEventElapsedTime(&ms, s->lazy.ev[0], s->lazy.ev[1]));
  out[0] = ms;
  HIP_TRY(hipEventElapsedTime(&ms, s->lazy.ev[1], s->lazy.ev[2]));
  out[1] = ms;
  HIP_TRY(hipEventElapsedTime(&ms, s->lazy.ev[3], s->lazy.ev[4]));
  out[2] = ms;
  return GAR_HIP_OK;
}

int gar_hip_collapse_feedback(gar_hip_solver *s) {
  GAR_GUARD(s);
  if (!s)
    return fail(GAR_HIP_ERR_ARG, "null solver");
  GAR_MULTI(s, gar_hip_collapse_feedback(s->multi->subs[0])); // stage 0 lives on the first device
  s->cur.feedback_collapsed();
  if (s->num_legs < 2 || s->leg_begin != 0)
    return GAR_HIP_OK; // no-op except Parallel (riccati-base.hpp:33)
  if (s->fold) { // the wave-leg family's own records (then re-expanded on request); flagged problems: generic records
    const int *flags = status_flags(s);
    hipLaunchKernelGGL(s->leg_collapse_kernel, dim3((unsigned)s->batch), dim3(256), 0, s->stream, s->buf.d_meta2.get(), s->buf.d_fac2.get(),
                       (long long)s->flay->fac_doubles, s->batch, flags, 0);
    hipLaunchKernelGGL(gar::gar_collapse_feedback, dim3((unsigned)s->batch), dim3(256), 0, s->stream, s->buf.d_meta.get(), s->buf.d_fac.get(),
                       (long long)s->fac_doubles, s->batch, flags, 1);
    s->cur.expansion_outdated();
  } else {
    hipLaunchKernelGGL(s->leg_collapse_kernel ? s->leg_collapse_kernel : gar::gar_collapse_feedback,
                       dim3((unsigned)s->batch), dim3(256), 0, s->stream, s->buf.d_meta.get(), s->buf.d_fac.get(),
                       (long long)s->fac_doubles, s->batch, (const int *)nullptr, 0);
  }
  HIP_TRY(hipGetLastError());
  return GAR_HIP_OK; // (asynchronous: whoever reads the gains next is ordered behind it on the stream)
}

int gar_hip_cycle_append(gar_hip_solver *s, const int32_t d[5]) {
  GAR_GUARD(s);
  if (!s || !d)
    return fail(GAR_HIP_ERR_ARG, "bad argument");
  GAR_MULTI(s, multi_cycle_append(s, d));
  if (int rc = settle_gains_readback(s, kBehindHost))
    return rc;
  s->cur.solution_superseded();
  s->cur.matrices_changed("gar_hip_cycle_append");
  const int N = s->horizon;
  if (N < 1)
    return GAR_HIP_OK;
  if (int rc = commit(s)) // host writes addressed the old stage numbering: flush them first
    return rc;
  // new dims sequence (the CALLER's dimensions): old[1..N-1], new knot, old[N]  (rotate_vec_left(datas,0,1) +
  // re-created last-but-one factor, proximal-riccati.hxx:79-86)
  const std::vector<int32_t> &od = s->user_dims5;
  std::vector<int32_t> nd(od.size());
  for (int t = 0; t + 1 < N; ++t)
    std::copy(&od[5 * (t + 1)], &od[5 * (t + 1)] + 5, &nd[5 * t]);
  std::copy(d, d + 5, &nd[5 * (N - 1)]);
  std::copy(&od[5 * N], &od[5 * N] + 5, &nd[5 * N]);
  bool uniform = true;
  for (int t = 0; t < N; ++t)
    for (int k = 0; k < 5; ++k)
      uniform &= (nd[5 * t + k] == d[k]) && (od[5 * t + k] == d[k]);
  if (uniform && s->num_legs == 1) {
    // A RING, not a copy: logical stage t (< N) moves to slot (t + ring0) mod N, i.e. every record
    // stays where it is -- problem knots and factors alike (rotate_vec_left(datas, 0, 1)) -- and what
    // was stage 0 becomes the last-but-one slot the caller overwrites next.  The kernels get ring0
    // (specialised families) or the rotated per-stage offsets (generic / dense kernels read them
    // from the stage descriptors): 14 KB of descriptors, asynchronously; no record is touched, the
    // stream is not synchronised.  (Round 1 copied (N-1) x 54 KB per problem and synchronised twice.)
    // (the caller's and the device's dimension sequences are unchanged; a padded solver's dummy rows stay in place)
    s->ring0 = (s->ring0 + 1) % N;
    for (int t = 0; t < N; ++t) {
      const int64_t p = (t + s->ring0) % N;
      s->meta[t].in_off = s->uni_in0 + p * s->uni_in_rec;
      s->meta[t].fac_off = p * s->uni_fac_rec;
    }
    HIP_TRY(hipMemcpyAsync(s->buf.d_meta, s->meta.data(), sizeof(gar_stage_meta) * s->meta.size(),
                           hipMemcpyHostToDevice, s->stream));
    if (s->serial_fold) { // the folded layout turns with the caller's: the family's records stay where they are too
      gar::HostLayout &f = *s->flay;
      f.ring0 = s->ring0;
      for (int t = 0; t < N; ++t) {
        const int64_t p = (t + s->ring0) % N;
        f.meta[t].in_off = f.uni_in0 + p * f.uni_in_rec;
        f.meta[t].fac_off = p * f.uni_fac_rec;
      }
      HIP_TRY(hipMemcpyAsync(s->buf.d_meta2, f.meta.data(), sizeof(gar_stage_meta) * f.meta.size(), hipMemcpyHostToDevice,
                             s->stream));
      HIP_TRY(hipMemset2DAsync(s->buf.d_fac2 + f.meta[N - 1].fac_off, sizeof(double) * (size_t)f.fac_doubles, 0,
                               sizeof(double) * (size_t)f.uni_fac_rec, (size_t)s->batch, s->stream));
      s->cur.expansion_outdated();
    }
    HIP_TRY(hipMemsetAsync(s->buf.d_init, 0, sizeof(double) * (size_t)s->init_doubles * s->batch, s->stream));
    // the last-but-one factor is re-created (zero) like the reference's StageFactor (:84-85): one
    // strided memset over the batch, asynchronous
    HIP_TRY(hipMemset2DAsync(s->buf.d_fac + s->meta[N - 1].fac_off, sizeof(double) * (size_t)s->fac_doubles, 0,
                             sizeof(double) * (size_t)s->uni_fac_rec, (size_t)s->batch, s->stream));
    if (s->padded) { // the slot's dummy diagonals (Q = I, R = I on the padded part) are part of the knot the caller
      // uploads next through gar_hip_upload_stage, which writes whole padded blocks: nothing to do here
    }
    return GAR_HIP_OK;
  }
  // dimensions changed (or leg mode: "just reinitialise everything", parallel-solver.hxx:246-258): rebuild the
  // layout and the buffers.  The new configuration -- padding, layouts, LDS plan, kernel family -- is validated on
  // a TRIAL object first: on failure this solver is untouched (ring position, stage offsets, device records and
  // descriptors included).  On success every device pointer handed out earlier (gar_hip_device_*) is invalid and
  // must be fetched again; resident problem data is not carried over.
  {
    gar_hip_solver trial;
    trial.device = s->device;
    trial.horizon = s->horizon;
    trial.user_nc0 = s->user_nc0;
    trial.batch = s->batch;
    trial.num_legs = s->num_legs;
    trial.rank = s->rank;
    trial.world = s->world;
    trial.dense = s->dense;
    trial.user_dims5 = nd;
    if (int rc = configure(&trial))
      return rc; // g_last_error says why
  }
  HIP_TRY(hipStreamSynchronize(s->stream));
  s->buf = {}; // (every buffer of the old layout, the lazily created ones included)
  s->cur = {}; // (... and nothing of it is current)
  s->user_dims5 = nd;
  // the pipelined schedule belongs to the kernel family that was bound: it is re-validated against the new one (its
  // half streams and events are kept), and silently off when the new shape has no such family
  const int wanted = s->pipe_requested; // 2: the caller's explicit wish; -1: the library's own choice; 0: off
  s->pipe_halves = 0;
  s->pipe.forked = false;
  s->pipe.evB_valid[0] = s->pipe.evB_valid[1] = false;
  if (int rc = configure(s))
    return rc;
  if (int rc = allocate(s))
    return rc;
  if (wanted != 0) { // (kept as the caller's wish even where this shape refuses it: a later rebuild may serve it again)
    if (gar_hip_set_pipeline(s, wanted) != GAR_HIP_OK)
      s->pipe_halves = 0;
    s->pipe_requested = wanted;
  }
  return GAR_HIP_OK;
}


#include "gar_entry_io.hpp"

} // extern "C"
