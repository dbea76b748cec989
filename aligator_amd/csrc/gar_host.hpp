// gar_host.hpp -- what the solver handle (gar_hip.cpp: gar_hip_solver) is made of, apart from its settings: the record
// layout of one problem (HostLayout: build_layout fills it; the caller-facing and the scratch layouts of a solver are
// bare ones), the kernel family bound to it (KernelBinding: select_kernel resets it by value and the bind_* functions of
// gar_select.hpp fill it) and the run state, grouped by lifetime (LayoutState -- with one work-area record per service on a
// resident batch, KktArea ... AffineMultiArea -- PipeState, LazyState) and held in the four move-only owners below, beside
// the one record of what is current (Current).  Included by gar_hip.cpp behind
// <hip/hip_runtime.h>, its standard headers (<atomic>, <cstdlib>, <cstring>, <map>, <mutex>, <string>, <utility>,
// <vector>: none is included here) and the kernel headers; internal linkage, like the rest of that unit's host code.
// Ahead of them: gar_option and its two predicates, which need nothing of a solver.
#pragma once

namespace {
// Behaviour switches (kernel family, padding, condensed solver, ...): `GAR_HIP_*` names, looked up in the overrides
// set through gar_hip_set_option first, in the environment second.  Most are read when a solver is created
// (family selection), some per launch (GAR_HIP_SPD_ACCEPT) -- include/gar_hip.h lists them.
std::mutex &option_mutex() {
  static std::mutex m;
  return m;
}
std::map<std::string, std::string> &option_overrides() {
  static std::map<std::string, std::string> o;
  return o;
}
const char *gar_option(const char *name) {
  // (the value is copied out under the lock into a per-thread slot: a concurrent gar_hip_set_option cannot pull the
  // string from under the caller; eight slots cover every use that holds more than one option at a time)
  thread_local std::string slot[8];
  thread_local unsigned next = 0;
  {
    std::lock_guard<std::mutex> g(option_mutex());
    auto it = option_overrides().find(name);
    if (it != option_overrides().end()) {
      std::string &v = slot[next++ & 7u];
      v = it->second;
      return v.c_str();
    }
  }
  return std::getenv(name);
}
// the two tests most switches are read with: "NAME=0 turns it off" (first character) and "NAME=word"
inline bool option_off(const char *name) { const char *v = gar_option(name); return v && v[0] == '0'; }
inline bool option_is(const char *name, const char *word) {
  const char *v = gar_option(name);
  return v && std::strcmp(v, word) == 0;
}
// ---- owners -----------------------------------------------------------------------------------------------------
// Every device buffer, pinned host buffer, stream and event of the library is held by one of the four owners below:
// move-only, released by reset() or the destructor, read through get() or the implicit conversion to the raw handle.
// Nothing else: no size, no reference count -- a caller that needs the size keeps it (kkt_doubles beside d_kkt).
template <class H, class Arg, hipError_t (*Release)(Arg)> struct Owner {
  Owner() = default;
  Owner(Owner &&o) noexcept : h(std::exchange(o.h, nullptr)) {}
  Owner &operator=(Owner &&o) noexcept {
    if (this != &o) {
      reset();
      h = std::exchange(o.h, nullptr);
    }
    return *this;
  }
  ~Owner() { reset(); }
  void reset() {
    if (h)
      (void)Release(h);
    h = nullptr;
  }
  H get() const { return h; }
  operator H() const { return h; }

protected:
  H h = nullptr;
};

// Every device / pinned-host allocation goes through the two buffer owners and is counted
// (gar_hip_debug_alloc_count): the reference runs backward / forward under ALIGATOR_NOMALLOC_SCOPED
// (gar/proximal-riccati.hxx:35, tests/nomalloc.cpp); tests/test_nomalloc.py asserts the same here -- the count
// does not move across repeated backward + forward calls.
std::atomic<long long> g_alloc_count{0};

template <class T> struct DevBuf : Owner<T *, void *, hipFree> { // n: elements of T
  hipError_t alloc(size_t n) {
    this->reset();
    g_alloc_count.fetch_add(1, std::memory_order_relaxed);
    return hipMalloc((void **)&this->h, sizeof(T) * n);
  }
  hipError_t zalloc(size_t n) {
    const hipError_t e = alloc(n);
    return e != hipSuccess ? e : hipMemset(this->h, 0, sizeof(T) * n);
  }
};
template <class T> struct PinnedBuf : Owner<T *, void *, hipHostFree> {
  hipError_t alloc(size_t n, unsigned flags) {
    this->reset();
    g_alloc_count.fetch_add(1, std::memory_order_relaxed);
    return hipHostMalloc((void **)&this->h, sizeof(T) * n, flags);
  }
};
struct Stream : Owner<hipStream_t, hipStream_t, hipStreamDestroy> {
  hipError_t create(unsigned flags) {
    reset();
    return hipStreamCreateWithFlags(&h, flags);
  }
  hipError_t create_with_priority(unsigned flags, int priority) {
    reset();
    return hipStreamCreateWithPriority(&h, flags, priority);
  }
};
struct Event : Owner<hipEvent_t, hipEvent_t, hipEventDestroy> {
  hipError_t create() { // (with timing)
    reset();
    return hipEventCreate(&h);
  }
  hipError_t create(unsigned flags) {
    reset();
    return hipEventCreateWithFlags(&h, flags);
  }
};
} // namespace

namespace gar {
namespace {

struct HostLayout {
  // ---- in ----
  int horizon = 0, nc0 = 0, num_legs = 1;
  bool dense = false;         // RiccatiSolverDense (gar_dense.hpp): factor records carry nu+nc+2*nx2 gain rows
  std::vector<int32_t> dims5; // dimensions of the DEVICE records (= the caller's unless padded)
  // ---- out (build_layout) ----
  std::vector<gar_stage_meta> meta;
  int64_t prob_doubles = 0, fac_doubles = 0, sol_doubles = 0, init_doubles = 0;
  int64_t G0_off = 0, g0_off = 0;
  int64_t sol_x = 0, sol_u = 0, sol_v = 0, sol_l = 0; // base offsets of xs/us/vs/lbdas
  int nx0 = 0, nth0 = 0, n0 = 0;
  // MPC cycling as a ring (uniform serial problems): logical stage t < horizon lives in record slot
  // (t + ring0) mod horizon; meta[t].in_off / fac_off follow, the records never move
  int ring0 = 0;
  int64_t uni_in0 = 0, uni_in_rec = 0, uni_fac_rec = 0; // slot 0 and the record pitches (layout time)
  // device-resident updateLQSubproblem: layout of one problem's derivative buffer
  std::vector<long long> deriv_off; // per stage
  long long deriv_doubles = 0, d_G0 = 0, d_g0 = 0, d_iH = 0;
  // bulk read-back (gar_hip_fetch_results): per-stage offsets inside ff_all / fb_all
  std::vector<long long> gain_off; // 2 per stage
  long long ff_all_doubles = 0, fb_all_doubles = 0;
};

// The member initialisers are the unbound state ("generic"): a rebuild for other dimensions must not keep launching the
// old shape's kernels over the new records.
struct KernelBinding {
  std::string kernel_name = "generic";
  // specialised backward kernel (gar_mfma.hpp), null = generic
  void (*mfma_kernel)(MfmaParams) = nullptr;
  void (*mfma_fwd_kernel)(MfmaFwdParams) = nullptr;
  size_t mfma_fwd_lds_bytes = 0; // gar_forward_mfma: the packed Vxx' of a stage goes through LDS
  int mfma_lds_doubles = 0;
  // one-wave-per-problem backward kernel (gar_wave.hpp), preferred when bound
  void (*wave_kernel)(MfmaParams, int) = nullptr;
  void (*wave_coupled_kernel)(MfmaParams, int) = nullptr; // constrained sweeps: the second ...
  void (*wave_bk_kernel)(MfmaParams, int) = nullptr;      // ... and the third kernel of the chain
  int wave_lds_doubles = 0, waves_per_block = 1;
  int wave_block_threads = 64; // 128: two waves per problem (gar_wave_pair.hpp)
  bool fb_t2 = false;      // factor records keep fb / fth in the fbT2 device order (gar_mfma.hpp)
  bool vxx_packed = false; // ... and the lower triangle of Vxx, packed (gar_layout.h: the serial one-wave family)
  bool wide_vxx_packed = false; // (set by bind_wide: the serial two-wave family with packed records)
  bool qr_packed = false;  // knots t < N keep Q and R as packed lower triangles (gar_layout.h: the headline sweep)
  bool wave_fused_init = false;
  bool init_closed = true; // closed-form initial stage when G0 = +-I (GAR_HIP_INIT=bk: always factorise)
  // the pipelined sweep's kernels (gar_hip_set_pipeline) belong to the serial one-wave family
  void (*lean_fwd_kernel)(MfmaFwdParams, int) = nullptr;
  void (*wave_half_kernel)(MfmaParams, int) = nullptr; // the backward sweep under its half-batch launch name
  size_t lean_fwd_used = 0;            // LDS the kernel uses
  size_t lean_fwd_lds_bytes = 0;       // what the launch ASKS for (> half a CU: one workgroup per CU), see pipe_plan
  int wave_lds_doubles_small = 0;      // the backward launch without the fused initial stage's kkt0 overlay
  // one-wave-per-(problem, leg) kernels (gar_wave_leg.hpp), bound for uniform leg-mode problems
  void (*leg_bwd_kernel)(LegParams) = nullptr;
  void (*leg_tuple_kernel)(LegParams) = nullptr;
  void (*leg_fwd_kernel)(LegParams) = nullptr;
  void (*leg_collapse_kernel)(const gar_stage_meta *, double *, long long, int, const int *, int) = nullptr;
  int leg_lds_doubles = 0, leg_waves = 1;
  void (*cond_wave_kernel)(CondensedParams) = nullptr;
  int cond_wave_lds_doubles = 0;
  int cond_lds_doubles = 0; // gar_condensed_generic (leg mode: allocate)
  // block cyclic reduction of the condensed system (gar_cyclic.hpp), preferred when bound
  void (*cyc_setup_kernel)(CyclicParams) = nullptr;
  void (*cyc_reduce_kernel)(CyclicParams) = nullptr;
  void (*cyc_top_kernel)(CyclicParams) = nullptr;
  void (*cyc_backlevel_kernel)(CyclicParams) = nullptr;
  void (*cyc_recover_kernel)(CyclicParams) = nullptr;
  int cyc_lds_doubles = 0;
  int cyc_block_doubles = 0; // one NX x NX block of the cyclic-reduction kernels (gar_cyclic_recover's LDS)
  // Segment legs (gar_leg_seg.hpp): leg mode for shapes with a serial stage kernel but no wave-leg family -- the
  // plain part of every leg by that kernel into scratch records (flay: the same knots, nth = 0; d_fac2), the
  // parameter part by the generic matrix recursion, which writes the caller-visible records and the tuples
  void (*seg_bwd_kernel)(MfmaParams, int, int) = nullptr;
  void (*seg_fwd_kernel)(GenericParams) = nullptr; // its roll-out (gar_forward_wide_leg), leg mode
  int seg_lds_doubles = 0;
  // Constrained knots (nc > 0) in leg mode on the unconstrained wave-leg kernels (gar_fold.hpp): problems with D != 0
  // are flagged on the device (status_flags, gar_hip.cpp) and taken by the generic leg kernels ...
  bool fold = false;
  // ... unless the shape has the constrained segment legs (gar_cstr_seg.hpp, round 6): then the flagged problems run
  // on the serial constrained chain's stage kernels, leg by leg, + a parameter recursion; the knots keep Q, R packed
  // (qr_packed), the plain part's records go to the flagged problem's slice of d_fac2, d_cseg_resume holds the chain's
  // hand-over knot per (problem, local leg)
  bool cseg_on = false;
  CsegKernels cseg;
  // The serial twin of `fold` (GAR_HIP_SERIAL_FOLD=1; `fold` is set with it): a serial problem whose constrained knots
  // all have D = 0, on the unconstrained serial family of its (nx, nu).  The family sweeps the folded buffers
  // (flay, d_prob2, d_fac2) in its own record formats, kept in sf_*; the caller-facing buffers (d_prob, d_fac) are in
  // the any-dimension format -- fb_t2 = vxx_packed = qr_packed = false -- which is what the any-dimension serial kernels
  // read and write for the flagged problems and what gar_expand_serial writes for the others.
  bool serial_fold = false;
  bool serial_fold_fallback = false; // the any-dimension kernels fit a CU's LDS: they take the flagged problems
  bool sf_fb_t2 = false, sf_vxx_packed = false, sf_qr_packed = false;
};

// ---- work areas of the services on a resident batch ---------------------------------------------------------------
// One record per service: its device buffers, their record pitches and its kernels' LDS (bytes).  gar_resident.hpp's
// ensure_* build one as a local value and move-assign it whole on the service's first call after the layout was built: a
// work area is there with all its members or not at all (built()), and a failed allocation leaves the solver as it was.
// The one member that comes later is the staging buffer of the service's synchronous form, on ITS first call.
struct KktArea { // gar_hip_kkt_error (gar_kkt.hpp)
  DevBuf<double> stage, err; // the stage norms [batch][horizon + 1][4], the triples [batch][3]
  size_t lds_bytes = 0;      // one workgroup of gar_kkt_stage_residuals
  bool built() const { return stage; }
};
struct AffineArea { // gar_hip_backward_affine (gar_affine.hpp)
  DevBuf<double> W;       // Rhat^-1 [batch][horizon + 1][w_rec] (Current::W_valid)
  DevBuf<int> ok;         // the "re-solved" flags [batch]
  DevBuf<long long> off;  // the offsets of the caller's affine vector [horizon + 2]
  DevBuf<double> staging; // gar_hip_upload_affine: batch vectors
  int w_rec = 0, nx_max = 0;
  size_t sweep_lds_bytes = 0, prep_lds_bytes = 0;
  bool built() const { return off; }
};
struct RefineArea { // gar_hip_refine (gar_refine.hpp)
  DevBuf<double> rhs, out, init; // the right-hand side (the residual vectors), the correction's ff~ / vx~, its initial stage's result
  DevBuf<int> gate;              // the gate words [batch]
  int rhs_rec = 0, out_rec = 0, init_rec = 0;
  long long rhs_stride = 0, out_stride = 0;
  size_t sweep_lds_bytes = 0, roll_lds_bytes = 0, init_lds_bytes = 0;
  bool built() const { return gate; }
};
struct AdjointArea { // gar_hip_adjoint (gar_adjoint.hpp); right-hand side, ff~ / vx~ and the initial stage's result: the refinement's
  DevBuf<double> rec;           // the adjoint records [batch][sol_doubles]
  DevBuf<int> gate;             // the gate words [batch]
  DevBuf<double> staging, grad; // gar_hip_adjoint: cotangents | adjoints; the gradient records on the first call that asks for them
  size_t grad_lds_bytes = 0;
  bool built() const { return gate; }
};
// gar_hip_affine_solve_multi (gar_affine_multi.hpp): the work buffers of ONE CHUNK of `panels` panels of 16 columns per
// problem, sized by the batch, the horizon and the dimensions, never by nrhs
struct AffineMultiArea {
  DevBuf<double> rhs, out;      // the panel records of the right-hand sides and of Kff | Yff | Vx
  DevBuf<double> ivx, ig0, ires; // the initial stage's vx0, g0 and result per (problem, column)
  DevBuf<int> gate;             // the gate words [batch]
  DevBuf<double> staging;       // gar_hip_affine_solve_multi: one chunk of right-hand sides | one chunk of results
  int panels = 0, nu_max = 0, prhs_rec = 0, pout_rec = 0, ivx_rec = 0, ig0_rec = 0, init_rec = 0;
  long long prhs_stride = 0, pout_stride = 0;
  size_t sweep_lds_bytes = 0, roll_lds_bytes = 0, init_lds_bytes = 0;
  bool built() const { return gate; }
};

// ---- run state, by lifetime ---------------------------------------------------------------------------------------
// Layout lifetime: built by allocate() or, member by member (a work area: whole), on an entry point's first use; dropped as one value
// (`s->buf = {}`, behind a stream synchronisation) when gar_hip_cycle_append changes the dimensions, and with the solver.
struct LayoutState {
  DevBuf<gar_stage_meta> d_meta;
  DevBuf<double> d_prob, d_fac, d_sol, d_init, d_theta;
  DevBuf<int> d_status;
  DevBuf<double> d_kkt; // gar_hip_get_kkt's staging ((nu+nc)^2 doubles, allocated on first use)
  int64_t kkt_doubles = 0;
  // `flay`'s device records (gar_hip_solver::flay: the folded problem or the segment legs' scratch records)
  DevBuf<double> d_prob2, d_fac2;
  DevBuf<gar_stage_meta> d_meta2;
  DevBuf<int> d_cseg_resume;
  std::vector<int> h_coupled; // (Current::know_coupled)
  // leg mode: this rank's boundary tuples and, when the legs are sharded over ranks (world > 1), the buffer every
  // rank's tuples are gathered into -- with one rank the local buffer IS the gathered one (bound_all)
  DevBuf<double> d_bound_local, d_bound_gathered, d_csol, d_cscratch;
  double *bound_all() const { return d_bound_gathered ? d_bound_gathered.get() : d_bound_local.get(); }
  // host staging
  PinnedBuf<double> h_prob; // batch * prob_doubles (when small enough)
  bool staged = false, dirty = false;
  bool stage_nt = false; // pack with non-temporal stores (problems of >= 12 MiB; GAR_HIP_STAGE_NT=0/1 overrides)
  // what the host wrote into the staging area since the last flush: per problem, a sorted list of
  // disjoint [lo, hi) ranges (doubles).  commit() copies exactly these, so knots a device-resident
  // producer wrote in place (gar_hip_device_problems) survive a later set_init / upload_stage
  std::vector<std::vector<std::pair<int64_t, int64_t>>> dirty_iv;
  DevBuf<long long> d_trace;     // 64 cycle stamps (debug)
  DevBuf<long long> d_deriv_off; // device-resident updateLQSubproblem: HostLayout::deriv_off on the device
  // bulk read-back (gar_hip_fetch_results): HostLayout::gain_off on the device, the device gather buffer and the
  // pinned host buffer [solution | ff_all | fb_all] of one problem
  DevBuf<long long> d_gain_off;
  DevBuf<double> d_gains;
  PinnedBuf<double> h_results;
  // the caller-side knot offsets [horizon + 1] of a padded solver, on the first call that speaks the caller's packed layout on
  // the device (the upload scatter, the gradient kernel)
  DevBuf<long long> d_user_off;
  // the services on the resident batch, one work area each (above; gar_resident.hpp builds them on first use)
  KktArea kkt;
  AffineArea aff;
  RefineArea ref;
  AdjointArea adj;
  AffineMultiArea am;
};

// Layout lifetime, pure host state: what the device records and their host copies describe RIGHT NOW.  Four results are
// cached -- the factor records, the side buffer W = Rhat^-1 (gar_affine.hpp), the solution in HBM, the pinned host copies
// of the solution and of the gains (h_results) -- and every entry point that reuses one asks here whether it still may.
// The member functions are the transitions, named after the event; none makes a HIP call (the one piece of stream
// ordering that goes with them is settle_gains_readback, gar_hip.cpp).  A layout rebuild assigns the record whole,
// beside `buf = {}`.  DESIGN.md 1b has the table.
struct Current {
  enum Factors { kNone, kOfLastBackward, kStale };
  Factors factors = kNone;           // what gar_hip_backward_affine / gar_hip_refine may re-solve from
  const char *stale_cause = nullptr; // kStale: the entry point that changed matrix blocks
  double mueq = 0.0;                 // of the last backward (the fold, the re-solve's initial stage, the refinement)
  bool W_valid = false;              // AffineArea::W belongs to the factor records
  bool expanded = false;             // folded solvers: the caller-visible factor records are formed ...
  bool know_coupled = false;        // ... and LayoutState::h_coupled holds which problems the generic kernels took
  bool rolled_out = false;           // a roll-out of this factorisation is enqueued: there is a solution to refine
  bool host_solution = false;        // ... and so is its copy into h_results (gar_hip_backward_blocks, no parameter)
  int gains_b = -1;                  // problem whose gains are in flight to / in h_results (gar_hip_prefetch_gains), -1: none
  bool gains_collapsed = false;      // collapseFeedback ran since: stage 0's gains are fetched again

  // ---- transitions ----
  void backward_enqueued(double mu) {
    factors = kOfLastBackward;
    stale_cause = nullptr;
    mueq = mu;
    W_valid = expanded = know_coupled = rolled_out = host_solution = false;
  }
  void matrices_changed(const char *cause) { // (before the first backward there is nothing to make stale)
    if (factors != kNone)
      factors = kStale, stale_cause = cause;
    W_valid = false;
  }
  void W_allocated() { W_valid = false; }
  void W_formed() { W_valid = true; }
  void rollout_enqueued() { rolled_out = true; }
  void host_solution_enqueued() { host_solution = true; }
  void solution_superseded() { host_solution = false; } // rewritten in HBM, or about to be: a fetch copies again
  void gains_prefetched(int b) { gains_b = b, gains_collapsed = false; }
  void gains_settled() { gains_b = -1; } // consumed or discarded
  void feedback_collapsed() { gains_collapsed = true, host_solution = false; } // (a roll-out after it is a new one)
  // folded solvers: the caller-visible factor records are no longer those of the family's own (collapseFeedback on a
  // folded leg solver, a ring turn of a serial-fold solver): formed again on the next request
  void expansion_outdated() { expanded = false; }
  void records_expanded() { expanded = true; }
  void coupled_read() { know_coupled = true; }

  // ---- queries ----
  bool gains_on_their_way(int b) const { return gains_b == b; }
  bool gains_in_flight() const { return gains_b >= 0; }
  // problem b was taken by the generic kernels (D != 0: row-major fb in its records instead of fbT2)
  bool coupled(const std::vector<int> &h_coupled, int b) const { return know_coupled && h_coupled[(size_t)b] != 0; }
  // why `who` cannot re-solve / refine (`verb`) from the factor records; empty: it can
  std::string no_factors(const std::string &who, const char *verb) const {
    if (factors == kOfLastBackward)
      return {};
    if (factors == kStale)
      return who + ": matrix blocks changed since the last backward (" + stale_cause + "): call gar_hip_backward first";
    return who + ": no backward of this solver to " + verb + " from";
  }
};

// Solver lifetime: the pipelined sweep's half streams and events (gar_hip_set_pipeline; the serial one-wave family,
// batch >= 2), created as one group on the first request that is served; they survive a rebuild and die with the solver.
// The batch is cut in two halves with a stream each; backward sweeps alternate between the halves (events), the
// forward sweep of a half is gar_forward_lean, which fits in the registers and the LDS the backward wave of the
// OTHER half leaves free on every SIMD (gar_forward_lean.hpp): B(h0) | F(h0) + B(h1) | F(h1) + B'(h0) | ...
struct PipeState {
  Stream stream[2];
  Event evB[2], evF[2], evFork;
  Event evT[2][4]; // timing
  bool evB_valid[2] = {false, false};
  bool forked = false; // the half streams hold work the caller's stream has not been ordered behind
};

// Solver lifetime: what three entry points create on first use, each group whole or not at all; they survive a rebuild
// and die with the solver.
struct LazyState {
  // gar_hip_prefetch_gains: the bulk read-back of the gains started right behind the backward sweep on a second
  // stream, so that it overlaps the forward sweep and the solution read-back
  Stream aux_stream;
  Event ev_main, ev_pref;
  // gar_hip_backward_blocks on a problem without parameter: the roll-out and the solution's copy are enqueued BEHIND the
  // sweep before the host waits for the status word, so that gar_hip_forward / the solution fetch find them done
  PinnedBuf<int> h_status;
  Event ev_status, ev_sol;
  // gar_hip_set_timing: per-kernel timing of the sweep (bench.py's roofline figure): HIP events recorded on
  // the launch stream around the backward sweep kernel, the initial-stage kernel and the forward
  // sweep kernel of the LAST backward/forward calls
  Event ev[5];
};

} // namespace
} // namespace gar
