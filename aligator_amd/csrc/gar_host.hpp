// gar_host.hpp -- the two parts of the solver handle (gar_hip.cpp: gar_hip_solver derives from both) that are not run
// state: the record layout of one problem (HostLayout: build_layout fills it; the caller-facing and the scratch
// layouts of a solver are bare ones) and the kernel family bound to it (KernelBinding: select_kernel resets it by value
// and the bind_* functions of gar_select.hpp fill it).  Included by gar_hip.cpp behind its standard headers (<cstdlib>,
// <cstring>, <map>, <mutex>, <string>, <vector>: none is included here) and the kernel headers; internal linkage, like
// the rest of that unit's host code.  Ahead of them: gar_option and its two predicates, which need nothing of a solver.
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

} // namespace
} // namespace gar
