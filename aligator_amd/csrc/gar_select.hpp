// gar_select.hpp -- which kernel family serves a problem: the bind_* tables, select_kernel / select_leg_kernel, the padding decision (choose_padding) and configure().
// Part of the ONE translation unit gar_hip.cpp (included in place: it uses the solver struct and the helpers defined
// above its include line); split out for readability only.
#pragma once

// ---- specialised kernel dispatch ---------------------------------------------
template <int NX, int NU> void bind_mfma(gar_hip_solver *s) {
  s->mfma_kernel = gar::gar_backward_mfma<NX, NU>;
  s->mfma_fwd_kernel = gar::gar_forward_mfma<NX, NU>;
  s->mfma_fwd_lds_bytes = sizeof(double) * (size_t)gar_sym_packed_doubles(NX);
  s->fb_t2 = true;
  s->mfma_lds_doubles = gar::MfmaCfg<NX, NU>::total;
  s->kernel_name = "mfma<" + std::to_string(NX) + "," + std::to_string(NU) + ">";
  // Two backward kernels: one wave per problem (throughput: every SIMD runs its own problem) and
  // one 4-wave workgroup per problem (latency: a problem gets a whole CU; measured 2.2 ms vs
  // 3.0 ms per sweep while there are no more problems than CUs).  GAR_HIP_BACKWARD=wave|wg4
  // overrides the choice.
  const char *bw = gar_option("GAR_HIP_BACKWARD"); // (read once: unset, wg4, pair and anything else all matter)
  int cus = 256;
  (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, s->device);
  const bool want_wave = bw ? std::strcmp(bw, "wg4") != 0 : s->batch > cus;
  // GAR_HIP_BACKWARD=pair: two waves per problem, the tile columns split between them
  // (gar_wave_pair.hpp; <= 256 registers per wave, so two waves share a SIMD)
  constexpr bool can_pair = (NX % 16) != 0 && ((NX >> 4) >= (gar::WaveCfg<NX, NU>::TW / 2)) && (gar::WaveCfg<NX, NU>::TW / 2) >= 1;
  if (bw && std::strcmp(bw, "pair") == 0 && can_pair) {
    if constexpr (can_pair) {
      s->wave_kernel = gar::gar_backward_pair<NX, NU>;
      s->wave_fused_init = false;
      s->wave_lds_doubles = gar::PairCfg<NX, NU>::total;
      s->wave_block_threads = 128;
      s->waves_per_block = 1;
      s->kernel_name = "pair<" + std::to_string(NX) + "," + std::to_string(NU) + ">";
    }
  } else if (want_wave) {
    s->wave_kernel = gar::gar_backward_wave<NX, NU>;
    // the initial stage is fused into the sweep when its packed kkt0 fits beside V in a
    // quarter of the CU's LDS (four waves per CU)
    const int with_init = gar::WaveCfg<NX, NU>::total_with_init(s->nc0);
    s->wave_fused_init = (size_t)with_init * sizeof(double) <= 40 * 1024 && s->nth0 == 0;
    const int sweep = gar::WaveCfg<NX, NU>::total;
    s->wave_lds_doubles = s->wave_fused_init ? std::max(with_init, sweep) : sweep;
    s->waves_per_block = 1; // one 64-thread workgroup per problem (constant LDS base)
    s->kernel_name = "wave<" + std::to_string(NX) + "," + std::to_string(NU) + ">";
    s->qr_packed = true; // the sweep reads only the lower triangles of Q and R (gar_layout.h)
    // the pipelined sweep's roll-out (gar_hip_set_pipeline): reads the packed Vxx records
    s->lean_fwd_kernel = gar::gar_forward_lean<NX, NU>;
    s->wave_half_kernel = gar::gar_backward_wave_half<NX, NU>;
    s->lean_fwd_used = gar::LeanFwdCfg<NX, NU>::USED; // (what it uses; pipe_plan decides what it asks for)
    s->wave_lds_doubles_small = sweep;
  }
}

// Wide shapes (nx + nu > 64, e.g. the Talos walk's (56, 22) padded to (56, 24)): the one-wave-per-problem
// backward sweep only (gar_wave2.hpp; fb ROW-major = the generic record layout), the initial stage
// and the forward sweep on the generic kernels.
template <int NX, int NU> void bind_wide(gar_hip_solver *s) {
  // two waves per problem (the tile columns split between them) unless GAR_HIP_WIDE=single
  const bool pair = !option_is("GAR_HIP_WIDE", "single");
  const bool generic_fwd = option_is("GAR_HIP_WIDE", "generic-forward");
  if (!generic_fwd)
    s->mfma_fwd_kernel = gar::gar_forward_wide<NX, NU>; // row-major fb: fb_t2 stays false
  s->wave_fused_init = false;
  s->waves_per_block = 1;
  s->fb_t2 = false;
  if (pair) {
    // packed records (gar_wave_pair.hpp): lower triangles of Q, R in the knots, of Vxx in the factors
    // -- with the roll-out that reads them (the any-dimension roll-out reads the flag from its parameters)
    // (the any-dimension roll-out reads full Vxx blocks: GAR_HIP_WIDE=generic-forward keeps the full records)
    constexpr bool PKD = NX % 4 == 0;
    if (PKD && !generic_fwd) {
      s->wave_kernel = gar::gar_backward_pair<NX, NU, PKD>;
      s->qr_packed = true;
      s->wide_vxx_packed = true;
      s->mfma_fwd_kernel = gar::gar_forward_wide<NX, NU, true>;
      s->mfma_fwd_lds_bytes = sizeof(double) * (size_t)gar_sym_packed_doubles(NX);
    } else {
      s->wave_kernel = gar::gar_backward_pair<NX, NU, false>;
    }
    s->wave_lds_doubles = gar::PairCfg<NX, NU>::total;
    s->wave_block_threads = 128;
    s->kernel_name = "pair<" + std::to_string(NX) + "," + std::to_string(NU) + ">";
  } else {
    s->wave_kernel = gar::gar_backward_wave<NX, NU>;
    s->wave_lds_doubles = gar::WaveCfg<NX, NU>::total;
    s->kernel_name = "wave<" + std::to_string(NX) + "," + std::to_string(NU) + ">";
  }
}

template <int NX, int NU> void bind_leg(gar_hip_solver *s) {
  s->fb_t2 = true;
  // two waves per leg (plain part / parameter part) unless GAR_HIP_LEG_WAVES=1
  s->leg_waves = option_is("GAR_HIP_LEG_WAVES", "1") ? 1 : 2;
  s->leg_bwd_kernel = s->leg_waves == 2 ? gar::gar_backward_wave_leg2<NX, NU> : gar::gar_backward_wave_leg<NX, NU>;
  s->leg_tuple_kernel = gar::gar_leg_tuples<NX, NU>;
  s->leg_fwd_kernel = gar::gar_forward_wave_leg<NX, NU>;
  s->leg_collapse_kernel = gar::gar_collapse_feedback_t2<NX, NU>;
  s->leg_lds_doubles = s->leg_waves == 2 ? gar::WaveCfg<NX, NU>::leg2_total : gar::WaveCfg<NX, NU>::leg_total;
  if (!option_is("GAR_HIP_CONDENSED", "generic")) {
    const int lds = 4 * NX * NX + 16 * NX + NX + NX + (NX & 1) + (NX + 16) / 2 + 2 +
                    2 * (2 * s->num_legs) * NX + 2;
    if ((size_t)lds * sizeof(double) <= 160 * 1024) {
      s->cond_wave_kernel = gar::gar_condensed_wave<NX>;
      s->cond_wave_lds_doubles = lds;
    }
    if (!option_is("GAR_HIP_CONDENSED", "chain")) {
      s->cyc_setup_kernel = gar::gar_cyclic_setup<NX>;
      s->cyc_reduce_kernel = gar::gar_cyclic_reduce<NX>;
      s->cyc_top_kernel = gar::gar_cyclic_top<NX>;
      s->cyc_backlevel_kernel = gar::gar_cyclic_backlevel<NX>;
      s->cyc_recover_kernel = gar::gar_cyclic_recover<NX>;
      s->cyc_lds_doubles = gar::CyclicLds<NX>::total;
      s->cyc_block_doubles = NX * NX;
    }
  }
  s->kernel_name = "wave_leg<" + std::to_string(NX) + "," + std::to_string(NU) + ">";
}

// the wide shape in leg mode: segment legs (gar_leg_seg.hpp) on the two-wave stage kernel -- unconstrained problems
// (the fold serves the wave-leg family alone) whose parameter stage fits a CU's LDS; GAR_HIP_SEG_LEGS=0: off
template <int NX, int NU> void bind_seg_leg(gar_hip_solver *s) {
  for (int t = 0; t <= s->horizon; ++t)
    if (s->dims5[5 * (size_t)t + 2] != 0)
      return;
  if (option_off("GAR_HIP_SEG_LEGS") || (size_t)gar::leg_stage_lds_doubles(NX, NU) * sizeof(double) > 160 * 1024)
    return;
  s->seg_bwd_kernel = gar::gar_backward_pair_leg<NX, NU>;
  s->seg_fwd_kernel = gar::gar_forward_wide_leg<NX, NU>;
  s->seg_lds_doubles = gar::PairCfg<NX, NU>::total;
  s->fb_t2 = false; // row-major fb: the generic roll-out, condensed solve and collapse serve the family
  s->kernel_name = "pair_leg<" + std::to_string(NX) + "," + std::to_string(NU) + ">";
}

// uniform problems with NC constraints on every knot: the one-wave-per-problem kernels with the
// reduced KKT system factorised by the wave-scope Bunch-Kaufman (gar_wave.hpp, NC > 0)
template <int NX, int NU, int NC> void bind_cstr(gar_hip_solver *s) {
  s->wave_kernel = gar::gar_backward_wave<NX, NU, NC>;
  s->wave_coupled_kernel = gar::gar_backward_wave_coupled<NX, NU, NC>;
  s->wave_bk_kernel = gar::gar_backward_wave_bk<NX, NU, NC>;
  s->mfma_fwd_kernel = gar::gar_forward_mfma<NX, NU, NC>;
  s->mfma_fwd_lds_bytes = sizeof(double) * (size_t)gar_sym_packed_doubles(NX);
  s->fb_t2 = true;
  const int with_init = gar::WaveCfg<NX, NU, NC>::total_with_init(s->nc0);
  s->wave_fused_init = (size_t)with_init * sizeof(double) <= 64 * 1024 && s->nth0 == 0;
  s->wave_lds_doubles = s->wave_fused_init ? with_init : gar::WaveCfg<NX, NU, NC>::total;
  s->waves_per_block = 1;
  s->kernel_name = "wave<" + std::to_string(NX) + "," + std::to_string(NU) + "," + std::to_string(NC) + ">";
  s->qr_packed = true; // the chain's three kernels read only the lower triangles of Q and R (gar_layout.h)
}

// The (nx, nu) shapes with kernels of their own, and what binds them serial in time and in leg mode: select_kernel,
// select_leg_kernel and choose_padding (which pads onto the cheapest row that holds the caller's shape) all read
// kSpecialised.  (The constrained segment legs are instantiated in a translation unit of their own and keep the list
// of their shapes there: gar::cseg_bind, gar_cstr_seg.cpp.)
using BindFn = void (*)(gar_hip_solver *);
struct SpecShape { int nx, nu; BindFn bind_serial, bind_leg; };
struct CstrShape { int nx, nu, nc; BindFn bind; };
#define GAR_WAVE_SHAPES(X) X(36, 12) X(32, 12) X(16, 8) X(12, 8) X(12, 4) X(8, 4)
#define GAR_LEG_BINDER(NX, NU) bind_leg<NX, NU>,
#define GAR_SHAPE_ROW(NX, NU) {NX, NU, bind_mfma<NX, NU>, bind_leg<NX, NU>},
// (the compiler emits the kernels in the order their binders are first named: the leg families, the constrained ones
// below, then the serial ones -- this line names the first group ahead of the table's rows and so keeps the code object
// what it was when two if-chains named them)
[[maybe_unused]] constexpr BindFn kLegBindersFirst[] = {GAR_WAVE_SHAPES(GAR_LEG_BINDER) bind_seg_leg<56, 24>};
// the shapes with nc constraints on every knot, serial in time (the reference's bench/gar-riccati.cpp shape)
constexpr CstrShape kConstrained[] = {{36, 12, 32, bind_cstr<36, 12, 32>}, {16, 8, 8, bind_cstr<16, 8, 8>}, {8, 4, 4, bind_cstr<8, 4, 4>}};
constexpr SpecShape kSpecialised[] = {GAR_WAVE_SHAPES(GAR_SHAPE_ROW){56, 24, bind_wide<56, 24>, bind_seg_leg<56, 24>}};
#undef GAR_WAVE_SHAPES
#undef GAR_LEG_BINDER
#undef GAR_SHAPE_ROW

// leg mode: uniform unconstrained problem whose every leg holds at least two knots
void select_leg_kernel(gar_hip_solver *s) {
  const int N = s->horizon;
  if (option_is("GAR_HIP_LEGS", "generic"))
    return;
  if (N < 1 || s->nxb != s->dims5[0])
    return;
  const int nx = s->dims5[0], nu = s->dims5[1];
  bool any_nc = false;
  for (int t = 0; t <= N; ++t) {
    const int32_t *d = &s->dims5[5 * t];
    if (d[0] != nx || d[1] != (t < N ? nu : 0) || d[3] != nx || d[4] != 0)
      return;
    any_nc |= d[2] != 0;
  }
  // constrained knots: folded onto the unconstrained family (gar_fold.hpp); the generic leg kernels are the
  // fallback for problems with D != 0, so they must fit a CU's LDS
  if (any_nc && (!s->lds_error.empty() || option_off("GAR_HIP_FOLD")))
    return;
  for (int i = 0; i < s->num_legs; ++i) {
    int i0, i1;
    gar_get_work(N, i, s->num_legs, &i0, &i1);
    if (i1 - i0 < (i + 1 < s->num_legs ? 2 : 1))
      return;
  }
  for (const SpecShape &sh : kSpecialised)
    if (sh.nx == nx && sh.nu == nu)
      sh.bind_leg(s);
  s->fold = any_nc && s->leg_bwd_kernel != nullptr;
}

// GAR_HIP_SERIAL_FOLD=1: a serial problem of an exact kSpecialised shape with constraints on some (or all) knots, on
// that shape's unconstrained serial family through the fold (gar_fold.hpp) -- the serial twin of select_leg_kernel's
// `fold`.  The uniform kConstrained rows keep their own chain.  The fold kernel stages C and C / mu in its default
// dynamic LDS.  The any-dimension kernels are the fallback for problems with D != 0; where they do not fit a CU's LDS
// ((56, 24) with constraints: no solver at all without the switch) there is none, and such a problem is reported as a
// failed stage (serial_fold_fallback, backward_serial).
bool select_serial_fold(gar_hip_solver *s) {
  const int N = s->horizon;
  if (!option_is("GAR_HIP_SERIAL_FOLD", "1") || s->world != 1 || s->padded)
    return false;
  const int nx = s->meta[0].nx, nu = s->meta[0].nu;
  int nc_max = 0;
  bool uniform_nc = true;
  for (int t = 0; t <= N; ++t) {
    const gar_stage_meta &m = s->meta[t];
    if (m.nx != nx || m.nu != (t < N ? nu : 0) || m.nx2 != nx || m.nth != 0)
      return false;
    nc_max = std::max(nc_max, (int)m.nc);
    uniform_nc &= m.nc == s->meta[0].nc;
  }
  if (nc_max == 0 || sizeof(double) * (size_t)gar::fold_lds_doubles(nx, nc_max) > 48 * 1024)
    return false;
  if (!s->lds_error.empty() && s->n0 > 128) // (the stand-alone initial stage beyond one wave is the any-dimension kernels')
    return false;
  if (uniform_nc)
    for (const CstrShape &sh : kConstrained)
      if (sh.nx == nx && sh.nu == nu && sh.nc == nc_max)
        return false;
  for (const SpecShape &sh : kSpecialised)
    if (sh.nx == nx && sh.nu == nu)
      sh.bind_serial(s);
  if (!(s->wave_kernel || s->mfma_kernel) || !s->mfma_fwd_kernel) { // (GAR_HIP_WIDE=generic-forward: no roll-out of the family's)
    static_cast<gar::KernelBinding &>(*s) = gar::KernelBinding{};
    s->init_closed = !option_is("GAR_HIP_INIT", "bk");
    return false;
  }
  s->sf_fb_t2 = s->fb_t2;
  s->sf_vxx_packed = s->fb_t2 || s->wide_vxx_packed;
  s->sf_qr_packed = s->qr_packed;
  s->fb_t2 = s->vxx_packed = s->qr_packed = false; // the caller-facing records: the any-dimension format
  s->lean_fwd_kernel = nullptr;                     // the pipelined schedule is not offered (pipe_eligible)
  s->wave_half_kernel = nullptr;
  s->fold = s->serial_fold = true;
  s->serial_fold_fallback = s->lds_error.empty();
  return true;
}

void select_kernel(gar_hip_solver *s) {
  static_cast<gar::KernelBinding &>(*s) = gar::KernelBinding{}; // nothing of the family bound before survives
  s->init_closed = !option_is("GAR_HIP_INIT", "bk");
  if (s->dense) {
    s->kernel_name = "dense";
    return;
  }
  const char *force = gar_option("GAR_HIP_FORCE_GENERIC");
  if (force && force[0] == '1')
    return;
  const int N = s->horizon;
  if (s->num_legs > 1) {
    select_leg_kernel(s);
    return;
  }
  if (N < 1)
    return;
  if (!s->multi && select_serial_fold(s))
    return;
  const gar_stage_meta &m0 = s->meta[0];
  if (m0.nth != 0 || m0.nx2 != m0.nx)
    return;
  for (int t = 1; t < N; ++t) {
    const gar_stage_meta &m = s->meta[t];
    if (m.nx != m0.nx || m.nu != m0.nu || m.nc != m0.nc || m.nth != 0 || m.nx2 != m0.nx ||
        m.in_off - s->meta[t - 1].in_off != s->meta[1 < N ? 1 : 0].in_off - m0.in_off)
      return;
  }
  // (the terminal knot's factor record is addressed through compile-time offsets that assume nx2 = nx rows of
  // [yff | Aff] in it; the nx2 = 0 terminal knot SolverProxDDP builds arrives here normalised to nx2 = nx --
  // normalise_terminal -- anything else is the any-dimension kernels')
  const gar_stage_meta &mt = s->meta[N];
  if (mt.nx != m0.nx || mt.nu != 0 || mt.nc != m0.nc || mt.nth != 0 || mt.nx2 != m0.nx)
    return;
  const int nx = m0.nx, nu = m0.nu;
  if (m0.nc != 0) { // every knot constrained (the reference's bench/gar-riccati.cpp shape)
    for (const CstrShape &sh : kConstrained)
      if (sh.nx == nx && sh.nu == nu && sh.nc == m0.nc)
        sh.bind(s);
    s->vxx_packed = s->fb_t2; // (serial one-wave family: gar_layout.h)
    return;
  }
  for (const SpecShape &sh : kSpecialised)
    if (sh.nx == nx && sh.nu == nu)
      sh.bind_serial(s);
  // the serial one-wave family keeps the lower triangle of Vxx, packed (gar_layout.h); round 6: the two-wave wide family too
  s->vxx_packed = s->fb_t2 || s->wide_vxx_packed;
}

// Decide the device dimensions from the caller's (see gar_hip_solver::padded).  GAR_HIP_PAD=0: never pad.
void choose_padding(gar_hip_solver *s) {
  s->dims5 = s->user_dims5;
  s->nc0 = s->user_nc0;
  s->padded = false;
  s->unx = s->unu = s->pnx = s->pnu = 0;
  const int N = s->horizon;
  if (s->dense || option_off("GAR_HIP_PAD") || N < 1)
    return;
  const int32_t *d0 = &s->user_dims5[0];
  const int nx = d0[0], nu = d0[1];
  if (nu == 0 || nx <= 0)
    return;
  for (int t = 0; t <= N; ++t) {
    const int32_t *d = &s->user_dims5[5 * t];
    if (d[0] != nx || d[1] != (t < N ? nu : 0) || d[2] != 0 || d[3] != nx || d[4] != 0)
      return;
  }
  long best = -1;
  int bx = 0, bu = 0;
  for (const SpecShape &sh : kSpecialised) {
    if (sh.nx == nx && sh.nu == nu)
      return; // the shape has its own kernels
    if (sh.nx >= nx && sh.nu >= nu) {
      const long cost = (long)sh.nx * (sh.nx + sh.nu);
      if (best < 0 || cost < best)
        best = cost, bx = sh.nx, bu = sh.nu;
    }
  }
  if (best < 0)
    return;
  s->padded = true;
  s->unx = nx;
  s->unu = nu;
  s->pnx = bx;
  s->pnu = bu;
  for (int t = 0; t <= N; ++t) {
    int32_t *d = &s->dims5[5 * t];
    d[0] = d[3] = bx;
    if (t < N)
      d[1] = bu;
  }
  s->nc0 = s->user_nc0 + (bx - nx); // the dummy states are pinned by extra rows of the initial constraint
}

int configure_padded_or_not(gar_hip_solver *s);

// Everything that can be decided and validated WITHOUT touching device memory: padding, both layouts, the LDS
// plan, leg-mode geometry, the kernel family.  create and cycle_append (on a trial object) share it.
int configure(gar_hip_solver *s) {
  choose_padding(s);
  for (;;) {
    const int rc = configure_padded_or_not(s);
    // Padded onto a specialised shape, but no kernel of that family binds (leg mode with a leg of fewer than two
    // knots, GAR_HIP_SEG_LEGS=0, parameter LDS beyond a CU, ...): the any-dimension kernels would then sweep the
    // PADDED shape -- several times the work and LDS of the caller's own, possibly beyond what fits.  Redo the
    // configuration on the caller's dimensions.
    if (s->padded && (rc != GAR_HIP_OK || !(s->wave_kernel || s->mfma_kernel || s->leg_bwd_kernel || s->seg_bwd_kernel))) {
      s->dims5 = s->user_dims5;
      s->nc0 = s->user_nc0;
      s->padded = false;
      s->unx = s->unu = s->pnx = s->pnu = 0;
      continue;
    }
    return rc;
  }
}

// A second layout of `src`'s problem: its inputs with one of them changed by `tweak`, laid out
template <class Tweak> int derive_layout(std::unique_ptr<gar::HostLayout> &out, const gar::HostLayout &src, Tweak tweak) {
  out = std::make_unique<gar::HostLayout>();
  out->horizon = src.horizon;
  out->nc0 = src.nc0;
  out->num_legs = src.num_legs;
  out->dense = src.dense;
  out->dims5 = src.dims5;
  tweak(*out);
  return build_layout(*out);
}

int configure_padded_or_not(gar_hip_solver *s) {
  if (int rc = build_layout(*s))
    return rc;
  if (int rc = plan_lds(s))
    return rc;
  s->ulay.reset();
  if (s->padded) // the caller-facing records: the caller's dimensions
    if (int rc = derive_layout(s->ulay, *s, [s](gar::HostLayout &u) { u.nc0 = s->user_nc0; u.dims5 = s->user_dims5; }))
      return rc;
  if (s->num_legs > 1) {
    const int J = s->num_legs, W = s->world;
    if (W < 1 || W > J || s->rank < 0 || s->rank >= W)
      return fail(GAR_HIP_ERR_ARG, "horizon sharding needs 1 <= ranks <= num_legs");
    s->leg_begin = (int)((long long)s->rank * J / W);
    s->leg_end = (int)((long long)(s->rank + 1) * J / W);
    s->legs_per_rank = (J + W - 1) / W; // chunk pitch of the gathered tuples (gar_generic.hpp, cond_tuple)
    int nxb = 0;
    for (const auto &m : s->meta)
      nxb = std::max(nxb, std::max(m.nx, m.nx2));
    if (s->nc0 > nxb)
      return fail(GAR_HIP_ERR_UNSUPPORTED, "leg mode needs nc0 <= nx");
    s->nxb = nxb;
    s->tuple_doubles = 3 * (int64_t)nxb * nxb + 2 * nxb;
  }
  select_kernel(s);
  if (!s->lds_error.empty() && !(s->wave_kernel || s->mfma_kernel || s->leg_bwd_kernel || s->seg_bwd_kernel))
    return fail(GAR_HIP_ERR_UNSUPPORTED, s->lds_error);
  s->flay.reset();
  if (s->seg_bwd_kernel) // scratch records of the plain kernels: the same knots, serial (nth = 0) layout
    if (int rc = derive_layout(s->flay, *s, [](gar::HostLayout &f) { f.num_legs = 1; }))
      return rc;
  if (s->fold) { // the folded problem: the same knots without their constraints
    auto unconstrained = [](gar::HostLayout &f) {
      for (int t = 0; t <= f.horizon; ++t)
        f.dims5[5 * (size_t)t + 2] = 0;
    };
    if (int rc = derive_layout(s->flay, *s, unconstrained))
      return rc;
    s->kernel_name += "+fold";
    // problems with D != 0: the constrained segment legs (gar_cstr_seg.hpp) where every knot carries the same number of
    // constraints and the shape has the serial constrained chain; their scratch records live in the flagged problem's
    // slice of the wave-leg family's factor buffer
    const int nx = s->dims5[0], nu = s->dims5[1], nc = s->dims5[2];
    bool uniform_nc = nc > 0;
    for (int t = 0; t <= s->horizon; ++t)
      uniform_nc &= s->dims5[5 * (size_t)t + 2] == nc;
    if (uniform_nc && !s->serial_fold && !option_off("GAR_HIP_CSTR_SEG_LEGS") && gar::cseg_bind(nx, nu, nc, &s->cseg) &&
        s->cseg.scratch_doubles(s->horizon, s->num_legs) <= s->flay->fac_doubles) {
      s->cseg_on = true;
      s->qr_packed = true; // the chain's kernels read only the lower triangles of Q and R (gar_layout.h); the fold unpacks
      s->kernel_name += "|wave_seg<" + std::to_string(nx) + "," + std::to_string(nu) + "," + std::to_string(nc) + ">";
    }
  }
  // (see gar_hip_backward_legs_async)
  s->mu_divides = s->cseg_on;
  s->any_nc = false;
  for (int t = 0; t <= s->horizon; ++t) {
    const int32_t *d = &s->dims5[5 * (size_t)t];
    // (a serial-fold solver divides like a leg-fold one: on the terminal knot outright, elsewhere on the fold's say-so)
    s->mu_divides |= d[2] > 0 && (d[1] == 0 || (s->wave_kernel != nullptr && !s->serial_fold));
    s->any_nc |= d[2] > 0;
  }
  return GAR_HIP_OK;
}

