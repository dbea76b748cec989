// gar_launch.hpp -- kernel parameter blocks (one make_* each) and launches of the sweeps, one function per kernel family:
// launch_backward, launch_forward, the pipelined schedule (gar_pipeline.hpp), launch_condensed.
// Part of the ONE translation unit gar_hip.cpp (included in place: it uses the solver struct and the helpers defined
// above its include line); split out for readability only.
#pragma once

// the timing API's event i (gar_hip_set_timing) on the launch stream; nothing unless timing is on (and `when`)
inline hipError_t stamp(gar_hip_solver *s, int i, bool when = true) {
  return s->timing && when ? hipEventRecord(s->lazy.ev[i], s->stream) : hipSuccess;
}

// MfmaParams of a stage sweep over the caller's knots: mfma_common + where the factor records go, mueq and the
// per-launch GAR_HIP_SPD_ACCEPT.  Called as it is, this is the scratch-record form of the segment legs and the constrained
// segment legs (fac = d_fac2): trace, init, init_stride, G0_off, g0_off, nc0, init_closed and ring0 stay ZERO there on
// purpose -- a leg has no fused initial stage, no ring and no trace.  make_mfma_params adds them for the serial sweeps.
gar::MfmaParams make_mfma_scratch_params(gar_hip_solver *s, double mueq, double *fac, long long fac_stride,
                                         long long fac_rec, long long fac_offN, int *resume) {
  gar::MfmaParams M = mfma_common(s, *s, s->buf.d_prob, fac, fac_stride);
  M.resume = resume;
  M.fac_rec = fac_rec;
  M.fac_offN = fac_offN;
  M.mueq = mueq;
  M.spd_accept = option_off("GAR_HIP_SPD_ACCEPT") ? 0 : 1;
  return M;
}
// parameters of the serial specialised sweeps (gar_backward_mfma, gar_backward_wave and its chain)
gar::MfmaParams make_mfma_params(gar_hip_solver *s, double mueq) {
  // (a serial-fold solver: the family sweeps the folded knots into its own records; the flags belong to the fold)
  const gar::HostLayout &L = s->serial_fold ? *s->flay : static_cast<const gar::HostLayout &>(*s);
  gar::MfmaParams M = make_mfma_scratch_params(s, mueq, s->serial_fold ? s->buf.d_fac2 : s->buf.d_fac, L.fac_doubles, L.uni_fac_rec,
                                               L.meta[s->horizon].fac_off, s->serial_fold ? nullptr : status_flags(s));
  if (s->serial_fold) {
    M.prob = s->buf.d_prob2;
    M.prob_stride = L.prob_doubles;
    M.in_off0 = L.uni_in0;
    M.in_rec = L.uni_in_rec;
    M.in_offN = L.meta[s->horizon].in_off;
  }
  M.trace = s->buf.d_trace;
  M.init = s->wave_kernel && s->wave_fused_init ? s->buf.d_init : nullptr;
  M.init_stride = s->init_doubles;
  M.G0_off = s->G0_off;
  M.g0_off = s->g0_off;
  M.nc0 = s->nc0;
  M.init_closed = s->init_closed ? 1 : 0;
  M.ring0 = s->ring0;
  return M;
}

// [l0, l1): the legs swept by a call.  Every caller sweeps all legs of this solver today (sweeping them in chunks as
// their knots arrive was measured and not kept, see gar_hip_backward_blocks).  The kernels index legs as blockIdx.x +
// leg_begin and the tuples as blockIdx.x: a chunk is the same launch with leg_begin = l0 and the tuple buffer advanced
// to leg l0's slot (tup_shift).
struct LegChunk {
  int l0, l1;
  bool first, last; // the chunk holds the solver's first / last leg: the timing events bracket the whole sweep
  long long tup_shift;
  dim3 grid(const gar_hip_solver *s) const { return dim3((unsigned)(l1 - l0), (unsigned)s->batch); }
};

// the parameter recursion of the segment legs and of the constrained segment legs (which set `only`)
gar::LegParamParams make_leg_param_params(gar_hip_solver *s, const LegChunk &c) {
  gar::LegParamParams Q{};
  Q.meta = s->buf.d_meta;
  Q.meta2 = s->buf.d_meta2;
  Q.prob = s->buf.d_prob;
  Q.fac2 = s->buf.d_fac2;
  Q.fac = s->buf.d_fac;
  Q.boundary = s->buf.d_bound_local + c.tup_shift;
  Q.status = s->buf.d_status;
  Q.prob_stride = s->prob_doubles;
  Q.fac_stride = s->fac_doubles;
  Q.fac2_stride = s->flay->fac_doubles;
  Q.boundary_stride = (long long)s->legs_per_rank * s->tuple_doubles;
  Q.horizon = s->horizon;
  Q.num_legs = s->num_legs;
  Q.leg_begin = c.l0;
  Q.tuple_doubles = (int)s->tuple_doubles;
  Q.nxb = s->nxb;
  Q.nxM = s->dims5[0];
  Q.nuM = s->dims5[1];
  Q.local_legs = c.l1 - c.l0;
  return Q;
}

gar::CsegParams make_cseg_params(gar_hip_solver *s, double mueq, const LegChunk &c) {
  gar::CsegParams Cp{};
  Cp.meta = s->buf.d_meta;
  Cp.prob = s->buf.d_prob;
  Cp.fac2 = s->buf.d_fac2;
  Cp.fac = s->buf.d_fac;
  Cp.status = s->buf.d_status;
  Cp.only = status_flags(s);
  Cp.prob_stride = s->prob_doubles;
  Cp.fac_stride = s->fac_doubles;
  Cp.fac2_stride = s->flay->fac_doubles;
  Cp.in_off0 = s->uni_in0;
  Cp.in_rec = s->uni_in_rec;
  Cp.horizon = s->horizon;
  Cp.num_legs = s->num_legs;
  Cp.leg_begin = c.l0;
  Cp.local_legs = c.l1 - c.l0;
  Cp.mueq = mueq;
  return Cp;
}

gar::CsegFwdParams make_cseg_fwd_params(gar_hip_solver *s) {
  gar::CsegFwdParams F{};
  F.meta = s->buf.d_meta;
  F.fac = s->buf.d_fac;
  F.sol = s->buf.d_sol;
  F.csol = s->buf.d_csol;
  F.only = status_flags(s);
  F.fac_stride = s->fac_doubles;
  F.sol_stride = s->sol_doubles;
  F.horizon = s->horizon;
  F.num_legs = s->num_legs;
  F.leg_begin = s->leg_begin;
  F.nxb = s->nxb;
  F.nc0 = s->nc0;
  return F;
}

// ---- backward, family by family ---------------------------------------------------------------------------------
// wave legs on a folded solver, the flagged problems (D != 0) on the constrained segment legs (gar_cstr_seg.hpp; every
// other problem: an early exit)
void backward_cstr_seg_legs(gar_hip_solver *s, double mueq, const LegChunk &c) {
  const dim3 grid = c.grid(s);
  const int *flagged = status_flags(s);
  const int N = s->horizon, l0 = c.l0;
  const gar::MfmaParams M = make_mfma_scratch_params(s, mueq, s->buf.d_fac2, s->flay->fac_doubles, s->cseg.rec,
                                                     (long long)N * s->cseg.rec, s->buf.d_cseg_resume);
  // (gar_cstr_seg.hpp) the leg-end stages -- V' = 0: no MFMA work, and the matrix on which Bunch-Kaufman pivots -- by a
  // workgroup each, then the chain once, leg by leg, from the knot below: decoupled -> coupled -> LDS Bunch-Kaufman;
  // CSTR_SEG_LEG_END = 0: the leg ends through the chain too, which then runs in two rounds -- coupled stage and LDS
  // Bunch-Kaufman for ONE stage each, then the same again from the hand-over knot, to the end
  if (!option_off("GAR_HIP_CSTR_SEG_LEG_END")) {
    hipLaunchKernelGGL(s->cseg.leg_end, grid, dim3((unsigned)s->cseg.stage_threads),
                       (size_t)s->cseg.leg_end_lds_doubles * sizeof(double), s->stream, M, s->num_legs, l0, flagged);
    for (int ph = 0; ph < 3; ++ph)
      hipLaunchKernelGGL(s->cseg.backward[ph], grid, dim3(64), (size_t)s->cseg.backward_lds_doubles * sizeof(double),
                         s->stream, M, s->num_legs, l0, flagged, ph == 0 ? gar::kCsegReenter : 0);
  } else {
    for (int round = 0; round < 2; ++round)
      for (int ph = 0; ph < 3; ++ph)
        hipLaunchKernelGGL(s->cseg.backward[ph], grid, dim3(64), (size_t)s->cseg.backward_lds_doubles * sizeof(double),
                           s->stream, M, s->num_legs, l0, flagged,
                           (round == 1 && ph == 0 ? gar::kCsegReenter : 0) | (round == 0 && ph >= 1 ? gar::kCsegSingle : 0));
  }
  const gar::CsegParams Cp = make_cseg_params(s, mueq, c);
  hipLaunchKernelGGL(s->cseg.chain, grid, dim3((unsigned)s->cseg.chain_threads),
                     (size_t)s->cseg.chain_lds_doubles * sizeof(double), s->stream, Cp);
  hipLaunchKernelGGL(s->cseg.stage, dim3((unsigned)N + 1, (unsigned)s->batch), dim3((unsigned)s->cseg.stage_threads),
                     (size_t)s->cseg.stage_lds_doubles * sizeof(double), s->stream, Cp);
  gar::LegParamParams Lp = make_leg_param_params(s, c);
  Lp.only = flagged;
  hipLaunchKernelGGL(gar::gar_leg_param_finish, grid, dim3(1024), 0, s->stream, Lp);
}

// the any-dimension leg sweep: every problem (only = null), or a folded solver's flagged ones
void backward_generic_legs(gar_hip_solver *s, double mueq, const LegChunk &c, const int *only) {
  gar::GenericParams G = make_params(s, mueq);
  G.only = only;
  G.leg_begin = c.l0;
  G.local_legs = c.l1 - c.l0;
  if (G.boundary)
    G.boundary += c.tup_shift;
  hipLaunchKernelGGL(gar::gar_backward_generic, c.grid(s), dim3(GAR_BACKWARD_THREADS), (size_t)s->lds.total * sizeof(double),
                     s->stream, G);
}

int backward_wave_legs(gar_hip_solver *s, double mueq, const LegChunk &c) {
  gar::LegParams Q = make_leg_params(s);
  Q.leg_begin = c.l0;
  Q.boundary += c.tup_shift;
  HIP_TRY(stamp(s, 0, c.first));
  if (s->fold) // knots with nc > 0: fold C, d into Q, q (gar_fold.hpp); problems with D != 0 get flagged
    hipLaunchKernelGGL(gar::gar_fold_constraints, dim3((unsigned)(s->horizon + 1), (unsigned)s->batch), dim3(256),
                       fold_lds_bytes(s), s->stream, make_fold_params(s));
  hipLaunchKernelGGL(s->leg_bwd_kernel, c.grid(s), dim3(64 * s->leg_waves), (size_t)s->leg_lds_doubles * sizeof(double),
                     s->stream, Q);
  hipLaunchKernelGGL(s->leg_tuple_kernel, c.grid(s), dim3(256), 0, s->stream, Q);
  if (s->fold && s->cseg_on) // ... and are swept by the constrained segment legs
    backward_cstr_seg_legs(s, mueq, c);
  else if (s->fold) // ... and are swept by the generic leg kernels (every other problem: an early exit)
    backward_generic_legs(s, mueq, c, status_flags(s));
  HIP_TRY(hipGetLastError());
  HIP_TRY(stamp(s, 1, c.last));
  return GAR_HIP_OK;
}

// segment legs (gar_leg_seg.hpp): plain part into the scratch records, then the parameter recursion + tuples
int backward_seg_legs(gar_hip_solver *s, double mueq, const LegChunk &c) {
  const gar::HostLayout &f = *s->flay;
  const int N = s->horizon;
  const gar::MfmaParams M = make_mfma_scratch_params(s, mueq, s->buf.d_fac2, f.fac_doubles, f.uni_fac_rec, f.meta[N].fac_off,
                                                     status_flags(s));
  const dim3 grid = c.grid(s);
  HIP_TRY(stamp(s, 0, c.first));
  hipLaunchKernelGGL(s->seg_bwd_kernel, grid, dim3(128), (size_t)s->seg_lds_doubles * sizeof(double), s->stream, M,
                     s->num_legs, c.l0);
  const gar::LegParamParams Q = make_leg_param_params(s, c);
  // the chain of Vxt alone per leg; everything else of every stage at once; the running sums and the tuples
  hipLaunchKernelGGL(gar::gar_leg_param_chain, grid, dim3(GAR_LEG_PARAM_THREADS),
                     (size_t)gar::leg_chain_lds_doubles(s->dims5[0]) * sizeof(double), s->stream, Q);
  hipLaunchKernelGGL(gar::gar_leg_param_stage, dim3((unsigned)N + 1, (unsigned)s->batch), dim3(GAR_LEG_STAGE_THREADS),
                     (size_t)gar::leg_stage_lds_doubles(s->dims5[0], s->dims5[1]) * sizeof(double), s->stream, Q);
  hipLaunchKernelGGL(gar::gar_leg_param_finish, grid, dim3(1024), 0, s->stream, Q);
  HIP_TRY(hipGetLastError());
  HIP_TRY(stamp(s, 1, c.last));
  return GAR_HIP_OK;
}

// the serial specialised sweep (4-wave mfma kernel, or the one-wave kernel and its constrained chain), then the initial stage
// the any-dimension kernels' view of a serial-fold solver's folded records: the stand-alone initial stage of the family
gar::GenericParams make_folded_params(gar_hip_solver *s, double mueq) {
  gar::GenericParams P = make_params(s, mueq);
  P.meta = s->buf.d_meta2;
  P.fac = s->buf.d_fac2;
  P.fac_stride = s->flay->fac_doubles;
  P.vxx_packed = s->sf_vxx_packed ? 1 : 0;
  return P;
}

int backward_serial(gar_hip_solver *s, double mueq) {
  const gar::MfmaParams M = make_mfma_params(s, mueq);
  const gar::GenericParams I = s->serial_fold ? make_folded_params(s, mueq) : make_params(s, mueq);
  HIP_TRY(stamp(s, 0));
  if (s->serial_fold) // knots with nc > 0: fold C, d into Q, q in the family's knot format; problems with D != 0 get flagged
    hipLaunchKernelGGL(gar::gar_fold_serial, dim3((unsigned)(s->horizon + 1), (unsigned)s->batch), dim3(256),
                       fold_lds_bytes(s), s->stream, make_serial_fold_params(s));
  if (s->wave_kernel) {
    const int wpb = s->waves_per_block;
    hipLaunchKernelGGL(s->wave_kernel, dim3((unsigned)((s->batch + wpb - 1) / wpb)),
                       dim3(s->wave_block_threads * wpb), (size_t)s->wave_lds_doubles * wpb * sizeof(double),
                       s->stream, M, s->batch);
    // constrained sweeps: the chain decoupled stage -> coupled stage -> LDS Bunch-Kaufman (gar_wave.hpp)
    for (auto k : {s->wave_coupled_kernel, s->wave_bk_kernel})
      if (k)
        hipLaunchKernelGGL(k, dim3((unsigned)((s->batch + wpb - 1) / wpb)), dim3(s->wave_block_threads * wpb),
                           (size_t)s->wave_lds_doubles * wpb * sizeof(double), s->stream, M, s->batch);
  } else {
    hipLaunchKernelGGL(s->mfma_kernel, dim3((unsigned)s->batch), dim3(256),
                       (size_t)s->mfma_lds_doubles * sizeof(double), s->stream, M);
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(stamp(s, 1));
  if (s->wave_kernel && s->wave_fused_init) {
    // nothing to launch: gar_backward_wave already produced kkt0.ff
  } else if (s->n0 <= 128) { // one wave per problem (wave-scope Bunch-Kaufman handles n <= 128)
    hipLaunchKernelGGL(gar::gar_initial_wave, dim3((unsigned)s->batch), dim3(64),
                       (size_t)gar::gar_initial_wave_lds_doubles(s->n0, s->nth0) * sizeof(double),
                       s->stream, I);
  } else {
    hipLaunchKernelGGL(gar::gar_initial_generic, dim3((unsigned)s->batch), dim3(256),
                       (size_t)s->lds.total * sizeof(double), s->stream, I);
  }
  if (s->serial_fold) {
    // The flagged problems: the family has swept their folded records like everyone's (it has no per-problem skip, and
    // none was added: its code is what it was) -- that result is never read.  Their status word is cleared and the
    // any-dimension serial sweep, initial stage included, takes them from the caller's knots into the caller-visible
    // records (every other problem: an early exit).  Where the any-dimension kernels do not fit a CU's LDS nobody can
    // take them: reported as failed.
    hipLaunchKernelGGL(gar::gar_fold_settle_flagged, dim3((unsigned)((s->batch + 255) / 256)), dim3(256), 0, s->stream,
                       status_words(s), status_flags(s), s->batch, s->serial_fold_fallback ? 0 : 1);
    if (s->serial_fold_fallback) {
      gar::GenericParams G = make_params(s, mueq);
      G.only = status_flags(s);
      hipLaunchKernelGGL(gar::gar_backward_generic, dim3(1u, (unsigned)s->batch), dim3(GAR_BACKWARD_THREADS),
                         (size_t)s->lds.total * sizeof(double), s->stream, G);
    }
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(stamp(s, 2));
  return GAR_HIP_OK;
}

// RiccatiSolverDense (gar_dense.hpp): nothing is bound for it (select_kernel), one workgroup per problem
int backward_dense(gar_hip_solver *s, double mueq) {
  hipLaunchKernelGGL(gar::gar_backward_dense, dim3((unsigned)s->batch), dim3(GAR_DENSE_THREADS),
                     (size_t)s->dense_lds.total * sizeof(double), s->stream, make_params(s, mueq));
  HIP_TRY(hipGetLastError());
  return GAR_HIP_OK;
}

int launch_backward(gar_hip_solver *s, double mueq, int l0 = -1, int l1 = -1) {
  RoctxRange range_(s->num_legs > 1 ? "gar::parallel_backward" : "gar::backwardImpl+factor_initial");
  if (l0 < 0)
    l0 = s->leg_begin, l1 = s->leg_end;
  const LegChunk c{l0, l1, l0 == s->leg_begin, l1 == s->leg_end, (long long)(l0 - s->leg_begin) * s->tuple_doubles};
  if (s->leg_bwd_kernel)
    return backward_wave_legs(s, mueq, c);
  if (s->seg_bwd_kernel)
    return backward_seg_legs(s, mueq, c);
  if (s->dense)
    return backward_dense(s, mueq);
  if (s->mfma_kernel || s->wave_kernel)
    return backward_serial(s, mueq);
  backward_generic_legs(s, mueq, c, nullptr);
  HIP_TRY(hipGetLastError());
  return GAR_HIP_OK;
}

constexpr size_t kCuLdsBytes = 160 * 1024, kLdsGranule = 1280; // gfx950: 160 KiB per CU, allocated in 320-dword pieces
inline size_t lds_round(size_t b) { return (b + kLdsGranule - 1) / kLdsGranule * kLdsGranule; }

gar::MfmaFwdParams make_mfma_fwd_params(gar_hip_solver *s) {
  gar::MfmaFwdParams F{};
  const int N = s->horizon;
  const gar::HostLayout &L = s->serial_fold ? *s->flay : static_cast<const gar::HostLayout &>(*s); // (the family's own records)
  F.fac = s->serial_fold ? s->buf.d_fac2 : s->buf.d_fac;
  F.init = s->buf.d_init;
  F.sol = s->buf.d_sol;
  F.fac_stride = L.fac_doubles;
  F.init_stride = s->init_doubles;
  F.sol_stride = s->sol_doubles;
  F.fac_rec = L.uni_fac_rec;
  F.fac_offN = L.meta[N].fac_off;
  F.horizon = N;
  F.nc0 = s->nc0;
  F.sol_u = (int)s->sol_u;
  F.sol_l = (int)s->sol_l;
  F.sol_v = (int)s->sol_v;
  F.ring0 = s->ring0;
  return F;
}

// ---- forward, family by family ----------------------------------------------------------------------------------
int forward_wave_legs(gar_hip_solver *s) {
  const gar::LegParams Q = make_leg_params(s);
  const dim3 grid((unsigned)(s->leg_end - s->leg_begin), (unsigned)s->batch);
  HIP_TRY(stamp(s, 3));
  hipLaunchKernelGGL(s->leg_fwd_kernel, grid, dim3(64), 0, s->stream, Q);
  if (s->fold) { // v_t = zff + Z x_t on this rank's stages; flagged problems: the generic roll-out
    hipLaunchKernelGGL(gar::gar_constraint_multipliers, dim3((unsigned)(s->horizon + 1), (unsigned)s->batch), dim3(64), 0,
                       s->stream, make_fold_params(s));
    if (s->cseg_on && !option_is("GAR_HIP_CSTR_SEG_FORWARD", "generic")) { // the constrained segment legs' own roll-out (gar_cstr_seg.hpp)
      hipLaunchKernelGGL(s->cseg.forward, grid, dim3(64), 0, s->stream, make_cseg_fwd_params(s));
    } else {
      gar::GenericParams G = make_params(s, 0.0);
      G.only = status_flags(s);
      hipLaunchKernelGGL(gar::gar_forward_generic, grid, dim3(GAR_FORWARD_THREADS), (size_t)s->lds.ftotal * sizeof(double),
                         s->stream, G);
    }
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(stamp(s, 4));
  return GAR_HIP_OK;
}

int forward_serial(gar_hip_solver *s) {
  const gar::MfmaFwdParams F = make_mfma_fwd_params(s);
  HIP_TRY(stamp(s, 3));
  // FORWARD = lean (per launch): the LDS-DMA roll-out of the pipelined schedule (gar_forward_lean.hpp, bit for bit the
  // same solution) for the whole batch in the plain schedule too -- one workgroup of four problems per CU at a time
  if (s->lean_fwd_kernel && option_is("GAR_HIP_FORWARD", "lean")) {
    if (s->lean_fwd_lds_bytes == 0) {
      s->lean_fwd_lds_bytes = std::max(lds_round(s->lean_fwd_used), lds_round(kCuLdsBytes / 2 + 1));
      HIP_TRY(hipFuncSetAttribute((const void *)s->lean_fwd_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)s->lean_fwd_lds_bytes));
    }
    hipLaunchKernelGGL(s->lean_fwd_kernel, dim3((unsigned)((s->batch + 3) / 4)), dim3(256), s->lean_fwd_lds_bytes, s->stream, F,
                       s->batch);
  } else {
    hipLaunchKernelGGL(s->mfma_fwd_kernel, dim3((unsigned)s->batch), dim3(64), s->mfma_fwd_lds_bytes, s->stream, F);
  }
  if (s->serial_fold) { // v_t = zff + Z x_t; the flagged problems: the any-dimension roll-out over the caller-visible records
    hipLaunchKernelGGL(gar::gar_constraint_multipliers, dim3((unsigned)(s->horizon + 1), (unsigned)s->batch), dim3(64), 0,
                       s->stream, make_fold_params(s));
    if (s->serial_fold_fallback) {
      gar::GenericParams G = make_params(s, 0.0);
      G.only = status_flags(s);
      hipLaunchKernelGGL(gar::gar_forward_generic, dim3(1u, (unsigned)s->batch), dim3(GAR_FORWARD_THREADS),
                         (size_t)s->lds.ftotal * sizeof(double), s->stream, G);
    }
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(stamp(s, 4));
  return GAR_HIP_OK;
}

// the any-dimension roll-out, a workgroup per (leg, problem); segment legs: their own, a wave each
int forward_seg_or_generic(gar_hip_solver *s, const gar::GenericParams &P) {
  const dim3 grid((unsigned)(s->leg_end - s->leg_begin), (unsigned)s->batch);
  HIP_TRY(stamp(s, 3));
  if (s->seg_bwd_kernel && s->seg_fwd_kernel && s->num_legs > 1)
    hipLaunchKernelGGL(s->seg_fwd_kernel, grid, dim3(64), 0, s->stream, P);
  else
    hipLaunchKernelGGL(gar::gar_forward_generic, grid, dim3(GAR_FORWARD_THREADS),
                       (size_t)s->lds.ftotal * sizeof(double), s->stream, P);
  HIP_TRY(hipGetLastError());
  HIP_TRY(stamp(s, 4));
  return GAR_HIP_OK;
}

int forward_by_family(gar_hip_solver *s, const double *theta_dev) {
  if (s->leg_fwd_kernel)
    return forward_wave_legs(s);
  if (s->mfma_fwd_kernel)
    return forward_serial(s);
  gar::GenericParams P = make_params(s, 0.0);
  P.theta = theta_dev;
  if (!s->dense)
    return forward_seg_or_generic(s, P);
  hipLaunchKernelGGL(gar::gar_forward_dense, dim3((unsigned)s->batch), dim3(256),
                     (size_t)s->lds.ftotal * sizeof(double), s->stream, P);
  HIP_TRY(hipGetLastError());
  return GAR_HIP_OK;
}
int launch_forward(gar_hip_solver *s, const double *theta_dev) {
  RoctxRange range_(s->num_legs > 1 ? "gar::parallel_forward" : "gar::forwardImpl");
  const int rc = forward_by_family(s, theta_dev);
  if (rc == GAR_HIP_OK)
    s->cur.rollout_enqueued();
  return rc;
}

#include "gar_pipeline.hpp"

gar::CondensedParams make_condensed_params(gar_hip_solver *s) {
  gar::CondensedParams C{};
  C.ball = s->buf.bound_all();
  C.prob = s->buf.d_prob;
  C.scratch = s->buf.d_cscratch;
  C.csol = s->buf.d_csol;
  C.status = s->buf.d_status;
  C.prob_stride = s->prob_doubles;
  C.scratch_stride = s->cscratch_doubles;
  C.G0_off = s->G0_off;
  C.g0_off = s->g0_off;
  C.batch = s->batch;
  C.num_legs = s->num_legs;
  C.legs_per_rank = s->legs_per_rank;
  C.world = s->world;
  C.tuple_doubles = (int)s->tuple_doubles;
  C.nxb = s->nxb;
  C.nc0 = s->nc0;
  C.nx0 = s->nx0;
  C.max_refinement = s->max_refinement;
  C.threshold = s->cond_threshold;
  C.backward_ok = s->cond_backward_ok;
  C.trace = s->buf.d_trace;
  C.gated = 0;
  return C;
}

// block cyclic reduction of the condensed system by the wave-leg family's own kernels (gar_cyclic.hpp)
void condensed_cyclic(gar_hip_solver *s, const gar::CondensedParams &C) {
  gar::CyclicParams Y{};
  Y.C = C;
  Y.h = 0;
  const int J = s->num_legs;
  const size_t lds = (size_t)s->cyc_lds_doubles * sizeof(double);
  // J waves for the legs + two for the initial condition's row (S_0 / r_0 and C_0), see gar_cyclic_setup
  hipLaunchKernelGGL(s->cyc_setup_kernel, dim3((unsigned)J + 2, (unsigned)s->batch), dim3(64),
                     lds + (size_t)s->cyc_block_doubles * sizeof(double), s->stream, Y);
  for (int h = 1; h < J; h *= 2) {
    Y.h = h;
    hipLaunchKernelGGL(s->cyc_reduce_kernel,
                       dim3((unsigned)((J + 2 * h - 1) / (2 * h)), (unsigned)s->batch), dim3(192),
                       2 * lds + (64 + (size_t)s->cyc_block_doubles) * sizeof(double), s->stream, Y);
  }
  // back-substitution: the levels holding at most 4 blocks in one workgroup, the wider ones a
  // launch each; then the states and the residual, a wave per leg
  int hmax = 1;
  while (2 * hmax < J)
    hmax *= 2;
  int htop = hmax;
  while (htop > 1 && (J / (htop / 2) + 1) / 2 <= 4)
    htop /= 2;
  Y.h = htop;
  hipLaunchKernelGGL(s->cyc_top_kernel, dim3((unsigned)s->batch), dim3(256), lds, s->stream, Y);
  for (int h = htop / 2; h >= 1; h /= 2) {
    Y.h = h;
    hipLaunchKernelGGL(s->cyc_backlevel_kernel,
                       dim3((unsigned)((J / h + 1) / 2), (unsigned)s->batch), dim3(64), 0,
                       s->stream, Y);
  }
  hipLaunchKernelGGL(s->cyc_recover_kernel, dim3((unsigned)J, (unsigned)s->batch), dim3(64),
                     (size_t)s->cyc_block_doubles * sizeof(double), s->stream, Y); // LDS: G0, padded
}

// the leg states eliminated leg-parallel, the chain on the J remaining blocks, the states back leg-parallel
// (gar_generic.hpp: gar_condensed_leg_eliminate); the full chain then runs gated, like behind cyclic reduction
void condensed_reduced(gar_hip_solver *s, const gar::CondensedParams &C) {
  const dim3 grid((unsigned)s->num_legs, (unsigned)s->batch);
  hipLaunchKernelGGL(gar::gar_condensed_leg_eliminate, grid, dim3(GAR_CONDENSED_THREADS),
                     (size_t)gar::gar_condensed_leg_lds_doubles(s->nxb) * sizeof(double), s->stream, C);
  if (s->cond_cr) {
    // the J remaining blocks by block cyclic reduction: a workgroup per block and level (gar_condensed_cr.hpp)
    const int J = s->num_legs;
    const size_t blk_bytes = (size_t)s->nxb * s->nxb * sizeof(double);
    // (the products of a level read their operands from LDS when four blocks fit a CU)
    const int staged = (size_t)gar::gar_condensed_cr_update_lds_doubles(s->nxb, 1) * sizeof(double) <= 160 * 1024;
    const size_t upd_bytes = (size_t)gar::gar_condensed_cr_update_lds_doubles(s->nxb, staged) * sizeof(double);
    hipLaunchKernelGGL(gar::gar_condensed_cr_assemble, grid, dim3(GAR_CONDENSED_THREADS), blk_bytes, s->stream, C);
    for (int h = 1; h < J; h *= 2) {
      hipLaunchKernelGGL(gar::gar_condensed_cr_eliminate, dim3((unsigned)((J - 1 + h) / (2 * h)), (unsigned)s->batch),
                         dim3(GAR_CONDENSED_THREADS),
                         (size_t)gar::gar_condensed_leg_lds_doubles(s->nxb) * sizeof(double), s->stream, C, h);
      hipLaunchKernelGGL(gar::gar_condensed_cr_update, dim3((unsigned)((J + 2 * h - 1) / (2 * h)), (unsigned)s->batch),
                         dim3(GAR_CONDENSED_THREADS), upd_bytes, s->stream, C, h, staged);
    }
    hipLaunchKernelGGL(gar::gar_condensed_cr_back, dim3((unsigned)s->batch), dim3(GAR_CONDENSED_THREADS),
                       (size_t)gar::gar_condensed_cr_back_lds_doubles(s->nxb, J) * sizeof(double), s->stream, C);
  } else {
    gar::CondensedParams R = C;
    R.reduced = 1;
    hipLaunchKernelGGL(gar::gar_condensed_generic, dim3((unsigned)s->batch), dim3(GAR_CONDENSED_THREADS),
                       (size_t)s->cond_lds_doubles * sizeof(double), s->stream, R);
  }
  hipLaunchKernelGGL(gar::gar_condensed_leg_states, grid, dim3(256), (size_t)(5 * s->nxb + 2) * sizeof(double),
                     s->stream, C);
}

int launch_condensed(gar_hip_solver *s) {
  RoctxRange range_("gar::assembleCondensedSystem+symmetricBlockTridiagSolve");
  gar::CondensedParams C = make_condensed_params(s);
  if (s->cyc_setup_kernel) {
    condensed_cyclic(s, C);
    HIP_TRY(hipGetLastError());
    C.gated = 1; // the chain kernel (with refinement) re-solves only what missed the threshold
  }
  if (s->cond_wave_kernel) {
    hipLaunchKernelGGL(s->cond_wave_kernel, dim3((unsigned)s->batch), dim3(64),
                       (size_t)s->cond_wave_lds_doubles * sizeof(double), s->stream, C);
  } else {
    if (!C.gated && s->cond_reduced) {
      condensed_reduced(s, C);
      C.gated = 1;
    }
    hipLaunchKernelGGL(gar::gar_condensed_generic, dim3((unsigned)s->batch), dim3(GAR_CONDENSED_THREADS),
                       (size_t)s->cond_lds_doubles * sizeof(double), s->stream, C);
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(stamp(s, 2)); // leg mode: the "initial stage" slot of the timing API is the condensed solve
  return GAR_HIP_OK;
}

int check_bt(const gar_hip_solver *s, int b, int t) {
  if (!s)
    return fail(GAR_HIP_ERR_ARG, "null solver");
  if (b < 0 || b >= s->batch)
    return fail(GAR_HIP_ERR_ARG, "problem index out of range");
  if (t < 0 || t > s->horizon)
    return fail(GAR_HIP_ERR_ARG, "stage index out of range");
  return GAR_HIP_OK;
}

int d2h(gar_hip_solver *s, double *dst, const double *src, int64_t n) {
  if (!dst || n <= 0)
    return GAR_HIP_OK;
  HIP_TRY(hipMemcpyAsync(dst, src, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, s->stream));
  return GAR_HIP_OK;
}

// ---- the KKT residuals of the whole batch (gar_kkt.hpp): one launch sequence for every solver family ------------------
gar::KktParams make_kkt_params(gar_hip_solver *s, double mueq, const double *theta_dev) {
  gar::KktParams K{};
  K.meta = s->buf.d_meta; // the caller-facing records, also on a folded solver (d_meta2 / d_prob2 stay inside the library)
  K.prob = s->buf.d_prob;
  K.sol = s->buf.d_sol;
  K.theta = theta_dev;
  K.stage = s->buf.d_kkt_stage;
  K.err = s->buf.d_kkt_err;
  K.prob_stride = s->prob_doubles;
  K.sol_stride = s->sol_doubles;
  K.G0_off = s->G0_off;
  K.g0_off = s->g0_off;
  K.horizon = s->horizon;
  K.nc0 = s->nc0;
  K.nth0 = s->nth0;
  K.qr_packed = s->qr_packed ? 1 : 0;
  K.mueq = mueq;
  return K;
}

// the two result buffers, on the first call after the layout was built (both or neither), and the kernel's LDS
int kkt_buffers(gar_hip_solver *s) {
  if (s->buf.d_kkt_stage)
    return GAR_HIP_OK;
  if ((int64_t)s->batch * (s->horizon + 1) > INT32_MAX) // one workgroup per (problem, stage), all of them in grid.x
    return fail(GAR_HIP_ERR_UNSUPPORTED, "gar_hip_kkt_error: batch x (horizon + 1) above 2^31 - 1 workgroups");
  int lds = 0; // (the knot is tiled, the stage's vectors are not: they bound the dimensions, below)
  for (const gar_stage_meta &m : s->meta)
    lds = std::max(lds, gar::kkt_lds_doubles(m.nx, m.nu, m.nc, m.nx2, m.nth, s->nc0));
  const size_t bytes = (size_t)lds * sizeof(double);
  if (bytes > kCuLdsBytes)
    return fail(GAR_HIP_ERR_UNSUPPORTED, "gar_hip_kkt_error: the stage vectors need " + std::to_string(bytes) +
                                             " B of LDS (> 160 KiB per CU)");
  HIP_TRY(max_lds(gar::gar_kkt_stage_residuals, (size_t)lds));
  DevBuf<double> st, er;
  HIP_TRY(st.zalloc((size_t)s->batch * (size_t)(s->horizon + 1) * 4));
  HIP_TRY(er.zalloc((size_t)s->batch * 3));
  s->buf.d_kkt_stage = std::move(st);
  s->buf.d_kkt_err = std::move(er);
  s->buf.kkt_lds_bytes = bytes;
  return GAR_HIP_OK;
}

// the kernel pair: a workgroup per (problem, stage), then the fold of the stage norms, a wave per problem
int launch_kkt_pair(gar_hip_solver *s, const gar::KktParams &K) {
  hipLaunchKernelGGL(gar::gar_kkt_stage_residuals, dim3((unsigned)s->batch * (unsigned)(s->horizon + 1)),
                     dim3(GAR_KKT_THREADS), s->buf.kkt_lds_bytes, s->stream, K);
  hipLaunchKernelGGL(gar::gar_kkt_reduce, dim3((unsigned)s->batch), dim3(64), 0, s->stream, K);
  HIP_TRY(hipGetLastError());
  return GAR_HIP_OK;
}

int launch_kkt(gar_hip_solver *s, double mueq, const double *theta_dev) {
  RoctxRange range_("gar::lqrComputeKktError");
  if (int rc = kkt_buffers(s))
    return rc;
  if (int rc = commit(s)) // knots the host staged since the last sweep
    return rc;
  return launch_kkt_pair(s, make_kkt_params(s, mueq, theta_dev));
}

// ---- the re-solve for new affine terms (gar_affine.hpp): scatter, prepare, the vector sweep, the initial stage -----------
// doubles of one problem's affine vector and the offsets of its stages (q_t | r_t | f_t ... g0), the CALLER's dimensions;
// a terminal knot given with nx2 = 0 has no f
int64_t affine_offsets(const gar_hip_solver *s, std::vector<long long> *off) {
  const int N = s->horizon;
  long long p = 0;
  if (off)
    off->assign((size_t)N + 2, 0);
  for (int t = 0; t <= N; ++t) {
    const int32_t *d = &s->user_dims5[5 * (size_t)t];
    if (off)
      (*off)[(size_t)t] = p;
    p += d[0] + d[1] + ((s->term_grown && t == N) ? 0 : d[3]);
  }
  if (off)
    (*off)[(size_t)N + 1] = p;
  return p + s->user_nc0;
}

// who is served: serial in time, one device, nc = nth = 0 on every knot, the stand-alone initial stage of one wave
int affine_check(const gar_hip_solver *s, const char *who) {
  if (!s)
    return fail(GAR_HIP_ERR_ARG, "null solver");
  const std::string w(who);
  if (s->multi)
    return fail(GAR_HIP_ERR_UNSUPPORTED, w + ": a multi-device solver is not served (the records live on several devices)");
  if (s->dense)
    return fail(GAR_HIP_ERR_UNSUPPORTED, w + ": the stage-dense solver is not served");
  if (s->num_legs != 1 || s->world != 1)
    return fail(GAR_HIP_ERR_UNSUPPORTED, w + ": leg mode is not served (num_legs = 1 only)");
  if (s->fold)
    return fail(GAR_HIP_ERR_UNSUPPORTED, w + ": a folded solver (constrained knots) is not served");
  for (int t = 0; t <= s->horizon; ++t) {
    const int32_t *d = &s->dims5[5 * (size_t)t];
    if (d[2] != 0 || d[4] != 0)
      return fail(GAR_HIP_ERR_UNSUPPORTED, w + ": knot " + std::to_string(t) + " is constrained or parameterised (nc = nth = 0 only)");
  }
  if (s->n0 > 128)
    return fail(GAR_HIP_ERR_UNSUPPORTED, w + ": nx + nc0 above 128 (the stand-alone initial stage of one wave)");
  return GAR_HIP_OK;
}

gar::AffineParams make_affine_params(gar_hip_solver *s) {
  gar::AffineParams A{};
  A.meta = s->buf.d_meta;
  A.prob = s->buf.d_prob;
  A.fac = s->buf.d_fac;
  A.W = s->buf.d_aff_W;
  A.status = status_words(s);
  A.ok = s->buf.d_aff_ok;
  A.src_off = s->buf.d_aff_off;
  A.prob_stride = s->prob_doubles;
  A.fac_stride = s->fac_doubles;
  A.src_stride = affine_offsets(s, nullptr);
  A.g0_off = s->g0_off;
  A.horizon = s->horizon;
  A.w_rec = s->buf.aff_w_rec;
  A.unx = s->padded ? s->unx : 0;
  A.unu = s->padded ? s->unu : 0;
  A.unc0 = s->user_nc0;
  A.qr_packed = s->qr_packed ? 1 : 0;
  A.vxx_packed = s->vxx_packed ? 1 : 0;
  A.fb_t2 = s->fb_t2 ? 1 : 0;
  A.nx_max = s->buf.aff_nx_max;
  return A;
}

// the side buffers, on the first call after the layout was built (all or none), and the two kernels' LDS
int affine_buffers(gar_hip_solver *s) {
  if (s->buf.d_aff_off)
    return GAR_HIP_OK;
  if ((int64_t)s->batch * (s->horizon + 1) > INT32_MAX)
    return fail(GAR_HIP_ERR_UNSUPPORTED, "gar_hip_backward_affine: batch x (horizon + 1) above 2^31 - 1 workgroups");
  int nu_max = 0, nx_max = 0, lds = 0, plds = 0;
  for (const gar_stage_meta &m : s->meta) {
    nu_max = std::max(nu_max, (int)m.nu);
    nx_max = std::max(nx_max, std::max((int)m.nx, (int)m.nx2));
  }
  for (const gar_stage_meta &m : s->meta) {
    lds = std::max(lds, gar::affine_sweep_lds_doubles(nx_max, m.nx, m.nu, m.nx2, s->fb_t2, s->vxx_packed));
    plds = std::max(plds, gar::affine_prepare_lds_doubles(m.nu, m.nx2, s->vxx_packed));
  }
  if ((size_t)std::max(lds, plds) * sizeof(double) > kCuLdsBytes)
    return fail(GAR_HIP_ERR_UNSUPPORTED, "gar_hip_backward_affine: a stage's blocks need " +
                                             std::to_string((size_t)std::max(lds, plds) * sizeof(double)) + " B of LDS (> 160 KiB per CU)");
  HIP_TRY(max_lds(gar::gar_backward_affine, (size_t)lds));
  HIP_TRY(max_lds(gar::gar_affine_prepare, (size_t)plds));
  std::vector<long long> off;
  affine_offsets(s, &off);
  const int w_rec = std::max(2, (nu_max * nu_max + 1) & ~1);
  DevBuf<double> W;
  DevBuf<int> ok;
  DevBuf<long long> doff;
  HIP_TRY(W.zalloc((size_t)s->batch * (size_t)(s->horizon + 1) * (size_t)w_rec));
  HIP_TRY(ok.zalloc((size_t)s->batch));
  HIP_TRY(doff.alloc(off.size()));
  HIP_TRY(hipMemcpy(doff, off.data(), sizeof(long long) * off.size(), hipMemcpyHostToDevice));
  s->buf.d_aff_W = std::move(W);
  s->buf.d_aff_ok = std::move(ok);
  s->buf.d_aff_off = std::move(doff);
  s->buf.aff_w_rec = w_rec;
  s->buf.aff_nx_max = nx_max;
  s->buf.aff_lds_bytes = (size_t)lds * sizeof(double);
  s->buf.aff_prep_lds_bytes = (size_t)plds * sizeof(double);
  s->cur.W_allocated();
  return GAR_HIP_OK;
}

// nb affine vectors at the DEVICE address src into the knots of problems b0 ..: staged host blocks go out first, so
// that no later flush writes older q, r, f over these
int launch_affine_scatter(gar_hip_solver *s, int b0, int nb, const double *src_dev) {
  if (nb == 0)
    return GAR_HIP_OK;
  if (int rc = commit(s))
    return rc;
  gar::AffineParams A = make_affine_params(s);
  A.src = src_dev;
  A.b0 = b0;
  hipLaunchKernelGGL(gar::gar_affine_scatter, dim3((unsigned)nb * (unsigned)(s->horizon + 1)), dim3(64), 0, s->stream, A);
  HIP_TRY(hipGetLastError());
  return GAR_HIP_OK;
}

// W = Rhat^-1 of every stage, formed once per factorisation: by the first re-solve or refinement step that needs it
int ensure_W(gar_hip_solver *s, const gar::AffineParams &A) {
  if (s->cur.W_valid)
    return GAR_HIP_OK;
  hipLaunchKernelGGL(gar::gar_affine_prepare, dim3((unsigned)s->batch * (unsigned)(s->horizon + 1)), dim3(64),
                     s->buf.aff_prep_lds_bytes, s->stream, A);
  HIP_TRY(hipGetLastError());
  s->cur.W_formed();
  return GAR_HIP_OK;
}

int launch_backward_affine(gar_hip_solver *s) {
  RoctxRange range_("gar::backward_affine");
  s->cur.solution_superseded(); // (the roll-out in HBM stays a solution gar_hip_refine may start from)
  if (int rc = settle_gains_readback(s, kBehindStream))
    return rc;
  if (int rc = commit(s)) // (a g0 staged through gar_hip_set_init)
    return rc;
  const gar::AffineParams A = make_affine_params(s);
  if (int rc = ensure_W(s, A))
    return rc;
  hipLaunchKernelGGL(gar::gar_backward_affine, dim3((unsigned)s->batch), dim3(64), s->buf.aff_lds_bytes, s->stream, A);
  // the initial stage: the stand-alone kernel backward_serial launches for the families that do not fuse it, on the
  // problems the sweep took (kkt0 is factorised again: its matrix is not kept)
  gar::GenericParams I = make_params(s, s->cur.mueq);
  I.only = s->buf.d_aff_ok;
  hipLaunchKernelGGL(gar::gar_initial_wave, dim3((unsigned)s->batch), dim3(64),
                     (size_t)gar::gar_initial_wave_lds_doubles(s->n0, s->nth0) * sizeof(double), s->stream, I);
  HIP_TRY(hipGetLastError());
  return GAR_HIP_OK;
}

// ---- one refinement step from the stored factorisation (gar_refine.hpp): residual vectors, sweep, initial stage, roll-out --
// the side buffers, on the first call after the layout was built (all or none), and the three kernels' LDS
int refine_buffers(gar_hip_solver *s) {
  if (s->buf.d_ref_gate)
    return GAR_HIP_OK;
  const int nx_max = s->buf.aff_nx_max; // (affine_buffers ran)
  int rhs_rec = 2, out_rec = 2, lds = 0, rlds = 0;
  for (const gar_stage_meta &m : s->meta) {
    rhs_rec = std::max(rhs_rec, gar::refine_rhs_f(m.nx, m.nu) + ((m.nx2 + 1) & ~1));
    out_rec = std::max(out_rec, gar::refine_out_vx(m.nu, m.nx2) + ((m.nx + 1) & ~1));
    lds = std::max(lds, gar::affine_sweep_lds_doubles(nx_max, m.nx, m.nu, m.nx2, s->fb_t2, s->vxx_packed) + 4);
    rlds = std::max(rlds, gar::refine_rollout_lds_doubles(nx_max, m.nx, m.nu, m.nx2, s->fb_t2, s->vxx_packed));
  }
  const int ilds = gar::gar_initial_wave_lds_doubles(s->n0, s->nth0);
  if ((size_t)std::max(lds, std::max(rlds, ilds)) * sizeof(double) > kCuLdsBytes)
    return fail(GAR_HIP_ERR_UNSUPPORTED, "gar_hip_refine: a stage's blocks need " +
                                             std::to_string((size_t)std::max(lds, std::max(rlds, ilds)) * sizeof(double)) +
                                             " B of LDS (> 160 KiB per CU)");
  HIP_TRY(max_lds(gar::gar_refine_sweep, (size_t)lds));
  HIP_TRY(max_lds(gar::gar_refine_rollout, (size_t)rlds));
  HIP_TRY(max_lds(gar::gar_refine_initial, (size_t)ilds));
  const int N = s->horizon, init_rec = std::max(2, (s->n0 + 1) & ~1);
  const long long rhs_stride = (long long)(N + 1) * rhs_rec + ((s->nc0 + 1) & ~1) + 2;
  const long long out_stride = (long long)(N + 1) * out_rec + 2; // (+ 2: the last stage names a record behind its own)
  DevBuf<double> rhs, out, init;
  DevBuf<int> gate;
  HIP_TRY(rhs.zalloc((size_t)s->batch * (size_t)rhs_stride));
  HIP_TRY(out.zalloc((size_t)s->batch * (size_t)out_stride));
  HIP_TRY(init.zalloc((size_t)s->batch * (size_t)init_rec));
  HIP_TRY(gate.zalloc((size_t)s->batch));
  s->buf.d_ref_rhs = std::move(rhs);
  s->buf.d_ref_out = std::move(out);
  s->buf.d_ref_init = std::move(init);
  s->buf.d_ref_gate = std::move(gate);
  s->buf.ref_rhs_rec = rhs_rec, s->buf.ref_out_rec = out_rec, s->buf.ref_init_rec = init_rec;
  s->buf.ref_rhs_stride = rhs_stride, s->buf.ref_out_stride = out_stride;
  s->buf.ref_sweep_lds_bytes = (size_t)lds * sizeof(double);
  s->buf.ref_roll_lds_bytes = (size_t)rlds * sizeof(double);
  s->buf.ref_init_lds_bytes = (size_t)ilds * sizeof(double);
  return GAR_HIP_OK;
}

// the KKT buffers of the solution in HBM (what gar_hip_kkt_error_async writes, at the mueq of the backward being reused),
// the residual vectors into the right-hand side and the gate words of the next step
int launch_refine_residual(gar_hip_solver *s, double threshold) {
  gar::KktParams K = make_kkt_params(s, s->cur.mueq, nullptr);
  K.rhs = s->buf.d_ref_rhs;
  K.gate = s->buf.d_ref_gate;
  K.status = status_words(s);
  K.rhs_stride = s->buf.ref_rhs_stride;
  K.rhs_rec = s->buf.ref_rhs_rec;
  K.threshold = threshold;
  return launch_kkt_pair(s, K);
}

// the parameter blocks of the redirected sweep, its initial stage and its roll-out: the refinement's side buffers, the
// gate words of the caller (the refinement's, or the adjoint's "status word zero")
void make_refine_params(gar_hip_solver *s, const int *gate, gar::AffineParams &A, gar::RefineParams &R) {
  A = make_affine_params(s);
  A.rhs = s->buf.d_ref_rhs;
  A.out = s->buf.d_ref_out;
  A.gate = gate;
  A.rhs_stride = s->buf.ref_rhs_stride, A.out_stride = s->buf.ref_out_stride;
  A.rhs_rec = s->buf.ref_rhs_rec, A.out_rec = s->buf.ref_out_rec;
  R = gar::RefineParams{};
  R.G = make_params(s, s->cur.mueq);
  R.rhs = A.rhs, R.out = A.out, R.init = s->buf.d_ref_init, R.gate = A.gate;
  R.rhs_stride = A.rhs_stride, R.out_stride = A.out_stride, R.init_rec = s->buf.ref_init_rec;
  R.rhs_rec = A.rhs_rec, R.out_rec = A.out_rec;
  R.fb_t2 = A.fb_t2, R.nx_max = A.nx_max;
}

// the correction of the gated problems, added to the solution records
int launch_refine_correction(gar_hip_solver *s) {
  gar::AffineParams A;
  gar::RefineParams R;
  make_refine_params(s, s->buf.d_ref_gate, A, R);
  if (int rc = ensure_W(s, A))
    return rc;
  const dim3 grid((unsigned)s->batch), wave(64);
  hipLaunchKernelGGL(gar::gar_refine_sweep, grid, wave, s->buf.ref_sweep_lds_bytes, s->stream, A);
  hipLaunchKernelGGL(gar::gar_refine_initial, grid, wave, s->buf.ref_init_lds_bytes, s->stream, R);
  hipLaunchKernelGGL(gar::gar_refine_rollout, grid, wave, s->buf.ref_roll_lds_bytes, s->stream, R);
  HIP_TRY(hipGetLastError());
  return GAR_HIP_OK;
}

// ---- gradients of a resident batch (gar_adjoint.hpp): the caller's packed layout on the device, the adjoint solve -------
// a padded solver's caller-side knot offsets on the device (the caller's layout does not turn with the ring); an unpadded
// solver's are the device's own stage descriptors
int user_layout_buffers(gar_hip_solver *s) {
  if (!s->padded || s->buf.d_adj_uoff)
    return GAR_HIP_OK;
  std::vector<long long> off;
  for (const gar_stage_meta &m : s->ulay->meta)
    off.push_back(m.in_off);
  DevBuf<long long> d;
  HIP_TRY(d.alloc(off.size()));
  HIP_TRY(hipMemcpy(d, off.data(), sizeof(long long) * off.size(), hipMemcpyHostToDevice));
  s->buf.d_adj_uoff = std::move(d);
  return GAR_HIP_OK;
}

// (affine_buffers ran: the offsets of the affine layout are on the device)
gar::AdjointParams make_adjoint_params(gar_hip_solver *s) {
  const gar::HostLayout &u = caller_layout(s);
  gar::AdjointParams P{};
  P.meta = s->buf.d_meta;
  P.U.in_off = s->padded ? s->buf.d_adj_uoff.get() : nullptr;
  P.U.stride = u.prob_doubles, P.U.G0_off = u.G0_off, P.U.g0_off = u.g0_off;
  P.U.unx = s->padded ? s->unx : 0, P.U.unu = s->padded ? s->unu : 0;
  P.U.nc0 = s->user_nc0;
  P.vec_off = s->buf.d_aff_off;
  P.vec_stride = affine_offsets(s, nullptr);
  P.status = status_words(s);
  P.rhs = s->buf.d_ref_rhs;
  P.gate = s->buf.d_adj_gate;
  P.rhs_stride = s->buf.ref_rhs_stride;
  P.rhs_rec = s->buf.ref_rhs_rec;
  P.sol = s->buf.d_sol;
  P.adj = s->buf.d_adj_rec;
  P.sol_stride = s->sol_doubles;
  P.prob = s->buf.d_prob;
  P.prob_stride = s->prob_doubles, P.G0_off = s->G0_off, P.g0_off = s->g0_off;
  P.horizon = s->horizon, P.nc0 = s->nc0, P.nx0 = s->nx0;
  P.qr_packed = s->qr_packed ? 1 : 0;
  return P;
}

// the adjoint records, the gate words and the LDS of the two kernels with dynamic LDS, on the first call after the layout
// was built (affine_buffers and refine_buffers ran)
int adjoint_buffers(gar_hip_solver *s) {
  if (s->buf.d_adj_gate)
    return GAR_HIP_OK;
  if (int rc = user_layout_buffers(s))
    return rc;
  int glds = 0;
  for (const gar_stage_meta &m : s->meta) // (the device's dimensions bound the caller's)
    glds = std::max(glds, gar::adjoint_grad_lds_doubles(m.nx, m.nu, m.nx2, s->nc0, s->nx0));
  if ((size_t)glds * sizeof(double) > kCuLdsBytes)
    return fail(GAR_HIP_ERR_UNSUPPORTED, "gar_hip_adjoint: a knot of the gradient record needs " +
                                             std::to_string((size_t)glds * sizeof(double)) + " B of LDS (> 160 KiB per CU)");
  HIP_TRY(max_lds(gar::gar_adjoint_gradients, (size_t)glds));
  HIP_TRY(max_lds(gar::gar_adjoint_rollout, s->buf.ref_roll_lds_bytes / sizeof(double)));
  DevBuf<double> rec;
  DevBuf<int> gate;
  HIP_TRY(rec.zalloc((size_t)s->batch * (size_t)s->sol_doubles));
  HIP_TRY(gate.zalloc((size_t)s->batch));
  s->buf.d_adj_rec = std::move(rec);
  s->buf.d_adj_gate = std::move(gate);
  s->buf.adj_grad_lds_bytes = (size_t)glds * sizeof(double);
  return GAR_HIP_OK;
}

// nb packed problems in the caller's layout at the DEVICE address src into the knots of problems b0 ...
int launch_user_upload(gar_hip_solver *s, int b0, int nb, const double *src_dev) {
  if (nb == 0)
    return GAR_HIP_OK;
  gar::AdjointParams P = make_adjoint_params(s);
  P.user = src_dev;
  P.b0 = b0;
  hipLaunchKernelGGL(gar::gar_user_upload_scatter, dim3((unsigned)nb * (unsigned)(s->horizon + 1)), dim3(GAR_ADJ_THREADS), 0,
                     s->stream, P);
  HIP_TRY(hipGetLastError());
  return GAR_HIP_OK;
}

// records (the solution's or the adjoint's) of problems b0 ... as nb vectors of the affine layout at the DEVICE address out
int launch_solution_gather(gar_hip_solver *s, int b0, int nb, const double *rec_dev, double *out_dev) {
  if (nb == 0)
    return GAR_HIP_OK;
  gar::AdjointParams P = make_adjoint_params(s);
  P.rec = rec_dev;
  P.vec = out_dev;
  P.b0 = b0;
  hipLaunchKernelGGL(gar::gar_solution_gather, dim3((unsigned)nb * (unsigned)(s->horizon + 1)), dim3(64), 0, s->stream, P);
  HIP_TRY(hipGetLastError());
  return GAR_HIP_OK;
}

// the cotangents at cot_dev -> the adjoint records; their affine-layout vectors to adj_dev and the gradient records to
// grad_dev where asked for.  Nothing of the primal is written.
int launch_adjoint(gar_hip_solver *s, const double *cot_dev, double *adj_dev, double *grad_dev) {
  RoctxRange range_("gar::adjoint");
  gar::AffineParams A;
  gar::RefineParams R;
  make_refine_params(s, s->buf.d_adj_gate, A, R);
  gar::RefineParams Radj = R; // the roll-out's "solution" is the adjoint record
  Radj.G.sol = s->buf.d_adj_rec;
  if (int rc = ensure_W(s, A))
    return rc;
  gar::AdjointParams P = make_adjoint_params(s);
  P.cot = cot_dev;
  P.grad = grad_dev;
  const dim3 grid((unsigned)s->batch), stages((unsigned)s->batch * (unsigned)(s->horizon + 1)), wave(64);
  hipLaunchKernelGGL(gar::gar_adjoint_scatter, stages, wave, 0, s->stream, P);
  hipLaunchKernelGGL(gar::gar_refine_sweep, grid, wave, s->buf.ref_sweep_lds_bytes, s->stream, A);
  hipLaunchKernelGGL(gar::gar_refine_initial, grid, wave, s->buf.ref_init_lds_bytes, s->stream, R);
  hipLaunchKernelGGL(gar::gar_adjoint_rollout, grid, wave, s->buf.ref_roll_lds_bytes, s->stream, Radj);
  HIP_TRY(hipGetLastError());
  if (adj_dev)
    if (int rc = launch_solution_gather(s, 0, s->batch, s->buf.d_adj_rec, adj_dev))
      return rc;
  if (grad_dev) {
    hipLaunchKernelGGL(gar::gar_adjoint_gradients, stages, dim3(GAR_ADJ_THREADS), s->buf.adj_grad_lds_bytes, s->stream, P);
    HIP_TRY(hipGetLastError());
  }
  return GAR_HIP_OK;
}

// ---- many affine terms at once (gar_affine_multi.hpp): panel scatter, the MFMA sweep, the initial stage, the MFMA roll-out ----
// bytes of the work buffers of one panel of one problem (the header's formula): the two panel records of every stage and
// the initial stage's three vectors of 16 columns
size_t affine_multi_panel_bytes(const gar_hip_solver *s, int prhs_rec, int pout_rec, int ivx_rec, int ig0_rec, int init_rec) {
  return sizeof(double) * ((size_t)(s->horizon + 1) * (size_t)(prhs_rec + pout_rec) +
                           (size_t)GAR_AM_COLS * (size_t)(ivx_rec + ig0_rec + init_rec));
}
// the work buffers of one chunk and the gate words, on the first call after the layout was built (all or none; a failed
// allocation leaves the solver as it was), and the three kernels' LDS (affine_buffers ran)
int affine_multi_buffers(gar_hip_solver *s) {
  if (s->buf.d_am_gate)
    return GAR_HIP_OK;
  const int nx_max = s->buf.aff_nx_max, N = s->horizon, C = GAR_AM_COLS;
  int nu_max = 0, rows = 1, lds = 0, rlds = 0;
  for (const gar_stage_meta &m : s->meta)
    nu_max = std::max(nu_max, (int)m.nu);
  for (const gar_stage_meta &m : s->meta) {
    rows = std::max(rows, (int)(m.nx + m.nu + m.nx2));
    lds = std::max(lds, gar::affine_multi_sweep_lds_doubles(nx_max, nu_max, m.nx, m.nu, m.nx2, s->fb_t2, s->vxx_packed));
    rlds = std::max(rlds, gar::affine_multi_rollout_lds_doubles(nx_max, nu_max, m.nx, m.nu, m.nx2, s->fb_t2, s->vxx_packed));
  }
  const int ilds = gar::gar_initial_wave_lds_doubles(s->n0, s->nth0);
  if ((size_t)std::max(lds, std::max(rlds, ilds)) * sizeof(double) > kCuLdsBytes)
    return fail(GAR_HIP_ERR_UNSUPPORTED, "gar_hip_affine_solve_multi: a stage's blocks and panels need " +
                                             std::to_string((size_t)std::max(lds, std::max(rlds, ilds)) * sizeof(double)) +
                                             " B of LDS (> 160 KiB per CU)");
  const int rec = C * rows, ivx_rec = std::max(2, (s->nx0 + 1) & ~1), ig0_rec = std::max(2, (s->nc0 + 1) & ~1);
  const int init_rec = std::max(2, (s->n0 + 1) & ~1);
  // panels per problem in a chunk: enough workgroups for the device at a small batch, at most 1 GiB of work buffers
  const size_t per_panel = affine_multi_panel_bytes(s, rec, rec, ivx_rec, ig0_rec, init_rec);
  int panels = std::min(8, std::max(1, (1024 + s->batch - 1) / s->batch));
  while (panels > 1 && per_panel * (size_t)s->batch * (size_t)panels > ((size_t)1 << 30))
    --panels;
  if ((int64_t)s->batch * panels * std::max(N + 1, C) > INT32_MAX)
    return fail(GAR_HIP_ERR_UNSUPPORTED, "gar_hip_affine_solve_multi: batch x (horizon + 1) above 2^31 - 1 workgroups");
  const size_t bp = (size_t)s->batch * (size_t)panels;
  const long long stride = (long long)(N + 1) * rec;
  DevBuf<double> rhs, out, ivx, ig0, ires;
  DevBuf<int> gate;
  hipError_t e = rhs.zalloc(bp * (size_t)stride);
  e = e != hipSuccess ? e : out.zalloc(bp * (size_t)stride);
  e = e != hipSuccess ? e : ivx.zalloc(bp * C * (size_t)ivx_rec);
  e = e != hipSuccess ? e : ig0.zalloc(bp * C * (size_t)ig0_rec);
  e = e != hipSuccess ? e : ires.zalloc(bp * C * (size_t)init_rec);
  e = e != hipSuccess ? e : gate.zalloc((size_t)s->batch);
  if (e != hipSuccess) {
    (void)hipGetLastError(); // (the error is reported here; the next launch check of this solver starts clean)
    return fail(GAR_HIP_ERR_DEVICE, "gar_hip_affine_solve_multi: " + std::to_string(per_panel * bp + sizeof(int) * (size_t)s->batch) +
                                        " B of work buffers: " + hipGetErrorString(e));
  }
  HIP_TRY(max_lds(gar::gar_affine_sweep_multi, (size_t)lds));
  HIP_TRY(max_lds(gar::gar_rollout_multi, (size_t)rlds));
  HIP_TRY(max_lds(gar::gar_affine_multi_initial, (size_t)ilds));
  s->buf.d_am_rhs = std::move(rhs), s->buf.d_am_out = std::move(out);
  s->buf.d_am_ivx = std::move(ivx), s->buf.d_am_ig0 = std::move(ig0), s->buf.d_am_ires = std::move(ires);
  s->buf.d_am_gate = std::move(gate);
  s->buf.am_panels = panels, s->buf.am_nu_max = nu_max;
  s->buf.am_prhs_rec = s->buf.am_pout_rec = rec;
  s->buf.am_ivx_rec = ivx_rec, s->buf.am_ig0_rec = ig0_rec, s->buf.am_init_rec = init_rec;
  s->buf.am_prhs_stride = s->buf.am_pout_stride = stride;
  s->buf.am_sweep_lds_bytes = (size_t)lds * sizeof(double);
  s->buf.am_roll_lds_bytes = (size_t)rlds * sizeof(double);
  s->buf.am_init_lds_bytes = (size_t)ilds * sizeof(double);
  return GAR_HIP_OK;
}

// columns [0, nrhs) of every problem: rhs_dev and out_dev are [batch][nrhs][affine doubles] at DEVICE addresses.  The host
// loops over chunks of am_panels panels; every kernel of a chunk is ordered behind the previous chunk's on the stream.
int launch_affine_multi(gar_hip_solver *s, int nrhs, const double *rhs_dev, double *out_dev) {
  RoctxRange range_("gar::affine_solve_multi");
  const gar::AffineParams A = make_affine_params(s);
  if (int rc = ensure_W(s, A))
    return rc;
  gar::AffineMultiParams P{};
  P.meta = s->buf.d_meta;
  P.U.unx = s->padded ? s->unx : 0, P.U.unu = s->padded ? s->unu : 0;
  P.U.nc0 = s->user_nc0;
  P.vec_off = s->buf.d_aff_off;
  P.vec_stride = affine_offsets(s, nullptr);
  P.status = status_words(s);
  P.prob = s->buf.d_prob, P.fac = s->buf.d_fac, P.W = s->buf.d_aff_W;
  P.prob_stride = s->prob_doubles, P.fac_stride = s->fac_doubles;
  P.w_rec = s->buf.aff_w_rec, P.horizon = s->horizon, P.nc0 = s->nc0;
  P.vxx_packed = A.vxx_packed, P.fb_t2 = A.fb_t2;
  P.nrhs = nrhs;
  P.rhs = rhs_dev, P.out = out_dev;
  P.prhs = s->buf.d_am_rhs, P.pout = s->buf.d_am_out;
  P.ivx = s->buf.d_am_ivx, P.ig0 = s->buf.d_am_ig0, P.ires = s->buf.d_am_ires;
  P.gate = s->buf.d_am_gate;
  P.prhs_stride = s->buf.am_prhs_stride, P.pout_stride = s->buf.am_pout_stride;
  P.prhs_rec = s->buf.am_prhs_rec, P.pout_rec = s->buf.am_pout_rec;
  P.ivx_rec = s->buf.am_ivx_rec, P.ig0_rec = s->buf.am_ig0_rec, P.init_rec = s->buf.am_init_rec;
  P.nx_max = s->buf.aff_nx_max, P.nu_max = s->buf.am_nu_max;
  gar::AffineMultiInit I{};
  I.G = make_params(s, s->cur.mueq);
  I.ivx = P.ivx, I.ig0 = P.ig0, I.ires = P.ires, I.gate = P.gate;
  I.ivx_rec = P.ivx_rec, I.ig0_rec = P.ig0_rec, I.init_rec = P.init_rec;
  const int C = GAR_AM_COLS, total = (nrhs + C - 1) / C;
  for (int p0 = 0; p0 < total; p0 += s->buf.am_panels) {
    P.c0 = p0 * C;
    P.panels = I.panels = std::min(s->buf.am_panels, total - p0);
    const unsigned groups = (unsigned)s->batch * (unsigned)P.panels;
    hipLaunchKernelGGL(gar::gar_affine_multi_scatter, dim3(groups * (unsigned)(s->horizon + 1)), dim3(GAR_AM_THREADS), 0,
                       s->stream, P);
    hipLaunchKernelGGL(gar::gar_affine_sweep_multi, dim3(groups), dim3(GAR_AM_THREADS), s->buf.am_sweep_lds_bytes, s->stream, P);
    hipLaunchKernelGGL(gar::gar_affine_multi_initial, dim3(groups * (unsigned)C), dim3(64), s->buf.am_init_lds_bytes, s->stream, I);
    hipLaunchKernelGGL(gar::gar_rollout_multi, dim3(groups), dim3(GAR_AM_THREADS), s->buf.am_roll_lds_bytes, s->stream, P);
    HIP_TRY(hipGetLastError());
  }
  return GAR_HIP_OK;
}
