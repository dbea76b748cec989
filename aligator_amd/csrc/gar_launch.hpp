// gar_launch.hpp -- kernel parameter blocks (one make_* each) and launches of the sweeps, one function per kernel family:
// launch_backward, launch_forward, the pipelined schedule (gar_pipeline.hpp), launch_condensed.  (What a batch that stays in
// HBM is asked besides its sweeps -- KKT residuals, re-solve, refinement, adjoint, many affine terms: gar_resident.hpp.)
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
