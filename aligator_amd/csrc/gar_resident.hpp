// gar_resident.hpp -- the host side of the services on a batch that stays in HBM: the KKT residuals (gar_kkt.hpp), the
// re-solve for new affine terms (gar_affine.hpp), iterative refinement (gar_refine.hpp), the adjoint with block gradients
// (gar_adjoint.hpp), many affine terms at once (gar_affine_multi.hpp).  Per service: what it owns is its work area
// (gar_host.hpp: KktArea ... AffineMultiArea), what it needs built before it is what its ensure_* calls first, and the order
// in which its entry points refuse is resident_begin's; then one make_* per parameter block and one launch_* per call.
// Part of the ONE translation unit gar_hip.cpp, included in place behind gar_launch.hpp under the same convention.
#pragma once

// ---- what the ensure_* share -------------------------------------------------------------------------------------------
// `doubles` of dynamic LDS against a CU's; `what` names the entry point and what needs them
int lds_fits(int doubles, const char *what) {
  const size_t bytes = (size_t)doubles * sizeof(double);
  if (bytes > kCuLdsBytes)
    return fail(GAR_HIP_ERR_UNSUPPORTED, std::string(what) + " " + std::to_string(bytes) + " B of LDS (> 160 KiB per CU)");
  return GAR_HIP_OK;
}
// one workgroup per (problem, stage) -- or per (problem, panel, stage or column) -- all of them in grid.x
int grid_fits(const gar_hip_solver *s, int64_t per_problem, const char *who) {
  if ((int64_t)s->batch * per_problem > INT32_MAX)
    return fail(GAR_HIP_ERR_UNSUPPORTED, std::string(who) + ": batch x (horizon + 1) above 2^31 - 1 workgroups");
  return GAR_HIP_OK;
}
hipError_t to_device(DevBuf<long long> &d, const std::vector<long long> &v) {
  const hipError_t e = d.alloc(v.size());
  return e != hipSuccess ? e : hipMemcpy(d, v.data(), sizeof(long long) * v.size(), hipMemcpyHostToDevice);
}

// ---- the KKT residuals of the whole batch (gar_kkt.hpp): one launch sequence for every solver family ------------------
gar::KktParams make_kkt_params(gar_hip_solver *s, double mueq, const double *theta_dev) {
  gar::KktParams K{};
  K.meta = s->buf.d_meta; // the caller-facing records, also on a folded solver (d_meta2 / d_prob2 stay inside the library)
  K.prob = s->buf.d_prob;
  K.sol = s->buf.d_sol;
  K.theta = theta_dev;
  K.stage = s->buf.kkt.stage;
  K.err = s->buf.kkt.err;
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

int ensure_kkt(gar_hip_solver *s) {
  if (s->buf.kkt.built())
    return GAR_HIP_OK;
  if (int rc = grid_fits(s, s->horizon + 1, "gar_hip_kkt_error"))
    return rc;
  int lds = 0; // (the knot is tiled, the stage's vectors are not: they bound the dimensions, below)
  for (const gar_stage_meta &m : s->meta)
    lds = std::max(lds, gar::kkt_lds_doubles(m.nx, m.nu, m.nc, m.nx2, m.nth, s->nc0));
  if (int rc = lds_fits(lds, "gar_hip_kkt_error: the stage vectors need"))
    return rc;
  HIP_TRY(max_lds(gar::gar_kkt_stage_residuals, (size_t)lds));
  gar::KktArea a;
  HIP_TRY(a.stage.zalloc((size_t)s->batch * (size_t)(s->horizon + 1) * 4));
  HIP_TRY(a.err.zalloc((size_t)s->batch * 3));
  a.lds_bytes = (size_t)lds * sizeof(double);
  s->buf.kkt = std::move(a);
  return GAR_HIP_OK;
}

// the kernel pair: a workgroup per (problem, stage), then the fold of the stage norms, a wave per problem
int launch_kkt_pair(gar_hip_solver *s, const gar::KktParams &K) {
  hipLaunchKernelGGL(gar::gar_kkt_stage_residuals, dim3((unsigned)s->batch * (unsigned)(s->horizon + 1)),
                     dim3(GAR_KKT_THREADS), s->buf.kkt.lds_bytes, s->stream, K);
  hipLaunchKernelGGL(gar::gar_kkt_reduce, dim3((unsigned)s->batch), dim3(64), 0, s->stream, K);
  HIP_TRY(hipGetLastError());
  return GAR_HIP_OK;
}

int launch_kkt(gar_hip_solver *s, double mueq, const double *theta_dev) {
  RoctxRange range_("gar::lqrComputeKktError");
  if (int rc = ensure_kkt(s))
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

// the caller's dimensions and the layout of an affine vector: what AdjointParams and AffineMultiParams share
template <class P> void fill_caller_vectors(gar_hip_solver *s, P &p) {
  p.U.unx = s->padded ? s->unx : 0, p.U.unu = s->padded ? s->unu : 0;
  p.U.nc0 = s->user_nc0;
  p.vec_off = s->buf.aff.off;
  p.vec_stride = affine_offsets(s, nullptr);
}

gar::AffineParams make_affine_params(gar_hip_solver *s) {
  const gar::AffineArea &a = s->buf.aff;
  gar::AffineParams A{};
  A.meta = s->buf.d_meta;
  A.prob = s->buf.d_prob;
  A.fac = s->buf.d_fac;
  A.W = a.W;
  A.status = status_words(s);
  A.ok = a.ok;
  A.src_off = a.off;
  A.prob_stride = s->prob_doubles;
  A.fac_stride = s->fac_doubles;
  A.src_stride = affine_offsets(s, nullptr);
  A.g0_off = s->g0_off;
  A.horizon = s->horizon;
  A.w_rec = a.w_rec;
  A.unx = s->padded ? s->unx : 0;
  A.unu = s->padded ? s->unu : 0;
  A.unc0 = s->user_nc0;
  A.qr_packed = s->qr_packed ? 1 : 0;
  A.vxx_packed = s->vxx_packed ? 1 : 0;
  A.fb_t2 = s->fb_t2 ? 1 : 0;
  A.nx_max = a.nx_max;
  return A;
}

int ensure_affine(gar_hip_solver *s) {
  if (s->buf.aff.built())
    return GAR_HIP_OK;
  if (int rc = grid_fits(s, s->horizon + 1, "gar_hip_backward_affine"))
    return rc;
  int nu_max = 0, nx_max = 0, lds = 0, plds = 0;
  for (const gar_stage_meta &m : s->meta) {
    nu_max = std::max(nu_max, (int)m.nu);
    nx_max = std::max(nx_max, std::max((int)m.nx, (int)m.nx2));
  }
  for (const gar_stage_meta &m : s->meta) {
    lds = std::max(lds, gar::affine_sweep_lds_doubles(nx_max, m.nx, m.nu, m.nx2, s->fb_t2, s->vxx_packed));
    plds = std::max(plds, gar::affine_prepare_lds_doubles(m.nu, m.nx2, s->vxx_packed));
  }
  if (int rc = lds_fits(std::max(lds, plds), "gar_hip_backward_affine: a stage's blocks need"))
    return rc;
  HIP_TRY(max_lds(gar::gar_backward_affine, (size_t)lds));
  HIP_TRY(max_lds(gar::gar_affine_prepare, (size_t)plds));
  std::vector<long long> off;
  affine_offsets(s, &off);
  gar::AffineArea a;
  a.w_rec = std::max(2, (nu_max * nu_max + 1) & ~1);
  a.nx_max = nx_max;
  a.sweep_lds_bytes = (size_t)lds * sizeof(double);
  a.prep_lds_bytes = (size_t)plds * sizeof(double);
  HIP_TRY(a.W.zalloc((size_t)s->batch * (size_t)(s->horizon + 1) * (size_t)a.w_rec));
  HIP_TRY(a.ok.zalloc((size_t)s->batch));
  HIP_TRY(to_device(a.off, off));
  s->buf.aff = std::move(a);
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
                     s->buf.aff.prep_lds_bytes, s->stream, A);
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
  hipLaunchKernelGGL(gar::gar_backward_affine, dim3((unsigned)s->batch), dim3(64), s->buf.aff.sweep_lds_bytes, s->stream, A);
  // the initial stage: the stand-alone kernel backward_serial launches for the families that do not fuse it, on the
  // problems the sweep took (kkt0 is factorised again: its matrix is not kept)
  gar::GenericParams I = make_params(s, s->cur.mueq);
  I.only = s->buf.aff.ok;
  hipLaunchKernelGGL(gar::gar_initial_wave, dim3((unsigned)s->batch), dim3(64),
                     (size_t)gar::gar_initial_wave_lds_doubles(s->n0, s->nth0) * sizeof(double), s->stream, I);
  HIP_TRY(hipGetLastError());
  return GAR_HIP_OK;
}

// ---- one refinement step from the stored factorisation (gar_refine.hpp): residual vectors, sweep, initial stage, roll-out --
int ensure_refine(gar_hip_solver *s) {
  if (s->buf.ref.built())
    return GAR_HIP_OK;
  if (int rc = ensure_affine(s)) // the chain vector's length; every step sweeps with W and the affine block
    return rc;
  const int nx_max = s->buf.aff.nx_max;
  gar::RefineArea r;
  r.rhs_rec = r.out_rec = 2;
  int lds = 0, rlds = 0;
  for (const gar_stage_meta &m : s->meta) {
    r.rhs_rec = std::max(r.rhs_rec, gar::refine_rhs_f(m.nx, m.nu) + ((m.nx2 + 1) & ~1));
    r.out_rec = std::max(r.out_rec, gar::refine_out_vx(m.nu, m.nx2) + ((m.nx + 1) & ~1));
    lds = std::max(lds, gar::affine_sweep_lds_doubles(nx_max, m.nx, m.nu, m.nx2, s->fb_t2, s->vxx_packed) + 4);
    rlds = std::max(rlds, gar::refine_rollout_lds_doubles(nx_max, m.nx, m.nu, m.nx2, s->fb_t2, s->vxx_packed));
  }
  const int ilds = gar::gar_initial_wave_lds_doubles(s->n0, s->nth0);
  if (int rc = lds_fits(std::max(lds, std::max(rlds, ilds)), "gar_hip_refine: a stage's blocks need"))
    return rc;
  HIP_TRY(max_lds(gar::gar_refine_sweep, (size_t)lds));
  HIP_TRY(max_lds(gar::gar_refine_rollout, (size_t)rlds));
  HIP_TRY(max_lds(gar::gar_refine_initial, (size_t)ilds));
  const int N = s->horizon;
  r.init_rec = std::max(2, (s->n0 + 1) & ~1);
  r.rhs_stride = (long long)(N + 1) * r.rhs_rec + ((s->nc0 + 1) & ~1) + 2;
  r.out_stride = (long long)(N + 1) * r.out_rec + 2; // (+ 2: the last stage names a record behind its own)
  r.sweep_lds_bytes = (size_t)lds * sizeof(double);
  r.roll_lds_bytes = (size_t)rlds * sizeof(double);
  r.init_lds_bytes = (size_t)ilds * sizeof(double);
  HIP_TRY(r.rhs.zalloc((size_t)s->batch * (size_t)r.rhs_stride));
  HIP_TRY(r.out.zalloc((size_t)s->batch * (size_t)r.out_stride));
  HIP_TRY(r.init.zalloc((size_t)s->batch * (size_t)r.init_rec));
  HIP_TRY(r.gate.zalloc((size_t)s->batch));
  s->buf.ref = std::move(r);
  return GAR_HIP_OK;
}

// the KKT buffers of the solution in HBM (what gar_hip_kkt_error_async writes, at the mueq of the backward being reused),
// the residual vectors into the right-hand side and the gate words of the next step
int launch_refine_residual(gar_hip_solver *s, double threshold) {
  gar::KktParams K = make_kkt_params(s, s->cur.mueq, nullptr);
  K.rhs = s->buf.ref.rhs;
  K.gate = s->buf.ref.gate;
  K.status = status_words(s);
  K.rhs_stride = s->buf.ref.rhs_stride;
  K.rhs_rec = s->buf.ref.rhs_rec;
  K.threshold = threshold;
  return launch_kkt_pair(s, K);
}

// the refinement's right-hand side and output with their pitches and the gate words of the caller (the refinement's, or
// the adjoint's "status word zero"): what AffineParams and RefineParams share
template <class P> void fill_refine_io(const gar::RefineArea &r, const int *gate, P &p) {
  p.rhs = r.rhs, p.out = r.out, p.gate = gate;
  p.rhs_stride = r.rhs_stride, p.out_stride = r.out_stride;
  p.rhs_rec = r.rhs_rec, p.out_rec = r.out_rec;
}
// the parameter blocks of the redirected sweep, its initial stage and its roll-out
void make_refine_params(gar_hip_solver *s, const int *gate, gar::AffineParams &A, gar::RefineParams &R) {
  A = make_affine_params(s);
  fill_refine_io(s->buf.ref, gate, A);
  R = gar::RefineParams{};
  R.G = make_params(s, s->cur.mueq);
  fill_refine_io(s->buf.ref, gate, R);
  R.init = s->buf.ref.init, R.init_rec = s->buf.ref.init_rec;
  R.fb_t2 = A.fb_t2, R.nx_max = A.nx_max;
}

// the correction of the gated problems, added to the solution records
int launch_refine_correction(gar_hip_solver *s) {
  gar::AffineParams A;
  gar::RefineParams R;
  make_refine_params(s, s->buf.ref.gate, A, R);
  if (int rc = ensure_W(s, A))
    return rc;
  const dim3 grid((unsigned)s->batch), wave(64);
  hipLaunchKernelGGL(gar::gar_refine_sweep, grid, wave, s->buf.ref.sweep_lds_bytes, s->stream, A);
  hipLaunchKernelGGL(gar::gar_refine_initial, grid, wave, s->buf.ref.init_lds_bytes, s->stream, R);
  hipLaunchKernelGGL(gar::gar_refine_rollout, grid, wave, s->buf.ref.roll_lds_bytes, s->stream, R);
  HIP_TRY(hipGetLastError());
  return GAR_HIP_OK;
}

// ---- gradients of a resident batch (gar_adjoint.hpp): the caller's packed layout on the device, the adjoint solve -------
// a padded solver's caller-side knot offsets on the device (the caller's layout does not turn with the ring); an unpadded
// solver's are the device's own stage descriptors.  On its own first use: the user upload wants it before any adjoint.
int ensure_user_layout(gar_hip_solver *s) {
  if (!s->padded || s->buf.d_user_off)
    return GAR_HIP_OK;
  std::vector<long long> off;
  for (const gar_stage_meta &m : s->ulay->meta)
    off.push_back(m.in_off);
  DevBuf<long long> d;
  HIP_TRY(to_device(d, off));
  s->buf.d_user_off = std::move(d);
  return GAR_HIP_OK;
}

// (what the scatter, the gather, the gradient kernel and the user upload read of it: null where a work area is not built)
gar::AdjointParams make_adjoint_params(gar_hip_solver *s) {
  const gar::HostLayout &u = caller_layout(s);
  gar::AdjointParams P{};
  P.meta = s->buf.d_meta;
  fill_caller_vectors(s, P);
  P.U.in_off = s->padded ? s->buf.d_user_off.get() : nullptr;
  P.U.stride = u.prob_doubles, P.U.G0_off = u.G0_off, P.U.g0_off = u.g0_off;
  P.status = status_words(s);
  P.rhs = s->buf.ref.rhs;
  P.gate = s->buf.adj.gate;
  P.rhs_stride = s->buf.ref.rhs_stride;
  P.rhs_rec = s->buf.ref.rhs_rec;
  P.sol = s->buf.d_sol;
  P.adj = s->buf.adj.rec;
  P.sol_stride = s->sol_doubles;
  P.prob = s->buf.d_prob;
  P.prob_stride = s->prob_doubles, P.G0_off = s->G0_off, P.g0_off = s->g0_off;
  P.horizon = s->horizon, P.nc0 = s->nc0, P.nx0 = s->nx0;
  P.qr_packed = s->qr_packed ? 1 : 0;
  return P;
}

int ensure_adjoint(gar_hip_solver *s) {
  if (s->buf.adj.built())
    return GAR_HIP_OK;
  // the affine layout's offsets and W; the right-hand side, ff~ / vx~ and the initial stage's result; the gradient's layout
  for (auto prerequisite : {ensure_affine, ensure_refine, ensure_user_layout})
    if (int rc = prerequisite(s))
      return rc;
  int glds = 0;
  for (const gar_stage_meta &m : s->meta) // (the device's dimensions bound the caller's)
    glds = std::max(glds, gar::adjoint_grad_lds_doubles(m.nx, m.nu, m.nx2, s->nc0, s->nx0));
  if (int rc = lds_fits(glds, "gar_hip_adjoint: a knot of the gradient record needs"))
    return rc;
  HIP_TRY(max_lds(gar::gar_adjoint_gradients, (size_t)glds));
  HIP_TRY(max_lds(gar::gar_adjoint_rollout, s->buf.ref.roll_lds_bytes / sizeof(double)));
  gar::AdjointArea a;
  HIP_TRY(a.rec.zalloc((size_t)s->batch * (size_t)s->sol_doubles));
  HIP_TRY(a.gate.zalloc((size_t)s->batch));
  a.grad_lds_bytes = (size_t)glds * sizeof(double);
  s->buf.adj = std::move(a);
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
  make_refine_params(s, s->buf.adj.gate, A, R);
  gar::RefineParams Radj = R; // the roll-out's "solution" is the adjoint record
  Radj.G.sol = s->buf.adj.rec;
  if (int rc = ensure_W(s, A))
    return rc;
  gar::AdjointParams P = make_adjoint_params(s);
  P.cot = cot_dev;
  P.grad = grad_dev;
  const dim3 grid((unsigned)s->batch), stages((unsigned)s->batch * (unsigned)(s->horizon + 1)), wave(64);
  hipLaunchKernelGGL(gar::gar_adjoint_scatter, stages, wave, 0, s->stream, P);
  hipLaunchKernelGGL(gar::gar_refine_sweep, grid, wave, s->buf.ref.sweep_lds_bytes, s->stream, A);
  hipLaunchKernelGGL(gar::gar_refine_initial, grid, wave, s->buf.ref.init_lds_bytes, s->stream, R);
  hipLaunchKernelGGL(gar::gar_adjoint_rollout, grid, wave, s->buf.ref.roll_lds_bytes, s->stream, Radj);
  HIP_TRY(hipGetLastError());
  if (adj_dev)
    if (int rc = launch_solution_gather(s, 0, s->batch, s->buf.adj.rec, adj_dev))
      return rc;
  if (grad_dev) {
    hipLaunchKernelGGL(gar::gar_adjoint_gradients, stages, dim3(GAR_ADJ_THREADS), s->buf.adj.grad_lds_bytes, s->stream, P);
    HIP_TRY(hipGetLastError());
  }
  return GAR_HIP_OK;
}

// ---- many affine terms at once (gar_affine_multi.hpp): panel scatter, the MFMA sweep, the initial stage, the MFMA roll-out ----
int ensure_affine_multi(gar_hip_solver *s) {
  if (s->buf.am.built())
    return GAR_HIP_OK;
  if (int rc = ensure_affine(s)) // the chain vector's length, the affine layout's offsets, W
    return rc;
  const int nx_max = s->buf.aff.nx_max, N = s->horizon, C = GAR_AM_COLS;
  gar::AffineMultiArea a;
  int rows = 1, lds = 0, rlds = 0;
  for (const gar_stage_meta &m : s->meta)
    a.nu_max = std::max(a.nu_max, (int)m.nu);
  for (const gar_stage_meta &m : s->meta) {
    rows = std::max(rows, (int)(m.nx + m.nu + m.nx2));
    lds = std::max(lds, gar::affine_multi_sweep_lds_doubles(nx_max, a.nu_max, m.nx, m.nu, m.nx2, s->fb_t2, s->vxx_packed));
    rlds = std::max(rlds, gar::affine_multi_rollout_lds_doubles(nx_max, a.nu_max, m.nx, m.nu, m.nx2, s->fb_t2, s->vxx_packed));
  }
  const int ilds = gar::gar_initial_wave_lds_doubles(s->n0, s->nth0);
  if (int rc = lds_fits(std::max(lds, std::max(rlds, ilds)), "gar_hip_affine_solve_multi: a stage's blocks and panels need"))
    return rc;
  a.prhs_rec = a.pout_rec = C * rows;
  a.ivx_rec = std::max(2, (s->nx0 + 1) & ~1), a.ig0_rec = std::max(2, (s->nc0 + 1) & ~1), a.init_rec = std::max(2, (s->n0 + 1) & ~1);
  a.prhs_stride = a.pout_stride = (long long)(N + 1) * a.prhs_rec;
  // bytes of the work buffers of one panel of one problem (the header's formula): the two panel records of every stage and
  // the initial stage's three vectors of 16 columns
  const size_t per_panel =
      sizeof(double) * ((size_t)2 * (size_t)a.prhs_stride + (size_t)C * (size_t)(a.ivx_rec + a.ig0_rec + a.init_rec));
  // panels per problem in a chunk: enough workgroups for the device at a small batch, at most 1 GiB of work buffers
  a.panels = std::min(8, std::max(1, (1024 + s->batch - 1) / s->batch));
  while (a.panels > 1 && per_panel * (size_t)s->batch * (size_t)a.panels > ((size_t)1 << 30))
    --a.panels;
  if (int rc = grid_fits(s, (int64_t)a.panels * std::max(N + 1, C), "gar_hip_affine_solve_multi"))
    return rc;
  const size_t bp = (size_t)s->batch * (size_t)a.panels;
  hipError_t e = a.rhs.zalloc(bp * (size_t)a.prhs_stride);
  e = e != hipSuccess ? e : a.out.zalloc(bp * (size_t)a.pout_stride);
  e = e != hipSuccess ? e : a.ivx.zalloc(bp * C * (size_t)a.ivx_rec);
  e = e != hipSuccess ? e : a.ig0.zalloc(bp * C * (size_t)a.ig0_rec);
  e = e != hipSuccess ? e : a.ires.zalloc(bp * C * (size_t)a.init_rec);
  e = e != hipSuccess ? e : a.gate.zalloc((size_t)s->batch);
  if (e != hipSuccess) { // the one allocation large enough to fail in practice: reported with its size
    (void)hipGetLastError(); // (the error is reported here; the next launch check of this solver starts clean)
    return fail(GAR_HIP_ERR_DEVICE, "gar_hip_affine_solve_multi: " + std::to_string(per_panel * bp + sizeof(int) * (size_t)s->batch) +
                                        " B of work buffers: " + hipGetErrorString(e));
  }
  HIP_TRY(max_lds(gar::gar_affine_sweep_multi, (size_t)lds));
  HIP_TRY(max_lds(gar::gar_rollout_multi, (size_t)rlds));
  HIP_TRY(max_lds(gar::gar_affine_multi_initial, (size_t)ilds));
  a.sweep_lds_bytes = (size_t)lds * sizeof(double);
  a.roll_lds_bytes = (size_t)rlds * sizeof(double);
  a.init_lds_bytes = (size_t)ilds * sizeof(double);
  s->buf.am = std::move(a);
  return GAR_HIP_OK;
}

// columns [0, nrhs) of every problem: rhs_dev and out_dev are [batch][nrhs][affine doubles] at DEVICE addresses.  The host
// loops over chunks of `panels` panels; every kernel of a chunk is ordered behind the previous chunk's on the stream.
int launch_affine_multi(gar_hip_solver *s, int nrhs, const double *rhs_dev, double *out_dev) {
  RoctxRange range_("gar::affine_solve_multi");
  const gar::AffineMultiArea &a = s->buf.am;
  const gar::AffineParams A = make_affine_params(s);
  if (int rc = ensure_W(s, A))
    return rc;
  gar::AffineMultiParams P{};
  P.meta = s->buf.d_meta;
  fill_caller_vectors(s, P);
  P.status = status_words(s);
  P.prob = s->buf.d_prob, P.fac = s->buf.d_fac, P.W = s->buf.aff.W;
  P.prob_stride = s->prob_doubles, P.fac_stride = s->fac_doubles;
  P.w_rec = A.w_rec, P.horizon = s->horizon, P.nc0 = s->nc0;
  P.vxx_packed = A.vxx_packed, P.fb_t2 = A.fb_t2;
  P.nrhs = nrhs;
  P.rhs = rhs_dev, P.out = out_dev;
  P.prhs = a.rhs, P.pout = a.out;
  P.ivx = a.ivx, P.ig0 = a.ig0, P.ires = a.ires;
  P.gate = a.gate;
  P.prhs_stride = a.prhs_stride, P.pout_stride = a.pout_stride;
  P.prhs_rec = a.prhs_rec, P.pout_rec = a.pout_rec;
  P.ivx_rec = a.ivx_rec, P.ig0_rec = a.ig0_rec, P.init_rec = a.init_rec;
  P.nx_max = A.nx_max, P.nu_max = a.nu_max;
  gar::AffineMultiInit I{};
  I.G = make_params(s, s->cur.mueq);
  I.ivx = P.ivx, I.ig0 = P.ig0, I.ires = P.ires, I.gate = P.gate;
  I.ivx_rec = P.ivx_rec, I.ig0_rec = P.ig0_rec, I.init_rec = P.init_rec;
  const int C = GAR_AM_COLS, total = (nrhs + C - 1) / C;
  for (int p0 = 0; p0 < total; p0 += a.panels) {
    P.c0 = p0 * C;
    P.panels = I.panels = std::min(a.panels, total - p0);
    const unsigned groups = (unsigned)s->batch * (unsigned)P.panels;
    hipLaunchKernelGGL(gar::gar_affine_multi_scatter, dim3(groups * (unsigned)(s->horizon + 1)), dim3(GAR_AM_THREADS), 0,
                       s->stream, P);
    hipLaunchKernelGGL(gar::gar_affine_sweep_multi, dim3(groups), dim3(GAR_AM_THREADS), a.sweep_lds_bytes, s->stream, P);
    hipLaunchKernelGGL(gar::gar_affine_multi_initial, dim3(groups * (unsigned)C), dim3(64), a.init_lds_bytes, s->stream, I);
    hipLaunchKernelGGL(gar::gar_rollout_multi, dim3(groups), dim3(GAR_AM_THREADS), a.roll_lds_bytes, s->stream, P);
    HIP_TRY(hipGetLastError());
  }
  return GAR_HIP_OK;
}

// ---- the prologue of every entry point of these services ---------------------------------------------------------------
// (ptr, b0, nb) of an entry point that takes problems b0 .. b0 + nb - 1 at ptr (a null solver is affine_check's to refuse)
const char *bad_range(const gar_hip_solver *s, const void *ptr, int b0, int nb) {
  return s && (!ptr || b0 < 0 || nb < 0 || b0 + nb > s->batch) ? "bad argument" : nullptr;
}
enum { kNeedsSolution = 1, kSupersedesSolution = 2, kCommits = 4 };
// The refusals, in the one order every entry point keeps: (1) is the solver served?  (2) the entry point's own arguments
// (`bad_argument`: what is wrong with them, null: nothing)  (3) factors of the last backward to `verb` from (null: not
// needed)  (4) kNeedsSolution: a roll-out of that factorisation.  Then (5) the work areas, each ensure_* building what it
// needs before it, and (6) kCommits: staged host blocks go out (a g0 or G0 staged through gar_hip_set_init) --
// kSupersedesSolution: the entry point rewrites the solution in HBM, the host copy gar_hip_backward_blocks left is dropped.
int resident_begin(gar_hip_solver *s, const char *who, const char *bad_argument, const char *verb, unsigned flags,
                   std::initializer_list<int (*)(gar_hip_solver *)> areas) {
  if (int rc = affine_check(s, who))
    return rc;
  const std::string w(who);
  if (bad_argument)
    return fail(GAR_HIP_ERR_ARG, w + ": " + bad_argument);
  if (verb) {
    const std::string refusal = s->cur.no_factors(w, verb);
    if (!refusal.empty())
      return fail(GAR_HIP_ERR_ARG, refusal);
  }
  if ((flags & kNeedsSolution) && !s->cur.rolled_out)
    return fail(GAR_HIP_ERR_ARG, w + ": no forward since the last backward (there is no solution to " + verb + ")");
  for (auto ensure : areas)
    if (int rc = ensure(s))
      return rc;
  if (flags & kSupersedesSolution)
    s->cur.solution_superseded();
  return (flags & kCommits) ? commit(s) : GAR_HIP_OK;
}
