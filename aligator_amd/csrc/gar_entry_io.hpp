// gar_entry_io.hpp -- the caller-facing entry points that convert between the caller's blocks and the device's records:
// gar_hip_upload_stage, gar_hip_set_init and the per-stage getters (gains, value function, kktMat, initial stage,
// solution), each ONE body for padded and unpadded solvers over the block maps of gar_record_io.hpp; behind them the
// condensed-solve queries, the device-layout getters and the debug counters (inside extern "C").
// Part of the ONE translation unit gar_hip.cpp (included in place: it uses the solver struct and the helpers defined
// above its include line); split out for readability only.
#pragma once

int gar_hip_upload_stage(gar_hip_solver *s, int b, int t, const double *Q, const double *S, const double *R,
                         const double *q, const double *r, const double *A, const double *B, const double *f,
                         const double *C, const double *D, const double *d, const double *Gth, const double *Gx,
                         const double *Gu, const double *Gv, const double *gamma) {
  GAR_GUARD(s);
  if (int rc = check_bt(s, b, t))
    return rc;
  GAR_MULTI(s, gar_hip_upload_stage(multi_owner(s, t), b, t, Q, S, R, q, r, A, B, f, C, D, d, Gth, Gx, Gu, Gv, gamma));
  s->cur.matrices_changed("gar_hip_upload_stage");
  if (s->term_grown && t == s->horizon) // the caller's terminal A (0 x nx) and f are empty: zeros in the record
    A = f = s->term_zeros.data();
  const gar_stage_meta &u = caller_layout(s).meta[t], &m = s->meta[t];
  if (!Q || !q || !A || !f || (u.nu > 0 && (!S || !R || !r || !B)))
    return fail(GAR_HIP_ERR_ARG, "gar_hip_upload_stage: null block");
  const int nth_st = (m.flags & GAR_KNOT_HAS_PARAM) ? m.nth : 0;
  BlockMap maps[16];
  knot_block_maps(maps, u, m, nth_st, s->qr_packed && t < s->horizon);
  const double *const src[16] = {Q, S, R, q, r, A, B, f, C, D, d, Gth, Gx, Gu, Gv, gamma};
  return write_blocks(s, b, m.in_off, gar_knot_doubles(m.nx, m.nu, m.nc, m.nx2, nth_st), maps, src, 16);
}

int gar_hip_set_init(gar_hip_solver *s, int b, const double *G0, const double *g0) {
  GAR_GUARD(s);
  if (int rc = check_bt(s, b, 0))
    return rc;
  GAR_MULTI(s, multi_set_init(s, b, G0, g0));
  if (s->user_nc0 > 0 && (!G0 || !g0))
    return fail(GAR_HIP_ERR_ARG, "gar_hip_set_init: null block");
  const gar::HostLayout &u = caller_layout(s);
  BlockMap maps[2];
  init_block_maps(maps, u.nc0, u.nx0, s->nc0, s->nx0, s->G0_off, s->g0_off, u.G0_off, u.g0_off);
  const double *const src[2] = {G0, g0};
  return write_blocks(s, b, 0, s->g0_off + s->nc0, maps, src, 2);
}

int gar_hip_set_condensed_backward_ok(gar_hip_solver *s, double omega) {
  if (!s || !(omega >= 0.0))
    return fail(GAR_HIP_ERR_ARG, "bad backward-error bound");
  s->cond_backward_ok = omega;
  GAR_MULTI(s, multi_all(s, [&](gar_hip_solver *q) { return gar_hip_set_condensed_backward_ok(q, omega); }));
  return GAR_HIP_OK;
}

#ifdef GAR_CTRACE
extern "C" int gar_hip_debug_ctrace(long long *out) {
  long long z[16] = {0};
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(gar::g_ctrace), sizeof(z)) != hipSuccess) return 1;
  if (hipMemcpyToSymbol(HIP_SYMBOL(gar::g_ctrace), z, sizeof(z)) != hipSuccess) return 2;
  return 0;
}
extern "C" int gar_hip_debug_ptrace(long long *out) {
  long long z[16] = {0};
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(gar::g_ptrace), sizeof(z)) != hipSuccess) return 1;
  if (hipMemcpyToSymbol(HIP_SYMBOL(gar::g_ptrace), z, sizeof(z)) != hipSuccess) return 2;
  return 0;
}
extern "C" int gar_hip_debug_crtrace(long long *out) {
  long long z[16] = {0};
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(gar::g_crtrace), sizeof(z)) != hipSuccess) return 1;
  if (hipMemcpyToSymbol(HIP_SYMBOL(gar::g_crtrace), z, sizeof(z)) != hipSuccess) return 2;
  return 0;
}
#endif
int gar_hip_condensed_resolved(gar_hip_solver *s, int b, int *out) {
  GAR_GUARD(s);
  if (int rc = check_bt(s, b, 0))
    return rc;
  GAR_MULTI(s, gar_hip_condensed_resolved(s->multi->subs[0], b, out));
  if (s->num_legs < 2 || !out)
    return fail(GAR_HIP_ERR_ARG, "condensed info needs leg mode");
  const double *info = s->buf.d_cscratch + (int64_t)b * s->cscratch_doubles + cond_info_off(s);
  double v = 0.0;
  if (int rc = d2h(s, &v, info + 3, 1))
    return rc;
  HIP_TRY(hipStreamSynchronize(s->stream));
  *out = v != 0.0 ? 1 : 0;
  return GAR_HIP_OK;
}

int gar_hip_condensed_backward_error(gar_hip_solver *s, int b, double *out) {
  GAR_GUARD(s);
  if (int rc = check_bt(s, b, 0))
    return rc;
  GAR_MULTI(s, gar_hip_condensed_backward_error(s->multi->subs[0], b, out));
  if (s->num_legs < 2 || !out)
    return fail(GAR_HIP_ERR_ARG, "condensed info needs leg mode");
  const double *info = s->buf.d_cscratch + (int64_t)b * s->cscratch_doubles + cond_info_off(s);
  double v[3] = {0.0, 0.0, 0.0};
  if (int rc = d2h(s, v, info, 3))
    return rc;
  HIP_TRY(hipStreamSynchronize(s->stream));
  *out = v[2] > 0.0 ? v[0] / v[2] : 0.0;
  return GAR_HIP_OK;
}

int gar_hip_get_solution(gar_hip_solver *s, int b, double *xs, double *us, double *vs, double *lbdas) {
  GAR_GUARD(s);
  if (int rc = check_bt(s, b, 0))
    return rc;
  GAR_MULTI(s, multi_get_solution(s, b, xs, us, vs, lbdas));
  if (!s->padded)
    return get_solution_dev(s, b, xs, us, vs, lbdas);
  std::vector<double> rec((size_t)s->sol_doubles);
  HIP_TRY(hipMemcpyAsync(rec.data(), s->buf.d_sol + (int64_t)b * s->sol_doubles, sizeof(double) * rec.size(),
                         hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  strip_solution(s, rec.data(), xs, us, vs, lbdas);
  return GAR_HIP_OK;
}

int gar_hip_get_gains(gar_hip_solver *s, int b, int t, double *ff, double *fb, double *fth) {
  GAR_GUARD(s);
  if (int rc = check_bt(s, b, t))
    return rc;
  GAR_MULTI(s, gar_hip_get_gains(multi_owner(s, t), b, t, ff, fb, fth));
  const gar_stage_meta &m = s->meta[t];
  const int nx2r = s->dense ? 2 * m.nx2 : m.nx2; // stage-dense solver: rows [K; Z; L; Y]
  const int NR = m.nu + m.nc + nx2r, NX = m.nx, NT = m.nth;
  // the caller's rows and columns: all of them; under padding the real controls and states; of a terminal knot given
  // with nx2 = 0 the nc rows [zff | Z | Zth] that lead the record's (a padded solver has nc = 0: nothing to hand back)
  RowMap rows{NR, NR, 0};
  int nx = NX, nt = NT;
  if (s->term_grown && t == s->horizon) {
    if (m.nc == 0 || s->padded)
      return GAR_HIP_OK;
    rows = RowMap{m.nc, m.nc, 0};
  } else if (s->padded) {
    const int nu = m.nu > 0 ? s->unu : 0;
    rows = RowMap{nu + s->unx, nu, m.nu - nu};
    nx = s->unx;
    nt = NT > 0 ? nx : 0;
  }
  if (int rc = ensure_expanded(s))
    return rc;
  const gar_factor_offsets o = gar_factor_layout(NX, m.nu, m.nc, nx2r, NT);
  std::vector<double> rec((size_t)o.Vxx); // ff | fb | fth lead the factor record: one copy
  if (int rc = d2h(s, rec.data(), s->buf.d_fac + (int64_t)b * s->fac_doubles + m.fac_off, o.Vxx))
    return rc;
  HIP_TRY(hipStreamSynchronize(s->stream));
  // the specialised kernel families keep fb (and fth) in the fbT2 device order; back to StageFactor's row-major
  // [K; Z; Aff] (riccati-kernel.hpp:96-97)
  const bool t2 = records_t2(s, b) && t < s->horizon;
  take_gains(ff, rec.data() + o.ff, false, NR, 1, rows, 1);
  take_gains(fb, rec.data() + o.fb, t2, NR, NX, rows, nx);
  take_gains(fth, rec.data() + o.fth, t2, NR, NT, rows, nt);
  return GAR_HIP_OK;
}

int gar_hip_get_value(gar_hip_solver *s, int b, int t, double *Vxx, double *vx, double *Vxt, double *Vtt,
                      double *vt) {
  GAR_GUARD(s);
  if (int rc = check_bt(s, b, t))
    return rc;
  GAR_MULTI(s, gar_hip_get_value(multi_owner(s, t), b, t, Vxx, vx, Vxt, Vtt, vt));
  if (int rc = ensure_expanded(s))
    return rc;
  const gar_stage_meta &m = s->meta[t];
  const gar_factor_offsets o = gar_factor_layout(m.nx, m.nu, m.nc, s->dense ? 2 * m.nx2 : m.nx2, m.nth);
  const int NX = m.nx, NT = m.nth, nx = s->padded ? s->unx : NX, nt = s->padded ? (NT > 0 ? nx : 0) : NT;
  std::vector<double> rec((size_t)(o.total - o.Vxx)); // Vxx | vx | Vxt | Vtt | vt close the factor record: one copy
  if (int rc = d2h(s, rec.data(), s->buf.d_fac + (int64_t)b * s->fac_doubles + m.fac_off + o.Vxx, o.total - o.Vxx))
    return rc;
  HIP_TRY(hipStreamSynchronize(s->stream));
  // (the serial one-wave family keeps the lower triangle of Vxx, packed: gar_layout.h)
  const struct { double *dst; BlockMap map; } out[5] = {
      {Vxx, {nx, nx, NX, NX, 0, 0, 0.0, s->vxx_packed ? kSym : kFull}},
      {vx, {nx, 1, NX, 1, o.vx - o.Vxx, 0, 0.0, kFull}},
      {Vxt, {nx, nt, NX, NT, o.Vxt - o.Vxx, 0, 0.0, kFull}},
      {Vtt, {nt, nt, NT, NT, o.Vtt - o.Vxx, 0, 0.0, kFull}},
      {vt, {nt, 1, NT, 1, o.vt - o.Vxx, 0, 0.0, kFull}}};
  for (const auto &e : out)
    if (e.dst)
      take_block(e.dst, e.map, rec.data());
  return GAR_HIP_OK;
}

int gar_hip_get_kkt(gar_hip_solver *s, int b, int t, double mueq, double *out) {
  GAR_GUARD(s);
  if (int rc = check_bt(s, b, t))
    return rc;
  GAR_MULTI(s, gar_hip_get_kkt(multi_owner(s, t), b, t, mueq, out));
  if (s->dense)
    return fail(GAR_HIP_ERR_UNSUPPORTED, "kktMat of the stage-dense solver is not kept (the whole stage matrix: gar_dense.hpp)");
  if (!out)
    return fail(GAR_HIP_ERR_ARG, "null output");
  if (int rc = ensure_expanded(s))
    return rc;
  const gar_stage_meta &m = s->meta[t];
  const int nk = m.nu + m.nc;
  if (nk == 0)
    return GAR_HIP_OK;
  if ((int64_t)nk * nk > s->buf.kkt_doubles) {
    s->buf.kkt_doubles = 0;
    HIP_TRY(s->buf.d_kkt.alloc((size_t)nk * nk)); // (lets the smaller one go first)
    s->buf.kkt_doubles = (int64_t)nk * nk;
  }
  if (commit(s) != GAR_HIP_OK)
    return GAR_HIP_ERR_DEVICE;
  const int nth_st = (m.flags & GAR_KNOT_HAS_PARAM) ? m.nth : 0;
  const gar_knot_offsets ko = gar_knot_layout(m.nx, m.nu, m.nc, m.nx2, nth_st);
  const double *knot = s->buf.d_prob + (int64_t)b * s->prob_doubles + m.in_off;
  // the stage's value-function term: none at the terminal knot and at the last knot of a leg (each leg ends
  // with terminalSolve, parallel-solver.hxx:150-160)
  const double *Vn = nullptr;
  if (t < s->horizon && !(m.flags & GAR_KNOT_LEG_END) && m.nu > 0) {
    const gar_stage_meta &mn = s->meta[t + 1];
    const gar_factor_offsets fn = gar_factor_layout(mn.nx, mn.nu, mn.nc, mn.nx2, mn.nth);
    Vn = s->buf.d_fac + (int64_t)b * s->fac_doubles + mn.fac_off + fn.Vxx;
  }
  hipLaunchKernelGGL(gar::gar_kkt_matrix, dim3(1), dim3(256), 0, s->stream, knot, ko, Vn, m.nx2, m.nu, m.nc, mueq,
                     s->buf.d_kkt.get(), s->vxx_packed ? 1 : 0, (s->qr_packed && t < s->horizon) ? 1 : 0);
  HIP_TRY(hipGetLastError());
  std::vector<double> K((size_t)nk * nk);
  if (int rc = d2h(s, K.data(), s->buf.d_kkt, (int64_t)nk * nk))
    return rc;
  HIP_TRY(hipStreamSynchronize(s->stream));
  const int n = s->padded ? s->unu : nk; // (a padded solver is unconstrained: the real controls' corner)
  take_block(out, BlockMap{n, n, nk, nk, 0, 0, 0.0, kFull}, K.data());
  return GAR_HIP_OK;
}

int gar_hip_get_initial(gar_hip_solver *s, int b, double *kkt0_ff, double *kkt0_fth, double *thGrad,
                        double *thHess) {
  GAR_GUARD(s);
  if (int rc = check_bt(s, b, 0))
    return rc;
  GAR_MULTI(s, gar_hip_get_initial(s->multi->subs[0], b, kkt0_ff, kkt0_fth, thGrad, thHess));
  const int n0 = s->n0, NT = s->nth0, NX = s->nx0;
  // kkt0.ff = [x0; lbd0]: under padding the real entries of each part
  const int nx = s->padded ? s->unx : NX, nt = s->padded ? (NT > 0 ? nx : 0) : NT;
  const RowMap rows = s->padded ? RowMap{nx + s->user_nc0, nx, NX - nx} : RowMap{n0, n0, 0};
  const int64_t o_fth = n0, o_g = o_fth + (int64_t)n0 * NT, o_H = o_g + NT, total = o_H + (int64_t)NT * NT;
  std::vector<double> rec((size_t)total);
  if (int rc = d2h(s, rec.data(), s->buf.d_init + (int64_t)b * s->init_doubles, total))
    return rc;
  HIP_TRY(hipStreamSynchronize(s->stream));
  take_gains(kkt0_ff, rec.data(), false, n0, 1, rows, 1);
  take_gains(kkt0_fth, rec.data() + o_fth, false, n0, NT, rows, nt);
  if (thGrad)
    take_block(thGrad, BlockMap{nt, 1, NT, 1, o_g, 0, 0.0, kFull}, rec.data());
  if (thHess)
    take_block(thHess, BlockMap{nt, nt, NT, NT, o_H, 0, 0.0, kFull}, rec.data());
  return GAR_HIP_OK;
}

/* ---- the device side of a (possibly padded) solver, for device-resident producers and consumers ---------------- */
int gar_hip_device_stage_layout(const gar_hip_solver *s, int t, int64_t out[11]) {
  if (int rc = check_bt(s, 0, t))
    return rc;
  const gar_stage_meta &m = s->meta[t];
  out[0] = m.nx; out[1] = m.nu; out[2] = m.nc; out[3] = m.nx2; out[4] = s->dims5[5 * (size_t)t + 4];
  out[5] = m.in_off; out[6] = m.fac_off; out[7] = m.x_off; out[8] = m.u_off; out[9] = m.v_off; out[10] = m.l_off;
  return GAR_HIP_OK;
}

gar_hip_solver *gar_hip_multi_create(int ndev, const int *dev_ids, int horizon, const int32_t *dims5, int nc0, int batch,
                                     int num_legs) {
  return multi_create(ndev, dev_ids, horizon, dims5, nc0, batch, num_legs);
}

int gar_hip_num_devices(const gar_hip_solver *s) { return !s ? 0 : (s->multi ? (int)s->multi->subs.size() : 1); }

int gar_hip_stage_device(const gar_hip_solver *s, int t) {
  if (int rc = check_bt(s, 0, t))
    return rc;
  return s->multi ? s->multi->subs[(size_t)s->multi->owner[(size_t)t]]->device : s->device;
}

const char *gar_hip_multi_exchange_name(const gar_hip_solver *s) {
  return (s && s->multi) ? (s->multi->pull ? "pull" : "copy") : "";
}

long long gar_hip_debug_alloc_count(void) { return g_alloc_count.load(std::memory_order_relaxed); }

int gar_hip_device_sizes(const gar_hip_solver *s, int64_t out[8]) {
  if (!s || !out)
    return fail(GAR_HIP_ERR_ARG, "bad argument");
  out[0] = s->prob_doubles; out[1] = s->fac_doubles; out[2] = s->sol_doubles; out[3] = s->nc0;
  out[4] = s->G0_off; out[5] = s->g0_off; out[6] = s->padded ? 1 : 0; out[7] = s->init_doubles;
  return GAR_HIP_OK;
}

int gar_hip_packed_stage_dims(const gar_hip_solver *s, int t, int32_t out[5]) {
  if (!s || !out || t < 0 || t > s->horizon)
    return fail(GAR_HIP_ERR_ARG, "gar_hip_packed_stage_dims: bad argument");
  std::copy(&s->user_dims5[5 * (size_t)t], &s->user_dims5[5 * (size_t)t] + 5, out);
  return GAR_HIP_OK;
}

int gar_hip_device_record_format(const gar_hip_solver *s) {
  if (!s)
    return 0;
  return (s->qr_packed ? GAR_HIP_FMT_QR_PACKED : 0) | (s->vxx_packed ? GAR_HIP_FMT_VXX_PACKED : 0) |
         (s->fb_t2 ? GAR_HIP_FMT_FB_T2 : 0);
}

