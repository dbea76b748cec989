// gar_adjoint.hpp -- differentiate a resident batch (gar_hip_adjoint; unconstrained knots, nc = 0, nth = 0): the adjoint
// solve from the stored factorisation and the gradient with respect to every block of the caller's packed problem.
//
// With K z = -b the KKT system of oracle/dense_kkt.py (z = (lbd0, x_t, u_t, lbd_{t+1} ...), b = (g0, q_t, r_t, f_t ...))
// and g = dL/dz the cotangent of a scalar loss, d = (dlbd0, dx_t, du_t, dlbd_{t+1} ...) is THE LQ SOLUTION FOR THE SAME
// MATRICES AND THE AFFINE TERMS g (K d = -g), and
//   dL/dq_t = dx_t   dL/dr_t = du_t   dL/df_t = dlbd_{t+1}   dL/dg0 = dlbd0
//   dL/dQ_t = 1/2 (dx x^T + x dx^T)   dL/dR_t = 1/2 (du u^T + u du^T)   dL/dS_t = dx u^T + x du^T
//   dL/dA_t = dlbd' x^T + lbd' dx^T   dL/dB_t = dlbd' u^T + lbd' du^T   dL/dG0  = dlbd0 x0^T + lbd0 dx0^T
// (Q, R as the symmetric matrices the solver reads: both triangles written, bitwise symmetric; the terminal knot has no
// A, B, f: zeros where its record keeps the slots).
//
// Five kernels, all through the stage descriptors (padding, the cycleAppend ring, packed triangles, a terminal knot kept
// as nx2 = nx); the sweep and the initial stage between the first two are gar_refine_sweep and gar_refine_initial as they
// are, gated by "status word zero":
//   gar_adjoint_scatter      grid (batch * (N + 1)) x 64: the caller's cotangent vector (the affine layout: per stage
//                            dx_t | du_t | dlbd_{t+1} slots, then dlbd0; the caller's dimensions) into the right-hand
//                            side of the refinement sweep (q~ | r~ | pad | f~, g0~ behind the last stage); the dummy
//                            entries of a padded solver are written as zeros; stage 0 writes the gate word
//   gar_adjoint_rollout      gar_rollout<true> (gar_refine.hpp): dx, du, dlbd STORED into the adjoint record (the
//                            solution record's layout); a record of zeros for a failed problem
//   gar_solution_gather      grid (nb * (N + 1)) x 64: a solution or adjoint record into a vector of the affine layout
//   gar_adjoint_gradients    grid (batch * (N + 1)) x 256, no chain: one knot of the gradient record in the CALLER's
//                            packed-problem layout from (x, u, lbd') and (dx, du, dlbd') of that stage.  Write-bound
//                            (29.5 KB out against 1.3 KB in at (36, 12)): the six vectors go to LDS, every entry is two
//                            products and an add from there (no integer division per entry: a thread steps its (row,
//                            column) by the block size), the knot is assembled as ONE LDS image and leaves it in
//                            coalesced 16-byte non-temporal stores from the even offsets of the record
//   gar_user_upload_scatter  grid (nb * (N + 1)) x 256: nb packed problems in the CALLER's layout into the device knots --
//                            gar_affine_scatter for every block: the lower triangles of Q / R packed where the family
//                            keeps them; under padding the dummy rows and columns are written as put_block
//                            (gar_record_io.hpp) writes them, so that a solver fed through this entry alone is complete
// Where stage t's blocks lie in the caller's packed problem is stated once: user_knot, below.
#pragma once
#include "gar_refine.hpp"

namespace gar {

// the caller's packed problem (gar_hip_upload_packed's layout): G0 | g0 | knots, each knot Q S R q r A B f, full blocks
struct UserLayout {
  const long long *in_off; // padded solvers: the caller's offset of knot t; null: the device's own (meta[t].in_off)
  long long stride, G0_off, g0_off;
  int unx, unu; // the caller's (nx, nu) of a padded solver (unx = 0: not padded)
  int nc0;      // the caller's nc0
};
struct UserKnot {
  int nx, nu, nx2;
  long long off;
  gar_knot_offsets o;
};
__device__ __forceinline__ UserKnot user_knot(const UserLayout &U, const gar_stage_meta &m, int t) {
  UserKnot k;
  const bool pad = U.unx > 0;
  k.nx = pad ? U.unx : m.nx;
  k.nu = pad ? (m.nu > 0 ? U.unu : 0) : m.nu;
  k.nx2 = pad ? (m.nx2 > 0 ? U.unx : 0) : m.nx2;
  k.off = U.in_off ? U.in_off[t] : m.in_off;
  k.o = gar_knot_layout(k.nx, k.nu, 0, k.nx2, 0);
  return k;
}

struct AdjointParams {
  const gar_stage_meta *meta;
  UserLayout U;
  const long long *vec_off; // [horizon + 2] offsets of stage t's x | u | lbd' slots in an affine-layout vector, then lbd0
  long long vec_stride;
  const int *status;
  // scatter
  const double *cot;
  double *rhs;
  int *gate;
  long long rhs_stride;
  int rhs_rec;
  // gather: rec (solution or adjoint records) -> vec
  const double *rec;
  double *vec;
  // gradients
  const double *sol, *adj;
  double *grad;
  long long sol_stride;
  // upload
  const double *user;
  double *prob;
  long long prob_stride, G0_off, g0_off;
  int horizon, nc0, nx0, b0, qr_packed; // (nc0, nx0: the device's)
};

// ---- the cotangent as the right-hand side ------------------------------------------------------------------------------
__global__ void __launch_bounds__(64) gar_adjoint_scatter(AdjointParams P) {
  const int N = P.horizon, lane = (int)threadIdx.x;
  const int t = (int)(blockIdx.x % (unsigned)(N + 1)), b = (int)(blockIdx.x / (unsigned)(N + 1));
  const gar_stage_meta m = P.meta[t];
  const UserKnot k = user_knot(P.U, m, t);
  const double *src = P.cot + (long long)b * P.vec_stride;
  const double *s = src + P.vec_off[t];
  double *problem = P.rhs + (long long)b * P.rhs_stride;
  double *rec = problem + (long long)t * P.rhs_rec;
  const int of = refine_rhs_f(m.nx, m.nu);
  const int nf = t == N ? 0 : k.nx2; // (the terminal knot has no dynamics: its slot, where the vector has one, is not read)
  for (int i = lane; i < m.nx; i += 64)
    rec[i] = i < k.nx ? s[i] : 0.0;
  for (int i = lane; i < m.nu; i += 64)
    rec[m.nx + i] = i < k.nu ? s[k.nx + i] : 0.0;
  for (int i = lane; i < m.nx2; i += 64)
    rec[of + i] = i < nf ? s[k.nx + k.nu + i] : 0.0;
  if (t == 0) {
    for (int i = lane; i < P.nc0; i += 64)
      problem[(long long)(N + 1) * P.rhs_rec + i] = i < P.U.nc0 ? src[P.vec_off[N + 1] + i] : 0.0;
    if (lane == 0)
      P.gate[b] = P.status[b] == 0 ? 1 : 0;
  }
}

// ---- the roll-out that keeps the adjoint as a result of its own --------------------------------------------------------
constexpr auto gar_adjoint_rollout = &gar_rollout<true>;

// ---- a solution or adjoint record as a vector of the affine layout ------------------------------------------------------
__global__ void __launch_bounds__(64) gar_solution_gather(AdjointParams P) {
  const int N = P.horizon, lane = (int)threadIdx.x;
  const int t = (int)(blockIdx.x % (unsigned)(N + 1)), bl = (int)(blockIdx.x / (unsigned)(N + 1));
  const gar_stage_meta m = P.meta[t];
  const UserKnot k = user_knot(P.U, m, t);
  const double *rec = P.rec + (long long)(P.b0 + bl) * P.sol_stride;
  double *dst = P.vec + (long long)bl * P.vec_stride;
  double *d = dst + P.vec_off[t];
  const int slot = (int)(P.vec_off[t + 1] - P.vec_off[t]) - k.nx - k.nu; // (0 for a terminal knot given with nx2 = 0)
  const int l_next = P.meta[t == N ? t : t + 1].l_off;
  for (int i = lane; i < k.nx; i += 64)
    d[i] = rec[m.x_off + i];
  for (int i = lane; i < k.nu; i += 64)
    d[k.nx + i] = rec[m.u_off + i];
  for (int i = lane; i < slot; i += 64)
    d[k.nx + k.nu + i] = t == N ? 0.0 : rec[l_next + i];
  if (t == 0)
    for (int i = lane; i < P.U.nc0; i += 64)
      dst[P.vec_off[N + 1] + i] = rec[m.l_off + i];
}

// ---- block fills without a division per entry ---------------------------------------------------------------------------
// dst[j * r + i] = f(i, j) over an r x c column-major block by `nthr` threads: a thread finds its first (i, j) by one
// division and steps by nthr = dj * r + di from there
template <class F> __device__ __forceinline__ void adj_fill(int r, int c, int tid, int nthr, F f) {
  const int n = r * c;
  if (n == 0)
    return;
  int j = tid / r, i = tid - j * r;
  const int dj = nthr / r, di = nthr - dj * r;
  for (int e = tid; e < n; e += nthr) {
    f(e, i, j);
    i += di, j += dj;
    if (i >= r)
      i -= r, ++j;
  }
}

// ---- the gradient record --------------------------------------------------------------------------------------------------
#define GAR_ADJ_THREADS 256
enum AdjStore { kAdjStore8 = 0, kAdjStore16 = 1, kAdjStore16Nt = 2 }; // (the forms measured, with their times)
constexpr int kAdjStoreKept = kAdjStore16Nt; // (the fastest of the three: the kernel never re-reads its output)
// LDS of one workgroup: the six vectors (and lbd0, dlbd0 with stage 0), then the image of a knot or of G0 | g0
__host__ __device__ inline int adjoint_grad_lds_doubles(int nx, int nu, int nx2, int nc0, int nx0) {
  const int knot = (int)((gar_knot_doubles(nx, nu, 0, nx2, 0) + 1) & ~1ll), head = (nc0 * nx0 + nc0 + 1) & ~1;
  return ((2 * (nx + nu + nx2 + nc0) + 1) & ~1) + (knot > head ? knot : head);
}
// n doubles (even) of the LDS image to 16-byte-aligned dst
template <int FORM> __device__ __forceinline__ void adj_store_image(double *dst, const double *img, int n, int tid) {
  if constexpr (FORM == kAdjStore8) {
    for (int e = tid; e < n; e += GAR_ADJ_THREADS)
      dst[e] = img[e];
  } else {
    gar_double2 *d2 = reinterpret_cast<gar_double2 *>(dst);
    const gar_double2 *s2 = reinterpret_cast<const gar_double2 *>(img);
    for (int e = tid; 2 * e < n; e += GAR_ADJ_THREADS) {
      if constexpr (FORM == kAdjStore16Nt)
        __builtin_nontemporal_store(s2[e], d2 + e);
      else
        d2[e] = s2[e];
    }
  }
}
template <int FORM> __device__ __forceinline__ void adjoint_gradients_block(const AdjointParams &P) {
  const int N = P.horizon, tid = (int)threadIdx.x, nthr = GAR_ADJ_THREADS;
  const int t = (int)(blockIdx.x % (unsigned)(N + 1)), b = (int)(blockIdx.x / (unsigned)(N + 1));
  const gar_stage_meta m = P.meta[t];
  const bool last = t == N;
  const UserKnot k = user_knot(P.U, m, t);
  const int nx = k.nx, nu = k.nu, n2 = k.nx2, nc0 = t == 0 ? P.U.nc0 : 0;
  const int l_next = P.meta[last ? t : t + 1].l_off;
  // a failed problem: every operand an exact zero, so every entry of its record is one (nothing of its solution is read)
  const bool live = P.status[b] == 0;
  const double *sol = P.sol + (long long)b * P.sol_stride, *adj = P.adj + (long long)b * P.sol_stride;
  double *x = gar_smem, *u = x + nx, *l = u + nu, *dx = l + n2, *du = dx + nx, *dl = du + nu, *l0 = dl + n2, *dl0 = l0 + nc0;
  double *img = gar_smem + ((2 * (nx + nu + n2 + nc0) + 1) & ~1);
  for (int i = tid; i < nx; i += nthr)
    x[i] = live ? sol[m.x_off + i] : 0.0, dx[i] = live ? adj[m.x_off + i] : 0.0;
  for (int i = tid; i < nu; i += nthr)
    u[i] = live ? sol[m.u_off + i] : 0.0, du[i] = live ? adj[m.u_off + i] : 0.0;
  for (int i = tid; i < n2; i += nthr) { // (no lbd' at the terminal knot: A, B, f of a record that keeps them are zeros)
    const bool on = live && !last;
    l[i] = on ? sol[l_next + i] : 0.0, dl[i] = on ? adj[l_next + i] : 0.0;
  }
  for (int i = tid; i < nc0; i += nthr)
    l0[i] = live ? sol[m.l_off + i] : 0.0, dl0[i] = live ? adj[m.l_off + i] : 0.0;
  __syncthreads();
  // ---- the knot: Q S R q r A B f, every block full and column-major, then the pad to an even length ----
  // (Q, R: entry (i, j) and entry (j, i) evaluate the same expression -- the larger index first -- so they agree bitwise)
  double *g = img + k.o.Q;
  adj_fill(nx, nx, tid, nthr, [=](int e, int i, int j) {
    const int a = i >= j ? i : j, c = i >= j ? j : i;
    g[e] = 0.5 * (dx[a] * x[c] + x[a] * dx[c]);
  });
  g = img + k.o.S;
  adj_fill(nx, nu, tid, nthr, [=](int e, int i, int j) { g[e] = dx[i] * u[j] + x[i] * du[j]; });
  g = img + k.o.R;
  adj_fill(nu, nu, tid, nthr, [=](int e, int i, int j) {
    const int a = i >= j ? i : j, c = i >= j ? j : i;
    g[e] = 0.5 * (du[a] * u[c] + u[a] * du[c]);
  });
  g = img + k.o.A;
  adj_fill(n2, nx, tid, nthr, [=](int e, int i, int j) { g[e] = dl[i] * x[j] + l[i] * dx[j]; });
  g = img + k.o.B;
  adj_fill(n2, nu, tid, nthr, [=](int e, int i, int j) { g[e] = dl[i] * u[j] + l[i] * du[j]; });
  for (int i = tid; i < nx; i += nthr)
    img[k.o.q + i] = dx[i];
  for (int i = tid; i < nu; i += nthr)
    img[k.o.r + i] = du[i];
  for (int i = tid; i < n2; i += nthr)
    img[k.o.f + i] = dl[i];
  if (tid == 0 && (k.o.total & 1))
    img[k.o.total] = 0.0;
  __syncthreads();
  double *out = P.grad + (long long)b * P.U.stride;
  adj_store_image<FORM>(out + k.off, img, (k.o.total + 1) & ~1, tid);
  if (t != 0)
    return;
  // ---- with stage 0: G0 | g0 and the pad behind them (the record's head) ----
  __syncthreads();
  const int nh = nc0 * nx + nc0;
  adj_fill(nc0, nx, tid, nthr, [=](int e, int i, int j) { img[e] = dl0[i] * x[j] + l0[i] * dx[j]; });
  for (int i = tid; i < nc0; i += nthr)
    img[nc0 * nx + i] = dl0[i];
  if (tid == 0 && (nh & 1))
    img[nh] = 0.0;
  __syncthreads();
  adj_store_image<FORM>(out + P.U.G0_off, img, (nh + 1) & ~1, tid);
}
__global__ void __launch_bounds__(GAR_ADJ_THREADS) gar_adjoint_gradients(AdjointParams P) {
  adjoint_gradients_block<kAdjStoreKept>(P);
}

// ---- the caller's packed problems into the device knots -------------------------------------------------------------------
// the caller's r x c block at `src` into the device's R x C one at `dst` (`lower`: its packed lower triangle); the dummy
// rows and columns of a padded block: `diag` on the entries (r + i, c + i), zeros elsewhere
__device__ __forceinline__ void adj_put_block(double *dst, int R, int C, const double *src, int r, int c, double diag,
                                              bool lower, int tid, int nthr) {
  adj_fill(R, C, tid, nthr, [=](int e, int i, int j) {
    const double v = (i < r && j < c) ? src[j * r + i] : ((i >= r && i - r == j - c) ? diag : 0.0);
    if (!lower)
      dst[e] = v;
    else if (i >= j)
      dst[gar_lower_index(R, i, j)] = v;
  });
}
__global__ void __launch_bounds__(GAR_ADJ_THREADS) gar_user_upload_scatter(AdjointParams P) {
  const int N = P.horizon, tid = (int)threadIdx.x, nthr = GAR_ADJ_THREADS;
  const int t = (int)(blockIdx.x % (unsigned)(N + 1)), bl = (int)(blockIdx.x / (unsigned)(N + 1));
  const gar_stage_meta m = P.meta[t];
  const UserKnot k = user_knot(P.U, m, t);
  const gar_knot_offsets o = gar_knot_layout(m.nx, m.nu, m.nc, m.nx2, 0);
  const double *user = P.user + (long long)bl * P.U.stride, *s = user + k.off;
  double *problem = P.prob + (long long)(P.b0 + bl) * P.prob_stride, *rec = problem + m.in_off;
  const bool lower = P.qr_packed && t < N;
  adj_put_block(rec + o.Q, m.nx, m.nx, s + k.o.Q, k.nx, k.nx, 1.0, lower, tid, nthr);
  adj_put_block(rec + o.S, m.nx, m.nu, s + k.o.S, k.nx, k.nu, 0.0, false, tid, nthr);
  adj_put_block(rec + o.R, m.nu, m.nu, s + k.o.R, k.nu, k.nu, 1.0, lower, tid, nthr);
  adj_put_block(rec + o.q, m.nx, 1, s + k.o.q, k.nx, 1, 0.0, false, tid, nthr);
  adj_put_block(rec + o.r, m.nu, 1, s + k.o.r, k.nu, 1, 0.0, false, tid, nthr);
  adj_put_block(rec + o.A, m.nx2, m.nx, s + k.o.A, k.nx2, k.nx, 0.0, false, tid, nthr);
  adj_put_block(rec + o.B, m.nx2, m.nu, s + k.o.B, k.nx2, k.nu, 0.0, false, tid, nthr);
  adj_put_block(rec + o.f, m.nx2, 1, s + k.o.f, k.nx2, 1, 0.0, false, tid, nthr);
  if (t == 0) { // [G0 0; 0 -I] | [g0; 0]
    adj_put_block(problem + P.G0_off, P.nc0, P.nx0, user + P.U.G0_off, P.U.nc0, k.nx, -1.0, false, tid, nthr);
    adj_put_block(problem + P.g0_off, P.nc0, 1, user + P.U.g0_off, P.U.nc0, 1, 0.0, false, tid, nthr);
  }
}

} // namespace gar
