// gar_refine.hpp -- one step of iterative refinement for every problem of a resident batch, from the stored
// factorisation (gar_hip_refine; unconstrained knots, nc = 0, nth = 0).  The reference refines only the condensed system
// of its parallel solver (parallel-solver.hxx:187-199); this is the same idea on the serial recursion.
//
//   rho   = the KKT residual VECTORS of the solution in HBM: q~ = gx, r~ = gu, f~ = A x + B u + f - x', g0~ = g0 + G0 x0
//           (gar_kkt.hpp: gar_kkt_stage_residuals with KktParams::rhs set; gar_kkt_reduce writes the gate words)
//   delta = the solution of the LQ problem with the SAME matrices and the affine terms rho:
//           the vector sweep   (gar_affine.hpp: gar_refine_sweep)   ff~ = [kff~; yff~], vx~ of every stage from fb, Vxx', W, B
//           the initial stage  (gar_refine_initial, below)          [Vxx0 G0^T; G0 0] [dx0; dl0] = -[vx~0; g0~]
//           the roll-out       (gar_refine_rollout, below)          du = kff~ + K dx, dx' = yff~ + Aff dx, dl' = vx~' + Vxx' dx'
//   xs, us, lbdas += delta
// Nothing of the knots or the factor records is written: rho, ff~, vx~ and the initial stage's result live in three side
// buffers, a record per stage at a uniform pitch (both halves of a record start on an even double: 16-byte pieces):
//   rhs[b][t * rhs_rec]: q~ (nx) | r~ (nu) | pad | f~ (nx2)    then g0~ (nc0) at [(N + 1) * rhs_rec]   (refine_rhs_f)
//   out[b][t * out_rec]: kff~ (nu) | yff~ (nx2) | pad | vx~ (nx)                                       (refine_out_vx)
//   init[b][init_rec]:   dx0 (nx) | dl0 (nc0)
// All three kernels leave a problem alone when gate[b] == 0: a failed backward (status != 0), a residual at or below the
// caller's threshold, a non-finite one.
//
// gar_refine_rollout: grid (batch) x 64, one wave per problem, sequential over the stages.  Stage t's blocks -- fb =
// [K; Aff] in the family's order, ff~, Vxx' (packed or full) and vx~' -- go HBM -> LDS by LDS-DMA in 16-byte pieces, all
// in flight before one wait (19.6 KB at (36, 12): eight waves share a CU); dx, du, dl are formed lane per row and ADDED
// to the solution record in place.  Run-time dimensions through the stage descriptors; no register array, no scratch.
// The dummy states and controls of a padded solver have exactly zero residuals and decoupled matrices: their
// corrections are sums of exact zeros and the entries stay exactly 0.0.
#pragma once
#include "gar_affine.hpp"
#include "gar_generic.hpp"

namespace gar {

struct RefineParams {
  GenericParams G; // meta, prob, fac, sol and their strides, G0_off, nc0, horizon, init_closed, vxx_packed (make_params)
  const double *rhs, *out;
  double *init;
  const int *gate;
  long long rhs_stride, out_stride, init_rec;
  int rhs_rec, out_rec, fb_t2, nx_max;
};

// ---- the initial stage of the correction: the family's stand-alone one on redirected vx0, g0 and result ---------------
// (kkt0 is factorised again, or the closed form taken, exactly as gar_initial_wave does for the solve itself; the matrix
// is the one the backward factorised, so the status word has nothing to learn and is not written)
__global__ void __launch_bounds__(64) gar_refine_initial(RefineParams R) {
  const WG w = wave_self();
  const int b = (int)blockIdx.x;
  if (R.gate[b] == 0)
    return;
  const gar_stage_meta m0 = R.G.meta[0];
  const double *vx0 = R.out + (long long)b * R.out_stride + refine_out_vx(m0.nu, m0.nx2);
  const double *g0 = R.rhs + (long long)b * R.rhs_stride + (long long)(R.G.horizon + 1) * R.rhs_rec;
  (void)initial_wave_problem(w, R.G, b, vx0, g0, R.init + (long long)b * R.init_rec);
}

// ---- the roll-out of the correction -----------------------------------------------------------------------------------
__host__ __device__ inline int refine_rollout_lds_doubles(int nx_max, int nx, int nu, int nx2, int fb_t2, int vxx_packed) {
  const int nr = nu + nx2, nvv = vxx_packed ? nx2 * (nx2 + 1) / 2 : nx2 * nx2;
  const int fb = fb_t2 ? ((nx + 1) / 2) * (2 * nr + 2) : nr * nx;
  return 2 * ((nx_max + 1) & ~1) + (fb + 2) + (nr + 2) + (nvv + 2) + (nx2 + 2);
}
// One kernel template, two instances.  gar_rollout<false> is gar_refine_rollout.  gar_rollout<true> is gar_adjoint_rollout
// (gar_adjoint.hpp): the same recursion with dx, du, dl STORED instead of added -- R.G.sol then names the adjoint records
// (the solution records' layout and pitch) -- and a record of exact zeros for a problem the gate leaves out.  (The body
// stands in the kernel itself, not in a device function the kernel calls: that is what keeps the instructions of the
// <false> instance those of the kernel it replaces.)
#define GAR_ROLLOUT_PUT(p, v)                                                                                            \
  do {                                                                                                                   \
    if constexpr (ADJOINT)                                                                                               \
      (p) = (v);                                                                                                         \
    else                                                                                                                 \
      (p) += (v);                                                                                                        \
  } while (0)
template <bool ADJOINT> __global__ void __launch_bounds__(64) gar_rollout(RefineParams R) {
  const int b = (int)blockIdx.x, lane = (int)threadIdx.x, N = R.G.horizon;
  if (R.gate[b] == 0) {
    if constexpr (ADJOINT)
      for (long long e = lane; e < R.G.sol_stride; e += 64)
        R.G.sol[(long long)b * R.G.sol_stride + e] = 0.0;
    return;
  }
  const double *factors = R.G.fac + (long long)b * R.G.fac_stride;
  const double *outb = R.out + (long long)b * R.out_stride;
  double *sol = R.G.sol + (long long)b * R.G.sol_stride;
  const int pk = R.G.vxx_packed, half = (R.nx_max + 1) & ~1;
  double *dx = gar_smem, *dxn = gar_smem + half;
  { // dx0, dl0 of the initial stage
    const gar_stage_meta m0 = R.G.meta[0];
    const double *io = R.init + (long long)b * R.init_rec;
    for (int i = lane; i < m0.nx; i += 64) {
      const double v = io[i];
      dx[i] = v;
      GAR_ROLLOUT_PUT(sol[m0.x_off + i], v);
    }
    for (int k = lane; k < R.G.nc0; k += 64)
      GAR_ROLLOUT_PUT(sol[m0.l_off + k], io[m0.nx + k]);
  }
  wave_sync();
  for (int t = 0; t <= N; ++t) {
    const gar_stage_meta m = R.G.meta[t];
    const bool last = t == N;
    const gar_stage_meta mn = R.G.meta[last ? t : t + 1];
    const int nx = m.nx, nu = m.nu, n2 = last ? 0 : m.nx2, nr = m.nu + m.nc + m.nx2;
    const int rows = last ? nu : nr; // (the terminal record: K alone)
    const bool t2 = R.fb_t2 && !last;
    const int pitch = 2 * nr + 2;
    const gar_factor_offsets fo = gar_factor_layout(m.nx, m.nu, m.nc, m.nx2, m.nth);
    const gar_factor_offsets fn = gar_factor_layout(mn.nx, mn.nu, mn.nc, mn.nx2, mn.nth);
    const int nvv = pk ? n2 * (n2 + 1) / 2 : n2 * n2;
    // ---- this stage's blocks: HBM -> LDS, every piece in flight before the one wait (aff_describe's parity rule) ----
    int p = 2 * half;
    auto fetch = [&p, lane](const double *rec, int a, int n, int lds_doubles) {
      const int o0 = p + (a & 1);
      aff_dma(reinterpret_cast<const gar_double2 *>(rec + (a & ~1)), p, aff_span(a, n) / 2, lane);
      p += lds_doubles;
      return o0;
    };
    int oFb;
    if (t2) { // pair block c of nr pieces to c * pitch
      const gar_double2 *src = reinterpret_cast<const gar_double2 *>(factors + m.fac_off + (fo.fb & ~1));
      oFb = p + (fo.fb & 1);
      for (int c = 0; 2 * c < nx; ++c)
        aff_dma(src + c * nr, p + c * pitch, nr, lane);
      p += ((nx + 1) / 2) * pitch;
    } else {
      oFb = fetch(factors + m.fac_off, fo.fb, rows * nx, aff_span(fo.fb, rows * nx));
    }
    const int oFf = fetch(outb + (long long)t * R.out_rec, 0, nu + n2, aff_span(0, nu + n2));
    const int oV = fetch(factors + mn.fac_off, fn.Vxx, nvv, aff_span(fn.Vxx, nvv));
    const int ovx = refine_out_vx(mn.nu, mn.nx2);
    const int oVx = fetch(outb + (long long)(t + 1) * R.out_rec, ovx, n2, aff_span(ovx, n2));
    GAR_WAIT_VMCNT(0);
    wave_sync();
    const double *fbs = gar_smem + oFb, *ffs = gar_smem + oFf, *Vs = gar_smem + oV, *vxs = gar_smem + oVx;
    // ---- du = kff~ + K dx (rows < nu), dx' = yff~ + Aff dx (rows >= nu + nc): lane per row ----
    for (int r = lane; r < nu + n2; r += 64) {
      const int row = r < nu ? r : r + m.nc;
      double acc = ffs[r];
      if (t2) {
        const double *rp = fbs + 2 * row; // element (row, j) at (j / 2) pitch + 2 row + (j & 1)
#pragma unroll 12
        for (int j = 0; j < nx; ++j)
          acc += rp[(j >> 1) * pitch + (j & 1)] * dx[j];
      } else {
        const double *rp = fbs + row * nx;
#pragma unroll 12
        for (int j = 0; j < nx; ++j)
          acc += rp[j] * dx[j];
      }
      if (r < nu) {
        GAR_ROLLOUT_PUT(sol[m.u_off + r], acc);
      } else {
        dxn[r - nu] = acc;
        GAR_ROLLOUT_PUT(sol[mn.x_off + (r - nu)], acc);
      }
    }
    wave_sync();
    // ---- dl' = vx~' + Vxx' dx': element (i, j) of the lower triangle at F(min) + max ----
    for (int i = lane; i < n2; i += 64) {
      double acc = vxs[i];
      const int fi = pk ? (2 * i < n2 ? i * n2 : (n2 - 1 - i) * (n2 + 1) + 1) : i * n2;
#pragma unroll 12
      for (int j = 0; j < n2; ++j) {
        const int fj = pk ? (2 * j < n2 ? j * n2 : (n2 - 1 - j) * (n2 + 1) + 1) : j * n2;
        acc += Vs[i >= j ? fj + i : fi + j] * dxn[j];
      }
      GAR_ROLLOUT_PUT(sol[mn.l_off + i], acc);
    }
    double *tmp = dx;
    dx = dxn;
    dxn = tmp;
    GAR_WAIT_LGKMCNT0(); // (every LDS read of this stage has returned before the next stage's pieces land)
    wave_sync();
  }
}
#undef GAR_ROLLOUT_PUT
constexpr auto gar_refine_rollout = &gar_rollout<false>; // the correction of a refinement step, added in place

} // namespace gar
