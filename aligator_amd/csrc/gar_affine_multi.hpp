// gar_affine_multi.hpp -- solve a resident batch for MANY affine terms at once (gar_hip_affine_solve_multi; unconstrained
// knots, nc = 0, nth = 0): the vector half of the Riccati recursion (gar_affine.hpp) and the roll-out (gar_refine.hpp) with
// the right-hand sides of one problem side by side as the columns of a PANEL of 16, so that every mat-vec of the
// single-column path is a (matrix) x (n x 16 panel) product on v_mfma_f64_16x16x4_f64 tiles and a stage's matrices are
// fetched once per 16 columns.  DESIGN.md 5.3f.
//
// A panel is row-major at a pitch of 16 doubles: entry (row i, column j) at 16 i + j -- the B operand of the MFMA (lane l
// holds B[k = l >> 4][j = l & 15]) reads 64 consecutive doubles, the accumulator (lane l, register r: row (l >> 4) + 4 r,
// column l & 15) stores 16 consecutive ones.  For t = N ... 0, with Q, R, F the panels of the caller's q, r, f columns:
//   Vplus = Vx' + Vxx' F      Rhat = R + B^T Vplus      Kff = -W Rhat      Yff = F + B Kff      Vx = Q + fb^T [R; Vplus]
// (the terminal knot: Rhat = R, W = R^-1, Vx = Q + K^T R, no Yff), then the initial stage per (problem, column), then for
// t = 0 ... N
//   [dU; dX'] = [Kff; Yff] + [K; Aff] dX      dL' = Vx' + Vxx' dX'
// Nothing of the primal is read but the matrices (fb, Vxx', W, B) and nothing of it is written.  The work buffers hold ONE
// CHUNK of panels (P panels of every problem, P fixed by the batch on the first call); the host loops over chunks:
//   prhs[b P + p][t * prhs_rec]: [Q (nx) | R (nu) | F (nx2)] x 16
//   pout[b P + p][t * pout_rec]: [Kff (nu) | Yff (nx2) | Vx (nx)] x 16
//   ivx, ig0, ires[(b P + p) 16 + j]: vx0 (nx0), g0 (nc0) and the initial stage's result dx0 | dl0 of column j, contiguous
//                                (initial_wave_problem takes plain vectors)
//
// Four kernels, all through the stage descriptors (padding, the cycleAppend ring, packed triangles, the fbT2 order, a
// terminal knot kept as nx2 = nx):
//   gar_affine_multi_scatter  grid (batch * P * (N + 1)) x 256: the caller's vectors [batch][nrhs][affine layout] transposed
//                             into one stage's panel record; the dummy entries of a padded solver and the columns beyond
//                             nrhs of the tail panel are WRITTEN as zeros; stage 0 writes g0 and the gate word
//   gar_affine_sweep_multi    grid (batch * P) x 256: one workgroup of four waves per (problem, panel), sequential over
//                             the stages.  Matrices and the stage's panel record go HBM -> LDS by LDS-DMA in 16-byte
//                             pieces (aff_describe's ranges and parity rule), all in flight before one wait; the five
//                             products are MFMA tiles dealt to the waves by tile row; Vx' stays in LDS
//   gar_affine_multi_initial  grid (batch * P * 16) x 64: initial_wave_problem on redirected vx0, g0 and result
//   gar_rollout_multi         grid (batch * P) x 256: forward over the stages; writes x_t | u_t | lbd_{t+1} straight into
//                             the caller's `out` (padding stripped, a column's entries of one stage consecutive across the
//                             lanes), exact zeros for a gated problem
#pragma once
#include "gar_adjoint.hpp"

namespace gar {

#define GAR_AM_COLS 16     // columns of a panel
#define GAR_AM_THREADS 256 // four waves
#define GAR_AM_OPITCH 18   // pitch of the roll-out's computed panels in LDS: a column read (stride 18) spreads over 16 banks

struct AffineMultiParams {
  const gar_stage_meta *meta;
  UserLayout U;             // (unx, unu, nc0: the caller's dimensions of a padded solver)
  const long long *vec_off; // [horizon + 2] offsets of stage t's slots in an affine-layout vector, then of g0 / lbd0
  long long vec_stride;
  const int *status;
  const double *prob, *fac, *W;
  long long prob_stride, fac_stride;
  int w_rec, horizon, nc0; // (nc0: the device's)
  int vxx_packed, fb_t2;
  int nrhs, c0, panels; // this chunk: `panels` panels per problem, the first one starting at column c0
  const double *rhs;    // [batch][nrhs][vec_stride], the caller's
  double *out;          // the same shape
  double *prhs, *pout, *ivx, *ig0, *ires;
  int *gate;
  long long prhs_stride, pout_stride;
  int prhs_rec, pout_rec, ivx_rec, ig0_rec, init_rec;
  int nx_max, nu_max; // nx_max: over nx and nx2 of every stage
};
struct AffineMultiInit {
  GenericParams G;
  const double *ivx, *ig0;
  double *ires;
  const int *gate;
  int ivx_rec, ig0_rec, init_rec, panels;
};

// LDS of one workgroup (doubles): the panels at fixed offsets, the stage's matrices behind them
__host__ __device__ inline int affine_multi_sweep_panel_rows(int nx_max, int nu_max) { return 5 * nx_max + 3 * nu_max; }
__host__ __device__ inline int affine_multi_fb_doubles(int nx, int nu, int nx2, int fb_t2) {
  const int nr = nu + nx2;
  return fb_t2 ? ((nx + 1) / 2) * (2 * nr + 2) : nr * nx + 2;
}
__host__ __device__ inline int affine_multi_sweep_lds_doubles(int nx_max, int nu_max, int nx, int nu, int nx2, int fb_t2,
                                                              int vxx_packed) {
  const int nvv = vxx_packed ? nx2 * (nx2 + 1) / 2 : nx2 * nx2;
  return GAR_AM_COLS * affine_multi_sweep_panel_rows(nx_max, nu_max) + (nvv + 2) + affine_multi_fb_doubles(nx, nu, nx2, fb_t2) +
         (nu * nu + 2) + (nx2 * nu + 2);
}
__host__ __device__ inline int affine_multi_rollout_lds_doubles(int nx_max, int nu_max, int nx, int nu, int nx2, int fb_t2,
                                                                int vxx_packed) {
  const int nvv = vxx_packed ? nx2 * (nx2 + 1) / 2 : nx2 * nx2;
  return GAR_AM_OPITCH * (2 * (nu_max + nx_max) + nx_max) + GAR_AM_COLS * (nu_max + 2 * nx_max) + (nvv + 2) +
         affine_multi_fb_doubles(nx, nu, nx2, fb_t2);
}

// n pieces from src to the LDS image at gar_smem + dst (doubles, even; workgroup-uniform) by all waves of the workgroup:
// wave w takes the pieces 64 w ... 64 w + 63 of every 64 * nwaves
__device__ __forceinline__ void am_dma(const gar_double2 *src, int dst, int n, const WG &w) {
  char *d = reinterpret_cast<char *>(gar_smem + dst);
  for (int k0 = 64 * w.wave; k0 < n; k0 += w.nthr)
    if (k0 + w.lane < n)
      wave_dma16(reinterpret_cast<const char *>(src + k0 + w.lane), d + 16 * k0);
}
// a block of n doubles at rec + a into LDS at p (even), keeping the parity of a (aff_describe's rule: fetched from the even
// offset below to the even offset above).  -> the LDS offset of element 0; p advances by lds_doubles
__device__ __forceinline__ int am_fetch(int &p, const double *rec, int a, int n, int lds_doubles, const WG &w) {
  const int o0 = p + (a & 1);
  am_dma(reinterpret_cast<const gar_double2 *>(rec + (a & ~1)), p, aff_span(a, n) / 2, w);
  p += lds_doubles;
  return o0;
}
// fb = [K; Aff] of a stage: the fbT2 order lands with a pitch of 2 nr + 2 per pair of columns (gar_affine.hpp)
__device__ __forceinline__ int am_fetch_fb(int &p, const double *frec, int fb, int rows, int nx, int nr, bool t2, const WG &w) {
  if (!t2)
    return am_fetch(p, frec, fb, rows * nx, aff_span(fb, rows * nx), w);
  const int pitch = 2 * nr + 2, o0 = p + (fb & 1);
  const gar_double2 *src = reinterpret_cast<const gar_double2 *>(frec + (fb & ~1));
  for (int c = 0; 2 * c < nx; ++c)
    am_dma(src + c * nr, p + c * pitch, nr, w);
  p += ((nx + 1) / 2) * pitch;
  return o0;
}
// entry (row, col) of fb in LDS
__device__ __forceinline__ int am_fb(bool t2, int pitch, int nx, int row, int col) {
  return t2 ? (col >> 1) * pitch + 2 * row + (col & 1) : row * nx + col;
}

// D (M x 16, pitch pd) = C0 (pitch pc; null: zero) + sgn * A (M x K) Bp (K x 16, pitch pb) on f64 MFMA 16x16x4 tiles, tile
// row ti by wave (ti + rot) % nwaves.  A through aidx(i, k) -> its LDS offset.  Rows and k-steps beyond M and K are fed as
// zeros from clamped addresses (wg_gemm's rule: no conditional load).  D may alias C0.  No barrier inside.
template <class AIdx>
__device__ __forceinline__ void am_gemm(const WG &w, int rot, int M, int K, const double *As, AIdx aidx, const double *Bp,
                                        int pb, const double *C0, int pc, double *D, int pd, double sgn) {
  const int li = w.lane & 15, lk = w.lane >> 4;
  int first = w.wave - rot;
  while (first < 0)
    first += w.nwaves;
  for (int ti = first; 16 * ti < M; ti += w.nwaves) {
    const int i0 = ti << 4;
    double4_t acc;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = i0 + lk + 4 * r;
      const double c = C0 ? C0[(row < M ? row : M - 1) * pc + li] : 0.0;
      acc[r] = (C0 && row < M) ? c : 0.0;
    }
    const int ai = i0 + li, aic = ai < M ? ai : M - 1;
    const bool aok = ai < M;
    for (int k0 = 0; k0 < K; k0 += 16) {
      double a[4], b[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int k = k0 + 4 * q + lk, kc = k < K ? k : K - 1;
        a[q] = As[aidx(aic, kc)];
        b[q] = Bp[kc * pb + li];
        a[q] = (aok && k < K) ? sgn * a[q] : 0.0;
        b[q] = k < K ? b[q] : 0.0;
      }
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (k0 + 4 * q < K)
          acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[q], b[q], acc, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = i0 + lk + 4 * r;
      if (row < M)
        D[row * pd + li] = acc[r];
    }
  }
}

// ---- the caller's vectors as panel records ----------------------------------------------------------------------------------
__global__ void __launch_bounds__(GAR_AM_THREADS) gar_affine_multi_scatter(AffineMultiParams P) {
  const int N = P.horizon, tid = (int)threadIdx.x;
  const int t = (int)(blockIdx.x % (unsigned)(N + 1)), bp = (int)(blockIdx.x / (unsigned)(N + 1));
  const int b = bp / P.panels, p = bp - b * P.panels, c0 = P.c0 + GAR_AM_COLS * p;
  const gar_stage_meta m = P.meta[t];
  const UserKnot k = user_knot(P.U, m, t);
  const int nf = t == N ? 0 : k.nx2; // (the terminal knot has no dynamics: its slot, where the vector has one, is not read)
  const double *src = P.rhs + ((long long)b * P.nrhs + c0) * P.vec_stride; // column c0 of problem b
  const double *s = src + P.vec_off[t];
  double *rec = P.prhs + (long long)bp * P.prhs_stride + (long long)t * P.prhs_rec;
  const int rows = m.nx + m.nu + m.nx2;
  for (int e = tid; e < rows * GAR_AM_COLS; e += GAR_AM_THREADS) {
    const int i = e >> 4, j = e & 15;
    int from = -1; // the entry of the caller's vector; -1: a dummy entry
    if (i < m.nx)
      from = i < k.nx ? i : -1;
    else if (i < m.nx + m.nu)
      from = i - m.nx < k.nu ? k.nx + (i - m.nx) : -1;
    else
      from = i - m.nx - m.nu < nf ? k.nx + k.nu + (i - m.nx - m.nu) : -1;
    rec[e] = (from >= 0 && c0 + j < P.nrhs) ? s[(long long)j * P.vec_stride + from] : 0.0;
  }
  if (t == 0) {
    double *g = P.ig0 + (long long)bp * GAR_AM_COLS * P.ig0_rec;
    for (int e = tid; e < GAR_AM_COLS * P.nc0; e += GAR_AM_THREADS) {
      const int j = e / P.nc0, i = e - j * P.nc0;
      g[j * P.ig0_rec + i] = (i < P.U.nc0 && c0 + j < P.nrhs) ? src[(long long)j * P.vec_stride + P.vec_off[N + 1] + i] : 0.0;
    }
    if (tid == 0 && p == 0)
      P.gate[b] = P.status[b] == 0 ? 1 : 0;
  }
}

// ---- the vector half of the sweep on panels ---------------------------------------------------------------------------------
__global__ void __launch_bounds__(GAR_AM_THREADS) gar_affine_sweep_multi(AffineMultiParams P) {
  const WG w = wg_self();
  const int bp = (int)blockIdx.x, b = bp / P.panels, N = P.horizon, tid = w.tid;
  if (P.gate[b] == 0) // (a failed backward: the roll-out writes this problem's zeros)
    return;
  const int pk = P.vxx_packed, nxm = P.nx_max, num = P.nu_max, C = GAR_AM_COLS;
  // the panels
  double *VxC = gar_smem, *Fp = VxC + C * nxm, *Qp = Fp + C * nxm, *RV = Qp + C * nxm, *Rhat = RV + C * (num + nxm);
  double *KY = Rhat + C * num;
  const int oF = C * nxm, oQ = 2 * C * nxm, oR = 3 * C * nxm, base = C * affine_multi_sweep_panel_rows(nxm, num);
  const double *factors = P.fac + (long long)b * P.fac_stride;
  const double *prhs = P.prhs + (long long)bp * P.prhs_stride;
  double *pout = P.pout + (long long)bp * P.pout_stride;
  for (int t = N; t >= 0; --t) {
    const gar_stage_meta m = P.meta[t];
    const bool last = t == N;
    const gar_stage_meta mn = P.meta[last ? t : t + 1];
    const int nx = m.nx, nu = m.nu, n2 = last ? 0 : m.nx2, nr = m.nu + m.nc + m.nx2;
    const int rows = last ? nu : nr; // (the terminal record: K alone)
    const bool t2 = P.fb_t2 && !last;
    const int pitch = 2 * nr + 2;
    const gar_knot_offsets o = gar_knot_layout(m.nx, m.nu, m.nc, m.nx2, 0);
    const gar_factor_offsets fo = gar_factor_layout(m.nx, m.nu, m.nc, m.nx2, m.nth);
    const gar_factor_offsets fn = gar_factor_layout(mn.nx, mn.nu, mn.nc, mn.nx2, mn.nth);
    const int nvv = pk ? n2 * (n2 + 1) / 2 : n2 * n2;
    // ---- this stage's blocks and panel record: HBM -> LDS, every piece in flight before the one wait ----
    int p = base;
    const int oV = am_fetch(p, factors + mn.fac_off, fn.Vxx, nvv, aff_span(fn.Vxx, nvv), w);
    const int oFb = am_fetch_fb(p, factors + m.fac_off, fo.fb, rows, nx, nr, t2, w);
    const int oW = am_fetch(p, P.W + ((long long)b * (N + 1) + t) * P.w_rec, 0, nu * nu, aff_span(0, nu * nu), w);
    const int oB = am_fetch(p, P.prob + (long long)b * P.prob_stride + m.in_off, o.B, n2 * nu, aff_span(o.B, n2 * nu), w);
    const gar_double2 *rec = reinterpret_cast<const gar_double2 *>(prhs + (long long)t * P.prhs_rec);
    am_dma(rec, oQ, nx * (C / 2), w);
    am_dma(rec + nx * (C / 2), oR, nu * (C / 2), w);
    am_dma(rec + (nx + nu) * (C / 2), oF, n2 * (C / 2), w);
    GAR_WAIT_VMCNT(0);
    __syncthreads();
    const double *Vs = gar_smem + oV, *fbs = gar_smem + oFb, *Ws = gar_smem + oW, *Bs = gar_smem + oB;
    double *Vplus = RV + C * nu, *Kff = KY, *Yff = KY + C * nu;
    // ---- Vplus = Vx' + Vxx' F ----
    am_gemm(w, 0, n2, n2, Vs, [=](int i, int k) { return aff_sym(pk, n2, i, k); }, Fp, C, VxC, C, Vplus, C, 1.0);
    __syncthreads();
    // ---- Rhat = R + B^T Vplus ----
    am_gemm(w, 0, nu, n2, Bs, [=](int i, int k) { return i * n2 + k; }, Vplus, C, RV, C, Rhat, C, 1.0);
    __syncthreads();
    // ---- Kff = -W Rhat ----
    am_gemm(w, 0, nu, nu, Ws, [=](int i, int k) { return k * nu + i; }, Rhat, C, nullptr, C, Kff, C, -1.0);
    __syncthreads();
    // ---- Yff = F + B Kff;  Vx = Q + fb^T [R; Vplus] (the tile rows of the second dealt from where the first's end) ----
    am_gemm(w, 0, n2, nu, Bs, [=](int i, int k) { return k * n2 + i; }, Kff, C, Fp, C, Yff, C, 1.0);
    am_gemm(w, ((n2 + 15) >> 4) % w.nwaves, nx, nu + n2, fbs,
            [=](int j, int k) { return am_fb(t2, pitch, nx, k < nu ? k : k + m.nc, j); }, RV, C, Qp, C, VxC, C, 1.0);
    __syncthreads();
    // ---- Kff | Yff | Vx into the stage's side record; vx0 of every column for the initial stage ----
    gar_double2 *dst = reinterpret_cast<gar_double2 *>(pout + (long long)t * P.pout_rec);
    const gar_double2 *ky = reinterpret_cast<const gar_double2 *>(KY), *vx = reinterpret_cast<const gar_double2 *>(VxC);
    for (int e = tid; e < (nu + n2) * (C / 2); e += w.nthr)
      dst[e] = ky[e];
    for (int e = tid; e < nx * (C / 2); e += w.nthr)
      dst[(nu + m.nx2) * (C / 2) + e] = vx[e];
    if (t == 0) {
      double *iv = P.ivx + (long long)bp * C * P.ivx_rec;
      for (int j = w.wave; j < C; j += w.nwaves)
        for (int i = w.lane; i < nx; i += 64)
          iv[j * P.ivx_rec + i] = VxC[i * C + j];
    }
    GAR_WAIT_LGKMCNT0(); // (every LDS read of this stage has returned before the next stage's pieces land)
    __syncthreads();
  }
}

// ---- the initial stage of every column: the family's stand-alone one on redirected vx0, g0 and result --------------------
__global__ void __launch_bounds__(64) gar_affine_multi_initial(AffineMultiInit I) {
  const WG w = wave_self();
  const int col = (int)blockIdx.x, bp = col / GAR_AM_COLS, b = bp / I.panels;
  if (I.gate[b] == 0)
    return;
  (void)initial_wave_problem(w, I.G, b, I.ivx + (long long)col * I.ivx_rec, I.ig0 + (long long)col * I.ig0_rec,
                             I.ires + (long long)col * I.init_rec);
}

// ---- the roll-out on panels, into the caller's layout -----------------------------------------------------------------------
__global__ void __launch_bounds__(GAR_AM_THREADS) gar_rollout_multi(AffineMultiParams P) {
  const WG w = wg_self();
  const int bp = (int)blockIdx.x, b = bp / P.panels, pn = bp - b * P.panels, c0 = P.c0 + GAR_AM_COLS * pn, N = P.horizon;
  const int C = GAR_AM_COLS, OP = GAR_AM_OPITCH;
  int ncols = P.nrhs - c0; // the columns of this panel the caller has
  ncols = ncols < C ? ncols : C;
  double *outp = P.out + ((long long)b * P.nrhs + c0) * P.vec_stride;
  if (P.gate[b] == 0) { // exact zeros in all its columns
    for (int j = w.wave; j < ncols; j += w.nwaves)
      for (long long e = w.lane; e < P.vec_stride; e += 64)
        outp[(long long)j * P.vec_stride + e] = 0.0;
    return;
  }
  const int pk = P.vxx_packed, nxm = P.nx_max, num = P.nu_max;
  double *UX[2] = {gar_smem, gar_smem + OP * (num + nxm)};
  double *dL = gar_smem + 2 * OP * (num + nxm);
  const int oFF = OP * (2 * (num + nxm) + nxm), oVxN = oFF + C * (num + nxm), base = oVxN + C * nxm;
  const double *factors = P.fac + (long long)b * P.fac_stride;
  const double *pout = P.pout + (long long)bp * P.pout_stride;
  const double *ires = P.ires + (long long)bp * C * P.init_rec;
  double *dX = UX[1];
  { // dx0 of the initial stage; dl0 straight to the caller's lbd0
    const gar_stage_meta m0 = P.meta[0];
    for (int j = w.wave; j < C; j += w.nwaves) {
      for (int i = w.lane; i < m0.nx; i += 64)
        dX[i * OP + j] = ires[j * P.init_rec + i];
      if (j < ncols)
        for (int i = w.lane; i < P.U.nc0; i += 64)
          outp[(long long)j * P.vec_stride + P.vec_off[N + 1] + i] = ires[j * P.init_rec + m0.nx + i];
    }
  }
  __syncthreads();
  for (int t = 0; t <= N; ++t) {
    const gar_stage_meta m = P.meta[t];
    const bool last = t == N;
    const gar_stage_meta mn = P.meta[last ? t : t + 1];
    const int nx = m.nx, nu = m.nu, n2 = last ? 0 : m.nx2, nr = m.nu + m.nc + m.nx2;
    const int rows = last ? nu : nr;
    const bool t2 = P.fb_t2 && !last;
    const int pitch = 2 * nr + 2;
    const gar_factor_offsets fo = gar_factor_layout(m.nx, m.nu, m.nc, m.nx2, m.nth);
    const gar_factor_offsets fn = gar_factor_layout(mn.nx, mn.nu, mn.nc, mn.nx2, mn.nth);
    const int nvv = pk ? n2 * (n2 + 1) / 2 : n2 * n2;
    int p = base;
    const int oFb = am_fetch_fb(p, factors + m.fac_off, fo.fb, rows, nx, nr, t2, w);
    const int oV = am_fetch(p, factors + mn.fac_off, fn.Vxx, nvv, aff_span(fn.Vxx, nvv), w);
    am_dma(reinterpret_cast<const gar_double2 *>(pout + (long long)t * P.pout_rec), oFF, (nu + n2) * (C / 2), w); // Kff | Yff
    if (!last)                                                                                                       // Vx'
      am_dma(reinterpret_cast<const gar_double2 *>(pout + (long long)(t + 1) * P.pout_rec) + (mn.nu + mn.nx2) * (C / 2), oVxN,
             n2 * (C / 2), w);
    GAR_WAIT_VMCNT(0);
    __syncthreads();
    const double *fbs = gar_smem + oFb, *Vs = gar_smem + oV;
    double *D = UX[t & 1], *dXn = D + OP * nu;
    // ---- [dU; dX'] = [Kff; Yff] + [K; Aff] dX ----
    am_gemm(w, 0, nu + n2, nx, fbs, [=](int i, int k) { return am_fb(t2, pitch, nx, i < nu ? i : i + m.nc, k); }, dX, OP,
            gar_smem + oFF, C, D, OP, 1.0);
    __syncthreads();
    // ---- dL' = Vx' + Vxx' dX' ----
    am_gemm(w, 0, n2, n2, Vs, [=](int i, int k) { return aff_sym(pk, n2, i, k); }, dXn, OP, gar_smem + oVxN, C, dL, OP, 1.0);
    __syncthreads();
    // ---- x_t | u_t | lbd_{t+1} of every column the caller has, the caller's dimensions ----
    const UserKnot k = user_knot(P.U, m, t);
    const int slot = (int)(P.vec_off[t + 1] - P.vec_off[t]) - k.nx - k.nu; // (0 for a terminal knot given with nx2 = 0)
    for (int j = w.wave; j < ncols; j += w.nwaves) {
      double *d = outp + (long long)j * P.vec_stride + P.vec_off[t];
      for (int i = w.lane; i < k.nx + k.nu + slot; i += 64) {
        const int iu = i - k.nx, il = iu - k.nu;
        const double *from = i < k.nx ? dX + i * OP : (iu < k.nu ? D + iu * OP : dL + il * OP);
        const double v = from[j];
        d[i] = (il >= 0 && last) ? 0.0 : v;
      }
    }
    dX = dXn;
    GAR_WAIT_LGKMCNT0(); // (every LDS read of this stage has returned before the next stage's pieces land)
    __syncthreads();
  }
}

} // namespace gar
