// gar_affine.hpp -- re-solve for new affine terms (q, r, f, g0) from the factor records the last backward left:
// the VECTOR half of the Riccati recursion (riccati-kernel.hxx:209-277), unconstrained knots (nc = 0, nth = 0).
//
// Stage t's factor record holds fb = [K; Aff] and ff = [kff; yff], stage t+1's holds Vxx' and vx'.  With new q, r, f,
// for t = N ... 0:
//   vplus = vx' + Vxx' f            (t < N; Vxx' symmetric, read from its lower triangle, packed or full per family)
//   rhat  = r + B^T vplus
//   kff   = -W rhat                 W = (R + B^T Vxx' B)^-1, from the side buffer gar_affine_prepare fills
//   yff   = f + B kff
//   vx    = q + fb^T [r; vplus]     (= qhat + Shat kff: Shat kff = K^T rhat and A + B K = Aff)
//   terminal knot: rhat = r, W = R^-1 (nu > 0), vx = q + K^T r, no yff
// vx uses Aff FROM THE FACTOR RECORD (not A from the knot: the same byte count, and the knot's A is then never read).
// Only ff and vx of every record are rewritten; fb, Vxx and everything of the knots stay bit for bit.  The initial stage
// is the family's stand-alone one (gar_generic.hpp: gar_initial_wave), launched behind the sweep by the host.
//
// Three kernels, all through the stage descriptors (padding, the cycleAppend ring, a terminal knot kept as nx2 = nx):
//   gar_affine_scatter    grid (nb * (N + 1)) x 64: q, r, f of one knot (and g0 with stage 0) out of a packed
//                         per-problem affine vector in the CALLER's dimensions into the device knot record; under
//                         padding the real entries only -- the dummy ones and everything else are not touched
//   gar_affine_prepare    grid (batch * (N + 1)) x 64, no chain: W of one stage from knot t and factor t + 1, by the
//                         wave-scope Bunch-Kaufman of gar_device.hpp (the LDL^T it is when no pivoting is needed), the
//                         full symmetric matrix into W[b][t]; about 9.5 KB of reads per stage at (36, 12): byte-bound
//   gar_backward_affine   grid (batch) x 64: one wave per problem, sequential over the stages.  A stage's blocks
//                         (Vxx', fb, W, B, f, q, r: 25 KB at (36, 12)) go HBM -> LDS as 16-byte pieces by LDS-DMA, all
//                         of them in flight before one wait, into ONE LDS image (six waves share a CU and cover each
//                         other's fetch); the mat-vecs run from there, lane per row / column.  fb in the fbT2 order gets
//                         a pitch of 2 nr + 2 in LDS (2 nr is a multiple of the bank count at the headline shape).
//                         No register array, no scratch.
// Problems whose status word is non-zero (a failed backward) are left alone by prepare and by the sweep; `ok[b]` tells
// the initial stage which problems to take.
// gar_refine_sweep is the sweep's second instance (backward_affine_wave<true>): q | r and f from a right-hand-side buffer
// instead of the knot, ff and vx into a side buffer instead of the factor record, gated per problem (gar_refine.hpp).
#pragma once
#include "gar_device.hpp"
#include "gar_kkt.hpp" // kkt_group_sum, GAR_KKT_GROUP: four lanes share a short row
#include "gar_layout.h"

namespace gar {

struct AffineParams {
  const gar_stage_meta *meta;
  double *prob;    // the device knot records (scatter writes q, r, f, g0; prepare and the sweep read)
  double *fac;     // the factor records
  double *W;       // [batch][horizon + 1][w_rec]: W of stage t, nu x nu column-major
  int *status;     // the status words of the last backward
  int *ok;         // [batch]: 1 = re-solved, 0 = left alone (status != 0)
  const double *src;        // scatter: nb packed affine vectors (device)
  const long long *src_off; // scatter: [horizon + 2] offsets of stage t's q | r | f, then of g0
  long long prob_stride, fac_stride, src_stride, g0_off;
  int horizon, w_rec, b0;
  int unx, unu, unc0; // scatter: the caller's (nx, nu) of a padded solver (unx = 0: not padded), the caller's nc0
  int qr_packed, vxx_packed, fb_t2;
  int nx_max; // the sweep's chain vector vx'
  // gar_refine_sweep only (gar_refine.hpp; null / zero for the re-solve): q~ | r~, f~ of stage t are read from
  // rhs[b][t * rhs_rec] (gar_kkt.hpp: refine_rhs_f) instead of the knot, and ff~ = [kff; yff], vx~ go to
  // out[b][t * out_rec] (refine_out_vx) instead of the factor record; problems with gate[b] == 0 are left alone
  const double *rhs;
  double *out;
  const int *gate;
  long long rhs_stride, out_stride;
  int rhs_rec, out_rec;
};
// offset of vx~ inside a stage's record of the correction: ff~ = kff (nu) | yff (nx2) | pad to even | vx~ (nx)
__host__ __device__ inline int refine_out_vx(int nu, int nx2) { return (nu + nx2 + 1) & ~1; }

// lds[k] = rec[a + k], k < n, by one wave.  rec is 16-byte aligned and &lds[0] has the parity of a: 16-byte loads from
// the even offsets, eight in flight per lane before the first store, one double at an odd end.
__device__ inline void aff_fetch(double *lds, const double *rec, int a, int n, int lane) {
  if (n <= 0)
    return;
  const int b = a + n, a2 = (a + 1) & ~1, b2 = b & ~1;
  for (int e0 = a2 + 2 * lane; e0 < b2; e0 += 8 * 128) {
    gar_double2 v[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int e = e0 + 128 * q;
      v[q] = *reinterpret_cast<const gar_double2 *>(rec + (e < b2 ? e : e0));
    }
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int e = e0 + 128 * q;
      if (e < b2)
        *reinterpret_cast<gar_double2 *>(lds + (e - a)) = v[q];
    }
  }
  if (lane == 0 && (a & 1))
    lds[0] = rec[a];
  if (lane == 63 && (b & 1) && b - 1 >= a2)
    lds[b - 1 - a] = rec[b - 1];
}
// element (i, j) of the symmetric n x n block, from its lower triangle: packed (gar_sym_index) or full column-major
__device__ __forceinline__ int aff_sym(int packed, int n, int i, int j) {
  const int a = i >= j ? i : j, b = i >= j ? j : i;
  return packed ? gar_sym_index(1, n, a, b) : b * n + a;
}

// ---- q, r, f, g0 out of the caller's packed affine vectors ------------------------------------------------------------
__global__ void __launch_bounds__(64) gar_affine_scatter(AffineParams P) {
  const int N = P.horizon, lane = (int)threadIdx.x;
  const int t = (int)(blockIdx.x % (unsigned)(N + 1)), bl = (int)(blockIdx.x / (unsigned)(N + 1));
  const gar_stage_meta m = P.meta[t];
  const gar_knot_offsets o = gar_knot_layout(m.nx, m.nu, m.nc, m.nx2, (m.flags & GAR_KNOT_HAS_PARAM) ? m.nth : 0);
  double *problem = P.prob + (long long)(P.b0 + bl) * P.prob_stride;
  double *rec = problem + m.in_off;
  const double *src = P.src + (long long)bl * P.src_stride;
  const double *s = src + P.src_off[t];
  const int nq = P.unx > 0 ? P.unx : m.nx, nr = P.unx > 0 ? (m.nu > 0 ? P.unu : 0) : m.nu;
  const int nf = (int)(P.src_off[t + 1] - P.src_off[t]) - nq - nr; // (0 for a terminal knot given with nx2 = 0)
  for (int k = lane; k < nq; k += 64)
    rec[o.q + k] = s[k];
  for (int k = lane; k < nr; k += 64)
    rec[o.r + k] = s[nq + k];
  for (int k = lane; k < nf; k += 64)
    rec[o.f + k] = s[nq + nr + k];
  if (t == 0)
    for (int k = lane; k < P.unc0; k += 64)
      problem[P.g0_off + k] = src[P.src_off[N + 1] + k];
}

// ---- W = (R + B^T Vxx' B)^-1 of one stage -------------------------------------------------------------------------------
__host__ __device__ inline int affine_prepare_lds_doubles(int nu, int nx2, int vxx_packed) {
  const int nvv = vxx_packed ? nx2 * (nx2 + 1) / 2 : nx2 * nx2;
  return (nvv + 1) + 2 * (nx2 * nu + 1) + 2 * nu * nu + (nu + 2) + (nu + 16) / 2 + 8;
}
__global__ void __launch_bounds__(64) gar_affine_prepare(AffineParams P) {
  const WG w = wave_self();
  const int N = P.horizon, lane = w.lane;
  const int t = (int)(blockIdx.x % (unsigned)(N + 1)), b = (int)(blockIdx.x / (unsigned)(N + 1));
  if (P.status[b] != 0)
    return;
  const gar_stage_meta m = P.meta[t];
  const int nu = m.nu, nx = m.nx;
  if (nu == 0)
    return;
  const bool last = t == N;
  const int n2 = last ? 0 : m.nx2;
  const gar_knot_offsets o = gar_knot_layout(nx, nu, m.nc, m.nx2, 0);
  const double *rec = P.prob + (long long)b * P.prob_stride + m.in_off;
  const int pk = P.vxx_packed, nvv = pk ? n2 * (n2 + 1) / 2 : n2 * n2;
  double *p = gar_smem;
  auto take = [&p](int n, int parity) {
    if (((int)(p - gar_smem) ^ parity) & 1)
      ++p;
    double *q = p;
    p += n;
    return q;
  };
  const gar_stage_meta mn = P.meta[last ? t : t + 1];
  const gar_factor_offsets fn = gar_factor_layout(mn.nx, mn.nu, mn.nc, mn.nx2, mn.nth);
  double *Vs = take(nvv, fn.Vxx), *Bs = take(n2 * nu, o.B), *T = take(n2 * nu, 0);
  double *M = take(nu * nu, 0), *X = take(nu * nu, 0), *sub = take(nu + 1, 0);
  int *piv = (int *)take((nu + 16) / 2 + 2, 0), *ctrl = piv + nu;
  if (!last) {
    aff_fetch(Vs, P.fac + (long long)b * P.fac_stride + mn.fac_off, fn.Vxx, nvv, lane);
    aff_fetch(Bs, rec, o.B, n2 * nu, lane);
  }
  wave_sync();
  for (int e = lane; e < n2 * nu; e += 64) { // T = Vxx' B
    const int k = e / n2, i = e - k * n2;
    double acc = 0.0;
    for (int j = 0; j < n2; ++j)
      acc += Vs[aff_sym(pk, n2, i, j)] * Bs[k * n2 + j];
    T[e] = acc;
  }
  wave_sync();
  const bool rp = P.qr_packed && !last;
  for (int e = lane; e < nu * nu; e += 64) { // Rhat from its lower triangle, mirrored; X = I
    const int j = e / nu, i = e - j * nu;
    const int a = i >= j ? i : j, c = i >= j ? j : i;
    double acc = rec[o.R + (rp ? gar_lower_index(nu, a, c) : c * nu + a)];
    for (int l = 0; l < n2; ++l)
      acc += Bs[a * n2 + l] * T[c * n2 + l];
    M[e] = acc;
    X[e] = i == j ? 1.0 : 0.0;
  }
  wave_sync();
  const int failed = wg_bk_factor(w, nu, M, nu, sub, piv, ctrl);
  if (failed) { // (a backward that succeeded factorised this matrix: not reached on its records)
    if (lane == 0)
      atomicOr(&P.status[b], 1);
    return;
  }
  wg_bk_solve(w, nu, M, nu, sub, piv, X, 1, nu, nu);
  wave_sync();
  double *out = P.W + ((long long)b * (N + 1) + t) * P.w_rec;
  for (int e = lane; e < nu * nu; e += 64) {
    const int j = e / nu, i = e - j * nu;
    out[e] = 0.5 * (X[e] + X[i * nu + j]);
  }
}

// ---- the vector half of the sweep -------------------------------------------------------------------------------------
// One stage's blocks as the sweep fetches them: five ranges of 16-byte pieces, HBM -> LDS by LDS-DMA (gar_device.hpp:
// wave_dma16; no register holds them).  A block that starts or ends on an odd double is fetched from the even offset
// below / to the even offset above (the neighbour lies inside the same record, whose length is even) and lands in LDS
// with the same parity, so every piece is one aligned 16-byte transfer.
struct AffStage {
  int nx, nu, nr, n2, last, t2, pitch;
  int oV, oFb, oW, oBf, oQr, oVplus, oRhat, oKff; // LDS offsets (doubles) of element 0 of each block / vector
  const gar_double2 *sV, *sFb, *sW, *sBf, *sQr;  // the first piece of each block in HBM
  int rV, rFb, rW, rBf, rQr;                     // LDS offset (doubles, even) of that piece
  int nV, nFb, nW, nBf, nQr;                     // pieces
  double *frec; // where ff and vx go: the factor record (the refinement sweep: the stage's record of the correction)
  int ff, vx, nc;
  int oF;                // f in LDS: behind B (the refinement sweep: a block of its own, from the right-hand side)
  const gar_double2 *sF; // the refinement sweep's f~
  int rF, nF;
};
__host__ __device__ inline int aff_span(int a, int n) { return n > 0 ? (((a & 1) + n + 1) & ~1) : 0; }
__host__ __device__ inline int affine_sweep_lds_doubles(int nx_max, int nx, int nu, int nx2, int fb_t2, int vxx_packed) {
  const int nr = nu + nx2, nvv = vxx_packed ? nx2 * (nx2 + 1) / 2 : nx2 * nx2;
  const int fb = fb_t2 ? ((nx + 1) / 2) * (2 * nr + 2) : nr * nx;
  return ((nx_max + 1) & ~1) + (nvv + 2) + (fb + 2) + (nu * nu + 2) + (nx2 * nu + nx2 + 2) + (nx + nu + 2) + (nx2 + 2) +
         2 * (nu + 2);
}
template <bool REFINE> __device__ inline AffStage aff_describe(const AffineParams &P, int b, int t, int base) {
  AffStage s;
  const int N = P.horizon;
  const gar_stage_meta m = P.meta[t];
  s.last = t == N;
  s.nx = m.nx, s.nu = m.nu, s.nc = m.nc, s.nr = m.nu + m.nc + m.nx2, s.n2 = s.last ? 0 : m.nx2;
  const gar_knot_offsets o = gar_knot_layout(m.nx, m.nu, m.nc, m.nx2, 0);
  const gar_factor_offsets fo = gar_factor_layout(m.nx, m.nu, m.nc, m.nx2, m.nth);
  const gar_stage_meta mn = P.meta[s.last ? t : t + 1];
  const gar_factor_offsets fn = gar_factor_layout(mn.nx, mn.nu, mn.nc, mn.nx2, mn.nth);
  const double *knot = P.prob + (long long)b * P.prob_stride + m.in_off;
  double *factors = P.fac + (long long)b * P.fac_stride;
  const double *frec = factors + m.fac_off; // fb is read from here
  if constexpr (REFINE) {
    s.frec = P.out + (long long)b * P.out_stride + (long long)t * P.out_rec;
    s.ff = 0, s.vx = refine_out_vx(m.nu, m.nx2);
  } else {
    s.frec = factors + m.fac_off;
    s.ff = fo.ff, s.vx = fo.vx;
  }
  s.t2 = P.fb_t2 && !s.last;
  s.pitch = 2 * s.nr + 2;
  const int nvv = P.vxx_packed ? s.n2 * (s.n2 + 1) / 2 : s.n2 * s.n2;
  const int rows = s.last ? s.nu : s.nr; // (the terminal record: K alone)
  int p = base;
  auto block = [&p](const double *rec, int a, int n, int lds_doubles, const gar_double2 *&src, int &r, int &o0) {
    r = p;
    o0 = p + (a & 1);
    src = reinterpret_cast<const gar_double2 *>(rec + (a & ~1));
    p += lds_doubles;
    return aff_span(a, n) / 2;
  };
  s.nV = block(factors + mn.fac_off, fn.Vxx, nvv, aff_span(fn.Vxx, nvv), s.sV, s.rV, s.oV);
  s.nFb = block(frec, fo.fb, rows * s.nx, s.t2 ? ((s.nx + 1) / 2) * s.pitch : aff_span(fo.fb, rows * s.nx), s.sFb,
                s.rFb, s.oFb);
  s.nW = block(P.W + ((long long)b * (N + 1) + t) * P.w_rec, 0, s.nu * s.nu, aff_span(0, s.nu * s.nu), s.sW, s.rW, s.oW);
  if constexpr (REFINE) { // B from the knot; f~ and q~ | r~ from the right-hand side (both start on an even double)
    const double *rhs = P.rhs + (long long)b * P.rhs_stride + (long long)t * P.rhs_rec;
    const int of = refine_rhs_f(s.nx, s.nu);
    s.nBf = block(knot, o.B, s.n2 * s.nu, aff_span(o.B, s.n2 * s.nu), s.sBf, s.rBf, s.oBf);
    s.nF = block(rhs, of, s.n2, aff_span(of, s.n2), s.sF, s.rF, s.oF);
    s.nQr = block(rhs, 0, s.nx + s.nu, aff_span(0, s.nx + s.nu), s.sQr, s.rQr, s.oQr);
  } else {
    s.nBf = block(knot, o.B, s.n2 * s.nu + s.n2, aff_span(o.B, s.n2 * s.nu + s.n2), s.sBf, s.rBf, s.oBf); // B | f side by side
    s.nQr = block(knot, o.q, s.nx + s.nu, aff_span(o.q, s.nx + s.nu), s.sQr, s.rQr, s.oQr);                 // q | r too
    s.oF = s.oBf + s.n2 * s.nu, s.sF = nullptr, s.rF = s.nF = 0;
  }
  s.oVplus = p, p += (s.n2 + 1) & ~1;
  s.oRhat = p, p += (s.nu + 1) & ~1;
  s.oKff = p;
  return s;
}
// n pieces from src to the LDS image at gar_smem + dst (doubles, even; wave-uniform): 64 pieces per instruction
__device__ __forceinline__ void aff_dma(const gar_double2 *src, int dst, int n, int lane) {
  char *d = reinterpret_cast<char *>(gar_smem + dst);
  for (int k0 = 0; k0 < n; k0 += 64)
    if (k0 + lane < n)
      wave_dma16(reinterpret_cast<const char *>(src + k0 + lane), d + 16 * k0);
}

// REFINE: the same sweep on redirected operands (AffineParams::rhs, out, gate) -- gar_refine_sweep below
template <bool REFINE> __device__ __forceinline__ void backward_affine_wave(const AffineParams &P) {
  const int b = (int)blockIdx.x, lane = (int)threadIdx.x, N = P.horizon;
  if constexpr (REFINE) {
    if (P.gate[b] == 0) // (written by gar_kkt_reduce: failed problems, and those at or below the threshold)
      return;
  } else {
    const bool skip = P.status[b] != 0;
    if (lane == 0)
      P.ok[b] = skip ? 0 : 1;
    if (skip)
      return;
  }
  const int g = lane / GAR_KKT_GROUP, sub = lane % GAR_KKT_GROUP, ng = 64 / GAR_KKT_GROUP;
  double *vxn = gar_smem; // vx of stage t + 1: the chain
  const int base = (P.nx_max + 1) & ~1, pk = P.vxx_packed;
  for (int t = N; t >= 0; --t) {
    const AffStage s = aff_describe<REFINE>(P, b, t, base);
    // ---- this stage's blocks: HBM -> LDS, every piece in flight before the one wait ----
    aff_dma(s.sV, s.rV, s.nV, lane);
    if (s.t2) { // pair block c of nr pieces to c * pitch
      for (int c = 0; 2 * c < s.nx; ++c)
        aff_dma(s.sFb + c * s.nr, s.rFb + c * s.pitch, s.nr, lane);
    } else {
      aff_dma(s.sFb, s.rFb, s.nFb, lane);
    }
    aff_dma(s.sW, s.rW, s.nW, lane);
    aff_dma(s.sBf, s.rBf, s.nBf, lane);
    if constexpr (REFINE)
      aff_dma(s.sF, s.rF, s.nF, lane);
    aff_dma(s.sQr, s.rQr, s.nQr, lane);
    GAR_WAIT_VMCNT(0);
    wave_sync();
    const int nx = s.nx, nu = s.nu, n2 = s.n2;
    const double *Vs = gar_smem + s.oV, *fbs = gar_smem + s.oFb, *Ws = gar_smem + s.oW, *Bs = gar_smem + s.oBf;
    const double *fs = gar_smem + s.oF, *qs = gar_smem + s.oQr, *rs = qs + nx;
    double *vplus = gar_smem + s.oVplus, *rhat = gar_smem + s.oRhat, *kff = gar_smem + s.oKff;
    // ---- vplus = vx' + Vxx' f: element (i, j) of the lower triangle at F(min) + max ----
    for (int i = lane; i < n2; i += 64) {
      double acc = vxn[i];
      const int fi = pk ? (2 * i < n2 ? i * n2 : (n2 - 1 - i) * (n2 + 1) + 1) : i * n2;
#pragma unroll 12
      for (int j = 0; j < n2; ++j) {
        const int fj = pk ? (2 * j < n2 ? j * n2 : (n2 - 1 - j) * (n2 + 1) + 1) : j * n2;
        acc += Vs[i >= j ? fj + i : fi + j] * fs[j];
      }
      vplus[i] = acc;
    }
    wave_sync();
    // ---- rhat = r + B^T vplus ----
    for (int k0 = 0; k0 < nu; k0 += ng) {
      const int k = k0 + g;
      double acc = 0.0;
      if (k < nu) {
#pragma unroll 9
        for (int i = sub; i < n2; i += GAR_KKT_GROUP)
          acc += Bs[k * n2 + i] * vplus[i];
      }
      acc = kkt_group_sum(acc);
      if (k < nu && sub == 0)
        rhat[k] = rs[k] + acc;
    }
    wave_sync();
    // ---- kff = -W rhat ----
    for (int k0 = 0; k0 < nu; k0 += ng) {
      const int k = k0 + g;
      double acc = 0.0;
      if (k < nu)
        for (int l = sub; l < nu; l += GAR_KKT_GROUP)
          acc += Ws[l * nu + k] * rhat[l];
      acc = kkt_group_sum(acc);
      if (k < nu && sub == 0)
        kff[k] = -acc;
    }
    wave_sync();
    // ---- ff = [kff; yff], yff = f + B kff;  vx = q + fb^T [r; vplus] ----
    for (int k = lane; k < nu; k += 64)
      s.frec[s.ff + k] = kff[k];
    for (int i = lane; i < n2; i += 64) {
      double acc = fs[i];
#pragma unroll 12
      for (int k = 0; k < nu; ++k)
        acc += Bs[k * n2 + i] * kff[k];
      s.frec[s.ff + nu + s.nc + i] = acc;
    }
    for (int j = lane; j < nx; j += 64) {
      double acc = qs[j];
      const double *col = s.t2 ? fbs + (j >> 1) * s.pitch + (j & 1) : fbs + j;
      const int rstep = s.t2 ? 2 : nx;
#pragma unroll 12
      for (int r = 0; r < nu; ++r)
        acc += col[r * rstep] * rs[r];
      col += (nu + s.nc) * rstep;
#pragma unroll 12
      for (int i = 0; i < n2; ++i)
        acc += col[i * rstep] * vplus[i];
      s.frec[s.vx + j] = acc;
      vxn[j] = acc; // (read by the next stage's first phase only: a barrier lies between)
    }
    GAR_WAIT_LGKMCNT0(); // (every LDS read of this stage has returned before the next stage's pieces land)
    wave_sync();
  }
}
__global__ void __launch_bounds__(64) gar_backward_affine(AffineParams P) { backward_affine_wave<false>(P); }
// the correction's vector sweep of a refinement step: affine_sweep_lds_doubles + 4 doubles of dynamic LDS
__global__ void __launch_bounds__(64) gar_refine_sweep(AffineParams P) { backward_affine_wave<true>(P); }

} // namespace gar
