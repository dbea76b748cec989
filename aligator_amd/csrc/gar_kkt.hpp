// gar_kkt.hpp -- lqrComputeKktError (gar/utils.hxx:88-182) for the whole batch, on the device.
//
// The reference evaluates the KKT residuals of ONE problem on the host; every test of its solvers asserts on the triple
// (dynErr, cstErr, dualErr) it returns.  Here the problems and their solutions live in HBM (31 GB of knots at the
// headline size): the residuals are formed where the records are.  Two kernels, no MFMA -- the work is mat-vec, one
// multiply-add per knot entry, and the bound is the knot bytes:
//   gar_kkt_stage_residuals  grid (batch * (horizon + 1)): one workgroup per (problem, stage) reads the knot record and the
//                            solution record THROUGH the stage descriptors (padding, the cycleAppend ring, mixed nc,
//                            a terminal knot kept as nx2 = nx are all described there) and writes the four infinity
//                            norms |dyn|, |cst|, |gx|, |gu| of its stage; stage 0's dyn slot also covers g0 + G0 x0
//   gar_kkt_reduce           grid (batch): one wave per problem folds the stages to (dynErr, cstErr, dualErr)
// Term by term (utils.hxx:116-178; the nu > 0 guards are zero-column blocks here):
//   cst = C x + D u + d - mueq v            gx = q + Q x + S u + C^T v + (t = 0 ? G0^T lbda0 : -lbda_t) + A^T lbda_{t+1} [+ Gx th]
//   dyn = A x + B u + f - x_{t+1}  (t < N)  gu = r + S^T x + R u + D^T v + B^T lbda_{t+1} [+ Gu th]
// _gt is not part of the returned triple and is not formed.
//
// A knot is fetched from HBM ONCE, with 16-byte loads (the records are 16-byte aligned; a block that starts on an odd
// double gets one 8-byte load at either end), into an LDS tile of GAR_KKT_TILE doubles -- the (36, 12) knot in one piece,
// a longer record tile after tile, cut anywhere: every product below tests its entry against the tile's range.  M x and
// M^T y of a block (A, B, S, C, D, G0) are formed from that one copy.  With GAR_HIP_FMT_QR_PACKED the lower triangles of
// Q and R are all that is fetched, and the symmetric product is formed from the triangle.  The terminal knot's A, B, f
// and, without theta, the parameter blocks are not fetched.
//
// Ownership instead of barriers: entry k of every residual vector is only ever updated by ONE thread (lane 0 of the
// GAR_KKT_GROUP-lane group k mod #groups), whichever block contributes -- a row of M x and a column of M^T y are both
// summed by the group that owns the entry, GAR_KKT_GROUP lanes striding over the other index, folded by two shuffles.
// So the products of a tile need no barrier between them: two per tile (staged / consumed), whatever the knot holds.
//
// The norms are maxima that do NOT swallow a NaN (kkt_nanmax): a non-finite residual entry makes its norm non-finite.
// That is numpy's max, not std::max (which the reference uses and which drops a NaN in second position); the result is
// independent of the order of the reduction.
#pragma once
#include "gar_layout.h"

#ifndef GAR_KKT_THREADS
#define GAR_KKT_THREADS 256 // one workgroup of four waves per (stage, problem); 64: one wave (DESIGN.md 5.3b has the A/B)
#endif
#define GAR_KKT_TILE 4096   // doubles of a record in LDS at a time (32 KiB + the stage's vectors: four workgroups share a CU)
#define GAR_KKT_GROUP 4     // lanes that share one row / column of a product

namespace gar {

struct KktParams {
  const gar_stage_meta *meta;
  const double *prob;  // the caller-facing knot records (gar_hip_device_problems)
  const double *sol;   // xs | us | vs | lbdas
  const double *theta; // batch x nth0, or null
  double *stage;       // [batch][horizon + 1][4]: dyn, cst, gx, gu
  double *err;         // [batch][3]: dynErr, cstErr, dualErr
  long long prob_stride, sol_stride, G0_off, g0_off;
  int horizon, nc0, nth0;
  int qr_packed; // knots t < horizon keep Q, R as packed lower triangles (gar_layout.h)
  double mueq;
  // gar_hip_refine (gar_refine.hpp), all null / zero for every other caller: the residual VECTORS gx | gu, dyn of stage
  // t go to rhs[b][t * rhs_rec] (refine_rhs_f(nx, nu) doubles between them), g0 + G0 x0 behind the last stage's; the
  // reduction writes gate[b] = 1 where the problem is to be refined: status[b] == 0 and max(dynErr, dualErr) finite and
  // above `threshold`
  double *rhs;
  int *gate;
  const int *status;
  long long rhs_stride;
  int rhs_rec;
  double threshold;
};
// offset of f~ inside a stage's right-hand-side record: q~ (nx) | r~ (nu) | pad to even | f~ (nx2)
__host__ __device__ inline int refine_rhs_f(int nx, int nu) { return (nx + nu + 1) & ~1; }

// LDS of gar_kkt_stage_residuals for one stage: the tile, the seven input vectors, the five residual vectors
__host__ __device__ inline int kkt_lds_doubles(int nx, int nu, int nc, int nx2, int nth, int nc0) {
  auto even = [](int n) { return (n + 1) & ~1; };
  const int nl = nx > nc0 ? nx : nc0;
  return GAR_KKT_TILE + 2 * even(nx) + 2 * even(nu) + 2 * even(nc) + even(nl) + 3 * even(nx2) + even(nth) + even(nc0);
}

__device__ inline double kkt_nanmax(double m, double a) { return m != m ? m : ((a > m || a != a) ? a : m); }

__device__ inline double kkt_group_sum(double v) {
#pragma unroll
  for (int s = 1; s < GAR_KKT_GROUP; s *= 2)
    v += __shfl_xor(v, s);
  return v;
}

// [a, b) of the record, as far as it falls into the tile [c0, c0 + GAR_KKT_TILE): 16-byte loads from the even offsets
// (rec is 16-byte aligned and c0 is even: global and LDS parities agree), one double at an odd end
__device__ inline void kkt_stage_range(double *tile, const double *rec, int c0, int a, int b, int tid, int nthr) {
  a = a > c0 ? a : c0;
  b = b < c0 + GAR_KKT_TILE ? b : c0 + GAR_KKT_TILE;
  if (a >= b)
    return;
  const int a2 = (a + 1) & ~1, b2 = b & ~1;
  for (int e = a2 + 2 * tid; e < b2; e += 2 * nthr) {
    const gar_double2 v = *reinterpret_cast<const gar_double2 *>(rec + e);
    *reinterpret_cast<gar_double2 *>(tile + (e - c0)) = v;
  }
  if (tid == 0 && (a & 1))
    tile[a - c0] = rec[a];
  if (tid == nthr - 1 && (b & 1) && b - 1 >= a2)
    tile[b - 1 - c0] = rec[b - 1];
}

// The r x c column-major block at record offset `off`, the part of it the tile holds:
//   y[i] += sum_j M(i, j) xin[j]  (y non-null)      z[j] += sum_i M(i, j) win[i]  (z non-null)
// Every thread of the workgroup calls it (the shuffles are wave-wide); the trip counts do not depend on the thread.
__device__ inline void kkt_block(const double *tile, int c0, int off, int r, int c, const double *xin, double *y,
                                 const double *win, double *z, int tid, int nthr) {
  const int lo = off > c0 ? off : c0, hi = off + r * c < c0 + GAR_KKT_TILE ? off + r * c : c0 + GAR_KKT_TILE;
  if (lo >= hi)
    return;
  const int e0 = lo - off, e1 = hi - off, base = off - c0; // entry e of the block: tile[base + e], e0 <= e < e1
  const int g = tid / GAR_KKT_GROUP, sub = tid % GAR_KKT_GROUP, ng = nthr / GAR_KKT_GROUP;
  if (y)
    for (int i0 = 0; i0 < r; i0 += ng) {
      const int i = i0 + g;
      double acc = 0.0;
      if (i < r)
        for (int j = sub; j < c; j += GAR_KKT_GROUP) {
          const int e = i + j * r;
          if (e >= e0 && e < e1)
            acc += tile[base + e] * xin[j];
        }
      acc = kkt_group_sum(acc);
      if (i < r && sub == 0)
        y[i] += acc;
    }
  if (z)
    for (int j0 = 0; j0 < c; j0 += ng) {
      const int j = j0 + g;
      double acc = 0.0;
      if (j < c)
        for (int i = sub; i < r; i += GAR_KKT_GROUP) {
          const int e = i + j * r;
          if (e >= e0 && e < e1)
            acc += tile[base + e] * win[i];
        }
      acc = kkt_group_sum(acc);
      if (j < c && sub == 0)
        z[j] += acc;
    }
}

// y += M xin for the symmetric n x n block kept as its packed lower triangle (gar_lower_index) at `off`
__device__ inline void kkt_sym_packed(const double *tile, int c0, int off, int n, const double *xin, double *y, int tid,
                                      int nthr) {
  const int len = n * (n + 1) / 2;
  const int lo = off > c0 ? off : c0, hi = off + len < c0 + GAR_KKT_TILE ? off + len : c0 + GAR_KKT_TILE;
  if (lo >= hi)
    return;
  const int e0 = lo - off, e1 = hi - off, base = off - c0;
  const int g = tid / GAR_KKT_GROUP, sub = tid % GAR_KKT_GROUP, ng = nthr / GAR_KKT_GROUP;
  for (int i0 = 0; i0 < n; i0 += ng) {
    const int i = i0 + g;
    double acc = 0.0;
    if (i < n)
      for (int j = sub; j < n; j += GAR_KKT_GROUP) {
        const int e = i >= j ? gar_lower_index(n, i, j) : gar_lower_index(n, j, i);
        if (e >= e0 && e < e1)
          acc += tile[base + e] * xin[j];
      }
    acc = kkt_group_sum(acc);
    if (i < n && sub == 0)
      y[i] += acc;
  }
}

// y += the n-vector at record offset `off` (by the owners of y's entries)
__device__ inline void kkt_vector(const double *tile, int c0, int off, int n, double *y, int tid, int nthr) {
  const int g = tid / GAR_KKT_GROUP, sub = tid % GAR_KKT_GROUP, ng = nthr / GAR_KKT_GROUP;
  if (sub != 0)
    return;
  for (int k = g; k < n; k += ng) {
    const int e = off + k - c0;
    if (e >= 0 && e < GAR_KKT_TILE)
      y[k] += tile[e];
  }
}

// grid (batch * (horizon + 1)), the stage the fast index -- all of it in grid.x, as the sweeps keep their batch, so that
// a batch above 65 535 is served -- x GAR_KKT_THREADS (any multiple of 64), kkt_lds_doubles of dynamic LDS
__global__ void __launch_bounds__(GAR_KKT_THREADS) gar_kkt_stage_residuals(KktParams P) {
  const int N = P.horizon;
  const int t = (int)(blockIdx.x % (unsigned)(N + 1)), b = (int)(blockIdx.x / (unsigned)(N + 1));
  const int tid = (int)threadIdx.x, nthr = (int)blockDim.x;
  const gar_stage_meta m = P.meta[t];
  const gar_stage_meta mn = P.meta[t < N ? t + 1 : t];
  const int nx = m.nx, nu = m.nu, nc = m.nc, nx2 = m.nx2, nc0 = P.nc0;
  const bool last = t == N;
  const int nst = (m.flags & GAR_KNOT_HAS_PARAM) ? m.nth : 0; // the parameter blocks the record carries
  const bool par = P.theta != nullptr; // (kkt_check: then every record carries nst = nth0 > 0 columns)
  const int nl = t == 0 ? nc0 : nx; // lbda_t
  double *tile = gar_smem, *p = tile + GAR_KKT_TILE;
  auto take = [&p](int n) {
    double *q = p;
    p += (n + 1) & ~1;
    return q;
  };
  double *xs = take(nx), *us = take(nu), *vs = take(nc), *lt = take(nx > nc0 ? nx : nc0), *ln = take(nx2), *xn = take(nx2),
         *th = take(nst);
  double *gx = take(nx), *gu = take(nu), *cst = take(nc), *dyn = take(nx2), *ini = take(nc0);
  const double *sol = P.sol + (long long)b * P.sol_stride;
  for (int k = tid; k < nx; k += nthr)
    xs[k] = sol[m.x_off + k], gx[k] = 0.0;
  for (int k = tid; k < nu; k += nthr)
    us[k] = sol[m.u_off + k], gu[k] = 0.0;
  for (int k = tid; k < nc; k += nthr)
    vs[k] = sol[m.v_off + k], cst[k] = 0.0;
  for (int k = tid; k < nl; k += nthr)
    lt[k] = sol[m.l_off + k];
  for (int k = tid; k < nx2; k += nthr) {
    ln[k] = last ? 0.0 : sol[mn.l_off + k];
    xn[k] = last ? 0.0 : sol[mn.x_off + k];
    dyn[k] = 0.0;
  }
  for (int k = tid; k < nc0; k += nthr)
    ini[k] = 0.0;
  if (par)
    for (int k = tid; k < nst; k += nthr)
      th[k] = P.theta[(long long)b * P.nth0 + k];
  __syncthreads();

  const double *problem = P.prob + (long long)b * P.prob_stride;
  { // the knot record, tile after tile
    const double *rec = problem + m.in_off;
    const gar_knot_offsets o = gar_knot_layout(nx, nu, nc, nx2, nst);
    const bool pk = P.qr_packed && !last;
    const int nQ = pk ? nx * (nx + 1) / 2 : nx * nx, nR = pk ? nu * (nu + 1) / 2 : nu * nu;
    const int end = par ? o.total : o.Gth;
    for (int c0 = 0; c0 < end; c0 += GAR_KKT_TILE) {
      kkt_stage_range(tile, rec, c0, o.Q, o.Q + nQ, tid, nthr);
      kkt_stage_range(tile, rec, c0, o.S, o.R, tid, nthr);
      kkt_stage_range(tile, rec, c0, o.R, o.R + nR, tid, nthr);
      if (last) { // (A, B, f of the terminal knot: nothing of the residuals reads them)
        kkt_stage_range(tile, rec, c0, o.q, o.A, tid, nthr);
        kkt_stage_range(tile, rec, c0, o.C, end, tid, nthr);
      } else {
        kkt_stage_range(tile, rec, c0, o.q, end, tid, nthr);
      }
      __syncthreads();
      if (pk) {
        kkt_sym_packed(tile, c0, o.Q, nx, xs, gx, tid, nthr);
        kkt_sym_packed(tile, c0, o.R, nu, us, gu, tid, nthr);
      } else {
        kkt_block(tile, c0, o.Q, nx, nx, xs, gx, nullptr, nullptr, tid, nthr);
        kkt_block(tile, c0, o.R, nu, nu, us, gu, nullptr, nullptr, tid, nthr);
      }
      kkt_block(tile, c0, o.S, nx, nu, us, gx, xs, gu, tid, nthr);
      kkt_vector(tile, c0, o.q, nx, gx, tid, nthr);
      kkt_vector(tile, c0, o.r, nu, gu, tid, nthr);
      if (!last) {
        kkt_block(tile, c0, o.A, nx2, nx, xs, dyn, ln, gx, tid, nthr);
        kkt_block(tile, c0, o.B, nx2, nu, us, dyn, ln, gu, tid, nthr);
        kkt_vector(tile, c0, o.f, nx2, dyn, tid, nthr);
      }
      kkt_block(tile, c0, o.C, nc, nx, xs, cst, vs, gx, tid, nthr);
      kkt_block(tile, c0, o.D, nc, nu, us, cst, vs, gu, tid, nthr);
      kkt_vector(tile, c0, o.d, nc, cst, tid, nthr);
      if (par) {
        kkt_block(tile, c0, o.Gx, nx, nst, th, gx, nullptr, nullptr, tid, nthr);
        kkt_block(tile, c0, o.Gu, nu, nst, th, gu, nullptr, nullptr, tid, nthr);
      }
      __syncthreads();
    }
  }
  if (t == 0 && nc0 > 0) { // the initial condition: g0 + G0 x0 into the dynamics error, G0^T lbda0 into gx
    const double *rec = problem + P.G0_off; // (G0 opens the problem's record: 16-byte aligned as the knots are)
    const int oG = 0, og = (int)(P.g0_off - P.G0_off), end = og + nc0;
    for (int c0 = 0; c0 < end; c0 += GAR_KKT_TILE) {
      kkt_stage_range(tile, rec, c0, oG, oG + nc0 * nx, tid, nthr);
      kkt_stage_range(tile, rec, c0, og, end, tid, nthr);
      __syncthreads();
      kkt_block(tile, c0, oG, nc0, nx, xs, ini, lt, gx, tid, nthr);
      kkt_vector(tile, c0, og, nc0, ini, tid, nthr);
      __syncthreads();
    }
  }
  { // what no block carries, by the owners of the entries: -lbda_t, -x_{t+1}, -mueq v
    const int g = tid / GAR_KKT_GROUP, sub = tid % GAR_KKT_GROUP, ng = nthr / GAR_KKT_GROUP;
    if (sub == 0) {
      if (t > 0)
        for (int k = g; k < nx; k += ng)
          gx[k] -= lt[k];
      if (!last)
        for (int k = g; k < nx2; k += ng)
          dyn[k] -= xn[k];
      for (int k = g; k < nc; k += ng)
        cst[k] -= P.mueq * vs[k];
    }
  }
  __syncthreads();
  if (P.rhs) { // the vectors themselves: the right-hand side of a refinement step (device dimensions)
    double *out = P.rhs + (long long)b * P.rhs_stride + (long long)t * P.rhs_rec;
    for (int k = tid; k < nx; k += nthr)
      out[k] = gx[k];
    for (int k = tid; k < nu; k += nthr)
      out[nx + k] = gu[k];
    if (!last)
      for (int k = tid; k < nx2; k += nthr)
        out[refine_rhs_f(nx, nu) + k] = dyn[k];
    if (t == 0)
      for (int k = tid; k < nc0; k += nthr)
        P.rhs[(long long)b * P.rhs_stride + (long long)(N + 1) * P.rhs_rec + k] = ini[k];
  }
  // the four infinity norms: norm q by wave q mod #waves alone (its 64 lanes stride over the vector, six shuffles fold them)
  const int lane = tid & 63, wave = tid >> 6, nw = nthr >> 6;
  for (int q = 0; q < 4; ++q) {
    if (q % nw != wave)
      continue; // (wave-uniform)
    double v = 0.0;
    if (q == 0) {
      if (!last)
        for (int k = lane; k < nx2; k += 64)
          v = kkt_nanmax(v, fabs(dyn[k]));
      if (t == 0)
        for (int k = lane; k < nc0; k += 64)
          v = kkt_nanmax(v, fabs(ini[k]));
    } else {
      const double *r = q == 1 ? cst : q == 2 ? gx : gu;
      const int n = q == 1 ? nc : q == 2 ? nx : nu;
      for (int k = lane; k < n; k += 64)
        v = kkt_nanmax(v, fabs(r[k]));
    }
    for (int s = 32; s >= 1; s /= 2)
      v = kkt_nanmax(v, __shfl_xor(v, s));
    if (lane == 0)
      P.stage[((long long)b * (N + 1) + t) * 4 + q] = v;
  }
}

// grid (batch) x 64: the stage norms of one problem -> dynErr, cstErr, dualErr = max(gx, gu)
__global__ void __launch_bounds__(64) gar_kkt_reduce(KktParams P) {
  const int b = (int)blockIdx.x, lane = (int)threadIdx.x;
  const double *st = P.stage + (long long)b * (P.horizon + 1) * 4;
  double dynE = 0.0, cstE = 0.0, dualE = 0.0;
  for (int t = lane; t <= P.horizon; t += 64) {
    dynE = kkt_nanmax(dynE, st[4 * t]);
    cstE = kkt_nanmax(cstE, st[4 * t + 1]);
    dualE = kkt_nanmax(dualE, kkt_nanmax(st[4 * t + 2], st[4 * t + 3]));
  }
  for (int s = 32; s >= 1; s /= 2) {
    dynE = kkt_nanmax(dynE, __shfl_xor(dynE, s));
    cstE = kkt_nanmax(cstE, __shfl_xor(cstE, s));
    dualE = kkt_nanmax(dualE, __shfl_xor(dualE, s));
  }
  if (lane == 0) {
    P.err[3 * (long long)b] = dynE;
    P.err[3 * (long long)b + 1] = cstE;
    P.err[3 * (long long)b + 2] = dualE;
    if (P.gate) {
      const double e = kkt_nanmax(dynE, dualE);
      P.gate[b] = (P.status[b] == 0 && fabs(e) <= 1.7976931348623157e308 && !(e <= P.threshold)) ? 1 : 0;
    }
  }
}

} // namespace gar
