// gar_record_io.hpp -- how a caller's block maps onto a device record, stated ONCE for the host code: upload
// (gar_hip_upload_stage, gar_hip_set_init, gar_hip_upload_packed), download (gar_hip_download_packed) and the getters
// (gar_entry_io.hpp).  The rules:
//   * padding onto a specialised shape (gar_hip_solver::padded): the caller's r x c block is the top-left corner of the
//     device's R x C one; dummy controls and states get Q = R = I on the dummy diagonal, zeros elsewhere, and the
//     initial constraint becomes [G0 0; 0 -I] | [g0; 0] -- the -I rows pin the dummy states to zero;
//   * Q and R of the knots t < N as packed lower triangles (qr_packed; gar_layout.h: gar_lower_index), the rest of
//     the block -- the hole -- never written;
//   * Vxx as its packed lower triangle (vxx_packed; gar_layout.h: gar_sym_index);
//   * fb and fth in the fbT2 order of the specialised families (gar_mfma.hpp);
//   * gain rows: the real controls and states of a padded block (rows [0, nu) and [NU, NU + nx)), the leading nc rows
//     of a terminal knot given with nx2 = 0 (term_grown).
// The kernels that apply the same rules on the device -- gar_update_lq, gar_update_lq_padded, gar_gather_gains
// (gar_generic.hpp) -- are written out on their own.  Host only: no HIP call, nothing of gar_hip_solver; internal
// linkage, like gar_host.hpp.
#pragma once

#include "gar_layout.h"

#include <cstddef>
#include <cstdint>
#include <cstring>
#if defined(__SSE2__)
#include <emmintrin.h>
#endif

namespace {

// Host copy into the pinned staging area with non-temporal stores: the destination is written once and next read by
// the DMA engine, so it should not be pulled into (read-for-ownership) nor left in the caches of the packing core --
// a third less memory traffic than memcpy's cached stores on the 19 MB of a (56, 22), N = 256 problem (measured on
// the GPU box's host: 920 -> 560 us).  Only for problems that do not fit the last-level cache next to their source
// (LayoutState::stage_nt): the 7.6 MB of the north-star problem pack at cache speed with plain stores (150 us
// against 440 us with non-temporal ones).  The stores are weakly ordered: stage_fence before a DMA engine reads them.
inline void stage_copy(double *dst, const double *src, size_t n, bool nt) {
#if defined(__SSE2__) && !defined(__HIP_DEVICE_COMPILE__)
  if (nt && n >= 512) {
    size_t i = 0;
    if (reinterpret_cast<uintptr_t>(dst) & 15) // 8-byte aligned at least: one scalar brings it to 16
      dst[i] = src[i], ++i;
    for (; i + 8 <= n; i += 8) {
      const __m128d a = _mm_loadu_pd(src + i), b = _mm_loadu_pd(src + i + 2), c = _mm_loadu_pd(src + i + 4),
                    d = _mm_loadu_pd(src + i + 6);
      _mm_stream_pd(dst + i, a);
      _mm_stream_pd(dst + i + 2, b);
      _mm_stream_pd(dst + i + 4, c);
      _mm_stream_pd(dst + i + 6, d);
    }
    for (; i < n; ++i)
      dst[i] = src[i];
    return;
  }
#endif
  std::memcpy(dst, src, sizeof(double) * n);
}
inline void stage_fence() {
#if defined(__SSE2__) && !defined(__HIP_DEVICE_COMPILE__)
  _mm_sfence();
#endif
}

// ---- blocks -------------------------------------------------------------------------------------------------------
enum BlockStore { kFull = 0, kLower, kSym }; // column-major R x C | gar_lower_index(R, i, j) | gar_sym_index(1, R, i, j)

// The caller's column-major r x c block inside the device's R x C one (r <= R, c <= C; an unpadded solver is r == R,
// c == C), at `off` of the device record and `uoff` of the caller's packed record; `diag` on the device block's
// entries (r + i, c + i) -- the diagonal beyond the caller's block.
struct BlockMap {
  int r, c, R, C;
  int64_t off, uoff;
  double diag;
  BlockStore store;
  int64_t doubles() const { return store == kFull ? (int64_t)R * C : (int64_t)R * (R + 1) / 2; } // what is written
};

// the 16 blocks of knot t in the C ABI's order Q S R q r A B f C D d Gth Gx Gu Gv gamma: u / d = the knot's meta in the
// caller's / the device's layout, nth_stored of both records, qr_lower = (qr_packed && t < N)
inline void knot_block_maps(BlockMap out[16], const gar_stage_meta &u, const gar_stage_meta &d, int nth_stored,
                            bool qr_lower) {
  const gar_knot_offsets a = gar_knot_layout(u.nx, u.nu, u.nc, u.nx2, nth_stored),
                         b = gar_knot_layout(d.nx, d.nu, d.nc, d.nx2, nth_stored);
  const BlockStore qr = qr_lower ? kLower : kFull;
  const int nth = nth_stored;
  out[0] = {u.nx, u.nx, d.nx, d.nx, b.Q, a.Q, 1.0, qr};
  out[1] = {u.nx, u.nu, d.nx, d.nu, b.S, a.S, 0.0, kFull};
  out[2] = {u.nu, u.nu, d.nu, d.nu, b.R, a.R, 1.0, qr};
  out[3] = {u.nx, 1, d.nx, 1, b.q, a.q, 0.0, kFull};
  out[4] = {u.nu, 1, d.nu, 1, b.r, a.r, 0.0, kFull};
  out[5] = {u.nx2, u.nx, d.nx2, d.nx, b.A, a.A, 0.0, kFull};
  out[6] = {u.nx2, u.nu, d.nx2, d.nu, b.B, a.B, 0.0, kFull};
  out[7] = {u.nx2, 1, d.nx2, 1, b.f, a.f, 0.0, kFull};
  out[8] = {u.nc, u.nx, d.nc, d.nx, b.C, a.C, 0.0, kFull};
  out[9] = {u.nc, u.nu, d.nc, d.nu, b.D, a.D, 0.0, kFull};
  out[10] = {u.nc, 1, d.nc, 1, b.d, a.d, 0.0, kFull};
  out[11] = {nth, nth, nth, nth, b.Gth, a.Gth, 0.0, kFull};
  out[12] = {u.nx, nth, d.nx, nth, b.Gx, a.Gx, 0.0, kFull};
  out[13] = {u.nu, nth, d.nu, nth, b.Gu, a.Gu, 0.0, kFull};
  out[14] = {u.nc, nth, d.nc, nth, b.Gv, a.Gv, 0.0, kFull};
  out[15] = {nth, 1, nth, 1, b.gamma, a.gamma, 0.0, kFull};
}

// G0 | g0: the caller's nc0 x nx and nc0 inside the device's NC0 x NX and NC0 (NC0 - nc0 = NX - nx), each at its own
// offset in both records
inline void init_block_maps(BlockMap out[2], int nc0, int nx, int NC0, int NX, int64_t G0_off, int64_t g0_off,
                            int64_t uG0_off, int64_t ug0_off) {
  out[0] = {nc0, nx, NC0, NX, G0_off, uG0_off, -1.0, kFull};
  out[1] = {nc0, 1, NC0, 1, g0_off, ug0_off, 0.0, kFull};
}

// `src` (the caller's block; null: zeros) into the device record `rec`.  r == R: the real columns in one piece,
// non-temporal when `nt` says so (stage_copy); otherwise column by column, the dummy rows zeroed beside each.  A
// packed triangle (kLower) is written column by column; its hole is not.
inline void put_block(double *rec, const BlockMap &m, const double *src, bool nt) {
  double *dst = rec + m.off;
  const size_t r = (size_t)m.r, R = (size_t)m.R;
  if (m.store == kLower) {
    for (int j = 0; j < m.R; ++j) {
      double *col = dst + gar_lower_index(m.R, j, j);
      if (j < m.r && src)
        std::memcpy(col, src + (size_t)j * r + j, sizeof(double) * (size_t)(m.r - j));
      else if (j < m.r)
        std::memset(col, 0, sizeof(double) * (size_t)(m.r - j));
      const int top = j < m.r ? m.r - j : 0; // the dummy rows of this column
      std::memset(col + top, 0, sizeof(double) * (size_t)(m.R - j - top));
      if (j >= m.r)
        col[0] = m.diag;
    }
    return;
  }
  if (R * (size_t)m.C == 0)
    return;
  if (!src) {
    std::memset(dst, 0, sizeof(double) * R * (size_t)m.C);
  } else if (r == R) {
    stage_copy(dst, src, r * (size_t)m.c, nt);
    std::memset(dst + r * (size_t)m.c, 0, sizeof(double) * R * (size_t)(m.C - m.c));
  } else {
    for (int j = 0; j < m.c; ++j) {
      std::memcpy(dst + (size_t)j * R, src + (size_t)j * r, sizeof(double) * r);
      std::memset(dst + (size_t)j * R + r, 0, sizeof(double) * (R - r));
    }
    std::memset(dst + (size_t)m.c * R, 0, sizeof(double) * R * (size_t)(m.C - m.c));
  }
  if (m.diag != 0.0)
    for (int i = 0; m.r + i < m.R && m.c + i < m.C; ++i)
      dst[(size_t)(m.c + i) * R + (size_t)(m.r + i)] = m.diag;
}

// the caller's r x c block out of the device record: `dst` column-major; a packed block gives both triangles
inline void take_block(double *dst, const BlockMap &m, const double *rec) {
  const double *src = rec + m.off;
  const size_t r = (size_t)m.r;
  if (m.store == kFull) {
    for (int j = 0; j < m.c; ++j)
      std::memcpy(dst + (size_t)j * r, src + (size_t)j * (size_t)m.R, sizeof(double) * r);
    return;
  }
  for (int j = 0; j < m.r; ++j)
    for (int i = j; i < m.r; ++i)
      dst[(size_t)j * r + i] = dst[(size_t)i * r + j] =
          src[m.store == kLower ? gar_lower_index(m.R, i, j) : gar_sym_index(1, m.R, i, j)];
}

// ---- gain rows ----------------------------------------------------------------------------------------------------
// The caller's rows of a device gain block: row i < lead is the device's row i, row i >= lead its row i + skip.
// Padding: the real controls, then the real states -- {nu + nx, nu, NU - nu}; kkt0 under padding: x0, then lbd0 --
// {nx + nc0, nx, NX - nx}; a terminal knot given with nx2 = 0: its nc leading rows -- {nc, nc, 0}.
struct RowMap {
  int n, lead, skip;
  int operator()(int i) const { return i < lead ? i : i + skip; }
};

// element (row, j) of an NR x NC gain block `blk`: row-major, or (t2) the fbT2 device order of the specialised families
inline double gain_at(const double *blk, bool t2, int NR, int NC, int row, int j) {
  return blk[t2 ? (size_t)(j >> 1) * (size_t)(2 * NR) + (size_t)(2 * row + (j & 1)) : (size_t)row * (size_t)NC + (size_t)j];
}

// the caller's rows.n x nc block (row-major; null: nothing to do) out of the device's NR x NC one
inline void take_gains(double *dst, const double *blk, bool t2, int NR, int NC, RowMap rows, int nc) {
  if (!dst)
    return;
  for (int i = 0; i < rows.n; ++i)
    for (int j = 0; j < nc; ++j)
      dst[(size_t)i * (size_t)nc + (size_t)j] = gain_at(blk, t2, NR, NC, rows(i), j);
}

} // namespace
