// TEST-ONLY, host only: aligator_amd/csrc/gar_record_io.hpp against element-by-element definitions written out here.
// Every put writes into a destination framed by sentinel doubles and is compared, bit for bit and over the whole frame,
// with an image built from the definition: real entries, dummy entries (exactly 0 / 1 / -1), untouched holes behind
// packed triangles, intact sentinels.  Every take must give the source back bit for bit.  Built with
// -fsanitize=address,undefined (tests/unit/Makefile: record_io); run by tests/test_record_io.py.
#include "gar_record_io.hpp"

#include <cstdio>
#include <vector>

namespace {

int g_checks = 0, g_failed = 0;
#define CHECK(cond, ...)                                                                                               \
  do {                                                                                                                 \
    ++g_checks;                                                                                                        \
    if (!(cond)) {                                                                                                     \
      ++g_failed;                                                                                                      \
      std::printf("FAILED %s:%d: %s -- ", __FILE__, __LINE__, #cond);                                                  \
      std::printf(__VA_ARGS__);                                                                                        \
      std::printf("\n");                                                                                               \
    }                                                                                                                  \
  } while (0)

constexpr double kSentinel = -7.03125e+200;
bool same_bits(const double *a, const double *b, size_t n) { return n == 0 || std::memcmp(a, b, sizeof(double) * n) == 0; }

unsigned long long g_seed = 88172645463325252ull;
double rnd() { // xorshift: values in (-1, 1), never zero, one or minus one
  g_seed ^= g_seed << 13, g_seed ^= g_seed >> 7, g_seed ^= g_seed << 17;
  const double v = (double)(g_seed >> 11) / 9007199254740992.0;
  return (v - 0.5) * 1.99 + 1e-3;
}
// a caller's r x c block, symmetric when square (the packed formats keep one triangle)
std::vector<double> source(int r, int c) {
  std::vector<double> a((size_t)r * c);
  for (int j = 0; j < c; ++j)
    for (int i = 0; i < r; ++i)
      a[(size_t)j * r + i] = (r == c && i < j) ? a[(size_t)i * r + j] : rnd();
  return a;
}

// THE DEFINITION: element (i, j) of the device's R x C block
double device_element(const BlockMap &m, const double *src, int i, int j) {
  if (i < m.r && j < m.c)
    return src ? src[(size_t)j * m.r + i] : 0.0;
  if (i >= m.r && j >= m.c && i - m.r == j - m.c)
    return m.diag;
  return 0.0;
}
// ... and where it is stored inside the block (-1: not stored)
long stored_at(const BlockMap &m, int i, int j) {
  if (m.store == kFull)
    return (long)j * m.R + i;
  return i >= j ? (long)i + ((2L * m.R - j - 1) * j) / 2 : -1; // LAPACK "L" packed: column after column
}

// a record of `doubles` with `front` sentinels before and 9 behind; `front` odd: the record is 8 bytes off 16
struct Frame {
  std::vector<double> buf;
  size_t front;
  Frame(size_t doubles, size_t front_) : buf(front_ + doubles + 9, kSentinel), front(front_) {}
  double *rec() { return buf.data() + front; }
};

void put_and_check(const BlockMap *maps, const double *const *src, int n, size_t doubles, bool nt, size_t front,
                   const char *what) {
  Frame got(doubles, front), want(doubles, front);
  for (int k = 0; k < n; ++k) {
    const BlockMap &m = maps[k];
    put_block(got.rec(), m, src[k], nt);
    long dummies = 0;
    for (int j = 0; j < m.C; ++j)
      for (int i = 0; i < m.R; ++i) {
        const long at = stored_at(m, i, j);
        if (at < 0)
          continue;
        const double v = device_element(m, src[k], i, j);
        want.rec()[m.off + at] = v;
        if (i >= m.r || j >= m.c) {
          ++dummies;
          CHECK(v == 0.0 || (v == m.diag && i - m.r == j - m.c), "%s block %d (%d, %d)", what, k, i, j);
        }
      }
    CHECK(m.store != kFull || dummies == (long)m.R * m.C - (long)m.r * m.c, "%s block %d", what, k);
    CHECK(m.off >= 0 && m.off + m.doubles() <= (int64_t)doubles, "%s block %d leaves the record", what, k);
  }
  CHECK(same_bits(got.buf.data(), want.buf.data(), got.buf.size()), "%s: record image (nt %d, front %zu)", what, (int)nt, front);
  // and back: the caller's blocks, both triangles of a packed one
  for (int k = 0; k < n; ++k) {
    const BlockMap &m = maps[k];
    const size_t sz = (size_t)m.r * m.c;
    std::vector<double> out(sz + 2, kSentinel), zeros(sz, 0.0);
    take_block(out.data() + 1, m, got.rec());
    CHECK(same_bits(out.data() + 1, src[k] ? src[k] : zeros.data(), sz), "%s block %d taken back", what, k);
    CHECK(out[0] == kSentinel && out[sz + 1] == kSentinel, "%s block %d take wrote outside", what, k);
  }
}

gar_stage_meta meta_of(int nx, int nu, int nc, int nx2, int nth) {
  gar_stage_meta m{};
  m.nx = nx, m.nu = nu, m.nc = nc, m.nx2 = nx2, m.nth = nth;
  return m;
}

// one knot, caller (nx, nu, nc, nth) -> device (NX, NU, nc, nth): maps, image, round trip
void check_knot(int nx, int nu, int NX, int NU, int nc, int nth, bool qr_lower, bool nt, size_t front, bool nulls,
                const char *what) {
  const gar_stage_meta u = meta_of(nx, nu, nc, nx, nth), d = meta_of(NX, NU, nc, NX, nth);
  BlockMap maps[16];
  knot_block_maps(maps, u, d, nth, qr_lower);
  // the C ABI's block order and shapes, the offsets of gar_knot_layout on either side
  const gar_knot_offsets a = gar_knot_layout(nx, nu, nc, nx, nth), b = gar_knot_layout(NX, NU, nc, NX, nth);
  const int32_t ao[16] = {a.Q, a.S, a.R, a.q, a.r, a.A, a.B, a.f, a.C, a.D, a.d, a.Gth, a.Gx, a.Gu, a.Gv, a.gamma};
  const int32_t bo[16] = {b.Q, b.S, b.R, b.q, b.r, b.A, b.B, b.f, b.C, b.D, b.d, b.Gth, b.Gx, b.Gu, b.Gv, b.gamma};
  const int rc[16][2] = {{nx, nx}, {nx, nu}, {nu, nu}, {nx, 1}, {nu, 1}, {nx, nx}, {nx, nu}, {nx, 1},
                         {nc, nx}, {nc, nu}, {nc, 1}, {nth, nth}, {nx, nth}, {nu, nth}, {nc, nth}, {nth, 1}};
  const int RC[16][2] = {{NX, NX}, {NX, NU}, {NU, NU}, {NX, 1}, {NU, 1}, {NX, NX}, {NX, NU}, {NX, 1},
                         {nc, NX}, {nc, NU}, {nc, 1}, {nth, nth}, {NX, nth}, {NU, nth}, {nc, nth}, {nth, 1}};
  std::vector<std::vector<double>> data(16);
  const double *src[16];
  for (int k = 0; k < 16; ++k) {
    const BlockMap &m = maps[k];
    CHECK(m.r == rc[k][0] && m.c == rc[k][1] && m.R == RC[k][0] && m.C == RC[k][1], "%s block %d shape", what, k);
    CHECK(m.off == bo[k] && m.uoff == ao[k], "%s block %d offsets", what, k);
    CHECK(m.store == ((k == 0 || k == 2) && qr_lower ? kLower : kFull), "%s block %d store", what, k);
    CHECK(m.diag == (k == 0 || k == 2 ? 1.0 : 0.0), "%s block %d diag", what, k);
    data[k] = source(m.r, m.c);
    src[k] = (nulls && k >= 8) ? nullptr : data[k].data(); // C D d Gth Gx Gu Gv gamma may be absent: zeros
  }
  put_and_check(maps, src, 16, (size_t)gar_knot_doubles(NX, NU, nc, NX, nth), nt, front, what);
}

void check_init(int nc0, int nx, int NX, const char *what) {
  const int NC0 = nc0 + (NX - nx);
  BlockMap maps[2];
  init_block_maps(maps, nc0, nx, NC0, NX, 0, (int64_t)NC0 * NX, 0, (int64_t)nc0 * nx);
  const std::vector<double> G0 = source(nc0, nx), g0 = source(nc0, 1);
  const double *src[2] = {G0.data(), g0.data()};
  put_and_check(maps, src, 2, (size_t)NC0 * NX + NC0, false, 4, what);
  // [G0 0; 0 -I] | [g0; 0], entry by entry
  Frame f((size_t)NC0 * NX + NC0, 5);
  put_block(f.rec(), maps[0], G0.data(), false);
  put_block(f.rec(), maps[1], g0.data(), false);
  for (int j = 0; j < NX; ++j)
    for (int i = 0; i < NC0; ++i) {
      const double want = (i < nc0 && j < nx) ? G0[(size_t)j * nc0 + i] : (i >= nc0 && j >= nx && i - nc0 == j - nx) ? -1.0 : 0.0;
      CHECK(f.rec()[(size_t)j * NC0 + i] == want, "%s G0 (%d, %d)", what, i, j);
    }
  for (int i = 0; i < NC0; ++i)
    CHECK(f.rec()[(size_t)NC0 * NX + i] == (i < nc0 ? g0[i] : 0.0), "%s g0 %d", what, i);
}

// Vxx kept as its packed lower triangle, rectangular packed (gar_layout.h: gar_sym_index), n even; the caller takes
// the leading nx x nx part
void check_sym_take(int nx, int n) {
  const std::vector<double> V = source(n, n);
  std::vector<double> blk((size_t)n * n, kSentinel);
  for (int c = 0; c < n / 2; ++c) { // super-column c: column c's rows c .. n-1, then column n-1-c's rows n-1-c .. n-1
    double *p = blk.data() + (size_t)c * (n + 1);
    for (int i = c; i < n; ++i)
      *p++ = V[(size_t)c * n + i];
    for (int i = n - 1 - c; i < n; ++i)
      *p++ = V[(size_t)(n - 1 - c) * n + i];
  }
  std::vector<double> out((size_t)nx * nx + 2, kSentinel);
  take_block(out.data() + 1, BlockMap{nx, nx, n, n, 0, 0, 0.0, kSym}, blk.data());
  for (int j = 0; j < nx; ++j)
    for (int i = 0; i < nx; ++i)
      CHECK(out[1 + (size_t)j * nx + i] == V[(size_t)j * n + i], "sym take n %d (%d, %d)", n, i, j);
  CHECK(out[0] == kSentinel && out.back() == kSentinel, "sym take n %d wrote outside", n);
}

// gain rows: an NR x NC device block in either storage order, the caller's rows through a RowMap
void check_gains(int NR, int NC, bool t2, RowMap rows, int nc, const char *what) {
  const int pairs = (NC + 1) / 2;
  std::vector<double> blk(t2 ? (size_t)pairs * 2 * NR : (size_t)NR * NC, kSentinel);
  auto value = [](int row, int j) { return 1000.0 * row + j + 0.5; };
  for (int row = 0; row < NR; ++row)
    for (int j = 0; j < NC; ++j) // fbT2: column pairs, row after row inside a pair
      blk[t2 ? (size_t)(j / 2) * (size_t)(2 * NR) + (size_t)(2 * row + j % 2) : (size_t)row * NC + j] = value(row, j);
  std::vector<double> out((size_t)rows.n * nc + 2, kSentinel);
  take_gains(out.data() + 1, blk.data(), t2, NR, NC, rows, nc);
  for (int i = 0; i < rows.n; ++i) {
    const int row = i < rows.lead ? i : i + rows.skip;
    for (int j = 0; j < nc; ++j)
      CHECK(out[1 + (size_t)i * nc + j] == value(row, j), "%s (%d, %d)", what, i, j);
  }
  CHECK(out[0] == kSentinel && out.back() == kSentinel, "%s wrote outside", what);
  take_gains(nullptr, blk.data(), t2, NR, NC, rows, nc); // a null output is allowed
}

} // namespace

int main() {
  for (int lower = 0; lower < 2; ++lower) {
    check_knot(4, 2, 8, 4, 0, 0, lower, false, 4, false, "(4,2)->(8,4)");
    check_knot(7, 3, 8, 4, 0, 0, lower, false, 5, false, "(7,3)->(8,4)");
    check_knot(12, 6, 12, 8, 0, 0, lower, false, 4, false, "(12,6)->(12,8)"); // r == R: the one-piece path
    for (int nt = 0; nt < 2; ++nt)                                             // Q: 3136 doubles, over the threshold of 512
      for (size_t front = 4; front < 6; ++front)                               // front 5: the record is 8 bytes off 16
        check_knot(56, 22, 56, 24, 0, 0, lower, nt, front, false, "(56,22)->(56,24)");
    check_knot(8, 4, 8, 4, 0, 0, lower, false, 4, false, "(8,4) unpadded");
    check_knot(36, 12, 36, 12, 0, 0, lower, true, 5, false, "(36,12) unpadded, non-temporal");
    check_knot(7, 0, 8, 0, 0, 0, false, false, 4, false, "terminal knot, nu = 0, padded");
    check_knot(8, 0, 8, 0, 4, 0, false, false, 4, false, "terminal knot, nu = 0, nc = 4");
    check_knot(6, 3, 6, 3, 3, 2, lower, false, 5, false, "nc = 3, stored nth = 2");
    check_knot(6, 3, 6, 3, 3, 2, lower, false, 4, true, "nc = 3, stored nth = 2, null C .. gamma");
    check_knot(8, 4, 8, 4, 4, 0, lower, true, 4, true, "(8,4,4), null C D d");
  }
  { // a null source of a padded and of a packed block: zeros, the dummy diagonal all the same
    const BlockMap maps[3] = {{3, 3, 5, 5, 0, 0, 1.0, kFull}, {3, 3, 5, 5, 25, 0, 1.0, kLower}, {0, 0, 4, 4, 50, 0, 1.0, kLower}};
    const double *none[3] = {nullptr, nullptr, nullptr};
    put_and_check(maps, none, 3, 50 + 16, false, 5, "null sources");
  }
  check_init(4, 4, 8, "init nc0 = nx");
  check_init(2, 7, 8, "init nc0 < nx");
  check_init(0, 6, 8, "init nc0 = 0");
  check_init(5, 5, 5, "init unpadded");
  check_sym_take(8, 8);
  check_sym_take(6, 8);
  check_sym_take(36, 36);
  for (int t2 = 0; t2 < 2; ++t2) {
    check_gains(12, 8, t2, RowMap{12, 12, 0}, 8, "gains, every row");
    check_gains(12, 8, t2, RowMap{10, 3, 1}, 7, "gains, padded (7,3)->(8,4)");
    check_gains(12, 7, t2, RowMap{12, 12, 0}, 7, "gains, odd column count");
    check_gains(12, 8, t2, RowMap{4, 4, 0}, 8, "gains, terminal knot given with nx2 = 0: nc rows");
    check_gains(16, 1, false, RowMap{11, 7, 1}, 1, "kkt0.ff, padded");
  }
  std::printf("%d checks, %d failed\n", g_checks, g_failed);
  if (g_failed == 0)
    std::printf("record io ok\n");
  return g_failed == 0 ? 0 : 1;
}
