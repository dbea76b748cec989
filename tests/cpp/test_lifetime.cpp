// test_lifetime.cpp -- who owns the solver's device buffers, pinned buffers, streams and events, seen from outside: every
// scenario below drives the C ABI (include/gar_hip.h, nothing else of the library) through a sequence that makes
// buffers, streams and events come and go -- lazily created ones, a rebuild while they are live, refused requests --
// and ends in gar_hip_solver_destroy.  Linked against the wave emulator's build of the library (tests/emu), where a
// device buffer, an event and a stream are plain malloc blocks, and built WITH it under -fsanitize=address
// (make -C tests/cpp asan): a missed release is a leak report at exit, a double release or a use after a rebuild an
// immediate error.  After each scenario the change of gar_hip_debug_alloc_count is printed and compared with kExpected
// -- the counts this program printed on the commit BEFORE the owners of csrc/gar_host.hpp existed: "the same allocations".
#include "gar_hip.h"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

extern "C" void emu_set_device_count(int n); // tests/emu/emu_runtime.cpp: the emulator's only knob used here

namespace {

int g_failures = 0;
#define CHECK(cond)                                                                                                    \
  do {                                                                                                                 \
    if (!(cond)) {                                                                                                     \
      std::printf("  CHECK failed, line %d: %s   [%s]\n", __LINE__, #cond, gar_hip_last_error());                      \
      ++g_failures;                                                                                                    \
    }                                                                                                                  \
  } while (0)

const double kMu = 1e-8;

double rnd() { // (a fixed sequence: the program allocates the same on every run)
  static uint64_t x = 88172645463325252ull;
  x ^= x << 13, x ^= x >> 7, x ^= x << 17;
  return (double)(x >> 11) / (double)(1ull << 53) - 0.5;
}

struct Knot {
  int32_t d[5];
  std::vector<double> Q, S, R, q, r, A, B, f, C, D, dd;
};
// Q = R = I, S = 0, A, B, C random, D = 0 (what every constrained family and the folds take)
Knot make_knot(int nx, int nu, int nc, int nx2) {
  Knot k{{nx, nu, nc, nx2, 0}, {}, {}, {}, {}, {}, {}, {}, {}, {}, {}, {}};
  auto fill = [](std::vector<double> &v, size_t n, double scale) {
    v.resize(n);
    for (double &x : v)
      x = scale * rnd();
  };
  k.Q.assign((size_t)nx * nx, 0.0), k.R.assign((size_t)nu * nu, 0.0), k.S.assign((size_t)nx * nu, 0.0);
  for (int i = 0; i < nx; ++i)
    k.Q[(size_t)i * nx + i] = 1.0;
  for (int i = 0; i < nu; ++i)
    k.R[(size_t)i * nu + i] = 1.0;
  fill(k.q, nx, 1.0), fill(k.r, nu, 1.0), fill(k.A, (size_t)nx2 * nx, 0.6), fill(k.B, (size_t)nx2 * nu, 1.0), fill(k.f, nx2, 1.0);
  fill(k.C, (size_t)nc * nx, 1.0), fill(k.dd, nc, 1.0);
  k.D.assign((size_t)nc * nu, 0.0);
  return k;
}
struct Problem {
  std::vector<Knot> knots;
  std::vector<double> G0, g0; // x0 pinned: G0 = -I
  std::vector<int32_t> dims5() const {
    std::vector<int32_t> d;
    for (const Knot &k : knots)
      d.insert(d.end(), k.d, k.d + 5);
    return d;
  }
  int horizon() const { return (int)knots.size() - 1; }
  int nc0() const { return knots[0].d[0]; }
};
// N knots (nx, nu, nc) and the terminal one, without controls (what the specialised families take), with term_nc
// constraints when given
Problem make_problem(int nx, int nu, int nc, int N, int term_nc = -1) {
  Problem p;
  for (int t = 0; t <= N; ++t)
    p.knots.push_back(t == N ? make_knot(nx, 0, term_nc >= 0 ? term_nc : nc, nx) : make_knot(nx, nu, nc, nx));
  p.G0.assign((size_t)nx * nx, 0.0);
  for (int i = 0; i < nx; ++i)
    p.G0[(size_t)i * nx + i] = -1.0;
  p.g0.resize((size_t)nx);
  for (double &x : p.g0)
    x = rnd();
  return p;
}
const double *ptr(const std::vector<double> &v) { return v.empty() ? nullptr : v.data(); }
int upload_knot(gar_hip_solver *s, int b, int t, const Knot &k) {
  return gar_hip_upload_stage(s, b, t, ptr(k.Q), ptr(k.S), ptr(k.R), ptr(k.q), ptr(k.r), ptr(k.A), ptr(k.B), ptr(k.f), ptr(k.C),
                              ptr(k.D), ptr(k.dd), nullptr, nullptr, nullptr, nullptr, nullptr);
}
void upload(gar_hip_solver *s, const Problem &p, int batch) {
  for (int b = 0; b < batch; ++b) {
    for (int t = 0; t <= p.horizon(); ++t)
      CHECK(upload_knot(s, b, t, p.knots[(size_t)t]) == GAR_HIP_OK);
    CHECK(gar_hip_set_init(s, b, p.G0.data(), p.g0.data()) == GAR_HIP_OK);
  }
}
// backward + forward + the bulk read-back; the solution record, for comparisons
std::vector<double> solve(gar_hip_solver *s) {
  CHECK(gar_hip_backward(s, kMu) == GAR_HIP_OK);
  CHECK(gar_hip_num_failed(s) == 0);
  CHECK(gar_hip_forward(s, nullptr) == GAR_HIP_OK);
  CHECK(gar_hip_fetch_results(s, 0, 3) == GAR_HIP_OK);
  int64_t offs[3];
  const double *h = gar_hip_host_results(s, offs);
  CHECK(h != nullptr);
  const size_t n = (size_t)gar_hip_solution_doubles(s);
  std::vector<double> sol(h ? h + offs[0] : nullptr, h ? h + offs[0] + n : nullptr);
  for (double x : sol)
    if (!(x == x) || x > 1e12 || x < -1e12) {
      CHECK(!"finite solution");
      break;
    }
  return sol;
}

// ---- the scenarios ------------------------------------------------------------------------------------------------
// 1: serial (8, 4), N = 3 -- every lazily created member live at destroy; 2 (cycle = true): then a ring cycle_append
// and a rebuilding one while they are live.  (The terminal knot has two constraints: gar_hip_get_kkt's staging grows;
// the any-dimension kernels serve it, scenarios 3 and 8 run the (8, 4) family.)
void serial_all_lazy(int batch, bool cycle) {
  Problem p = make_problem(8, 4, 0, 3, 2);
  const std::vector<int32_t> dims = p.dims5();
  gar_hip_solver *s = gar_hip_solver_create(0, 3, dims.data(), p.nc0(), batch, 1);
  CHECK(s != nullptr);
  if (!s)
    return;
  upload(s, p, batch);
  solve(s);
  CHECK(gar_hip_prefetch_gains(s, 0) == GAR_HIP_OK);
  CHECK(gar_hip_fetch_results(s, 0, 3) == GAR_HIP_OK);
  double kkt[16];
  CHECK(gar_hip_get_kkt(s, 0, 3, kMu, kkt) == GAR_HIP_OK); // 2 x 2 ...
  CHECK(gar_hip_get_kkt(s, 0, 0, kMu, kkt) == GAR_HIP_OK); // ... then 4 x 4: regrown
  long long stamps[64];
  CHECK(gar_hip_debug_trace(s, 1, stamps) == GAR_HIP_OK);
  CHECK(gar_hip_debug_trace(s, 0, stamps) == GAR_HIP_OK);
  CHECK(gar_hip_debug_trace(s, 1, stamps) == GAR_HIP_OK); // (live at destroy / at the rebuild)
  CHECK(gar_hip_set_timing(s, 1) == GAR_HIP_OK);
  { // (on the emulator device memory is host memory: a zero derivative buffer)
    std::vector<double> deriv((size_t)gar_hip_deriv_doubles(s) * (size_t)batch, 0.0);
    CHECK(gar_hip_update_lq_subproblem_device(s, deriv.data(), 0.0, 1) == GAR_HIP_OK);
    CHECK(gar_hip_sync(s) == GAR_HIP_OK);
  }
  { // the whole problem and backward in one call (one problem: a batch is refused before anything is made)
    std::vector<const double *> blocks;
    for (const Knot &k : p.knots)
      for (const double *b : {ptr(k.Q), ptr(k.S), ptr(k.R), ptr(k.q), ptr(k.r), ptr(k.A), ptr(k.B), ptr(k.f), ptr(k.C), ptr(k.D),
                              ptr(k.dd), (const double *)nullptr, (const double *)nullptr, (const double *)nullptr,
                              (const double *)nullptr, (const double *)nullptr})
        blocks.push_back(b);
    const int rc = gar_hip_backward_blocks(s, blocks.data(), p.G0.data(), p.g0.data(), kMu);
    CHECK(batch == 1 ? rc == GAR_HIP_OK : rc == GAR_HIP_ERR_ARG);
    if (batch == 1) {
      CHECK(gar_hip_forward(s, nullptr) == GAR_HIP_OK);
      CHECK(gar_hip_fetch_results(s, 0, 3) == GAR_HIP_OK);
    } else {
      upload(s, p, batch);
    }
  }
  if (cycle) {
    CHECK(gar_hip_cycle_append(s, p.knots[0].d) == GAR_HIP_OK); // same dimensions: the ring, nothing is freed
    solve(s);
    const Knot other = make_knot(8, 3, 0, 8);
    CHECK(gar_hip_cycle_append(s, other.d) == GAR_HIP_OK); // other dimensions: rebuilt, every lazy buffer live
    p.knots.erase(p.knots.begin());
    p.knots.insert(p.knots.end() - 1, other);
    upload(s, p, batch);
    solve(s);
  }
  gar_hip_solver_destroy(s);
}

// 3: the pipelined schedule asked for again and again
void pipeline_again() {
  Problem p = make_problem(8, 4, 0, 3);
  const std::vector<int32_t> dims = p.dims5();
  gar_hip_solver *s = gar_hip_solver_create(0, 3, dims.data(), p.nc0(), 2, 1);
  CHECK(s != nullptr);
  if (!s)
    return;
  CHECK(gar_hip_set_pipeline(s, 2) == GAR_HIP_OK);
  CHECK(gar_hip_set_pipeline(s, 2) == GAR_HIP_OK);
  CHECK(gar_hip_set_pipeline(s, 0) == GAR_HIP_OK);
  CHECK(gar_hip_set_pipeline(s, 2) == GAR_HIP_OK);
  CHECK(gar_hip_pipeline(s) == 2);
  upload(s, p, 2);
  CHECK(gar_hip_backward_async(s, kMu) == GAR_HIP_OK);
  CHECK(gar_hip_forward_async(s, nullptr) == GAR_HIP_OK);
  CHECK(gar_hip_sync(s) == GAR_HIP_OK);
  CHECK(gar_hip_num_failed(s) == 0);
  gar_hip_solver_destroy(s);
}

// 4: leg mode -- plain, constrained knots (the folded second layout), a ranked pair (the gathered boundary buffer)
void leg_modes() {
  for (int nc : {0, 4}) {
    Problem p = make_problem(8, 4, nc, 7);
    const std::vector<int32_t> dims = p.dims5();
    gar_hip_solver *s = gar_hip_solver_create(0, 7, dims.data(), p.nc0(), 1, 3);
    CHECK(s != nullptr);
    if (!s)
      continue;
    upload(s, p, 1);
    solve(s);
    CHECK(gar_hip_device_boundary_all(s) == gar_hip_device_boundary_local(s)); // one rank: one buffer
    gar_hip_solver_destroy(s);
  }
  Problem p = make_problem(8, 4, 0, 7);
  const std::vector<int32_t> dims = p.dims5();
  for (int rank = 0; rank < 2; ++rank) {
    gar_hip_solver *s = gar_hip_solver_create_ranked(0, 7, dims.data(), p.nc0(), 1, 3, rank, 2);
    CHECK(s != nullptr);
    if (!s)
      continue;
    upload(s, p, 1);
    CHECK(gar_hip_backward_legs_async(s, kMu) == GAR_HIP_OK);
    CHECK(gar_hip_sync(s) == GAR_HIP_OK);
    CHECK(gar_hip_device_boundary_all(s) != nullptr && gar_hip_device_boundary_all(s) != gar_hip_device_boundary_local(s));
    gar_hip_solver_destroy(s);
  }
}

// 5: the stage-dense solver
void dense() {
  Problem p = make_problem(6, 3, 2, 3);
  const std::vector<int32_t> dims = p.dims5();
  gar_hip_solver *s = gar_hip_solver_create_dense(0, 3, dims.data(), p.nc0(), 1);
  CHECK(s != nullptr);
  if (!s)
    return;
  upload(s, p, 1);
  solve(s);
  gar_hip_solver_destroy(s);
}

// 6: the serial fold: a terminal knot with four constraints, D = 0, on the unconstrained (8, 4) family
void serial_fold() {
  CHECK(gar_hip_set_option("GAR_HIP_SERIAL_FOLD", "1") == GAR_HIP_OK);
  Problem p = make_problem(8, 4, 0, 3, 4);
  const std::vector<int32_t> dims = p.dims5();
  gar_hip_solver *s = gar_hip_solver_create(0, 3, dims.data(), p.nc0(), 2, 1);
  CHECK(gar_hip_set_option("GAR_HIP_SERIAL_FOLD", nullptr) == GAR_HIP_OK);
  CHECK(s != nullptr);
  if (!s)
    return;
  CHECK(std::strstr(gar_hip_kernel_name(s), "+fold") != nullptr);
  upload(s, p, 2);
  solve(s);
  CHECK(gar_hip_cycle_append(s, p.knots[0].d) == GAR_HIP_OK); // the ring turns both layouts
  solve(s);
  gar_hip_solver_destroy(s);
}

// 7: one handle over two (emulated) devices
void multi_device() {
  emu_set_device_count(2);
  Problem p = make_problem(8, 4, 0, 7);
  const std::vector<int32_t> dims = p.dims5();
  const int devs[2] = {0, 1};
  gar_hip_solver *s = gar_hip_multi_create(2, devs, 7, dims.data(), p.nc0(), 1, 4);
  CHECK(s != nullptr);
  if (s) {
    CHECK(gar_hip_num_devices(s) == 2);
    upload(s, p, 1);
    solve(s); // (the merged pinned record)
    const Knot other = make_knot(8, 3, 0, 8);
    CHECK(gar_hip_cycle_append(s, other.d) == GAR_HIP_OK);
    p.knots.erase(p.knots.begin());
    p.knots.insert(p.knots.end() - 1, other);
    upload(s, p, 1);
    solve(s);
    gar_hip_solver_destroy(s);
  }
  emu_set_device_count(1);
}

// 8: what the library refuses
void refusals() {
  {
    Problem p = make_problem(8, 4, 0, 3);
    const std::vector<int32_t> dims = p.dims5();
    CHECK(gar_hip_solver_create(0, 3, dims.data(), p.nc0(), 1, 6) == nullptr); // more legs than stages
  }
  { // a rejected cycle_append after two ring cycles leaves the solver solving as before
    Problem p = make_problem(8, 4, 0, 6);
    const std::vector<int32_t> dims = p.dims5();
    gar_hip_solver *s = gar_hip_solver_create(0, 6, dims.data(), p.nc0(), 1, 1);
    CHECK(s != nullptr);
    if (s) {
      upload(s, p, 1);
      for (int i = 0; i < 2; ++i) {
        CHECK(gar_hip_cycle_append(s, p.knots[0].d) == GAR_HIP_OK);
        CHECK(upload_knot(s, 0, 5, make_knot(8, 4, 0, 8)) == GAR_HIP_OK);
      }
      const std::vector<double> before = solve(s);
      const int32_t bad[2][5] = {{-1, 4, 0, 8, 0}, {400, 100, 0, 400, 0}}; // invalid; a knot no kernel's LDS plan holds
      for (const auto &d : bad) {
        CHECK(gar_hip_cycle_append(s, d) != GAR_HIP_OK);
        CHECK(solve(s) == before);
      }
      gar_hip_solver_destroy(s);
    }
  }
  { // (56, 24) with constraints has no any-dimension kernels (a CU's LDS); with the fold switch off, no solver at all
    CHECK(gar_hip_set_option("GAR_HIP_SERIAL_FOLD", "0") == GAR_HIP_OK);
    Problem p = make_problem(56, 24, 0, 2, 8);
    const std::vector<int32_t> dims = p.dims5();
    CHECK(gar_hip_solver_create(0, 2, dims.data(), p.nc0(), 1, 1) == nullptr);
    CHECK(gar_hip_set_option("GAR_HIP_SERIAL_FOLD", nullptr) == GAR_HIP_OK);
  }
}

// 9: every service on a resident batch (KKT residuals, re-solve, refinement, adjoint with gradients, many affine terms, the
// device-resident caller's two calls) with its work area live at a ring cycle_append, at a rebuilding one and at destroy.
// (Unconstrained: scenario 1's terminal constraints make these services refuse.)
void resident_calls(gar_hip_solver *s, int batch) {
  const size_t n = (size_t)gar_hip_affine_doubles(s) * (size_t)batch, np = (size_t)gar_hip_problem_doubles(s) * (size_t)batch;
  std::vector<double> vec(n), adj(n), grad(np), rhs(17 * n), out(17 * n), packed(np);
  for (std::vector<double> *v : {&vec, &rhs})
    for (double &x : *v)
      x = rnd();
  double kkt[6];
  CHECK(gar_hip_kkt_error(s, kMu, nullptr, kkt, nullptr) == GAR_HIP_OK);
  CHECK(gar_hip_upload_affine(s, 0, batch, vec.data()) == GAR_HIP_OK);
  CHECK(gar_hip_backward_affine(s) == GAR_HIP_OK);
  CHECK(gar_hip_forward(s, nullptr) == GAR_HIP_OK);
  int32_t steps[2];
  CHECK(gar_hip_refine(s, 1, -1.0, steps) == GAR_HIP_OK);
  CHECK(gar_hip_adjoint(s, vec.data(), adj.data(), grad.data()) == GAR_HIP_OK);
  CHECK(gar_hip_affine_solve_multi(s, 17, rhs.data(), out.data()) == GAR_HIP_OK);
  // (on the emulator device memory is host memory)
  CHECK(gar_hip_solution_vectors_device(s, 0, batch, adj.data()) == GAR_HIP_OK);
  CHECK(gar_hip_download_packed(s, 0, batch, packed.data()) == GAR_HIP_OK);
  CHECK(gar_hip_upload_packed_user_device(s, 0, batch, packed.data()) == GAR_HIP_OK);
  CHECK(gar_hip_sync(s) == GAR_HIP_OK);
}
void resident_services() {
  const int batch = 2;
  Problem p = make_problem(8, 4, 0, 3);
  const std::vector<int32_t> dims = p.dims5();
  gar_hip_solver *s = gar_hip_solver_create(0, 3, dims.data(), p.nc0(), batch, 1);
  CHECK(s != nullptr);
  if (!s)
    return;
  upload(s, p, batch);
  solve(s);
  resident_calls(s, batch);
  CHECK(gar_hip_cycle_append(s, p.knots[0].d) == GAR_HIP_OK); // same dimensions: the ring, every work area stays
  solve(s);
  resident_calls(s, batch);
  const Knot other = make_knot(8, 5, 0, 8);
  CHECK(gar_hip_cycle_append(s, other.d) == GAR_HIP_OK); // other dimensions: rebuilt, every work area live
  p.knots.erase(p.knots.begin());
  p.knots.insert(p.knots.end() - 1, other);
  upload(s, p, batch);
  solve(s);
  resident_calls(s, batch);
  gar_hip_solver_destroy(s);
}

struct Scenario {
  const char *name;
  void (*run)();
  long long allocs; // gar_hip_debug_alloc_count's change, recorded on the parent commit
};
const Scenario kExpected[] = {
    {"1 serial, every lazy member live, batch 2", [] { serial_all_lazy(2, false); }, 16},
    {"1 serial, every lazy member live, batch 1", [] { serial_all_lazy(1, false); }, 17},
    {"2 ring and rebuilding cycle_append, batch 2", [] { serial_all_lazy(2, true); }, 27},
    {"2 ring and rebuilding cycle_append, batch 1", [] { serial_all_lazy(1, true); }, 28},
    {"3 set_pipeline 2, 2, 0, 2", pipeline_again, 8},
    {"4 leg mode: plain, constrained, ranked pair", leg_modes, 56},
    {"5 dense", dense, 11},
    {"6 serial fold, ring cycle_append", serial_fold, 14},
    {"7 two devices behind one handle", multi_device, 62},
    {"8 refusals", refusals, 11},
    {"9 resident services live, ring and rebuilding cycle_append, batch 2", resident_services, 64},
};

} // namespace

int main() {
  for (const Scenario &sc : kExpected) {
    const long long a0 = gar_hip_debug_alloc_count();
    sc.run();
    const long long n = gar_hip_debug_alloc_count() - a0;
    std::printf("scenario %-68s allocations %lld (expected %lld)\n", sc.name, n, sc.allocs);
    if (n != sc.allocs) {
      std::printf("  allocation count differs\n");
      ++g_failures;
    }
  }
  std::printf("%s\n", g_failures ? "FAILED" : "lifetime ok");
  return g_failures ? 1 : 0;
}
