// Which store form does gar_adjoint_gradients (csrc/gar_adjoint.hpp) leave its LDS image with?  The kernel's own body
// (adjoint_gradients_block<FORM>) instantiated for the three forms it can take -- plain 8-byte stores, 16-byte stores from
// the even offsets of the record, 16-byte non-temporal stores -- on synthetic solution and adjoint records at the headline
// geometry: (36, 12), N = 256, batch 4 096, the caller's packed layout (29.5 KB per knot, 31 GB per launch).  Best of 5
// after a warm-up launch, the three forms alternating.  DESIGN.md 5.3e quotes the table.
// Build: hipcc -O3 -std=c++17 --offload-arch=gfx950 -I../../aligator_amd/csrc grad_store_forms.cpp -o grad_store_forms
//        ./grad_store_forms [batch [horizon]]
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "gar_generic.hpp"
#include "gar_adjoint.hpp"

template <int FORM> __global__ void __launch_bounds__(GAR_ADJ_THREADS) grad_form(gar::AdjointParams P) {
  gar::adjoint_gradients_block<FORM>(P);
}
__global__ void fill(double *p, long long n, double scale) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
    p[i] = scale * (double)((i * 2654435761ll) % 1999 - 999) / 999.0;
}
#define CHECK(x)                                                                                                         \
  do {                                                                                                                   \
    hipError_t e_ = (x);                                                                                                 \
    if (e_ != hipSuccess) {                                                                                              \
      std::printf("%s: %s\n", #x, hipGetErrorString(e_));                                                                \
      return 1;                                                                                                          \
    }                                                                                                                    \
  } while (0)

int main(int argc, char **argv) {
  const int batch = argc > 1 ? std::atoi(argv[1]) : 4096, N = argc > 2 ? std::atoi(argv[2]) : 256;
  const int nx = 36, nu = 12, nc0 = nx;
  // the layouts build_layout (gar_hip.cpp) gives these dimensions: G0 | g0 | knots, records on even offsets; xs | us | lbdas
  std::vector<gar_stage_meta> meta((size_t)N + 1);
  long long in = ((long long)nc0 * nx + nc0 + 1) & ~1ll;
  int x = 0, u = 0, l = nc0;
  for (int t = 0; t <= N; ++t) {
    gar_stage_meta &m = meta[(size_t)t];
    m = gar_stage_meta{};
    m.nx = nx, m.nu = t < N ? nu : 0, m.nx2 = nx;
    m.in_off = in;
    in += (gar_knot_doubles(m.nx, m.nu, 0, m.nx2, 0) + 1) & ~1ll;
    m.x_off = x, x += m.nx;
    m.u_off = u, u += m.nu;
    m.l_off = t == 0 ? 0 : l;
    if (t > 0)
      l += nx;
  }
  const long long sol_doubles = (x + u + l + 1) & ~1ll;
  for (gar_stage_meta &m : meta)
    m.u_off += x, m.l_off += x + u;
  gar_stage_meta *d_meta;
  double *sol, *adj, *grad;
  int *status;
  CHECK(hipMalloc((void **)&d_meta, sizeof(gar_stage_meta) * meta.size()));
  CHECK(hipMemcpy(d_meta, meta.data(), sizeof(gar_stage_meta) * meta.size(), hipMemcpyHostToDevice));
  CHECK(hipMalloc((void **)&sol, sizeof(double) * sol_doubles * batch));
  CHECK(hipMalloc((void **)&adj, sizeof(double) * sol_doubles * batch));
  CHECK(hipMalloc((void **)&grad, sizeof(double) * in * batch));
  CHECK(hipMalloc((void **)&status, sizeof(int) * batch));
  CHECK(hipMemset(status, 0, sizeof(int) * batch));
  hipLaunchKernelGGL(fill, dim3(4096), dim3(256), 0, 0, sol, sol_doubles * batch, 1.0);
  hipLaunchKernelGGL(fill, dim3(4096), dim3(256), 0, 0, adj, sol_doubles * batch, 0.5);
  gar::AdjointParams P{};
  P.meta = d_meta;
  P.U.stride = in, P.U.G0_off = 0, P.U.g0_off = (long long)nc0 * nx, P.U.nc0 = nc0;
  P.status = status;
  P.sol = sol, P.adj = adj, P.grad = grad, P.sol_stride = sol_doubles;
  P.horizon = N, P.nc0 = nc0, P.nx0 = nx;
  const size_t lds = sizeof(double) * (size_t)gar::adjoint_grad_lds_doubles(nx, nu, nx, nc0, nx);
  const dim3 grid((unsigned)batch * (unsigned)(N + 1)), block(GAR_ADJ_THREADS);
  hipEvent_t e0, e1;
  CHECK(hipEventCreate(&e0));
  CHECK(hipEventCreate(&e1));
  float best[3] = {1e30f, 1e30f, 1e30f};
  for (int r = 0; r < 6; ++r)
    for (int form = 0; form < 3; ++form) {
      CHECK(hipEventRecord(e0, 0));
      if (form == 0)
        hipLaunchKernelGGL(grad_form<gar::kAdjStore8>, grid, block, lds, 0, P);
      else if (form == 1)
        hipLaunchKernelGGL(grad_form<gar::kAdjStore16>, grid, block, lds, 0, P);
      else
        hipLaunchKernelGGL(grad_form<gar::kAdjStore16Nt>, grid, block, lds, 0, P);
      CHECK(hipEventRecord(e1, 0));
      CHECK(hipEventSynchronize(e1));
      CHECK(hipGetLastError());
      float ms;
      CHECK(hipEventElapsedTime(&ms, e0, e1));
      if (r > 0 && ms < best[form])
        best[form] = ms;
    }
  const double gb = 8.0 * (double)in * batch / 1e9;
  const char *name[3] = {"8-byte stores", "16-byte stores", "16-byte non-temporal stores"};
  for (int form = 0; form < 3; ++form)
    std::printf("%-28s %8.3f ms  %6.2f TB/s written (%.1f GB, %d x %d records)\n", name[form], best[form],
                gb / best[form], gb, batch, N + 1);
  return 0;
}
