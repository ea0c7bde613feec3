// Which mapping should ecckd_heating_rate's kernel have?  Two that read each flux level from HBM once, with the same
// arithmetic (include/ecckd_hip.h, "Heating rates"), lanes along columns, 256 threads, 64-bit offsets, fp64, no cp:
//   walk   one lane per (column, plane) walks the layers with the previous level's three values in registers, four levels
//          in flight (the form of rte-ecckd_amd/csrc/kernels_heating_rate.hip)
//   tile   one lane per cell: it loads both edges of its layer itself, so every level is asked for twice and the second
//          request is left to the caches; work runs column fastest, then layer, then plane, by grid stride
// Prints the median and min-max of `reps` interleaved launches of each, and whether the results are the same bits.
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off tools/ubench_heating_rate.hip -o build_tmp/ubench_heating_rate
// Run:   build_tmp/ubench_heating_rate ncol nlay nouter [reps]
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define CHECK(x)                                                                     \
  do {                                                                               \
    hipError_t e_ = (x);                                                             \
    if (e_ != hipSuccess) {                                                          \
      std::fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_));                   \
      return 1;                                                                      \
    }                                                                                \
  } while (0)

constexpr int kBlock = 256;
constexpr double kGrav = 9.80665, kCpDry = 1004.64;

__global__ void __launch_bounds__(kBlock) walk(const double *__restrict__ flux_up, const double *__restrict__ flux_dn,
                                               const double *__restrict__ plev, double *__restrict__ hr, int ncol_, int nlay,
                                               int nouter_) {
  const size_t ncol = ncol_, nouter = nouter_, lev_plane = ncol * (size_t)(nlay + 1), lay_plane = ncol * (size_t)nlay;
  const size_t nwork = ((ncol + kBlock - 1) / kBlock) * nouter;
  for (size_t w = blockIdx.x; w < nwork; w += gridDim.x) {
    const size_t plane = w % nouter, col = (w / nouter) * kBlock + threadIdx.x;
    if (col >= ncol) continue;
    const double *fu = flux_up + plane * lev_plane + col, *fd = flux_dn + plane * lev_plane + col, *p = plev + col;
    double *out = hr + plane * lay_plane + col;
    double u0 = __builtin_nontemporal_load(fu), d0 = __builtin_nontemporal_load(fd), p0 = *p;
#pragma unroll 4
    for (int l = 0; l < nlay; ++l) {
      const size_t q0 = (size_t)l * ncol, q1 = q0 + ncol;
      const double u1 = __builtin_nontemporal_load(fu + q1), d1 = __builtin_nontemporal_load(fd + q1), p1 = p[q1];
      const double du = u1 - u0, dd = d1 - d0;
      const double dnet = du - dd, dp = p1 - p0;
      out[q0] = (dnet * kGrav) / (kCpDry * dp);
      u0 = u1; d0 = d1; p0 = p1;
    }
  }
}

__global__ void __launch_bounds__(kBlock) tile(const double *__restrict__ flux_up, const double *__restrict__ flux_dn,
                                               const double *__restrict__ plev, double *__restrict__ hr, int ncol_, int nlay,
                                               int nouter_) {
  const size_t ncol = ncol_, ncb = (ncol + kBlock - 1) / kBlock, lev_plane = ncol * (size_t)(nlay + 1), lay_plane = ncol * (size_t)nlay;
  const size_t nwork = ncb * (size_t)nlay * (size_t)nouter_;
  for (size_t w = blockIdx.x; w < nwork; w += gridDim.x) {
    const size_t col = (w % ncb) * kBlock + threadIdx.x, l = (w / ncb) % (size_t)nlay, plane = w / (ncb * (size_t)nlay);
    if (col >= ncol) continue;
    const size_t q = plane * lev_plane + l * ncol + col, qp = l * ncol + col;
    const double du = flux_up[q + ncol] - flux_up[q], dd = flux_dn[q + ncol] - flux_dn[q];
    const double dnet = du - dd, dp = plev[qp + ncol] - plev[qp];
    hr[plane * lay_plane + qp] = (dnet * kGrav) / (kCpDry * dp);
  }
}

int main(int argc, char **argv) {
  if (argc < 4) {
    std::fprintf(stderr, "usage: ubench_heating_rate ncol nlay nouter [reps]\n");
    return 1;
  }
  const int ncol = std::atoi(argv[1]), nlay = std::atoi(argv[2]), nouter = std::atoi(argv[3]), reps = argc > 4 ? std::atoi(argv[4]) : 20;
  if (ncol < 1 || nlay < 1 || nouter < 1 || reps < 1) return 1;
  const size_t lev = (size_t)ncol * (nlay + 1), lay = (size_t)ncol * nlay;
  std::vector<double> h(lev * nouter), hp(lev);
  unsigned long long s = 88172645463325252ull;
  auto rnd = [&] { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return (double)(s >> 11) * 0x1p-53; };
  double *fu, *fd, *p, *o1, *o2;
  CHECK(hipMalloc(&fu, lev * nouter * 8)); CHECK(hipMalloc(&fd, lev * nouter * 8)); CHECK(hipMalloc(&p, lev * 8));
  CHECK(hipMalloc(&o1, lay * nouter * 8)); CHECK(hipMalloc(&o2, lay * nouter * 8));
  for (auto &v : h) v = 500. * rnd();
  CHECK(hipMemcpy(fu, h.data(), h.size() * 8, hipMemcpyHostToDevice));
  for (auto &v : h) v = 500. * rnd();
  CHECK(hipMemcpy(fd, h.data(), h.size() * 8, hipMemcpyHostToDevice));
  for (int c = 0; c < ncol; ++c) {
    double v = 10.;
    for (int l = 0; l <= nlay; ++l) { hp[(size_t)l * ncol + c] = v; v += 1. + 4999. * rnd(); }
  }
  CHECK(hipMemcpy(p, hp.data(), hp.size() * 8, hipMemcpyHostToDevice));
  const size_t ncb = ((size_t)ncol + kBlock - 1) / kBlock, resident = 256 * 8;
  const unsigned gw = (unsigned)std::min(ncb * nouter, resident), gt = (unsigned)std::min(ncb * nlay * nouter, resident);
  hipEvent_t e0, e1;
  CHECK(hipEventCreate(&e0)); CHECK(hipEventCreate(&e1));
  std::vector<float> tw, tt;
  for (int r = -3; r < reps; ++r) {   // three warm-up rounds
    float ms;
    CHECK(hipEventRecord(e0, 0));
    hipLaunchKernelGGL(walk, dim3(gw), dim3(kBlock), 0, 0, fu, fd, p, o1, ncol, nlay, nouter);
    CHECK(hipEventRecord(e1, 0)); CHECK(hipEventSynchronize(e1)); CHECK(hipEventElapsedTime(&ms, e0, e1));
    if (r >= 0) tw.push_back(ms);
    CHECK(hipEventRecord(e0, 0));
    hipLaunchKernelGGL(tile, dim3(gt), dim3(kBlock), 0, 0, fu, fd, p, o2, ncol, nlay, nouter);
    CHECK(hipEventRecord(e1, 0)); CHECK(hipEventSynchronize(e1)); CHECK(hipEventElapsedTime(&ms, e0, e1));
    if (r >= 0) tt.push_back(ms);
  }
  CHECK(hipGetLastError());
  std::vector<double> r1(lay * nouter), r2(lay * nouter);
  CHECK(hipMemcpy(r1.data(), o1, r1.size() * 8, hipMemcpyDeviceToHost));
  CHECK(hipMemcpy(r2.data(), o2, r2.size() * 8, hipMemcpyDeviceToHost));
  const bool same = std::memcmp(r1.data(), r2.data(), r1.size() * 8) == 0;
  std::sort(tw.begin(), tw.end()); std::sort(tt.begin(), tt.end());
  const double bytes = 8. * ncol * ((2. * nouter + 1) * (nlay + 1) + (double)nouter * nlay);
  std::printf("{\"ncol\": %d, \"nlay\": %d, \"nouter\": %d, \"bytes\": %.0f, \"walk_ms\": [%.4f, %.4f, %.4f], \"tile_ms\": [%.4f, %.4f, %.4f], "
              "\"walk_TB_per_s\": %.3f, \"tile_TB_per_s\": %.3f, \"same_bits\": %s}\n",
              ncol, nlay, nouter, bytes, tw[tw.size() / 2], tw.front(), tw.back(), tt[tt.size() / 2], tt.front(), tt.back(),
              bytes / (tw[tw.size() / 2] * 1e-3) / 1e12, bytes / (tt[tt.size() / 2] * 1e-3) / 1e12, same ? "true" : "false");
  return same ? 0 : 2;
}
