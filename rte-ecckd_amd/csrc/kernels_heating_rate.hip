// kernels_heating_rate.hip -- heating rates: the divergence of the net flux across each layer to the temperature tendency
// in K s-1 -- what a host model calls after the flux calls, once per flux set (longwave / shortwave, clear / all sky) or
// once for all of them stacked as outer planes, and per band after the by-band calls.
//
// Restates RTE-RRTMGP's compute_heating_rate [RTE-ext: extensions/mo_heating_rates.F90; the library is not part of the
// reference tree].  The definition is spelt operation by operation in include/ecckd_hip.h (ecckd_heating_rate); every
// expression here keeps that order, the build has FMA contraction off and the quotient is the language's division
// (correctly rounded in both precisions; no reciprocal), so the results are those of an IEEE evaluation of the formulas
// in the precision of the call.
//
// Mapping (gfx950): a streaming kernel judged by bytes moved over time,
//   sizeof(real) * ncol * ((2*nouter + 1)*(nlay+1) + (nouter + [cp])*nlay).
// Lanes run along columns, so every load and store of a wave is one coalesced line.  One lane owns a (column, outer plane)
// pair and walks the column's layers with the previous level's flux_up, flux_dn and pressure in registers: each flux
// level is loaded once (nontemporal: a read-once stream).  The pressures (and cp) are loaded once per plane; work items
// are numbered with the plane fastest, so the blocks that share a column block's pressures are dispatched together and
// all but the first read them from the caches, not from HBM.  The layer loop is unrolled by four: the loads of four
// levels are independent of the arithmetic and go out together, which is what keeps enough bytes in flight when
// ncol*nouter gives only a wave or two per SIMD.  256 threads per block; the grid is what is resident at a time (8 blocks
// per CU), the rest of the work by grid stride.  All offsets are 64-bit: ncol*(nlay+1)*nouter passes 2^31 at 1e6 columns
// x 138 levels x 16 planes.  No LDS, no atomics.
#include "kernels.hpp"

namespace ecckd {
namespace {

constexpr int kHrBlock = 256;
constexpr int kHrBlocksPerCu = 8;   // 32 waves per CU
constexpr int kHrUnroll = 4;        // levels in flight per lane

template <typename real, bool CP>
__global__ void __launch_bounds__(kHrBlock) heating_rate_kernel(const HeatingRateArgs a) {
  const real *__restrict__ flux_up = reinterpret_cast<const real *>(a.flux_up);
  const real *__restrict__ flux_dn = reinterpret_cast<const real *>(a.flux_dn);
  const real *__restrict__ plev = reinterpret_cast<const real *>(a.plev);
  [[maybe_unused]] const real *__restrict__ cp = reinterpret_cast<const real *>(a.cp);
  real *__restrict__ heating_rate = reinterpret_cast<real *>(a.heating_rate);
  const real grav = (real)a.grav;
  [[maybe_unused]] const real cp_dry = (real)a.cp_dry;
  const size_t ncol = (size_t)a.ncol, nouter = (size_t)a.nouter;
  const size_t lev_plane = ncol * (size_t)(a.nlay + 1), lay_plane = ncol * (size_t)a.nlay;
  const size_t nwork = ((ncol + kHrBlock - 1) / kHrBlock) * nouter;   // (column block, plane), the plane fastest

  for (size_t w = blockIdx.x; w < nwork; w += gridDim.x) {
    const size_t plane = w % nouter, col = (w / nouter) * kHrBlock + threadIdx.x;
    if (col >= ncol) continue;   // (the ragged last column block; nothing below synchronises)
    const real *fu = flux_up + plane * lev_plane + col, *fd = flux_dn + plane * lev_plane + col, *p = plev + col;
    real *hr = heating_rate + plane * lay_plane + col;
    real u0 = __builtin_nontemporal_load(fu), d0 = __builtin_nontemporal_load(fd), p0 = *p;
#pragma unroll kHrUnroll
    for (int l = 0; l < a.nlay; ++l) {
      const size_t q0 = (size_t)l * ncol, q1 = q0 + ncol;
      const real u1 = __builtin_nontemporal_load(fu + q1), d1 = __builtin_nontemporal_load(fd + q1), p1 = p[q1];
      real c = cp_dry;
      if constexpr (CP) c = cp[q0 + col];
      const real du = u1 - u0;
      const real dd = d1 - d0;
      const real dnet = du - dd;
      const real dp = p1 - p0;
      hr[q0] = (dnet * grav) / (c * dp);
      u0 = u1; d0 = d1; p0 = p1;
    }
  }
}

}  // namespace

unsigned heating_rate_grid(int ncol, int nouter, int cus) {
  const size_t want = (((size_t)ncol + kHrBlock - 1) / kHrBlock) * (size_t)nouter;
  const size_t resident = (size_t)(cus > 0 ? cus : 256) * kHrBlocksPerCu;
  return (unsigned)(want > resident ? resident : want);
}

hipError_t launch_heating_rate(const HeatingRateArgs &a, hipStream_t s) {
  if (a.ncol < 1 || a.nlay < 1 || a.nouter < 1) return hipErrorInvalidValue;
  typedef void (*K)(const HeatingRateArgs);
  const K k = a.f32 ? (a.cp ? heating_rate_kernel<float, true> : heating_rate_kernel<float, false>)
                    : (a.cp ? heating_rate_kernel<double, true> : heating_rate_kernel<double, false>);
  hipLaunchKernelGGL(k, dim3(heating_rate_grid(a.ncol, a.nouter, a.cus)), dim3(kHrBlock), 0, s, a);
  return hipGetLastError();
}

}  // namespace ecckd
