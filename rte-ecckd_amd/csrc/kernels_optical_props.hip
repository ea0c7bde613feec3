// kernels_optical_props.hip -- element-wise operations on optical properties: what an all-sky host calls between
// gas_optics and rte_sw / rte_lw to add cloud and aerosol optics (given on the model's bands) to the gas optics.
//
// Restates RTE-RRTMGP's optical-props kernels of the v1.5 era [RTE-ext: mo_optical_props_kernels.F90; the library is not
// part of the reference tree -- reference Makefile:19,33 links it]: delta_scale_2str_k / delta_scale_2str_f_k and
// increment_1scalar_by_1scalar, increment_1scalar_by_2stream, increment_2stream_by_1scalar, increment_2stream_by_2stream
// with their inc_*_bybnd forms.  Every expression keeps the order spelt there (the build has FMA contraction off), so the
// fp64 results are those of an IEEE evaluation of the formulas.
//
// Mapping (gfx950): pure streaming kernels.  Increment: one thread per (column, layer), the column fastest, so every
// load and store of a wave is one full coalesced line; the thread walks the bands and, inside a band, its g-points with
// the band's op2 values in registers (read once per band, not once per g-point); grid-stride loop; no LDS.  The work per
// byte is a handful of flops: the kernels are judged by bytes moved over time against the HBM ceiling.
#include <type_traits>

#include "kernels.hpp"

namespace ecckd {
namespace {

// max(eps, x) as the Fortran intrinsic on finite arguments; a NaN gives eps (the numerators carry the NaN on)
template <typename real> __device__ __forceinline__ real floor_eps(real x) { return x > op_eps<real>() ? x : op_eps<real>(); }

constexpr int kOpBlock = 256;
constexpr int kOpMaxBlocks = 8192;   // 32 blocks of 256 threads per CU (a full CU of waves four times over; not tuned)

// OP1_2STR / OP2_2STR: which side carries ssa and g.  BYBAND: op2 lives on bands (OptPropsArgs::band_first).
// MASKED (increment_masked_kernel; ecckd_increment_masked): where bit g of the cell's word a.mask(column, layer) is clear
// the g-point is incremented as if tau2 were +0 there -- the same operations on a zero optical depth (what RTE-RRTMGP's
// draw_samples followed by increment computes), so ssa2 / g2 are still read and multiplied.
// SCALED (increment_scaled_kernel; ecckd_increment_scaled): the g-point is incremented by t2 = tau2 * scaling(column,
// layer, g) -- float32 whatever `real` is --, and increment's products t2 * (1 - ssa2), t2 * ssa2 and that times g2 are
// formed per g-point from t2, not once per band; any number of g-points.
// The kernels (increment_kernel, increment_masked_kernel, increment_scaled_kernel, below) are thin entries to this body.
template <typename real, bool OP1_2STR, bool OP2_2STR, bool BYBAND, bool MASKED, bool SCALED = false>
__device__ __forceinline__ void increment_body(const OptPropsArgs &a) {
  static_assert(!(MASKED && SCALED), "a scaling of 0 is the clear bit: one or the other");
  const size_t n2 = (size_t)a.ncol * a.nlay;
  real *tau1 = reinterpret_cast<real *>(a.tau1), *ssa1 = reinterpret_cast<real *>(a.ssa1), *g1 = reinterpret_cast<real *>(a.g1);
  const real *tau2 = reinterpret_cast<const real *>(a.tau2), *ssa2 = reinterpret_cast<const real *>(a.ssa2),
             *g2 = reinterpret_cast<const real *>(a.g2);
  const int nouter = BYBAND ? a.nband : a.ng;
  for (size_t cell = (size_t)blockIdx.x * kOpBlock + threadIdx.x; cell < n2; cell += (size_t)gridDim.x * kOpBlock) {
    [[maybe_unused]] unsigned long long word = 0ull;
    if constexpr (MASKED) word = a.mask[cell];
    for (int b = 0; b < nouter; ++b) {
      const size_t q2 = cell + n2 * b;
      const real t2_in = tau2[q2];
      real s2 = real(0), gg2 = real(0);
      if constexpr (OP2_2STR) { s2 = ssa2[q2]; if constexpr (OP1_2STR) gg2 = g2[q2]; }
      // what the band contributes to every one of its g-points
      const real tabs2_in = OP2_2STR ? t2_in * (real(1) - s2) : t2_in;   // 1scl += 2str: absorption optical depth
      const real tscat2_in = t2_in * s2;
      const real tsg2_in = tscat2_in * gg2;
      // MASKED: ... and to the g-points that do not see it: the same products of a zero optical depth
      [[maybe_unused]] const real tabs2_0 = OP2_2STR ? real(0) * (real(1) - s2) : real(0);
      [[maybe_unused]] const real tscat2_0 = real(0) * s2;
      [[maybe_unused]] const real tsg2_0 = tscat2_0 * gg2;
      const int glo = BYBAND ? a.band_first[b] : b, ghi = BYBAND ? a.band_first[b + 1] : b + 1;
      for (int g = glo; g < ghi; ++g) {
        const size_t q = cell + n2 * g;
        const bool seen = MASKED ? ((word >> g) & 1ull) != 0ull : true;
        real t2 = seen ? t2_in : real(0), tabs2 = seen ? tabs2_in : tabs2_0;
        real tscat2 = seen ? tscat2_in : tscat2_0, tsg2 = seen ? tsg2_in : tsg2_0;
        if constexpr (SCALED) {
          t2 = t2_in * (real)a.scaling[q];
          tabs2 = OP2_2STR ? t2 * (real(1) - s2) : t2;
          tscat2 = t2 * s2;
          tsg2 = tscat2 * gg2;
        }
        if constexpr (!OP1_2STR) {
          tau1[q] = tau1[q] + tabs2;
        } else if constexpr (!OP2_2STR) {
          const real t1 = tau1[q];
          const real tau12 = t1 + t2;
          ssa1[q] = t1 * ssa1[q] / floor_eps(tau12);
          tau1[q] = tau12;
        } else {
          const real t1 = tau1[q], s1 = ssa1[q];
          const real tau12 = t1 + t2;
          const real tscat1 = t1 * s1;
          const real tauscat12 = tscat1 + tscat2;
          g1[q] = (tscat1 * g1[q] + tsg2) / floor_eps(tauscat12);
          ssa1[q] = tauscat12 / floor_eps(tau12);
          tau1[q] = tau12;
        }
      }
    }
  }
}

template <typename real, bool OP1_2STR, bool OP2_2STR, bool BYBAND>
__global__ void __launch_bounds__(kOpBlock) increment_kernel(const OptPropsArgs a) {
  increment_body<real, OP1_2STR, OP2_2STR, BYBAND, false>(a);
}
template <typename real, bool OP1_2STR, bool OP2_2STR, bool BYBAND>
__global__ void __launch_bounds__(kOpBlock) increment_masked_kernel(const OptPropsArgs a) {
  increment_body<real, OP1_2STR, OP2_2STR, BYBAND, true>(a);
}

template <typename real, bool OP1_2STR, bool OP2_2STR, bool BYBAND>
__global__ void __launch_bounds__(kOpBlock) increment_scaled_kernel(const OptPropsArgs a) {
  increment_body<real, OP1_2STR, OP2_2STR, BYBAND, false, true>(a);
}

template <typename real, bool FORWARD>
__global__ void __launch_bounds__(kOpBlock) delta_scale_kernel(size_t n, const real *tau, const real *ssa, const real *g, const real *forward,
                                                               real *tau_out, real *ssa_out, real *g_out) {
  for (size_t q = (size_t)blockIdx.x * kOpBlock + threadIdx.x; q < n; q += (size_t)gridDim.x * kOpBlock) {
    const real t = tau[q], w = ssa[q], gq = g[q];
    const real f = FORWARD ? forward[q] : gq * gq;
    const real wf = w * f;
    tau_out[q] = t * (real(1) - wf);
    ssa_out[q] = (w - wf) / floor_eps(real(1) - wf);
    g_out[q] = (gq - f) / floor_eps(real(1) - f);
  }
}

unsigned op_blocks(size_t n) {
  size_t b = (n + kOpBlock - 1) / kOpBlock;
  return (unsigned)(b > (size_t)kOpMaxBlocks ? (size_t)kOpMaxBlocks : b);
}

template <typename real>
hipError_t launch_increment_t(const OptPropsArgs &a, hipStream_t s) {
  typedef void (*K)(const OptPropsArgs);
  const bool one = a.ssa1 != nullptr, two = a.ssa2 != nullptr, bb = a.nband > 0;
  K k;
  if (!one && !two) k = bb ? increment_kernel<real, false, false, true> : increment_kernel<real, false, false, false>;
  else if (!one) k = bb ? increment_kernel<real, false, true, true> : increment_kernel<real, false, true, false>;
  else if (!two) k = bb ? increment_kernel<real, true, false, true> : increment_kernel<real, true, false, false>;
  else k = bb ? increment_kernel<real, true, true, true> : increment_kernel<real, true, true, false>;
  if (a.mask) {
    if (!one && !two) k = bb ? increment_masked_kernel<real, false, false, true> : increment_masked_kernel<real, false, false, false>;
    else if (!one) k = bb ? increment_masked_kernel<real, false, true, true> : increment_masked_kernel<real, false, true, false>;
    else if (!two) k = bb ? increment_masked_kernel<real, true, false, true> : increment_masked_kernel<real, true, false, false>;
    else k = bb ? increment_masked_kernel<real, true, true, true> : increment_masked_kernel<real, true, true, false>;
  }
  if (a.scaling) {
    if (!one && !two) k = bb ? increment_scaled_kernel<real, false, false, true> : increment_scaled_kernel<real, false, false, false>;
    else if (!one) k = bb ? increment_scaled_kernel<real, false, true, true> : increment_scaled_kernel<real, false, true, false>;
    else if (!two) k = bb ? increment_scaled_kernel<real, true, false, true> : increment_scaled_kernel<real, true, false, false>;
    else k = bb ? increment_scaled_kernel<real, true, true, true> : increment_scaled_kernel<real, true, true, false>;
  }
  hipLaunchKernelGGL(k, dim3(op_blocks((size_t)a.ncol * a.nlay)), dim3(kOpBlock), 0, s, a);
  return hipGetLastError();
}

template <typename real>
hipError_t launch_delta_scale_t(size_t n, const double *tau, const double *ssa, const double *g, const double *forward, double *tau_out,
                                double *ssa_out, double *g_out, hipStream_t s) {
  auto P = [](const double *p) { return reinterpret_cast<const real *>(p); };
  auto Q = [](double *p) { return reinterpret_cast<real *>(p); };
  if (forward)
    hipLaunchKernelGGL((delta_scale_kernel<real, true>), dim3(op_blocks(n)), dim3(kOpBlock), 0, s, n, P(tau), P(ssa), P(g), P(forward),
                       Q(tau_out), Q(ssa_out), Q(g_out));
  else
    hipLaunchKernelGGL((delta_scale_kernel<real, false>), dim3(op_blocks(n)), dim3(kOpBlock), 0, s, n, P(tau), P(ssa), P(g), P(forward),
                       Q(tau_out), Q(ssa_out), Q(g_out));
  return hipGetLastError();
}

}  // namespace

hipError_t launch_increment(const OptPropsArgs &a, hipStream_t s) {
  if (a.ncol <= 0 || a.nlay <= 0 || a.ng <= 0) return hipSuccess;
  if (a.mask && (a.ng > 64 || a.scaling)) return hipErrorInvalidValue;
  return a.f32 ? launch_increment_t<float>(a, s) : launch_increment_t<double>(a, s);
}

hipError_t launch_delta_scale(size_t n, const double *tau, const double *ssa, const double *g, const double *forward, double *tau_out,
                              double *ssa_out, double *g_out, int f32, hipStream_t s) {
  if (n == 0) return hipSuccess;
  return f32 ? launch_delta_scale_t<float>(n, tau, ssa, g, forward, tau_out, ssa_out, g_out, s)
             : launch_delta_scale_t<double>(n, tau, ssa, g, forward, tau_out, ssa_out, g_out, s);
}

}  // namespace ecckd
