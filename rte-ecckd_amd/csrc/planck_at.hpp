// planck_at.hpp -- the Planck source of one temperature for one g-point, shared by the longwave kernels that recompute
// sources from temperatures (kernels_rte_lw_split.hip, kernels_rte_lw_jac.hip) so that they produce the same bits.
#pragma once
#include <hip/hip_runtime.h>

namespace ecckd {
namespace {

// Planck source of one temperature for one g-point (calculate_planck_function, :275-288), table rows from
// global memory (59 KB: L1/L2 resident).  tp0 = temperature_planck(1), rdt = 1/(temperature_planck(2)-(1)).
struct PlanckTab { const double *tab; double t0, dt, rdt; int ntp, ng; };
// `tab` / `stride`: the table the rows are read from -- the model's (ng,ntp) table in global memory (stride ng), or the
// block's copy in LDS whose rows are padded to an odd number of doubles: the 32 columns of a wave sit in different
// (neighbouring) rows, and with a stride of 32 doubles they would all hit the same two banks.
__device__ __forceinline__ double planck_at(const PlanckTab &P, const double *tab, int stride, double T, int g, double pi, double rpi) {
  double ti = (T - P.t0) * P.rdt;
  {   // exact quotient (Markstein) so that the row and the weights are the reference's
    const double rem = fma(-ti, P.dt, T - P.t0);
    ti = fma(rem, P.rdt, ti);
  }
  double v;
  if (ti >= 0.) {
    ti = 1. + ti;
    const int it0 = ti >= (double)(P.ntp - 1) ? P.ntp - 1 : (int)ti;
    const double w1 = ti - it0, w0 = 1. - w1;
    const double *r = tab + (it0 - 1) * stride + g;
    v = w0 * r[0] + w1 * r[stride];
  } else {
    v = (T / P.t0) * tab[g];
  }
  const double q = v * rpi;   // correctly rounded v / pi
  return fma(fma(-q, pi, v), rpi, q);
}

}  // namespace
}  // namespace ecckd
