// lw_two_stream.hpp -- one cell of RTE-RRTMGP's lw_solver_2stream (lw_two_stream + lw_source_2str), shared by the
// two-stream longwave solvers (kernels_rte_lw_2str.hip, kernels_rte_gpt.hip) so that both produce the same bits per cell.
// [RTE-ext: restated from the public v1.5-era mo_rte_solver_kernels.F90; the library is not in the reference tree.
// Parity with RTE-RRTMGP is unpinned.]
#pragma once
#include <hip/hip_runtime.h>

#include "sw_two_stream.hpp"

namespace ecckd {
namespace {

constexpr double kLw2D = 1.66;                       // diffusivity factor of the two-stream longwave coefficients
constexpr double kLw2Pi = 3.14159265358979323846;    // acos(-1._wp)
constexpr double kLw2KFloor = 1.e-12;                // lower bound of (gamma1-gamma2)(gamma1+gamma2) under the square root
constexpr double kLw2TauMin = 1.e-8;                 // layers at or below this optical depth emit nothing

struct Lw2Cell { double Rdif, Tdif, src_up, src_dn; };

// Bt / Bb: the level sources above and below the layer.  FAST: rcp / sw_sqrt / sw_exp of sw_two_stream.hpp (the argument
// of sw_sqrt lies in [1e-12, D^2]); otherwise IEEE `/`, sqrt, exp in the order spelt in DESIGN.md.
template <bool FAST>
__device__ __forceinline__ Lw2Cell lw_two_stream(double tau, double ssa, double g, double Bt, double Bb) {
  const double gamma1 = kLw2D * (1. - 0.5 * ssa * (1. + g));
  const double gamma2 = kLw2D * 0.5 * ssa * (1. - g);
  const double kk0 = (gamma1 - gamma2) * (gamma1 + gamma2);
  const double k = sw_sqrt<FAST>(kk0 > kLw2KFloor ? kk0 : kLw2KFloor);
  const double e1 = sw_exp<FAST>(-tau * k), e2 = e1 * e1;
  const double RT = rcp<FAST>(k * (1. + e2) + gamma1 * (1. - e2));
  Lw2Cell c;
  c.Rdif = RT * gamma2 * (1. - e2);
  c.Tdif = RT * 2. * k * e1;
  // source linear in optical depth between the two levels (a layer the test below drops may divide by zero here: the
  // quotient is computed and discarded, nothing traps).  An INFINITE optical depth: IEEE mode gives Z = 0 and finite fluxes;
  // the fast mode's rcp<true>(inf) is NaN (its correction step forms fma(-inf, 0, 1)) and the layer emits, so the column's
  // fluxes are NaN -- confined to that column.  Unlike sw_exp, which serves any tau up to inf, the fast mode takes finite tau.
  const double den = tau * (gamma1 + gamma2);
  const double Z = FAST ? (Bb - Bt) * rcp<true>(den) : (Bb - Bt) / den;
  const double su = kLw2Pi * ((Z + Bt) - c.Rdif * (-Z + Bt) - c.Tdif * (Z + Bb));
  const double sd = kLw2Pi * ((-Z + Bb) - c.Rdif * (Z + Bb) - c.Tdif * (-Z + Bt));
  const bool emits = tau > kLw2TauMin;
  c.src_up = emits ? su : 0.;
  c.src_dn = emits ? sd : 0.;
  return c;
}

// Source at memory level jm (0-based, 0 .. nlay) from lev_source_dec(jm) and lev_source_inc(jm-1), whichever exist (the
// caller loads `dec` / `inc` from clamped indices); independent of top_at_1.  IEEE sqrt in both arithmetic modes: a
// product of two Planck sources may underflow to zero, which the fast square root does not take.
__device__ __forceinline__ double lw2_level_source(int jm, int nlay, double dec, double inc) {
  return jm == 0 ? dec : (jm == nlay ? inc : sqrt(dec * inc));
}

}  // namespace
}  // namespace ecckd
