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

// ---- single precision (ecckd_rte_lw_2stream_f32; the definition is spelt in include/ecckd_hip.h) ----
// The fp64 expressions cannot be retyped: in float 1 - e2 loses its digits in a thin layer and under the k floor, gamma1 -
// gamma2 loses them near ssa = 1, and the source terms (Z + Bt) - Rdif (-Z + Bt) - Tdif (Z + Bb) cancel quantities of size
// dB / tau down to a result of size tau B.  The float cell forms every such difference from its parts instead:
//   gamma1 - gamma2 = D (1 - ssa);   1 - e1 = n1 = -expm1(-x), x = k tau;   1 - e2 = m = n1 (1 + e1);   1 + e2 = 2 - m;
//   1 - Rdif - Tdif = A1 = RT (k n1^2 + (gamma1 - gamma2) m);
//   Z (1 + Rdif - Tdif) - Tdif dB = dB A2,  A2 = RT (k n1^2 / (tau (gamma1 + gamma2)) + k G),  G = m / x - 2 e1;
//   src_up = pi (Bt A1 + dB A2),  src_dn = pi (Bb A1 - dB A2)
// -- sums of positive terms but for G = 2 e1 (sinh(x) / x - 1), which is its series below kLw2XLinF (where the errors of
// the two forms cross: tests/test_lw_2stream_f32_host.py).  To first order in tau both sources are
// pi (gamma1 - gamma2) tau (Bt + Bb) / 2.  The floor under the square root stays 1e-12 (nothing divides by 1 - e2 any more);
// a layer emits where tau > 1e-30, so that the two quotients are taken of normal numbers.
constexpr float kLw2DF = 1.66f;
constexpr float kLw2PiF = 3.14159265358979323846f;
constexpr float kLw2KFloorF = 1.e-12f;
constexpr float kLw2TauMinF = 1.e-30f;
constexpr float kLw2XLinF = 0.7f;

template <typename real> struct Lw2CellT { real Rdif, Tdif, src_up, src_dn; };

// FAST: rcp<true> (hardware reciprocal and one Newton step); expf / expm1f / sqrtf are the device library's in both modes
template <bool FAST>
__device__ __forceinline__ Lw2CellT<float> lw_two_stream(float tau, float ssa, float g, float Bt, float Bb) {
  const float gamma1 = kLw2DF * (1.f - 0.5f * ssa * (1.f + g));
  const float gamma2 = kLw2DF * 0.5f * ssa * (1.f - g);
  const float gm = kLw2DF * (1.f - ssa);
  const float gp = gamma1 + gamma2;
  const float kk0 = gm * gp;
  const float k = sw_sqrt<FAST>(kk0 > kLw2KFloorF ? kk0 : kLw2KFloorF);
  const float x = tau * k;
  const float e1 = sw_exp<FAST>(-x);
  const float n1 = -expm1f(-x);
  const float m = n1 * (1.f + e1);
  const float RT = rcp<FAST>(k * (2.f - m) + gamma1 * m);
  Lw2CellT<float> c;
  c.Rdif = RT * gamma2 * m;
  c.Tdif = RT * 2.f * k * e1;
  const float kn = k * n1 * n1;
  const float A1 = RT * (kn + gm * m);
  const float x2 = x * x;
  const float Gs = e1 * (x2 * (1.f / 3.f)) * (1.f + (x2 * (1.f / 20.f)) * (1.f + x2 * (1.f / 42.f)));
  const float Gd = m * rcp<FAST>(x) - 2.f * e1;
  const float G = x < kLw2XLinF ? Gs : Gd;
  const float A2 = RT * (kn * rcp<FAST>(tau * gp) + k * G);
  const float dB = Bb - Bt;
  const float su = kLw2PiF * (Bt * A1 + dB * A2);
  const float sd = kLw2PiF * (Bb * A1 - dB * A2);
  const bool emits = tau > kLw2TauMinF;
  c.src_up = emits ? su : 0.f;
  c.src_dn = emits ? sd : 0.f;
  return c;
}

// (sqrtf of a product that underflows gives 0: a level source below 1e-19 W m-2 sr-1, which no flux can show)
__device__ __forceinline__ float lw2_level_source(int jm, int nlay, float dec, float inc) {
  return jm == 0 ? dec : (jm == nlay ? inc : sqrtf(dec * inc));
}

}  // namespace
}  // namespace ecckd
