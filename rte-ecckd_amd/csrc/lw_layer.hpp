// lw_layer.hpp -- the per-cell pieces of the longwave solvers, each written once: exp() and `/` of lw_source_noscat, the
// source function and transmittance of a layer, and the optical depth a cell has under particles, a McICA mask and the
// rescaling.  Shared by kernels_rte_lw.hip (exp and `/`), kernels_rte_lw_split.hip and kernels_rte_lw_jac.hip so that they
// produce the same bits per cell.
// [RTE-ext: the expressions they serve are restated from the public v1.5-era mo_rte_solver_kernels.F90 -- SURVEY.md
// Appendix B.1; call site example/rfmip-rad-irf/ecckd_rfmip_lw.F90:130-135.]
//
// The register-resident solver runs one wave per SIMD and issues one fp64 instruction every ~10 clocks: at 1e6 columns
// its ~75 vector instructions per cell ARE its run time (8.5e6 wave-instructions per CU at 0.40 per clock = 10.2 ms
// against 10.4 measured), so every instruction of the per-cell body counts.
#pragma once
#include <hip/hip_runtime.h>

#include "kernels.hpp"

namespace ecckd {
namespace {

// exp(x), fp64: the reduction x = n ln2 + r, |r| <= ln2 / 2, and a degree-11 polynomial (1 + r + r^2 g(r), g interpolated at
// Chebyshev nodes; <= 0.84 ulp on 4e4 random arguments against 200-bit arithmetic -- the accuracy class of the device
// library's exp).  Instead of that routine's two compares and three selects for results beyond the double range the
// argument is clamped to [-1100, 1100] (v_ldexp_f64 turns n < -1074 into +0 and n > 1023 into inf): 19 instructions
// against 22.  A NaN argument gives exp(-1100) = 0 (v_max_f64 returns its other operand): the callers' NaN reaches the
// fluxes through the optical depth itself (omt / tl, tl * (...)), see lw_source_noscat below each call.
__device__ __forceinline__ double lw_exp(double x) {
  x = __builtin_fmin(__builtin_fmax(x, -1100.), 1100.);
  const double n = __builtin_rint(x * 0x1.71547652b82fep+0);   // log2(e)
  double r = fma(n, -0x1.62e42fee00000p-1, x);                // ln2, upper 32 bits: n * hi is exact
  r = fma(n, -0x1.a39ef35793c76p-33, r);                        // ln2 - hi
  double p = 0x1.af38d53857513p-26;
  p = fma(p, r, 0x1.2891a8c1d838dp-22);
  p = fma(p, r, 0x1.71de0d9c145d0p-19);
  p = fma(p, r, 0x1.a019b8ef67c6cp-16);
  p = fma(p, r, 0x1.a01a01a7c8d47p-13);
  p = fma(p, r, 0x1.6c16c17893833p-10);
  p = fma(p, r, 0x1.11111111109adp-7);
  p = fma(p, r, 0x1.5555555553d4fp-5);
  p = fma(p, r, 0x1.5555555555556p-3);
  p = fma(p, r, 0x1.0000000000001p-1);
  p = fma(p, r, 1.);
  p = fma(p, r, 1.);
  return __builtin_amdgcn_ldexp(p, (int)n);
}
__device__ __forceinline__ float lw_exp(float x) { return expf(x); }

// x / d, fp64: the instruction sequence the compiler emits for `/` (reciprocal, two Newton steps, quotient, one residual
// correction) WITHOUT its v_div_scale / v_div_fixup frame -- 9 instructions against 11.  That frame rescales operands whose
// quotient or reciprocal leaves the normal range; for the one division of lw_source_noscat, (1 - t) / tl with
// tl in (tau_thresh, 1e290) and 1 - t in [tl / 2, 1], it never acts, and the quotient is the same bits as `/`
// (tools/check_lw_div.hip).  Outside: tl <= tau_thresh selects the series (whatever this returns, NaN and inf included,
// is dropped by the select); the divisor is bounded by 1e290, so an optical depth beyond -- up to inf -- gives ~1e-290
// where `/` gives less: both vanish against the flux.  A NaN divisor becomes 1e290 here (v_min_f64 returns its other
// operand) and reaches the fluxes through the series branch, which the select takes for it.
__device__ __forceinline__ double lw_div(double x, double d) {
  d = __builtin_fmin(d, 1e290);
  double r = __builtin_amdgcn_rcp(d);
  r = fma(fma(-d, r, 1.), r, r);
  r = fma(fma(-d, r, 1.), r, r);
  const double q = x * r;
  return fma(fma(-d, q, x), r, q);
}
__device__ __forceinline__ float lw_div(float x, float d) { return x / d; }

// Transmittance and the two sources of a layer (lw_source_noscat) from its slant optical depth tl, the
// layer source and the level sources at its down-sweep far edge (bdn) and its up-sweep far edge (bup).  Both branches of
// lw_source_noscat's merge() are evaluated and selected (no branch); SER3: the three-term series below tau_thresh.
// source_up is materialised here: left alone, the optimiser sinks the expression into the up sweep and keeps its five
// inputs alive per layer instead of the one result.
template <bool SER3, typename real>
__device__ __forceinline__ void lw_layer_source(real tl, real tau_thresh, real lay, real bdn, real bup, real &t, real &sdn, real &su_out) {
  t = lw_exp(-tl);
  const real omt = real(1) - t;
  const real fact_big = lw_div(omt, tl) - t;
  const real fact_small = SER3 ? tl * (real(0.5) + tl * (-real(1) / real(3) + tl * (real(1) / real(8))))
                               : tl * (real(0.5) - real(1) / real(3) * tl);
  const real fact = tl > tau_thresh ? fact_big : fact_small;
  sdn = omt * bdn + real(2) * fact * (lay - bdn);
  real su = omt * bup + real(2) * fact * (lay - bup);
  asm volatile("" : "+v"(su));
  su_out = su;
}

// Optical depth of a cell of the fused all-sky forms: the gas optical depth plus the particles of the lane's band, as they
// are (SKY = 1: one-stream particles, increment_1scalar_by_1scalar) or their absorption optical depth part_tau * (1 -
// part_ssa) (SKY = 2: two-stream particles, increment_1scalar_by_2stream) -- the expressions of kernels_optical_props.hip
// operation by operation.  cloudy: the McICA mask's bit of the cell (true without a mask); where it is clear the cell uses
// part_tau = 0 in front of the expressions.  (The flag and not the mask word: the callers carry words of different widths.)
template <int SKY>
__device__ __forceinline__ double lw_cell_tau(double tau_gas, double part_tau, double part_ssa, bool cloudy) {
  static_assert(SKY == 1 || SKY == 2, "one- or two-stream particles");
  const double tp = cloudy ? part_tau : 0.;
  return SKY == 1 ? tau_gas + tp : tau_gas + tp * (1. - part_ssa);
}

// Optical depth of a cell under the rescaled solver (include/ecckd_hip.h, "Rescaled longwave"): tau * sc, and Cn of the
// adjustment terms, from the cell's (tau, ssa, g).  BAND = false: (tau, ssa, g) are the cell's, as read from arrays (cloudy
// is not looked at).  BAND = true: tau is the gas optical depth and (part_tau, ssa, g) the triple of the lane's band; the
// cell's triple is formed with the operations of increment_body<double, true, true, true, MASK> of
// kernels_optical_props.hip on op1 = (tau_gas, +0, +0), its two IEEE divisions included.
// (IEEE division in Cn: ssa = g = 1 gives 0/0, a NaN that stays in its column.)
template <bool BAND>
__device__ __forceinline__ void lw_cell_rescaled(double tau, double part_tau, double ssa, double g, bool cloudy, double &tau_sc,
                                                 double &Cn) {
  if constexpr (BAND) {
    constexpr double tiny3 = op_eps<double>();
    const double tp = cloudy ? part_tau : 0.;
    const double tscat2 = tp * ssa;
    const double tsg2 = tscat2 * g;
    const double tau12 = tau + tp;
    const double tscat1 = tau * 0.;
    const double tauscat12 = tscat1 + tscat2;
    g = (tscat1 * 0. + tsg2) / (tauscat12 > tiny3 ? tauscat12 : tiny3);
    ssa = tauscat12 / (tau12 > tiny3 ? tau12 : tiny3);
    tau = tau12;
  }
  const double wb = ssa * (1. - g) * 0.5;
  const double sc = (1. - ssa) + wb;
  tau_sc = tau * sc;
  Cn = 0.4 * (wb / sc);
}

}  // namespace
}  // namespace ecckd
