// kernels_rte_lw.hip -- longwave no-scattering flux solver with the broadband g-point
// reduction fused in.
//
// Replaces RTE-RRTMGP's rte_lw as the reference calls it (example/rfmip-rad-irf/
// ecckd_rfmip_lw.F90:130-135): lw_solver_noscat_GaussQuad (transmittance, lw_source_noscat,
// lw_transport_noscat) followed by ty_fluxes_broadband%reduce (sum_broadband).
//
// Mapping (gfx950): one wave = CW columns x GW=64/CW g-points (CW = 32: measured 5 % faster than
// 16).  A load instruction therefore touches GW segments of CW*8 B (whole 128 B lines) of the
// column-fastest inputs.
// Each lane owns one (column, g-point) pair at a time and walks the layer recurrence:
//   down sweep: reads tau/lay_source/lev_source_{inc,dec} ONCE (4x8 B per cell, software
//               prefetched PF layers ahead), keeps trans(l) and source_up(l) in registers
//               (fully unrolled over NL layers), accumulates 2*pi*w*I_dn per level;
//   up sweep:   runs out of registers, accumulates 2*pi*w*I_up per level.
// The sum over g-points is a wave shuffle butterfly over the GW lanes that share a column
// followed by an add into a wave-private LDS accumulator (no inter-wave traffic, no atomics,
// deterministic).  After the last g-point group the accumulators are the broadband fluxes.
// Registers (512 per lane at one wave per SIMD) are the only place on the chip large enough
// for the 2*NL doubles per pair that the up sweep needs; the HBM latency is hidden by the
// explicit prefetch ring instead of by occupancy.
//
// NL > 0, EXACT: nlay == NL exactly, no per-layer predicates in the unrolled code (the 60-layer
//   benchmark and RFMIP shape).
// NL > 0, !EXACT: any nlay <= NL.  Layers s >= nlay of the unrolled code are made transparent
//   (tau = 0: trans = 1, sources 0) and accumulate into a dummy LDS row; the predicate s < nlay is
//   re-derived from an opaque copy of nlay at every use -- as a plain comparison the optimiser
//   hoists NL loop-invariant booleans and spills the SGPR file.  Costs NL/nlay of the arithmetic.
// NL > 0, OVER: nlay > NL.  The bottom NL layers run from registers as above; trans/source_up of
//   the top nlay - NL layers go through a per-wave global scratch ring (16 B/cell written and read
//   back for those layers only).
// SHARED: the two level-source arrays describe ONE value per level,
//   lev_source_inc(:,l,:) == lev_source_dec(:,l+1,:) -- what ecckd's gas optics produces
//   (src/gas_optics_ecckd.f90:419-424: both are slices of one buffer).  Either the caller asserts it
//   (ecckd_rte_lw_shared_levels) or the two arrays ARE the views of one level buffer (include/ecckd_hip.h,
//   "Level buffer": lev_source_inc == lev_source_dec + ncol), which the C ABI sees by itself.  The source
//   at the far edge of a layer is then the near-edge source of the next one: it is carried in a register and
//   only the first layer reads the second array (24 instead of 32 B/cell).  Same arithmetic, same bits.
//   The level arrays have a g-plane stride of their own here, RteLwArgs::lev_gstride: nlay*ncol for two
//   separate arrays, (nlay+1)*ncol for the views of the buffer.
#include <cstdlib>

#include "kernels.hpp"
#include "lw_layer.hpp"

namespace ecckd {
namespace {

#ifndef ECCKD_LW_PF
#define ECCKD_LW_PF 8
#endif
#ifndef ECCKD_LW_CW
#define ECCKD_LW_CW 32
#endif
#ifndef ECCKD_LW_CW_F32
#define ECCKD_LW_CW_F32 32
#endif
// prefetch depth in layers: 8 (measured 2 % faster than 4, equal to 12 and 16); 4 for the 96-layer variants,
// whose 2 x 96 resident values leave no room for a deeper ring
constexpr int prefetch_depth(int NL) { return NL >= 96 ? 4 : ECCKD_LW_PF; }
#ifndef ECCKD_LW_SPAN
#define ECCKD_LW_SPAN 2
#endif
constexpr int kSchedSpan = ECCKD_LW_SPAN;   // layers the instruction scheduler may interleave

template <typename real, int CW>
__device__ __forceinline__ real gsum(real v) {
  // sum over the lanes that share a column: lane = cl + CW*gs
#pragma unroll
  for (int o = CW; o < 64; o <<= 1) v = v + __shfl_xor(v, o);
  return v;
}

// acc += v by the owner lane (gs == 0) only, as one fire-and-forget ds_add_f64 (an exec-masked
// read/wait/add/write would expose the full LDS latency twice per layer at one wave per SIMD).
// The accumulators are double in both precisions: ds_add_f32 retires one lane every 3 clocks on
// gfx950 (193 clocks per wave instruction, tools/ubench_atomic.hip) against 6-13 clocks for
// ds_add_f64, and the broadband sum is the better for it.
// Every lane issues the atomic and non-owners add +0.0, which leaves the sum bit-identical whatever
// order the LDS unit serialises them in.  Exec-masking the owners makes the
// atomic itself cheaper (10.0 against 12.9 clocks at 4 waves per CU) but the exec juggling costs
// more than that in the kernel: measured 2-5 % slower.
template <typename real>
__device__ __forceinline__ void acc_add(double *p, real v, bool owner) {
  __hip_atomic_fetch_add(p, owner ? (double)v : 0., __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
}

// OFF32 (the exact-layer-count variants): the inputs of a g-point group are addressed as a wave-uniform pointer to the
// group's first plane plus ONE 32-bit byte offset per lane, advanced by a layer per request -- the loads take the pointer in
// SGPRs and no vector instruction builds an address (five 64-bit vector operations per layer otherwise, in a kernel that is
// paid per instruction).  Needs GW planes to span less than 4 GiB; launch_real() falls back to 64-bit offsets beyond.
//
// The kernels (rte_lw_kernel, rte_lw_allsky_f32_kernel, below) share one body, rte_lw_body.inc, included into each.  (An
// include, not a force-inlined function taking the arguments by reference: with that form twelve fp64 instantiations of
// rte_lw_kernel -- the padded SHARED ones and the overflow ones -- parked 1 to 10 more SGPRs in VGPR lanes; with the include
// every existing instantiation keeps its figures, profiles/allsky_f32_kernel_resources_*.txt.)
// ALLSKY (rte_lw_allsky_f32_kernel; ecckd_lw_fluxes_allsky_f32 and its McICA / both-skies forms): the particulate optical
// depth of the layer on the cell's band, a.part_tau / a.part_ssa (ncol,nlay,nband) through gpt2band, is added to the gas
// optical depth where the layer consumes tau -- tau + tp * (1 - sp), the operations of the by-band
// increment_1scalar_by_2stream in float (kernels_optical_props.hip; the build has FMA contraction off).  a.part_ssa null
// (one-stream particles) is served as sp = 0: tp * 1 is tp in every case.  a.part_mask (McICA): the 32-bit half of the
// (column, layer) word that holds the cell's g-point; a clear bit makes tp = 0, so the cell adds 0 * (1 - sp) as
// increment_masked_kernel does.  Both are wave-uniform selects, not template flags: the instantiations are not multiplied.
// The band values ride the prefetch ring of tau (same slots, same pinning), at offsets that differ from tau's by a
// per-pair constant: no address of their own is advanced.  Everything ALLSKY adds sits under `if constexpr`.
template <typename real, int NL, int CW, bool EXACT, bool OVER, bool SHARED, bool SER3, bool OFF32 = false>
__global__ void __launch_bounds__(64) rte_lw_kernel(const RteLwArgs a) {
  constexpr bool ALLSKY = false;
#include "rte_lw_body.inc"
}
// the all-sky / McICA form of the single-precision solver (ALLSKY above): one entry per variant launch_real<float, false> takes
template <int NL, int CW, bool EXACT, bool OVER, bool SER3, bool OFF32 = false>
__global__ void __launch_bounds__(64) rte_lw_allsky_f32_kernel(const RteLwArgs a) {
  typedef float real;
  constexpr bool SHARED = false, ALLSKY = true;
#include "rte_lw_body.inc"
}

// Sums the per-iteration partial fluxes of the tail tiles in iteration order.  A whole-tile wave adds the value of
// iteration 0, 1, ... to an accumulator that starts at +0; a tail unit holds 0 + v_it == v_it, so adding the units in
// the same order reproduces the whole-tile sum bit for bit: whether a column lands in a tail tile does not show.
template <typename real>
__global__ void __launch_bounds__(256) rte_lw_tail_reduce(const double *partials, int niter, int nlev, int cw, long tail_first,
                                                          long ntail, int ncol, long lev0, long lstep, real *flux_dn, real *flux_up) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= ntail * nlev * cw) return;
  const int cl = (int)(idx % cw), s = (int)((idx / cw) % nlev);
  const long t = idx / ((long)cw * nlev);
  const long col = (tail_first + t) * cw + cl;
  if (col >= ncol) return;
  const double *p = partials + (t * niter * 2 * nlev + s) * cw + cl;
  double dn = 0., up = 0.;
  for (int it = 0; it < niter; ++it, p += 2L * nlev * cw) {
    dn += p[0];
    up += p[(long)nlev * cw];
  }
  const long q = col + (long)ncol * (lev0 + lstep * s);
  flux_dn[q] = (real)dn;
  flux_up[q] = (real)up;
}

constexpr int kOverWaves = 2048;   // grid of the overflow variant (its scratch ring is per wave)
constexpr int kMaxRegisterLayers = 96;   // largest unrolled variant: 2 * 96 values + ~90 working registers of 512
constexpr int kOverCW = 16;   // 16 * (nlay + 2) * CW bytes of LDS accumulators per wave: 16 columns keep 4 waves per CU

template <typename real, int NL, int CW, bool EXACT, bool OVER, bool SHARED, bool SER3, bool OFF32 = false, bool ALLSKY = false>
hipError_t launch_ser(const RteLwArgs &a, hipStream_t s) {
  void (*k)(const RteLwArgs);
  if constexpr (ALLSKY) k = rte_lw_allsky_f32_kernel<NL, CW, EXACT, OVER, SER3, OFF32>;
  else k = rte_lw_kernel<real, NL, CW, EXACT, OVER, SHARED, SER3, OFF32>;
  const size_t lds = sizeof(double) * 2 * (size_t)(a.nlay + 1 + (EXACT ? 0 : 1)) * CW;
  if (lds > (size_t)kLdsBudget) return hipErrorInvalidValue;
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(k),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  long tiles = ((long)a.ncol + CW - 1) / CW;
  if (OVER && tiles > kOverWaves) tiles = kOverWaves;
  const long ntail = (!OVER && a.tail_first >= 0) ? tiles - a.tail_first : 0;
  const int niter = ((a.ng + 64 / CW - 1) / (64 / CW)) * a.nmus;
  const long blocks = tiles - ntail + ntail * niter;
  hipLaunchKernelGGL(k, dim3((unsigned)blocks), dim3(64), lds, s, a);
  e = hipGetLastError();
  if (e != hipSuccess || ntail == 0) return e;
  const int nlev = a.nlay + 1;
  const long n = ntail * nlev * CW;
  const long lev0 = a.top_at_1 ? 0 : a.nlay, lstep = a.top_at_1 ? 1 : -1;
  hipLaunchKernelGGL(rte_lw_tail_reduce<real>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a.partials, niter, nlev, CW,
                     a.tail_first, ntail, a.ncol, lev0, lstep, reinterpret_cast<real *>(a.flux_dn), reinterpret_cast<real *>(a.flux_up));
  return hipGetLastError();
}

template <typename real, int NL, int CW, bool EXACT, bool OVER, bool SHARED, bool ALLSKY = false>
hipError_t launch_one(const RteLwArgs &a, hipStream_t s) {
  if constexpr (EXACT) {   // 32-bit lane offsets when the planes of a g-point group span less than 4 GiB (see OFF32)
    // (the environment hook lets tests run the 64-bit form, which only calls beyond 4.4e6 columns take otherwise)
    // (SHARED: the level arrays' planes are lev_gstride apart, a level more than the others' in the buffer form)
    // (ALLSKY: the band planes are addressed from their first element, so all of them have to lie within 4 GiB as well)
    const double plane = SHARED && a.lev_gstride > (long long)a.ncol * a.nlay ? (double)a.lev_gstride : (double)a.ncol * a.nlay;
    const bool bands_fit = !ALLSKY || (double)a.ncol * a.nlay * a.nband * sizeof(real) < 4294967296.;
    if (plane * (64 / CW) * sizeof(real) < 4294967296. && bands_fit && !getenv("ECCKD_LW_NO_OFF32"))
      return a.series3 ? launch_ser<real, NL, CW, EXACT, OVER, SHARED, true, true, ALLSKY>(a, s)
                       : launch_ser<real, NL, CW, EXACT, OVER, SHARED, false, true, ALLSKY>(a, s);
  }
  return a.series3 ? launch_ser<real, NL, CW, EXACT, OVER, SHARED, true, false, ALLSKY>(a, s)
                   : launch_ser<real, NL, CW, EXACT, OVER, SHARED, false, false, ALLSKY>(a, s);
}

template <typename real, bool SHARED, bool ALLSKY = false>
hipError_t launch_real(const RteLwArgs &a, hipStream_t s) {
  constexpr int CW = sizeof(real) == 8 ? ECCKD_LW_CW : ECCKD_LW_CW_F32;
  if (a.nlay == 60) return launch_one<real, 60, CW, true, false, SHARED, ALLSKY>(a, s);
  if (a.nlay <= 32) return launch_one<real, 32, CW, false, false, SHARED, ALLSKY>(a, s);
  if (a.nlay <= 48) return launch_one<real, 48, CW, false, false, SHARED, ALLSKY>(a, s);
  if (a.nlay <= 64) return launch_one<real, 64, CW, false, false, SHARED, ALLSKY>(a, s);
  if (a.nlay <= 80) return launch_one<real, 80, CW, false, false, SHARED, ALLSKY>(a, s);
  if (a.nlay <= kMaxRegisterLayers) return launch_one<real, 96, CW, false, false, SHARED, ALLSKY>(a, s);
  return launch_one<real, 96, kOverCW, false, true, SHARED, ALLSKY>(a, s);
}

}  // namespace

// Tail split of the register-resident solver.  A wave owns a SIMD (512 registers), so `slots` tiles run at a time and
// the tiles beyond the last full round keep a fraction of the SIMDs busy for a whole tile time (1e5 columns: 3 125
// tiles on 1 024 SIMDs, the 4th round holds 53).  When that costs more than kTailGain of the call, the tail tiles are
// handed out one g-pair iteration per wave instead (53 x 16 units, one sixteenth of a round) and summed by
// rte_lw_tail_reduce, with the same bits.  Returns the bytes of `partials` the split needs (0: no split) and the first
// tail tile; the caller sets a.tail_first / a.partials when it can provide them and leaves tail_first = -1 otherwise.
size_t rte_lw_tail_plan(const RteLwArgs &a, int slots, long *tail_first) {
  constexpr double kTailGain = 0.03;
  constexpr size_t kTailMaxBytes = (size_t)64 << 20;
  *tail_first = -1;
  if (a.ncol <= 0 || a.nlay > kMaxRegisterLayers || slots <= 0) return 0;
  if (a.use_split && rte_lw_split_applies(a)) return 0;
  const int cw = a.f32 ? ECCKD_LW_CW_F32 : ECCKD_LW_CW, gw = 64 / cw;
  const long niter = (long)((a.ng + gw - 1) / gw) * a.nmus;
  const long tiles = ((long)a.ncol + cw - 1) / cw, full = tiles / slots * slots, ntail = tiles - full;
  if (ntail == 0 || niter < 2) return 0;
  const double before = (double)(full / slots + 1);
  const double after = (double)(full / slots) + (double)((ntail * niter + slots - 1) / slots) / (double)niter;
  if (before - after < kTailGain * before) return 0;
  const size_t bytes = sizeof(double) * 2 * (size_t)(a.nlay + 1) * cw * (size_t)(ntail * niter);
  if (bytes > kTailMaxBytes) return 0;
  *tail_first = full;
  return bytes;
}

size_t rte_lw_scratch_bytes(int ncol, int nlay, int ng) {
  (void)ng;
  if (nlay <= kMaxRegisterLayers) return 0;
  long tiles = ((long)ncol + kOverCW - 1) / kOverCW;
  if (tiles > kOverWaves) tiles = kOverWaves;
  return sizeof(double) * 2 * (size_t)(nlay - kMaxRegisterLayers) * 64 * (size_t)tiles;
}

hipError_t launch_rte_lw(const RteLwArgs &a, hipStream_t s) {
  if (a.ncol <= 0) return hipSuccess;
  if (a.use_split && rte_lw_split_applies(a)) return launch_rte_lw_split(a, s);
  if (a.shared_levels && !a.f32) return launch_real<double, true>(a, s);   // (no single-precision entry point sets it)
  return a.f32 ? launch_real<float, false>(a, s) : launch_real<double, false>(a, s);
}

// The register-resident single-precision solver with the particles added where it consumes tau (rte_lw_allsky_f32_kernel):
// a as for launch_rte_lw with f32 = 1 and two separate level arrays, plus part_tau / part_ssa (null: one-stream particles) /
// part_mask (null: unmasked), (ncol,nlay,nband) floats and (ncol,nlay) words.  Same variant, ring and tail split as
// launch_rte_lw takes for the shape.
hipError_t launch_rte_lw_allsky_f32(const RteLwArgs &a, hipStream_t s) {
  if (a.ncol <= 0) return hipSuccess;
  if (!a.f32 || !a.part_tau || a.shared_levels || (a.part_mask && a.ng > 64)) return hipErrorInvalidValue;
  return launch_real<float, false, true>(a, s);
}

}  // namespace ecckd
