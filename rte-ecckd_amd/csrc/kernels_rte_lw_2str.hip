// kernels_rte_lw_2str.hip -- two-stream longwave flux solver (clouds scatter) with the broadband g-point reduction
// fused in: RTE-RRTMGP's lw_solver_2stream, what rte_lw runs on ty_optical_props_2str with use_2stream = .true.
// [RTE-ext: restated from the public v1.5-era mo_rte_solver_kernels.F90; parity with RTE-RRTMGP is unpinned.]
//
// Mapping (gfx950): as rte_sw_body (kernels_rte_sw.hip) -- one wave = 16 columns x 4 g-points, lanes that share a column
// are summed with a wave shuffle butterfly into wave-private LDS accumulators [2][nlay+1][16]; persistent grid.
// Two passes per (column, g-point): surface -> top computes the two-stream coefficients and layer sources and runs the
// adding recurrence (albedo, source of upward radiation), parking both per level in a per-wave scratch ring
// ([array][level][lane], 512 B coalesced rows); top -> surface re-reads tau / ssa / g and the level sources, recomputes
// the coefficients and propagates the fluxes.  The level source is carried from one layer to the next: one sqrt and two
// loads per level.  Per cell and pass: tau, ssa, g, lev_source_dec, lev_source_inc (40 B), plus 16 B to and 16 B from
// the ring: 112 B -- in single precision (real = float) 20 B, 8 B and 8 B: 56 B.
#include <type_traits>

#include "kernels.hpp"
#include "lw_two_stream.hpp"

namespace ecckd {
namespace {

template <int I, int N, class F>
__device__ __forceinline__ void static_for_l2(F &&f) {
  if constexpr (I < N) {
    f(std::integral_constant<int, I>{});
    static_for_l2<I + 1, N>(f);
  }
}

template <int CW>
__device__ __forceinline__ double gsum_l2(double v) {
#pragma unroll
  for (int o = CW; o < 64; o <<= 1) v = v + __shfl_xor(v, o);   // joins lanes of ONE column only
  return v;
}

constexpr int kL2Waves = 4096;        // persistent grid, as rte_sw (three waves per SIMD resident)
constexpr int kL2WavesPerSimd = 3;
constexpr int kL2WavesPerSimdF32 = 2;   // (see l2_prefetch)
constexpr int kL2CW = 16;

// acc += v by the owner lane only: one fire-and-forget ds_add_f64 (see kernels_rte_sw.hip)
__device__ __forceinline__ void acc_add_l2(double *p, double v, bool owner) {
  __hip_atomic_fetch_add(p, owner ? v : 0., __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
}

// What a lane keeps in flight per layer: the cell's three properties (PART: the gas optical depth and the band triple,
// MASK: the half of the mask word that holds the lane's g-point) and the two level-source values of the layer's far level.
template <typename real, bool PART> struct L2Slot;
template <typename real> struct L2Slot<real, false> { real t, s, g, dec, inc; };
template <typename real> struct L2Slot<real, true> { real t, pt, ps, pg, dec, inc; unsigned m; };

// layers in flight per lane.  fp64: 3 (PART: 2) at three waves per SIMD.  Single precision: 6 (PART: 4) at TWO waves per
// SIMD (kL2WavesPerSimdF32).  The double accumulators in LDS bound the resident waves whatever `real` is -- 256 B per level and
// wave: 10 waves per CU at 60 layers, 4 at 137 -- so a third wave per SIMD is rarely there to lose, and a float layer in
// flight is half the bytes: the float kernels need twice the depth to keep as many bytes in flight per wave.  A layer in
// flight costs 17-20 VGPRs, most of them the addresses of its loads, so that depth does not fit three waves per SIMD (depth 4
// spills there; depth 3 / 3 / 2 fits and was measured 0-10 % slower at 60 and 137 layers: DESIGN.md section 5.5c).
template <typename real, bool PART> constexpr int l2_prefetch() { return (PART ? 2 : 3) * (sizeof(real) == 4 ? 2 : 1); }

template <typename real> __device__ __forceinline__ real l2_pi();
template <> __device__ __forceinline__ double l2_pi<double>() { return kLw2Pi; }
template <> __device__ __forceinline__ float l2_pi<float>() { return kLw2PiF; }

// real: storage and arithmetic type of everything per cell (tau, ssa, g or the band triple, both level-source planes, the
// ring, sfc_emis, sfc_source, inc_flux, the flux outputs: float data behind the double pointers of RteLw2strArgs); the
// g-point sums, the LDS accumulators and the owner-lane adds are double whatever `real` is, as in rte_sw_body.
// FAST: arithmetic mode 0.  PART / MASK: the fused all-sky call (RteLw2strArgs::part_*).
template <typename real, int CW, bool FAST, bool PART, bool MASK>
__device__ __forceinline__ void rte_lw_2str_body(const RteLw2strArgs &a) {
  static_assert(PART || !MASK, "a cloud mask belongs to the all-sky form");
  constexpr int GW = 64 / CW;
  constexpr int PF = l2_prefetch<real, PART>();
  typedef L2Slot<real, PART> Slot;
  typedef decltype(lw_two_stream<FAST>(real(0), real(0), real(0), real(0), real(0))) Cell;
  extern __shared__ double acc[];    // [2][nlay+1][CW]: up, dn
  auto P = [](const double *p) { return reinterpret_cast<const real *>(p); };
  auto Q = [](double *p) { return reinterpret_cast<real *>(p); };
  const int lane = threadIdx.x;
  const int cl = lane % CW, gs = lane / CW;
  const bool owner = gs == 0;
  const int ncol = a.ncol, nlay = a.nlay, ng = a.ng, nlev = nlay + 1;
  double *acc_up = acc, *acc_dn = acc + nlev * CW;
  const long lay0 = a.top_at_1 ? 0 : nlay - 1, lev0 = a.top_at_1 ? 0 : nlay;
  const long lstep = a.top_at_1 ? 1 : -1;
  // (elements of `real`: the float ring takes the first half of what rte_lw_2str_scratch_bytes provides)
  real *sc = Q(a.scratch) + (long)blockIdx.x * (2L * nlev) * 64 + lane;
  real *sAlb = sc, *sSrc = sc + 64L * nlev;
  const int ngroups = (ng + GW - 1) / GW;
  const long ntiles = ((long)ncol + CW - 1) / CW;

  for (long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const long col = tile * CW + cl;
    const bool valid = col < ncol;
    const long cc = valid ? col : (long)ncol - 1;
    for (int i = lane; i < 2 * nlev * CW; i += 64) acc[i] = 0.;

    for (int gi = 0; gi < ngroups; ++gi) {
      const int g = gi * GW + gs;
      const bool gact = g < ng;
      const int gg = gact ? g : ng - 1;
      const double keep = gact ? 1. : 0.;
      const long base = cc + (long)ncol * nlay * gg;
      const int band = a.gpt2band[gg];
      // layer sl (counted from the top) and the two values behind the source of level `lv` into a prefetch slot
      auto fetch = [&](int sl, int lv, Slot &p) __attribute__((always_inline)) {
        const long lm = lay0 + lstep * sl;
        const long q = base + (long)ncol * lm;
        p.t = P(a.tau)[q];
        if constexpr (PART) {
          const long qb = cc + (long)ncol * (lm + (long)nlay * band);
          p.pt = P(a.part_tau)[qb]; p.ps = P(a.part_ssa)[qb]; p.pg = P(a.part_g)[qb];
          if constexpr (MASK) p.m = reinterpret_cast<const unsigned *>(a.part_mask)[2 * (cc + (long)ncol * lm) + (gg >> 5)];
        } else {
          p.s = P(a.ssa)[q]; p.g = P(a.g)[q];
        }
        const long jm = lev0 + lstep * lv;
        p.dec = P(a.lev_source_dec)[base + (long)ncol * (jm < nlay ? jm : nlay - 1)];
        p.inc = P(a.lev_source_inc)[base + (long)ncol * (jm > 0 ? jm - 1 : 0)];
      };
      auto level = [&](int lv, const Slot &p) __attribute__((always_inline)) {
        return lw2_level_source((int)(lev0 + lstep * lv), nlay, p.dec, p.inc);
      };
      auto cell = [&](const Slot &p, real Bt, real Bb) __attribute__((always_inline)) {
        if constexpr (PART) {
          // increment_body<real, true, true, true, MASK> of kernels_optical_props.hip on op1 = (tau_gas, +0, +0)
          constexpr real eps = op_eps<real>();
          real t2 = p.pt;
          if constexpr (MASK) t2 = (p.m >> (gg & 31)) & 1u ? t2 : real(0);
          const real tscat2 = t2 * p.ps;
          const real tsg2 = tscat2 * p.pg;
          const real tau12 = p.t + t2;
          const real tscat1 = p.t * real(0);
          const real tauscat12 = tscat1 + tscat2;
          const real cg = (tscat1 * real(0) + tsg2) / (tauscat12 > eps ? tauscat12 : eps);
          const real cssa = tauscat12 / (tau12 > eps ? tau12 : eps);
          return lw_two_stream<FAST>(tau12, cssa, cg, Bt, Bb);
        } else {
          return lw_two_stream<FAST>(p.t, p.s, p.g, Bt, Bb);
        }
      };

      // ---- pass 1, surface -> top: coefficients, layer sources, adding ----
      const real emis = P(a.sfc_emis)[band + (long)a.nband * cc];
      real albedo = real(1) - emis;
      real src = l2_pi<real>() * emis * P(a.sfc_source)[cc + (long)ncol * gg];
      sAlb[64L * nlay] = albedo;
      sSrc[64L * nlay] = src;
      Slot slot[PF];
      fetch(nlay - 1, nlay, slot[0]);                 // (only the surface level's two values are used)
      real Bb = level(nlay, slot[0]);
#pragma unroll
      for (int d = 0; d < PF; ++d) { const int sl = nlay - 1 - d > 0 ? nlay - 1 - d : 0; fetch(sl, sl, slot[d]); }
      // (fixed prefetch slots, the layer loop unrolled by the depth: see rte_sw_body)
      auto layer1 = [&](int s, auto slot_c) __attribute__((always_inline)) {
        constexpr int d = decltype(slot_c)::value;
        const Slot p = slot[d];
        { const int sn = s - PF > 0 ? s - PF : 0; fetch(sn, sn, slot[d]); }
        const real Bt = level(s, p);
        const Cell c = cell(p, Bt, Bb);
        const real den = rcp<FAST>(real(1) - c.Rdif * albedo);
        src = c.src_up + c.Tdif * den * (src + albedo * c.src_dn);
        albedo = c.Rdif + c.Tdif * c.Tdif * albedo * den;
        sAlb[64L * s] = albedo;
        sSrc[64L * s] = src;
        Bb = Bt;
      };
      {
        int s = nlay - 1;
        for (; s >= PF - 1; s -= PF)
          static_for_l2<0, PF>([&](auto dc) __attribute__((always_inline)) { layer1(s - decltype(dc)::value, dc); });
        static_for_l2<0, PF>([&](auto dc) __attribute__((always_inline)) {
          if (s - decltype(dc)::value >= 0) layer1(s - decltype(dc)::value, dc);
        });
      }

      // ---- pass 2, top -> surface: fluxes ----
      real Bt = Bb;                                    // the source of level 0, as pass 1 left it
      real fdn = a.inc_flux ? P(a.inc_flux)[cc + (long)ncol * gg] : real(0);
      {
        const real fup = fdn * albedo + src;
        const double vu = gsum_l2<CW>(keep * (double)fup), vd = gsum_l2<CW>(keep * (double)fdn);
        acc_add_l2(&acc_up[cl], vu, owner);
        acc_add_l2(&acc_dn[cl], vd, owner);
      }
      real palb[PF], psrc[PF];
#pragma unroll
      for (int d = 0; d < PF; ++d) {
        const int sl = d < nlay ? d : nlay - 1;
        palb[d] = sAlb[64L * (sl + 1)]; psrc[d] = sSrc[64L * (sl + 1)];
        fetch(sl, sl + 1, slot[d]);
      }
      auto layer2 = [&](int s, auto slot_c) __attribute__((always_inline)) {
        constexpr int d = decltype(slot_c)::value;
        const real alb_next = palb[d], src_next = psrc[d];
        const Slot p = slot[d];
        {
          const int sn = s + PF < nlay ? s + PF : nlay - 1;
          palb[d] = sAlb[64L * (sn + 1)]; psrc[d] = sSrc[64L * (sn + 1)];
          fetch(sn, sn + 1, slot[d]);
        }
        const real Bn = level(s + 1, p);
        const Cell c = cell(p, Bt, Bn);
        const real den = rcp<FAST>(real(1) - c.Rdif * alb_next);   // the same expression as in pass 1: same bits
        fdn = (c.Tdif * fdn + c.Rdif * src_next + c.src_dn) * den;
        const real fup = fdn * alb_next + src_next;
        Bt = Bn;
        const double vu = gsum_l2<CW>(keep * (double)fup), vd = gsum_l2<CW>(keep * (double)fdn);
        acc_add_l2(&acc_up[(s + 1) * CW + cl], vu, owner);
        acc_add_l2(&acc_dn[(s + 1) * CW + cl], vd, owner);
      };
      {
        int s = 0;
        for (; s + PF <= nlay; s += PF)
          static_for_l2<0, PF>([&](auto dc) __attribute__((always_inline)) { layer2(s + decltype(dc)::value, dc); });
        static_for_l2<0, PF>([&](auto dc) __attribute__((always_inline)) {
          if (s + decltype(dc)::value < nlay) layer2(s + decltype(dc)::value, dc);
        });
      }
    }

    if (valid) {
      for (int s = gs; s < nlev; s += GW) {
        const long q = col + (long)ncol * (lev0 + lstep * s);
        Q(a.flux_up)[q] = (real)acc_up[s * CW + cl];
        Q(a.flux_dn)[q] = (real)acc_dn[s * CW + cl];
      }
    }
  }
}

template <int CW, bool FAST>
__global__ void __launch_bounds__(64, kL2WavesPerSimd) rte_lw_2str_kernel(const RteLw2strArgs a) {
  rte_lw_2str_body<double, CW, FAST, false, false>(a);
}
// the fused all-sky forms (fast arithmetic mode only), under their own names so that their figures can be told apart in the
// code object (tools/kernel_resources.py)
template <int CW>
__global__ void __launch_bounds__(64, kL2WavesPerSimd) rte_lw_2str_allsky_kernel(const RteLw2strArgs a) {
  rte_lw_2str_body<double, CW, true, true, false>(a);
}
template <int CW>
__global__ void __launch_bounds__(64, kL2WavesPerSimd) rte_lw_2str_mcica_kernel(const RteLw2strArgs a) {
  rte_lw_2str_body<double, CW, true, true, true>(a);
}
// the single-precision forms (launch_rte_lw_2str_f32; fast arithmetic mode only), each under its own name
template <int CW>
__global__ void __launch_bounds__(64, kL2WavesPerSimdF32) rte_lw_2str_f32_kernel(const RteLw2strArgs a) {
  rte_lw_2str_body<float, CW, true, false, false>(a);
}
template <int CW>
__global__ void __launch_bounds__(64, kL2WavesPerSimdF32) rte_lw_2str_allsky_f32_kernel(const RteLw2strArgs a) {
  rte_lw_2str_body<float, CW, true, true, false>(a);
}
template <int CW>
__global__ void __launch_bounds__(64, kL2WavesPerSimdF32) rte_lw_2str_mcica_f32_kernel(const RteLw2strArgs a) {
  rte_lw_2str_body<float, CW, true, true, true>(a);
}

long l2_blocks(int ncol) {
  long tiles = ((long)ncol + kL2CW - 1) / kL2CW;
  return tiles > kL2Waves ? kL2Waves : tiles;
}

}  // namespace

size_t rte_lw_2str_scratch_bytes(int ncol, int nlay, int ng) {
  (void)ng;
  if (ncol <= 0 || nlay < 1) return 0;
  return sizeof(double) * (size_t)(2L * (nlay + 1)) * 64 * (size_t)l2_blocks(ncol);
}

namespace {
hipError_t launch_l2(void (*k)(const RteLw2strArgs), const RteLw2strArgs &a, hipStream_t s) {
  constexpr int CW = kL2CW;
  const size_t lds = sizeof(double) * 2 * (size_t)(a.nlay + 1) * CW;
  if (lds > (size_t)kLdsBudget) return hipErrorInvalidValue;
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k, dim3((unsigned)l2_blocks(a.ncol)), dim3(64), lds, s, a);
  return hipGetLastError();
}
}  // namespace

hipError_t launch_rte_lw_2str(const RteLw2strArgs &a, hipStream_t s) {
  if (a.ncol <= 0) return hipSuccess;
  constexpr int CW = kL2CW;
  if (!a.scratch) return hipErrorInvalidValue;
  if (a.part_tau && (a.exact_division || !a.part_ssa || !a.part_g)) return hipErrorInvalidValue;
  if (a.part_mask && (!a.part_tau || a.ng > 64)) return hipErrorInvalidValue;
  auto k = a.part_mask ? rte_lw_2str_mcica_kernel<CW>
           : a.part_tau ? rte_lw_2str_allsky_kernel<CW>
           : a.exact_division ? rte_lw_2str_kernel<CW, false> : rte_lw_2str_kernel<CW, true>;
  return launch_l2(k, a, s);
}

hipError_t launch_rte_lw_2str_f32(const RteLw2strArgs &a, hipStream_t s) {
  if (a.ncol <= 0) return hipSuccess;
  constexpr int CW = kL2CW;
  if (!a.scratch || a.exact_division) return hipErrorInvalidValue;
  if (a.part_tau && (!a.part_ssa || !a.part_g)) return hipErrorInvalidValue;
  if (a.part_mask && (!a.part_tau || a.ng > 64)) return hipErrorInvalidValue;
  auto k = a.part_mask ? rte_lw_2str_mcica_f32_kernel<CW> : a.part_tau ? rte_lw_2str_allsky_f32_kernel<CW> : rte_lw_2str_f32_kernel<CW>;
  return launch_l2(k, a, s);
}

}  // namespace ecckd
