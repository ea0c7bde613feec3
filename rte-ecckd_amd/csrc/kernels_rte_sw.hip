// kernels_rte_sw.hip -- shortwave two-stream + adding flux solver with the broadband g-point
// reduction fused in, and the toa_src broadcast of gas_optics_ext.
//
// Replaces RTE-RRTMGP's rte_sw as the reference calls it (example/rfmip-rad-irf/
// ecckd_rfmip_sw.F90:148-154): sw_two_stream (Zdunkowski PIFM / Meador-Weaver), sw_source_2str,
// adding, flux_dn = diffuse + direct, then ty_fluxes_broadband%reduce.
//
// Mapping (gfx950): as the LW solver -- one wave = CW columns x GW=64/CW g-points, lanes that
// share a column are summed with a wave shuffle butterfly into wave-private LDS accumulators.
// Two passes per (column, g-point): bottom->top computes the two-stream coefficients and runs the
// adding recurrences with the source normalised by the direct beam (which is only known on the way
// down); top->bottom propagates the direct beam and the fluxes.  The per-level albedo and source go
// through a per-wave global scratch ring ([array][level][lane], 512 B coalesced rows); the second pass
// recomputes the two-stream coefficients (see rte_sw_body for why).
// (Registers cannot hold it next to a useful occupancy: the coefficient arithmetic is ~250 fp64
// instructions per cell and needs several waves per SIMD to issue at rate.)
// Any layer count and both precisions: the route of every call the layer-systolic solver does not serve (more than 60
// layers, or "sw_solver" = 1), the fused shortwave path (DERIVE) included.
#include <type_traits>

#include "kernels.hpp"
#include "sw_two_stream.hpp"

namespace ecckd {
namespace {

// f(integral_constant<int, I>) for I = I0 .. N-1 as straight-line code (compile-time slot indices)
template <int I, int N, class F>
__device__ __forceinline__ void static_for_sw(F &&f) {
  if constexpr (I < N) {
    f(std::integral_constant<int, I>{});
    static_for_sw<I + 1, N>(f);
  }
}

template <int CW>
__device__ __forceinline__ double gsum(double v) {
#pragma unroll
  for (int o = CW; o < 64; o <<= 1) v = v + __shfl_xor(v, o);
  return v;
}

#ifndef ECCKD_SW_WAVES
#define ECCKD_SW_WAVES 4096   // 12 waves per CU are resident (143 VGPRs); a grid of 4096 measured 15 % faster than 2048
#endif
// Registers: the kernel needs 143 VGPRs, i.e. three waves per SIMD (12 per CU).  Forcing it under 128 for four waves
// per SIMD was measured in round 2 (same box, tools/ab.py): with the compiler's 2-9 spills 3.80-3.88 ms, with a prefetch
// depth of 2 (no spill) 3.81-3.85 ms, against 3.78 ms as is -- the kernel is bound by fp64 issue, which three waves per
// SIMD already saturate (tools/ubench.hip: 0.74 of 0.86 wave-instructions/clk/CU), so the allocation is left alone.
#ifndef ECCKD_SW_WAVES_PER_SIMD
#define ECCKD_SW_WAVES_PER_SIMD 3
#endif
#ifndef ECCKD_SW_CW
#define ECCKD_SW_CW 16
#endif
#ifndef ECCKD_SW_PF
#define ECCKD_SW_PF 3
#endif
constexpr int kPF = ECCKD_SW_PF;   // layers of optical properties in flight per lane
constexpr int kSwWaves = ECCKD_SW_WAVES;

// acc += v by the owner lane only (the other lanes add +0.0): one fire-and-forget ds_add_f64,
// order-independent result (see kernels_rte_lw.hip).
__device__ __forceinline__ void acc_add(double *p, double v, bool owner) {
  __hip_atomic_fetch_add(p, owner ? v : 0., __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
}

// Pass 2 reads tau/ssa/g again and recomputes the two-stream coefficients; only the two per-level
// quantities go through the scratch ring (24 + 16 + 24 + 16 = 80 B/cell of traffic, twice the
// arithmetic).  Storing the four per-layer products pass 2 needs as well costs 120 B/cell, and the
// kernel is bound by that traffic, not by the arithmetic: measured 4.52 ms stored vs 3.85 ms
// recomputed per 1e5 columns x 27 g-points (recomputed: 52 % of the fp64 VALU rate).
//
// real: storage and arithmetic type of everything per cell (inputs, two-stream arithmetic, scratch ring, outputs); the
// g-point sums, the LDS accumulators and the tail partials are double whatever `real` is, as in rte_sw_sys_kernel.
// DERIVE: fused shortwave path (RteSwArgs::derive): tau is the total optical depth and ssa / g / toa come from
// rte_sw_sys_kernel's expressions (src/gas_optics_ecckd.f90:313-317,455-472); the lane's layer slots then prefetch the two
// level pressures of a layer in place of its ssa and g.
// ALLSKY (with DERIVE; ecckd_sw_fluxes_allsky): the layer's particulate triple on the cell's band (RteSwArgs::part_*) rides
// in the prefetch slot too and is added to the gas optics where ssa is formed -- RTE-RRTMGP's increment_2stream_by_2stream
// with op1 = (tau, moles*ray/tau, 0): no per-g-point ssa or g exists in memory.  A lane walks all layers of one g-point before the
// next, so the triple cannot stay in registers across the g-points of a band as it could in a layer-resident solver: it is
// requested per (layer, g-point), three band-plane loads beside the layer's tau and its two pressures.
// MASK (with ALLSKY; ecckd_sw_fluxes_allsky_mcica): the 32-bit half of the layer's cloud-mask word (RteSwArgs::part_mask,
// one 64-bit word per (column, layer)) that holds the lane's g-point rides with the triple; where the bit is clear the
// cell uses a particulate optical depth of 0 in front of the same expressions.
// The kernels (rte_sw_kernel, rte_sw_allsky_kernel and rte_sw_mcica_kernel, below) are thin entries to this body.
template <typename real> struct SwPart { real t, s, g; unsigned m; };
// WIN (with MASK; ecckd_sw_flux_bands): the launch covers a band of the model and its g-point g sees bit
// RteSwArgs::mask_first + g of the mask word, as in rte_sw_sys_body.
// SCALE (with ALLSKY, without MASK; ecckd_sw_flux_scaled): the cell's float32 optical-depth scaling (RteSwArgs::part_scaling,
// one value per (column, layer, g-point), at the index of tau) rides in the slot of the mask half-word, as its bits; the
// cell uses the particulate optical depth tp * scaling in front of the same expressions.
template <typename real, int CW, bool FAST, bool CLAMP, bool DERIVE, bool ALLSKY = false, bool MASK = false, bool WIN = false,
          bool SCALE = false>
__device__ __forceinline__ void rte_sw_body(const RteSwArgs &a) {
  static_assert(!SCALE || (ALLSKY && !MASK), "the scaling belongs to the all-sky form and stands in the mask's place");
  static_assert(DERIVE || !ALLSKY, "the all-sky form extends the fused (DERIVE) form");
  static_assert(ALLSKY || !MASK, "a cloud mask belongs to the all-sky form");
  static_assert(MASK || !WIN, "a band window concerns the mask bit alone");
  constexpr int GW = 64 / CW;
  // (fp32 DERIVE: the correctly rounded fp32 division of ssa makes three layers in flight spill; two do not)
  // (ALLSKY: three more values per layer in flight; with three layers the 168 registers of three waves per SIMD spill)
  constexpr int PF = ((DERIVE && sizeof(real) == 4) || ALLSKY) ? 2 : kPF;
  extern __shared__ double acc[];   // [3][nlay+1][CW]: up, dn, dir
  auto P = [](const double *p) { return reinterpret_cast<const real *>(p); };
  auto Q = [](double *p) { return reinterpret_cast<real *>(p); };
  const int lane = threadIdx.x;
  const int cl = lane % CW, gs = lane / CW;
  const bool owner = gs == 0;
  const int ncol = a.ncol, nlay = a.nlay, ng = a.ng, nlev = nlay + 1;
  double *acc_up = acc, *acc_dn = acc + nlev * CW, *acc_dir = acc + 2 * nlev * CW;
  const long lay0 = a.top_at_1 ? 0 : nlay - 1, lev0 = a.top_at_1 ? 0 : nlay;
  const long lstep = a.top_at_1 ? 1 : -1;
  // scratch ring of this wave: the level arrays albedo and normalised source, each [level][64 lanes]
  // (elements of `real`: the fp32 ring takes half of what rte_sw_scratch_bytes provides)
  real *sc = Q(a.scratch) + (long)blockIdx.x * (2L * nlev) * 64 + lane;
  real *sAlb = sc, *sSrc = sc + 64L * nlev;
  const int ngroups = (ng + GW - 1) / GW;
  const long ntiles = ((long)ncol + CW - 1) / CW;
  const real k_floor = (real)a.k_floor;
  const real k_floor_tau = (real)a.k_floor_tau;
  const real gw = (real)a.gw;

  // Work units (see rte_sw_tail_plan): units [0, tail_first) are whole tiles; beyond that a unit is ONE g-point group
  // of a tail tile and leaves its sums in `partials` for rte_sw_tail_reduce.
  const long tail_first = a.tail_first < 0 ? ntiles : a.tail_first;
  const long nunits = tail_first + (ntiles - tail_first) * ngroups;
  for (long unit = blockIdx.x; unit < nunits; unit += gridDim.x) {
    long tile = unit;
    int g0 = 0, g1 = ngroups;
    if (unit >= tail_first) {
      const long u = unit - tail_first;
      tile = tail_first + u / ngroups;
      g0 = (int)(u - (tile - tail_first) * ngroups);
      g1 = g0 + 1;
    }
    const long col = tile * CW + cl;
    const bool valid = col < ncol;
    const long cc = valid ? col : (long)ncol - 1;
    for (int i = lane; i < 3 * nlev * CW; i += 64) acc[i] = 0.;
    const real mu0 = P(a.mu0)[cc];
    const real mu0_inv = real(1) / mu0;
    const real tscale = (DERIVE && a.toa_scale) ? P(a.toa_scale)[cc] : real(1);

    for (int gi = g0; gi < g1; ++gi) {
      const int g = gi * GW + gs;
      const bool gact = g < ng;
      const int gg = gact ? g : ng - 1;
      const double keep = gact ? 1. : 0.;
      const long base = cc + (long)ncol * nlay * gg;
      const int band = a.gpt2band[gg];
      [[maybe_unused]] const int gm = WIN ? gg + a.mask_first : gg;   // MASK: the cell's bit of the mask word
      const real ray = DERIVE ? P(a.rayleigh)[gg] : real(0);
      // optical properties of layer sl (counted from the top) into prefetch slot d.  DERIVE: pssa / pg take plev at the
      // layer's two levels, turned into ssa by props() once they have arrived
      auto fetch = [&](int sl, real &t, real &x, real &y, SwPart<real> &pp) __attribute__((always_inline)) {
        const long lm = lay0 + lstep * sl;   // layer index in memory
        const long q = base + (long)ncol * lm;
        t = P(a.tau)[q];
        if constexpr (ALLSKY) {
          const long qb = cc + (long)ncol * (lm + (long)nlay * band);
          pp.t = P(a.part_tau)[qb]; pp.s = P(a.part_ssa)[qb]; pp.g = P(a.part_g)[qb];
          if constexpr (MASK) pp.m = reinterpret_cast<const unsigned *>(a.part_mask)[2 * (cc + (long)ncol * lm) + (gm >> 5)];
          if constexpr (SCALE) pp.m = reinterpret_cast<const unsigned *>(a.part_scaling)[q];
        }
        if constexpr (DERIVE) { x = P(a.plev)[cc + (long)ncol * lm]; y = P(a.plev)[cc + (long)ncol * (lm + 1)]; }
        else { x = P(a.ssa)[q]; y = P(a.g)[q]; }
      };
      // two-stream coefficients of a cell from its prefetch slot
      auto props = [&](real ctau, real x, real y, const SwPart<real> &pp) __attribute__((always_inline)) {
        if constexpr (ALLSKY) {
          constexpr real eps = op_eps<real>();
          const real tau_r = ((y - x) * gw) * ray;             // :313-316: the Rayleigh optical depth, tau*ssa of the gas optics
          real tp = pp.t;
          if constexpr (MASK) tp = (pp.m >> (gm & 31)) & 1u ? tp : real(0);
          if constexpr (SCALE) tp = tp * (real)__uint_as_float(pp.m);
          const real tsp = tp * pp.s;
          const real ts = tau_r + tsp, tau12 = ctau + tp;      // increment_2stream_by_2stream
          const real cg = (tsp * pp.g) / (ts > eps ? ts : eps);
          const real cssa = ts / (tau12 > eps ? tau12 : eps);
          return two_stream<real, FAST, CLAMP, false>(tau12, cssa, cg, mu0, mu0_inv, k_floor, k_floor_tau);
        }
        else if constexpr (DERIVE) {
          const real moles = (y - x) * gw;                     // :313-314
          const real cssa = (moles * ray) / ctau;              // :316, :459-460 (IEEE division in every mode)
          return two_stream<real, FAST, CLAMP, true>(ctau, cssa, real(0), mu0, mu0_inv, k_floor, k_floor_tau);   // g = 0
        }
        else
          return __all(y == real(0)) ? two_stream<real, FAST, CLAMP, true>(ctau, x, y, mu0, mu0_inv, k_floor, k_floor_tau)
                                     : two_stream<real, FAST, CLAMP, false>(ctau, x, y, mu0, mu0_inv, k_floor, k_floor_tau);
      };

      // ---- pass 1, bottom -> top: two-stream coefficients (sw_two_stream) and the adding
      // recurrences (albedo, source of upward radiation).  The direct beam is not known yet on the
      // way up, so the source is carried normalised by the direct flux at its own level:
      //   src(l) = nsrc(l) * F_dir(l),  F_dir(l+1) = Tnoscat(l) * F_dir(l)
      real albedo = P(a.alb_dif)[band + (long)a.nband * cc];
      real nsrc = P(a.alb_dir)[band + (long)a.nband * cc];   // src_sfc = F_dir(sfc) * sfc_alb_dir
      sAlb[64L * nlay] = albedo;
      sSrc[64L * nlay] = nsrc;
      // (the optical properties of layer s - PF are requested before the arithmetic of layer s: the
      // loop is a serial recurrence and the compiler does not pipeline it)
      real ptau[PF], pssa[PF], pg[PF];
      SwPart<real> ppart[PF];   // (ALLSKY only)
#pragma unroll
      for (int d = 0; d < PF; ++d) fetch(nlay - 1 - d > 0 ? nlay - 1 - d : 0, ptau[d], pssa[d], pg[d], ppart[d]);
      // The layer loop is unrolled by the prefetch depth so that every layer has a FIXED slot of the prefetch registers:
      // shifting the slots along (ptau[d] = ptau[d + 1]) reads registers whose loads are still in flight and made the
      // compiler wait with vmcnt(0) in every iteration -- one layer of loads in flight instead of PF (round 2).
      auto layer1 = [&](int s, auto slot_c) __attribute__((always_inline)) {
        constexpr int d = decltype(slot_c)::value;
        const real ctau = ptau[d], cx = pssa[d], cy = pg[d];
        const SwPart<real> cp = ppart[d];
        fetch(s - PF > 0 ? s - PF : 0, ptau[d], pssa[d], pg[d], ppart[d]);
        const TwoStreamT<real> ts = props(ctau, cx, cy, cp);
        const real denom = rcp<FAST>(real(1) - ts.Rdif * albedo);                          // adding, Eq 10
        // Eq 11 divided by F_dir(l): src_up = Rdir*F_dir(l), src_dn = Tdir*F_dir(l), src(l+1) = nsrc*Tnoscat*F_dir(l)
        nsrc = ts.Rdir + ts.Tdif * denom * (nsrc * ts.Tnoscat + albedo * ts.Tdir);
        albedo = ts.Rdif + ts.Tdif * ts.Tdif * albedo * denom;                        // Eq 9
        sAlb[64L * s] = albedo;
        sSrc[64L * s] = nsrc;
      };
      {
        int s = nlay - 1;
        for (; s >= PF - 1; s -= PF)                 // whole groups: slot d serves layer s - d
          static_for_sw<0, PF>([&](auto dc) __attribute__((always_inline)) { layer1(s - decltype(dc)::value, dc); });
        static_for_sw<0, PF>([&](auto dc) __attribute__((always_inline)) {   // the last, partial group
          if (s - decltype(dc)::value >= 0) layer1(s - decltype(dc)::value, dc);
        });
      }

      // ---- pass 2, top -> bottom: direct beam and fluxes (Eq 12, 13) ----
      const real toa = DERIVE ? P(a.solar)[gg] * tscale : P(a.toa)[cc + (long)ncol * gg];   // :468-472
      real fdir = toa * mu0;
      real fdn = real(0);
      {
        const real fup = fdn * albedo + nsrc * fdir;
        const double vu = gsum<CW>(keep * (double)fup), vd = gsum<CW>(keep * (double)(fdn + fdir)), vr = gsum<CW>(keep * (double)fdir);
        acc_add(&acc_up[cl], vu, owner);
        acc_add(&acc_dn[cl], vd, owner);
        acc_add(&acc_dir[cl], vr, owner);
      }
      real palb[PF], pnsrc[PF];
#pragma unroll
      for (int d = 0; d < PF; ++d) {
        const int sl = d < nlay ? d : nlay - 1;
        palb[d] = sAlb[64L * (sl + 1)]; pnsrc[d] = sSrc[64L * (sl + 1)];
        fetch(sl, ptau[d], pssa[d], pg[d], ppart[d]);
      }
      auto layer2 = [&](int s, auto slot_c) __attribute__((always_inline)) {   // (fixed prefetch slots: see pass 1)
        constexpr int d = decltype(slot_c)::value;
        const real alb_next = palb[d], nsrc_next = pnsrc[d];
        const real ctau = ptau[d], cx = pssa[d], cy = pg[d];
        const SwPart<real> cp = ppart[d];
        {
          const int sn = s + PF < nlay ? s + PF : nlay - 1;
          palb[d] = sAlb[64L * (sn + 1)]; pnsrc[d] = sSrc[64L * (sn + 1)];
          fetch(sn, ptau[d], pssa[d], pg[d], ppart[d]);
        }
        const TwoStreamT<real> ts = props(ctau, cx, cy, cp);
        const real denom = rcp<FAST>(real(1) - ts.Rdif * alb_next);  // the same expression as in pass 1: same bits
        const real A = ts.Tdif * denom, B = ts.Rdif * denom, C = ts.Tdir * denom, Tn = ts.Tnoscat;
        const real fdir_next = Tn * fdir;
        const real src_next = nsrc_next * fdir_next;
        fdn = A * fdn + B * src_next + C * fdir;
        const real fup = fdn * alb_next + src_next;
        fdir = fdir_next;
        const double vu = gsum<CW>(keep * (double)fup), vd = gsum<CW>(keep * (double)(fdn + fdir)), vr = gsum<CW>(keep * (double)fdir);
        acc_add(&acc_up[(s + 1) * CW + cl], vu, owner);
        acc_add(&acc_dn[(s + 1) * CW + cl], vd, owner);
        acc_add(&acc_dir[(s + 1) * CW + cl], vr, owner);
      };
      {
        int s = 0;
        for (; s + PF <= nlay; s += PF)              // whole groups: slot d serves layer s + d
          static_for_sw<0, PF>([&](auto dc) __attribute__((always_inline)) { layer2(s + decltype(dc)::value, dc); });
        static_for_sw<0, PF>([&](auto dc) __attribute__((always_inline)) {   // the last, partial group
          if (s + decltype(dc)::value < nlay) layer2(s + decltype(dc)::value, dc);
        });
      }
    }

    if (unit >= tail_first) {   // one g-point group of a tail tile: [unit][up, dn, dir][nlev][CW]
      double *pp = a.partials + (unit - tail_first) * 3 * nlev * CW;
      for (int s = gs; s < nlev; s += GW) {
        pp[s * CW + cl] = acc_up[s * CW + cl];
        pp[(nlev + s) * CW + cl] = acc_dn[s * CW + cl];
        pp[(2 * nlev + s) * CW + cl] = acc_dir[s * CW + cl];
      }
    } else if (valid) {
      for (int s = gs; s < nlev; s += GW) {
        const long q = col + (long)ncol * (lev0 + lstep * s);
        Q(a.flux_up)[q] = (real)acc_up[s * CW + cl];
        Q(a.flux_dn)[q] = (real)acc_dn[s * CW + cl];
        if (a.flux_dir) Q(a.flux_dir)[q] = (real)acc_dir[s * CW + cl];
      }
    }
  }
}

// fp64, ssa / g / toa read from memory: the instantiations the API path has always taken, under their own names
template <int CW, bool FAST, bool CLAMP>
__global__ void __launch_bounds__(64, ECCKD_SW_WAVES_PER_SIMD) rte_sw_kernel(const RteSwArgs a) {
  rte_sw_body<double, CW, FAST, CLAMP, false>(a);
}
// single precision, and the fused form (DERIVE) in either precision
template <typename real, int CW, bool FAST, bool CLAMP, bool DERIVE>
__global__ void __launch_bounds__(64, ECCKD_SW_WAVES_PER_SIMD) rte_sw_kernel(const RteSwArgs a) {
  rte_sw_body<real, CW, FAST, CLAMP, DERIVE>(a);
}

// fused all-sky form (fp64, fast arithmetic mode): its own name, so that the figures of the clear-sky instantiations can be
// told apart in the code object (tools/kernel_resources.py)
template <int CW, bool CLAMP>
__global__ void __launch_bounds__(64, ECCKD_SW_WAVES_PER_SIMD) rte_sw_allsky_kernel(const RteSwArgs a) {
  rte_sw_body<double, CW, true, CLAMP, true, true>(a);
}

// ... with a McICA cloud mask (RteSwArgs::part_mask), under its own name
template <int CW, bool CLAMP>
__global__ void __launch_bounds__(64, ECCKD_SW_WAVES_PER_SIMD) rte_sw_mcica_kernel(const RteSwArgs a) {
  rte_sw_body<double, CW, true, CLAMP, true, true, true>(a);
}

// ... with a sampled optical-depth scaling (RteSwArgs::part_scaling) in the mask's place, under its own name
template <int CW, bool CLAMP>
__global__ void __launch_bounds__(64, ECCKD_SW_WAVES_PER_SIMD) rte_sw_scaled_kernel(const RteSwArgs a) {
  rte_sw_body<double, CW, true, CLAMP, true, true, false, false, true>(a);
}

// ... on a band window of the model (ecckd_sw_flux_bands with a mask), under its own name
template <int CW, bool CLAMP>
__global__ void __launch_bounds__(64, ECCKD_SW_WAVES_PER_SIMD) rte_sw_mcica_bands_kernel(const RteSwArgs a) {
  rte_sw_body<double, CW, true, CLAMP, true, true, true, true>(a);
}

// the single-precision all-sky forms (ecckd_sw_fluxes_allsky_f32 / _mcica_f32), each under its own name: the body forms ssa
// and g in `real`, with the floor 3 * tiny(1._sp) of ecckd_increment_f32 (op_eps<float>) and the single-precision k floor
template <int CW, bool CLAMP>
__global__ void __launch_bounds__(64, ECCKD_SW_WAVES_PER_SIMD) rte_sw_allsky_f32_kernel(const RteSwArgs a) {
  rte_sw_body<float, CW, true, CLAMP, true, true>(a);
}
template <int CW, bool CLAMP>
__global__ void __launch_bounds__(64, ECCKD_SW_WAVES_PER_SIMD) rte_sw_mcica_f32_kernel(const RteSwArgs a) {
  rte_sw_body<float, CW, true, CLAMP, true, true, true>(a);
}

// Sums the per-group partial fluxes of the tail tiles in group order: the order in which a whole-tile wave adds the
// same values to accumulators that start at +0, hence the same bits (see rte_lw_tail_reduce, kernels_rte_lw.hip).
template <typename real>
__global__ void __launch_bounds__(256) rte_sw_tail_reduce(const double *partials, int ngroups, int nlev, int cw, long tail_first,
                                                          long ntail, int ncol, long lev0, long lstep, real *flux_up,
                                                          real *flux_dn, real *flux_dir) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= ntail * nlev * cw) return;
  const int cl = (int)(idx % cw), s = (int)((idx / cw) % nlev);
  const long t = idx / ((long)cw * nlev);
  const long col = (tail_first + t) * cw + cl;
  if (col >= ncol) return;
  const double *p = partials + (t * ngroups * 3 * nlev + s) * cw + cl;
  double up = 0., dn = 0., dir = 0.;
  for (int gi = 0; gi < ngroups; ++gi, p += 3L * nlev * cw) {
    up += p[0];
    dn += p[(long)nlev * cw];
    dir += p[2L * nlev * cw];
  }
  const long q = col + (long)ncol * (lev0 + lstep * s);
  flux_up[q] = (real)up;
  flux_dn[q] = (real)dn;
  if (flux_dir) flux_dir[q] = (real)dir;
}

template <typename real>
__global__ void toa_src_kernel(const real *solar, int ncol, int ng, real *toa) {
  const long n = (long)ncol * ng;
  for (long q = (long)blockIdx.x * blockDim.x + threadIdx.x; q < n; q += (long)gridDim.x * blockDim.x)
    toa[q] = solar[q / ncol];   // src/gas_optics_ecckd.f90:468-472
}

template <typename real>
__global__ void sum_planes_kernel(const real *planes, int nplanes, size_t n, real *out) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    real acc = 0;
    for (int b = 0; b < nplanes; ++b) acc += planes[(size_t)b * n + i];
    out[i] = acc;
  }
}

}  // namespace

size_t rte_sw_scratch_bytes(int ncol, int nlay, int ng) {
  (void)ng;
  long tiles = ((long)ncol + ECCKD_SW_CW - 1) / ECCKD_SW_CW;
  if (tiles > kSwWaves) tiles = kSwWaves;
  return sizeof(double) * (size_t)(2L * (nlay + 1)) * 64 * (size_t)tiles;
}

namespace {
size_t sw_ring_bytes(int nlay, long blocks) {
  return sizeof(double) * (size_t)(2L * (nlay + 1)) * 64 * (size_t)blocks;
}
}  // namespace

// Tail split of rte_sw, as rte_lw_tail_plan (kernels_rte_lw.hip): the grid is persistent (kSwWaves blocks, three per
// SIMD); the tiles of a call that does not fill one round are handed out one g-point group per wave.  Returns the bytes the split
// needs in all -- the scratch ring of the (possibly larger) grid, then the partial sums at offset *partials_at -- or 0.
size_t rte_sw_tail_plan(const RteSwArgs &a, long *tail_first, size_t *partials_at) {
  constexpr double kTailGain = 0.03;
  constexpr size_t kTailMaxBytes = (size_t)64 << 20;
  *tail_first = -1;
  *partials_at = 0;
  if (a.ncol <= 0) return 0;
  constexpr int CW = ECCKD_SW_CW, GW = 64 / CW;
  const long ngroups = (a.ng + GW - 1) / GW;
  const long tiles = ((long)a.ncol + CW - 1) / CW, full = tiles / kSwWaves * kSwWaves, ntail = tiles - full;
  if (ntail == 0 || ngroups < 2) return 0;
  // Only calls of less than one round: with three waves per SIMD a part-empty last round costs next to nothing (the
  // waves left on a SIMD run faster: 100 000 columns 3.36 against 3.39 ms with and without the split, 50 000 columns
  // 1.85 against 1.81), while a small call gains the factor the groups run side by side (1 000 columns: 0.43 -> 0.08 ms).
  if (full > 0) return 0;
  const double before = (double)(full / kSwWaves + 1);
  const double after = (double)(full / kSwWaves) + (double)((ntail * ngroups + kSwWaves - 1) / kSwWaves) / (double)ngroups;
  if (before - after < kTailGain * before) return 0;
  const size_t part = sizeof(double) * 3 * (size_t)(a.nlay + 1) * CW * (size_t)(ntail * ngroups);
  if (part > kTailMaxBytes) return 0;
  long blocks = full + ntail * ngroups;
  if (blocks > kSwWaves) blocks = kSwWaves;
  *tail_first = full;
  *partials_at = (sw_ring_bytes(a.nlay, blocks) + 255) & ~(size_t)255;
  return *partials_at + part;
}

namespace {
// The instantiations a call can take: fp64 in both arithmetic modes through the 3-parameter kernel; single precision in
// both modes; the fused form (DERIVE) in the fast mode only (ecckd_sw_fluxes refuses reference-order arithmetic).
typedef void (*RteSwKernel)(const RteSwArgs);
template <typename real, bool DERIVE>
RteSwKernel rte_sw_kernel_for(const RteSwArgs &a) {
  constexpr int CW = ECCKD_SW_CW;
  if constexpr (std::is_same<real, double>::value && !DERIVE)
    return a.dir_clamp ? (a.exact_division ? rte_sw_kernel<CW, false, true> : rte_sw_kernel<CW, true, true>)
                       : (a.exact_division ? rte_sw_kernel<CW, false, false> : rte_sw_kernel<CW, true, false>);
  else if constexpr (DERIVE)
    return a.exact_division ? nullptr
                            : (a.dir_clamp ? rte_sw_kernel<real, CW, true, true, true> : rte_sw_kernel<real, CW, true, false, true>);
  else
    return a.dir_clamp ? (a.exact_division ? rte_sw_kernel<real, CW, false, true, false> : rte_sw_kernel<real, CW, true, true, false>)
                       : (a.exact_division ? rte_sw_kernel<real, CW, false, false, false> : rte_sw_kernel<real, CW, true, false, false>);
}
}  // namespace

hipError_t launch_rte_sw(const RteSwArgs &a, hipStream_t s) {
  if (a.ncol <= 0) return hipSuccess;
  constexpr int CW = ECCKD_SW_CW;
  // (the all-sky form exists in the fast arithmetic mode only; ecckd_sw_fluxes_allsky refuses the rest with a message)
  if (a.allsky && (a.exact_division || !a.derive)) return hipErrorInvalidValue;
  if (a.allsky && a.part_mask && a.mask_window != 2 && (a.mask_window ? a.mask_first < 0 || a.mask_first + a.ng > 64 || a.f32 : a.ng > 64))
    return hipErrorInvalidValue;
  const bool scaled = a.mask_window == 2;   // (part_scaling in part_mask's storage)
  if (scaled && (!a.allsky || !a.part_scaling || a.f32)) return hipErrorInvalidValue;
  auto k = scaled ? (a.dir_clamp ? rte_sw_scaled_kernel<CW, true> : rte_sw_scaled_kernel<CW, false>)
           : a.allsky && a.part_mask && a.mask_window
               ? (a.dir_clamp ? rte_sw_mcica_bands_kernel<CW, true> : rte_sw_mcica_bands_kernel<CW, false>)
           : a.allsky && a.f32 ? (a.part_mask ? (a.dir_clamp ? rte_sw_mcica_f32_kernel<CW, true> : rte_sw_mcica_f32_kernel<CW, false>)
                                            : (a.dir_clamp ? rte_sw_allsky_f32_kernel<CW, true> : rte_sw_allsky_f32_kernel<CW, false>))
           : a.allsky && a.part_mask ? (a.dir_clamp ? rte_sw_mcica_kernel<CW, true> : rte_sw_mcica_kernel<CW, false>)
           : a.allsky ? (a.dir_clamp ? rte_sw_allsky_kernel<CW, true> : rte_sw_allsky_kernel<CW, false>)
           : a.f32 ? (a.derive ? rte_sw_kernel_for<float, true>(a) : rte_sw_kernel_for<float, false>(a))
                 : (a.derive ? rte_sw_kernel_for<double, true>(a) : rte_sw_kernel_for<double, false>(a));
  if (!k) return hipErrorInvalidValue;
  const size_t lds = sizeof(double) * 3 * (size_t)(a.nlay + 1) * CW;
  if (lds > (size_t)kLdsBudget) return hipErrorInvalidValue;
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(k),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  const long tiles = ((long)a.ncol + CW - 1) / CW;
  const long ntail = a.tail_first >= 0 ? tiles - a.tail_first : 0;
  const int ngroups = (a.ng + 64 / CW - 1) / (64 / CW);
  long blocks = tiles - ntail + ntail * ngroups;
  if (blocks > kSwWaves) blocks = kSwWaves;
  hipLaunchKernelGGL(k, dim3((unsigned)blocks), dim3(64), lds, s, a);
  e = hipGetLastError();
  if (e != hipSuccess || ntail == 0) return e;
  return launch_rte_sw_tail_reduce(a, ngroups, CW, a.tail_first, ntail, s);
}

hipError_t launch_rte_sw_tail_reduce(const RteSwArgs &a, int nchunks, int cw, long tail_first, long ntail, hipStream_t s) {
  const int nlev = a.nlay + 1;
  const long n = ntail * nlev * cw;
  if (n <= 0) return hipSuccess;
  const long lev0 = a.top_at_1 ? 0 : a.nlay, lstep = a.top_at_1 ? 1 : -1;
  if (a.f32)
    hipLaunchKernelGGL(rte_sw_tail_reduce<float>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a.partials, nchunks, nlev, cw,
                       tail_first, ntail, a.ncol, lev0, lstep, reinterpret_cast<float *>(a.flux_up),
                       reinterpret_cast<float *>(a.flux_dn), reinterpret_cast<float *>(a.flux_dir));
  else
    hipLaunchKernelGGL(rte_sw_tail_reduce<double>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a.partials, nchunks, nlev, cw,
                       tail_first, ntail, a.ncol, lev0, lstep, a.flux_up, a.flux_dn, a.flux_dir);
  return hipGetLastError();
}

hipError_t launch_toa_src(const double *solar, int ncol, int ng, double *toa_src, int f32, hipStream_t s) {
  const long n = (long)ncol * ng;
  if (n <= 0) return hipSuccess;
  long blocks = (n + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  if (f32)
    hipLaunchKernelGGL(toa_src_kernel<float>, dim3((unsigned)blocks), dim3(256), 0, s, reinterpret_cast<const float *>(solar), ncol, ng,
                       reinterpret_cast<float *>(toa_src));
  else
    hipLaunchKernelGGL(toa_src_kernel<double>, dim3((unsigned)blocks), dim3(256), 0, s, solar, ncol, ng, toa_src);
  return hipGetLastError();
}

hipError_t launch_sum_planes(const double *planes, int nplanes, size_t n, double *out, int f32, hipStream_t s) {
  if (n == 0) return hipSuccess;
  size_t blocks = (n + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  if (f32)
    hipLaunchKernelGGL(sum_planes_kernel<float>, dim3((unsigned)blocks), dim3(256), 0, s,
                       reinterpret_cast<const float *>(planes), nplanes, n, reinterpret_cast<float *>(out));
  else
    hipLaunchKernelGGL(sum_planes_kernel<double>, dim3((unsigned)blocks), dim3(256), 0, s, planes, nplanes, n, out);
  return hipGetLastError();
}

}  // namespace ecckd
