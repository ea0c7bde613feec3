// kernels_rte_lw_split.hip -- longwave no-scattering solver, layer-split form: the NW waves of a group share one tile of
// (CW columns x 64/CW g-points) and each walks a SEGMENT of SEG = nlay/NW layers.
//
// Algorithm.  The register-resident solver of kernels_rte_lw.hip keeps trans(l) and source_up(l) of all 60 layers in
// registers (one wave per SIMD) and is bound by its own fp64 issue cadence, not by HBM (tools/ubench.hip: 0.40
// wave-instructions/clk/CU at 4 waves per CU against 0.74-0.81 at 12-16).  The layer recurrences are AFFINE,
//     I_dn(l+1) = t(l) I_dn(l) + s_dn(l),      I_up(l) = t(l) I_up(l+1) + s_up(l),
// so a segment of layers composes into (T, D, U) with  I_out = T I_in + D  and  U_out = T U_in + U.
//   phase 1: each wave does the expensive part (exp, the source functions: lw_layer.hpp) for its own SEG layers, keeps
//            t, s_dn, s_up of each in registers and composes (T, D, U);
//   exchange: the NW composites go through LDS, one block barrier per iteration (a g-point group at one angle);
//   phase 2: every wave folds the composites of the waves above into the intensity that enters its segment from above, and
//            -- behind the surface -- those of the waves below into the one that enters from below, then finishes its SEG
//            levels of both sweeps out of registers into the tile's accumulator planes in LDS ([level][column]).
// Same arithmetic per cell as lw_solver_noscat; the intensities entering a segment are composed in a different association
// than a top-to-bottom walk would (relative 1e-16).  A block walks tiles by grid stride; every group of a block walks the
// same number of tiles (block barriers inside): a group whose tile lies beyond the end computes on clamped columns and
// stores nothing.
//
// Forms.  One body, rte_lw_split_body<F>, described by a SplitForm F; SplitLds<F> is its LDS layout.  Per group: two
// accumulator planes and the exchange per sky (43.5 KB at 60 layers), + a third plane with a Jacobian (15.6 KB); behind the
// groups the Planck table of the recomputing forms (ntp rows of an odd number of doubles).
//
//   kernel (rte_lw_split_...)   public call                                      groups x skies in LDS, table, J plane   waves/SIMD
//   _kernel, PLANCK = false     ecckd_rte_lw with "lw_solver" = 1                1 x 1                                   3
//   _kernel, PLANCK = true      ecckd_lw_fluxes                                  2 x 1 + table                           2
//   _allsky_kernel              ecckd_lw_fluxes_allsky                           2 x 1 + table                           2
//   _mcica_kernel               ecckd_lw_fluxes_allsky_mcica                     2 x 1 + table                           2
//   _both_kernel                ecckd_lw_fluxes_clear_allsky, "lw_both_skies" 1  1 x 2 + table                           1
//   _jac_kernel                 ecckd_lw_fluxes_jac, "lw_jac_inline" = 1         1 x 1 + J + table                       1
//   _rescaled_kernel            ecckd_rte_lw_rescaled                            1 x 1                                   2
//   _rescaled_allsky_kernel     ecckd_lw_fluxes_allsky_rescaled                  1 x 1 + table                           1
//   _rescaled_jac_kernel        ecckd_lw_fluxes_rescaled_jac, "lw_jac_inline" 1  1 x 1 + J + table                       1
//
// PLANCK ("fused longwave"): the three source arrays are not read from HBM but recomputed from
// tlay / tlev and the Planck table (src/gas_optics_ecckd.f90:245-289, :407-424), so gas optics only has to write tau: 16
// instead of 64 B/cell between the two kernels.  Two groups per block share one copy of the table in LDS: read from global
// memory instead, the two dependent table loads per source leave the kernel latency-bound at its two waves per SIMD
// (measured 21 ms per 1e6 columns against 11 from LDS).
// SKY = 1 / 2 (PLANCK forms): the particles of the layer on the model's bands, a.part_tau (ncol,nlay,nband), join the gas
// optical depth in front of tl = tau * D (lw_cell_tau of lw_layer.hpp).  The two g-points of a wave may sit in different
// bands, so the band offset is per lane; the band values ride in prefetch slots next to the gas optical depth (one load per
// (layer, iteration) from planes that stay in L2).  MASK: a.part_mask holds one 64-bit word per (column, layer); the lane's
// g-point is fixed for an iteration, so a prefetch slot carries only the 32-bit half of the word that holds it.
// BOTH: the clear sky (the gas optical depth as it is read) and the all sky of a tile in one pass.  The three Planck
// sources of a cell and the surface source are evaluated once; everything that hangs on the optical depth -- a SplitSky --
// exists twice.  The second sky takes the LDS of the second group and the block's four waves sit one per SIMD.
// JAC (PLANCK forms): the surface-temperature Jacobian of flux_up next to the fluxes.  Its surface term
// eps * (B(tsfc + 1) - B(tsfc)) is folded through the exchanged T of the waves below and carried through the up sweep with
// the T[s] the sweep holds in registers: one multiply and one accumulator add per (cell, angle).
// RESC: the rescaled no-scattering solver (include/ecckd_hip.h, "Rescaled longwave").  The cell has (tau, ssa, g) -- read
// from a.tau / a.ssa / a.g, or formed from the gas optical depth and the band triple (lw_cell_rescaled of lw_layer.hpp) --
// and phase 1 keeps five values per layer: t, sdn, CA = Cn*(1 - t*t), SUA = sup - Cn*(sdn*t + sup) (in SU[]) and
// SDA = sdn - Cn*(sup*t + sdn).  The three sweeps are three affine recurrences whose sources are known once the sweep before
// is finished, so phase 2 has three exchanges:
//   1. (T, D) as above gives dn0 entering the segment; the wave walks dn0 through its layers, SU[s] += CA[s]*dn0[s], and
//      composes U of the adjusted up sweep;
//   2. (T, U): the adjusted up sweep, accumulated per level, SDA[s] += CA[s]*up[s+1], and D of the adjusted down sweep (into
//      the slot of the first exchange's D, which every wave has read before the second barrier);
//   3. (T, D): the adjusted down sweep, accumulated per level.
// RESC with JAC: with every source zero dn0 == 0 and the adjusted up sweep reduces to up[s] = t * up[s+1], so the Jacobian
// is the JAC form's, carried through the adjusted up sweep behind the second exchange.
// Both rescaled forms walk 15 layers per wave with 4 waves per block and 32 columns per tile: the fused call equals the
// composed one bit for bit only if both compose their segments alike ("lw_split_seg" does not act here).
//
// Bit for bit.  Every form evaluates a sky's cells with the same helpers and feeds a level's accumulator its g-points in the
// same order, so: each sky of BOTH gives the fluxes of the single-sky kernels; the fluxes of a JAC form are those of the form
// without it; SHARED (the level sources of neighbouring layers are one value, read once) gives the fluxes of the generic
// array form; the fused rescaled call gives those of the composed route.
#include <cstdlib>
#include <type_traits>

#include "kernels.hpp"
#include "lw_layer.hpp"
#include "planck_at.hpp"

namespace ecckd {
namespace {

#ifndef ECCKD_SPLIT_SEG
#define ECCKD_SPLIT_SEG 10   // layers per wave; 60 / SEG waves per block
#endif
#ifndef ECCKD_SPLIT_PF
#define ECCKD_SPLIT_PF 2
#endif
#ifndef ECCKD_SPLIT_WAVES_PER_SIMD
#define ECCKD_SPLIT_WAVES_PER_SIMD 3
#endif
#ifndef ECCKD_SPLIT_PF_PLANCK
#define ECCKD_SPLIT_PF_PLANCK 2
#endif

__host__ __device__ constexpr int planck_stride(int ng) { return ng | 1; }   // odd number of doubles per row

// One form of the kernel.  SEG layers per wave, NW waves per group, CW columns per tile; SHARED: one value per level source;
// SER3: three-term series; PLANCK: sources recomputed; SKY: 0 gas only, 1 / 2 one- / two-stream particles; MASK: McICA mask;
// BOTH: clear and all sky; JAC: flux_up_jac; RESC: the rescaled solver; WPS: waves per SIMD the kernel is compiled for.
template <int SEG_, int NW_, int CW_, bool SHARED_, bool SER3_, bool PLANCK_, int SKY_, bool MASK_, bool BOTH_, bool JAC_, bool RESC_,
          int WPS_, bool WIN_ = false>
struct SplitForm {
  static constexpr int SEG = SEG_, NW = NW_, CW = CW_, SKY = SKY_, WPS = WPS_;
  static constexpr bool SHARED = SHARED_, SER3 = SER3_, PLANCK = PLANCK_, MASK = MASK_, BOTH = BOTH_, JAC = JAC_, RESC = RESC_;
  static constexpr bool WIN = WIN_;                                     // band windows: blockIdx.y is the band (BandsForm)
  static constexpr int NL = SEG * NW;                                   // layers
  static constexpr int GW = 64 / CW;                                    // g-points per wave
  static constexpr int NSKY = BOTH ? 2 : 1;                             // skies per group: [0] the call's own, [1] the clear sky
  static constexpr int NG = (BOTH || JAC || RESC) ? 1 : PLANCK ? 2 : 1; // tile groups per block
  static constexpr int THREADS = 64 * NW * NG;
  // layers in flight per lane (RESC on arrays: six arrays in flight per layer, no room for a second layer)
  static constexpr int PF = (RESC && !PLANCK) ? 1 : PLANCK ? ECCKD_SPLIT_PF_PLANCK : ECCKD_SPLIT_PF;
  // Schedule, not arithmetic: whether the up fold reads every composite ahead of its first multiply, and whether the down
  // sweep goes ahead of the up fold.  Either way the same operations in the same association; the compiler's schedule of
  // phase 2 follows the order of the statements, and these are the orders at which each family keeps the time it had with
  // phase 2 written out per form (profiles/README.md, lw_split_refactor).
  static constexpr bool UP_READS_AHEAD = !RESC, DOWN_SWEEP_FIRST = !BOTH;
  static_assert(SKY == 0 || PLANCK, "the all-sky form extends the Planck-recomputing solver");
  static_assert(SKY != 0 || !MASK, "a cloud mask belongs to the all-sky form");
  static_assert(SKY != 0 || !BOTH, "the dual-sky form extends the all-sky form");
  static_assert(!JAC || (PLANCK && !BOTH), "the Jacobian form extends the single-sky Planck-recomputing solver");
  static_assert(!RESC || (!SHARED && !BOTH && (!JAC || PLANCK) && (PLANCK ? SKY == 2 : SKY == 0)),
                "the rescaled form reads arrays, or recomputes Planck sources and takes a two-stream band triple");
  static_assert(!SHARED || !PLANCK, "shared level sources are a property of the array form");
  static_assert(!WIN || (PLANCK && !BOTH && !JAC && !RESC), "band windows extend the single-sky Planck-recomputing forms");
};

// The forms by the template parameters of their kernels
template <int SEG, int NW, int CW, bool SHARED, bool SER3, bool PLANCK, int WPS>
using ClearForm = SplitForm<SEG, NW, CW, SHARED, SER3, PLANCK, 0, false, false, false, false, WPS>;
template <int SEG, int NW, int CW, bool SER3, bool TWOSTR, bool MASK, int WPS>
using AllskyForm = SplitForm<SEG, NW, CW, false, SER3, true, TWOSTR ? 2 : 1, MASK, false, false, false, WPS>;
template <int SEG, int NW, int CW, bool SER3, bool TWOSTR, bool MASK>
using BothForm = SplitForm<SEG, NW, CW, false, SER3, true, TWOSTR ? 2 : 1, MASK, true, false, false, 1>;
template <int SEG, int NW, int CW, bool SER3, int SKY, bool MASK>
using JacForm = SplitForm<SEG, NW, CW, false, SER3, true, SKY, MASK, false, true, false, 1>;
template <int SEG, int NW, int CW, bool SER3, int WPS>
using RescaledForm = SplitForm<SEG, NW, CW, false, SER3, false, 0, false, false, false, true, WPS>;
template <int SEG, int NW, int CW, bool SER3, bool MASK, bool JAC, int WPS>
using RescaledAllskyForm = SplitForm<SEG, NW, CW, false, SER3, true, 2, MASK, false, JAC, true, WPS>;
// the band-window form of the clear-sky (SKY = 0), all-sky and McICA kernels (ecckd_lw_flux_bands)
template <int SEG, int NW, int CW, bool SER3, int SKY, bool MASK, int WPS>
using BandsForm = SplitForm<SEG, NW, CW, false, SER3, true, SKY, MASK, false, false, false, WPS, true>;

// LDS of a block, in doubles: per group and sky two accumulator planes [NL+1][CW] and the exchange [2][NW][3][64], behind
// the skies of a group the Jacobian's plane, behind the groups the Planck table [ntp][planck_stride(ng)]
template <class F>
struct SplitLds {
  static constexpr int kPlane = (F::NL + 1) * F::CW;
  static constexpr int kExchange = F::NW * 3 * 64;   // one of the two that alternate
  static constexpr int kSky = 2 * kPlane + 2 * kExchange;
  static constexpr int kGroup = F::NSKY * kSky + (F::JAC ? kPlane : 0);
  // offsets inside a group
  static constexpr int acc_dn(int sky) { return sky * kSky; }
  static constexpr int acc_up(int sky) { return acc_dn(sky) + kPlane; }
  static constexpr int exchange(int sky) { return acc_up(sky) + kPlane; }
  static constexpr int kAccJac = F::NSKY * kSky;
  static constexpr int kTable = F::NG * kGroup;
  static constexpr size_t bytes(int ntp, int ng) {
    return sizeof(double) * ((size_t)kTable + (F::PLANCK ? (size_t)ntp * planck_stride(ng) : 0));
  }
};

template <int CW>
__device__ __forceinline__ double gsum(double v) {
#pragma unroll
  for (int o = CW; o < 64; o <<= 1) v = v + __shfl_xor(v, o);
  return v;
}

// acc += v by the owner lane (the others add +0.0): one fire-and-forget ds_add_f64 (see kernels_rte_lw.hip)
__device__ __forceinline__ void acc_add(double *p, double v, bool owner) {
  __hip_atomic_fetch_add(p, owner ? v : 0., __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// N prefetch slots of an input that the form reads; nothing where it does not
template <class T, bool HAS, int N> struct Slots { T v[N]; };
template <class T, int N> struct Slots<T, false, N> {};

// What a lane is in its group during one iteration
struct SplitLane {
  int lane, cl, w, s0;   // lane of the wave, column of the tile, wave of the group, its first layer in walking order
  bool owner;            // the lane that adds its column's g-point sum to the accumulators
  double wfac;           // 2 pi w_k, or 0 on a lane beyond the last g-point
};

// What hangs on the optical depth of one sky: the wave's layers, its composites, the sky's exchange slot and planes
template <class F>
struct SplitSky {
  double T[F::SEG], SDN[F::SEG], SU[F::SEG];
  double Tq = 1., Dq = 0.;
  double *acc_dn, *acc_up, *x;

  // layer s of the segment from its slant optical depth and sources
  __device__ __forceinline__ void layer(int s, double tl, double tau_thresh, double lay, double bdn, double bup) {
    lw_layer_source<F::SER3>(tl, tau_thresh, lay, bdn, bup, T[s], SDN[s], SU[s]);
  }
  __device__ __forceinline__ void compose_down(int s) {
    Dq = T[s] * Dq + SDN[s];
    Tq = Tq * T[s];
  }
  __device__ __forceinline__ double compose_up() const {
    double Uq = 0.;
#pragma unroll
    for (int s = F::SEG - 1; s >= 0; --s) Uq = T[s] * Uq + SU[s];
    return Uq;
  }
};

// Fold the exchanged (T, D) of the waves from the top down: returns what leaves the last segment, Iin what enters segment w
template <int NW>
__device__ __forceinline__ double fold_down(const double *x, const SplitLane &L, double I, double &Iin) {
  double t[NW], d[NW];   // (all reads first: their LDS latencies overlap)
#pragma unroll
  for (int q = 0; q < NW; ++q) {
    t[q] = x[(q * 3 + 0) * 64 + L.lane];
    d[q] = x[(q * 3 + 1) * 64 + L.lane];
  }
  Iin = I;
#pragma unroll
  for (int q = 0; q < NW; ++q) {
    if (q == L.w) Iin = I;
    I = t[q] * I + d[q];
  }
  return I;
}
// ... and (T, U) from the surface up.  AHEAD: all reads first, else each where the fold uses it (SplitForm::UP_READS_AHEAD)
template <int NW, bool AHEAD>
__device__ __forceinline__ double fold_up(const double *x, const SplitLane &L, double U, double &Uin) {
  double t[NW], u[NW];
  if constexpr (AHEAD) {
#pragma unroll
    for (int q = 0; q < NW; ++q) {
      t[q] = x[(q * 3 + 0) * 64 + L.lane];
      u[q] = x[(q * 3 + 2) * 64 + L.lane];
    }
  }
  Uin = U;
#pragma unroll
  for (int q = NW - 1; q >= 0; --q) {
    if constexpr (!AHEAD) {
      t[q] = x[(q * 3 + 0) * 64 + L.lane];
      u[q] = x[(q * 3 + 2) * 64 + L.lane];
    }
    if (q == L.w) Uin = U;
    U = t[q] * U + u[q];
  }
  return U;
}
// ... and the Jacobian's surface term through the T of the waves below: what enters segment w from below
template <int NW>
__device__ __forceinline__ double fold_jac(const double *x, const SplitLane &L, double Jq) {
  double J = Jq;
#pragma unroll
  for (int q = NW - 1; q >= 0; --q) {
    if (q == L.w) J = Jq;
    Jq = x[(q * 3 + 0) * 64 + L.lane] * Jq;
  }
  return J;
}

// Down sweep of the segment, I <- T[s] I + S[s].  ACC: into the plane's levels s0 .. s0+SEG-1 (the level above each layer);
// the last wave adds the surface.  ADJ (RESC): the radiance entering a layer from above adjusts A[s] by CA[s].
template <class F, bool ACC, bool ADJ>
__device__ __forceinline__ void sweep_down(const SplitLane &L, const double *T, const double *S, double I, double *acc,
                                           const double *CA = nullptr, double *A = nullptr) {
#pragma unroll
  for (int s = 0; s < F::SEG; ++s) {
    if constexpr (ACC) acc_add(&acc[(L.s0 + s) * F::CW + L.cl], gsum<F::CW>(L.wfac * I), L.owner);
    if constexpr (ADJ) A[s] = A[s] + CA[s] * I;
    I = T[s] * I + S[s];
  }
  if constexpr (ACC) {
    if (L.w == F::NW - 1) acc_add(&acc[F::NL * F::CW + L.cl], gsum<F::CW>(L.wfac * I), L.owner);
  }
}
// Up sweep, U <- T[s] U + S[s], into the plane's levels s0+SEG .. s0+1 (the level below each layer); the first wave adds the
// top.  ADJ (RESC): the radiance entering a layer from below adjusts A[s].  JAC: J <- T[s] J rides along into acc_jac.
template <class F, bool ADJ>
__device__ __forceinline__ void sweep_up(const SplitLane &L, const double *T, const double *S, double U, double *acc,
                                         [[maybe_unused]] double J, [[maybe_unused]] double *acc_jac, const double *CA = nullptr,
                                         double *A = nullptr) {
#pragma unroll
  for (int s = F::SEG - 1; s >= 0; --s) {
    acc_add(&acc[(L.s0 + s + 1) * F::CW + L.cl], gsum<F::CW>(L.wfac * U), L.owner);
    if constexpr (ADJ) A[s] = A[s] + CA[s] * U;
    U = T[s] * U + S[s];
    if constexpr (F::JAC) {
      acc_add(&acc_jac[(L.s0 + s + 1) * F::CW + L.cl], gsum<F::CW>(L.wfac * J), L.owner);
      J = T[s] * J;
    }
  }
  if (L.w == 0) acc_add(&acc[L.cl], gsum<F::CW>(L.wfac * U), L.owner);
  if constexpr (F::JAC) {
    if (L.w == 0) acc_add(&acc_jac[L.cl], gsum<F::CW>(L.wfac * J), L.owner);
  }
}

// What a form writes beside a.flux_up / a.flux_dn
struct SplitExtra {
  double *flux_up_clear = nullptr, *flux_dn_clear = nullptr;   // BOTH
  double *flux_up_jac = nullptr;                               // JAC
};

// The g-point windows of the band form (F::WIN; ecckd_lw_flux_bands): band b covers the 0-based g-points
// [first[b], first[b + 1]) of the model.  Block (x, b) of the grid solves band b of its tiles: the g-point groups are formed
// from the band's first g-point, in the order a launch over that band's planes alone forms them, and everything that lives
// on the model's g-points -- the tau plane, the Planck table, inc_flux, the band map, the mask bit -- is indexed by the
// model's g-point.  The fluxes go to plane b of a.flux_up / a.flux_dn, (ncol,nlay+1,nband).
struct BandWindows { unsigned short first[257]; };

template <class F>
__device__ __forceinline__ void rte_lw_split_body(const RteLwArgs &a, const PlanckTab &pt, const double *tlay, const double *tlev,
                                                  const double *tsfc, const SplitExtra &out = SplitExtra{},
                                                  const BandWindows *bw = nullptr) {
  constexpr int SEG = F::SEG, NW = F::NW, CW = F::CW, GW = F::GW, NL = F::NL, NG = F::NG, PF = F::PF, NSKY = F::NSKY;
  constexpr bool SHARED = F::SHARED, PLANCK = F::PLANCK, MASK = F::MASK, JAC = F::JAC, RESC = F::RESC, WIN = F::WIN;
  constexpr int SKY = F::SKY;
  using Lds = SplitLds<F>;
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  double *const lds = reinterpret_cast<double *>(lds_raw);
  const int tid = threadIdx.x, lane = tid & 63;
  const int grp = (tid >> 6) / NW, w = (tid >> 6) % NW, gtid = tid - grp * 64 * NW;
  double *const group = lds + grp * Lds::kGroup;
  double *acc_dn[NSKY], *acc_up[NSKY], *xch[NSKY];
#pragma unroll
  for (int k = 0; k < NSKY; ++k) {
    acc_dn[k] = group + Lds::acc_dn(k);
    acc_up[k] = group + Lds::acc_up(k);
    xch[k] = group + Lds::exchange(k);
  }
  [[maybe_unused]] double *acc_jac = group + Lds::kAccJac;   // (JAC)
  [[maybe_unused]] const int pstride = PLANCK ? planck_stride(a.ng) : 0;
  [[maybe_unused]] double *ptab = lds + Lds::kTable;            // (PLANCK) [ntp][pstride]
  if constexpr (WIN) {   // the window's columns of the table alone, where the whole table has them: staging costs what the band is wide
    const int first = bw->first[blockIdx.y], count = bw->first[blockIdx.y + 1] - first;
    for (int i = tid; i < pt.ntp * count; i += F::THREADS) {
      const int r = i / count, g = first + (i - r * count);
      ptab[r * pstride + g] = pt.tab[r * pt.ng + g];
    }
  } else if constexpr (PLANCK) {
    for (int i = tid; i < pt.ntp * pt.ng; i += F::THREADS) {
      const int r = i / pt.ng, g = i - r * pt.ng;
      ptab[r * pstride + g] = pt.tab[i];
    }
  }
  const int cl = lane % CW, gs = lane / CW;
  // WIN: the block's window [g0, g0 + ng) of the model's g-points and its plane of the outputs; else all of them, plane 0
  int win_first = 0, win_count = 0;
  long win_plane = 0;
  if constexpr (WIN) {
    win_first = bw->first[blockIdx.y];
    win_count = bw->first[blockIdx.y + 1] - win_first;
    win_plane = (long)blockIdx.y * a.ncol * (NL + 1);
  }
  // (a.ng is read here, where the forms without windows always read it: their register figures depend on it)
  const int ncol = a.ncol, ng = WIN ? win_count : a.ng, g0 = win_first;
  const double pi = acos(-1.);
  const double pi_f32 = (double)3.14159265359f, rpi_f32 = 1. / pi_f32;   // src/gas_optics_ecckd.f90:53 (PLANCK)
  const double tau_thresh = a.tau_thresh;
  const long lay0 = a.top_at_1 ? 0 : NL - 1, lev0 = a.top_at_1 ? 0 : NL;
  const long lstep = a.top_at_1 ? 1 : -1;
  const double *Bdn = a.top_at_1 ? a.lev_source_inc : a.lev_source_dec;
  const double *Bup = a.top_at_1 ? a.lev_source_dec : a.lev_source_inc;
  const int ngroups = (ng + GW - 1) / GW;
  const int niter = ngroups * a.nmus;
  const long ntiles = ((long)ncol + CW - 1) / CW;
  const int s0 = w * SEG;   // first layer of this wave, in walking order from the top
  // SHARED: the level arrays have a g-plane stride of their own (RteLwArgs::lev_gstride: NL*ncol, or (NL+1)*ncol for the two
  // views of one level buffer); dlev is what it exceeds the layer arrays' by: 0 or ncol
  [[maybe_unused]] const int dlev = SHARED && a.lev_gstride ? (int)((long)a.lev_gstride - (long)ncol * NL) : 0;
  auto planck = [&](double temp, int g) { return planck_at(pt, ptab, pstride, temp, g, pi_f32, rpi_f32); };

#pragma unroll
  for (int k = 0; k < NSKY; ++k)
    for (int i = gtid; i < 2 * Lds::kPlane; i += 64 * NW) acc_dn[k][i] = 0.;
  if constexpr (JAC)
    for (int i = gtid; i < Lds::kPlane; i += 64 * NW) acc_jac[i] = 0.;
  __syncthreads();

  for (long tile0 = (long)blockIdx.x * NG; tile0 < ntiles; tile0 += (long)gridDim.x * NG) {
    const long tile = tile0 + grp;
    const long col = tile * CW + cl;
    const bool valid = col < ncol;
    const long cc = valid ? col : (long)ncol - 1;

    // prefetch slots: the gas optical depth (RESC on arrays: the cell's), and what the form reads beside it
    double ptau[PF];
    Slots<double, !PLANCK, PF> play_, pbdn;            // arrays: lay_source(l), the level source at the far edge of l
    Slots<double, !PLANCK && !SHARED, PF> pbup;        // ... and at the near edge
    Slots<double, PLANCK, PF> ptl, ptv;                // PLANCK: tlay(l), tlev(far edge of l)
    Slots<double, SKY != 0, PF> ppt;                   // SKY: part_tau(l) of the lane's band
    Slots<double, SKY == 2, PF> pps;                   // ... and part_ssa(l)
    Slots<double, RESC && !PLANCK, PF> pss;            // RESC on arrays: ssa(l) of the cell
    Slots<double, RESC, PF> pgg;                       // RESC: g(l) of the cell, or part_g(l) of the lane's band
    Slots<unsigned, MASK, PF> pmk;                     // MASK: the half of part_mask(column, l) that holds the lane's g-point
    [[maybe_unused]] long qb = 0;                      // SKY: offset of the lane's band plane
    [[maybe_unused]] int mhalf = 0, mbit = 0;          // MASK: which half, and the bit inside it
    [[maybe_unused]] const unsigned *mask32 = reinterpret_cast<const unsigned *>(a.part_mask);
    long qn = 0;
    const long qstep = (long)ncol * lstep;
    [[maybe_unused]] long q2 = 0;      // PLANCK: offset into tlay / tlev rows (no g dimension)
    [[maybe_unused]] int glev = 0;     // SHARED: the lane's g-point; its plane of the level arrays lies dlev * glev beyond that of the others
    [[maybe_unused]] double near_first = 0.;   // SHARED / PLANCK: near-edge source (temperature) of the segment's first layer

    auto pair_start = [&](int it) {
      const int g = (it / a.nmus) * GW + gs;
      const int gg = g0 + (g < ng ? g : ng - 1);
      qn = cc + (long)ncol * NL * gg + (long)ncol * (lay0 + lstep * s0);
      asm volatile("" : "+v"(qn));
      if constexpr (PLANCK) {
        q2 = cc + (long)ncol * (lay0 + lstep * s0);
        // level at the near (upper, in walking order) edge of the first layer of the segment
        near_first = tlev[cc + (long)ncol * (lev0 + lstep * s0)];
        if constexpr (SKY != 0) qb = (long)ncol * NL * a.gpt2band[gg];
        if constexpr (MASK) mhalf = gg >> 5;
      } else if constexpr (SHARED) {
        glev = gg;
        asm volatile("" : "+v"(glev));
        near_first = __builtin_nontemporal_load(Bup + (qn + (long)dlev * glev));
      }
    };
    auto issue = [&](int slot) {
      ptau[slot] = __builtin_nontemporal_load(a.tau + qn);
      if constexpr (PLANCK) {
        ptl.v[slot] = tlay[q2];
        ptv.v[slot] = tlev[q2 + (a.top_at_1 ? (long)ncol : 0)];   // far edge of the layer: level index l+1 (top_at_1) or l
        if constexpr (SKY != 0) ppt.v[slot] = a.part_tau[q2 + qb];
        if constexpr (SKY == 2) pps.v[slot] = a.part_ssa[q2 + qb];
        if constexpr (RESC) pgg.v[slot] = a.part_g[q2 + qb];
        if constexpr (MASK) pmk.v[slot] = mask32[2 * q2 + mhalf];
        q2 += qstep;
      } else {
        play_.v[slot] = __builtin_nontemporal_load(a.lay_source + qn);
        if constexpr (SHARED) {
          asm volatile("" : "+v"(glev));   // (the product below is formed here, in the add, and not kept in a register pair)
          pbdn.v[slot] = __builtin_nontemporal_load(Bdn + (qn + (long)dlev * glev));
        } else {
          pbdn.v[slot] = __builtin_nontemporal_load(Bdn + qn);
          pbup.v[slot] = __builtin_nontemporal_load(Bup + qn);
        }
        if constexpr (RESC) {
          pss.v[slot] = __builtin_nontemporal_load(a.ssa + qn);
          pgg.v[slot] = __builtin_nontemporal_load(a.g + qn);
        }
      }
      qn += qstep;
      asm volatile("" : "+v"(qn));
    };

    pair_start(0);
#pragma unroll
    for (int s = 0; s < PF; ++s) issue(s);

    for (int it = 0; it < niter; ++it) {
      const int gi = it / a.nmus, k = it - gi * a.nmus;
      const int g = gi * GW + gs;
      const bool gact = g < ng;
      const int gg = g0 + (gact ? g : ng - 1);
      const double D = a.Ds[k];
      if constexpr (MASK) mbit = gg & 31;   // (pair_start(it + 1), below, moves mhalf on while this iteration's slots are used up)
      const SplitLane L{lane, cl, w, s0, gs == 0, gact ? 2. * pi * a.wts[k] : 0.};

      // ---------------- phase 1: this wave's SEG layers ----------------
      SplitSky<F> sky[NSKY];
#pragma unroll
      for (int n = 0; n < NSKY; ++n) {
        sky[n].acc_dn = acc_dn[n];
        sky[n].acc_up = acc_up[n];
        sky[n].x = xch[n] + (it & 1) * Lds::kExchange;
      }
      SplitSky<F> &own = sky[0];
      Slots<double, RESC, SEG> CA, SDA;   // RESC: Cn*(1 - t*t), and the adjusted down source
      [[maybe_unused]] double carry = PLANCK ? planck(near_first, gg) : near_first;
#pragma unroll
      for (int s = 0; s < SEG; ++s) {
        const int u = s % PF;
        const double tau_gas = ptau[u];
        double tau = tau_gas;
        [[maybe_unused]] bool cloudy = true;
        if constexpr (MASK) cloudy = (pmk.v[u] >> mbit) & 1u;
        [[maybe_unused]] double Cn = 0.;
        if constexpr (RESC && PLANCK) lw_cell_rescaled<true>(tau_gas, ppt.v[u], pps.v[u], pgg.v[u], cloudy, tau, Cn);
        else if constexpr (RESC) lw_cell_rescaled<false>(tau_gas, 0., pss.v[u], pgg.v[u], true, tau, Cn);
        else if constexpr (SKY == 2) tau = lw_cell_tau<2>(tau_gas, ppt.v[u], pps.v[u], cloudy);
        else if constexpr (SKY == 1) tau = lw_cell_tau<1>(tau_gas, ppt.v[u], 0., cloudy);
        double lay, bdn, bup;
        if constexpr (PLANCK) {
          lay = planck(ptl.v[u], gg);
          bdn = planck(ptv.v[u], gg);
          bup = carry;
        } else {
          lay = play_.v[u];
          bdn = pbdn.v[u];
          if constexpr (SHARED) bup = carry;
          else bup = pbup.v[u];
        }
        if (s + PF < SEG) {
          asm volatile("" : "+v"(qn), "+v"(own.Dq));   // keep the loads of layer s+PF below layer s-1
          issue(u);
        }
        own.layer(s, tau * D, tau_thresh, lay, bdn, bup);
        if constexpr (RESC) {
          const double t = own.T[s], sdn = own.SDN[s], su = own.SU[s];
          CA.v[s] = Cn * (1. - t * t);
          own.SU[s] = su - Cn * (sdn * t + su);
          SDA.v[s] = sdn - Cn * (su * t + sdn);
        }
        own.compose_down(s);
        if constexpr (F::BOTH) {   // the same cell under the clear sky: the gas optical depth alone
          sky[1].layer(s, tau_gas * D, tau_thresh, lay, bdn, bup);
          sky[1].compose_down(s);
        }
        if constexpr (SHARED || PLANCK) carry = bdn;
      }
      // the next pair's first layers start streaming now (RESC: the up sweep's sources wait for dn0, behind the first exchange)
      double Uq[NSKY];
      if constexpr (!RESC) {
#pragma unroll
        for (int n = 0; n < NSKY; ++n) Uq[n] = sky[n].compose_up();
      }
      if (it + 1 < niter) {
        pair_start(it + 1);
#pragma unroll
        for (int s = 0; s < PF; ++s) issue(s);
      }
#pragma unroll
      for (int n = 0; n < NSKY; ++n) {
        sky[n].x[(w * 3 + 0) * 64 + lane] = sky[n].Tq;
        sky[n].x[(w * 3 + 1) * 64 + lane] = sky[n].Dq;
        if constexpr (!RESC) sky[n].x[(w * 3 + 2) * 64 + lane] = Uq[n];
      }
      __syncthreads();

      // ---------------- phase 2: boundary intensities of this segment, then the sweeps ----------------
      double Itop = 0.;   // radn_dn(top): no incident diffuse flux, or inc_flux as an intensity (Appendix B.1)
      if (a.inc_flux) {
        const double f = a.inc_flux[cc + (long)ncol * gg];
        Itop = a.inc_isotropic ? f / pi : f / (2. * pi * a.wts[k]);
      }
      double Iin, Uin;
      double Ibot = fold_down<NW>(own.x, L, Itop, Iin);
      const double eps = a.sfc_emis[a.gpt2band[gg] + (long)a.nband * cc];
      const double sfc_src = PLANCK ? planck(tsfc[cc], gg) : a.sfc_source[cc + (long)ncol * gg];
      // JAC: d(intensity) / d(tsfc) entering this segment from below -- the surface term through the T of the waves below
      auto jac_in = [&](const double *x) { return fold_jac<NW>(x, L, eps * (planck(tsfc[cc] + 1., gg) - sfc_src)); };
      if constexpr (RESC) {
        double *x = own.x;
        const double Usfc = Ibot * (1. - eps) + eps * sfc_src;   // the surface has seen the unadjusted dn0
        // 1. dn0 through this segment: the sources of the adjusted up sweep
        sweep_down<F, false, true>(L, own.T, own.SDN, Iin, nullptr, CA.v, own.SU);
        x[(w * 3 + 2) * 64 + lane] = own.compose_up();
        __syncthreads();
        // 2. the adjusted up sweep; the radiance entering a layer from below adjusts its down source
        fold_up<NW, F::UP_READS_AHEAD>(x, L, Usfc, Uin);
        [[maybe_unused]] double J = 0.;
        if constexpr (JAC) J = jac_in(x);   // with all sources zero dn0 == 0 and the adjusted up sweep is J = t * J
        sweep_up<F, true>(L, own.T, own.SU, Uin, own.acc_up, J, acc_jac, CA.v, SDA.v);
        double D3 = 0.;
#pragma unroll
        for (int s = 0; s < SEG; ++s) D3 = own.T[s] * D3 + SDA.v[s];
        x[(w * 3 + 1) * 64 + lane] = D3;   // (every wave read the first exchange's D before the barrier above)
        __syncthreads();
        // 3. the adjusted down sweep
        fold_down<NW>(x, L, Itop, Iin);
        sweep_down<F, true, false>(L, own.T, SDA.v, Iin, own.acc_dn);
      } else {
#pragma unroll
        for (int n = 0; n < NSKY; ++n) {   // (BOTH: once more on the clear sky's composites into the clear sky's planes)
          const SplitSky<F> &S = sky[n];
          if (n > 0) Ibot = fold_down<NW>(S.x, L, Itop, Iin);
          const double Usfc = Ibot * (1. - eps) + eps * sfc_src;   // surface
          if constexpr (F::DOWN_SWEEP_FIRST) sweep_down<F, true, false>(L, S.T, S.SDN, Iin, S.acc_dn);
          fold_up<NW, F::UP_READS_AHEAD>(S.x, L, Usfc, Uin);
          [[maybe_unused]] double J = 0.;
          if constexpr (JAC) J = jac_in(S.x);
          if constexpr (!F::DOWN_SWEEP_FIRST) sweep_down<F, true, false>(L, S.T, S.SDN, Iin, S.acc_dn);
          sweep_up<F, false>(L, S.T, S.SU, Uin, S.acc_up, J, acc_jac);
        }
      }
    }

    // broadband fluxes of the tile: level s-th from the top -> lev0 + lstep*s
    __syncthreads();
    for (int i = gtid; i < Lds::kPlane; i += 64 * NW) {
      const int s = i / CW, c = i - s * CW;
      const long cg = tile * CW + c;
      if (cg < ncol) {
        const long q = cg + (long)ncol * (lev0 + lstep * s);
        a.flux_dn[q + win_plane] = acc_dn[0][i];
        a.flux_up[q + win_plane] = acc_up[0][i];
        if constexpr (F::BOTH) {
          out.flux_dn_clear[q] = acc_dn[1][i];
          out.flux_up_clear[q] = acc_up[1][i];
        }
        if constexpr (JAC) out.flux_up_jac[q] = acc_jac[i];
      }
#pragma unroll
      for (int n = 0; n < NSKY; ++n) {
        acc_dn[n][i] = 0.;
        acc_up[n][i] = 0.;
      }
      if constexpr (JAC) acc_jac[i] = 0.;
    }
    __syncthreads();
  }
}

// The kernels: each builds its form from its own parameters.
template <int SEG, int NW, int CW, bool SHARED, bool SER3, bool PLANCK, int WPS>
__global__ void __launch_bounds__((ClearForm<SEG, NW, CW, SHARED, SER3, PLANCK, WPS>::THREADS), WPS)
rte_lw_split_kernel(const RteLwArgs a, const PlanckTab pt, const double *tlay, const double *tlev, const double *tsfc) {
  rte_lw_split_body<ClearForm<SEG, NW, CW, SHARED, SER3, PLANCK, WPS>>(a, pt, tlay, tlev, tsfc);
}

// All-sky form of the Planck-recomputing solver.  TWOSTR: the particles carry part_ssa (absorption optical depth), else
// part_tau is added as it is.
template <int SEG, int NW, int CW, bool SER3, bool TWOSTR, int WPS>
__global__ void __launch_bounds__((AllskyForm<SEG, NW, CW, SER3, TWOSTR, false, WPS>::THREADS), WPS)
rte_lw_split_allsky_kernel(const RteLwArgs a, const PlanckTab pt, const double *tlay, const double *tlev, const double *tsfc) {
  rte_lw_split_body<AllskyForm<SEG, NW, CW, SER3, TWOSTR, false, WPS>>(a, pt, tlay, tlev, tsfc);
}

// ... with a McICA cloud mask (RteLwArgs::part_mask), under its own name
template <int SEG, int NW, int CW, bool SER3, bool TWOSTR, int WPS>
__global__ void __launch_bounds__((AllskyForm<SEG, NW, CW, SER3, TWOSTR, true, WPS>::THREADS), WPS)
rte_lw_split_mcica_kernel(const RteLwArgs a, const PlanckTab pt, const double *tlay, const double *tlev, const double *tsfc) {
  rte_lw_split_body<AllskyForm<SEG, NW, CW, SER3, TWOSTR, true, WPS>>(a, pt, tlay, tlev, tsfc);
}

// The dual-sky form: clear-sky and all-sky fluxes of a tile in one pass
template <int SEG, int NW, int CW, bool SER3, bool TWOSTR, bool MASK>
__global__ void __launch_bounds__((BothForm<SEG, NW, CW, SER3, TWOSTR, MASK>::THREADS), 1)
rte_lw_split_both_kernel(const RteLwArgs a, const PlanckTab pt, const double *tlay, const double *tlev, const double *tsfc,
                         double *flux_up_clear, double *flux_dn_clear) {
  rte_lw_split_body<BothForm<SEG, NW, CW, SER3, TWOSTR, MASK>>(a, pt, tlay, tlev, tsfc, SplitExtra{flux_up_clear, flux_dn_clear, nullptr});
}

// The Jacobian form: the fluxes of the clear-sky (SKY = 0), all-sky or McICA kernel and flux_up_jac from one pass
template <int SEG, int NW, int CW, bool SER3, int SKY, bool MASK>
__global__ void __launch_bounds__((JacForm<SEG, NW, CW, SER3, SKY, MASK>::THREADS), 1)
rte_lw_split_jac_kernel(const RteLwArgs a, const PlanckTab pt, const double *tlay, const double *tlev, const double *tsfc,
                        double *flux_up_jac) {
  rte_lw_split_body<JacForm<SEG, NW, CW, SER3, SKY, MASK>>(a, pt, tlay, tlev, tsfc, SplitExtra{nullptr, nullptr, flux_up_jac});
}

// The rescaled forms: on arrays (tau, ssa, g, three sources) ...
template <int SEG, int NW, int CW, bool SER3, int WPS>
__global__ void __launch_bounds__((RescaledForm<SEG, NW, CW, SER3, WPS>::THREADS), WPS)
rte_lw_split_rescaled_kernel(const RteLwArgs a, const PlanckTab pt) {
  rte_lw_split_body<RescaledForm<SEG, NW, CW, SER3, WPS>>(a, pt, nullptr, nullptr, nullptr);
}
// ... Planck-recomputing with the two-stream band triple (MASK: and a McICA cloud mask) ...
template <int SEG, int NW, int CW, bool SER3, bool MASK, int WPS>
__global__ void __launch_bounds__((RescaledAllskyForm<SEG, NW, CW, SER3, MASK, false, WPS>::THREADS), WPS)
rte_lw_split_rescaled_allsky_kernel(const RteLwArgs a, const PlanckTab pt, const double *tlay, const double *tlev, const double *tsfc) {
  rte_lw_split_body<RescaledAllskyForm<SEG, NW, CW, SER3, MASK, false, WPS>>(a, pt, tlay, tlev, tsfc);
}
// ... and that form with flux_up_jac of the all sky next to the fluxes
template <int SEG, int NW, int CW, bool SER3, bool MASK>
__global__ void __launch_bounds__((RescaledAllskyForm<SEG, NW, CW, SER3, MASK, true, 1>::THREADS), 1)
rte_lw_split_rescaled_jac_kernel(const RteLwArgs a, const PlanckTab pt, const double *tlay, const double *tlev, const double *tsfc,
                                 double *flux_up_jac) {
  rte_lw_split_body<RescaledAllskyForm<SEG, NW, CW, SER3, MASK, true, 1>>(a, pt, tlay, tlev, tsfc, SplitExtra{nullptr, nullptr, flux_up_jac});
}

// The band-window form (ecckd_lw_flux_bands): the clear-sky (SKY = 0), all-sky or McICA kernel on one band of the model per
// block row; one launch writes every band plane
template <int SEG, int NW, int CW, bool SER3, int SKY, bool MASK, int WPS>
__global__ void __launch_bounds__((BandsForm<SEG, NW, CW, SER3, SKY, MASK, WPS>::THREADS), WPS)
rte_lw_split_bands_kernel(const RteLwArgs a, const PlanckTab pt, const double *tlay, const double *tlev, const double *tsfc,
                          const BandWindows bw) {
  rte_lw_split_body<BandsForm<SEG, NW, CW, SER3, SKY, MASK, WPS>>(a, pt, tlay, tlev, tsfc, SplitExtra{}, &bw);
}

// The fused forms walk 15 layers per wave with 4 waves per group and 32 columns per tile.  Planck-recomputing forms with two
// groups per block need 244-249 VGPRs: two waves per SIMD (three spill 25-54 registers).
constexpr int kSeg = 15, kNW = 4, kCW = 32;
constexpr int kPlanckWps = 2;
constexpr int kRescWps = 2;         // arrays: 75 doubles of layer state per lane, two waves per SIMD
constexpr int kRescWpsPlanck = 1;   // Planck-recomputing: one block per CU (its LDS), one wave per SIMD

// The one launch of every form F through its kernel k: LDS from the layout, the budget, the grid.
// Grid cap: four rounds of resident blocks; past it a block walks tiles by grid stride and reloads neither the Planck table
// nor its code.  Of the Planck-recomputing forms one block is resident per CU (its LDS), so 256 * 4 blocks are four rounds;
// the array forms have WPS blocks per CU.  A one-group block carries one tile per iteration where the two-group kernels carry
// two, so at equal block count the longest block runs ceil(tiles / 1024) tiles: 4 against a mean of 3.05 at 1e5 columns (the
// tail is one tile, a quarter of a round), 31 against 30.5 at 1e6.  The timings of DESIGN section 5.5c were taken with this
// cap.
template <class F, class... KArgs, class... Args>
hipError_t launch_form(void (*k)(KArgs...), const RteLwArgs &a, const PlanckTab &pt, hipStream_t s, Args... rest) {
  const size_t lds = SplitLds<F>::bytes(pt.ntp, a.ng);
  if (lds > (size_t)kLdsBudget) return hipErrorInvalidValue;
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  long blocks = (((long)a.ncol + F::CW - 1) / F::CW + F::NG - 1) / F::NG;
  const long cap = F::PLANCK ? 256L * 4 : 256L * F::WPS * 4;
  if (blocks > cap) blocks = cap;
  hipLaunchKernelGGL(k, dim3((unsigned)blocks), dim3(F::THREADS), lds, s, a, pt, rest...);
  return hipGetLastError();
}

// A run-time bool as a compile-time one: f(std::true_type{}) or f(std::false_type{})
template <class Fn>
hipError_t with_bool(bool b, Fn f) {
  return b ? f(std::true_type{}) : f(std::false_type{});
}
// The particles of a call as compile-time constants: f(SKY, MASK) with SKY 0 (none), 1 (one-stream) or 2 (two-stream)
template <class Fn>
hipError_t with_particles(const RteLwArgs &a, Fn f) {
  if (!a.part_tau) return f(std::integral_constant<int, 0>{}, std::false_type{});
  if (a.part_mask && a.ng > 64) return hipErrorInvalidValue;
  const bool two = !(a.part_1scl || !a.part_ssa);
  return with_bool(a.part_mask != nullptr, [&](auto mask) {
    return two ? f(std::integral_constant<int, 2>{}, mask) : f(std::integral_constant<int, 1>{}, mask);
  });
}

const PlanckTab no_table(const RteLwArgs &a) { return PlanckTab{nullptr, 0., 1., 1., 2, a.ng}; }

}  // namespace

// LDS of the Planck-recomputing forms: does the model's Planck table fit next to the accumulators of two groups?  (The
// shipped 32 / 36-g models do; a 64-g table does not.)
bool rte_lw_planck_fits(int ng, int ntp) {
  return SplitLds<ClearForm<kSeg, kNW, kCW, false, false, true, kPlanckWps>>::bytes(ntp, ng) <= (size_t)kLdsBudget;
}
// ... of the rescaled form: next to one group, with or without the Jacobian's plane
bool rte_lw_rescaled_planck_fits(int ng, int ntp, bool jac) {
  const size_t lds = jac ? SplitLds<RescaledAllskyForm<kSeg, kNW, kCW, false, false, true, 1>>::bytes(ntp, ng)
                         : SplitLds<RescaledAllskyForm<kSeg, kNW, kCW, false, false, false, kRescWpsPlanck>>::bytes(ntp, ng);
  return lds <= (size_t)kLdsBudget;
}

bool rte_lw_split_applies(const RteLwArgs &a) {
  return !a.f32 && a.nlay == 60 && a.ncol > 0;
}

hipError_t launch_rte_lw_split(const RteLwArgs &a, hipStream_t s) {
  constexpr int WPS = ECCKD_SPLIT_WAVES_PER_SIMD;
  const PlanckTab none = no_table(a);
  return with_bool(a.series3, [&](auto ser3) {
    return with_bool(a.shared_levels, [&](auto shared) {
      constexpr bool SER3 = decltype(ser3)::value, SHARED = decltype(shared)::value;
      const double *nil = nullptr;
      switch (a.split_seg) {   // layers per wave: 10 (6 waves per block, 157 VGPRs, 12 waves per CU), 12 or 15
        case 15: return launch_form<ClearForm<15, 4, 32, SHARED, SER3, false, WPS>>(rte_lw_split_kernel<15, 4, 32, SHARED, SER3, false, WPS>, a, none, s, nil, nil, nil);
        case 12: return launch_form<ClearForm<12, 5, 32, SHARED, SER3, false, WPS>>(rte_lw_split_kernel<12, 5, 32, SHARED, SER3, false, WPS>, a, none, s, nil, nil, nil);
        default: return launch_form<ClearForm<10, 6, 32, SHARED, SER3, false, WPS>>(rte_lw_split_kernel<10, 6, 32, SHARED, SER3, false, WPS>, a, none, s, nil, nil, nil);
      }
    });
  });
}

hipError_t launch_rte_lw_planck(const RteLwArgs &a, const double *planck, int ntp, double t0, double dt, const double *tlay,
                                const double *tlev, const double *tsfc, hipStream_t s, double *flux_up_clear,
                                double *flux_dn_clear, double *flux_up_jac) {
  if (a.f32 || a.nlay != 60 || a.ncol <= 0) return hipErrorInvalidValue;
  const PlanckTab pt{planck, t0, dt, 1. / dt, ntp, a.ng};
  const bool both = flux_up_clear || flux_dn_clear;
  // the Jacobian form (ecckd_lw_fluxes_jac, "lw_jac_inline" = 1) has no dual-sky kernel; the dual-sky kernel
  // (ecckd_lw_fluxes_clear_allsky, "lw_both_skies" = 1) writes both clear-sky arrays and needs particles
  if (flux_up_jac && both) return hipErrorInvalidValue;
  if (both && (!flux_up_clear || !flux_dn_clear || !a.part_tau)) return hipErrorInvalidValue;
  return with_bool(a.series3, [&](auto ser3) {
    return with_particles(a, [&](auto sky, auto mask) {
      constexpr bool SER3 = decltype(ser3)::value, MASK = decltype(mask)::value;
      constexpr int SKY = decltype(sky)::value;
      if (flux_up_jac)
        return launch_form<JacForm<kSeg, kNW, kCW, SER3, SKY, MASK>>(rte_lw_split_jac_kernel<kSeg, kNW, kCW, SER3, SKY, MASK>, a, pt, s, tlay,
                                                                     tlev, tsfc, flux_up_jac);
      if constexpr (SKY != 0) {
        constexpr bool TWO = SKY == 2;
        if (both)
          return launch_form<BothForm<kSeg, kNW, kCW, SER3, TWO, MASK>>(rte_lw_split_both_kernel<kSeg, kNW, kCW, SER3, TWO, MASK>, a, pt, s,
                                                                        tlay, tlev, tsfc, flux_up_clear, flux_dn_clear);
        if constexpr (MASK)
          return launch_form<AllskyForm<kSeg, kNW, kCW, SER3, TWO, true, kPlanckWps>>(rte_lw_split_mcica_kernel<kSeg, kNW, kCW, SER3, TWO, kPlanckWps>,
                                                                                      a, pt, s, tlay, tlev, tsfc);
        else
          return launch_form<AllskyForm<kSeg, kNW, kCW, SER3, TWO, false, kPlanckWps>>(rte_lw_split_allsky_kernel<kSeg, kNW, kCW, SER3, TWO, kPlanckWps>,
                                                                                       a, pt, s, tlay, tlev, tsfc);
      } else {
        return launch_form<ClearForm<kSeg, kNW, kCW, false, SER3, true, kPlanckWps>>(rte_lw_split_kernel<kSeg, kNW, kCW, false, SER3, true, kPlanckWps>,
                                                                                     a, pt, s, tlay, tlev, tsfc);
      }
    });
  });
}

// launch_rte_lw_planck with one output plane per band: a.flux_up / a.flux_dn are (ncol,nlay+1,nband) and band_first[b] is the
// first 0-based g-point of band b (band_first[nband] = a.ng; ascending, no empty band).  One launch, grid (tiles, band): a
// block row takes the tiles by grid stride as the broadband kernel does.  The block cap of launch_form is shared among the
// rows (at least 128 blocks each): a block stages its window of the Planck table once and walks several tiles with it.
hipError_t launch_rte_lw_planck_bands(const RteLwArgs &a, const double *planck, int ntp, double t0, double dt, const double *tlay,
                                      const double *tlev, const double *tsfc, const unsigned short *band_first, hipStream_t s) {
  if (a.f32 || a.nlay != kSeg * kNW || a.ncol <= 0 || a.nband < 1 || a.nband > 256 || !band_first) return hipErrorInvalidValue;
  if (a.part_mask && a.ng > 64) return hipErrorInvalidValue;
  BandWindows bw{};
  for (int b = 0; b <= a.nband; ++b) bw.first[b] = band_first[b];
  for (int b = 0; b < a.nband; ++b)
    if (bw.first[b + 1] <= bw.first[b] || bw.first[b + 1] > a.ng) return hipErrorInvalidValue;
  if (bw.first[0] != 0 || bw.first[a.nband] != a.ng) return hipErrorInvalidValue;
  const PlanckTab pt{planck, t0, dt, 1. / dt, ntp, a.ng};
  return with_bool(a.series3, [&](auto ser3) {
    return with_particles(a, [&](auto sky, auto mask) {
      constexpr bool SER3 = decltype(ser3)::value, MASK = decltype(mask)::value;
      constexpr int SKY = decltype(sky)::value;
      using F = BandsForm<kSeg, kNW, kCW, SER3, SKY, MASK, kPlanckWps>;
      auto k = rte_lw_split_bands_kernel<kSeg, kNW, kCW, SER3, SKY, MASK, kPlanckWps>;
      const size_t lds = SplitLds<F>::bytes(ntp, a.ng);
      if (lds > (size_t)kLdsBudget) return hipErrorInvalidValue;
      hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      if (e != hipSuccess) return e;
      long blocks = (((long)a.ncol + F::CW - 1) / F::CW + F::NG - 1) / F::NG;
      const long cap = 256L * 4 / a.nband > 128 ? 256L * 4 / a.nband : 128;
      if (blocks > cap) blocks = cap;
      hipLaunchKernelGGL(k, dim3((unsigned)blocks, (unsigned)a.nband), dim3(F::THREADS), lds, s, a, pt, tlay, tlev, tsfc, bw);
      return hipGetLastError();
    });
  });
}

hipError_t launch_rte_lw_rescaled_split(const RteLwArgs &a, hipStream_t s) {
  if (a.f32 || a.nlay != kSeg * kNW || a.ncol <= 0 || !a.ssa || !a.g) return hipErrorInvalidValue;
  return with_bool(a.series3, [&](auto ser3) {
    constexpr bool SER3 = decltype(ser3)::value;
    return launch_form<RescaledForm<kSeg, kNW, kCW, SER3, kRescWps>>(rte_lw_split_rescaled_kernel<kSeg, kNW, kCW, SER3, kRescWps>, a, no_table(a), s);
  });
}

hipError_t launch_rte_lw_rescaled_planck(const RteLwArgs &a, const double *planck, int ntp, double t0, double dt,
                                         const double *tlay, const double *tlev, const double *tsfc, hipStream_t s,
                                         double *flux_up_jac) {
  if (a.f32 || a.nlay != kSeg * kNW || a.ncol <= 0 || !a.part_tau || !a.part_ssa || !a.part_g) return hipErrorInvalidValue;
  if (a.part_mask && a.ng > 64) return hipErrorInvalidValue;
  const PlanckTab pt{planck, t0, dt, 1. / dt, ntp, a.ng};
  return with_bool(a.series3, [&](auto ser3) {
    return with_bool(a.part_mask != nullptr, [&](auto mask) {
      constexpr bool SER3 = decltype(ser3)::value, MASK = decltype(mask)::value;
      if (flux_up_jac)   // the Jacobian form (ecckd_lw_fluxes_rescaled_jac, "lw_jac_inline" = 1)
        return launch_form<RescaledAllskyForm<kSeg, kNW, kCW, SER3, MASK, true, 1>>(rte_lw_split_rescaled_jac_kernel<kSeg, kNW, kCW, SER3, MASK>, a,
                                                                                    pt, s, tlay, tlev, tsfc, flux_up_jac);
      return launch_form<RescaledAllskyForm<kSeg, kNW, kCW, SER3, MASK, false, kRescWpsPlanck>>(
          rte_lw_split_rescaled_allsky_kernel<kSeg, kNW, kCW, SER3, MASK, kRescWpsPlanck>, a, pt, s, tlay, tlev, tsfc);
    });
  });
}

}  // namespace ecckd
