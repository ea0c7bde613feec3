// kernels_rte_lw_split.hip -- longwave no-scattering solver, layer-split form: the NW waves of a block share one
// tile of (CW columns x 64/CW g-points) and each walks a SEGMENT of SEG = nlay/NW layers.
//
// Why: the register-resident solver of kernels_rte_lw.hip keeps trans(l) and source_up(l) of all 60 layers in
// registers (2 x 60 doubles: one wave per SIMD), and one wave alone issues an fp64 instruction only every ~10
// clocks (tools/ubench.hip: 0.40 wave-instructions/clk/CU at 4 waves per CU against 0.74-0.81 at 12-16): that
// kernel is bound by its own issue cadence, not by HBM.  The layer recurrences are AFFINE,
//     I_dn(l+1) = t(l) I_dn(l) + s_dn(l),      I_up(l) = t(l) I_up(l+1) + s_up(l),
// so a segment of layers composes into (T, D, U) with  I_out = T I_in + D  and  U_out = T U_in + U.  Each wave
// does the expensive part (exp, the source functions) for its own 15 layers only -- 3 x 15 doubles in registers,
// three waves per SIMD -- then the NW composites are exchanged through LDS (one block barrier per g-point group),
// every wave folds them into the intensities that enter its segment from above and from below, and finishes
// its 15 levels of both sweeps out of registers.  Same arithmetic per cell as lw_solver_noscat; the intensities
// entering a segment are composed in a different association than a top-to-bottom walk would (relative 1e-16).
//
// PLANCK variant ("fused longwave"): the three source arrays are not read from HBM
// but recomputed from tlay / tlev and the Planck table (src/gas_optics_ecckd.f90:245-289, :407-424) inside
// the solver, so gas optics only has to write tau: 16 instead of 64 B/cell between the two kernels.
#include <cstdlib>

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
// layers in flight per lane
constexpr int split_pf(bool planck) { return planck ? ECCKD_SPLIT_PF_PLANCK : ECCKD_SPLIT_PF; }

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

// NG tile groups of NW waves per block.  The Planck-recomputing form runs two groups per block (8 waves) that share one
// copy of the Planck table in LDS (61-68 KB): read from global memory instead, the two dependent table loads per source
// leave the kernel latency-bound at its two waves per SIMD (measured 21 ms per 1e6 columns against 11 from LDS).
constexpr int split_groups(bool planck) { return planck ? 2 : 1; }
__host__ __device__ constexpr int planck_stride(int ng) { return ng | 1; }   // odd number of doubles per row

// The kernel text, shared by the clear-sky kernel (SKY = 0: rte_lw_split_kernel) and the all-sky form of the
// Planck-recomputing solver (rte_lw_split_allsky_kernel).  SKY = 1 / 2: the particulate optical depth of the layer on the
// model's bands, a.part_tau (ncol,nlay,nband), is added to the gas optical depth in front of tl = tau * D -- as it is
// (1: one-stream particles, increment_1scalar_by_1scalar) or as the absorption optical depth part_tau * (1 - part_ssa)
// (2: two-stream particles, increment_1scalar_by_2stream), the expressions of kernels_optical_props.hip operation by
// operation.  The two g-points of a wave may sit in different bands, so the band offset is per lane; the band values ride
// in prefetch slots next to ptau[] (one load per (layer, iteration) from planes that stay in L2).
// MASK (with SKY; rte_lw_split_mcica_kernel, ecckd_lw_fluxes_allsky_mcica): a.part_mask holds one 64-bit word per
// (column, layer); where bit g is clear the cell uses part_tau = 0 in front of the expressions above -- one select per
// cell.  The lane's g-point is fixed for an iteration, so a prefetch slot carries only the 32-bit half of the word that
// holds it.
// BOTH (with SKY; rte_lw_split_both_kernel, ecckd_lw_fluxes_clear_allsky): the dual-sky form.  One group per block walks
// the clear sky (the gas optical depth as it is read) and the all sky of its tile in one pass: the three Planck sources of
// a cell and the surface source are evaluated once, everything that hangs on the optical depth -- t, sdn, su, the
// composites, the exchange and the accumulators -- exists twice, and the clear-sky fluxes go to flux_up_clear /
// flux_dn_clear.  The second exchange and accumulator set takes the LDS of the second group, and the block's four waves
// sit one per SIMD with the whole register file.  Each sky's per-cell expressions and the order in which a level's
// accumulator receives its g-points are those of the single-sky kernels: the fluxes are theirs bit for bit.
// JAC (PLANCK forms; rte_lw_split_jac_kernel, ecckd_lw_fluxes_jac with "lw_jac_inline" = 1): the surface-temperature
// Jacobian of flux_up next to the fluxes.  Its surface term eps * (B(tsfc + 1) - B(tsfc)) is folded through the
// transmissivities of the waves below (x[(q*3+0)...], already exchanged) and carried through the up sweep with the T[s] the
// sweep holds in registers: one multiply and one accumulator add per (cell, angle).  The third accumulator plane
// ([NL+1][CW], 15.6 KB) does not fit next to two groups and the Planck table, so this form runs one group per block and
// one wave per SIMD like the dual-sky form (59.1 KB + the table).  The flux expressions and the order in which a level's
// flux accumulators receive their g-points are untouched: the fluxes are the single-sky kernels' bit for bit.
// RESC (rte_lw_split_rescaled_kernel, ecckd_rte_lw_rescaled; with PLANCK and SKY = 2 rte_lw_split_rescaled_allsky_kernel,
// ecckd_lw_fluxes_allsky_rescaled): the rescaled no-scattering solver (include/ecckd_hip.h, "Rescaled longwave").  The cell
// has (tau, ssa, g) -- read from a.tau / a.ssa / a.g, or formed from the gas optical depth and the band triple with the
// operations of increment_2stream_by_2stream (kernels_optical_props.hip) -- and phase 1 keeps five values per layer: t, sdn,
// CA = Cn*(1 - t*t), SUA = sup - Cn*(sdn*t + sup) (in SU[]) and SDA = sdn - Cn*(sup*t + sdn).  The three sweeps are three
// affine recurrences whose sources are known once the sweep before is finished, so phase 2 has three exchanges:
//   1. (T, D) as above gives dn0 entering the segment; the wave walks dn0 through its layers, SU[s] += CA[s]*dn0[s], and
//      composes U of the adjusted up sweep;
//   2. (T, U): the adjusted up sweep, accumulated per level as above, SDA[s] += CA[s]*up[s+1], and D of the adjusted down
//      sweep (into the slot of the first exchange's D, which every wave has read before the second barrier);
//   3. (T, D): the adjusted down sweep, accumulated per level as above.
// One group per block.  No other instantiation changes: every RESC statement sits behind `if constexpr`.
// RESC with JAC (PLANCK forms; rte_lw_split_rescaled_jac_kernel, ecckd_lw_fluxes_rescaled_jac with "lw_jac_inline" = 1): with
// every source zero dn0 == 0 and the adjusted up sweep reduces to up[s] = t * up[s+1], so the Jacobian is the JAC form's:
// the surface term folded through the exchanged T of the waves below, then carried through the adjusted up sweep behind the
// second exchange (one multiply and one accumulator add per (cell, angle)).  The third accumulator plane sits behind the
// exchange area; the flux statements and their order are untouched, so the fluxes are the rescaled kernel's bit for bit.
template <int SEG, int NW, int CW, bool SHARED, bool SER3, bool PLANCK, int SKY, bool MASK = false, bool BOTH = false, bool JAC = false,
          bool RESC = false>
__device__ __forceinline__ void rte_lw_split_body(const RteLwArgs &a, const PlanckTab &pt, const double *tlay, const double *tlev,
                                                  const double *tsfc, [[maybe_unused]] double *flux_up_clear = nullptr,
                                                  [[maybe_unused]] double *flux_dn_clear = nullptr,
                                                  [[maybe_unused]] double *flux_up_jac = nullptr) {
  static_assert(SKY == 0 || PLANCK, "the all-sky form extends the Planck-recomputing solver");
  static_assert(SKY != 0 || !MASK, "a cloud mask belongs to the all-sky form");
  static_assert(SKY != 0 || !BOTH, "the dual-sky form extends the all-sky form");
  static_assert(!JAC || (PLANCK && !BOTH), "the Jacobian form extends the single-sky Planck-recomputing solver");
  static_assert(!RESC || (!SHARED && !BOTH && (!JAC || PLANCK) && (PLANCK ? SKY == 2 : SKY == 0)),
                "the rescaled form reads arrays, or recomputes Planck sources and takes a two-stream band triple");
  constexpr int GW = 64 / CW;
  constexpr int NL = SEG * NW;
  constexpr int NG = (BOTH || JAC || RESC) ? 1 : split_groups(PLANCK);
  constexpr int kSplitPF = (RESC && !PLANCK) ? 1 : split_pf(PLANCK);   // (RESC on arrays: six arrays in flight per layer, no room for a second layer)
  constexpr int kSkyDoubles = 2 * (NL + 1) * CW + 2 * NW * 3 * 64;   // accumulators and exchange of one sky
  constexpr int kGroupDoubles = (BOTH ? 2 : 1) * kSkyDoubles + (JAC ? (NL + 1) * CW : 0);
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int grp = (tid >> 6) / NW, w = (tid >> 6) % NW, gtid = tid - grp * 64 * NW;
  double *acc_dn = reinterpret_cast<double *>(lds_raw) + grp * kGroupDoubles;   // [NL+1][CW]
  double *acc_up = acc_dn + (NL + 1) * CW;                                         // [NL+1][CW]
  double *xch = acc_up + (NL + 1) * CW;                                            // [2][NW][3][64]
  // BOTH: the clear sky's set behind the all sky's, laid out alike
  [[maybe_unused]] double *acc_dn_c = acc_dn + kSkyDoubles, *acc_up_c = acc_up + kSkyDoubles, *xch_c = xch + kSkyDoubles;
  [[maybe_unused]] double *acc_jac = acc_dn + kSkyDoubles;   // JAC: [NL+1][CW] behind the exchange
  [[maybe_unused]] const int pstride = PLANCK ? planck_stride(a.ng) : 0;
  [[maybe_unused]] double *ptab = reinterpret_cast<double *>(lds_raw) + NG * kGroupDoubles;   // PLANCK: [ntp][pstride]
  if (PLANCK) {
    for (int i = tid; i < pt.ntp * pt.ng; i += 64 * NW * NG) {
      const int r = i / pt.ng, g = i - r * pt.ng;
      ptab[r * pstride + g] = pt.tab[i];
    }
  }
  const int cl = lane % CW, gs = lane / CW;
  const bool owner = gs == 0;
  const int ncol = a.ncol, ng = a.ng;
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

  for (int i = gtid; i < 2 * (NL + 1) * CW; i += 64 * NW) acc_dn[i] = 0.;
  if (BOTH)
    for (int i = gtid; i < 2 * (NL + 1) * CW; i += 64 * NW) acc_dn_c[i] = 0.;
  if (JAC)
    for (int i = gtid; i < (NL + 1) * CW; i += 64 * NW) acc_jac[i] = 0.;
  __syncthreads();

  // every group of the block walks the same number of tiles (block barriers inside): a group whose tile lies beyond the
  // end computes on clamped columns and stores nothing
  for (long tile0 = (long)blockIdx.x * NG; tile0 < ntiles; tile0 += (long)gridDim.x * NG) {
    const long tile = tile0 + grp;
    const long col = tile * CW + cl;
    const bool valid = col < ncol;
    const long cc = valid ? col : (long)ncol - 1;

    double ptau[kSplitPF];
    [[maybe_unused]] double play_[PLANCK ? 1 : kSplitPF], pbdn[PLANCK ? 1 : kSplitPF], pbup[(PLANCK || SHARED) ? 1 : kSplitPF];
    [[maybe_unused]] double ptl[PLANCK ? kSplitPF : 1], ptv[PLANCK ? kSplitPF : 1];   // PLANCK: tlay(l), tlev(far edge of l)
    [[maybe_unused]] double ppt[SKY ? kSplitPF : 1], pps[SKY == 2 ? kSplitPF : 1];   // SKY: part_tau(l), part_ssa(l) of the lane's band
    [[maybe_unused]] long qb = 0;      // SKY: offset of the lane's band plane
    [[maybe_unused]] double pss[RESC && !PLANCK ? kSplitPF : 1], pgg[RESC ? kSplitPF : 1];   // RESC: ssa(l) of the cell (arrays); g(l) of the cell, or part_g(l) of the lane's band
    [[maybe_unused]] unsigned pmk[MASK ? kSplitPF : 1];   // MASK: the half of part_mask(column, l) that holds the lane's g-point
    [[maybe_unused]] int mhalf = 0, mbit = 0;             // MASK: which half, and the bit inside it
    [[maybe_unused]] const unsigned *mask32 = reinterpret_cast<const unsigned *>(a.part_mask);
    long qn = 0;
    const long qstep = (long)ncol * lstep;
    [[maybe_unused]] long q2 = 0;      // PLANCK: offset into tlay / tlev rows (no g dimension)
    [[maybe_unused]] int glev = 0;     // SHARED: the lane's g-point; its plane of the level arrays lies dlev * glev beyond that of the others
    [[maybe_unused]] double near_first = 0.;   // SHARED / PLANCK: near-edge source (temperature) of the segment's first layer

    auto pair_start = [&](int it) {
      const int g = (it / a.nmus) * GW + gs;
      const int gg = g < ng ? g : ng - 1;
      qn = cc + (long)ncol * NL * gg + (long)ncol * (lay0 + lstep * s0);
      asm volatile("" : "+v"(qn));
      if (PLANCK) {
        q2 = cc + (long)ncol * (lay0 + lstep * s0);
        // level at the near (upper, in walking order) edge of the first layer of the segment
        near_first = tlev[cc + (long)ncol * (lev0 + lstep * s0)];
        if (SKY) qb = (long)ncol * NL * a.gpt2band[gg];
        if (MASK) mhalf = gg >> 5;
      } else if (SHARED) {
        glev = gg;
        asm volatile("" : "+v"(glev));
        near_first = __builtin_nontemporal_load(Bup + (qn + (long)dlev * glev));
      }
    };
    auto issue = [&](int slot) {
      ptau[slot] = __builtin_nontemporal_load(a.tau + qn);
      if (PLANCK) {
        ptl[slot] = tlay[q2];
        ptv[slot] = tlev[q2 + (a.top_at_1 ? (long)ncol : 0)];   // far edge of the layer: level index l+1 (top_at_1) or l
        if (SKY) ppt[slot] = a.part_tau[q2 + qb];
        if (SKY == 2) pps[slot] = a.part_ssa[q2 + qb];
        if constexpr (RESC) pgg[slot] = a.part_g[q2 + qb];
        if (MASK) pmk[slot] = mask32[2 * q2 + mhalf];
        q2 += qstep;
      } else {
        play_[slot] = __builtin_nontemporal_load(a.lay_source + qn);
        if constexpr (SHARED) {
          asm volatile("" : "+v"(glev));   // (the product below is formed here, in the add, and not kept in a register pair)
          pbdn[slot] = __builtin_nontemporal_load(Bdn + (qn + (long)dlev * glev));
        } else {
          pbdn[slot] = __builtin_nontemporal_load(Bdn + qn);
        }
        if (!SHARED) pbup[slot] = __builtin_nontemporal_load(Bup + qn);
        if constexpr (RESC) {
          pss[slot] = __builtin_nontemporal_load(a.ssa + qn);
          pgg[slot] = __builtin_nontemporal_load(a.g + qn);
        }
      }
      qn += qstep;
      asm volatile("" : "+v"(qn));
    };

    pair_start(0);
#pragma unroll
    for (int s = 0; s < kSplitPF; ++s) issue(s);

    for (int it = 0; it < niter; ++it) {
      const int gi = it / a.nmus, k = it - gi * a.nmus;
      const int g = gi * GW + gs;
      const bool gact = g < ng;
      const int gg = gact ? g : ng - 1;
      const double D = a.Ds[k];
      if (MASK) mbit = gg & 31;   // (pair_start(it + 1), below, moves mhalf on while this iteration's slots are used up)
      const double wfac = gact ? 2. * pi * a.wts[k] : 0.;

      // ---------------- phase 1: this wave's SEG layers ----------------
      double T[SEG], SDN[SEG], SU[SEG];
      double Tq = 1., Dq = 0.;
      [[maybe_unused]] double Tc[BOTH ? SEG : 1], SDNc[BOTH ? SEG : 1], SUc[BOTH ? SEG : 1];   // BOTH: the clear sky's
      [[maybe_unused]] double Tqc = 1., Dqc = 0.;
      [[maybe_unused]] double CA[RESC ? SEG : 1], SDA[RESC ? SEG : 1];   // RESC: Cn*(1 - t*t), and the adjusted down source
      [[maybe_unused]] double carry = PLANCK ? planck_at(pt, ptab, pstride, near_first, gg, pi_f32, rpi_f32) : near_first;
#pragma unroll
      for (int s = 0; s < SEG; ++s) {
        double tau = ptau[s % kSplitPF];
        [[maybe_unused]] const double tau_c = tau;   // BOTH: the gas optical depth alone
        [[maybe_unused]] double tp = 0.;
        if (SKY) tp = ppt[s % kSplitPF];
        if (MASK) tp = (pmk[s % kSplitPF] >> mbit) & 1u ? tp : 0.;
        if constexpr (!RESC) {
        if (SKY == 1) tau = tau + tp;
        if (SKY == 2) tau = tau + tp * (1. - pps[s % kSplitPF]);
        }
        [[maybe_unused]] double Cn = 0.;
        if constexpr (RESC) {
          double cssa, cg;
          if constexpr (PLANCK) {
            // increment_body<double, true, true, true, MASK> of kernels_optical_props.hip on op1 = (tau_gas, +0, +0)
            constexpr double tiny3 = op_eps<double>();
            const double tscat2 = tp * pps[s % kSplitPF];
            const double tsg2 = tscat2 * pgg[s % kSplitPF];
            const double tau12 = tau + tp;
            const double tscat1 = tau * 0.;
            const double tauscat12 = tscat1 + tscat2;
            cg = (tscat1 * 0. + tsg2) / (tauscat12 > tiny3 ? tauscat12 : tiny3);
            cssa = tauscat12 / (tau12 > tiny3 ? tau12 : tiny3);
            tau = tau12;
          } else {
            cssa = pss[s % kSplitPF];
            cg = pgg[s % kSplitPF];
          }
          const double wb = cssa * (1. - cg) * 0.5;
          const double sc = (1. - cssa) + wb;
          tau = tau * sc;
          Cn = 0.4 * (wb / sc);   // (IEEE division: ssa = g = 1 gives 0/0, a NaN that stays in its column)
        }
        double lay, bdn, bup;
        if (PLANCK) {
          lay = planck_at(pt, ptab, pstride, ptl[s % kSplitPF], gg, pi_f32, rpi_f32);
          bdn = planck_at(pt, ptab, pstride, ptv[s % kSplitPF], gg, pi_f32, rpi_f32);
          bup = carry;
        } else {
          lay = play_[s % kSplitPF];
          bdn = pbdn[s % kSplitPF];
          bup = SHARED ? carry : pbup[s % kSplitPF];
        }
        if (s + kSplitPF < SEG) {
          asm volatile("" : "+v"(qn), "+v"(Dq));   // keep the loads of layer s+PF below layer s-1
          issue(s % kSplitPF);
        }
        const double tl = tau * D;
        const double t = lw_exp(-tl);
        const double omt = 1. - t;
        const double fact_big = lw_div(omt, tl) - t;
        const double fact_small = SER3 ? tl * (0.5 + tl * (-1. / 3. + tl * (1. / 8.))) : tl * (0.5 - 1. / 3. * tl);
        const double fact = tl > tau_thresh ? fact_big : fact_small;
        const double sdn = omt * bdn + 2. * fact * (lay - bdn);
        double su = omt * bup + 2. * fact * (lay - bup);
        asm volatile("" : "+v"(su));
        T[s] = t; SDN[s] = sdn; SU[s] = su;
        if constexpr (RESC) {
          CA[s] = Cn * (1. - t * t);
          SU[s] = su - Cn * (sdn * t + su);
          SDA[s] = sdn - Cn * (su * t + sdn);
        }
        Dq = t * Dq + sdn;
        Tq = Tq * t;
        if (BOTH) {   // the same cell under the clear sky: the expressions above on tau_c
          const double tlc = tau_c * D;
          const double tc = lw_exp(-tlc);
          const double omtc = 1. - tc;
          const double factc_big = lw_div(omtc, tlc) - tc;
          const double factc_small = SER3 ? tlc * (0.5 + tlc * (-1. / 3. + tlc * (1. / 8.))) : tlc * (0.5 - 1. / 3. * tlc);
          const double factc = tlc > tau_thresh ? factc_big : factc_small;
          const double sdnc = omtc * bdn + 2. * factc * (lay - bdn);
          double suc = omtc * bup + 2. * factc * (lay - bup);
          asm volatile("" : "+v"(suc));
          Tc[s] = tc; SDNc[s] = sdnc; SUc[s] = suc;
          Dqc = tc * Dqc + sdnc;
          Tqc = Tqc * tc;
        }
        if (SHARED || PLANCK) carry = bdn;
      }
      double Uq = 0.;
      if constexpr (!RESC) {   // (RESC: the up sweep's sources wait for dn0, behind the first exchange)
#pragma unroll
      for (int s = SEG - 1; s >= 0; --s) Uq = T[s] * Uq + SU[s];
      }
      [[maybe_unused]] double Uqc = 0.;
      if (BOTH) {
#pragma unroll
        for (int s = SEG - 1; s >= 0; --s) Uqc = Tc[s] * Uqc + SUc[s];
      }
      // the next pair's first layers start streaming now
      if (it + 1 < niter) {
        pair_start(it + 1);
#pragma unroll
        for (int s = 0; s < kSplitPF; ++s) issue(s);
      }
      double *x = xch + (it & 1) * (NW * 3 * 64);
      x[(w * 3 + 0) * 64 + lane] = Tq;
      x[(w * 3 + 1) * 64 + lane] = Dq;
      if constexpr (!RESC) x[(w * 3 + 2) * 64 + lane] = Uq;
      [[maybe_unused]] double *xc = xch_c + (it & 1) * (NW * 3 * 64);
      if (BOTH) {
        xc[(w * 3 + 0) * 64 + lane] = Tqc;
        xc[(w * 3 + 1) * 64 + lane] = Dqc;
        xc[(w * 3 + 2) * 64 + lane] = Uqc;
      }
      __syncthreads();

      // ---------------- phase 2: boundary intensities of this segment, then both sweeps ----------------
      double I = 0.;   // radn_dn(top): no incident diffuse flux, or inc_flux as an intensity (Appendix B.1)
      if (a.inc_flux) {
        const double f = a.inc_flux[cc + (long)ncol * gg];
        I = a.inc_isotropic ? f / pi : f / (2. * pi * a.wts[k]);
      }
      [[maybe_unused]] const double Itop = I;
      double Iin = I;
#pragma unroll
      for (int q = 0; q < NW; ++q) {
        if (q == w) Iin = I;
        I = x[(q * 3 + 0) * 64 + lane] * I + x[(q * 3 + 1) * 64 + lane];
      }
      const double eps = a.sfc_emis[a.gpt2band[gg] + (long)a.nband * cc];
      const double sfc_src = PLANCK ? planck_at(pt, ptab, pstride, tsfc[cc], gg, pi_f32, rpi_f32) : a.sfc_source[cc + (long)ncol * gg];
      double U = I * (1. - eps) + eps * sfc_src;   // surface
      if constexpr (RESC) {
        // the surface has seen the unadjusted dn0.  dn0 through this segment: the sources of the adjusted up sweep
        const double Usfc = U;
        I = Iin;
#pragma unroll
        for (int s = 0; s < SEG; ++s) {
          SU[s] = SU[s] + CA[s] * I;
          I = T[s] * I + SDN[s];
        }
#pragma unroll
        for (int s = SEG - 1; s >= 0; --s) Uq = T[s] * Uq + SU[s];
        x[(w * 3 + 2) * 64 + lane] = Uq;
        __syncthreads();
        U = Usfc;
        double Uin = U;
#pragma unroll
        for (int q = NW - 1; q >= 0; --q) {
          if (q == w) Uin = U;
          U = x[(q * 3 + 0) * 64 + lane] * U + x[(q * 3 + 2) * 64 + lane];
        }
        [[maybe_unused]] double J = 0.;   // JAC: d(intensity) / d(tsfc) entering this segment from below
        if constexpr (JAC) {   // with all sources zero dn0 == 0 and the adjusted up sweep is J = t * J: the fold of the JAC form above
          double Jq = eps * (planck_at(pt, ptab, pstride, tsfc[cc] + 1., gg, pi_f32, rpi_f32) - sfc_src);
          J = Jq;
#pragma unroll
          for (int q = NW - 1; q >= 0; --q) {
            if (q == w) J = Jq;
            Jq = x[(q * 3 + 0) * 64 + lane] * Jq;
          }
        }
        // adjusted up sweep: levels s0+SEG .. s0+1; the radiance entering a layer from below adjusts its down source
        U = Uin;
#pragma unroll
        for (int s = SEG - 1; s >= 0; --s) {
          acc_add(&acc_up[(s0 + s + 1) * CW + cl], gsum<CW>(wfac * U), owner);
          SDA[s] = SDA[s] + CA[s] * U;
          U = T[s] * U + SU[s];
          if constexpr (JAC) {
            acc_add(&acc_jac[(s0 + s + 1) * CW + cl], gsum<CW>(wfac * J), owner);
            J = T[s] * J;
          }
        }
        if (w == 0) acc_add(&acc_up[cl], gsum<CW>(wfac * U), owner);
        if constexpr (JAC) {
          if (w == 0) acc_add(&acc_jac[cl], gsum<CW>(wfac * J), owner);
        }
        double D3 = 0.;
#pragma unroll
        for (int s = 0; s < SEG; ++s) D3 = T[s] * D3 + SDA[s];
        x[(w * 3 + 1) * 64 + lane] = D3;   // (every wave read the first exchange's D before the barrier above)
        __syncthreads();
        I = Itop;
        Iin = I;
#pragma unroll
        for (int q = 0; q < NW; ++q) {
          if (q == w) Iin = I;
          I = x[(q * 3 + 0) * 64 + lane] * I + x[(q * 3 + 1) * 64 + lane];
        }
        // adjusted down sweep: levels s0 .. s0+SEG-1; the last wave adds the surface
        I = Iin;
#pragma unroll
        for (int s = 0; s < SEG; ++s) {
          acc_add(&acc_dn[(s0 + s) * CW + cl], gsum<CW>(wfac * I), owner);
          I = T[s] * I + SDA[s];
        }
        if (w == NW - 1) acc_add(&acc_dn[NL * CW + cl], gsum<CW>(wfac * I), owner);
      } else {
      double Uin = U;
#pragma unroll
      for (int q = NW - 1; q >= 0; --q) {
        if (q == w) Uin = U;
        U = x[(q * 3 + 0) * 64 + lane] * U + x[(q * 3 + 2) * 64 + lane];
      }
      [[maybe_unused]] double J = 0.;   // JAC: d(intensity) / d(tsfc) entering this segment from below
      if (JAC) {
        double Jq = eps * (planck_at(pt, ptab, pstride, tsfc[cc] + 1., gg, pi_f32, rpi_f32) - sfc_src);
        J = Jq;
#pragma unroll
        for (int q = NW - 1; q >= 0; --q) {
          if (q == w) J = Jq;
          Jq = x[(q * 3 + 0) * 64 + lane] * Jq;
        }
      }
      // down sweep of the segment: levels s0 .. s0+SEG-1 (the level above each layer); the last wave adds the surface
      I = Iin;
#pragma unroll
      for (int s = 0; s < SEG; ++s) {
        acc_add(&acc_dn[(s0 + s) * CW + cl], gsum<CW>(wfac * I), owner);
        I = T[s] * I + SDN[s];
      }
      if (w == NW - 1) acc_add(&acc_dn[NL * CW + cl], gsum<CW>(wfac * I), owner);
      // up sweep: levels s0+SEG .. s0+1 (the level below each layer); the first wave adds the top
      U = Uin;
#pragma unroll
      for (int s = SEG - 1; s >= 0; --s) {
        acc_add(&acc_up[(s0 + s + 1) * CW + cl], gsum<CW>(wfac * U), owner);
        U = T[s] * U + SU[s];
        if (JAC) {
          acc_add(&acc_jac[(s0 + s + 1) * CW + cl], gsum<CW>(wfac * J), owner);
          J = T[s] * J;
        }
      }
      if (w == 0) acc_add(&acc_up[cl], gsum<CW>(wfac * U), owner);
      if (JAC && w == 0) acc_add(&acc_jac[cl], gsum<CW>(wfac * J), owner);
      }
      if (BOTH) {   // phase 2 once more, on the clear sky's composites into the clear sky's accumulators
        double Ic = Itop, Iinc = Itop;
#pragma unroll
        for (int q = 0; q < NW; ++q) {
          if (q == w) Iinc = Ic;
          Ic = xc[(q * 3 + 0) * 64 + lane] * Ic + xc[(q * 3 + 1) * 64 + lane];
        }
        double Uc = Ic * (1. - eps) + eps * sfc_src;   // surface
        double Uinc = Uc;
#pragma unroll
        for (int q = NW - 1; q >= 0; --q) {
          if (q == w) Uinc = Uc;
          Uc = xc[(q * 3 + 0) * 64 + lane] * Uc + xc[(q * 3 + 2) * 64 + lane];
        }
        Ic = Iinc;
#pragma unroll
        for (int s = 0; s < SEG; ++s) {
          acc_add(&acc_dn_c[(s0 + s) * CW + cl], gsum<CW>(wfac * Ic), owner);
          Ic = Tc[s] * Ic + SDNc[s];
        }
        if (w == NW - 1) acc_add(&acc_dn_c[NL * CW + cl], gsum<CW>(wfac * Ic), owner);
        Uc = Uinc;
#pragma unroll
        for (int s = SEG - 1; s >= 0; --s) {
          acc_add(&acc_up_c[(s0 + s + 1) * CW + cl], gsum<CW>(wfac * Uc), owner);
          Uc = Tc[s] * Uc + SUc[s];
        }
        if (w == 0) acc_add(&acc_up_c[cl], gsum<CW>(wfac * Uc), owner);
      }
    }

    // broadband fluxes of the tile: level s-th from the top -> lev0 + lstep*s
    __syncthreads();
    for (int i = gtid; i < (NL + 1) * CW; i += 64 * NW) {
      const int s = i / CW, c = i - s * CW;
      const long cg = tile * CW + c;
      if (cg < ncol) {
        const long q = cg + (long)ncol * (lev0 + lstep * s);
        a.flux_dn[q] = acc_dn[i];
        a.flux_up[q] = acc_up[i];
        if (BOTH) {
          flux_dn_clear[q] = acc_dn_c[i];
          flux_up_clear[q] = acc_up_c[i];
        }
        if (JAC) flux_up_jac[q] = acc_jac[i];
      }
      acc_dn[i] = 0.;
      acc_up[i] = 0.;
      if (JAC) acc_jac[i] = 0.;
      if (BOTH) {
        acc_dn_c[i] = 0.;
        acc_up_c[i] = 0.;
      }
    }
    __syncthreads();
  }
}

template <int SEG, int NW, int CW, bool SHARED, bool SER3, bool PLANCK, int WPS>
__global__ void __launch_bounds__(64 * NW * split_groups(PLANCK), WPS) rte_lw_split_kernel(const RteLwArgs a, const PlanckTab pt,
                                                                                          const double *tlay, const double *tlev,
                                                                                          const double *tsfc) {
  rte_lw_split_body<SEG, NW, CW, SHARED, SER3, PLANCK, 0>(a, pt, tlay, tlev, tsfc);
}

// All-sky form of the Planck-recomputing solver.  TWOSTR: the particles carry part_ssa (absorption optical depth), else
// part_tau is added as it is.
template <int SEG, int NW, int CW, bool SER3, bool TWOSTR, int WPS>
__global__ void __launch_bounds__(64 * NW * split_groups(true), WPS) rte_lw_split_allsky_kernel(const RteLwArgs a, const PlanckTab pt,
                                                                                               const double *tlay, const double *tlev,
                                                                                               const double *tsfc) {
  rte_lw_split_body<SEG, NW, CW, false, SER3, true, TWOSTR ? 2 : 1>(a, pt, tlay, tlev, tsfc);
}

// ... with a McICA cloud mask (RteLwArgs::part_mask), under its own name
template <int SEG, int NW, int CW, bool SER3, bool TWOSTR, int WPS>
__global__ void __launch_bounds__(64 * NW * split_groups(true), WPS) rte_lw_split_mcica_kernel(const RteLwArgs a, const PlanckTab pt,
                                                                                              const double *tlay, const double *tlev,
                                                                                              const double *tsfc) {
  rte_lw_split_body<SEG, NW, CW, false, SER3, true, TWOSTR ? 2 : 1, true>(a, pt, tlay, tlev, tsfc);
}

// The dual-sky form (BOTH of rte_lw_split_body): clear-sky and all-sky fluxes of a tile in one pass, one group per block and
// one wave per SIMD.  MASK: with a McICA cloud mask.
template <int SEG, int NW, int CW, bool SER3, bool TWOSTR, bool MASK>
__global__ void __launch_bounds__(64 * NW, 1) rte_lw_split_both_kernel(const RteLwArgs a, const PlanckTab pt, const double *tlay,
                                                                       const double *tlev, const double *tsfc,
                                                                       double *flux_up_clear, double *flux_dn_clear) {
  rte_lw_split_body<SEG, NW, CW, false, SER3, true, TWOSTR ? 2 : 1, MASK, true>(a, pt, tlay, tlev, tsfc, flux_up_clear, flux_dn_clear);
}

// The Jacobian form (JAC of rte_lw_split_body): the fluxes of the clear-sky (SKY = 0), all-sky or McICA kernel and
// flux_up_jac from one pass, one group per block and one wave per SIMD.
template <int SEG, int NW, int CW, bool SER3, int SKY, bool MASK>
__global__ void __launch_bounds__(64 * NW, 1) rte_lw_split_jac_kernel(const RteLwArgs a, const PlanckTab pt, const double *tlay,
                                                                      const double *tlev, const double *tsfc, double *flux_up_jac) {
  rte_lw_split_body<SEG, NW, CW, false, SER3, true, SKY, MASK, false, true>(a, pt, tlay, tlev, tsfc, nullptr, nullptr, flux_up_jac);
}

// The rescaled forms (RESC of rte_lw_split_body), one group per block: on arrays (tau, ssa, g, three sources) ...
template <int SEG, int NW, int CW, bool SER3, int WPS>
__global__ void __launch_bounds__(64 * NW, WPS) rte_lw_split_rescaled_kernel(const RteLwArgs a, const PlanckTab pt) {
  rte_lw_split_body<SEG, NW, CW, false, SER3, false, 0, false, false, false, true>(a, pt, nullptr, nullptr, nullptr);
}
// ... and Planck-recomputing with the two-stream band triple (MASK: and a McICA cloud mask)
template <int SEG, int NW, int CW, bool SER3, bool MASK, int WPS>
__global__ void __launch_bounds__(64 * NW, WPS) rte_lw_split_rescaled_allsky_kernel(const RteLwArgs a, const PlanckTab pt,
                                                                                    const double *tlay, const double *tlev,
                                                                                    const double *tsfc) {
  rte_lw_split_body<SEG, NW, CW, false, SER3, true, 2, MASK, false, false, true>(a, pt, tlay, tlev, tsfc);
}

// ... and that form with flux_up_jac of the all sky next to the fluxes (RESC with JAC): one wave per SIMD as it is
template <int SEG, int NW, int CW, bool SER3, bool MASK>
__global__ void __launch_bounds__(64 * NW, 1) rte_lw_split_rescaled_jac_kernel(const RteLwArgs a, const PlanckTab pt, const double *tlay,
                                                                               const double *tlev, const double *tsfc,
                                                                               double *flux_up_jac) {
  rte_lw_split_body<SEG, NW, CW, false, SER3, true, 2, MASK, false, true, true>(a, pt, tlay, tlev, tsfc, nullptr, nullptr, flux_up_jac);
}

// Both rescaled forms walk 15 layers per wave with 4 waves per block and 32 columns per tile: the fused call equals the
// composed one bit for bit only if both compose their segments alike ("lw_split_seg" does not act here).
constexpr int kRescSeg = 15, kRescNW = 4, kRescCW = 32;
constexpr int kRescWps = 2;         // arrays: 75 doubles of layer state per lane, two waves per SIMD
constexpr int kRescWpsPlanck = 1;   // Planck-recomputing: one block per CU (its LDS), one wave per SIMD
constexpr size_t resc_lds_doubles() { return 2 * (size_t)(kRescSeg * kRescNW + 1) * kRescCW + 2 * kRescNW * 3 * 64; }

template <bool SER3>
hipError_t launch_rescaled(const RteLwArgs &a, hipStream_t s) {
  const PlanckTab none{nullptr, 0., 1., 1., 2, a.ng};
  auto k = rte_lw_split_rescaled_kernel<kRescSeg, kRescNW, kRescCW, SER3, kRescWps>;
  const size_t lds = sizeof(double) * resc_lds_doubles();
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  long blocks = ((long)a.ncol + kRescCW - 1) / kRescCW;
  const long cap = 256L * kRescWps * 4;   // four rounds of resident blocks; the rest by grid stride (as launch_split)
  if (blocks > cap) blocks = cap;
  hipLaunchKernelGGL(k, dim3((unsigned)blocks), dim3(64 * kRescNW), lds, s, a, none);
  return hipGetLastError();
}

template <bool SER3, bool MASK>
hipError_t launch_rescaled_planck(const RteLwArgs &a, const PlanckTab &pt, const double *tlay, const double *tlev, const double *tsfc,
                                  hipStream_t s) {
  auto k = rte_lw_split_rescaled_allsky_kernel<kRescSeg, kRescNW, kRescCW, SER3, MASK, kRescWpsPlanck>;
  const size_t lds = sizeof(double) * (resc_lds_doubles() + (size_t)pt.ntp * planck_stride(a.ng));
  if (lds > (size_t)kLdsBudget) return hipErrorInvalidValue;
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  long blocks = ((long)a.ncol + kRescCW - 1) / kRescCW;
  const long cap = 256L * 4;   // one block is resident per CU; the rest by grid stride, as launch_split_both
  if (blocks > cap) blocks = cap;
  hipLaunchKernelGGL(k, dim3((unsigned)blocks), dim3(64 * kRescNW), lds, s, a, pt, tlay, tlev, tsfc);
  return hipGetLastError();
}

constexpr size_t resc_jac_lds_doubles() { return resc_lds_doubles() + (size_t)(kRescSeg * kRescNW + 1) * kRescCW; }

template <bool SER3, bool MASK>
hipError_t launch_rescaled_planck_jac(const RteLwArgs &a, const PlanckTab &pt, const double *tlay, const double *tlev,
                                      const double *tsfc, double *flux_up_jac, hipStream_t s) {
  auto k = rte_lw_split_rescaled_jac_kernel<kRescSeg, kRescNW, kRescCW, SER3, MASK>;
  // the rescaled form's accumulators and exchange, the Jacobian's plane, the Planck table
  const size_t lds = sizeof(double) * (resc_jac_lds_doubles() + (size_t)pt.ntp * planck_stride(a.ng));
  if (lds > (size_t)kLdsBudget) return hipErrorInvalidValue;
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  long blocks = ((long)a.ncol + kRescCW - 1) / kRescCW;
  const long cap = 256L * 4;   // as launch_rescaled_planck
  if (blocks > cap) blocks = cap;
  hipLaunchKernelGGL(k, dim3((unsigned)blocks), dim3(64 * kRescNW), lds, s, a, pt, tlay, tlev, tsfc, flux_up_jac);
  return hipGetLastError();
}

template <int SEG, int NW, int CW, bool SER3, int SKY, bool MASK>
hipError_t launch_split_jac(const RteLwArgs &a, const PlanckTab &pt, const double *tlay, const double *tlev, const double *tsfc,
                            double *flux_up_jac, hipStream_t s) {
  auto k = rte_lw_split_jac_kernel<SEG, NW, CW, SER3, SKY, MASK>;
  // one group: two flux accumulator planes and the exchange, the Jacobian's plane, the Planck table
  const size_t lds = sizeof(double) * (3 * (size_t)(SEG * NW + 1) * CW + 2 * NW * 3 * 64 + (size_t)pt.ntp * planck_stride(a.ng));
  if (lds > (size_t)kLdsBudget) return hipErrorInvalidValue;
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  long blocks = ((long)a.ncol + CW - 1) / CW;
  const long cap = 256L * 4;   // one block is resident per CU (its LDS); the rest by grid stride, as launch_split_both
  if (blocks > cap) blocks = cap;
  hipLaunchKernelGGL(k, dim3((unsigned)blocks), dim3(64 * NW), lds, s, a, pt, tlay, tlev, tsfc, flux_up_jac);
  return hipGetLastError();
}

template <int SEG, int NW, int CW, bool SER3, bool TWOSTR, bool MASK>
hipError_t launch_split_both(const RteLwArgs &a, const PlanckTab &pt, const double *tlay, const double *tlev, const double *tsfc,
                             double *flux_up_clear, double *flux_dn_clear, hipStream_t s) {
  auto k = rte_lw_split_both_kernel<SEG, NW, CW, SER3, TWOSTR, MASK>;
  // two skies of one group: the accumulators and exchange of the single-sky kernels' two groups
  const size_t lds = sizeof(double) * (2 * (2 * (size_t)(SEG * NW + 1) * CW + 2 * NW * 3 * 64) + (size_t)pt.ntp * planck_stride(a.ng));
  if (lds > (size_t)kLdsBudget) return hipErrorInvalidValue;
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  long blocks = ((long)a.ncol + CW - 1) / CW;
  // One block is resident per CU (its LDS), so 256 * 4 blocks are four rounds; past the cap a block walks tiles by grid
  // stride and reloads neither the Planck table nor its code.  A block here carries one tile per iteration where the
  // single-sky kernels carry two, so at equal block count the longest block runs ceil(tiles / 1024) tiles: 4 against a mean
  // of 3.05 at 1e5 columns (the tail is one tile, a quarter of a round), 31 against 30.5 at 1e6.  The timings of DESIGN
  // section 5.5c were taken with this cap.
  const long cap = 256L * 4;
  if (blocks > cap) blocks = cap;
  hipLaunchKernelGGL(k, dim3((unsigned)blocks), dim3(64 * NW), lds, s, a, pt, tlay, tlev, tsfc, flux_up_clear, flux_dn_clear);
  return hipGetLastError();
}

// SKY: 0 the clear-sky kernel, 1 / 2 the all-sky form with one- / two-stream particles (PLANCK only); MASK: with a.part_mask
template <int SEG, int NW, int CW, bool SHARED, bool SER3, bool PLANCK, int WPS = ECCKD_SPLIT_WAVES_PER_SIMD, int SKY = 0, bool MASK = false>
hipError_t launch_split(const RteLwArgs &a, const PlanckTab &pt, const double *tlay, const double *tlev, const double *tsfc,
                        hipStream_t s) {
  void (*k)(const RteLwArgs, const PlanckTab, const double *, const double *, const double *);
  if constexpr (SKY != 0 && MASK) k = rte_lw_split_mcica_kernel<SEG, NW, CW, SER3, SKY == 2, WPS>;
  else if constexpr (SKY != 0) k = rte_lw_split_allsky_kernel<SEG, NW, CW, SER3, SKY == 2, WPS>;
  else k = rte_lw_split_kernel<SEG, NW, CW, SHARED, SER3, PLANCK, WPS>;
  constexpr int NG = split_groups(PLANCK);
  const size_t lds = sizeof(double) * (NG * (2 * (size_t)(SEG * NW + 1) * CW + 2 * NW * 3 * 64) +
                                       (PLANCK ? (size_t)pt.ntp * planck_stride(a.ng) : 0));
  if (lds > (size_t)kLdsBudget) return hipErrorInvalidValue;
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  long blocks = (((long)a.ncol + CW - 1) / CW + NG - 1) / NG;
  const long cap = PLANCK ? 256L * 4 : 256L * WPS * 4;   // four rounds of resident blocks; the rest by grid stride
  if (blocks > cap) blocks = cap;
  hipLaunchKernelGGL(k, dim3((unsigned)blocks), dim3(64 * NW * NG), lds, s, a, pt, tlay, tlev, tsfc);
  return hipGetLastError();
}

}  // namespace

// LDS of the Planck-recomputing form (launch_seg<..., PLANCK = true>: 15 layers per wave, 4 waves, 32 columns): does the
// model's Planck table fit next to the accumulators?  (The shipped 32 / 36-g models do; a 64-g table does not.)
bool rte_lw_planck_fits(int ng, int ntp) {
  constexpr int SEG = 15, NW = 4, CW = 32, NG = split_groups(true);
  const size_t lds = sizeof(double) * (NG * (2 * (size_t)(SEG * NW + 1) * CW + 2 * NW * 3 * 64) + (size_t)ntp * planck_stride(ng));
  return lds <= (size_t)kLdsBudget;
}

bool rte_lw_split_applies(const RteLwArgs &a) {
  return !a.f32 && a.nlay == 60 && a.ncol > 0;
}

template <bool SHARED, bool SER3, bool PLANCK>
static hipError_t launch_seg(const RteLwArgs &a, const PlanckTab &pt, const double *tlay, const double *tlev, const double *tsfc,
                             hipStream_t s) {
  // The Planck-recomputing form needs 244 VGPRs: 15 layers per wave, two waves per SIMD (three spill 25-54 registers)
  if constexpr (PLANCK) {
    // all-sky (a.part_tau): the band planes ride in prefetch slots; still two waves per SIMD without a spill
    if (a.part_tau && a.part_mask) {   // McICA: 249 / 241 VGPRs, no spill
      if (a.ng > 64) return hipErrorInvalidValue;
      if (a.part_1scl || !a.part_ssa) return launch_split<15, 4, 32, SHARED, SER3, PLANCK, 2, 1, true>(a, pt, tlay, tlev, tsfc, s);
      return launch_split<15, 4, 32, SHARED, SER3, PLANCK, 2, 2, true>(a, pt, tlay, tlev, tsfc, s);
    }
    if (a.part_tau) {
      if (a.part_1scl || !a.part_ssa) return launch_split<15, 4, 32, SHARED, SER3, PLANCK, 2, 1>(a, pt, tlay, tlev, tsfc, s);
      return launch_split<15, 4, 32, SHARED, SER3, PLANCK, 2, 2>(a, pt, tlay, tlev, tsfc, s);
    }
    return launch_split<15, 4, 32, SHARED, SER3, PLANCK, 2>(a, pt, tlay, tlev, tsfc, s);
  } else {
  switch (a.split_seg) {   // layers per wave: 10 (6 waves per block, 157 VGPRs, 12 waves per CU), 12 or 15
    case 15: return launch_split<15, 4, 32, SHARED, SER3, PLANCK>(a, pt, tlay, tlev, tsfc, s);
    case 12: return launch_split<12, 5, 32, SHARED, SER3, PLANCK>(a, pt, tlay, tlev, tsfc, s);
    default: return launch_split<10, 6, 32, SHARED, SER3, PLANCK>(a, pt, tlay, tlev, tsfc, s);
  }
  }
}

hipError_t launch_rte_lw_split(const RteLwArgs &a, hipStream_t s) {
  const PlanckTab none{nullptr, 0., 1., 1., 2, a.ng};
  if (a.shared_levels)
    return a.series3 ? launch_seg<true, true, false>(a, none, nullptr, nullptr, nullptr, s)
                     : launch_seg<true, false, false>(a, none, nullptr, nullptr, nullptr, s);
  return a.series3 ? launch_seg<false, true, false>(a, none, nullptr, nullptr, nullptr, s)
                   : launch_seg<false, false, false>(a, none, nullptr, nullptr, nullptr, s);
}

template <bool SER3>
static hipError_t launch_both(const RteLwArgs &a, const PlanckTab &pt, const double *tlay, const double *tlev, const double *tsfc,
                              double *up_c, double *dn_c, hipStream_t s) {
  const bool two = !(a.part_1scl || !a.part_ssa);
  if (a.part_mask) {
    if (a.ng > 64) return hipErrorInvalidValue;
    return two ? launch_split_both<15, 4, 32, SER3, true, true>(a, pt, tlay, tlev, tsfc, up_c, dn_c, s)
               : launch_split_both<15, 4, 32, SER3, false, true>(a, pt, tlay, tlev, tsfc, up_c, dn_c, s);
  }
  return two ? launch_split_both<15, 4, 32, SER3, true, false>(a, pt, tlay, tlev, tsfc, up_c, dn_c, s)
             : launch_split_both<15, 4, 32, SER3, false, false>(a, pt, tlay, tlev, tsfc, up_c, dn_c, s);
}

template <bool SER3>
static hipError_t launch_jac_inline(const RteLwArgs &a, const PlanckTab &pt, const double *tlay, const double *tlev, const double *tsfc,
                                    double *jac, hipStream_t s) {
  if (!a.part_tau) return launch_split_jac<15, 4, 32, SER3, 0, false>(a, pt, tlay, tlev, tsfc, jac, s);
  const bool two = !(a.part_1scl || !a.part_ssa);
  if (a.part_mask) {
    if (a.ng > 64) return hipErrorInvalidValue;
    return two ? launch_split_jac<15, 4, 32, SER3, 2, true>(a, pt, tlay, tlev, tsfc, jac, s)
               : launch_split_jac<15, 4, 32, SER3, 1, true>(a, pt, tlay, tlev, tsfc, jac, s);
  }
  return two ? launch_split_jac<15, 4, 32, SER3, 2, false>(a, pt, tlay, tlev, tsfc, jac, s)
             : launch_split_jac<15, 4, 32, SER3, 1, false>(a, pt, tlay, tlev, tsfc, jac, s);
}

hipError_t launch_rte_lw_planck(const RteLwArgs &a, const double *planck, int ntp, double t0, double dt, const double *tlay,
                                const double *tlev, const double *tsfc, hipStream_t s, double *flux_up_clear,
                                double *flux_dn_clear, double *flux_up_jac) {
  if (a.f32 || a.nlay != 60 || a.ncol <= 0) return hipErrorInvalidValue;
  const PlanckTab pt{planck, t0, dt, 1. / dt, ntp, a.ng};
  if (flux_up_jac) {   // the Jacobian form (ecckd_lw_fluxes_jac, "lw_jac_inline" = 1); the dual-sky kernel has none
    if (flux_up_clear || flux_dn_clear) return hipErrorInvalidValue;
    return a.series3 ? launch_jac_inline<true>(a, pt, tlay, tlev, tsfc, flux_up_jac, s)
                     : launch_jac_inline<false>(a, pt, tlay, tlev, tsfc, flux_up_jac, s);
  }
  if (flux_up_clear || flux_dn_clear) {   // the dual-sky kernel (ecckd_lw_fluxes_clear_allsky, "lw_both_skies" = 1)
    if (!flux_up_clear || !flux_dn_clear || !a.part_tau) return hipErrorInvalidValue;
    return a.series3 ? launch_both<true>(a, pt, tlay, tlev, tsfc, flux_up_clear, flux_dn_clear, s)
                     : launch_both<false>(a, pt, tlay, tlev, tsfc, flux_up_clear, flux_dn_clear, s);
  }
  return a.series3 ? launch_seg<false, true, true>(a, pt, tlay, tlev, tsfc, s)
                   : launch_seg<false, false, true>(a, pt, tlay, tlev, tsfc, s);
}

hipError_t launch_rte_lw_rescaled_split(const RteLwArgs &a, hipStream_t s) {
  if (a.f32 || a.nlay != kRescSeg * kRescNW || a.ncol <= 0 || !a.ssa || !a.g) return hipErrorInvalidValue;
  return a.series3 ? launch_rescaled<true>(a, s) : launch_rescaled<false>(a, s);
}

bool rte_lw_rescaled_planck_fits(int ng, int ntp, bool jac) {
  return sizeof(double) * ((jac ? resc_jac_lds_doubles() : resc_lds_doubles()) + (size_t)ntp * planck_stride(ng)) <= (size_t)kLdsBudget;
}

hipError_t launch_rte_lw_rescaled_planck(const RteLwArgs &a, const double *planck, int ntp, double t0, double dt,
                                         const double *tlay, const double *tlev, const double *tsfc, hipStream_t s,
                                         double *flux_up_jac) {
  if (a.f32 || a.nlay != kRescSeg * kRescNW || a.ncol <= 0 || !a.part_tau || !a.part_ssa || !a.part_g) return hipErrorInvalidValue;
  if (a.part_mask && a.ng > 64) return hipErrorInvalidValue;
  const PlanckTab pt{planck, t0, dt, 1. / dt, ntp, a.ng};
  if (flux_up_jac) {   // the Jacobian form (ecckd_lw_fluxes_rescaled_jac, "lw_jac_inline" = 1)
    if (a.part_mask)
      return a.series3 ? launch_rescaled_planck_jac<true, true>(a, pt, tlay, tlev, tsfc, flux_up_jac, s)
                       : launch_rescaled_planck_jac<false, true>(a, pt, tlay, tlev, tsfc, flux_up_jac, s);
    return a.series3 ? launch_rescaled_planck_jac<true, false>(a, pt, tlay, tlev, tsfc, flux_up_jac, s)
                     : launch_rescaled_planck_jac<false, false>(a, pt, tlay, tlev, tsfc, flux_up_jac, s);
  }
  if (a.part_mask)
    return a.series3 ? launch_rescaled_planck<true, true>(a, pt, tlay, tlev, tsfc, s)
                     : launch_rescaled_planck<false, true>(a, pt, tlay, tlev, tsfc, s);
  return a.series3 ? launch_rescaled_planck<true, false>(a, pt, tlay, tlev, tsfc, s)
                   : launch_rescaled_planck<false, false>(a, pt, tlay, tlev, tsfc, s);
}

}  // namespace ecckd
