// kernels_rte_lw_jac.hip -- the longwave surface-temperature Jacobian, flux_up_jac(ncol,nlay+1) (include/ecckd_hip.h,
// "Longwave surface-temperature Jacobian"), as a kernel of its own next to the flux solvers.
//
// The Jacobian of the upward flux with respect to the surface temperature needs neither the layer sources nor the downward
// sweep: per g-point and angle it is the surface term  J = eps * sfc_source_jac  carried up through the transmissivities,
//     J(level above layer l) = t_k(l) * J(level below),      t_k(l) = lw_exp(-tau(l) * D_k),
// and summed over g-points and angles with the weights of flux_up.  t_k is formed with the flux solvers' own lw_exp
// (lw_layer.hpp) on the optical depth that the flux solver of the call sees, so the Jacobian belongs to the fluxes it
// comes with.
//
// Mapping (gfx950): one wave = one tile of 32 columns x 2 g-points (the lane layout of kernels_rte_lw_split.hip: column
// = lane % 32, g-point of the pair = lane / 32), one wave per block.  The wave walks its g-point pairs one after the other
// and, for each, the layers from the surface upwards ONCE for all angles: tau is read once (8 B per cell), column-fastest,
// kJacPF layers ahead of their use.  A level's value is summed over the pair by one shuffle and added by the lower half of
// the wave into the tile's accumulator in LDS ([level][column] doubles).  One wave owns its accumulators and adds the pairs
// in ascending order: the result does not depend on the grid or on timing.  Levels beyond what fits the LDS budget
// (more than 639 layers) are served in chunks of levels, each chunk by a walk of its own from the surface.
//
// Surface term: from sfc_source_jac(ncol,ng) (ecckd_rte_lw_jac), or -- PLANCK -- B(tsfc + 1) - B(tsfc) from the model's
// Planck table in global memory (two evaluations per (column, g-point), against nlay cells), the fused calls' form.
// SKY / MASK: the particulate optical depth on the model's bands and the McICA mask, applied to the gas optical depth by
// lw_cell_tau (lw_layer.hpp), the function rte_lw_split_body calls for the same cell (the 60-layer fused route, whose flux
// kernel leaves the scratch tau as gas optics wrote it).
// RESC: the rescaled solver's Jacobian (include/ecckd_hip.h, "Rescaled longwave: clear sky and Jacobian").  With every source
// zero the rescaled transport is J = t_k * J with t_k = lw_exp(-((tau * sc) * D_k)), sc = (1 - ssa) + (ssa * (1 - g)) * 0.5:
// tau * sc comes from lw_cell_rescaled (lw_layer.hpp), which the rescaled form of rte_lw_split_body calls too.  Two forms:
// arrays (SKY = 0: a.ssa and a.g beside a.tau, 24 B per cell -- ecckd_rte_lw_rescaled_jac and the fused general route, whose
// increment left the cell's triple in scratch), and SKY = 2 with a.part_g and the optional mask (the 60-layer fused route:
// the cell's triple from the gas optical depth and the band triple).
#include "kernels.hpp"
#include "lw_layer.hpp"
#include "planck_at.hpp"

namespace ecckd {
namespace {

constexpr int kJacCW = 32;   // columns per tile
constexpr int kJacGW = 2;    // g-points per wave
constexpr int kJacPF = 4;    // layers in flight per lane

// The kernel text, shared by rte_lw_jac_kernel (RESC = false) and rte_lw_rescaled_jac_kernel (RESC = true)
template <bool PLANCK, int SKY, bool MASK, bool RESC, class Args>
__device__ __forceinline__ void rte_lw_jac_body(const Args &a, const PlanckTab &pt) {
  static_assert(SKY != 0 || !MASK, "a cloud mask belongs to the all-sky form");
  static_assert(!RESC || SKY == 0 || SKY == 2, "the rescaled form reads the cell's (tau, ssa, g) or forms it from a two-stream band triple");
  constexpr int CW = kJacCW, GW = kJacGW, PF = kJacPF;
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  double *acc = reinterpret_cast<double *>(lds_raw);   // [levels of a chunk][CW]
  const int lane = threadIdx.x;
  const int cl = lane % CW, gs = lane / CW;
  const bool owner = gs == 0;
  const int ncol = a.ncol, nlay = a.nlay, ng = a.ng, nmus = a.nmus;
  const int nlev = nlay + 1, LC = a.lev_chunk;
  const double pi = acos(-1.);
  [[maybe_unused]] const double pi_f32 = (double)3.14159265359f, rpi_f32 = 1. / pi_f32;   // src/gas_optics_ecckd.f90:53
  const long ntiles = ((long)ncol + CW - 1) / CW;
  const int ngroups = (ng + GW - 1) / GW;
  // walking order: s = 0 is the surface level, layer s lies between the levels s and s + 1
  const long lay0 = a.top_at_1 ? nlay - 1 : 0, lev0 = a.top_at_1 ? nlay : 0;
  const long lstep = a.top_at_1 ? -1 : 1;
  const long qstep = (long)ncol * lstep;
  double wfac[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) wfac[k] = k < nmus ? 2. * pi * a.wts[k] : 0.;

  for (int i = lane; i < LC * CW; i += 64) acc[i] = 0.;
  __syncthreads();

  for (long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const long col = tile * CW + cl;
    const bool valid = col < ncol;
    const long cc = valid ? col : (long)ncol - 1;
    for (int c0 = 0; c0 < nlev; c0 += LC) {   // levels c0 .. c1-1 of the walk
      const int c1 = c0 + LC < nlev ? c0 + LC : nlev;
      for (int gi = 0; gi < ngroups; ++gi) {
        const int g = gi * GW + gs;
        const bool gact = g < ng;
        const int gg = gact ? g : ng - 1;
        const double eps = a.sfc_emis[a.gpt2band[gg] + (long)a.nband * cc];
        double jsfc;
        if (PLANCK) {
          const double ts = a.tsfc[cc];
          const double b0 = planck_at(pt, pt.tab, pt.ng, ts, gg, pi_f32, rpi_f32);
          const double b1 = planck_at(pt, pt.tab, pt.ng, ts + 1., gg, pi_f32, rpi_f32);
          jsfc = b1 - b0;
        } else {
          jsfc = a.sfc_source_jac[cc + (long)ncol * gg];
        }
        double J[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) J[k] = eps * jsfc;
        const double gw_ = gact ? 1. : 0.;   // a lane beyond the last g-point carries weight 0 (as in flux_up)

        auto level = [&](int s) {   // the wave's contribution to level s
          double v = 0.;
#pragma unroll
          for (int k = 0; k < 4; ++k)
            if (k < nmus) v = v + (gw_ * wfac[k]) * J[k];
          v = v + __shfl_xor(v, CW);
          if (s >= c0) __hip_atomic_fetch_add(&acc[(s - c0) * CW + cl], owner ? v : 0., __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        };

        long q2 = cc + (long)ncol * lay0;                // (column, layer) of the walk
        long qn = q2 + (long)ncol * nlay * gg;           // ... of the lane's g-point
        [[maybe_unused]] const long qb = SKY ? (long)ncol * nlay * a.gpt2band[gg] : 0;
        // loads of the layers s .. s+PF-1 in flight; a slot past the last layer repeats the last one (never used)
        double ptau[PF];
        [[maybe_unused]] double ppt[SKY ? PF : 1], pps[SKY == 2 ? PF : 1];
        [[maybe_unused]] unsigned long long pmk[MASK ? PF : 1];
        [[maybe_unused]] double pss[RESC && SKY == 0 ? PF : 1], pgg[RESC ? PF : 1];   // RESC: ssa(l) of the cell; g(l) of the cell or of the band
        int issued = 0;
        auto issue = [&](int slot) {
          ptau[slot] = __builtin_nontemporal_load(a.tau + qn);
          if (SKY) ppt[slot] = a.part_tau[q2 + qb];
          if (SKY == 2) pps[slot] = a.part_ssa[q2 + qb];
          if (MASK) pmk[slot] = a.part_mask[q2];
          if constexpr (RESC) {
            if constexpr (SKY == 0) {
              pss[slot] = __builtin_nontemporal_load(a.ssa + qn);
              pgg[slot] = __builtin_nontemporal_load(a.g + qn);
            } else {
              pgg[slot] = a.part_g[q2 + qb];
            }
          }
          ++issued;
          if (issued < nlay) { qn += qstep; q2 += qstep; }
        };
#pragma unroll
        for (int s = 0; s < PF; ++s) issue(s);

        const int nwalk = c1 - 1;   // layers 0 .. nwalk-1 lie below the chunk's last level
        for (int sb = 0; sb < nwalk; sb += PF) {
#pragma unroll
          for (int u = 0; u < PF; ++u) {
            const int s = sb + u;
            if (s < nwalk) {
              level(s);
              double tau = ptau[u];
              [[maybe_unused]] bool cloudy = true;
              if constexpr (MASK) cloudy = (pmk[u] >> gg) & 1ull;
              [[maybe_unused]] double Cn;   // (the rescaled fluxes' adjustment factor: not needed here)
              if constexpr (RESC && SKY == 2) lw_cell_rescaled<true>(ptau[u], ppt[u], pps[u], pgg[u], cloudy, tau, Cn);
              else if constexpr (RESC) lw_cell_rescaled<false>(ptau[u], 0., pss[u], pgg[u], true, tau, Cn);
              else if constexpr (SKY == 2) tau = lw_cell_tau<2>(ptau[u], ppt[u], pps[u], cloudy);
              else if constexpr (SKY == 1) tau = lw_cell_tau<1>(ptau[u], ppt[u], 0., cloudy);
              issue(u);
#pragma unroll
              for (int k = 0; k < 4; ++k) {
                if (k < nmus) {
                  const double tl = tau * a.Ds[k];
                  J[k] = lw_exp(-tl) * J[k];
                }
              }
            }
          }
        }
        level(nwalk);
      }
      // the chunk's levels of the tile: level s of the walk -> lev0 + lstep * s
      __syncthreads();
      for (int i = lane; i < (c1 - c0) * CW; i += 64) {
        const int s = i / CW, c = i - s * CW;
        const long cg = tile * CW + c;
        if (cg < ncol) a.flux_up_jac[cg + (long)ncol * (lev0 + lstep * (c0 + s))] = acc[i];
        acc[i] = 0.;
      }
      __syncthreads();
    }
  }
}

template <bool PLANCK, int SKY, bool MASK>
__global__ void __launch_bounds__(64) rte_lw_jac_kernel(const RteLwJacArgs a, const PlanckTab pt) {
  rte_lw_jac_body<PLANCK, SKY, MASK, false>(a, pt);
}

// ... of the rescaled solver, under its own name: SKY = 0 on arrays (tau, ssa, g), SKY = 2 on the gas optical depth and the
// two-stream band triple (MASK: and a McICA cloud mask)
template <bool PLANCK, int SKY, bool MASK>
__global__ void __launch_bounds__(64) rte_lw_rescaled_jac_kernel(const RteLwRescJacArgs a, const PlanckTab pt) {
  rte_lw_jac_body<PLANCK, SKY, MASK, true>(a, pt);
}

// sfc_source_jac(i,g) = B_g(tsfc(i) + 1) - B_g(tsfc(i)): one thread per (column, g-point), the table from global memory
__global__ void __launch_bounds__(256) planck_sfc_jac_kernel(const PlanckTab pt, int ncol, const double *tsfc, double *out) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)ncol * pt.ng) return;
  const int g = (int)(i / ncol);
  const long c = i - (long)g * ncol;
  const double pi_f32 = (double)3.14159265359f, rpi_f32 = 1. / pi_f32;   // src/gas_optics_ecckd.f90:53
  const double ts = tsfc[c];
  const double b0 = planck_at(pt, pt.tab, pt.ng, ts, g, pi_f32, rpi_f32);
  const double b1 = planck_at(pt, pt.tab, pt.ng, ts + 1., g, pi_f32, rpi_f32);
  out[i] = b1 - b0;
}

template <class Args>
hipError_t launch_jac_kernel(void (*k)(const Args, const PlanckTab), const Args &a, const PlanckTab &pt, hipStream_t s);

template <bool PLANCK>
hipError_t launch_resc_jac(const RteLwRescJacArgs &a, const PlanckTab &pt, hipStream_t s) {
  void (*k)(const RteLwRescJacArgs, const PlanckTab);
  if (a.ssa) k = rte_lw_rescaled_jac_kernel<PLANCK, 0, false>;   // on the cell's (tau, ssa, g)
  else k = a.part_mask ? rte_lw_rescaled_jac_kernel<PLANCK, 2, true> : rte_lw_rescaled_jac_kernel<PLANCK, 2, false>;
  return launch_jac_kernel(k, a, pt, s);
}

template <bool PLANCK>
hipError_t launch_jac(const RteLwJacArgs &a, const PlanckTab &pt, hipStream_t s) {
  void (*k)(const RteLwJacArgs, const PlanckTab);
  const bool two = a.part_tau && a.part_ssa;
  if (a.part_tau && a.part_mask) k = two ? rte_lw_jac_kernel<PLANCK, 2, true> : rte_lw_jac_kernel<PLANCK, 1, true>;
  else if (a.part_tau) k = two ? rte_lw_jac_kernel<PLANCK, 2, false> : rte_lw_jac_kernel<PLANCK, 1, false>;
  else k = rte_lw_jac_kernel<PLANCK, 0, false>;
  return launch_jac_kernel(k, a, pt, s);
}

template <class Args>
hipError_t launch_jac_kernel(void (*k)(const Args, const PlanckTab), const Args &a, const PlanckTab &pt, hipStream_t s) {
  Args b = a;
  const int max_lev = kLdsBudget / (int)(sizeof(double) * kJacCW);
  b.lev_chunk = a.nlay + 1 < max_lev ? a.nlay + 1 : max_lev;
  const size_t lds = sizeof(double) * (size_t)b.lev_chunk * kJacCW;
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  long blocks = ((long)a.ncol + kJacCW - 1) / kJacCW;
  const long cap = 256L * 64;   // beyond that a block walks tiles by grid stride
  if (blocks > cap) blocks = cap;
  hipLaunchKernelGGL(k, dim3((unsigned)blocks), dim3(64), lds, s, b, pt);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_rte_lw_jac(const RteLwJacArgs &a, const double *planck, int ntp, double t0, double dt, hipStream_t s) {
  if (a.ncol <= 0) return hipSuccess;
  if (a.nlay < 1 || a.ng < 1 || a.nmus < 1 || a.nmus > 4 || !a.tau || !a.sfc_emis || !a.flux_up_jac) return hipErrorInvalidValue;
  if (a.part_mask && (!a.part_tau || a.ng > 64)) return hipErrorInvalidValue;
  if (a.sfc_source_jac) return launch_jac<false>(a, PlanckTab{nullptr, 0., 1., 1., 2, a.ng}, s);
  if (!a.tsfc || !planck) return hipErrorInvalidValue;
  return launch_jac<true>(a, PlanckTab{planck, t0, dt, 1. / dt, ntp, a.ng}, s);
}

hipError_t launch_rte_lw_rescaled_jac(const RteLwRescJacArgs &a, const double *planck, int ntp, double t0, double dt, hipStream_t s) {
  if (a.ncol <= 0) return hipSuccess;
  if (a.nlay < 1 || a.ng < 1 || a.nmus < 1 || a.nmus > 4 || !a.tau || !a.sfc_emis || !a.flux_up_jac) return hipErrorInvalidValue;
  // ssa and g together and without particles, or part_g with part_tau and part_ssa (and a mask of at most 64 g-points)
  if (a.ssa ? (!a.g || a.part_tau || a.part_ssa || a.part_g || a.part_mask) : (a.g || !a.part_tau || !a.part_ssa || !a.part_g))
    return hipErrorInvalidValue;
  if (a.part_mask && a.ng > 64) return hipErrorInvalidValue;
  if (a.sfc_source_jac) return launch_resc_jac<false>(a, PlanckTab{nullptr, 0., 1., 1., 2, a.ng}, s);
  if (!a.tsfc || !planck) return hipErrorInvalidValue;
  return launch_resc_jac<true>(a, PlanckTab{planck, t0, dt, 1. / dt, ntp, a.ng}, s);
}

hipError_t launch_planck_sfc_jac(const double *planck, int ng, int ntp, double t0, double dt, int ncol, const double *tsfc,
                                 double *sfc_source_jac, hipStream_t s) {
  if (ncol <= 0) return hipSuccess;
  const PlanckTab pt{planck, t0, dt, 1. / dt, ntp, ng};
  const long n = (long)ncol * ng;
  hipLaunchKernelGGL(planck_sfc_jac_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, pt, ncol, tsfc, sfc_source_jac);
  return hipGetLastError();
}

}  // namespace ecckd
