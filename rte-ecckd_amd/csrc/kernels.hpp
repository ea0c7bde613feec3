// kernels.hpp -- launch interface between the C ABI (capi.cpp) and the gfx950 kernels.
// All pointers are device pointers on the current device; every array is column-major with the
// column index fastest (the reference's layout, src/gas_optics_ecckd.f90:69-72).
#pragma once
#include <hip/hip_runtime.h>

namespace ecckd {

constexpr int kMaxSeq = 16;          // src/gas_optics_ecckd.f90:24 (at most 16 tables)
constexpr int kTauPassGases = 10;    // gases one tau launch accumulates (more -> another pass)
constexpr int kLdsBudget = 160 * 1024;

// One entry of the per-call gas sequence: a table of the model matched to a gas of gas_desc,
// in gas_desc order (src/gas_optics_ecckd.f90:348-374).
struct SeqGas {
  const double *coef;     // (ng,np,nt,nv) table in device memory
  const double *vmr;      // device pointer or nullptr -> scalar
  long long cs, ls;       // vmr(i,l) = vmr[i*cs + l*ls]
  double scalar;
  double ref;             // reference_mole_fraction (relative_linear)
  double mf0;             // mole_fraction(1)                       (look_up_table)
  double log_mf0;         // log(mole_fraction(1))                  (host libm, as the reference)
  double d_log_vmr;       // log(mole_fraction(2)/mole_fraction(1)) (host libm)
  int code;               // ECCKD_NONE / LINEAR / LOOK_UP_TABLE / RELATIVE_LINEAR
  int nv;
  int slot;               // bilinear: slot inside a slab row; LUT: unused
  int clamp;              // 1 if the table holds negative coefficients -> per-g clamp needed
};

struct TauArgs {
  int ncol, nlay, ng, np, nt;
  const double *plev, *tlay;
  const double *temperature;   // (np,nt) device; only T(:,1) is used (:131-132)
  const double *zero;          // a zero word of the model's device image (loads of unused / scalar gas slots)
  double lp0, dlp, dt, gw;     // :104-107
  int nseq;
  SeqGas seq[kMaxSeq];
  int nbil;                    // bilinear gases in this pass (slab row holds nbil*ng values)
  int bil_seq[kMaxSeq];        // slab slot -> index into seq
  int lut;                     // index into seq of the look_up_table gas, or -1
  // Merged slot (fused kernel, fast arithmetic; merge_scalar_gases()): the gases of this pass whose mole fraction is one
  // number for the whole call -- scalar entries of gas_desc and the none_ composite -- share ONE slab slot holding
  // sum_k merge_mult[k] * coefficient_k, built while the slab is staged; its weight is simple_weight alone.
  int merge_slot;              // slab slot of the merged table, or -1
  int nmerge;                  // gases in it (0 or >= 2)
  int merge_seq[kMaxSeq];      // their indices into seq, in gas_desc order
  double merge_mult[kMaxSeq];  // vmr, vmr - reference, or 1 (none_): >= 0, finite, rounded to the working precision
  int accumulate;              // start from the tau already in memory (later passes)
  double *tau;
  // shortwave epilogue (src/gas_optics_ecckd.f90:455-460); rayleigh == nullptr for LW
  const double *rayleigh;
  double *ssa, *g;
  // launch geometry chosen by the host
  int R;                       // pressure rows of the LDS slab
  int col_chunks;              // grid.x; each block walks tiles chunk by chunk
  int seg;                     // fused kernel: tiles per segment (slab-range pre-pass + barriers once per segment)
};

// Division by a wave-uniform constant, d with its reciprocal (kernels_gas_fused.hip: udiv()).
struct UDiv { double d, r; int exact; };

// Per-slot view of the gases of a pass for the fused kernel: slot s < nbil is the s-th bilinear
// gas, slot kTauPassGases is the look_up_table gas.  `vmr` is ALWAYS a valid device address (the
// load is issued unconditionally, all slots in one round; slots without an array read TauArgs::zero, a
// word the model owns, so that a NaN in the caller's arrays stays in its own column).  The mole fraction that enters the
// weight is fma(alpha, loaded, beta) with alpha in {0, 1}, which spells every case of
// src/gas_optics_ecckd.f90:143-149 exactly: array/linear (1, 0); array/relative_linear (1, -ref);
// scalar/linear (0, scalar); scalar/relative_linear (0, scalar - ref); none_ (0, 1); unused (0, 0).
struct SlotArgs {
  const double *vmr;
  long long ls;                // layer stride, elements
  unsigned cs_bytes;           // column stride, bytes (32-bit: checked on the host)
  double alpha, beta;
};

// Fused gas-optics launch (kernels_gas_fused.hip): the tau arguments plus the Planck side.
struct FusedArgs {
  TauArgs tau;
  UDiv ud_dlp, ud_dt, ud_dlv, ud_pdt;          // filled by launch_gas_fused
  SlotArgs slot[kTauPassGases + 1];            // filled by launch_gas_fused
  int f32;                     // 1: every data pointer addresses float arrays (LW fused path only)
  int slab32;                  // fp64 call: stage the tables in LDS as the float32 they are (model checked: every value is
                               // float32-representable): 1 always, 2 where the columns are spread over many pressure rows
                               // (spread probe); prepare_gas_fused clears it where no such instantiation exists
  int *choose_buf;             // slab32 == 2: one int of device memory owned by the call's stream (the probe's counter), or null
  const int *choose;           // (set by launch_gas_fused) the probe's counter, or null: unconditional launch
  int choose_total;            // (set by launch_gas_fused) waves of 64 columns in the call
  int mode;                    // 0 tau only, 1 longwave (tau + Planck sources), 2 shortwave epilogue
  int tile_sync;               // "gas_tile_sync": 1 = the waves of a block meet at an execution barrier before every tile
  int input_ahead;             // "gas_input_ahead": 1 = a wave loads the per-column inputs of its next tile before the chunk loops
                               // of the tile in hand (512-thread instantiations; the others ignore it)
  int ntp;
  int pw;                      // Planck rows staged in LDS (ntp, or a window); filled by launch_gas_fused
  const double *planck;        // (ng,ntp) device
  double pt0, pdt;             // temperature_planck(1), (2)-(1)
  const double *tlev, *tsfc;   // tlev may be nullptr
  double *lay_source, *lev_source_inc, *lev_source_dec, *sfc_source;
  long long lev_gstride;       // g-plane stride of the two level arrays, elements: nlay*ncol for separate arrays (0 means that),
                               // (nlay+1)*ncol for the two views of one level buffer (include/ecckd_hip.h, "Level buffer"):
                               // lev_source_inc == lev_source_dec + ncol, and each level is stored once
  int wave_roles;              // "gas_wave_roles": 1 = gas_roles_kernel (kernels_gas_roles.hip: tau waves and source waves share a
                               // block) where it exists, -1 = where it is the default of the shape; prepare_gas_fused resolves it
                               // to 0 or 1 (fp64 longwave over the fp64 slab, the shapes of gas_roles_applies)
};

struct PlanckArgs {
  int ncol, nlay, ng, ntp;
  const double *planck;        // (ng,ntp) device
  double t0, dt;               // temperature_planck(1), (2)-(1)   (:271-272)
  const double *tlay, *tlev, *tsfc;    // tlev may be nullptr
  double *lay_source, *lev_source_inc, *lev_source_dec, *sfc_source;
  int lev_chunks;              // grid.y
  long long lev_gstride;       // as FusedArgs::lev_gstride
};

struct RteLwArgs {
  int ncol, nlay, ng, top_at_1, nmus;
  double Ds[4], wts[4];
  const double *tau, *lay_source, *lev_source_inc, *lev_source_dec, *sfc_source;
  const double *sfc_emis;      // (nband,ncol)
  int nband;
  unsigned char gpt2band[256]; // 0-based band of each g-point
  double *flux_up, *flux_dn;
  double *scratch;             // generic-nlay path only
  int f32;                     // 1: the data pointers address float arrays
  int shared_levels;           // 1: lev_source_inc(:,l,:) == lev_source_dec(:,l+1,:): each level is read once
  long long lev_gstride = 0;   // g-plane stride of the two level arrays, elements: nlay*ncol (0 means that), or (nlay+1)*ncol
                               // for the two views of one level buffer (then shared_levels is set: only those kernels take it)
  const double *inc_flux;      // (ncol,ng) incident diffuse flux at the top of the domain, or nullptr (none)
  // version switches of the un-pinned RTE-RRTMGP solver (ecckd_set_solver_option)
  double tau_thresh;           // lw_source_noscat: series below this optical depth (sqrt(epsilon) of the precision)
  int series3;                 // 0: tau*(0.5 - tau/3) (v1.5), 1: tau*(0.5 + tau*(-1/3 + tau/8))
  int inc_isotropic;           // 0: I_dn(top) = inc_flux/(2 pi w_k) per angle, 1: inc_flux/pi
  // implementation choice for fp64 / 60 layers (ecckd_set_solver_option "lw_solver", "lw_split_seg")
  int use_split;               // 1: layer-split solver (kernels_rte_lw_split.hip), 0: register-resident solver
  int split_seg;               // layers per wave of the layer-split solver: 10, 12 or 15
  // tail split (rte_lw_tail_plan): tiles from tail_first on are solved one g-pair iteration per wave; -1: none
  long tail_first = -1;
  double *partials = nullptr;  // [tail tile][iteration][dn, up][nlay+1][columns per tile]
  // Fused all-sky longwave path (ecckd_lw_fluxes_allsky; launch_rte_lw_planck only): the particulate optical properties of
  // the layer on the model's bands, part_tau / part_ssa (ncol,nlay,nband), are added to the gas optical depth inside the
  // solver: tau + part_tau * (1 - part_ssa), or tau + part_tau with part_1scl (one-stream particles; part_ssa unused) --
  // RTE-RRTMGP's increment_1scalar_by_2stream / _by_1scalar, spelt as in kernels_optical_props.hip
  const double *part_tau = nullptr, *part_ssa = nullptr;
  int part_1scl = 0;
  // McICA (ecckd_lw_fluxes_allsky_mcica): one word per (column, layer), bit g set = g-point g sees the layer's particles;
  // where it is clear the cell uses part_tau = 0.  Null: every g-point sees them (the unmasked kernels).
  const unsigned long long *part_mask = nullptr;
  // Rescaled no-scattering solver (launch_rte_lw_rescaled_split / _planck only; include/ecckd_hip.h, "Rescaled longwave"):
  // ssa / g (ncol,nlay,ng) beside tau, or -- the Planck-recomputing form -- part_g beside part_tau / part_ssa
  const double *ssa = nullptr, *g = nullptr, *part_g = nullptr;
};

// Longwave surface-temperature Jacobian (kernels_rte_lw_jac.hip): flux_up_jac(ncol,nlay+1) from tau, the surface term and
// the quadrature of the flux solver.  The surface term is sfc_source_jac(ncol,ng), or -- null -- formed in the kernel from
// tsfc(ncol) and the model's Planck table.  part_tau / part_ssa / part_mask: as in RteLwArgs (the fused 60-layer route,
// where the flux kernel adds the particles as it reads tau); null: tau is the optical depth the solver saw.
struct RteLwJacArgs {
  int ncol, nlay, ng, top_at_1, nmus;
  double Ds[4], wts[4];
  const double *tau;
  const double *sfc_source_jac, *tsfc;
  const double *sfc_emis;      // (nband,ncol)
  int nband;
  unsigned char gpt2band[256]; // 0-based band of each g-point
  const double *part_tau = nullptr, *part_ssa = nullptr;
  const unsigned long long *part_mask = nullptr;
  double *flux_up_jac;
  int lev_chunk = 0;           // (set by the launcher) levels whose accumulators one block holds in LDS
};
hipError_t launch_rte_lw_jac(const RteLwJacArgs &a, const double *planck, int ntp, double t0, double dt, hipStream_t s);
// ... of the rescaled solver (include/ecckd_hip.h, "Rescaled longwave: clear sky and Jacobian"): ssa / g (ncol,nlay,ng) beside
// tau, or part_g beside part_tau / part_ssa (tau is the gas optical depth; part_mask optional) -- the transmissivity is that
// of tau * ((1 - ssa) + (ssa * (1 - g)) * 0.5).  An argument block of its own: the kernels above keep theirs.
struct RteLwRescJacArgs : RteLwJacArgs {
  const double *ssa = nullptr, *g = nullptr, *part_g = nullptr;
};
hipError_t launch_rte_lw_rescaled_jac(const RteLwRescJacArgs &a, const double *planck, int ntp, double t0, double dt, hipStream_t s);
// sfc_source_jac(ncol,ng) = B(tsfc + 1) - B(tsfc) from the model's table planck(ng,ntp)
hipError_t launch_planck_sfc_jac(const double *planck, int ng, int ntp, double t0, double dt, int ncol, const double *tsfc,
                                 double *sfc_source_jac, hipStream_t s);

struct RteSwArgs {
  int ncol, nlay, ng, top_at_1;
  const double *tau, *ssa, *g, *mu0, *toa;
  const double *alb_dir, *alb_dif;   // (nband,ncol)
  int nband;
  unsigned char gpt2band[256];
  double *flux_up, *flux_dn, *flux_dir;   // flux_dir may be nullptr
  double *scratch;
  int exact_division;          // 1 (reference-order arithmetic mode): IEEE `/`; 0: reciprocal + Newton steps
  // version switches (ecckd_set_solver_option)
  double k_floor;              // lower bound of (gamma1-gamma2)(gamma1+gamma2) under the square root (1e-12)
  double k_floor_tau = 0.;     // > 0 (single precision, default floor): a cell's bound is min(k_floor, k_floor_tau / tau^2)
  int dir_clamp;               // 1: Rdir/Tdir energy clamps of later RTE-RRTMGP releases
  // tail split (rte_sw_tail_plan): tiles from tail_first on are solved one g-point group per wave; -1: none
  long tail_first = -1;
  double *partials = nullptr;  // [tail tile][group][up, dn, dir][nlay+1][columns per tile]
  int f32 = 0;                 // 1: the data pointers address float arrays (layer-systolic solver only)
  // Layer-systolic solver (kernels_rte_sw_sys.hip; rte_sw_sys_applies()): tiles of 64 columns; tiles from sys_tail_first
  // on are solved in chunks of sys_gchunk g-points per block, the chunk sums go through `partials`
  // ([tail tile][chunk][up, dn, dir][nlay+1][64]) and are added in chunk order by rte_sw_tail_reduce.
  int use_sys = 0;
  long sys_tail_first = -1;
  int sys_gchunk = 0;
  int sys_npark = 0;           // (set by the launcher) lower waves that park the next g-point's coefficients in LDS
  unsigned sys_park_at = 0;    // (set by the launcher) byte offset of the parking areas in the block's LDS
  // Fused shortwave path (ecckd_sw_fluxes): `tau` is the total optical depth and nothing else is read per cell --
  // ssa = (moles*rayleigh(g))/tau with moles = (plev(l+1)-plev(l))*gw, g = 0, toa = solar(g): gas_optics_ext's own
  // expressions (src/gas_optics_ecckd.f90:313-317,455-472).  derive != 0 selects it; ssa / g / toa are then unused.
  int derive = 0;
  const double *plev = nullptr, *rayleigh = nullptr, *solar = nullptr;   // plev(ncol,nlay+1) device; (ng) device tables
  const double *toa_scale = nullptr;   // (ncol) or null: toa(i,g) = solar(g)*toa_scale(i), the driver's TSI rescaling (ecckd_rfmip_sw.F90:126-133)
  double gw = 0.;
  // Fused all-sky shortwave path (ecckd_sw_fluxes_allsky; derive != 0 as well): the particulate optical properties of the
  // layer on the model's bands, part_tau / part_ssa / part_g (ncol,nlay,nband), are added to the gas optics inside the
  // solver with the expressions of RTE-RRTMGP's increment_2stream_by_2stream (see kernels_optical_props.hip)
  int allsky = 0;
  const double *part_tau = nullptr, *part_ssa = nullptr, *part_g = nullptr;
  // McICA (ecckd_sw_fluxes_allsky_mcica): as RteLwArgs::part_mask.  In the same storage (so that the kernels of the calls
  // above keep their argument block), mask_window = 2 (ecckd_sw_flux_scaled; two-pass solver, fp64): the sampled
  // optical-depth scaling, float32 (ncol,nlay,ng); the cell's particulate optical depth is part_tau * scaling in front of
  // the all-sky expressions
  union {
    const unsigned long long *part_mask = nullptr;
    const float *part_scaling;
  };
  // Band window (ecckd_sw_flux_bands; fp64, with part_mask): the launch covers the g-points mask_first .. mask_first + ng - 1
  // of the model -- tau, rayleigh, solar and the outputs are that band's own -- and g-point g of the launch sees bit
  // mask_first + g of the mask word.  mask_window = 0: bit g (the kernels of the calls above).
  int mask_window = 0, mask_first = 0;
};

// Two-stream longwave solver (kernels_rte_lw_2str.hip): clouds scatter.  tau / ssa / g / lev_source_* (ncol,nlay,ng),
// sfc_source(ncol,ng), sfc_emis(nband,ncol), inc_flux(ncol,ng) or null; fp64.  lay_source is not an argument: RTE-RRTMGP's
// lw_solver_2stream never reads it.
struct RteLw2strArgs {
  int ncol, nlay, ng, top_at_1;
  const double *tau, *ssa, *g, *lev_source_inc, *lev_source_dec, *sfc_source;
  const double *sfc_emis;      // (nband,ncol)
  int nband;
  unsigned char gpt2band[256]; // 0-based band of each g-point
  const double *inc_flux;
  double *flux_up, *flux_dn;
  double *scratch;             // per-wave ring [2][nlay+1][64]: rte_lw_2str_scratch_bytes
  int exact_division;          // 1 (reference-order arithmetic mode): IEEE `/`, sqrt, exp; 0: rcp / sw_sqrt / sw_exp
  // Fused all-sky path (ecckd_lw_fluxes_allsky_2stream): `tau` is the gas optical depth, ssa / g are not read; the layer's
  // particulate triple on the cell's band, part_* (ncol,nlay,nband), is added where the cell's properties are formed, with
  // the operations of the by-band increment_2stream_by_2stream on op1 = (tau, 0, 0) (kernels_optical_props.hip)
  const double *part_tau = nullptr, *part_ssa = nullptr, *part_g = nullptr;
  const unsigned long long *part_mask = nullptr;   // as RteLwArgs::part_mask (ng <= 64)
};
size_t rte_lw_2str_scratch_bytes(int ncol, int nlay, int ng);
hipError_t launch_rte_lw_2str(const RteLw2strArgs &a, hipStream_t s);
// ... in single precision (ecckd_rte_lw_2stream_f32, ecckd_lw_fluxes_allsky_2stream_f32): float arrays behind every data
// pointer of the same argument block, the mask excepted; fast arithmetic mode only; the ring, in floats, takes the first
// half of rte_lw_2str_scratch_bytes
hipError_t launch_rte_lw_2str_f32(const RteLw2strArgs &a, hipStream_t s);

// Element-wise operations on optical properties (kernels_optical_props.hip): RTE-RRTMGP's delta_scale_2str_k / _f_k and
// the increment_* kernels (by g-point and by band).  Arrays (ncol,nlay,n), column fastest; f32: float data behind the pointers.
struct OptPropsArgs {
  int ncol, nlay, ng;
  int nband;                   // 0: op2 on the same ng points; > 0: op2 is (ncol,nlay,nband)
  int f32;
  double *tau1, *ssa1, *g1;    // ssa1 / g1 null: op1 is one-stream
  const double *tau2, *ssa2, *g2;   // ssa2 / g2 null: op2 is one-stream
  unsigned short band_first[257];   // nband > 0: band b covers the 0-based g-points [band_first[b], band_first[b+1])
  // ecckd_increment_masked: one word per (column, layer), bit g clear = the cell is incremented as if tau2 were +0 there
  // (ng <= 64); null: the unmasked kernels
  const unsigned long long *mask = nullptr;
  // ecckd_increment_scaled: float32 (ncol,nlay,ng) whatever the precision of the call; the g-point is incremented by
  // tau2 * scaling, the products formed per g-point (any ng); null: the kernels above.  Not together with `mask`.
  const float *scaling = nullptr;
};
// eps = 3 * tiny(1._wp): the floor of the denominators in those kernels (and where the all-sky solver forms ssa and g)
template <typename real> __host__ __device__ constexpr real op_eps() {
  return sizeof(real) == 4 ? real(3) * real(1.17549435e-38f) : real(3) * real(2.2250738585072014e-308);
}
hipError_t launch_increment(const OptPropsArgs &a, hipStream_t s);
// (tau, ssa, g) of n cells delta-scaled into (tau_out, ssa_out, g_out) -- the same pointers for the in-place call;
// forward: the forward-scattering fraction f per cell, or null: f = g*g
hipError_t launch_delta_scale(size_t n, const double *tau, const double *ssa, const double *g, const double *forward, double *tau_out,
                              double *ssa_out, double *g_out, int f32, hipStream_t s);

// Cloud optics (kernels_cloud_optics.hip; the definition is in include/ecckd_hip.h, ecckd_cloud_optics): water paths and
// effective radii (ncol,nlay) to band planes (ncol,nlay,nband).  A table row is nsize-1 (value, slope) pairs of the call's
// precision, slope[i] = table[i+1] - table[i]; a phase's image is [quantity: ext, ssa, asy][band][nsize-1] pairs.
template <typename real> struct alignas(2 * sizeof(real)) CloudLutPair { real value, slope; };
constexpr size_t kCloudOpticsLdsBytes = 32768;   // both images at most this large: staged in LDS; else read through L2
struct CloudOpticsArgs {
  int ncol, nlay, nband, f32;
  int cus;                         // compute units of the device (sizes the grid); 0: 256
  int nsize_liq, nsize_ice;
  double radliq_lwr, radliq_step, radice_lwr, radice_step;   // (f32: float values, exactly representable here)
  const void *lut_liq, *lut_ice;   // device images in the call's precision; lut_ice: the chosen roughness
  const double *clwp, *ciwp, *reliq, *reice;
  double *tau, *ssa, *g;           // ssa and g null: the one-scalar form
};
// bytes of both images as the kernel stages them (the one-scalar form leaves the asymmetry rows out)
size_t cloud_optics_image_bytes(int nband, int nsize_liq, int nsize_ice, bool two_stream, bool f32);
hipError_t launch_cloud_optics(const CloudOpticsArgs &a, hipStream_t s);

// Aerosol optics (kernels_aerosol_optics.hip; the definition is in include/ecckd_hip.h, ecckd_aerosol_optics): type, size,
// mass (ncol,nlay,nspec) and relative humidity (ncol,nlay) to band planes (ncol,nlay,nband), written or -- accumulate --
// added with ecckd_increment's operations.  The image is [quantity: ext, ssa, asy][band][entry] pairs of the call's
// precision; the entries of a row: dust[nbin], salt[nbin][nrh-1], sulfate[nrh-1], hydrophilic black carbon[nrh-1],
// hydrophilic organic carbon[nrh-1], hydrophobic black carbon, hydrophobic organic carbon.  The head: rh_levels[nrh],
// d[nrh-1] = levels[i+1] - levels[i], bin_lims[2*nbin], in the call's precision.
__host__ __device__ constexpr int kAoEntries(int nbin, int nrh) { return nbin * nrh + 3 * (nrh - 1) + 2; }
constexpr size_t kAerosolOpticsLdsBytes = kCloudOpticsLdsBytes;   // the image at most this large: staged in LDS; else L2
constexpr int kAoMaxRegisterSpecies = 16;  // more species per call take the compatibility instantiation (ns = 0 below)
// resident blocks of 256 threads per CU (= waves per SIMD the kernel is compiled for) with ns species slots in registers
__host__ __device__ constexpr int kAoBlocksPerCu(int ns) { return ns >= 1 && ns <= 2 ? 8 : ns <= 8 ? 4 : 2; }
struct AerosolOpticsArgs {
  int ncol, nlay, nband, nspec, f32, accumulate;
  int cus;                         // compute units of the device (sizes the grid); 0: 256
  int nbin, nrh;
  const void *head, *image;        // device, in the call's precision
  const int *type;
  const double *size, *mass, *relhum;
  double *tau, *ssa, *g;           // ssa and g null: the one-scalar form
};
// bytes of the image as the kernel stages it (the one-scalar form leaves the asymmetry rows out)
size_t aerosol_optics_image_bytes(int nband, int nbin, int nrh, bool two_stream, bool f32);
// blocks of 256 threads the call launches: what is resident, at most one block per 256 cells (lds_image_bytes 0: L2 route)
unsigned aerosol_optics_grid(int ncol, int nlay, int nspec, int cus, size_t lds_image_bytes);
hipError_t launch_aerosol_optics(const AerosolOpticsArgs &a, hipStream_t s);

// Heating rates (kernels_heating_rate.hip; the definition is in include/ecckd_hip.h, ecckd_heating_rate): fluxes
// (ncol,nlay+1,nouter) and pressures (ncol,nlay+1) to the temperature tendency (ncol,nlay,nouter) in K s-1.
struct HeatingRateArgs {
  int ncol, nlay, nouter, f32;
  int cus;                         // compute units of the device (sizes the grid); 0: 256
  double grav, cp_dry;             // (f32: float values, exactly representable here)
  const double *flux_up, *flux_dn, *plev;
  const double *cp;                // (ncol,nlay), or null: cp_dry in every cell
  double *heating_rate;
};
// blocks of 256 threads the call launches: what is resident, at most one block per (256 columns, outer plane)
unsigned heating_rate_grid(int ncol, int nouter, int cus);
hipError_t launch_heating_rate(const HeatingRateArgs &a, hipStream_t s);

// McICA cloud mask (kernels_cloud_sampling.hip; the definition is in include/ecckd_hip.h, ecckd_cloud_mask_sample):
// cloud_frac (ncol,nlay), overlap_param (ncol,nlay-1; exp_ran only), mask (ncol,nlay); 1 <= ngpt <= 64
hipError_t launch_cloud_mask_sample(int ncol, int nlay, int ngpt, int exp_ran, const double *cloud_frac, const double *overlap_param,
                                    unsigned long long seed, long long col0, unsigned long long *mask, hipStream_t s);
// Sampled optical-depth scaling (same file; the definition is in include/ecckd_hip.h, ecckd_cloud_scaling_sample): the
// ranks of launch_cloud_mask_sample, read as the position inside the cloud, through the table values(nfsd,nq) (device,
// q fastest) at the cell's fsd(ncol,nlay) -- null: fsd_const everywhere -- to scaling (ncol,nlay,ngpt) float32; mask
// (ncol,nlay) or null.  A table of at most kCloudOpticsLdsBytes is staged in LDS, a larger one is read through L2.
struct CloudScalingArgs {
  int ncol, nlay, ngpt, exp_ran;
  const double *cloud_frac, *overlap_param, *fsd;
  double fsd_const;
  int nfsd, nq;
  double fsd0, dfsd;
  const double *values;
  unsigned long long seed;
  long long col0;
  float *scaling;
  unsigned long long *mask;
};
hipError_t launch_cloud_scaling_sample(const CloudScalingArgs &a, hipStream_t s);

// Spectral-output solvers (kernels_rte_gpt.hip): RTE-RRTMGP's kernel-level interfaces.  LW uses tau, lay_source,
// lev_source_*, sfc_emis(ncol,ng), sfc_src(ncol,ng), inc_flux(ncol,ng)|null, Ds/wts; SW uses tau, ssa, g, mu0(ncol),
// fdir_top(ncol,ng) (direct flux at the top = toa*mu0), inc_dif(ncol,ng)|null, alb_dir/alb_dif(ncol,ng).
// flux_up / flux_dn / flux_dir are (ncol,nlay+1,ng).
struct RteGptArgs {
  int ncol, nlay, ng, top_at_1, nmus;
  double Ds[4], wts[4];
  const double *tau, *lay_source, *lev_source_inc, *lev_source_dec, *sfc_emis, *sfc_src, *inc_flux;
  const double *ssa, *g, *mu0, *fdir_top, *inc_dif, *alb_dir, *alb_dif;
  double *flux_up, *flux_dn, *flux_dir;
  double tau_thresh, k_floor;
  int series3, inc_isotropic, dir_clamp;
};
hipError_t launch_lw_gpt(const RteGptArgs &a, hipStream_t s);
hipError_t launch_sw_gpt(const RteGptArgs &a, hipStream_t s);
// lw_solver_2stream: tau, ssa, g, lev_source_*, sfc_emis / sfc_src / inc_flux (ncol,ng); lay_source is not read
hipError_t launch_lw_2str_gpt(const RteGptArgs &a, hipStream_t s);
// lw_solver_1rescl_GaussQuad (the rescaled no-scattering solver), spectral fluxes: the compatibility kernel of
// ecckd_lw_solver_1rescl_gpt and of ecckd_rte_lw_rescaled away from 60 layers.  sfc_emis is (ncol,ng), or -- nband > 0 --
// (nband,ncol) read through gpt2band.  work (ncol,nlay+1,ng): the radiances one sweep leaves for the next.
struct RteLwRescGptArgs {
  int ncol, nlay, ng, top_at_1, nmus;
  double Ds[4], wts[4];
  const double *tau, *ssa, *g, *lay_source, *lev_source_inc, *lev_source_dec, *sfc_emis, *sfc_src, *inc_flux;
  int nband;
  unsigned char gpt2band[256];
  double *flux_up, *flux_dn, *work;
  double tau_thresh;
  int series3, inc_isotropic;
};
hipError_t launch_lw_1rescl_gpt(const RteLwRescGptArgs &a, hipStream_t s);

// Host-side helpers -------------------------------------------------------------------------
int tau_slab_rows(int ng, int np, int nt, int nbil, int nv_lut);   // R that fits LDS (>= 0)
size_t tau_lds_bytes(int ng, int np, int nt, int nbil, int nv_lut, int R);
size_t rte_lw_scratch_bytes(int ncol, int nlay, int ng);
size_t rte_lw_tail_plan(const RteLwArgs &a, int slots, long *tail_first);
size_t rte_sw_scratch_bytes(int ncol, int nlay, int ng);
size_t rte_sw_tail_plan(const RteSwArgs &a, long *tail_first, size_t *partials_at);

hipError_t launch_tau(TauArgs &a, hipStream_t s);
// What prepare_gas_fused() decided for one pass.
struct FusedPlan {
  int empty = 0;               // ncol == 0: nothing to launch
  size_t lds_bytes = 0;
  int anyclamp = 0, GC = 0, NB = 0;
  int merged = 0;              // gases sharing the merged slot
  int slab_rows = 0, planck_rows = 0, col_chunks = 0;
};
hipError_t prepare_gas_fused(FusedArgs &a, FusedPlan &plan);
// Folds the call-constant gases of a pass into one slot (TauArgs::merge_*); rewrites nbil / bil_seq.  Returns the number
// of gases merged (0: nothing changed).  Only for the fused kernel (the reference-order kernels take each gas alone).
int merge_scalar_gases(TauArgs &t, int f32);
int fused_slab_rows(int ng, int np, int nt, int nbil, int nv_lut, int pl_rows, int min_rows, int anyclamp, int f32, int block = 0);   // block: threads per block (0: the default 512)
int fused_planck_rows(int ng, int np, int nt, int nbil, int nv_lut, int ntp, int anyclamp, int f32);
hipError_t launch_gas_fused(FusedArgs &a, hipStream_t s);
// gas_roles_kernel (kernels_gas_roles.hip), the wave-roles form of the fp64 longwave launch: is there an instantiation for
// (g-points per chunk, bilinear slots); is it that shape's default ("gas_wave_roles" = -1: decided by measurement,
// profiles/gas_wave_roles.json); the launch itself (a prepared by prepare_gas_fused with wave_roles = 1)
bool gas_roles_applies(int GC, int NB);
bool gas_roles_default(int GC, int NB);
hipError_t launch_gas_roles(const FusedArgs &a, int GC, int NB, size_t lds_bytes, hipStream_t s);
// planck_edge_kernel (kernels_planck.hip): the sources of a fused longwave launch that belong to no layer -- sfc_source and,
// with tlev, lev_source_dec of storage layer 0; launch_gas_fused calls it once per longwave call, on the same stream
hipError_t launch_planck_edge(const FusedArgs &a, hipStream_t s);
hipError_t launch_planck(PlanckArgs &a, hipStream_t s);
// the Planck sources as a stand-alone fast kernel (paired 16-byte stores)
hipError_t launch_planck_pair(const PlanckArgs &a, int f32, hipStream_t s);
size_t planck_pair_lds_bytes(int ng, int ntp, int f32);
UDiv make_udiv(double d, int f32);
hipError_t launch_toa_src(const double *solar, int ncol, int ng, double *toa_src, int f32, hipStream_t s);
// out(i) = sum_b planes(i, b): broadband from per-band fluxes
hipError_t launch_sum_planes(const double *planes, int nplanes, size_t n, double *out, int f32, hipStream_t s);
hipError_t launch_rte_lw(const RteLwArgs &a, hipStream_t s);
// the single-precision register-resident solver with a.part_tau / part_ssa / part_mask added where it consumes tau
// (rte_lw_allsky_f32_kernel; f32 = 1, two separate level arrays, any layer count; ring and tail split as launch_rte_lw)
hipError_t launch_rte_lw_allsky_f32(const RteLwArgs &a, hipStream_t s);
// layer-split form (kernels_rte_lw_split.hip): fp64, 60 layers
bool rte_lw_split_applies(const RteLwArgs &a);
bool rte_lw_planck_fits(int ng, int ntp);   // the Planck-recomputing form: does the model's table fit in LDS?
hipError_t launch_rte_lw_split(const RteLwArgs &a, hipStream_t s);
// ... with the Planck sources recomputed in the solver from tlay(ncol,nlay), tlev(ncol,nlay+1), tsfc(ncol) and the
// model's table planck(ng,ntp) (a.lay_source / lev_source_* / sfc_source are not read)
// flux_up_clear / flux_dn_clear (both or neither; with a.part_tau): the dual-sky kernel, which walks the clear sky and the
// all sky in one pass and stores the clear-sky fluxes there
// flux_up_jac (without the clear-sky outputs): the Jacobian form, which also stores the surface-temperature Jacobian of flux_up
hipError_t launch_rte_lw_planck(const RteLwArgs &a, const double *planck, int ntp, double t0, double dt, const double *tlay,
                                const double *tlev, const double *tsfc, hipStream_t s, double *flux_up_clear = nullptr,
                                double *flux_dn_clear = nullptr, double *flux_up_jac = nullptr);
// ... one output plane per band (ecckd_lw_flux_bands): a.flux_up / a.flux_dn are (ncol,nlay+1,nband), band_first[b] the first
// 0-based g-point of band b and band_first[nband] = a.ng.  One launch; block row b solves the g-points of band b alone, in
// the groups a launch over that band's planes would form, and reads everything that lives on g-points at the model's index
hipError_t launch_rte_lw_planck_bands(const RteLwArgs &a, const double *planck, int ntp, double t0, double dt, const double *tlay,
                                      const double *tlev, const double *tsfc, const unsigned short *band_first, hipStream_t s);
// The rescaled no-scattering solver in the layer-split form (fp64, 60 layers): three exchanges per iteration.  a.ssa / a.g
// beside a.tau and the three source arrays ...
hipError_t launch_rte_lw_rescaled_split(const RteLwArgs &a, hipStream_t s);
// ... or the Planck-recomputing form: a.tau is the gas optical depth and the cell's (tau, ssa, g) is formed from the band
// triple a.part_tau / part_ssa / part_g (and a.part_mask) with the operations of the by-band increment_2stream_by_2stream
// flux_up_jac (ncol,nlay+1), or null: the Jacobian form, which stores the surface-temperature Jacobian of flux_up as well
// (rte_lw_rescaled_planck_fits(..., true): its third accumulator plane fits too)
bool rte_lw_rescaled_planck_fits(int ng, int ntp, bool jac = false);
hipError_t launch_rte_lw_rescaled_planck(const RteLwArgs &a, const double *planck, int ntp, double t0, double dt,
                                         const double *tlay, const double *tlev, const double *tsfc, hipStream_t s,
                                         double *flux_up_jac = nullptr);
hipError_t launch_rte_sw(const RteSwArgs &a, hipStream_t s);
// layer-systolic shortwave solver (kernels_rte_sw_sys.hip): any precision, nlay <= 60
bool rte_sw_sys_applies(const RteSwArgs &a);
size_t rte_sw_sys_plan(RteSwArgs &a, int cus);   // fills sys_tail_first / sys_gchunk; returns the bytes of `partials` (0: none)
hipError_t launch_rte_sw_sys(const RteSwArgs &a, int cus, hipStream_t s);
// partial sums of the tail tiles -> fluxes, in chunk order (kernels_rte_sw.hip)
hipError_t launch_rte_sw_tail_reduce(const RteSwArgs &a, int nchunks, int cw, long tail_first, long ntail, hipStream_t s);

// Column compaction (kernels_columns.hip).  Arrays are viewed as (ninner, ncol, nouter), ninner fastest; elem_bytes 4 or 8.
// day_index(ncol capacity) <- the ascending list of columns with mu0 > mu0_min (compared in double; NaN: night); work:
// daylit_work_bytes(ncol) of device memory, work[0] <- the count, behind it the block offsets.  Deterministic: no atomics.
int daylit_blocks(int ncol);
size_t daylit_work_bytes(int ncol);
hipError_t launch_daylit_columns(const void *mu0, int f32, int ncol, double mu0_min, int *day_index, int *work, hipStream_t s);
// dst(i,k,o) = src(i,index(k),o), k < nday; an index outside [0,ncol) is clamped
hipError_t launch_gather_columns(int ninner, int ncol, int nouter, int elem_bytes, int nday, const int *index, const void *src,
                                 void *dst, hipStream_t s);
// dst(k,l) = src[index(k)*col_stride + l*lay_stride] (strides in elements): a gas array of the ABI to a dense (nday,nlay)
hipError_t launch_gather_strided(int ncol, int nlay, int elem_bytes, int nday, const int *index, long long col_stride,
                                 long long lay_stride, const void *src, void *dst, hipStream_t s);
// dst(i,index(k),o) = src(i,k,o) and `fill` (as double, or rounded to float for 4-byte elements) in every column of dst
// that the list does not hold, in one pass over dst; the list must ascend; an index outside [0,ncol) is skipped
hipError_t launch_scatter_columns(int ninner, int ncol, int nouter, int elem_bytes, int nday, const int *index, const void *src,
                                  void *dst, double fill, hipStream_t s);

}  // namespace ecckd
