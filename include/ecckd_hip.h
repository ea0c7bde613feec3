/*
 * ecckd_hip.h -- C ABI of librte_ecckd_hip.so: the MI355X (gfx950) implementation of the
 * rte-ecckd hot path (ecCKD gas optics + RTE LW/SW flux solvers).
 *
 * This is the drop-in boundary.  Every entry point is `extern "C"`, takes plain pointers and
 * sizes, and is what a Fortran `iso_c_binding` interface block (or ctypes) binds; the
 * reference-side binding is shown in INTEGRATION.md and shipped in
 * rte-ecckd_amd/fortran/gas_optics_ecckd.F90.  Citations `file:line` are into the reference
 * repository (earth-system-radiation/rte-ecckd).
 *
 * Conventions
 *   - All arrays are contiguous, Fortran column-major, column index fastest, fp64:
 *     plev(ncol,nlay+1), tlay(ncol,nlay), tau(ncol,nlay,ngpt), flux(ncol,nlay+1) ...
 *   - `memspace` says where the DATA arrays live: ECCKD_HOST (the library stages them
 *     through device buffers it owns, and synchronises before returning) or ECCKD_DEVICE
 *     (pointers are device pointers on the model's GPU; the call is asynchronous on
 *     `stream`).  Small descriptor arrays (gas names, pointer tables, strides, Ds/weights,
 *     band2gpt) are always host memory.
 *     ECCKD_DEVICE calls never synchronise and never allocate once a (shape, stream) pair has been
 *     seen: they can be captured in a HIP graph after one warm-up call on the capturing stream (the
 *     solvers' scratch rings are per stream, see ecckd_set_stream_scratch).
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream).
 *   - Return value: 0 on success, non-zero on error; the message (same texts as the
 *     reference's character(len=128) results, src/gas_optics_ecckd.f90:331,393,442) is
 *     returned by ecckd_last_error().  There is no CPU fallback: without a usable GPU every
 *     compute entry point fails with an error.
 *   - Re-entrancy: a model is immutable after ecckd_model_finalize (the reference's
 *     `intent(in) :: this`, :385,:434); concurrent calls on different streams are safe in
 *     ECCKD_DEVICE mode.  ECCKD_HOST mode uses a per-model staging arena and is serialised
 *     by an internal mutex.
 */
#ifndef ECCKD_HIP_H
#define ECCKD_HIP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ECCKD_HOST 0
#define ECCKD_DEVICE 1
/* ECCKD_MIXED: the big arrays live on the device, the small ones on the host -- the calling convention of a
 * host model (Fortran, say) that keeps optical_props / sources in HBM between gas_optics and rte_* but holds
 * its atmosphere and wants its fluxes in host memory.  Device pointers: tau, ssa, g, lay_source,
 * lev_source_inc, lev_source_dec, sfc_source.  Host pointers, staged by the library: plev, tlay, tlev, tsfc,
 * gas arrays, toa_src / toa_flux, mu0, sfc_emis, albedos, inc_flux, fluxes.  The call synchronises before it
 * returns.  About 3.4 KB per column cross the bus instead of 34 KB (ECCKD_HOST).  Accepted by
 * ecckd_gas_optics_lw / _sw, ecckd_rte_lw (and _shared_levels, _inc_flux) and ecckd_rte_sw. */
#define ECCKD_MIXED 2

/* concentration_dependence_code values, src/gas_optics_ecckd.f90:54-57 */
#define ECCKD_NONE 0
#define ECCKD_LINEAR 1
#define ECCKD_LOOK_UP_TABLE 2
#define ECCKD_RELATIVE_LINEAR 3

#define ECCKD_MAX_GASES 16   /* src/gas_optics_ecckd.f90:24-25 */
#define ECCKD_NAME_LEN 32    /* character(len=32) gas names, :25 */

typedef struct ecckd_model ecckd_model_t; /* replaces type(ty_gas_optics_ecckd), :23-48 */

/* Message of the most recent failing call on this thread (never NULL). */
const char *ecckd_last_error(void);

/* ---------------------------------------------------------------------------------------
 * Model construction.  Two routes, both ending in an immutable device-resident model:
 *   (1) ecckd_model_load  = load_and_init, example/rfmip-rad-irf/mo_load_coefficients.F90:19-146
 *       (own netCDF-3 classic reader; no libnetcdf needed);
 *   (2) ecckd_model_begin / _set_* / _add_gas / _finalize = filling the public members of
 *       ty_gas_optics_ecckd directly (src/gas_optics_ecckd.f90:24-36), for hosts that
 *       already hold the tables.
 * --------------------------------------------------------------------------------------- */

/* load_and_init(ecckd, filename, available_gases): available_gases is accepted and ignored
 * by the reference (mo_load_coefficients.F90:19,23) and therefore has no parameter here. */
int ecckd_model_load(const char *filename, int device, ecckd_model_t **model);

/* log_pressure(np) [ln Pa] (:27), temperature(np,nt) [K] (:34); ng = size(gpoint_fraction,2)
 * (:26, only its extent is ever used, :110). */
int ecckd_model_begin(int ng, int np, int nt, const double *log_pressure,
                      const double *temperature, ecckd_model_t **model);
/* planck_function(ng,ntp) (:30), temperature_planck(ntp) (:35)  -> source_is_internal */
int ecckd_model_set_planck(ecckd_model_t *model, int ntp, const double *temperature_planck,
                           const double *planck_function);
/* solar_irradiance(ng) (:33), rayleigh_molar_scattering_coeff(ng) (:31) -> source_is_external */
int ecckd_model_set_solar(ecckd_model_t *model, const double *solar_irradiance,
                          const double *rayleigh_molar_scattering_coeff);
/* ty_optical_props%init(band_lims_wvn(2,nband), band2gpt(2,nband)) as called at
 * mo_load_coefficients.F90:74; band2gpt is 1-based, inclusive. */
int ecckd_model_set_bands(ecckd_model_t *model, int nband, const double *band_lims_wvn,
                          const int *band2gpt);
/* One AbsorptionTable (:13-19) + its name (:25).  coefficient is (ng,np,nt,nv); nv = 1 and
 * mole_fraction = NULL unless code == ECCKD_LOOK_UP_TABLE. */
int ecckd_model_add_gas(ecckd_model_t *model, const char *name, int concentration_dependence_code,
                        int composite_only, int nv, const double *mole_fraction,
                        double reference_mole_fraction, const double *coefficient);
/* Upload the tables to GPU `device` (HIP ordinal) and freeze the model.  device == -1 makes a
 * host-only model (also accepted by ecckd_model_load): the getters work, compute calls fail. */
int ecckd_model_finalize(ecckd_model_t *model, int device);
void ecckd_model_destroy(ecckd_model_t *model);

/* Type-bound getters of ty_gas_optics_ecckd (:38-45, :477-553) and of its parent
 * (get_ngpt/get_nband, used at ecckd_rfmip_sw.F90:78-79). */
int ecckd_model_get_ngpt(const ecckd_model_t *model);
int ecckd_model_get_nband(const ecckd_model_t *model);
int ecckd_model_get_ngas(const ecckd_model_t *model);                       /* :477-483 */
/* name is ECCKD_NAME_LEN bytes, NUL-terminated; index is 0-based. */
int ecckd_model_get_gas_name(const ecckd_model_t *model, int index, char *name);   /* :507-513 */
int ecckd_model_source_is_internal(const ecckd_model_t *model);             /* :487-493 */
int ecckd_model_source_is_external(const ecckd_model_t *model);             /* :497-503 */
double ecckd_model_get_press_min(const ecckd_model_t *model);               /* :517-523 */
double ecckd_model_get_press_max(const ecckd_model_t *model);               /* :527-533 */
double ecckd_model_get_temp_min(const ecckd_model_t *model);                /* :537-543 */
double ecckd_model_get_temp_max(const ecckd_model_t *model);                /* :547-553 */
double ecckd_model_get_total_solar_irradiance(const ecckd_model_t *model);  /* :36 */
/* band2gpt(2,nband), 1-based inclusive; band_lims_wvn(2,nband) */
int ecckd_model_get_band2gpt(const ecckd_model_t *model, int *band2gpt);
int ecckd_model_get_band_lims_wvn(const ecckd_model_t *model, double *band_lims_wvn);
int ecckd_model_get_device(const ecckd_model_t *model);

/* ---------------------------------------------------------------------------------------
 * gas_optics.  `gas_desc` (type(ty_gas_concs)) crosses the boundary as:
 *   ngas          gas_desc%get_num_gases()                         (:340)
 *   gas_names     ngas records of ECCKD_NAME_LEN chars, blank- or NUL-padded, in
 *                 gas_desc%get_gas_names() order                  (:342; order matters: :348)
 *   vmr[j]        data pointer of gas j in `memspace`, or NULL to use vmr_scalar[j]
 *   vmr_col_stride[j], vmr_lay_stride[j]
 *                 element strides so that get_vmr's broadcast (:351) is
 *                 vmr(i,l) = vmr[j][i*col_stride + l*lay_stride]:
 *                 (1,ncol) for a (ncol,nlay) array, (0,1) for a profile, (1,0) per column
 *   vmr_scalar[j] value used when vmr[j] == NULL (a ty_gas_concs scalar)
 * Gases unknown to the model are skipped, composite-only gases contribute the composite
 * table once (:358-373).
 * --------------------------------------------------------------------------------------- */

/* ---------------------------------------------------------------------------------------
 * Level buffer.  ecCKD's Planck level sources hold ONE value per level: the reference fills a
 * (ncol,nlay+1,ngpt) buffer and copies it into both arrays (src/gas_optics_ecckd.f90:419-424).
 * An entry point that takes lev_source_inc and lev_source_dec (ncol,nlay,ngpt) treats them as
 * the two views of ONE array lev(ncol,nlay+1,ngpt) exactly when
 *     lev_source_inc == lev_source_dec + ncol        (elements of the call's precision).
 * Then
 *     lev_source_dec(i,l,g) = lev[i + ncol*(l     + (nlay+1)*g)]
 *     lev_source_inc(i,l,g) = lev[i + ncol*(l + 1 + (nlay+1)*g)]       (0-based i, l, g)
 * i.e. both views have a g-plane stride of (nlay+1)*ncol instead of nlay*ncol, and
 * lev_source_inc(:,l,:) IS lev_source_dec(:,l+1,:) in memory.  Two contiguous arrays of more
 * than one plane at these addresses would overlap, so nothing else can be meant (with
 * nlay*ngpt == 1 both readings name the same memory).  No signature changes; nothing has to be
 * asserted by the caller.  A writer stores each level once, a reader reads it once: 24 instead of
 * 32 B/cell on either side, and ncol*(nlay-1)*ngpt elements less memory.
 *   Accept the form (fp64; ECCKD_DEVICE and ECCKD_MIXED):
 *     ecckd_gas_optics_lw, ecckd_planck_sources (writers);
 *     ecckd_rte_lw, ecckd_rte_lw_shared_levels, ecckd_rte_lw_inc_flux, ecckd_rte_lw_jac,
 *     ecckd_rte_lw_byband (readers: the shared-levels kernels, the same fluxes bit for bit).
 *   Refuse it (non-zero return, nothing written; ecckd_last_error() reads
 *   "<entry point>: lev_source_inc == lev_source_dec + ncol names one level buffer
 *   (ncol,nlay+1,ngpt); ... pass two separate arrays"):
 *     every entry point with ECCKD_HOST ("host arrays (ECCKD_HOST) are not taken in that form"),
 *     every *_f32 entry point ("single precision does not take that form"),
 *     ecckd_rte_lw_2stream, ecckd_rte_lw_rescaled, ecckd_rte_lw_rescaled_jac and the *_gpt
 *     solvers ("this entry point does not take that form").
 * ecckd_has_level_buffer() returns 1: a caller that loads the library at run time can tell a
 * build that knows the form from an older one (which would read and write overlapping arrays).
 * --------------------------------------------------------------------------------------- */
int ecckd_has_level_buffer(void);

/* gas_optics_int (:381-426): tau, lay_source, lev_source_inc, lev_source_dec are
 * (ncol,nlay,ngpt), sfc_source is (ncol,ngpt); the two level arrays may be the views of one
 * level buffer (above).  `play` and `col_dry` are unused by the
 * reference (:386,:394) and have no parameter.  tlev == NULL reproduces the reference:
 * tau, lay_source and sfc_source are written, then the call fails with
 * "tlev is required for ecckd" (:414-417).  Unlike the reference (:266-269 via :407) the
 * caller's lay_source is never reallocated. */
int ecckd_gas_optics_lw(const ecckd_model_t *model, int ncol, int nlay, const double *plev,
                        const double *tlay, const double *tsfc, const double *tlev, int ngas,
                        const char *gas_names, const double *const *vmr,
                        const long long *vmr_col_stride, const long long *vmr_lay_stride,
                        const double *vmr_scalar, double *tau, double *lay_source,
                        double *lev_source_inc, double *lev_source_dec, double *sfc_source,
                        int memspace, void *stream);

/* Single-precision flavour (a host built with RTE-RRTMGP's RTE_USE_SP, i.e. wp = real32): every
 * data array is float, arithmetic is float.  Implemented for the fused fast longwave path (one
 * pass, Planck table next to >= 3 slab rows: true for all ecCKD files in single precision); other
 * cases fail with a message.  vmr_scalar stays double (values, not arrays). */
int ecckd_gas_optics_lw_f32(const ecckd_model_t *model, int ncol, int nlay, const float *plev,
                            const float *tlay, const float *tsfc, const float *tlev, int ngas,
                            const char *gas_names, const float *const *vmr,
                            const long long *vmr_col_stride, const long long *vmr_lay_stride,
                            const double *vmr_scalar, float *tau, float *lay_source,
                            float *lev_source_inc, float *lev_source_dec, float *sfc_source,
                            int memspace, void *stream);

/* gas_optics_ext (:431-473): tau, ssa, g are (ncol,nlay,ngpt); toa_src is (ncol,ngpt).
 * ssa == NULL or g == NULL stands for an optical_props that is not ty_optical_props_2str:
 * tau (gas + Rayleigh) is written and the call fails with
 * "shortwave must use ty_optical_props_2str" (:461-463). */
int ecckd_gas_optics_sw(const ecckd_model_t *model, int ncol, int nlay, const double *plev,
                        const double *tlay, int ngas, const char *gas_names,
                        const double *const *vmr, const long long *vmr_col_stride,
                        const long long *vmr_lay_stride, const double *vmr_scalar, double *tau,
                        double *ssa, double *g, double *toa_src, int memspace, void *stream);

/* ---------------------------------------------------------------------------------------
 * RTE solvers (RTE-RRTMGP rte_lw / rte_sw as called at ecckd_rfmip_lw.F90:130-135 and
 * ecckd_rfmip_sw.F90:148-154) with the broadband g-point reduction
 * (ty_fluxes_broadband%reduce) fused in.  flux_up, flux_dn are (ncol,nlay+1).
 * --------------------------------------------------------------------------------------- */

/* No-scattering LW with Gauss-Jacobi quadrature, n_gauss_angles in 1..4.  sfc_emis is
 * (nband,ncol) as in rte_lw; band2gpt(2,nband) (1-based, inclusive) expands it to g-points
 * (ecckd_rfmip_lw.F90:112-116).  ngpt <= 256. */
int ecckd_rte_lw(int device, int ncol, int nlay, int ngpt, int top_at_1, int n_gauss_angles,
                 const double *tau, const double *lay_source, const double *lev_source_inc,
                 const double *lev_source_dec, const double *sfc_source, int nband,
                 const int *band2gpt, const double *sfc_emis, double *flux_up, double *flux_dn,
                 int memspace, void *stream);

/* ecckd_rte_lw for level sources that hold ONE value per level:
 *     lev_source_inc(:,l,:) == lev_source_dec(:,l+1,:)   for l = 1 .. nlay-1.
 * That is what ecckd_gas_optics_lw writes (src/gas_optics_ecckd.f90:419-424: both arrays are slices
 * of one (ncol,nlay+1,ngpt) buffer), but it is NOT part of RTE-RRTMGP's rte_lw contract (RRTMGP's
 * own gas optics fills the two arrays with different values), so the caller has to assert it by
 * calling this entry point.  The solver then reads each level once (24 instead of 32 B/cell): the
 * array that holds the far edge of the layers in walking order (lev_source_inc when top_at_1) in
 * full, the other one for the first layer only.  Same arithmetic and the same fluxes, bit for bit,
 * as ecckd_rte_lw when the assertion holds.  Same arguments. */
int ecckd_rte_lw_shared_levels(int device, int ncol, int nlay, int ngpt, int top_at_1,
                               int n_gauss_angles, const double *tau, const double *lay_source,
                               const double *lev_source_inc, const double *lev_source_dec,
                               const double *sfc_source, int nband, const int *band2gpt,
                               const double *sfc_emis, double *flux_up, double *flux_dn,
                               int memspace, void *stream);

/* ecckd_rte_lw with the optional incident diffuse flux at the top of the domain: rte_lw's `inc_flux(ncol,ngpt)`
 * argument [RTE-RRTMGP; no reference call site passes it: ecckd_rfmip_lw.F90:130-135].  I_dn(top) =
 * inc_flux/(2 pi w_k) for quadrature angle k (see the solver option
 * lw_inc_flux_isotropic).  inc_flux == NULL is ecckd_rte_lw.  fp64, generic level sources. */
int ecckd_rte_lw_inc_flux(int device, int ncol, int nlay, int ngpt, int top_at_1, int n_gauss_angles,
                          const double *tau, const double *lay_source, const double *lev_source_inc,
                          const double *lev_source_dec, const double *sfc_source, int nband,
                          const int *band2gpt, const double *sfc_emis, const double *inc_flux,
                          double *flux_up, double *flux_dn, int memspace, void *stream);

/* Single-precision flavour of ecckd_rte_lw. */
int ecckd_rte_lw_f32(int device, int ncol, int nlay, int ngpt, int top_at_1, int n_gauss_angles,
                     const float *tau, const float *lay_source, const float *lev_source_inc,
                     const float *lev_source_dec, const float *sfc_source, int nband,
                     const int *band2gpt, const float *sfc_emis, float *flux_up, float *flux_dn,
                     int memspace, void *stream);

/* ---------------------------------------------------------------------------------------
 * RTE-RRTMGP's KERNEL-level solver interfaces [RTE-ext: mo_rte_solver_kernels.F90 / mo_fluxes_broadband_kernels.F90 of the
 * v1.5 era; that library is not part of the reference tree -- reference Makefile:19,33 links it]: spectral fluxes
 * (ncol,nlay+1,ngpt), per-g-point boundary conditions (ncol,ngpt), quadrature passed in, the g-point sum left to
 * sum_broadband.  include/rte_kernels_hip.h + librte_kernels_hip.so export them under RTE-RRTMGP's own bind(C)
 * names and by-reference argument lists, so that they can stand in for RTE's kernel objects at link time.  These
 * are compatibility kernels (one thread per column and g-point); rte_lw / rte_sw callers get the fused solvers.
 *   inc_flux (LW) / inc_flux_dif (SW): diffuse flux incident at the top, (ncol,ngpt) or NULL
 *   flux_dir_top (SW): direct flux at the top of the domain, inc_flux*mu0, (ncol,ngpt)
 * --------------------------------------------------------------------------------------- */
int ecckd_lw_solver_noscat_gpt(int device, int ncol, int nlay, int ngpt, int top_at_1, int nmus, const double *Ds,
                               const double *weights, const double *tau, const double *lay_source,
                               const double *lev_source_inc, const double *lev_source_dec,
                               const double *sfc_emis, const double *sfc_src, const double *inc_flux,
                               double *gpt_flux_up, double *gpt_flux_dn, int memspace, void *stream);
int ecckd_sw_solver_2stream_gpt(int device, int ncol, int nlay, int ngpt, int top_at_1, const double *tau,
                                const double *ssa, const double *g, const double *mu0,
                                const double *flux_dir_top, const double *inc_flux_dif,
                                const double *sfc_alb_dir, const double *sfc_alb_dif, double *gpt_flux_up,
                                double *gpt_flux_dn, double *gpt_flux_dir, int memspace, void *stream);
int ecckd_sum_broadband(int device, int ncol, int nlev, int ngpt, const double *spectral_flux,
                        double *broadband_flux, int memspace, void *stream);

/* ---------------------------------------------------------------------------------------
 * Fused longwave path (no counterpart call in the reference, whose block loop calls
 * gas_optics and rte_lw back to back with nothing reading tau or the sources in between:
 * ecckd_rfmip_lw.F90:120-135).  The three source arrays are pure functions of tlay / tlev / tsfc and the model's
 * Planck table (src/gas_optics_ecckd.f90:407-424), so a host that only needs fluxes does not have to move them:
 * gas optics writes tau only (8 B/cell) and the solver recomputes the sources while it reads tau (8 B/cell) --
 * 16 instead of 64 B per (column, layer, g-point) between the two kernels.  Same arithmetic per cell (sources bit
 * identical to ecckd_gas_optics_lw); fast arithmetic mode, fp64.  60 layers take the fused kernels; any other layer
 * count is served by the general route (Planck kernel into library scratch, then the register-resident solver): the same
 * results at the API path's rate.  This path is bound by fp64 issue, not by HBM, and bench.py reports it apart from the
 * API-boundary roofline ("fused_lw").
 *   ecckd_gas_optics_lw_tau  gas_optical_depth (:323-376) alone: tau(ncol,nlay,ngpt)              ECCKD_DEVICE
 *   ecckd_rte_lw_fused       rte_lw on tau + temperatures; sfc_emis(nband,ncol), inc_flux(ncol,ngpt) or NULL  ECCKD_DEVICE
 *   ecckd_lw_fluxes          both, tau in library-owned stream-ordered scratch      ECCKD_DEVICE or ECCKD_HOST
 * --------------------------------------------------------------------------------------- */
int ecckd_gas_optics_lw_tau(const ecckd_model_t *model, int ncol, int nlay, const double *plev, const double *tlay,
                            int ngas, const char *gas_names, const double *const *vmr,
                            const long long *vmr_col_stride, const long long *vmr_lay_stride,
                            const double *vmr_scalar, double *tau, int memspace, void *stream);
int ecckd_rte_lw_fused(const ecckd_model_t *model, int ncol, int nlay, int top_at_1, int n_gauss_angles,
                       const double *tau, const double *tlay, const double *tlev, const double *tsfc,
                       const double *sfc_emis, const double *inc_flux, double *flux_up, double *flux_dn,
                       int memspace, void *stream);
int ecckd_lw_fluxes(const ecckd_model_t *model, int ncol, int nlay, const double *plev, const double *tlay,
                    const double *tsfc, const double *tlev, int ngas, const char *gas_names,
                    const double *const *vmr, const long long *vmr_col_stride, const long long *vmr_lay_stride,
                    const double *vmr_scalar, int top_at_1, int n_gauss_angles, const double *sfc_emis,
                    const double *inc_flux, double *flux_up, double *flux_dn, int memspace, void *stream);

/* Two-stream + adding SW.  mu0(ncol), toa_flux(ncol,ngpt), sfc_alb_dir/dif(nband,ncol).
 * flux_dn includes the direct beam; flux_dir (ncol,nlay+1) may be NULL. */
int ecckd_rte_sw(int device, int ncol, int nlay, int ngpt, int top_at_1, const double *tau,
                 const double *ssa, const double *g, const double *mu0, const double *toa_flux,
                 int nband, const int *band2gpt, const double *sfc_alb_dir,
                 const double *sfc_alb_dif, double *flux_up, double *flux_dn, double *flux_dir,
                 int memspace, void *stream);

/* Single-precision flavours of the shortwave pair and of ecckd_rte_lw_inc_flux (a host built with RTE-RRTMGP's
 * RTE_USE_SP: wp = real32, src/gas_optics_ecckd.f90:6).  Every data array is float, arithmetic is float, the g-point
 * sums are accumulated in double and rounded once.  ecckd_gas_optics_sw_f32: one-pass gas lists (all ecCKD files);
 * ecckd_rte_sw_f32 (and ecckd_rte_sw_byband_f32): any layer count, with the solver "sw_solver" picks as for fp64. */
int ecckd_gas_optics_sw_f32(const ecckd_model_t *model, int ncol, int nlay, const float *plev, const float *tlay,
                            int ngas, const char *gas_names, const float *const *vmr,
                            const long long *vmr_col_stride, const long long *vmr_lay_stride,
                            const double *vmr_scalar, float *tau, float *ssa, float *g, float *toa_src,
                            int memspace, void *stream);
int ecckd_rte_sw_f32(int device, int ncol, int nlay, int ngpt, int top_at_1, const float *tau, const float *ssa,
                     const float *g, const float *mu0, const float *toa_flux, int nband, const int *band2gpt,
                     const float *sfc_alb_dir, const float *sfc_alb_dif, float *flux_up, float *flux_dn,
                     float *flux_dir, int memspace, void *stream);
int ecckd_rte_lw_inc_flux_f32(int device, int ncol, int nlay, int ngpt, int top_at_1, int n_gauss_angles,
                              const float *tau, const float *lay_source, const float *lev_source_inc,
                              const float *lev_source_dec, const float *sfc_source, int nband,
                              const int *band2gpt, const float *sfc_emis, const float *inc_flux, float *flux_up,
                              float *flux_dn, int memspace, void *stream);

/* ---------------------------------------------------------------------------------------
 * Fused shortwave path (SURVEY.md section 8(f) rank 4 for the shortwave; no counterpart call in the reference, whose
 * block loop calls gas_optics and rte_sw back to back: ecckd_rfmip_sw.F90:118-154).  gas_optics_ext derives ssa, g and
 * toa_src from plev and two small tables (src/gas_optics_ecckd.f90:455-472: ssa = tau_rayleigh/tau with
 * tau_rayleigh = (plev(l+1)-plev(l))*global_weight*rayleigh_molar_scattering_coeff(g) (:313-317), g = 0,
 * toa_src = solar_irradiance(g)), so a host that only needs fluxes moves the TOTAL optical depth alone: gas optics
 * writes tau (8 B/cell) and the solver evaluates those same expressions while it reads it (8 B/cell) -- 16 instead of
 * 48 B per (column, layer, g-point).  Same arithmetic per cell: fluxes bit-identical to ecckd_gas_optics_sw +
 * ecckd_rte_sw.  tau lives in library-owned stream-ordered scratch.  Fast arithmetic mode; any layer count, with the
 * solver ecckd_rte_sw takes for the shape ("sw_solver"), so the bits match at every depth; ECCKD_DEVICE or ECCKD_HOST.
 * With ECCKD_DEVICE, tau sits at the start of the stream's scratch block and the solver's room follows it.  A host
 * that owns the block (ecckd_set_stream_scratch) sizes it as align256(ncol*nlay*ngpt*sizeof(real)) (align256: round
 * up to a multiple of 256 bytes) plus
 *   layer-systolic solver ("sw_solver" = 0, nlay <= 60): ecckd_rte_sw_tail_scratch_bytes(device, ncol, nlay, ngpt);
 *   two-pass solver (every other call): max(ecckd_rte_sw_scratch_bytes(ncol, nlay, ngpt),
 *                                           ecckd_rte_sw_tail_scratch_bytes(device, ncol, nlay, ngpt)).
 *   toa_scale(ncol) or NULL: toa(i,g) = solar_irradiance(g)*toa_scale(i) -- the drivers' rescaling to the file's total
 *   solar irradiance (ecckd_rfmip_sw.F90:126-133); mu0(ncol), sfc_alb_dir/dif(nband,ncol) as ecckd_rte_sw;
 *   flux_dir may be NULL.
 * bench.py reports it apart from the API-boundary roofline ("fused_sw").
 * --------------------------------------------------------------------------------------- */
int ecckd_sw_fluxes(const ecckd_model_t *model, int ncol, int nlay, const double *plev, const double *tlay, int ngas,
                    const char *gas_names, const double *const *vmr, const long long *vmr_col_stride,
                    const long long *vmr_lay_stride, const double *vmr_scalar, int top_at_1, const double *mu0,
                    const double *toa_scale, const double *sfc_alb_dir, const double *sfc_alb_dif, double *flux_up,
                    double *flux_dn, double *flux_dir, int memspace, void *stream);
int ecckd_sw_fluxes_f32(const ecckd_model_t *model, int ncol, int nlay, const float *plev, const float *tlay, int ngas,
                        const char *gas_names, const float *const *vmr, const long long *vmr_col_stride,
                        const long long *vmr_lay_stride, const double *vmr_scalar, int top_at_1, const float *mu0,
                        const float *toa_scale, const float *sfc_alb_dir, const float *sfc_alb_dif, float *flux_up,
                        float *flux_dn, float *flux_dir, int memspace, void *stream);

/* ---------------------------------------------------------------------------------------
 * All-sky: particulate (cloud, aerosol) optical properties between gas_optics and the solvers.  A host model carries
 * them on the model's BANDS, (ncol,nlay,nband); the reference's drivers have no such path (clear-sky RFMIP only), so
 * there is no counterpart call in the reference tree: the calls restate RTE-RRTMGP's ty_optical_props%delta_scale and
 * %increment [RTE-ext: mo_optical_props_kernels.F90 of the v1.5 era; the library is not in the reference tree], which
 * every all-sky RTE-RRTMGP driver calls between gas_optics and rte_sw / rte_lw.  Arrays are (ncol,nlay,n), column fastest,
 * n = g-points or bands; eps = 3*tiny(real); memspace ECCKD_DEVICE (asynchronous on `stream`) or ECCKD_HOST; fp64 and _f32.
 *
 * ecckd_delta_scale  [delta_scale_2str_k; with `forward`: delta_scale_2str_f_k], in place:
 *     f = forward ? forward : g*g;  wf = ssa*f;  tau = tau*(1-wf);  ssa = (ssa-wf)/max(eps,1-wf);  g = (g-f)/max(eps,1-f)
 *   forward(ncol,nlay,n) or NULL.  Values of `forward` outside [0,1] are an error with ECCKD_HOST arrays (checked before
 *   anything is launched) and give undefined results with ECCKD_DEVICE arrays (not checked: the call stays asynchronous).
 *
 * ecckd_increment  op1 += op2 in place; which pointers are NULL picks the combination (ssa and g go together):
 *     ssa1 NULL, ssa2 NULL  [increment_1scalar_by_1scalar]  tau1 = tau1 + tau2
 *     ssa1 NULL, ssa2 set   [increment_1scalar_by_2stream]  tau1 = tau1 + tau2*(1-ssa2)     (absorption only: what a
 *                                                            no-scattering longwave solver wants)
 *     ssa1 set,  ssa2 NULL  [increment_2stream_by_1scalar]  tau12 = tau1+tau2;  ssa1 = tau1*ssa1/max(eps,tau12);  tau1 = tau12
 *     ssa1 set,  ssa2 set   [increment_2stream_by_2stream]  tau12 = tau1+tau2;  tauscat12 = tau1*ssa1 + tau2*ssa2;
 *                                                            g1 = (tau1*ssa1*g1 + tau2*ssa2*g2)/max(eps,tauscat12);
 *                                                            ssa1 = tauscat12/max(eps,tau12);  tau1 = tau12
 *   nband = 0: op2 is on the same ngpt points (band2gpt ignored).  nband > 0 [the inc_*_bybnd forms]: op2 is
 *   (ncol,nlay,nband) and band2gpt(2,nband) -- host memory, 1-based, inclusive, as ecckd_model_get_band2gpt returns it --
 *   spreads each band over its g-points; the bands must tile 1..ngpt in ascending order (at most 256 bands, 65535
 *   g-points).  ssa without g, or a band table that does not tile, is refused with a message before any launch.
 *   Longwave all-sky: ecckd_gas_optics_lw, ecckd_increment(tau, NULL, NULL, nband, band2gpt, tau_c, ssa_c, g_c),
 *   ecckd_rte_lw.  Clouds plus aerosols: add them up on the band grid first (nband planes), then increment once.
 * --------------------------------------------------------------------------------------- */
int ecckd_delta_scale(int device, int ncol, int nlay, int n, double *tau, double *ssa, double *g, const double *forward,
                      int memspace, void *stream);
int ecckd_delta_scale_f32(int device, int ncol, int nlay, int n, float *tau, float *ssa, float *g, const float *forward,
                          int memspace, void *stream);
int ecckd_increment(int device, int ncol, int nlay, int ngpt, double *tau1, double *ssa1, double *g1, int nband,
                    const int *band2gpt, const double *tau2, const double *ssa2, const double *g2, int memspace, void *stream);
int ecckd_increment_f32(int device, int ncol, int nlay, int ngpt, float *tau1, float *ssa1, float *g1, int nband,
                        const int *band2gpt, const float *tau2, const float *ssa2, const float *g2, int memspace, void *stream);

/* Fused all-sky shortwave: ecckd_sw_fluxes with the combined particulate properties tau_p, ssa_p, g_p (ncol,nlay,nband_p)
 * on the model's bands (nband_p must equal ecckd_model_get_nband).  Gas optics writes the GAS total optical depth into
 * stream scratch as for ecckd_sw_fluxes; where the solver forms ssa = moles*ray/tau and g = 0 there, it forms here, with the
 * layer's band triple (tp, sp, gp) [increment_2stream_by_2stream with op1 = the gas optics]:
 *     tau_r = moles*ray;  ts = tau_r + tp*sp;  tau12 = tau + tp;
 *     g = (tp*sp*gp)/max(eps,ts);  ssa = ts/max(eps,tau12);  tau = tau12
 * so no per-g-point ssa or g array exists in memory.  delta_scale = 1: the library first delta-scales a COPY of the triple
 * with f = g*g [delta_scale_2str_k]; the caller's arrays are never written.  fp64, fast arithmetic mode only (reference-order
 * mode is refused with a message), any layer count, ECCKD_DEVICE or ECCKD_HOST, toa_scale as ecckd_sw_fluxes.  The solver
 * is the one ecckd_sw_fluxes takes for the shape ("sw_solver": layer-systolic up to 60 layers, else two-pass).  Fluxes agree
 * with ecckd_gas_optics_sw + ecckd_increment + ecckd_rte_sw to rounding, not bit for bit (ssa is formed in a different order).
 * Scratch (ECCKD_DEVICE; a host that owns the stream's block, ecckd_set_stream_scratch, sizes it so): what ecckd_sw_fluxes
 * needs for the shape (the fused shortwave path, above: align256(ncol*nlay*ngpt*8) plus the solver's term)
 *   + (delta_scale ? 3*align256(ncol*nlay*nband*8) : 0)
 * in that order: optical depth, solver room, the three scaled band planes.  The planes belong to the stream's block, so the capture rules of the solver scratch hold:
 * capture after one warm-up call on the stream, or with a caller-owned block. */
int ecckd_sw_fluxes_allsky(const ecckd_model_t *model, int ncol, int nlay, const double *plev, const double *tlay, int ngas,
                           const char *gas_names, const double *const *vmr, const long long *vmr_col_stride,
                           const long long *vmr_lay_stride, const double *vmr_scalar, int top_at_1, const double *mu0,
                           const double *toa_scale, const double *sfc_alb_dir, const double *sfc_alb_dif, int nband_p,
                           const double *tau_p, const double *ssa_p, const double *g_p, int delta_scale, double *flux_up,
                           double *flux_dn, double *flux_dir, int memspace, void *stream);

/* Fused all-sky longwave: ecckd_lw_fluxes with the combined particulate properties tau_p, ssa_p (ncol,nlay,nband_p) on the
 * model's bands (nband_p must equal ecckd_model_get_nband), in `memspace`, in the layer order of tlay.  The solver sees
 *     ssa_p set:   tau = tau_gas + tau_p*(1 - ssa_p)   [increment_1scalar_by_2stream, by band: absorption only]
 *     ssa_p NULL:  tau = tau_gas + tau_p               [increment_1scalar_by_1scalar, by band: one-stream particles]
 * spelt operation by operation as ecckd_increment spells them, so the fluxes equal those of ecckd_gas_optics_lw_tau +
 * ecckd_increment + ecckd_rte_lw_fused BIT FOR BIT.  There is no asymmetry argument and no delta scaling: a no-scattering
 * solver uses neither.  At 60 layers (both shipped longwave files) the Planck-recomputing layer-split solver adds the
 * layer's band value where it reads tau -- a few loads per (column, layer, band), no pass over the g-point arrays; any other
 * layer count, or a Planck table that does not fit LDS, takes the general route of ecckd_lw_fluxes with the by-band
 * increment kernel run on the scratch tau between gas optics and the solver (the rate of the API pair).
 * fp64, fast arithmetic mode only; n_gauss_angles 1..4; inc_flux or NULL; top_at_1 concerns the solver alone, as in
 * ecckd_lw_fluxes.  ECCKD_DEVICE is asynchronous on `stream`; ECCKD_HOST stages through the model's arena.  tau_p / ssa_p
 * are never written.  Refused with a message before any device is asked for, in this order: nband_p differs from the
 * model's band count; tau_p NULL; reference-order arithmetic mode; a model without a Planck table; tlev NULL; a host-only
 * model.
 * Scratch (ECCKD_DEVICE): exactly what ecckd_lw_fluxes takes from the stream's block for the shape -- the band planes are
 * read in place, nothing is staged.  At 60 layers with the fused kernels that is (ncol*nlay*ngpt + 32)*8 bytes (the gas
 * optical depth); a host that owns the block (ecckd_set_stream_scratch) sizes it so, and the capture rules of
 * ecckd_lw_fluxes hold unchanged: capture after one warm-up call on the stream, or with a caller-owned block. */
int ecckd_lw_fluxes_allsky(const ecckd_model_t *model, int ncol, int nlay, const double *plev, const double *tlay,
                           const double *tsfc, const double *tlev, int ngas, const char *gas_names,
                           const double *const *vmr, const long long *vmr_col_stride, const long long *vmr_lay_stride,
                           const double *vmr_scalar, int top_at_1, int n_gauss_angles, const double *sfc_emis,
                           const double *inc_flux, int nband_p, const double *tau_p, const double *ssa_p,
                           double *flux_up, double *flux_dn, int memspace, void *stream);

/* ---------------------------------------------------------------------------------------
 * McICA cloud sampling (Pincus et al. 2003): cloud fraction through the all-sky calls.  The calls above treat a cloudy
 * layer as overcast.  A host with a cloud fraction draws a per-g-point cloud mask from it under an overlap assumption and
 * the particulate optical depth of the (layer, g-point) cells that came out clear is taken as zero.
 *
 * A cloud mask is ONE `unsigned long long` per (column, layer): array (ncol,nlay), column fastest, in the layer order of
 * tlay; bit g (0-based g-point) set = that g-point sees the layer's particles.  It serves at most 64 g-points (every ecCKD
 * file: 27, 32, 36); every call below refuses ngpt > 64 with a message before anything is launched.
 *
 * ecckd_cloud_mask_sample: the definition is this project's own.  It restates the rank-carrying generator of Raisanen et
 * al. (2004), on which RTE-RRTMGP's mo_cloud_sampling (sampled_mask_max_ran, sampled_mask_exp_ran) is built, from the
 * published description; RTE-RRTMGP is not part of the reference tree, so PARITY WITH IT IS UNPINNED.  The random numbers
 * are made in the kernel by a counter-based generator, so the mask of a column depends on (seed, global column index,
 * layer, g-point) only -- not on the launch shape, the block a host cuts its columns into, or the GPU a column range is
 * sharded to; col0 = global index of the call's first column.  (An array of caller-made randoms is deliberately not taken.)
 *   - Philox4x32-10 (Salmon et al. 2011; multipliers 0xD2511F53, 0xCD9E8D57, Weyl constants 0x9E3779B9, 0xBB67AE85).
 *     For the global column c = col0 + i, layer l (0-based, array order) and g-point g (0-based):
 *         counter = (c & 0xffffffff, c >> 32, l, (g >> 2) | (s << 31)),  key = (seed & 0xffffffff, seed >> 32),
 *         draw = (output word (g & 3) >> 8) * 2^-24        (exact in fp64, in [0,1))
 *     s = 0 gives u(c,l,g), s = 1 gives v(c,l,g).
 *   - correlation of the rank between layers l-1 and l:  a(l) = 0 if l = 0 or either layer's cloud_frac is not > 0 (a clear
 *     layer -- zero, negative or NaN -- decorrelates: the "-random" part); else 1 (ECCKD_OVERLAP_MAX_RAN) or overlap_param(i, l-1) (ECCKD_OVERLAP_EXP_RAN)
 *   - rank:  r(l,g) = v(c,l,g) < a(l) ? r(l-1,g) : u(c,l,g)
 *   - bit g of mask(i,l) = cloud_frac(i,l) > 0 && r(l,g) >= 1 - cloud_frac(i,l)   (subtraction and comparison in fp64)
 *     Bits ngpt..63 are 0.  A NaN cloud fraction gives a clear layer; cloud_frac = 1 is always cloudy.
 *   Everything is integer arithmetic plus exact fp64 operations: the words are reproducible bit for bit
 *   (tests/mcica_helpers.py).  overlap_param (ncol,nlay-1) is read with ECCKD_OVERLAP_EXP_RAN only (else pass NULL).
 *   cloud_frac or overlap_param outside [0,1]: an error with ECCKD_HOST arrays (checked before anything is launched),
 *   undefined with ECCKD_DEVICE arrays (not checked: the call stays asynchronous) -- the rule of ecckd_delta_scale's `forward`.
 *   Refused with a message, in this order: ngpt > 64; ngpt < 1; unknown overlap; ECCKD_OVERLAP_EXP_RAN without
 *   overlap_param; bad ncol / nlay; cloud_frac or mask NULL; bad memspace; host values outside [0,1]; no device.
 *   fp64 only.  ECCKD_DEVICE is asynchronous on `stream` and uses no scratch; ECCKD_HOST stages and synchronises.
 *
 * ecckd_increment_masked (+ _f32): ecckd_increment with `mask` (ncol,nlay) in `memspace`.  Where bit g is clear the cell is
 * incremented AS IF tau2 WERE +0 THERE (what RTE-RRTMGP's draw_samples followed by increment computes), spelt with the
 * operations of ecckd_increment; ssa2 / g2 are still read, so a non-finite value in a masked-out cell propagates as it
 * would through 0*x.  All four combinations, on g-points and by band.  mask NULL: ecckd_increment.  ngpt > 64 with a mask
 * is refused first, then ecckd_increment's own list.
 *
 * ecckd_sw_fluxes_allsky_mcica / ecckd_lw_fluxes_allsky_mcica: the fused all-sky calls with `cloud_mask` (ncol,nlay) in
 * `memspace`.  The particulate optical depth a cell uses is  bit ? tau_p : 0  in front of the expressions of the unmasked
 * call -- one select per cell, nothing else changes; with delta_scale = 1 the band triple is scaled first (independent of
 * the mask), then masked.  cloud_mask NULL forwards to the unmasked call.  Longwave: fluxes equal ecckd_gas_optics_lw_tau +
 * ecckd_increment_masked + ecckd_rte_lw_fused BIT FOR BIT (60 layers: masked layer-split kernel; any other layer count: the
 * masked by-band increment on the scratch optical depth).  Shortwave: the masked forms of the layer-systolic (up to 60
 * layers) and two-pass solvers; agreement with the composed calls to rounding, as for the unmasked call.  Refused with a
 * message: a model of more than 64 g-points first, then the unmasked call's own list in its order.  Scratch sizes and
 * capture rules are those of the unmasked calls (the mask is read in place).  Parity with RTE-RRTMGP unpinned, as above.
 * --------------------------------------------------------------------------------------- */
#define ECCKD_OVERLAP_MAX_RAN 0
#define ECCKD_OVERLAP_EXP_RAN 1
int ecckd_cloud_mask_sample(int device, int ncol, int nlay, int ngpt, int overlap, const double *cloud_frac,
                            const double *overlap_param, unsigned long long seed, long long col0, unsigned long long *mask,
                            int memspace, void *stream);
int ecckd_increment_masked(int device, int ncol, int nlay, int ngpt, double *tau1, double *ssa1, double *g1, int nband,
                           const int *band2gpt, const double *tau2, const double *ssa2, const double *g2,
                           const unsigned long long *mask, int memspace, void *stream);
int ecckd_increment_masked_f32(int device, int ncol, int nlay, int ngpt, float *tau1, float *ssa1, float *g1, int nband,
                               const int *band2gpt, const float *tau2, const float *ssa2, const float *g2,
                               const unsigned long long *mask, int memspace, void *stream);
int ecckd_sw_fluxes_allsky_mcica(const ecckd_model_t *model, int ncol, int nlay, const double *plev, const double *tlay, int ngas,
                                 const char *gas_names, const double *const *vmr, const long long *vmr_col_stride,
                                 const long long *vmr_lay_stride, const double *vmr_scalar, int top_at_1, const double *mu0,
                                 const double *toa_scale, const double *sfc_alb_dir, const double *sfc_alb_dif, int nband_p,
                                 const double *tau_p, const double *ssa_p, const double *g_p, int delta_scale,
                                 const unsigned long long *cloud_mask, double *flux_up, double *flux_dn, double *flux_dir,
                                 int memspace, void *stream);
int ecckd_lw_fluxes_allsky_mcica(const ecckd_model_t *model, int ncol, int nlay, const double *plev, const double *tlay,
                                 const double *tsfc, const double *tlev, int ngas, const char *gas_names,
                                 const double *const *vmr, const long long *vmr_col_stride, const long long *vmr_lay_stride,
                                 const double *vmr_scalar, int top_at_1, int n_gauss_angles, const double *sfc_emis,
                                 const double *inc_flux, int nband_p, const double *tau_p, const double *ssa_p,
                                 const unsigned long long *cloud_mask, double *flux_up, double *flux_dn, int memspace,
                                 void *stream);

/* ---------------------------------------------------------------------------------------
 * In-cloud water variability: sampled optical-depth scaling.  A cloud mask carries one bit per g-point, so every cloudy
 * sub-column of the McICA calls above has the layer-mean optical depth (the plane-parallel-homogeneous bias remains).  A
 * host that knows the fractional standard deviation (FSD) of in-cloud water gets from ecckd_cloud_scaling_sample a
 * per-g-point factor od_scaling(column, layer, g-point) of the cloud optical depth -- 0 where the g-point is clear -- and
 * hands it to the consumers below in place of the mask; a host with a cloud generator of its own hands them ITS array.
 * EVERY DEFINITION HERE IS THIS PROJECT'S OWN, like the sampler's: PARITY WITH ecRad AND RTE-RRTMGP IS UNPINNED.  Each line
 * below is one correctly rounded IEEE fp64 operation (the build has contraction off), so tests/cloud_scaling_ref.py
 * reproduces the arrays bit for bit.
 *
 * A scaling array is `float` (ncol,nlay,ngpt), column fastest, in the layer order of tlay, whatever the precision of the
 * call that reads it: 4 bytes per cell against the optical depth's 8 (1e6 columns x 60 layers x 32 g-points: 7.7 GB).
 *
 * The scaling table (a host object, like the cloud-optics LUT): values(nfsd,nq), q fastest.  Row k belongs to the FSD
 * fsd0 + k*dfsd, column j is the scaling of the j-th of nq equal-probability bins of the in-cloud distribution (ascending).
 * ecckd_cloud_scaling_create refuses with a message: a null handle; nfsd < 2; nq < 1; dfsd not > 0 (or not finite, or fsd0
 * not finite); more than 2^24 entries; null values; a non-finite or negative value.  device = -1 makes a host-only object.
 * ecckd_cloud_scaling_lognormal (host code, no device) fills values(nfsd,nq) with the bin means of the unit-mean lognormal
 * distribution:  sigma^2 = log(1 + f^2);  entry j = nq * (Phi(z_{j+1} - sigma) - Phi(z_j - sigma)),  z_j = Phi^-1(j/nq),
 * z_0 = -inf, z_nq = +inf, Phi through erfc.  A row with f = 0 is all ones exactly.  The mean of a row is 1 to rounding; its
 * standard deviation is BELOW f (0.908 for f = 1 at nq = 16: bin means under-disperse) and approaches f as nq grows.
 * The gamma distribution is not built by the library: a host passes its own table through ecckd_cloud_scaling_create.
 *
 * ecckd_cloud_scaling_sample: the rank r(l,g) and "seen" (= the bit) are exactly those of ecckd_cloud_mask_sample -- the same
 * Philox counters, key and recurrence; `mask`, if not NULL, receives that call's words.  fsd (ncol,nlay) fp64, or NULL:
 * fsd_const serves every cell.  For a seen cell, with cf = cloud_frac(i,l), v the table, in fp64:
 *     p = (r - (1 - cf)) / cf                     the position of the sub-column inside the cloud
 *     j = min((int)(p * nq), nq - 1)
 *     x = (fsd - fsd0) / dfsd
 *     if !(x > 0):           k = 0,        w = 0      (a NaN lands here)
 *     else if x >= nfsd - 1: k = nfsd - 2, w = 1
 *     else:                  k = (int)x,   w = x - k
 *     s = v[k][j] + w * (v[k+1][j] - v[k][j]);     scaling = (float)s
 * An unseen cell gets +0.0f.  fsd is not read where the layer is clear.  Refused with a message, in this order: ngpt > 64
 * (the ranks of a column are held at once); ngpt < 1; unknown overlap; ECCKD_OVERLAP_EXP_RAN without overlap_param; bad
 * ncol / nlay; cloud_frac or scaling NULL; a NULL table; bad memspace; host values outside [0,1]; a host-only table or one
 * of another device; no device.  ECCKD_DEVICE is asynchronous on `stream` and uses no scratch; ECCKD_HOST stages.
 *
 * ecckd_increment_scaled (+ _f32): ecckd_increment's argument list plus `scaling`.  Per g-point  t2 = tau2 * (real)scaling,
 * then ecckd_increment's expressions on t2 -- t2*(1 - ssa2), t2*ssa2 and that product times g2 --, evaluated per g-point,
 * not hoisted per band.  All four combinations, on g-points and by band; any number of g-points.  With a scaling of exactly
 * 0 or 1 and finite tau2 >= 0 the result is that of ecckd_increment_masked with the corresponding bits, bit for bit; with
 * all ones that of ecckd_increment.  scaling NULL: ecckd_increment.  Refusals: ecckd_increment's list.
 *
 * ecckd_lw_flux_scaled / ecckd_sw_flux_scaled: the argument lists of the _mcica calls with `const float *cloud_scaling` in
 * place of the mask; fp64, fast arithmetic mode, ECCKD_DEVICE or ECCKD_HOST.  cloud_scaling NULL: the unmasked all-sky call.
 * (The names avoid "_fluxes" as ecckd_lw_flux_bands does.)  Refusals: the unmasked all-sky call's list in its order.
 *   Longwave, every layer count: gas optics into the work block, the scaled by-band increment in place, the solver of
 *   ecckd_rte_lw_fused without particles (60 layers: the layer-split kernel on the incremented optical depth).  The fluxes
 *   equal ecckd_gas_optics_lw_tau + ecckd_increment_scaled + ecckd_rte_lw_fused BIT FOR BIT.  Scratch: the optical depth plus
 *   what that solver takes, ecckd_lw_flux_scaled_scratch_bytes (the figures at ecckd_lw_fluxes_clear_allsky).
 *   Shortwave, every layer count: delta scaling of the band triple first (independent of the scaling), gas optics, then the
 *   scaled form of the TWO-PASS solver whatever "sw_solver" says: where the McICA form selects  bit ? tau_p : 0  it
 *   multiplies  tau_p * (double)scaling.  Agreement with gas optics + delta_scale + ecckd_increment_scaled + ecckd_rte_sw to
 *   rounding, as for the unmasked call.  Scratch: ecckd_sw_flux_scaled_scratch_bytes -- the formula at ecckd_sw_fluxes_allsky
 *   with the two-pass solver's term at every layer count.
 * NOT PROVIDED: both-skies, Jacobian, per-band, daylit and float32 forms of the fused scaled calls, the layer-systolic
 * shortwave form and an in-kernel 60-layer longwave form.  Two-stream and rescaled longwave are reachable through
 * ecckd_increment_scaled on two-stream properties followed by the existing solvers.
 * --------------------------------------------------------------------------------------- */
typedef struct ecckd_cloud_scaling ecckd_cloud_scaling_t;
int ecckd_cloud_scaling_create(int device, int nfsd, double fsd0, double dfsd, int nq, const double *values,
                               ecckd_cloud_scaling_t **table);
void ecckd_cloud_scaling_destroy(ecckd_cloud_scaling_t *table);
int ecckd_cloud_scaling_get_nfsd(const ecckd_cloud_scaling_t *table);
int ecckd_cloud_scaling_get_nq(const ecckd_cloud_scaling_t *table);
double ecckd_cloud_scaling_get_fsd0(const ecckd_cloud_scaling_t *table);
double ecckd_cloud_scaling_get_dfsd(const ecckd_cloud_scaling_t *table);
int ecckd_cloud_scaling_get_values(const ecckd_cloud_scaling_t *table, double *values);
int ecckd_cloud_scaling_lognormal(int nfsd, double fsd0, double dfsd, int nq, double *values);
int ecckd_cloud_scaling_sample(int device, int ncol, int nlay, int ngpt, int overlap, const double *cloud_frac,
                               const double *overlap_param, const double *fsd, double fsd_const,
                               const ecckd_cloud_scaling_t *table, unsigned long long seed, long long col0, float *scaling,
                               unsigned long long *mask, int memspace, void *stream);
int ecckd_increment_scaled(int device, int ncol, int nlay, int ngpt, double *tau1, double *ssa1, double *g1, int nband,
                           const int *band2gpt, const double *tau2, const double *ssa2, const double *g2, const float *scaling,
                           int memspace, void *stream);
int ecckd_increment_scaled_f32(int device, int ncol, int nlay, int ngpt, float *tau1, float *ssa1, float *g1, int nband,
                               const int *band2gpt, const float *tau2, const float *ssa2, const float *g2, const float *scaling,
                               int memspace, void *stream);
size_t ecckd_lw_flux_scaled_scratch_bytes(const ecckd_model_t *model, int ncol, int nlay);
size_t ecckd_sw_flux_scaled_scratch_bytes(const ecckd_model_t *model, int ncol, int nlay, int delta_scale);
int ecckd_lw_flux_scaled(const ecckd_model_t *model, int ncol, int nlay, const double *plev, const double *tlay,
                         const double *tsfc, const double *tlev, int ngas, const char *gas_names, const double *const *vmr,
                         const long long *vmr_col_stride, const long long *vmr_lay_stride, const double *vmr_scalar,
                         int top_at_1, int n_gauss_angles, const double *sfc_emis, const double *inc_flux, int nband_p,
                         const double *tau_p, const double *ssa_p, const float *cloud_scaling, double *flux_up,
                         double *flux_dn, int memspace, void *stream);
int ecckd_sw_flux_scaled(const ecckd_model_t *model, int ncol, int nlay, const double *plev, const double *tlay, int ngas,
                         const char *gas_names, const double *const *vmr, const long long *vmr_col_stride,
                         const long long *vmr_lay_stride, const double *vmr_scalar, int top_at_1, const double *mu0,
                         const double *toa_scale, const double *sfc_alb_dir, const double *sfc_alb_dif, int nband_p,
                         const double *tau_p, const double *ssa_p, const double *g_p, int delta_scale,
                         const float *cloud_scaling, double *flux_up, double *flux_dn, double *flux_dir, int memspace,
                         void *stream);

/* ---------------------------------------------------------------------------------------
 * Clear-sky and all-sky fluxes from one call.  A host that reports cloud radiative effect wants, for the same columns, the
 * fluxes of ecckd_*_fluxes and those of ecckd_*_fluxes_allsky[_mcica]; called one after the other they run the gas optics
 * twice on identical inputs.  ecckd_lw_fluxes_clear_allsky / ecckd_sw_fluxes_clear_allsky run it once and then both skies:
 *     flux_*_clear  =  what ecckd_lw_fluxes / ecckd_sw_fluxes writes for the arguments,
 *     flux_*        =  what ecckd_*_fluxes_allsky writes (cloud_mask NULL) or ecckd_*_fluxes_allsky_mcica (cloud_mask given),
 * BIT FOR BIT, at every layer count, in both orientations and for either value of "sw_solver" / "lw_both_skies": every pass
 * is the solver its single call would take, on the same optical depth.  fp64, fast arithmetic mode, ECCKD_DEVICE or
 * ECCKD_HOST.  tau_p / ssa_p / g_p and the mask are never written.  Shortwave: flux_dir may be NULL without flux_dir_clear,
 * and the reverse.
 *   Shortwave: delta scaling of the band triple (once), gas optics, the clear-sky solver, the all-sky / McICA solver.
 *   Longwave, 60 layers: gas optics, then ("lw_both_skies" = 0) the clear-sky and the all-sky layer-split kernel one after the
 *   other, or ("lw_both_skies" = 1) the dual-sky kernel, which evaluates the Planck sources of a cell once for both skies.
 *   Longwave, any other layer count (or a Planck table that does not fit LDS): gas optics, Planck sources into scratch once,
 *   the clear-sky solver, the by-band increment (masked with cloud_mask) in place on the scratch optical depth, the solver again.
 * Refused with a message before any device is asked for, in this order: cloud_mask with a model of more than 64 g-points;
 * the list of the unmasked all-sky call in its order; flux_up_clear or flux_dn_clear NULL; a clear-sky output pointer equal
 * to an all-sky output pointer.
 * Scratch (ECCKD_DEVICE): exactly what the corresponding all-sky call takes for the shape.  The two solver passes run one
 * after the other on the stream and share the solver room behind the optical depth, so a caller-owned block
 * (ecckd_set_stream_scratch) sized for ecckd_*_fluxes_allsky serves, and the capture rules are unchanged: capture after one
 * warm-up call on the stream, or with a caller-owned block.  Longwave at 60 layers: (ncol*nlay*ngpt + 32)*8 bytes; on the
 * general route the optical depth, the three Planck source arrays, the surface source and the solver's ring,
 * (4*ncol*nlay*ngpt + ncol*ngpt + 64)*8 + ecckd_rte_lw_scratch_bytes(ncol, nlay, ngpt) bytes; shortwave: the formula at
 * ecckd_sw_fluxes_allsky.
 * --------------------------------------------------------------------------------------- */
int ecckd_lw_fluxes_clear_allsky(const ecckd_model_t *model, int ncol, int nlay, const double *plev, const double *tlay,
                                 const double *tsfc, const double *tlev, int ngas, const char *gas_names,
                                 const double *const *vmr, const long long *vmr_col_stride, const long long *vmr_lay_stride,
                                 const double *vmr_scalar, int top_at_1, int n_gauss_angles, const double *sfc_emis,
                                 const double *inc_flux, int nband_p, const double *tau_p, const double *ssa_p,
                                 const unsigned long long *cloud_mask, double *flux_up, double *flux_dn, double *flux_up_clear,
                                 double *flux_dn_clear, int memspace, void *stream);
int ecckd_sw_fluxes_clear_allsky(const ecckd_model_t *model, int ncol, int nlay, const double *plev, const double *tlay, int ngas,
                                 const char *gas_names, const double *const *vmr, const long long *vmr_col_stride,
                                 const long long *vmr_lay_stride, const double *vmr_scalar, int top_at_1, const double *mu0,
                                 const double *toa_scale, const double *sfc_alb_dir, const double *sfc_alb_dif, int nband_p,
                                 const double *tau_p, const double *ssa_p, const double *g_p, int delta_scale,
                                 const unsigned long long *cloud_mask, double *flux_up, double *flux_dn, double *flux_dir,
                                 double *flux_up_clear, double *flux_dn_clear, double *flux_dir_clear, int memspace,
                                 void *stream);

/* ---------------------------------------------------------------------------------------
 * Single-precision fused fluxes: longwave, all-sky, McICA, both skies.  For a host built with wp = real32: the argument list
 * of the fp64 namesake with every `double` data pointer made `float`; vmr_scalar stays `const double *` and cloud_mask stays
 * `const unsigned long long *`, as in ecckd_sw_fluxes_f32 and ecckd_increment_masked_f32.  ECCKD_DEVICE (asynchronous on
 * `stream`) or ECCKD_HOST; fast arithmetic mode only; tau_p / ssa_p / g_p and the mask are never written; cloud_mask NULL in
 * a *_mcica_f32 or *_clear_allsky_f32 call is the unmasked call.  Each call answers the refusal list of its fp64 namesake, in
 * its order and with its messages, before any device is asked for (a mask with more than 64 g-points first).  No call sets a
 * thread-local.
 *
 * Longwave (ecckd_lw_fluxes_f32, _allsky_f32, _allsky_mcica_f32, _clear_allsky_f32), at every layer count: the
 * single-precision gas optics writes tau, lay_source, the two level arrays and sfc_source (float) into the work block and the
 * single-precision register-resident solver follows on them -- 1 to 4 angles, inc_flux and both orientations as
 * ecckd_rte_lw_inc_flux_f32.  The all-sky forms run rte_lw_allsky_f32_kernel, which adds the layer's particulate optical
 * depth on the cell's band where it consumes tau: tau + tau_p * (1 - ssa_p) (ssa_p NULL: tau + tau_p), and with a mask
 * tau + 0 * (1 - ssa_p) where the g-point's bit is clear -- the operations of ecckd_increment_f32 /
 * ecckd_increment_masked_f32 on one-stream optical properties, one by one.  The fluxes are therefore, BIT FOR BIT,
 *     ecckd_lw_fluxes_f32            =  ecckd_gas_optics_lw_f32 + ecckd_rte_lw_f32 (ecckd_rte_lw_inc_flux_f32 with inc_flux),
 *     ecckd_lw_fluxes_allsky_f32     =  ... with ecckd_increment_f32 of tau by the band planes in between,
 *     ..._allsky_mcica_f32           =  ... with ecckd_increment_masked_f32 in between,
 * without the read-modify-write pass over tau and without the host owning an (ncol,nlay,ngpt) array.  Both skies: the
 * clear-sky kernel and then the all-sky kernel on the same arrays (there is no dual-sky kernel).
 *   Scratch (ECCKD_DEVICE): ecckd_lw_fluxes_f32_scratch_bytes(model, ncol, nlay) bytes of the stream's block, the same for all
 *   four calls, laid out as: tau, lay_source, lev_source_inc, lev_source_dec, each A = align256(ncol*nlay*ngpt*4) bytes;
 *   sfc_source, align256(ncol*ngpt*4); the ring of the overflow solver, align256(ecckd_rte_lw_scratch_bytes(ncol, nlay,
 *   ngpt)) (0 up to 96 layers); align256(n) = n rounded up to a multiple of 256.  The partial sums of the tail split
 *   (ecckd_rte_lw_tail_scratch_bytes(device, ncol, nlay, ngpt, n_gauss_angles, 1)) follow only where the block has room for
 *   them -- a library-owned block outside a capture grows to hold them, a caller-owned block of exactly the size above runs
 *   without the split; the split does not change a bit.  24 bytes per cell go through memory between the kernels.
 *
 * Shortwave (ecckd_sw_fluxes_allsky_f32, _allsky_mcica_f32, _clear_allsky_f32): the route of the fp64 calls in float --
 * delta scaling of a copy of the band triple (ecckd_delta_scale_f32's kernel), the single-precision gas optics (total optical
 * depth only), then the solver ecckd_rte_sw_f32 takes for the shape (layer-systolic up to 60 layers, two-pass beyond or with
 * "sw_solver" = 1) in its all-sky / McICA float form, which forms ssa and g of a cell with the expressions of
 * ecckd_increment_f32 (floor 3*tiny(1._sp)) and keeps the single-precision k floor of ecckd_rte_sw_f32.  Both skies: the
 * clear-sky solver of ecckd_sw_fluxes_f32 first, on the same optical depth.  As in fp64 the fluxes agree with the composition
 * ecckd_gas_optics_sw_f32 + ecckd_delta_scale_f32 + ecckd_increment_f32 + ecckd_rte_sw_f32 to rounding, not bit for bit (ssa
 * is formed in another order); the clear-sky output of _clear_allsky_f32 equals ecckd_sw_fluxes_f32 and its all-sky output
 * equals ecckd_sw_fluxes_allsky[_mcica]_f32 bit for bit.
 *   Scratch (ECCKD_DEVICE): ecckd_sw_fluxes_allsky_f32_scratch_bytes(model, ncol, nlay, delta_scale) bytes, laid out as the
 *   fp64 block: the optical depth, align256(ncol*nlay*ngpt*4); the solver's room S; with delta_scale three planes of
 *   align256(ncol*nlay*nband*4).  S = ecckd_rte_sw_tail_scratch_bytes(device, ncol, nlay, ngpt) for the layer-systolic
 *   solver, else the larger of that and ecckd_rte_sw_scratch_bytes(ncol, nlay, ngpt).
 * The capture rules of the stream scratch hold for both: capture after one warm-up call on the stream, or with a
 * caller-owned block (ecckd_set_stream_scratch) of the size above.
 *
 * Out of scope: the Fortran shim (fp64 throughout); ecckd_sw_fluxes_daylit; the Jacobian and rescaled longwave calls in single
 * precision (the two-stream ones: "Two-stream longwave, single precision" below); per-band outputs; a single-precision Planck-recomputing longwave kernel (8 instead of 24 bytes
 * per cell between the kernels: the obvious follow-up, not measured); the in-solver addition for the fp64 general route at
 * layer counts other than 60.
 * --------------------------------------------------------------------------------------- */
size_t ecckd_lw_fluxes_f32_scratch_bytes(const ecckd_model_t *model, int ncol, int nlay);
size_t ecckd_sw_fluxes_allsky_f32_scratch_bytes(const ecckd_model_t *model, int ncol, int nlay, int delta_scale);
int ecckd_lw_fluxes_f32(const ecckd_model_t *model, int ncol, int nlay, const float *plev, const float *tlay, const float *tsfc,
                        const float *tlev, int ngas, const char *gas_names, const float *const *vmr,
                        const long long *vmr_col_stride, const long long *vmr_lay_stride, const double *vmr_scalar, int top_at_1,
                        int n_gauss_angles, const float *sfc_emis, const float *inc_flux, float *flux_up, float *flux_dn,
                        int memspace, void *stream);
int ecckd_lw_fluxes_allsky_f32(const ecckd_model_t *model, int ncol, int nlay, const float *plev, const float *tlay,
                               const float *tsfc, const float *tlev, int ngas, const char *gas_names, const float *const *vmr,
                               const long long *vmr_col_stride, const long long *vmr_lay_stride, const double *vmr_scalar,
                               int top_at_1, int n_gauss_angles, const float *sfc_emis, const float *inc_flux, int nband_p,
                               const float *tau_p, const float *ssa_p, float *flux_up, float *flux_dn, int memspace,
                               void *stream);
int ecckd_lw_fluxes_allsky_mcica_f32(const ecckd_model_t *model, int ncol, int nlay, const float *plev, const float *tlay,
                                     const float *tsfc, const float *tlev, int ngas, const char *gas_names,
                                     const float *const *vmr, const long long *vmr_col_stride, const long long *vmr_lay_stride,
                                     const double *vmr_scalar, int top_at_1, int n_gauss_angles, const float *sfc_emis,
                                     const float *inc_flux, int nband_p, const float *tau_p, const float *ssa_p,
                                     const unsigned long long *cloud_mask, float *flux_up, float *flux_dn, int memspace,
                                     void *stream);
int ecckd_lw_fluxes_clear_allsky_f32(const ecckd_model_t *model, int ncol, int nlay, const float *plev, const float *tlay,
                                     const float *tsfc, const float *tlev, int ngas, const char *gas_names,
                                     const float *const *vmr, const long long *vmr_col_stride, const long long *vmr_lay_stride,
                                     const double *vmr_scalar, int top_at_1, int n_gauss_angles, const float *sfc_emis,
                                     const float *inc_flux, int nband_p, const float *tau_p, const float *ssa_p,
                                     const unsigned long long *cloud_mask, float *flux_up, float *flux_dn, float *flux_up_clear,
                                     float *flux_dn_clear, int memspace, void *stream);
int ecckd_sw_fluxes_allsky_f32(const ecckd_model_t *model, int ncol, int nlay, const float *plev, const float *tlay, int ngas,
                               const char *gas_names, const float *const *vmr, const long long *vmr_col_stride,
                               const long long *vmr_lay_stride, const double *vmr_scalar, int top_at_1, const float *mu0,
                               const float *toa_scale, const float *sfc_alb_dir, const float *sfc_alb_dif, int nband_p,
                               const float *tau_p, const float *ssa_p, const float *g_p, int delta_scale, float *flux_up,
                               float *flux_dn, float *flux_dir, int memspace, void *stream);
int ecckd_sw_fluxes_allsky_mcica_f32(const ecckd_model_t *model, int ncol, int nlay, const float *plev, const float *tlay, int ngas,
                                     const char *gas_names, const float *const *vmr, const long long *vmr_col_stride,
                                     const long long *vmr_lay_stride, const double *vmr_scalar, int top_at_1, const float *mu0,
                                     const float *toa_scale, const float *sfc_alb_dir, const float *sfc_alb_dif, int nband_p,
                                     const float *tau_p, const float *ssa_p, const float *g_p, int delta_scale,
                                     const unsigned long long *cloud_mask, float *flux_up, float *flux_dn, float *flux_dir,
                                     int memspace, void *stream);
int ecckd_sw_fluxes_clear_allsky_f32(const ecckd_model_t *model, int ncol, int nlay, const float *plev, const float *tlay, int ngas,
                                     const char *gas_names, const float *const *vmr, const long long *vmr_col_stride,
                                     const long long *vmr_lay_stride, const double *vmr_scalar, int top_at_1, const float *mu0,
                                     const float *toa_scale, const float *sfc_alb_dir, const float *sfc_alb_dif, int nband_p,
                                     const float *tau_p, const float *ssa_p, const float *g_p, int delta_scale,
                                     const unsigned long long *cloud_mask, float *flux_up, float *flux_dn, float *flux_dir,
                                     float *flux_up_clear, float *flux_dn_clear, float *flux_dir_clear, int memspace,
                                     void *stream);

/* ---------------------------------------------------------------------------------------
 * The shortwave on the daylit columns only.  Every shortwave call above computes every column it is given; on a global grid
 * the sun is below the horizon in about half of them.  The reference's driver computes those with mu0 = 1 "for a better
 * measure of timing" and zeroes their fluxes afterwards (ecckd_rfmip_sw.F90:103-108,143-145,156-161); a production host
 * compacts the daylit columns in front of the shortwave and scatters the fluxes back.  These calls do that on the device.
 *
 * ecckd_daylit_columns (+ _f32: float mu0): day_index(0..nday-1) <- the columns i (0-BASED, ASCENDING) with
 *   mu0(i) > mu0_min, compared in double; a NaN mu0 is night.  day_index has room for ncol entries, in `memspace`; the entries
 *   from nday on are unspecified.  *nday is a HOST integer, valid on return: this is the one call of the group that
 *   synchronises (on `stream`), so it CANNOT BE CAPTURED into a graph (refused with a message on a capturing stream), while
 *   ecckd_sw_fluxes_daylit with a list made beforehand can.  The list is deterministic (ballot / popcount in the wave, a scan of
 *   the block counts; no atomic counter).  Scratch (ECCKD_DEVICE): 4*(ceil(ncol/256) + 1) bytes of the stream's block.
 *
 * ecckd_gather_columns / ecckd_scatter_columns: for hosts on the unfused route (ecckd_gas_optics_sw + ecckd_increment +
 *   ecckd_rte_sw).  An array is viewed as (ninner, ncol, nouter), ninner fastest; elem_bytes is 4 or 8 (8: fp64 and the
 *   64-bit mask words).  ninner = 1 serves every (ncol,nlay[,n]) array (nouter = nlay[*n]), nouter = 1 the (nband,ncol)
 *   albedos.
 *     gather:   dst(i,k,o) = src(i,day_index(k),o), k < nday; dst is (ninner, nday, nouter).
 *     scatter:  dst(i,day_index(k),o) = src(i,k,o), and `fill` in EVERY column of dst that the list does not hold (one pass:
 *               each element of dst is stored once); src is (ninner, nday, nouter).  fill is stored as a double in 8-byte
 *               elements and rounded to float in 4-byte elements (0 serves the mask words too).  nday = 0 fills dst.
 *   The list must be strictly ascending (the scatter finds a column by bisection).  With ECCKD_HOST a list that is not, or
 *   that leaves [0,ncol), is refused with a message.  A DEVICE list is not checked: the gather clamps an entry outside
 *   [0,ncol) and the scatter skips it, so no list can make a kernel address memory outside its arrays, but the results for
 *   such a list are undefined.  Asynchronous on `stream` with ECCKD_DEVICE, no scratch, capturable.
 *
 * ecckd_sw_fluxes_daylit: the superset of the fused shortwave calls, on the columns of the list.  After nday and day_index
 *   the argument list is that of ecckd_sw_fluxes_clear_allsky, and EVERY ARRAY IS DIMENSIONED WITH THE FULL ncol.
 *     tau_p NULL (then ssa_p, g_p, cloud_mask and the clear-sky outputs NULL too; nband_p ignored): ecckd_sw_fluxes;
 *     tau_p, ssa_p, g_p given: ecckd_sw_fluxes_allsky, with cloud_mask ecckd_sw_fluxes_allsky_mcica;
 *     flux_up_clear and flux_dn_clear given (flux_dir_clear optional) as well: ecckd_sw_fluxes_clear_allsky.
 *   The call gathers every input to nday columns, runs that call's pipeline unchanged on them -- with the solver "sw_solver"
 *   picks for nday columns, at any layer count -- and scatters each requested output into the caller's (ncol,nlay+1) array,
 *   with +0 at every level of the columns left out.  The fluxes of a listed column are BIT FOR BIT those of the existing
 *   call on the gathered columns.  nday = 0 only zeroes the outputs.  An output that is not requested is never written; the
 *   inputs are never written.  fp64, fast arithmetic mode only; ECCKD_HOST stages through the model's arena; ECCKD_DEVICE is
 *   asynchronous on `stream`.
 *   Refused with a message before any device is asked for, in this order: the list of ecckd_sw_fluxes_clear_allsky in its
 *   order (the particle entries only with tau_p given; tau_p NULL with ssa_p, g_p, cloud_mask or a clear-sky output); nday
 *   outside 0..ncol; day_index NULL with nday > 0; with ECCKD_HOST a list that is not strictly ascending or that leaves
 *   [0,ncol); then what ecckd_sw_fluxes refuses.  A device list is not checked (the kernel rule above holds).
 *   Scratch (ECCKD_DEVICE, from the stream's block; a host that owns the block, ecckd_set_stream_scratch, sizes it so), with
 *   a256 = align256 and every count taken for nday columns:
 *     ecckd_sw_fluxes_daylit_scratch_bytes(model, ncol, nday, nlay, ngas_arrays, with_particles, delta_scale, with_mask, with_clear)
 *       = what the inner call needs for nday columns (the formula at ecckd_sw_fluxes, plus 3*a256(nday*nlay*nband*8) with
 *         particles and delta_scale)
 *       + a256(nday*(nlay+1)*8) + a256(nday*nlay*8)                  plev, tlay
 *       + 2*a256(nday*8) + 2*a256(nband*nday*8)                      mu0, toa_scale (whether given or not), the two albedos
 *       + ngas_arrays*a256(nday*nlay*8)                              the gas arrays with a non-zero column stride (the others,
 *                                                                    and the scalars, are read in place)
 *       + (with_particles ? 3*a256(nday*nlay*nband*8) : 0) + (with_mask ? a256(nday*nlay*8) : 0)
 *       + (with_clear ? 6 : 3)*a256(nday*(nlay+1)*8)                 the fluxes of the inner call (direct beams whether given or not)
 *     in that order, the inner call's share first; 0 for nday = 0; ncol does not enter (the scatter works in place).  The
 *     capture rules of the stream's block apply: capture after one warm-up call on the stream, or with a caller-owned block.
 * --------------------------------------------------------------------------------------- */
int ecckd_daylit_columns(int device, int ncol, const double *mu0, double mu0_min, int *day_index, int *nday, int memspace,
                         void *stream);
int ecckd_daylit_columns_f32(int device, int ncol, const float *mu0, double mu0_min, int *day_index, int *nday, int memspace,
                             void *stream);
int ecckd_gather_columns(int device, int ninner, int ncol, int nouter, int elem_bytes, int nday, const int *day_index,
                         const void *src, void *dst, int memspace, void *stream);
int ecckd_scatter_columns(int device, int ninner, int ncol, int nouter, int elem_bytes, int nday, const int *day_index,
                          const void *src, void *dst, double fill, int memspace, void *stream);
size_t ecckd_sw_fluxes_daylit_scratch_bytes(const ecckd_model_t *model, int ncol, int nday, int nlay, int ngas_arrays,
                                            int with_particles, int delta_scale, int with_mask, int with_clear);
int ecckd_sw_fluxes_daylit(const ecckd_model_t *model, int ncol, int nlay, int nday, const int *day_index, const double *plev,
                           const double *tlay, int ngas, const char *gas_names, const double *const *vmr,
                           const long long *vmr_col_stride, const long long *vmr_lay_stride, const double *vmr_scalar,
                           int top_at_1, const double *mu0, const double *toa_scale, const double *sfc_alb_dir,
                           const double *sfc_alb_dif, int nband_p, const double *tau_p, const double *ssa_p, const double *g_p,
                           int delta_scale, const unsigned long long *cloud_mask, double *flux_up, double *flux_dn,
                           double *flux_dir, double *flux_up_clear, double *flux_dn_clear, double *flux_dir_clear, int memspace,
                           void *stream);

/* ---------------------------------------------------------------------------------------
 * Longwave surface-temperature Jacobian: the derivative of the upward flux profile with respect to the surface
 * temperature, RTE-RRTMGP's optional flux_up_Jac(ncol,nlay+1) of rte_lw (from sources%sfc_source_Jac) and, divided by its
 * surface value, ecRad's lw_derivatives.  A host gets it with the fluxes of the same call instead of calling the fluxes
 * twice, at tsfc and at tsfc + 1.  fp64.  [Parity with RTE-RRTMGP is unpinned, as for everything else about the solvers.]
 *
 *   sfc_source_jac(i,g) = B_g(tsfc(i) + 1) - B_g(tsfc(i)),  B = calculate_planck_function (src/gas_optics_ecckd.f90:275-288,
 *     the division by the f32 pi included), evaluated with the expressions that give sfc_source: tsfc + 1.0 as one fp64
 *     addition, two separately rounded Planck values, one fp64 subtraction (RRTMGP's convention: delta_Tsurf = 1 K in
 *     compute_Planck_source).  Units of sfc_source, per kelvin.
 *   flux_up_jac(i,lev) = sum_g sum_k 2 pi w_k J_kg(lev):
 *     at the surface level      J = sfc_emis(band(g), i) * sfc_source_jac(i,g),
 *     at the level above layer l  J = t_k(l) * J(level below),  t_k(l) = exp(-tau(i,l,g) * D_k),
 *     with the transmissivity the flux solver forms (the same exp, bit for bit) on the optical depth that sky's solver sees:
 *     gas only, or gas incremented by the (masked) particles exactly as the flux pass increments it.  Quadrature, 2 pi w_k
 *     scaling, g-point lanes of weight 0 and layout are those of flux_up: (ncol,nlay+1), indexed by top_at_1.  W m-2 K-1.
 *     It does not depend on inc_flux, on the layer and level sources, or on "lw_tau_thresh" / "lw_series_terms".
 *     ecRad's lw_derivatives(lev) = flux_up_jac(lev) / flux_up_jac(surface).
 *   The solver is linear in its sources, so flux_up_jac is the flux_up of rte_lw with lay_source = lev_source_inc =
 *   lev_source_dec = 0, no inc_flux and sfc_source = sfc_source_jac (the tests pin it to the oracle's rte_lw run that way).
 *
 * ecckd_planck_sfc_source_jac: sfc_source_jac(ncol,ngpt) from tsfc(ncol).  ECCKD_DEVICE: asynchronous on `stream`, no
 *   scratch; ECCKD_HOST: staged.  Refusals: those of ecckd_planck_sources for its arguments.
 * ecckd_rte_lw_jac: ecckd_rte_lw_inc_flux (inc_flux may be NULL) plus flux_up_jac.  ECCKD_HOST or ECCKD_DEVICE, any layer
 *   count.  flux_up / flux_dn are bit for bit those of ecckd_rte_lw_inc_flux with the same arguments (the same solver is
 *   launched, unchanged); flux_up_jac comes from a kernel of its own that reads tau once.  sfc_source_jac or flux_up_jac
 *   NULL, or flux_up_jac equal to a flux output, is refused with a message before any launch.  No scratch beyond what
 *   ecckd_rte_lw takes.
 * ecckd_lw_fluxes_jac: the superset of the four fused longwave calls.  tau_p NULL (with nband_p 0, ssa_p and cloud_mask
 *   NULL, no clear-sky outputs): the clear sky of ecckd_lw_fluxes; tau_p given: ecckd_lw_fluxes_allsky (cloud_mask NULL) or
 *   ecckd_lw_fluxes_allsky_mcica; flux_up_clear and flux_dn_clear given as well: ecckd_lw_fluxes_clear_allsky.  flux_up /
 *   flux_dn (and flux_*_clear) are BIT FOR BIT what that existing call writes, at every layer count, in both orientations
 *   and for every value of the solver options: its kernels are launched unchanged.  flux_up_jac is the Jacobian of the sky
 *   that flux_up holds (the all sky when particles are given); NULL: the existing call and nothing else.
 *   60 layers, "lw_jac_inline" = 1 (the default): the Jacobian form of the layer-split kernel (rte_lw_split_jac_kernel)
 *   carries the surface term through the up sweep it runs anyway -- one multiply and one accumulator add per (cell, angle);
 *   its third accumulator plane leaves room for one group per block, one wave per SIMD.  With the clear-sky outputs the call
 *   takes the two launches of "lw_both_skies" = 0 and the all-sky launch is the Jacobian form (the dual-sky kernel has none;
 *   the fluxes are the same bits either way).
 *   Otherwise ("lw_jac_inline" = 0, any other layer count, a Planck table that does not fit LDS): the stand-alone Jacobian
 *   kernel runs behind the flux pass(es) on the scratch optical depth and forms sfc_source_jac itself from tsfc and the
 *   Planck table.  At 60 layers the flux kernel adds the particles as it reads tau and leaves the scratch as gas optics wrote
 *   it, so the stand-alone kernel reads the band planes and the mask as well and applies them with the flux kernel's
 *   expressions; at any other layer count it finds tau incremented in place (both skies: behind the second pass).
 *   The two routes sum the g-points and angles of a level in different orders: they agree to rounding (1e-14 W m-2 K-1).
 *   Refused in this order: the existing call's list in its order; flux_up_jac equal to another output pointer; nband_p,
 *   ssa_p, cloud_mask or a clear-sky output without tau_p.
 *   Scratch (ECCKD_DEVICE): exactly that of the corresponding existing call -- nothing (ncol,ngpt) is staged -- so a
 *   caller-owned block sized for it serves and the capture rules are unchanged.
 * Out of scope: single precision; per-band or spectral Jacobians; the Jacobian in ecckd_lw_solver_noscat_gpt /
 *   librte_kernels_hip; the dual-sky kernel with a Jacobian; ECCKD_MIXED.
 * --------------------------------------------------------------------------------------- */
int ecckd_planck_sfc_source_jac(const ecckd_model_t *model, int ncol, const double *tsfc, double *sfc_source_jac, int memspace,
                                void *stream);
int ecckd_rte_lw_jac(int device, int ncol, int nlay, int ngpt, int top_at_1, int n_gauss_angles, const double *tau,
                     const double *lay_source, const double *lev_source_inc, const double *lev_source_dec,
                     const double *sfc_source, const double *sfc_source_jac, int nband, const int *band2gpt,
                     const double *sfc_emis, const double *inc_flux, double *flux_up, double *flux_dn, double *flux_up_jac,
                     int memspace, void *stream);
int ecckd_lw_fluxes_jac(const ecckd_model_t *model, int ncol, int nlay, const double *plev, const double *tlay,
                        const double *tsfc, const double *tlev, int ngas, const char *gas_names, const double *const *vmr,
                        const long long *vmr_col_stride, const long long *vmr_lay_stride, const double *vmr_scalar,
                        int top_at_1, int n_gauss_angles, const double *sfc_emis, const double *inc_flux, int nband_p,
                        const double *tau_p, const double *ssa_p, const unsigned long long *cloud_mask, double *flux_up,
                        double *flux_dn, double *flux_up_clear, double *flux_dn_clear, double *flux_up_jac, int memspace,
                        void *stream);

/* ---------------------------------------------------------------------------------------
 * Two-stream longwave: clouds SCATTER.  Every other longwave route of this library is the no-scattering solver and folds
 * particles into the optical depth as absorption (tau_gas + tau_p*(1 - ssa_p)).  These calls restate RTE-RRTMGP's
 * lw_solver_2stream of the v1.5 era [RTE-ext: mo_rte_solver_kernels.F90], the route rte_lw takes on ty_optical_props_2str
 * with use_2stream = .true.; like every solver here, PARITY WITH RTE-RRTMGP IS UNPINNED: the tests pin
 * the calls to an independent boundary-value solution of the two-stream equations instead.
 *   Per (column, g-point), layers counted from the top, D = 1.66:
 *     level source (memory index j = 1..nlay+1, whatever top_at_1): lev(1) = lev_source_dec(1), lev(nlay+1) =
 *       lev_source_inc(nlay), lev(j) = sqrt(lev_source_dec(j)*lev_source_inc(j-1)); lay_source is an argument, as in RTE, and
 *       is NEVER READ (it may be NULL);
 *     gamma1 = D*(1 - 0.5*ssa*(1 + g)), gamma2 = D*0.5*ssa*(1 - g), k = sqrt(max((gamma1-gamma2)*(gamma1+gamma2), 1e-12)),
 *       e1 = exp(-tau*k), e2 = e1*e1, RT = 1/(k*(1+e2) + gamma1*(1-e2)), Rdif = RT*gamma2*(1-e2), Tdif = RT*2*k*e1;
 *     tau > 1e-8: Z = (Bb - Bt)/(tau*(gamma1+gamma2)), src_up = pi*((Z+Bt) - Rdif*(-Z+Bt) - Tdif*(Z+Bb)),
 *       src_dn = pi*((-Z+Bb) - Rdif*(Z+Bb) - Tdif*(-Z+Bt)) with Bt / Bb the level sources above / below; else both 0;
 *     surface albedo 1 - sfc_emis, source pi*sfc_emis*sfc_source; adding upwards, fluxes downwards from
 *       flux_dn(top) = inc_flux (0 without one).  No quadrature: n_gauss_angles is not an argument.
 *   The two constants (1e-12, 1e-8) are RTE's and have no solver option.  Arithmetic follows ecckd_set_arithmetic as
 *   ecckd_rte_sw does (mode 1: IEEE division, sqrt, exp in the order above; mode 0: reciprocal, square root and exp of the
 *   shortwave two-stream kernel).  fp64.  A NaN or inf in one column stays in that column.  An infinite tau gives finite
 *   fluxes in mode 1 (Z = 0) and NaN fluxes for that column in mode 0 (the fast reciprocal of inf is NaN): mode 0 takes
 *   finite optical depths.
 * ecckd_rte_lw_2stream: broadband fluxes (ncol,nlay+1).  tau / ssa / g / lev_source_*(ncol,nlay,ngpt), sfc_source(ncol,ngpt),
 *   sfc_emis(nband,ncol) and band2gpt as ecckd_rte_lw; ngpt <= 256; inc_flux(ncol,ngpt) or NULL.  ECCKD_DEVICE: asynchronous
 *   on `stream`; the solver's ring (ecckd_rte_lw_2stream_scratch_bytes) comes from the stream's scratch block, so no
 *   allocation happens once a (shape, stream) pair has been seen and the capture rules are those of ecckd_rte_sw (one
 *   call before the capture, or ecckd_set_stream_scratch).  ECCKD_HOST: staged, synchronises.  Refused with a message before
 *   any launch: a null required pointer, bad sizes, a bad memspace, ECCKD_MIXED.
 * ecckd_lw_solver_2stream_gpt: RTE's kernel-level interface -- spectral fluxes (ncol,nlay+1,ngpt), sfc_emis / sfc_src /
 *   inc_flux (ncol,ngpt); IEEE arithmetic; a compatibility kernel (one thread per column and g-point).
 *   librte_kernels_hip exports it as lw_solver_2stream.
 * ecckd_rte_lw_2stream_scratch_bytes = 8 * 2*(nlay+1)*64 * min(ceil(ncol/16), 4096): one ring of two level arrays per wave.
 * ecckd_lw_fluxes_allsky_2stream: ecckd_lw_fluxes_allsky with scattering.  Gas optical depth into stream scratch, the
 *   Planck sources into scratch, then the solver, which loads the layer's band triple (tau_p, ssa_p, g_p)(ncol,nlay,nband_p)
 *   -- and the cloud-mask word, cloud_mask(ncol,nlay) or NULL, as ecckd_lw_fluxes_allsky_mcica -- beside the gas optical
 *   depth and forms the cell's (tau, ssa, g) with the operations of ecckd_increment[_masked] by band on (tau_gas, 0, 0):
 *   no per-g-point ssa or g exists in memory.  flux_up / flux_dn equal, BIT FOR BIT on finite inputs, the composed route
 *   ecckd_gas_optics_lw_tau, ecckd_planck_sources, ecckd_increment[_masked] by band on (tau, ssa = 0, g = 0),
 *   ecckd_rte_lw_2stream.  g_p and ssa_p are required (one-stream particles: ecckd_lw_fluxes_allsky).  Fast arithmetic
 *   mode; any layer count; ECCKD_DEVICE or ECCKD_HOST.  Refused in this order: cloud_mask with more than 64 g-points;
 *   nband_p different from the model's; tau_p, ssa_p or g_p NULL; reference-order arithmetic; no Planck table; tlev NULL;
 *   a host-only model.
 *   Scratch (ECCKD_DEVICE, from the stream's block), with n3 = ncol*nlay*ngpt and r32() rounding up to a multiple of 32:
 *     8*(r32(n3) + 3*n3 + r32(ncol*ngpt)) + ecckd_rte_lw_2stream_scratch_bytes(ncol, nlay, ngpt)
 *   in the order optical depth, the three Planck arrays, surface source, ring.
 * Out of scope: single precision of ecckd_lw_solver_2stream_gpt (the other two: the next block); per-band and Jacobian
 *   outputs; both skies in one call; delta scaling inside the fused
 *   call (the host calls ecckd_delta_scale on its band triple first); ECCKD_MIXED; a tail split for small calls; a
 *   Planck-recomputing form of the solver; the Fortran type-bound rte_lw(use_2stream=).  (RTE's rescaled no-scattering
 *   alternative, use_2stream = .false. with two-stream properties, is the next block.)
 * --------------------------------------------------------------------------------------- */
int ecckd_rte_lw_2stream(int device, int ncol, int nlay, int ngpt, int top_at_1, const double *tau, const double *ssa,
                         const double *g, const double *lay_source, const double *lev_source_inc, const double *lev_source_dec,
                         const double *sfc_source, int nband, const int *band2gpt, const double *sfc_emis, const double *inc_flux,
                         double *flux_up, double *flux_dn, int memspace, void *stream);
int ecckd_lw_solver_2stream_gpt(int device, int ncol, int nlay, int ngpt, int top_at_1, const double *tau, const double *ssa,
                                const double *g, const double *lay_source, const double *lev_source_inc,
                                const double *lev_source_dec, const double *sfc_emis, const double *sfc_src,
                                const double *inc_flux, double *gpt_flux_up, double *gpt_flux_dn, int memspace, void *stream);
size_t ecckd_rte_lw_2stream_scratch_bytes(int ncol, int nlay, int ngpt);
int ecckd_lw_fluxes_allsky_2stream(const ecckd_model_t *model, int ncol, int nlay, const double *plev, const double *tlay,
                                   const double *tsfc, const double *tlev, int ngas, const char *gas_names,
                                   const double *const *vmr, const long long *vmr_col_stride, const long long *vmr_lay_stride,
                                   const double *vmr_scalar, int top_at_1, const double *sfc_emis, const double *inc_flux,
                                   int nband_p, const double *tau_p, const double *ssa_p, const double *g_p,
                                   const unsigned long long *cloud_mask, double *flux_up, double *flux_dn, int memspace, void *stream);

/* ---------------------------------------------------------------------------------------
 * Two-stream longwave, single precision.  For a host built with wp = real32: ecckd_rte_lw_2stream and
 * ecckd_lw_fluxes_allsky_2stream with every `double` data pointer made `float` (vmr_scalar stays `const double *`, cloud_mask
 * `const unsigned long long *`, as in the other *_f32 fused calls).  Fast arithmetic mode only; ECCKD_DEVICE or ECCKD_HOST.
 * Per cell in float: tau, ssa, g (or the band triple), both level-source planes, sfc_emis, sfc_source, inc_flux, the ring and
 * the flux outputs; the g-point sums and the level accumulators are double, rounded to float once when the fluxes are stored.
 *   The float cell is NOT the fp64 block retyped: in float 1 - e2 loses its digits in a thin layer and under the k floor,
 *   gamma1 - gamma2 loses them near ssa = 1, and the fp64 source terms cancel quantities of size dB/tau down to a result of
 *   size tau*B (RTE's tau > 1e-8 switch means nothing at float resolution).  Every such difference is formed from its parts.
 *   Per (column, g-point), all operations in float, in this order, D = 1.66f, pi = 3.14159274f:
 *     level source: as above, sqrtf(lev_source_dec(j)*lev_source_inc(j-1)) in between;
 *     gamma1 = D*(1 - 0.5*ssa*(1 + g)), gamma2 = D*0.5*ssa*(1 - g), gm = D*(1 - ssa) [= gamma1 - gamma2], gp = gamma1 + gamma2,
 *       k = sqrtf(max(gm*gp, 1e-12)), x = tau*k, e1 = expf(-x), n1 = -expm1f(-x) [= 1 - e1], m = n1*(1 + e1) [= 1 - e2],
 *       RT = 1/(k*(2 - m) + gamma1*m), Rdif = RT*gamma2*m, Tdif = RT*2*k*e1;
 *     kn = k*n1*n1, A1 = RT*(kn + gm*m) [= 1 - Rdif - Tdif],
 *       G = x < 0.7 ? e1*(x*x*(1/3))*(1 + (x*x*(1/20))*(1 + x*x*(1/42))) : m*(1/x) - 2*e1   [= 2*e1*(sinh(x)/x - 1)],
 *       A2 = RT*(kn*(1/(tau*gp)) + k*G), dB = Bb - Bt,
 *       tau > 1e-30: src_up = pi*(Bt*A1 + dB*A2), src_dn = pi*(Bb*A1 - dB*A2); else both 0
 *       (to first order in tau both are pi*(gamma1-gamma2)*tau*(Bt+Bb)/2; the next order carries -+ dB);
 *     surface, adding and fluxes as in fp64, in float: den = 1/(1 - Rdif*albedo), src = src_up + Tdif*den*(src + albedo*src_dn),
 *       albedo = Rdif + Tdif*Tdif*albedo*den; flux_dn = (Tdif*flux_dn + Rdif*src(l+1) + src_dn)*den, flux_up = flux_dn*albedo(l+1)
 *       + src(l+1).
 *   1/y is the hardware reciprocal with one Newton step (as in every *_f32 solver), expf / expm1f / sqrtf are the device
 *   library's: tests/lw_2stream_f32_ref.py restates the block in numpy float32 with IEEE operations and is the reference of
 *   this definition, not a bit-for-bit pin of the kernel.  The threshold 0.7 is where the errors of the two forms of G cross;
 *   the floor 1e-12 is RTE's (nothing divides by 1 - e2 any more, so float needs no higher one); 1e-30 keeps the two quotients
 *   on normal numbers.  Distances from the fp64 calls: DESIGN.md section 3.  ssa = g = 1 (gp = 0) and an infinite tau give NaN
 *   fluxes for that column, as in fp64 mode 0; a NaN in one column stays in that column.
 * ecckd_rte_lw_2stream_f32: the argument list of ecckd_rte_lw_2stream.  The ring comes from the stream's block as in fp64; the
 *   call asks for ecckd_rte_lw_2stream_scratch_bytes(ncol, nlay, ngpt) and the float ring takes the first HALF of it,
 *   4 * 2*(nlay+1)*64 * min(ceil(ncol/16), 4096) bytes.  Refused in the order of the fp64 call, under this call's name: bad
 *   sizes; a null required pointer; one level buffer in place of two arrays; a bad band description; too many layers;
 *   ECCKD_MIXED; a bad memspace; then reference-order arithmetic; then the device.
 * ecckd_lw_fluxes_allsky_2stream_f32: the argument list of ecckd_lw_fluxes_allsky_2stream.  The single-precision gas optics
 *   writes tau and the Planck sources (float) into the work block, the float solver follows with the band triple and the mask
 *   word as in fp64 and forms the cell's (tau, ssa, g) with the operations of ecckd_increment[_masked]_f32 by band on
 *   (tau_gas, 0, 0).  flux_up / flux_dn equal, BIT FOR BIT on finite inputs, the composed route ecckd_gas_optics_lw_f32,
 *   ecckd_increment[_masked]_f32 by band on (tau, ssa = 0, g = 0), ecckd_rte_lw_2stream_f32.  Capture rules as the fp64 call.
 *   Refused in the fp64 call's order, under this call's name: cloud_mask with more than 64 g-points; nband_p different from
 *   the model's; tau_p, ssa_p or g_p NULL; reference-order arithmetic; no Planck table; tlev NULL; ECCKD_MIXED (named here;
 *   the fp64 call answers it as a bad memspace); a host-only model.
 *   Scratch (ECCKD_DEVICE, from the stream's block): ecckd_lw_fluxes_allsky_2stream_f32_scratch_bytes(model, ncol, nlay) =
 *     4*A + align256(ncol*ngpt*4) + align256(ecckd_rte_lw_2stream_scratch_bytes(ncol, nlay, ngpt)/2), A = align256(ncol*nlay*ngpt*4),
 *   in the order tau, lay_source (written by the gas optics, never read), lev_source_inc, lev_source_dec, sfc_source, ring.
 * Out of scope: the rescaled solver and the Jacobian in single precision; ecckd_lw_solver_2stream_gpt in float; per-band
 *   output; both skies in one two-stream call; the Fortran shim; reference-order arithmetic in float.
 * --------------------------------------------------------------------------------------- */
int ecckd_rte_lw_2stream_f32(int device, int ncol, int nlay, int ngpt, int top_at_1, const float *tau, const float *ssa,
                             const float *g, const float *lay_source, const float *lev_source_inc, const float *lev_source_dec,
                             const float *sfc_source, int nband, const int *band2gpt, const float *sfc_emis,
                             const float *inc_flux, float *flux_up, float *flux_dn, int memspace, void *stream);
size_t ecckd_lw_fluxes_allsky_2stream_f32_scratch_bytes(const ecckd_model_t *model, int ncol, int nlay);
int ecckd_lw_fluxes_allsky_2stream_f32(const ecckd_model_t *model, int ncol, int nlay, const float *plev, const float *tlay,
                                       const float *tsfc, const float *tlev, int ngas, const char *gas_names,
                                       const float *const *vmr, const long long *vmr_col_stride,
                                       const long long *vmr_lay_stride, const double *vmr_scalar, int top_at_1,
                                       const float *sfc_emis, const float *inc_flux, int nband_p, const float *tau_p,
                                       const float *ssa_p, const float *g_p, const unsigned long long *cloud_mask,
                                       float *flux_up, float *flux_dn, int memspace, void *stream);

/* ---------------------------------------------------------------------------------------
 * Rescaled longwave: cheap cloud scattering with the Gauss quadrature.  RTE-RRTMGP's lw_solver_1rescl_GaussQuad of the v1.5
 * era [RTE-ext: mo_rte_solver_kernels.F90; the method is Tang et al. 2018, J. Atmos. Sci. 75, 2217], the route rte_lw takes
 * on ty_optical_props_2str WITHOUT use_2stream = .true. -- RTE's default for two-stream properties.  The optical depth is
 * scaled by 1 - ssa*(1+g)/2, the ordinary no-scattering sweeps run on it, and the radiances receive a back-scattering
 * adjustment layer by layer.  Like every solver here, PARITY WITH RTE-RRTMGP IS UNPINNED: the
 * equations below are restated from the public source, and the tests pin the calls to a numpy restatement of them, to the
 * no-scattering solver in the two limits where they coincide, and to the two-stream solution they approximate.
 *   Per (column, g-point, quadrature angle k with secant D_k and weight w_k), layers s = 0..nlay-1 counted from the top,
 *   level s the top of layer s, in this order of operations:
 *     wb  = (ssa*(1 - g))*0.5        sc = (1 - ssa) + wb        tl = (tau*sc)*D_k        t = exp(-tl)
 *     Cn  = 0.4*(wb/sc)              CA = Cn*(1 - t*t)
 *     sdn, sup: lw_source_noscat on tl with lay_source / lev_source_inc / lev_source_dec exactly as ecckd_rte_lw (the
 *       "lw_tau_thresh" and "lw_series_terms" switches act on tl)
 *     SUA = sup - Cn*(sdn*t + sup)   SDA = sdn - Cn*(sup*t + sdn)        (formed once, with CA, beside t and sdn)
 *     sweep 1, top -> surface:  dn0[s+1] = t*dn0[s] + sdn;  dn0[0] from inc_flux as ecckd_rte_lw_inc_flux
 *                               ("lw_inc_flux_isotropic" included), 0 without one
 *     surface:                  up[nlay] = dn0[nlay]*(1 - emis) + emis*sfc_source       (the surface sees the unadjusted dn0)
 *     sweep 2, surface -> top:  up[s]   = t*up[s+1] + (SUA + CA*dn0[s])
 *     sweep 3, top -> surface:  dn[s+1] = t*dn[s]   + (SDA + CA*up[s+1]);  dn[0] = dn0[0]
 *     flux = 2*pi*w_k * radiance, summed over angles and g-points as ecckd_rte_lw
 *   The adjustment of the radiance that leaves a layer uses the radiance that enters the layer from the other side (dn0[s]
 *   in sweep 2, up[s+1] in sweep 3), so both values of top_at_1 give the same fluxes.  The constant 0.4 (Tang et al.) has no
 *   solver option.  ssa = g = 1 gives 0/0: unguarded, as in RTE -- the NaN stays in its column, as does any NaN or inf of
 *   the inputs.  With ssa = 0 the fluxes are those of ecckd_rte_lw_inc_flux; with g = 1 those of ecckd_rte_lw_inc_flux on
 *   tau*(1 - ssa) (both up to the order of the sums).  fp64.
 *   Arithmetic: the 60-layer kernels use the exp and the source-function division of the no-scattering solver
 *   (lw_layer.hpp) and IEEE division for wb/sc; the compatibility kernel is IEEE throughout.  ecckd_set_arithmetic does
 *   not act on ecckd_rte_lw_rescaled.
 * ecckd_rte_lw_rescaled: broadband fluxes (ncol,nlay+1); the arguments of ecckd_rte_lw_inc_flux with ssa and g
 *   (ncol,nlay,ngpt) behind tau; n_gauss_angles 1..4; both orientations; inc_flux or NULL.  60 layers: the layer-split
 *   kernel with three exchanges per (g-point group, angle) -- 15 layers per wave whatever "lw_split_seg" says, and
 *   "lw_solver" does not act.  Any other layer count: the compatibility kernel below into stream scratch followed by the
 *   g-point sum of ecckd_sum_broadband -- SLOW (three passes over the inputs per angle, spectral fluxes through memory).
 *   ECCKD_DEVICE: asynchronous on `stream`; scratch comes from the stream's block (capture rules of ecckd_rte_sw: one call
 *   before the capture, or ecckd_set_stream_scratch).  ECCKD_HOST: staged, synchronises.  Refused with a message before any
 *   launch and before a device is asked for, in this order: bad sizes; n_gauss_angles outside 1..4; a null required pointer
 *   (only inc_flux may be NULL); a bad band table; ECCKD_MIXED; a bad memspace.
 * ecckd_rte_lw_rescaled_scratch_bytes = 0 at 60 layers, else 8 * 3*r32(ncol*(nlay+1)*ngpt) with r32() rounding up to a
 *   multiple of 32: spectral flux_up, spectral flux_dn, and the radiances one sweep leaves for the next.
 * ecckd_lw_solver_1rescl_gpt: RTE's kernel-level interface, mirroring ecckd_lw_solver_noscat_gpt -- spectral fluxes
 *   (ncol,nlay+1,ngpt), sfc_emis / sfc_src / inc_flux (ncol,ngpt), nmus angles with Ds and weights; IEEE arithmetic; one
 *   thread per (column, g-point); any layer count.  It takes 8*r32(ncol*(nlay+1)*ngpt) bytes from the stream's block.
 * ecckd_lw_fluxes_allsky_rescaled: ecckd_lw_fluxes_allsky with the rescaled solver; the arguments of
 *   ecckd_lw_fluxes_allsky_2stream plus n_gauss_angles.  Gas optical depth into stream scratch; the solver forms the cell's
 *   (tau, ssa, g) from it and the layer's band triple (tau_p, ssa_p, g_p)(ncol,nlay,nband_p) -- and the cloud-mask word,
 *   cloud_mask(ncol,nlay) or NULL, as ecckd_lw_fluxes_allsky_mcica -- with the operations of ecckd_increment[_masked] by band
 *   on (tau_gas, 0, 0).  At 60 layers (and a Planck table that fits in LDS) no per-g-point ssa or g exists in memory: the
 *   Planck-recomputing layer-split kernel loads the band triple beside the gas optical depth.  Any other layer count: Planck
 *   sources, then the by-band increment on (tau, 0, 0), through scratch, then the compatibility route -- SLOW.  flux_up /
 *   flux_dn equal, BIT FOR BIT on finite inputs and at every layer count, the composed route ecckd_gas_optics_lw_tau,
 *   ecckd_planck_sources, ecckd_increment[_masked] by band on (tau, ssa = 0, g = 0), ecckd_rte_lw_rescaled.  Fast arithmetic
 *   mode; ECCKD_DEVICE or ECCKD_HOST; capturable in a graph after one warm-up call on the stream.  Refused in this order:
 *   cloud_mask with more than 64 g-points; nband_p different from the model's; tau_p, ssa_p or g_p NULL; reference-order
 *   arithmetic; no Planck table; tlev NULL; n_gauss_angles outside 1..4; a host-only model.
 * ecckd_lw_fluxes_allsky_rescaled_scratch_bytes (ECCKD_DEVICE, from the stream's block), n3 = r32(ncol*nlay*ngpt):
 *     60 layers:  8*n3                                              (the gas optical depth)
 *     otherwise:  8*(6*n3 + r32(ncol*ngpt)) + ecckd_rte_lw_rescaled_scratch_bytes(ncol, nlay, ngpt)
 *   in the order optical depth, ssa, g, the three Planck arrays, surface source, the solver's planes.
 * Out of scope: single precision; per-band outputs (the Jacobian and both skies in one call: the next block); delta scaling
 *   inside the fused call (the host calls ecckd_delta_scale on its band triple first); ECCKD_MIXED; a tail split for small calls; a fast form
 *   away from 60 layers; the Fortran type-bound rte_lw; RTE's bind(C) name lw_solver_1rescl_GaussQuad in librte_kernels_hip.
 * --------------------------------------------------------------------------------------- */
int ecckd_rte_lw_rescaled(int device, int ncol, int nlay, int ngpt, int top_at_1, int n_gauss_angles, const double *tau,
                          const double *ssa, const double *g, const double *lay_source, const double *lev_source_inc,
                          const double *lev_source_dec, const double *sfc_source, int nband, const int *band2gpt,
                          const double *sfc_emis, const double *inc_flux, double *flux_up, double *flux_dn, int memspace,
                          void *stream);
size_t ecckd_rte_lw_rescaled_scratch_bytes(int ncol, int nlay, int ngpt);
int ecckd_lw_solver_1rescl_gpt(int device, int ncol, int nlay, int ngpt, int top_at_1, int nmus, const double *Ds,
                               const double *weights, const double *tau, const double *ssa, const double *g,
                               const double *lay_source, const double *lev_source_inc, const double *lev_source_dec,
                               const double *sfc_emis, const double *sfc_src, const double *inc_flux, double *gpt_flux_up,
                               double *gpt_flux_dn, int memspace, void *stream);
int ecckd_lw_fluxes_allsky_rescaled(const ecckd_model_t *model, int ncol, int nlay, const double *plev, const double *tlay,
                                    const double *tsfc, const double *tlev, int ngas, const char *gas_names,
                                    const double *const *vmr, const long long *vmr_col_stride, const long long *vmr_lay_stride,
                                    const double *vmr_scalar, int top_at_1, int n_gauss_angles, const double *sfc_emis,
                                    const double *inc_flux, int nband_p, const double *tau_p, const double *ssa_p,
                                    const double *g_p, const unsigned long long *cloud_mask, double *flux_up, double *flux_dn,
                                    int memspace, void *stream);
size_t ecckd_lw_fluxes_allsky_rescaled_scratch_bytes(const ecckd_model_t *model, int ncol, int nlay);

/* ---------------------------------------------------------------------------------------
 * Rescaled longwave: clear sky and Jacobian.  What the other fused longwave calls provide, for the rescaled solver: both
 * skies from one gas-optics pass, and the surface-temperature Jacobian of flux_up (RTE's flux_up_Jac, which its rescaled
 * solver returns; ecRad's lw_derivatives).  fp64, ECCKD_DEVICE or ECCKD_HOST.
 *   The Jacobian: the three sweeps of "Rescaled longwave" with every layer, level and incident source zero.  Then dn0 == 0,
 *   the adjusted up sweep reduces to up[s] = t*up[s+1] (RTE: radn_up_Jac = trans * radn_up_Jac inside the rescaled
 *   transport), and per (column, g-point, angle k)
 *     J(surface)             = sfc_emis(band(g), i) * sfc_source_jac(i, g)
 *     J(level above layer s) = t_k(s) * J(level below),   t_k(s) = lw_exp(-((tau*sc)*D_k)),  sc = (1 - ssa) + (ssa*(1 - g))*0.5
 *     flux_up_jac(i, lev)    = sum over g and k of 2*pi*w_k * J
 *   with t_k formed operation by operation as the 60-layer flux kernel forms it on the cell's (tau, ssa, g), sfc_source_jac
 *   = B(tsfc + 1) - B(tsfc) as ecckd_planck_sfc_source_jac gives it, and the weights, layout and weight-0 lanes of flux_up.
 *   W m-2 K-1.  Under rescaling flux_dn ALSO depends on the surface temperature, through CA*up[s+1] in sweep 3: that
 *   derivative is NOT returned, as in RTE (the zero-source run's flux_dn is not zero: up to 0.29 W m-2 K-1 on the test
 *   columns).  inc_flux does not enter.
 * ecckd_rte_lw_rescaled_jac: ecckd_rte_lw_rescaled with sfc_source_jac(ncol,ngpt) behind sfc_source and
 *   flux_up_jac(ncol,nlay+1) behind flux_dn.  flux_up / flux_dn are those of ecckd_rte_lw_rescaled bit for bit (its kernels,
 *   launched unchanged); the Jacobian comes from the stand-alone Jacobian kernel on (tau, ssa, g) at every layer count (the
 *   60-layer arrays kernel is at its register limit).  No scratch beyond ecckd_rte_lw_rescaled_scratch_bytes.  Refused before
 *   any launch and before a device is asked for: the list of ecckd_rte_lw_rescaled in its order, then sfc_source_jac or
 *   flux_up_jac NULL, then flux_up_jac equal to flux_up or flux_dn.
 * ecckd_lw_fluxes_rescaled_jac: the superset of ecckd_lw_fluxes_allsky_rescaled, with flux_up_clear, flux_dn_clear and
 *   flux_up_jac (ncol,nlay+1) behind flux_dn; each may be NULL, and with all three NULL the call IS
 *   ecckd_lw_fluxes_allsky_rescaled.  flux_up / flux_dn are that call's bit for bit, with cloud_mask, at every layer count
 *   and in both orientations, whatever else is asked for.
 *   Clear-sky outputs (together or not at all): bit for bit what ecckd_lw_fluxes writes for the same atmosphere,
 *   n_gauss_angles and inc_flux, from the one scratch optical depth -- the clear-sky launch of ecckd_lw_fluxes_clear_allsky
 *   with "lw_both_skies" = 0, in front of the all-sky pass (general route: before the by-band increment, on the Planck
 *   sources the rescaled route has in scratch).  There is no dual-sky rescaled kernel.
 *   flux_up_jac: the Jacobian of the ALL sky.  60 layers and "lw_jac_inline" = 1 (the default): inside the rescaled all-sky
 *   kernel -- the surface term eps*(B(tsfc + 1) - B(tsfc)) folded through the transmissivities of the waves below and
 *   carried through the adjusted up sweep, a third accumulator plane in LDS; same occupancy (one wave per SIMD), no spill.
 *   Otherwise the stand-alone kernel behind the flux pass: at 60 layers on the gas optical depth and the (masked) band
 *   triple with the flux kernel's expressions, on the general route on the (tau, ssa, g) the increment left in scratch.
 *   The surface term is formed in the kernels from tsfc and the Planck table: nothing of size (ncol,ngpt) is staged.  The two
 *   routes sum in different orders: they agree to rounding, not bit for bit.
 *   ecckd_lw_fluxes_rescaled_jac_scratch_bytes(model, ncol, nlay, with_clear): with_clear = 0 equals
 *   ecckd_lw_fluxes_allsky_rescaled_scratch_bytes (flux_up_jac needs none).  with_clear != 0 adds, behind that block, what
 *   the clear pass needs on its general route: at 60 layers nothing for a model whose Planck table fits the clear-sky
 *   layer-split kernel (every shipped model), else 8*r32(3*ncol*nlay*ngpt + ncol*ngpt + 32 + ecckd_rte_lw_scratch_bytes/8);
 *   at any other layer count 8*r32(ecckd_rte_lw_scratch_bytes(ncol, nlay, ngpt)/8), the solver's ring.  Capturable after one
 *   warm-up call on the stream, and with ecckd_set_stream_scratch.
 *   Refused, all before the model is asked for its device: the list of ecckd_lw_fluxes_allsky_rescaled up to the angle
 *   count, in its order and with its messages; then exactly one clear-sky output NULL; then a clear-sky output equal to an
 *   all-sky output; then flux_up_jac equal to another output; then a host-only model and the rest of that list.
 * Out of scope: the two-stream solver (RTE has no Jacobian for it); a dual-sky rescaled kernel; single precision; per-band
 *   output; ECCKD_MIXED; a fast rescaled form away from 60 layers; the Fortran type-bound interface; a bind(C) name in
 *   librte_kernels_hip.
 * --------------------------------------------------------------------------------------- */
int ecckd_rte_lw_rescaled_jac(int device, int ncol, int nlay, int ngpt, int top_at_1, int n_gauss_angles, const double *tau,
                              const double *ssa, const double *g, const double *lay_source, const double *lev_source_inc,
                              const double *lev_source_dec, const double *sfc_source, const double *sfc_source_jac, int nband,
                              const int *band2gpt, const double *sfc_emis, const double *inc_flux, double *flux_up,
                              double *flux_dn, double *flux_up_jac, int memspace, void *stream);
int ecckd_lw_fluxes_rescaled_jac(const ecckd_model_t *model, int ncol, int nlay, const double *plev, const double *tlay,
                                 const double *tsfc, const double *tlev, int ngas, const char *gas_names,
                                 const double *const *vmr, const long long *vmr_col_stride, const long long *vmr_lay_stride,
                                 const double *vmr_scalar, int top_at_1, int n_gauss_angles, const double *sfc_emis,
                                 const double *inc_flux, int nband_p, const double *tau_p, const double *ssa_p,
                                 const double *g_p, const unsigned long long *cloud_mask, double *flux_up, double *flux_dn,
                                 double *flux_up_clear, double *flux_dn_clear, double *flux_up_jac, int memspace, void *stream);
size_t ecckd_lw_fluxes_rescaled_jac_scratch_bytes(const ecckd_model_t *model, int ncol, int nlay, int with_clear);

/* Spectral (per-band) fluxes: what RTE-RRTMGP callers get by passing a ty_fluxes_byband to rte_lw /
 * rte_sw instead of the ty_fluxes_broadband the reference drivers use (ecckd_rfmip_lw.F90:108-109).
 * bnd_flux_*(ncol,nlay+1,nband) = sum over the g-points of each band (one solver pass per band over its
 * contiguous g-points); flux_up / flux_dn / flux_dir (ncol,nlay+1) are optional (NULL) and hold the sum over
 * bands.  Other arguments as ecckd_rte_lw / ecckd_rte_sw. */
int ecckd_rte_lw_byband(int device, int ncol, int nlay, int ngpt, int top_at_1, int n_gauss_angles,
                        const double *tau, const double *lay_source, const double *lev_source_inc,
                        const double *lev_source_dec, const double *sfc_source, int nband,
                        const int *band2gpt, const double *sfc_emis, double *bnd_flux_up,
                        double *bnd_flux_dn, double *flux_up, double *flux_dn, int memspace, void *stream);
int ecckd_rte_sw_byband(int device, int ncol, int nlay, int ngpt, int top_at_1, const double *tau,
                        const double *ssa, const double *g, const double *mu0, const double *toa_flux,
                        int nband, const int *band2gpt, const double *sfc_alb_dir,
                        const double *sfc_alb_dif, double *bnd_flux_up, double *bnd_flux_dn,
                        double *bnd_flux_dir, double *flux_up, double *flux_dn, double *flux_dir,
                        int memspace, void *stream);
/* The same in single precision (float arrays throughout; the band sums are taken in float). */
int ecckd_rte_lw_byband_f32(int device, int ncol, int nlay, int ngpt, int top_at_1, int n_gauss_angles, const float *tau,
                            const float *lay_source, const float *lev_source_inc, const float *lev_source_dec,
                            const float *sfc_source, int nband, const int *band2gpt, const float *sfc_emis,
                            float *bnd_flux_up, float *bnd_flux_dn, float *flux_up, float *flux_dn, int memspace, void *stream);
int ecckd_rte_sw_byband_f32(int device, int ncol, int nlay, int ngpt, int top_at_1, const float *tau, const float *ssa,
                            const float *g, const float *mu0, const float *toa_flux, int nband, const int *band2gpt,
                            const float *sfc_alb_dir, const float *sfc_alb_dif, float *bnd_flux_up, float *bnd_flux_dn,
                            float *bnd_flux_dir, float *flux_up, float *flux_dn, float *flux_dir, int memspace, void *stream);

/* ---------------------------------------------------------------------------------------
 * Fused per-band fluxes: ty_fluxes_byband from the fused path -- clear sky, all-sky and McICA, longwave and shortwave.
 * The fused calls above return broadband fluxes; band fluxes (surface shortwave by band, outgoing longwave by band) were
 * to be had only from ecckd_rte_lw_byband / ecckd_rte_sw_byband, over per-g-point arrays the host holds.  These two calls
 * take the arguments of the fused calls and return
 *     bnd_flux_*(ncol,nlay+1,nband):  plane b = sum over the model's g-points band2gpt(1,b)..band2gpt(2,b),  nband =
 *                                     ecckd_model_get_nband; required (shortwave: bnd_flux_dir may be NULL),
 *     flux_up / flux_dn / flux_dir (ncol,nlay+1), each optional (NULL): the sum of the band planes in band order, made by
 *                                     the kernel behind ecckd_rte_*_byband -- the broadband members of a by-band call, NOT
 *                                     the bits of ecckd_lw_fluxes / ecckd_sw_fluxes, which add the g-points in one chain
 *                                     (the two agree to rounding).  flux_dir needs bnd_flux_dir, as in ecckd_rte_sw_byband.
 * Argument order: head, gases, boundary, particles, mask, outputs, memspace, stream.  Particles: nband_p = 0 with NULL
 * planes and NULL cloud_mask is the clear sky; nband_p = the model's band count is the all sky -- longwave tau_p with ssa_p
 * (absorption optical depth) or ssa_p NULL (one-stream particles) as ecckd_lw_fluxes_allsky, shortwave the triple tau_p,
 * ssa_p, g_p with delta_scale 0 / 1 (a library-owned copy is scaled) as ecckd_sw_fluxes_allsky; cloud_mask (ncol,nlay)
 * words or NULL as the *_mcica calls.  Inputs are never written.  fp64, fast arithmetic mode, ECCKD_DEVICE (asynchronous
 * on `stream`: one linear sequence of launches, no other stream, no atomics on global memory) or ECCKD_HOST.
 *
 * Routes.  Gas optics writes the optical depth into the stream's scratch block exactly as in the broadband fused calls;
 * then the solver the broadband call takes for the shape runs on BAND WINDOWS: a work unit solves the g-points of one band,
 * formed into groups from the band's first g-point as a launch over that band's planes alone forms them, and whatever lives
 * on the model's g-points (optical depth, Planck / solar / Rayleigh tables, inc_flux, the band planes, the mask bit) is read
 * at the model's g-point.
 *   Longwave, 60 layers (the Planck table fits LDS): ONE launch for all bands, grid (column tiles, band), of the
 *     Planck-recomputing layer-split solver in its band-window form (rte_lw_split_bands_kernel: clear, one- / two-stream
 *     particles, masked); a block stages the window's columns of the Planck table only.  No source array exists in memory.
 *   Longwave, any other layer count: the general route of ecckd_lw_fluxes -- Planck sources into scratch, the (masked)
 *     by-band increment in place on the scratch optical depth -- then the register-resident solver ONCE PER BAND on that
 *     band's planes (the padded 32..96-layer variants, the ring beyond 96 layers; a window is a pointer and a count there,
 *     the kernels are the parent's).
 *   Shortwave: ONCE PER BAND, the solver ecckd_sw_fluxes_allsky takes for the shape (layer-systolic up to 60 layers,
 *     two-pass beyond or with "sw_solver" = 1) on the band's planes of the optical depth and the band's entries of the two
 *     tables, each launch with the tail plan of its own g-point count (the plans do not change a bit); with a mask the
 *     band-window forms of the McICA kernels (rte_sw_sys_mcica_bands_kernel, rte_sw_mcica_bands_kernel), which read bit
 *     (band's first g-point + g).  No per-g-point ssa, g or source array exists in memory.
 * Measured (one MI355X, tools/bench_flux_bands.py, profiles/flux_bands.json), against the composed
 * by-band route / against the broadband fused call of the same variant: longwave 16 bands x 36 g, 60 layers (one launch)
 * 1.17-1.29x faster with particles or a mask, 1.06x (1e5 columns) and 0.97x (1e6: NOT faster) in clear sky / 1.33-1.47x the
 * broadband call; longwave 137 layers (per band) 0.88-0.89x: SLOWER than the composed route / 1.50-1.61x; shortwave 5 bands x
 * 27 g (per band) 60 layers 1.19-1.41x faster / 1.13-1.30x, 137 layers 1.00-1.07x / 1.17-1.20x.
 *
 * What the planes equal.  Longwave, every variant: the route ecckd_gas_optics_lw -> [ecckd_increment(_masked) by band] ->
 * ecckd_rte_lw_byband BIT FOR BIT (with inc_flux: ecckd_rte_lw_inc_flux on each band's planes).  Shortwave clear sky without
 * toa_scale: ecckd_gas_optics_sw -> ecckd_rte_sw_byband bit for bit.  Shortwave all-sky, McICA or with toa_scale: that route
 * with ecckd_delta_scale / ecckd_increment(_masked) in between, to rounding (ssa is formed in a different order, as in
 * ecckd_sw_fluxes_allsky; tests/test_gpu_flux_bands.py holds 1e-9 * max(1, max|flux_dn|)).  A model with one band: plane 0
 * and the broadband members are the bits of ecckd_lw_fluxes / ecckd_lw_fluxes_allsky[_mcica].
 *
 * Scratch (ECCKD_DEVICE; a host that owns the stream's block sizes it so; capture after one warm-up call on the stream, or
 * with a caller-owned block):
 *   ecckd_lw_flux_bands_scratch_bytes(model, ncol, nlay): what ecckd_lw_fluxes takes -- (ncol*nlay*ngpt + 32)*8 bytes at 60
 *     layers; on the general route (4*ncol*nlay*ngpt + ncol*ngpt + 64)*8 + ecckd_rte_lw_scratch_bytes(ncol, nlay, ngpt).
 *   ecckd_sw_flux_bands_scratch_bytes(model, ncol, nlay, delta_scale): the block of ecckd_sw_fluxes_allsky,
 *     align256(ncol*nlay*ngpt*8) + S + (delta_scale ? 3*align256(ncol*nlay*nband*8) : 0), in that order, where S is the
 *     largest solver term (ecckd_sw_fluxes: the tail scratch of the layer-systolic solver, else the larger of ring and tail
 *     scratch) over ngpt and the g-point counts of the bands: a band's launch plans its tail for its own count, and a plan
 *     a wide launch declines a narrow one may take.  Where the term of ngpt is the largest the block is exactly
 *     that of ecckd_sw_fluxes_allsky.
 *   Both return 0 for ncol <= 0, nlay <= 0 or a NULL model; nothing is added for band output (the planes are the caller's).
 *
 * Refused with a message that begins with the call's name, before any device is asked for, in this order: NULL model; a
 * cloud_mask with a model of more than 64 g-points; nband_p neither 0 nor the model's band count; nband_p > 0 with a
 * required plane NULL (longwave tau_p; shortwave any of the triple); nband_p = 0 with a plane or cloud_mask given;
 * [shortwave] delta_scale outside {0,1}; reference-order arithmetic mode; a model without a Planck table (longwave) /
 * without a solar table (shortwave); [longwave] tlev NULL; [longwave] n_gauss_angles outside 1..4; bnd_flux_up or
 * bnd_flux_dn NULL; [shortwave] flux_dir without bnd_flux_dir; two outputs that are the same array; a memspace other than
 * ECCKD_DEVICE / ECCKD_HOST (ECCKD_MIXED included); a model that is not finalized; a host-only model; then bad ncol / nlay
 * and NULL inputs.
 *
 * Out of scope: single precision; the rescaled and two-stream longwave solvers and the Jacobian by band; both skies in one
 * by-band call; ecckd_sw_fluxes_daylit by band; band output restricted to the surface and the top (a host slices the
 * planes); ecckd_rte_lw_byband / ecckd_rte_sw_byband themselves, which stay as they are; one launch for all bands on the
 * general longwave route and in the shortwave.
 * --------------------------------------------------------------------------------------- */
size_t ecckd_lw_flux_bands_scratch_bytes(const ecckd_model_t *model, int ncol, int nlay);
int ecckd_lw_flux_bands(const ecckd_model_t *model, int ncol, int nlay, const double *plev, const double *tlay,
                        const double *tsfc, const double *tlev, int ngas, const char *gas_names,
                        const double *const *vmr, const long long *vmr_col_stride, const long long *vmr_lay_stride,
                        const double *vmr_scalar, int top_at_1, int n_gauss_angles, const double *sfc_emis,
                        const double *inc_flux, int nband_p, const double *tau_p, const double *ssa_p,
                        const unsigned long long *cloud_mask, double *bnd_flux_up, double *bnd_flux_dn, double *flux_up,
                        double *flux_dn, int memspace, void *stream);
size_t ecckd_sw_flux_bands_scratch_bytes(const ecckd_model_t *model, int ncol, int nlay, int delta_scale);
int ecckd_sw_flux_bands(const ecckd_model_t *model, int ncol, int nlay, const double *plev, const double *tlay, int ngas,
                        const char *gas_names, const double *const *vmr, const long long *vmr_col_stride,
                        const long long *vmr_lay_stride, const double *vmr_scalar, int top_at_1, const double *mu0,
                        const double *toa_scale, const double *sfc_alb_dir, const double *sfc_alb_dif, int nband_p,
                        const double *tau_p, const double *ssa_p, const double *g_p, int delta_scale,
                        const unsigned long long *cloud_mask, double *bnd_flux_up, double *bnd_flux_dn, double *bnd_flux_dir,
                        double *flux_up, double *flux_dn, double *flux_dir, int memspace, void *stream);

/* ---------------------------------------------------------------------------------------
 * Cloud optics: liquid and ice water paths and effective radii per (column, layer) to the particulate properties on the
 * model's bands -- the planes the all-sky calls above take as tau_p, ssa_p, g_p (or op2 of ecckd_increment).  A host model
 * carries water paths and radii, not optical properties; this is the step between them.  The reference's drivers have no
 * such path (clear-sky RFMIP only), so there is no counterpart call in the reference tree: the call restates the
 * look-up-table form of RTE-RRTMGP's ty_cloud_optics%cloud_optics [RTE-ext: extensions/cloud_optics/mo_cloud_optics.F90
 * of the v1.5 era, compute_all_from_table and the combination of the phases in cloud_optics], which every all-sky
 * RTE-RRTMGP driver calls between gas_optics and increment.  RTE-RRTMGP is not part of the reference tree, so PARITY WITH
 * IT IS UNPINNED; the definition below is what the tests pin (tests/cloud_optics_ref.py restates it in numpy, and the
 * results are equal BIT FOR BIT in fp64 and in float: the build has FMA contraction off, every line below is one
 * correctly rounded IEEE operation in the precision of the call).  The Pade form of ty_cloud_optics is out of scope.
 *
 * Tables.  For each phase x in {liq, ice}: lut_ext (mass extinction, m2 g-1), lut_ssa, lut_asy of shape (nsize_x, nband),
 * size index fastest, covering the effective radii [radx_lwr, radx_upr] (microns) evenly:
 *     step = (radx_upr - radx_lwr)/(nsize_x - 1).
 * The ice tables carry a third dimension, (nsize_ice, nband, nrghice); the roughness icergh (1-based) is an argument of
 * the compute call, not state of the object (per-call state is passed explicitly in this C ABI).
 * ecckd_cloud_optics_create_lut takes HOST tables and makes the device copy once (device -1: a host-only object whose
 * getters and refusals work and whose compute call fails).  A slope table[i+1] - table[i] is formed there: it is the same
 * subtraction.  Refused with a message, in this order: handle NULL; nband < 1; nsize_liq or nsize_ice < 2; nrghice < 1;
 * radliq_upr <= radliq_lwr; radice_upr <= radice_lwr (a NaN bound too); a NULL table; no such device.
 *
 * ecckd_cloud_optics (+ _f32).  clwp, ciwp: water paths (g m-2), reliq, reice: effective radii (microns), all (ncol,nlay);
 * tau, ssa, g: (ncol,nlay,nband); column fastest.  Per cell and phase, with wp, re, the phase's tables (1-based below) and
 * nsize, r_lwr, step:
 *     cloudy = wp > 0                                   (NaN, 0, negative: not cloudy)
 *     if cloudy:
 *       s     = (re - r_lwr)/step
 *       index = min(floor(s)+1, nsize-1), then at least 1        (a NaN s takes index 1)
 *       fint  = s - (index-1)
 *       t   = wp * (ext(index) + fint*(ext(index+1)-ext(index)))
 *       ts  = t  * (ssa(index) + fint*(ssa(index+1)-ssa(index)))
 *       tsg = ts * (asy(index) + fint*(asy(index+1)-asy(index)))
 *     else t = ts = tsg = +0       (a select, not a product: re, and a NaN in it, does not reach a clear cell)
 *   With (lt, lts, ltsg) of the liquid and (it, its, itsg) of the ice, per band:
 *     two-stream (ssa and g given):   tau = lt+it;  tssa = lts+its;  g = (ltsg+itsg)/max(eps,tssa);  ssa = tssa/max(eps,tau)
 *     one-scalar (ssa and g NULL):    tau = (lt-lts) + (it-its)                  (the absorption optical depth)
 *   eps = epsilon(1.0) of the precision (2^-52, 2^-23); max(eps,x) is x where x > eps, else eps.  A clear cell gives
 *   tau = ssa = g = +0.  The lower clamp of index is this project's addition: it keeps an out-of-range or NaN radius in a
 *   DEVICE array from reading outside the table -- such a radius extrapolates (fint outside [0,1]) or gives NaN, in that
 *   cell only, and never faults.  _f32: the tables and the four radius bounds are rounded to float first (the slopes and
 *   the step are then float operations), everything above in float.
 *   Refused with a message before anything is launched, in this order: object NULL; icergh outside 1..nrghice; ssa
 *   without g or g without ssa; bad ncol / nlay; clwp, ciwp, reliq, reice or tau NULL; bad memspace; then, with HOST
 *   input arrays only (ECCKD_HOST, ECCKD_MIXED), as RTE's check_values does: a cloudy cell whose liquid radius lies
 *   outside [radliq_lwr, radliq_upr] (or is NaN); the same for ice; a negative liquid water path; a negative ice water
 *   path; then a host-only object; no device.  With ECCKD_DEVICE arrays the values are not checked (the call stays
 *   asynchronous; the rule ecckd_delta_scale states for `forward`) and the clamp above applies.
 *   ECCKD_DEVICE is asynchronous on `stream` and uses no scratch, so it is capture-safe without a warm-up; ECCKD_HOST
 *   stages through the device and synchronises; ECCKD_MIXED: host inputs, tau / ssa / g device buffers (synchronises).
 *   Kernel: one lane per cell, bands walked with coalesced plane stores; both phases' tables for the chosen roughness as
 *   (value, slope) pairs in LDS while they fit 32 KiB per block (five blocks stay resident per CU), that is while
 *     (ssa ? 3 : 2) * nband * ((nsize_liq-1) + (nsize_ice-1)) * 2*sizeof(real) <= 32768,
 *   else read in place through L2; a phase no lane of a wave holds is skipped, so clear waves read no table.
 * --------------------------------------------------------------------------------------- */
typedef struct ecckd_cloud_lut ecckd_cloud_optics_t; /* replaces type(ty_cloud_optics), LUT form */
int ecckd_cloud_optics_create_lut(int nband, int nsize_liq, int nsize_ice, int nrghice, double radliq_lwr, double radliq_upr,
                                  double radice_lwr, double radice_upr, const double *lut_extliq, const double *lut_ssaliq,
                                  const double *lut_asyliq, const double *lut_extice, const double *lut_ssaice,
                                  const double *lut_asyice, int device, ecckd_cloud_optics_t **cloud_optics);
void ecckd_cloud_optics_destroy(ecckd_cloud_optics_t *cloud_optics);
int ecckd_cloud_optics_get_nband(const ecckd_cloud_optics_t *cloud_optics);
int ecckd_cloud_optics_get_nrghice(const ecckd_cloud_optics_t *cloud_optics);
double ecckd_cloud_optics_get_min_radius_liq(const ecckd_cloud_optics_t *cloud_optics);
double ecckd_cloud_optics_get_max_radius_liq(const ecckd_cloud_optics_t *cloud_optics);
double ecckd_cloud_optics_get_min_radius_ice(const ecckd_cloud_optics_t *cloud_optics);
double ecckd_cloud_optics_get_max_radius_ice(const ecckd_cloud_optics_t *cloud_optics);
int ecckd_cloud_optics(const ecckd_cloud_optics_t *cloud_optics, int ncol, int nlay, const double *clwp, const double *ciwp,
                       const double *reliq, const double *reice, int icergh, double *tau, double *ssa, double *g, int memspace,
                       void *stream);
int ecckd_cloud_optics_f32(const ecckd_cloud_optics_t *cloud_optics, int ncol, int nlay, const float *clwp, const float *ciwp,
                           const float *reliq, const float *reice, int icergh, float *tau, float *ssa, float *g, int memspace,
                           void *stream);

/* ---------------------------------------------------------------------------------------
 * Aerosol optics: aerosol species, particle sizes, layer masses and relative humidity per (column, layer) to the
 * particulate properties on the model's bands -- the aerosol half of the planes the all-sky calls above take as tau_p,
 * ssa_p, g_p.  A host model carries tracers, size bins and humidity, not optical properties; this is the step between
 * them.  The counterpart in RTE-RRTMGP is ty_aerosol_optics_rrtmgp_merra [RTE-ext:
 * extensions/aerosols/mo_aerosol_optics_rrtmgp_merra.F90: load, aerosol_optics].  RTE-RRTMGP is not part of the reference
 * tree, so PARITY WITH IT IS UNPINNED; the definition below is this project's own and is what the tests pin
 * (tests/aerosol_optics_ref.py restates it in numpy, and the results are equal BIT FOR BIT in fp64 and in float: the build
 * has FMA contraction off, every line below is one correctly rounded IEEE operation in the precision of the call).  It
 * keeps RTE's table layout, type codes and call shape, and goes beyond it in two ways: several species per call (nspec;
 * nspec = 1 is RTE's call), summed in registers with each plane stored once, and `accumulate`, which adds the aerosol onto
 * planes that already hold the clouds ("add them up on the band grid first" then costs no pass of its own).
 * Out of scope: reading MERRA or any aerosol netCDF file (the host hands over tables); parity with RTE-RRTMGP's bits;
 * aerosol inside the gas-optics or solver kernels; per-g-point aerosol properties; delta scaling of the aerosol planes
 * (ecckd_delta_scale serves that).
 *
 * Type codes (RTE's): 0 none, 1 dust, 2 sea salt, 3 sulfate, 4 black carbon hydrophilic, 5 black carbon hydrophobic,
 * 6 organic carbon hydrophilic, 7 organic carbon hydrophobic.
 * Tables: HOST arrays in Fortran order (first index fastest), nval = 3 in the order mass extinction (m2 kg-1), ssa,
 * asymmetry:  bin_lims(2,nbin) microns;  rh_levels(nrh) as a fraction;  dust_tbl(nval,nbin,nband);
 * salt_tbl(nval,nrh,nbin,nband);  sulf_tbl, bcar_rh_tbl, ocar_rh_tbl (nval,nrh,nband);  bcar_tbl, ocar_tbl (nval,nband).
 * ecckd_aerosol_optics_create_lut makes the device copy once (device -1: a host-only object whose getters and refusals
 * work and whose compute call fails).  The differences d(i) = rh_levels(i+1) - rh_levels(i) and the slopes
 * tbl(i+1) - tbl(i) along the humidity are formed there: they are the same subtractions.  Refused with a message, in this
 * order: handle NULL; nband or nbin < 1; nrh < 2; rh_levels NULL, not strictly increasing, or NaN; bin_lims NULL, a bin with
 * lims(1,b) >= lims(2,b), or lims(2,b) > lims(1,b+1); a NULL table; no such device.
 *
 * ecckd_aerosol_optics (+ _f32).  aero_type (int32), aero_size (microns), aero_mass (kg m-2): (ncol,nlay,nspec);
 * relhum: (ncol,nlay); tau, ssa, g: (ncol,nlay,nband); column fastest; nspec >= 1.
 * Per cell, once (1-based):
 *     i = 1 + number of j in 2..nrh-1 with relhum >= rh_levels(j)          (a NaN takes 1)
 *     w = (relhum - rh_levels(i)) / d(i)
 *     w = w > 0 ? w : 0;  w = w < 1 ? w : 1     (below the first / above the last level: the edge value; NaN: 0)
 * Per species s, with type k, mass m and size r:
 *     active = 1 <= k <= 7 and m > 0                       (NaN, 0, negative mass: not active)
 *     dust, salt:  bin = the first b in 1..nbin with bin_lims(1,b) <= r and r < bin_lims(2,b)
 *                  no such b (NaN too): not active
 *     for q in ext, ssa, asy at the band:
 *         humidity-dependent types (2,3,4,6):  v_q = tbl_q(i) + w*(tbl_q(i+1) - tbl_q(i))
 *         others (1,5,7):                      v_q = tbl_q
 *     t = m*v_ext;  ts = t*v_ssa;  tsg = ts*v_asy          inactive: t = ts = tsg = +0 (a select, not a product)
 * Per band, over s = 1..nspec in order, starting from +0:
 *     T += t;  TS += ts;  TSG += tsg;  A += (t - ts)
 * Outputs:
 *     two-stream (ssa and g given):  tau = T;  ssa = TS/max(eps,T);  g = TSG/max(eps,TS)
 *     one-scalar (ssa and g NULL):   tau = A                                     (the absorption optical depth)
 *   eps = epsilon(1.0) of the precision (2^-52, 2^-23); max(eps,x) is x where x > eps, else eps, as in cloud optics.
 *   accumulate = 1: the planes hold op1 on entry.  With (tau2, ssa2, g2) exactly what accumulate = 0 would have stored,
 *   ecckd_increment's increment_2stream_by_2stream (one-scalar: increment_1scalar_by_1scalar) formulas are applied,
 *   operation for operation, with that call's own eps (3*tiny):
 *     tau12 = tau1 + tau2;  tscat1 = tau1*ssa1;  tscat2 = tau2*ssa2;  tsg2 = tscat2*g2;  tauscat12 = tscat1 + tscat2
 *     g1 = (tscat1*g1 + tsg2)/max(eps,tauscat12);  ssa1 = tauscat12/max(eps,tau12);  tau1 = tau12        (tau1 = tau1 + A)
 *   so the result is BIT FOR BIT the plain call into fresh planes followed by ecckd_increment on the band grid.
 *   _f32: the tables, bin limits and levels are rounded to float first (d(i) and the slopes are then float operations),
 *   everything above in float.
 *   Refused with a message before anything is launched, in this order: object NULL; nspec < 1; ssa without g or g without
 *   ssa; bad ncol / nlay; aero_type, aero_size, aero_mass, relhum or tau NULL; accumulate not 0 or 1; bad memspace; then,
 *   with HOST input arrays only (ECCKD_HOST, ECCKD_MIXED), the value checks: a type outside 0..7; a negative mass; an
 *   active dust or salt cell whose size lies in no bin; relhum outside [0,1], or NaN, in a cell that has an active
 *   humidity-dependent species; then a host-only object; no device.  With ECCKD_DEVICE arrays nothing is checked (the call
 *   stays asynchronous): a type outside 0..7 is "none", and no value can index outside a table -- i is a count bounded by
 *   the number of levels, the bin comes from comparisons, and an inactive species is not computed.
 *   ECCKD_DEVICE is asynchronous on `stream` and uses no scratch, so it is capture-safe without a warm-up; ECCKD_HOST
 *   stages through the device and synchronises; ECCKD_MIXED: host inputs, tau / ssa / g device buffers (synchronises).
 *   Kernel: one lane per cell, the interval and weight once per cell, the table entry once per species, bands the outer
 *   and species the inner loop with T, TS, TSG in registers, coalesced plane stores.  The tables are one image of
 *   (value, slope) pairs, [quantity][band][entry], with
 *     entries = nbin*nrh + 3*(nrh-1) + 2         (dust nbin; salt nbin*(nrh-1); sulfate, bc, oc hydrophilic nrh-1 each; bc, oc)
 *     image bytes = (ssa ? 3 : 2) * nband * entries * 2*sizeof(real)
 *   staged in LDS while image bytes <= 32768 (as for cloud optics), else read in place through L2.  Launch rule: blocks of
 *   256 cells, min(ceil(ncol*nlay/256), CUs * min(B, floor(163840 / image bytes) on the LDS route)) with B = 8 for nspec <= 2,
 *   4 for nspec <= 8 and for nspec > 16, 2 for 9 <= nspec <= 16 (the waves per SIMD the kernel is compiled for); the
 *   remaining cells by grid stride.  Up to 16 species keep their state in registers; more take a slower instantiation
 *   with the same results.
 * --------------------------------------------------------------------------------------- */
#define ECCKD_AERO_NONE 0
#define ECCKD_AERO_DUST 1
#define ECCKD_AERO_SALT 2
#define ECCKD_AERO_SULF 3
#define ECCKD_AERO_BCAR_RH 4
#define ECCKD_AERO_BCAR 5
#define ECCKD_AERO_OCAR_RH 6
#define ECCKD_AERO_OCAR 7
typedef struct ecckd_aerosol_lut ecckd_aerosol_optics_t; /* replaces type(ty_aerosol_optics_rrtmgp_merra) */
int ecckd_aerosol_optics_create_lut(int nband, int nbin, int nrh, const double *bin_lims, const double *rh_levels,
                                    const double *dust_tbl, const double *salt_tbl, const double *sulf_tbl, const double *bcar_tbl,
                                    const double *bcar_rh_tbl, const double *ocar_tbl, const double *ocar_rh_tbl, int device,
                                    ecckd_aerosol_optics_t **aerosol_optics);
void ecckd_aerosol_optics_destroy(ecckd_aerosol_optics_t *aerosol_optics);
int ecckd_aerosol_optics_get_nband(const ecckd_aerosol_optics_t *aerosol_optics);
int ecckd_aerosol_optics_get_nbin(const ecckd_aerosol_optics_t *aerosol_optics);
int ecckd_aerosol_optics_get_nrh(const ecckd_aerosol_optics_t *aerosol_optics);
int ecckd_aerosol_optics(const ecckd_aerosol_optics_t *aerosol_optics, int ncol, int nlay, int nspec, const int *aero_type,
                         const double *aero_size, const double *aero_mass, const double *relhum, int accumulate, double *tau,
                         double *ssa, double *g, int memspace, void *stream);
int ecckd_aerosol_optics_f32(const ecckd_aerosol_optics_t *aerosol_optics, int ncol, int nlay, int nspec, const int *aero_type,
                             const float *aero_size, const float *aero_mass, const float *relhum, int accumulate, float *tau,
                             float *ssa, float *g, int memspace, void *stream);

/* ---------------------------------------------------------------------------------------
 * Heating rates: the divergence of the net flux across each layer to the temperature tendency in K s-1 -- the last step
 * of a model's radiation call, after the flux calls above.  A radiation step needs it for up to four flux sets (longwave
 * and shortwave, clear and all sky), and per band where the host asks for by-band fluxes (ecckd_rte_*_byband).  The
 * counterpart in RTE-RRTMGP is compute_heating_rate [RTE-ext: extensions/mo_heating_rates.F90], which every all-sky
 * driver built on it calls after rte_lw / rte_sw.  RTE-RRTMGP is not part of the reference tree, so PARITY WITH IT IS
 * UNPINNED; the definition below restates its published expression and is what the tests pin (tests/heating_rate_ref.py
 * restates it in numpy, and the results are equal BIT FOR BIT in fp64 and in float: the build has FMA contraction off,
 * the quotient is a division, not a product with a reciprocal, and every line below is one correctly rounded IEEE
 * operation in the precision of the call).
 * Out of scope: heating rates as an extra output of the fused flux calls or inside the solver kernels (they move about
 * 1/30 of a flux call's bytes); net-flux or surface / top-of-atmosphere summaries.
 *
 * ecckd_heating_rate (+ _f32).  All arrays column fastest.
 *   flux_up, flux_dn: (ncol,nlay+1,nouter), W m-2.  For shortwave flux_dn is the TOTAL downward flux, direct beam
 *     included, as ecckd_rte_sw and the fused shortwave calls return it.
 *   plev: (ncol,nlay+1), Pa; shared by every outer plane.
 *   cp: (ncol,nlay), J kg-1 K-1, or NULL.  The host's own -- for instance moist -- specific heat per cell; it replaces
 *     cp_dry, which is then not looked at.
 *   heating_rate: (ncol,nlay,nouter), K s-1.  It must not alias an input.
 *   nouter = 1 for broadband fluxes; nouter = nband for the bnd_flux_* arrays of the by-band calls; a host that stacks
 *     its flux sets (longwave / shortwave, clear / all sky) in one allocation passes any other count.
 *   grav (m s-2) and cp_dry (J kg-1 K-1) are arguments, not library state; the customary values grav = 9.80665 and
 *     cp_dry = 1004.64 are the defaults of the Python and Fortran interfaces.
 * Per cell, with l the layer's index in memory (0-based) and levels l, l+1 its two edges:
 *     du   = flux_up[l+1] - flux_up[l]
 *     dd   = flux_dn[l+1] - flux_dn[l]
 *     dnet = du - dd
 *     dp   = plev[l+1] - plev[l]
 *     c    = cp ? cp[l] : cp_dry
 *     heating_rate[l] = (dnet * grav) / (c * dp)
 *   There is no top_at_1 argument because the expression does not depend on the orientation: with the levels stored the
 *   other way round du, dd (so dnet) and dp all change sign exactly -- a - b and b - a round to each other's negation --
 *   and the quotient of two negated operands is the same quotient.  Reversing the level axis of the inputs therefore
 *   reverses the layer axis of the result bit for bit.
 *   dp == 0 or a NaN gives what IEEE gives (an infinity or a NaN; the sign and payload of a NaN are the device's), in
 *   that cell only.
 *   _f32: the arrays are float; grav and cp_dry stay double in the signature and are rounded to float once; everything
 *   above in float.
 *   Refused with a message before anything is launched, in this order: ncol, nlay or nouter < 1; flux_up, flux_dn, plev or
 *   heating_rate NULL; grav not finite or not > 0, then -- without cp -- cp_dry not finite or not > 0; bad memspace; no
 *   such device.  The arrays' values are not checked, in any memory space.
 *   ECCKD_DEVICE is asynchronous on `stream` and uses no scratch, so it is capture-safe without a warm-up; ECCKD_HOST
 *   stages through the device and synchronises; ECCKD_MIXED: host inputs, heating_rate a device buffer (synchronises).
 *   Kernel: lanes along columns, one lane per (column, outer plane) walking the layers with the previous level's two
 *   fluxes and pressure in registers, so each flux level is loaded once; the planes of a column block run next to each
 *   other, so the pressures (and cp) leave HBM once and later planes find them in the caches.  64-bit offsets throughout
 *   (ncol*(nlay+1)*nouter may pass 2^31).  Launch rule: blocks of 256 columns of one plane,
 *   min(ceil(ncol/256)*nouter, 8*CUs), the rest by grid stride.  Algorithmic bytes:
 *     sizeof(real) * ncol * ((2*nouter + 1)*(nlay+1) + (nouter + [cp])*nlay)
 * --------------------------------------------------------------------------------------- */
int ecckd_heating_rate(int device, int ncol, int nlay, int nouter, const double *flux_up, const double *flux_dn,
                       const double *plev, double grav, double cp_dry, const double *cp, double *heating_rate,
                       int memspace, void *stream);
int ecckd_heating_rate_f32(int device, int ncol, int nlay, int nouter, const float *flux_up, const float *flux_dn,
                           const float *plev, double grav, double cp_dry, const float *cp, float *heating_rate,
                           int memspace, void *stream);

/* ---------------------------------------------------------------------------------------
 * Device memory for host languages without a HIP binding of their own (the Fortran shim's device-resident
 * twins of ty_optical_props / ty_source_func_lw own their buffers through these).  to_device: 1 = host to
 * device, 0 = device to host; synchronous.
 * --------------------------------------------------------------------------------------- */
int ecckd_device_malloc(int device, size_t bytes, void **ptr);
int ecckd_device_free(int device, void *ptr);
int ecckd_device_memcpy(int device, void *dst, const void *src, size_t bytes, int to_device);

/* ---------------------------------------------------------------------------------------
 * calculate_planck_function x 3 alone (src/gas_optics_ecckd.f90:245-289 as gas_optics_int applies it, :407-424):
 * lay_source(ncol,nlay,ngpt) from tlay, lev_source_inc / lev_source_dec from tlev(ncol,nlay+1) (tlev may be NULL: the
 * level sources are then left alone), sfc_source(ncol,ngpt) from tsfc.  Device arrays (ECCKD_DEVICE), fp64,
 * asynchronous on `stream`.  The same kernel ecckd_gas_optics_lw runs beside its optical-depth kernel.
 * --------------------------------------------------------------------------------------- */
int ecckd_planck_sources(const ecckd_model_t *model, int ncol, int nlay, const double *tlay, const double *tlev,
                         const double *tsfc, double *lay_source, double *lev_source_inc, double *lev_source_dec,
                         double *sfc_source, int memspace, void *stream);

/* ---------------------------------------------------------------------------------------
 * Launch plan of a gas_optics call (no counterpart in the reference; works on host-only models,
 * device -1, and launches nothing): how the library would run gas_optics for this model, gas list
 * (names only; LW if the model has a Planck table, else SW), size, precision and the current
 * arithmetic mode.
 *   plan[0] kernel passes over the gas list (<= 10 gases and one look_up_table gas per pass)
 *   plan[1] 1: first pass is the fused kernel, 0: reference-order tau kernel
 *   plan[2] 1: the Planck sources ride in that pass (LW), 0: separate Planck kernel / SW
 *   plan[3] pressure rows of the LDS slab      plan[4] Planck-table rows staged in LDS (ntp = whole table)
 *   plan[5] column chunks (grid.x)             plan[6] LDS bytes per block
 *   plan[7] g-points per chunk of the item pipeline
 * --------------------------------------------------------------------------------------- */
int ecckd_gas_optics_plan(const ecckd_model_t *model, int ncol, int nlay, int single_precision,
                          int ngas, const char *gas_names, int *plan);
/* The same with the shape of gas_desc: vmr_is_scalar[j] != 0 says gas j would be passed as one number (a null
 * pointer: every gas is an array).  Writes min(nplan, ECCKD_PLAN_LEN) entries; beyond the eight above:
 *   plan[8] bilinear slots of the kernel instantiation (2, 5, 7 or 10)
 *   plan[9] gases folded into the merged slot ("gas_merge_scalars" below; 0: none) */
#define ECCKD_PLAN_LEN 10
int ecckd_gas_optics_plan_ex(const ecckd_model_t *model, int ncol, int nlay, int single_precision,
                             int ngas, const char *gas_names, const int *vmr_is_scalar, int nplan, int *plan);

/* ---------------------------------------------------------------------------------------
 * Arithmetic mode of gas_optics (process-wide, atomic; read once per call).
 *   0 (default) fast: one fused kernel per call; the interpolation weights of a cell are
 *               multiplied out once and each coefficient costs one FMA.  Same formula as
 *               src/gas_optics_ecckd.f90:167-221, re-associated: tau differs from mode 1 by a
 *               few ulp.  Planck sources are identical in both modes.
 *   1           reference order: every product and sum in the order the Fortran expressions
 *               spell, no FMA contraction, gases accumulated in gas_desc order (:370).  tau then
 *               differs from an IEEE evaluation of the reference only through the device log().
 *   The shortwave solver follows the mode too.  Mode 1: IEEE division, the device library's sqrt and exp, the adding
 *   recurrences operation by operation in the restated order.  Mode 0 (fp64): reciprocals as v_rcp_f64 + one third-order
 *   step, sqrt and exp without the library's range handling (~1 ulp), multiply-add pairs of the recurrences fused, the
 *   pair a wave hands upwards from a division-free form of the adding recurrence, the flux recurrence pre-multiplied --
 *   fluxes within 1e-11 W m-2 of mode 1 (tests/test_gpu_round3.py: optical depths from 1e-12 to inf, NaN columns).
 *   Mode 0 raises "sw_k_floor" to the smallest normal double if it is set below.
 *   The longwave solver is the same in both modes; its division and exp are written out (csrc/lw_layer.hpp): the division
 *   gives the bits of `/` for optical depths x secant below 1e290 and ~1e-290 instead of less beyond (up to inf).
 * --------------------------------------------------------------------------------------- */
int ecckd_set_arithmetic(int mode);
int ecckd_get_arithmetic(void);

/* ---------------------------------------------------------------------------------------
 * Version switches of the solvers (process-wide; read once per call).  RTE-RRTMGP is an un-pinned dependency
 * of the reference (.github/workflows/continuous-integration.yml:98-102 checks out its default branch), and a few
 * details of rte_lw / rte_sw changed between releases.  The defaults are the v1.5-era forms; a host linked
 * against a later RTE-RRTMGP selects the matching forms here.  bench.py prints the active values.  PARITY UNPINNED: both
 * forms of every switch restate RTE-RRTMGP from the published sources -- the library is not in the reference tree and
 * the reference holds no fixture for it; the tests check the HIP solvers against this repository's
 * CPU restatement with the same switch, nothing more.
 *   "lw_tau_thresh"          lw_source_noscat uses the series below this tau*D (default sqrt(epsilon(1._wp));
 *                            later releases: sqrt(sqrt(epsilon)));  <= 0 restores the default
 *   "lw_series_terms"        2: tau*(0.5 - tau/3) (default);  3: tau*(0.5 + tau*(-1/3 + tau/8))
 *   "lw_inc_flux_isotropic"  0: I_dn(top) = inc_flux/(2 pi w_k) per angle (default);
 *                            1: inc_flux/pi (flux_dn(top) == inc_flux with any number of angles)
 *   "sw_k_floor"             k = sqrt(max((gamma1-gamma2)(gamma1+gamma2), sw_k_floor)), default 1e-12
 *                            (the single-precision solvers, unless it is set to 1e-6 or more, bound a cell of optical
 *                            depth tau by min(1e-6, 1e-4 / tau^2) instead: at 1e-12 float resolves nothing of a
 *                            conservative layer, ssa == 1 -- fluxes 8-12 W m-2 off, with the bound within 0.01 W m-2;
 *                            ecckd_get_solver_option reports the option as it was set)
 *   "sw_dir_clamp"           1: Rdir = max(0,min(Rdir,1-Tnoscat)), Tdir = max(0,min(Tdir,1-Tnoscat-Rdir))
 *                            (v1.6+); 0: no clamp (default)
 * Implementation choices through the same call (results agree to ~1e-16 relative; bench.py prints them too):
 *   "lw_solver"              fp64, 60 layers: 0 register-resident solver (one wave per SIMD), 1 layer-split solver
 *                            (waves of a block share a tile and take 10-15 layers each; three waves per SIMD)
 *   "lw_split_seg"           layers per wave of the layer-split solver: 10 (default), 12 or 15
 *   "lw_tail_split"          register-resident solver: 1 (default) the tiles beyond the last full round of waves (one
 *                            wave per SIMD) are solved one g-point pair per wave and summed in g-point order by a
 *                            second small kernel -- bit-identical fluxes, no idle SIMDs in the last round (1e5 columns:
 *                            3 125 tiles on 1 024 SIMDs).  Needs up to 64 MiB of stream scratch, taken only when it
 *                            can be had without an error (not inside a graph capture that has not seen the call
 *                            before, not beyond a caller-owned buffer): 0 switches it off.  A host that hands its own
 *                            block over (ecckd_set_stream_scratch) sizes it with ecckd_rte_lw_tail_scratch_bytes /
 *                            ecckd_rte_sw_tail_scratch_bytes (+ ecckd_rte_*_scratch_bytes where that is not 0)
 *   "sw_tail_split"          the same for rte_sw: 1 (default), 0 off; bit-identical fluxes.  Layer-systolic solver: the
 *                            tiles beyond the last full round of blocks (one block per CU; every tile of a call of
 *                            less than 16 384 columns) one g-point per block, up to 128 MiB of partial sums.  Two-pass
 *                            solver: calls that do not fill one round of its persistent grid, one g-point group per wave
 *   "sw_solver"              0 (default): layer-systolic solver (kernels_rte_sw_sys.hip: the two-stream coefficients are
 *                            computed once and stay in registers between the sweeps, the layers of a column are spread
 *                            over the waves of a block; at most 60 layers, no scratch ring; deeper calls take the
 *                            two-pass kernel); 1: two-pass kernel (any layer count; reads tau / ssa / g twice, scratch
 *                            ring) for every call.  Either value serves every shortwave entry point (fp64, fp32,
 *                            by band, ecckd_sw_fluxes).  The same two-stream coefficients per (column, g-point);
 *                            the fast mode's adding recurrences and the g-point sums differ in order (sequential /
 *                            shuffle tree): the two agree to the last bits
 *   "lw_both_skies"          ecckd_lw_fluxes_clear_allsky at 60 layers: 0 the clear-sky and the all-sky layer-split kernel
 *                            one after the other on the same optical depth; 1 (default: 1.09-1.11x faster than 0 at 1e5 columns,
 *                            1.04-1.05x at 1e6) the dual-sky kernel (rte_lw_split_both_kernel: Planck sources once per cell,
 *                            both skies in one pass, one wave per SIMD).  Bit-identical fluxes
 *   "lw_jac_inline"          ecckd_lw_fluxes_jac at 60 layers: 1 (default: 1.22-1.29x the time of the call without the
 *                            Jacobian, against 1.33-1.39x for 0, at 1e5 and 1e6 columns) flux_up_jac from the Jacobian form
 *                            of the layer-split kernel (rte_lw_split_jac_kernel); 0 the flux kernel, then the stand-alone
 *                            Jacobian kernel on the scratch optical depth.  Bit-identical fluxes; the Jacobians agree to
 *                            rounding
 *   "gas_merge_scalars"      fast arithmetic mode, fp64: 1 (default) the gases of gas_desc given as ONE number for the call
 *                            (vmr pointer NULL + vmr_scalar; get_vmr broadcasts them, src/gas_optics_ecckd.f90:351) and
 *                            the none_ composite share one table sum_k m_k*coefficient_k, m_k = vmr | vmr - reference | 1,
 *                            built on the fly: tau = ... + simple_weight * bilinear(merged table) instead of one
 *                            interpolation per gas (same real-number formula; the per-gas clamp :234-238 is kept
 *                            because only gases with m_k >= 0 and tables without negative entries are merged);
 *                            0: every gas interpolated on its own
 *   "gas_tile_sync"          fused gas-optics kernel (every mode and precision): 1 the waves of a block meet at an execution
 *                            barrier before every tile of columns, so that they write the tile's output planes together
 *                            (first-level address translations of a plane shared instead of fetched per wave); 0
 *                            they run free between the segment boundaries; -1 (default) what measured faster in each mode: 1 in
 *                            the longwave call (fp64: gas optics + rte_lw 1.0-1.4 % faster at 1e6 columns, 1.2-1.9 % at 1e5;
 *                            fp32 3-6 %) and in the shortwave call (2.3-2.8 % at 1e5 columns), 0 in
 *                            ecckd_gas_optics_lw_tau, where it costs 1-2 % of the kernel.  The same bits either way ("Address translation")
 *   "gas_input_ahead"        fused gas-optics kernel, longwave mode (both precisions): 1 a wave loads the per-column inputs of
 *                            its next tile of columns before it starts the stores of the tile in hand, 0 it loads them at the
 *                            top of the tile, behind those stores; -1 (default) what measured faster: 1 in fp64 (gas optics + rte_lw
 *                            0.5-0.9 % faster at 1e6 columns than with 0), 0 in fp32 (where 1 costs 3-4 %).  The shortwave and
 *                            tau-only modes ignore the option.  The same bits either way ("Layer-edge sources")
 *   "gas_wave_roles"         fp64 longwave gas optics over the fp64 image of the tables: 1 the kernel whose blocks of 768 threads
 *                            split the work of a tile by kind -- eight waves compute and store the optical depth, four the
 *                            Planck sources -- wherever it is built (7 or 2 gas slots, g-point count a multiple of 4); 0 never
 *                            (every wave does all the work of its columns); -1 (default) where it measured faster than the
 *                            commit before it: the seven-slot shapes (gas optics + rte_lw 2.5 % faster at 1e6 columns with the
 *                            32-g table, 2.8 % with the 36-g table, 1.5 % at 1e5 columns).  Single precision, the shortwave and
 *                            tau-only modes and the float32 image ("gas_slab_f32") keep their kernels.  The same bits either way
 *                            ("Wave roles")
 * --------------------------------------------------------------------------------------- */
int ecckd_set_solver_option(const char *name, double value);
int ecckd_get_solver_option(const char *name, double *value);

/* ---------------------------------------------------------------------------------------
 * Solver scratch (no counterpart in the reference).  ecckd_rte_sw (always) and ecckd_rte_lw (more than 96
 * layers) keep per-wave rings in global memory.  By default the library owns one block per (device, stream),
 * allocated at the first call that needs it and reused by every later call on that stream without any
 * synchronisation; inside a stream capture nothing is allocated (a call that would have to fails with a
 * message).  ecckd_set_stream_scratch hands a caller-owned device buffer over for the calls on `stream`
 * (buffer == NULL, bytes == 0 takes it back); ecckd_*_scratch_bytes say how much a shape needs (0: none);
 * ecckd_release_scratch synchronises the device and frees every library-owned block (caller-owned buffers stay
 * registered).  A block that was handed to a captured call belongs to that graph: the next eager call on the stream
 * takes a fresh one, so a graph may be replayed on any stream; graphs captured back to back on one stream share a
 * block (replay those on one stream), and a graph must be destroyed before ecckd_release_scratch.
 * --------------------------------------------------------------------------------------- */
size_t ecckd_rte_lw_scratch_bytes(int ncol, int nlay, int ngpt);
size_t ecckd_rte_sw_scratch_bytes(int ncol, int nlay, int ngpt);   /* (two-pass solver: "sw_solver" = 1, or more than 60 layers;
                                                                     an upper bound for fp32 as well; ecckd_sw_fluxes adds
                                                                     its optical depth: see the fused shortwave path) */
/* What the tail splits ("lw_tail_split", "sw_tail_split") of a call of this shape would take on top, with the
 * solver options as they are now (0: the call would not split). */
size_t ecckd_rte_lw_tail_scratch_bytes(int device, int ncol, int nlay, int ngpt, int n_gauss_angles, int single_precision);
size_t ecckd_rte_sw_tail_scratch_bytes(int device, int ncol, int nlay, int ngpt);
int ecckd_set_stream_scratch(int device, void *stream, void *buffer, size_t bytes);
int ecckd_release_scratch(int device);

/* ---------------------------------------------------------------------------------------
 * Measurement hooks (no counterpart in the reference, which has no timers: SURVEY.md §5).
 * While enabled, every kernel launch is bracketed by HIP events recorded on the stream the
 * kernel is launched on.  ecckd_prof_report waits for the recorded events, sums the elapsed
 * time per kernel name ("gas_lw_fused", "tau", "planck", "rte_lw", "rte_sw"), clears the records and returns
 * the number of distinct kernels; names is max_kernels records of ECCKD_NAME_LEN bytes.
 * --------------------------------------------------------------------------------------- */
int ecckd_prof_enable(int on);
int ecckd_prof_report(int max_kernels, char *names, double *total_ms, long long *launches);

/* Library / build identification ("gfx950", compile flags); never NULL. */
const char *ecckd_build_info(void);

#ifdef __cplusplus
}
#endif
#endif
