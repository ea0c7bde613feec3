/*
 * rte_kernels_lw_2stream_hip.h -- librte_kernels_hip.so: RTE-RRTMGP's two-stream longwave solver kernel under its own
 * bind(C) name, implemented on the MI355X by ecckd_lw_solver_2stream_gpt of librte_ecckd_hip.so.  Included by
 * rte_kernels_hip.h, whose conventions hold: every argument by reference, host arrays, column-major, top_at_1 a C _Bool,
 * flux_dn(:,top,:) holds the diffuse incident flux on entry, a failure prints ecckd_last_error() and stops the process.
 *
 *   subroutine lw_solver_2stream(ncol, nlay, ngpt, top_at_1, tau, ssa, g, lay_source, lev_source_inc, lev_source_dec,
 *                sfc_emis, sfc_src, flux_up, flux_dn) bind(C, name="lw_solver_2stream")
 *
 * [RTE-ext: restated from the public v1.5-era mo_rte_solver_kernels.F90; parity with RTE-RRTMGP is unpinned.]
 * tau / ssa / g / lay_source / lev_source_*(ncol,nlay,ngpt), sfc_emis / sfc_src(ncol,ngpt), flux_*(ncol,nlay+1,ngpt).
 * lay_source is an argument, as in RTE, and is never read.  The equations are in include/ecckd_hip.h.
 * Why a header of its own: the test suite pins the exact list of names declared in rte_kernels_hip.h
 * (tests/test_capi_host.py, through __graft_entry__.rte_kernel_symbols()), so the prototype lives here and that header
 * includes this one; tests/test_lw_2stream_host.py checks this header's names against the library's exports.
 */
#ifndef RTE_KERNELS_LW_2STREAM_HIP_H
#define RTE_KERNELS_LW_2STREAM_HIP_H
#include <stdbool.h>
#ifdef __cplusplus
extern "C" {
#endif

void lw_solver_2stream(const int *ncol, const int *nlay, const int *ngpt, const bool *top_at_1, const double *tau,
                       const double *ssa, const double *g, const double *lay_source, const double *lev_source_inc,
                       const double *lev_source_dec, const double *sfc_emis, const double *sfc_src, double *flux_up,
                       double *flux_dn);

#ifdef __cplusplus
}
#endif
#endif
