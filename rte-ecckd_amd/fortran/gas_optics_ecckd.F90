! gas_optics_ecckd.F90 -- drop-in replacement of the reference module `gas_optics_ecckd`
! (src/gas_optics_ecckd.f90): same module name, same public type ty_gas_optics_ecckd with the same
! type-bound procedures and argument lists, but the arithmetic runs on an MI355X through the C ABI
! of librte_ecckd_hip.so (include/ecckd_hip.h).  This file contains NO numerics: every procedure is
! a marshalling shim over one `bind(C)` entry point.
!
!   reference                                   here
!   ------------------------------------------  ------------------------------------------------
!   type(ty_gas_optics_ecckd) public members    opaque device-resident handle (type(c_ptr))
!   load_and_init(ecckd, file, gases)           err = ecckd%load(file [, available_gases] [, device])
!     (mo_load_coefficients.F90:19)             -> ecckd_model_load (own netCDF-3 reader)
!   ecckd%gas_optics(play,plev,tlay,tsfc,       same call                 -> ecckd_gas_optics_lw
!          gas_desc,optical_props,sources,tlev=)  (gas_optics_int, :381)
!   ecckd%gas_optics(play,plev,tlay,gas_desc,   same call                 -> ecckd_gas_optics_sw
!          optical_props,toa_src)                 (gas_optics_ext, :431)
!   get_ngas, get_gases, source_is_internal/    same names                -> ecckd_model_get_*
!   external, get_press_min/max, get_temp_min/max
!
! Differences a caller can observe: `this` carries no tables (they live on the GPU); sources%
! lay_source is never reallocated (the reference reallocates it, :266-269 via :407); a failing
! C call returns its message through the same character(len=128) result.
module gas_optics_ecckd
  use, intrinsic :: iso_c_binding
  use mo_gas_concentrations, only: ty_gas_concs
  use mo_ecckd_device, only: ty_optical_props_1scl_dev, ty_optical_props_2str_dev, ty_source_func_lw_dev, &
                             ECCKD_HOST, ECCKD_MIXED
  use mo_gas_optics, only: ty_gas_optics
  use mo_optical_props, only: ty_optical_props_arry, ty_optical_props_2str
  use mo_rte_kind, only: wp
  use mo_source_functions, only: ty_source_func_lw
  implicit none
  private

  integer, parameter, public :: none_ = 0            ! src/gas_optics_ecckd.f90:54-57
  integer, parameter, public :: linear = 1
  integer, parameter, public :: look_up_table = 2
  integer, parameter, public :: relative_linear = 3
  integer, parameter :: name_len = 32

  type, extends(ty_gas_optics), public :: ty_gas_optics_ecckd
    type(c_ptr) :: handle = c_null_ptr     !< ecckd_model_t*, owns the device-resident tables
  contains
    procedure, public :: load
    procedure, public :: finalize
    procedure, public :: source_is_internal
    procedure, public :: source_is_external
    procedure, public :: get_ngas
    procedure, public :: get_gases
    procedure, public :: get_press_min
    procedure, public :: get_press_max
    procedure, public :: get_temp_min
    procedure, public :: get_temp_max
    procedure, public :: gas_optics_int
    procedure, public :: gas_optics_ext
    procedure, public :: planck_sfc_source_jac   !< extension: sources%sfc_source_Jac = B(tsfc + 1) - B(tsfc)
    procedure, public :: lw_fluxes          !< extension: gas_optics + rte_lw in one call (fused longwave path)
    procedure, public :: sw_fluxes          !< extension: gas_optics + rte_sw in one call (fused shortwave path)
    procedure, public :: lw_fluxes_allsky   !< extension: lw_fluxes with particulate optics on the model's bands
    procedure, public :: sw_fluxes_allsky   !< extension: sw_fluxes with particulate optics on the model's bands
    procedure, public :: lw_flux_bands      !< extension: lw_fluxes / lw_fluxes_allsky with one flux plane per band of the model
    procedure, public :: sw_flux_bands      !< extension: sw_fluxes / sw_fluxes_allsky with one flux plane per band of the model
    procedure, public :: sw_fluxes_daylit   !< extension: sw_fluxes on the columns with mu0 > mu0_min only, zeros in the others
    procedure, public :: sample_cloud_mask  !< extension: McICA cloud mask from cloud fractions (ecckd_cloud_mask_sample)
    procedure, public :: sample_cloud_scaling  !< extension: sampled optical-depth scaling (ecckd_cloud_scaling_sample)
    procedure, public :: lw_flux_scaled     !< extension: lw_fluxes_allsky with a sampled optical-depth scaling (ecckd_lw_flux_scaled)
    procedure, public :: sw_flux_scaled     !< extension: sw_fluxes_allsky with a sampled optical-depth scaling (ecckd_sw_flux_scaled)
  end type ty_gas_optics_ecckd

  interface
    function c_model_load(filename, device, model) bind(C, name="ecckd_model_load") result(rc)
      import c_char, c_int, c_ptr
      character(kind=c_char), dimension(*), intent(in) :: filename
      integer(c_int), value :: device
      type(c_ptr), intent(out) :: model
      integer(c_int) :: rc
    end function c_model_load
    subroutine c_model_destroy(model) bind(C, name="ecckd_model_destroy")
      import c_ptr
      type(c_ptr), value :: model
    end subroutine c_model_destroy
    function c_last_error() bind(C, name="ecckd_last_error") result(msg)
      import c_ptr
      type(c_ptr) :: msg
    end function c_last_error
    pure function c_get_ngpt(model) bind(C, name="ecckd_model_get_ngpt") result(n)
      import c_ptr, c_int
      type(c_ptr), value :: model
      integer(c_int) :: n
    end function c_get_ngpt
    pure function c_get_nband(model) bind(C, name="ecckd_model_get_nband") result(n)
      import c_ptr, c_int
      type(c_ptr), value :: model
      integer(c_int) :: n
    end function c_get_nband
    pure function c_get_ngas(model) bind(C, name="ecckd_model_get_ngas") result(n)
      import c_ptr, c_int
      type(c_ptr), value :: model
      integer(c_int) :: n
    end function c_get_ngas
    pure function c_get_gas_name(model, idx, name) bind(C, name="ecckd_model_get_gas_name") result(rc)
      import c_ptr, c_int, c_char
      type(c_ptr), value :: model
      integer(c_int), value :: idx
      character(kind=c_char), dimension(*), intent(inout) :: name
      integer(c_int) :: rc
    end function c_get_gas_name
    pure function c_is_internal(model) bind(C, name="ecckd_model_source_is_internal") result(n)
      import c_ptr, c_int
      type(c_ptr), value :: model
      integer(c_int) :: n
    end function c_is_internal
    pure function c_is_external(model) bind(C, name="ecckd_model_source_is_external") result(n)
      import c_ptr, c_int
      type(c_ptr), value :: model
      integer(c_int) :: n
    end function c_is_external
    pure function c_press_min(model) bind(C, name="ecckd_model_get_press_min") result(v)
      import c_ptr, c_double
      type(c_ptr), value :: model
      real(c_double) :: v
    end function c_press_min
    pure function c_press_max(model) bind(C, name="ecckd_model_get_press_max") result(v)
      import c_ptr, c_double
      type(c_ptr), value :: model
      real(c_double) :: v
    end function c_press_max
    pure function c_temp_min(model) bind(C, name="ecckd_model_get_temp_min") result(v)
      import c_ptr, c_double
      type(c_ptr), value :: model
      real(c_double) :: v
    end function c_temp_min
    pure function c_temp_max(model) bind(C, name="ecckd_model_get_temp_max") result(v)
      import c_ptr, c_double
      type(c_ptr), value :: model
      real(c_double) :: v
    end function c_temp_max
    function c_get_band2gpt(model, band2gpt) bind(C, name="ecckd_model_get_band2gpt") result(rc)
      import c_ptr, c_int
      type(c_ptr), value :: model
      integer(c_int), dimension(*), intent(out) :: band2gpt
      integer(c_int) :: rc
    end function c_get_band2gpt
    function c_get_band_lims(model, lims) bind(C, name="ecckd_model_get_band_lims_wvn") result(rc)
      import c_ptr, c_int, c_double
      type(c_ptr), value :: model
      real(c_double), dimension(*), intent(out) :: lims
      integer(c_int) :: rc
    end function c_get_band_lims
    function c_gas_optics_lw(model, ncol, nlay, plev, tlay, tsfc, tlev, ngas, gas_names, vmr, cs, ls, &
                             scalar, tau, lay_source, lev_inc, lev_dec, sfc_source, memspace, stream) &
        bind(C, name="ecckd_gas_optics_lw") result(rc)
      import c_ptr, c_int, c_double, c_char, c_long_long
      type(c_ptr), value :: model
      integer(c_int), value :: ncol, nlay, ngas, memspace
      real(c_double), dimension(*), intent(in) :: plev, tlay, tsfc
      type(c_ptr), value :: tlev
      character(kind=c_char), dimension(*), intent(in) :: gas_names
      type(c_ptr), dimension(*), intent(in) :: vmr
      integer(c_long_long), dimension(*), intent(in) :: cs, ls
      real(c_double), dimension(*), intent(in) :: scalar
      type(c_ptr), value :: tau, lay_source, lev_inc, lev_dec, sfc_source   ! host (ECCKD_HOST) or device (ECCKD_MIXED)
      type(c_ptr), value :: stream
      integer(c_int) :: rc
    end function c_gas_optics_lw
    function c_gas_optics_sw(model, ncol, nlay, plev, tlay, ngas, gas_names, vmr, cs, ls, scalar, tau, &
                             ssa, g, toa_src, memspace, stream) bind(C, name="ecckd_gas_optics_sw") result(rc)
      import c_ptr, c_int, c_double, c_char, c_long_long
      type(c_ptr), value :: model
      integer(c_int), value :: ncol, nlay, ngas, memspace
      real(c_double), dimension(*), intent(in) :: plev, tlay
      character(kind=c_char), dimension(*), intent(in) :: gas_names
      type(c_ptr), dimension(*), intent(in) :: vmr
      integer(c_long_long), dimension(*), intent(in) :: cs, ls
      real(c_double), dimension(*), intent(in) :: scalar
      type(c_ptr), value :: tau, ssa, g                                     ! host (ECCKD_HOST) or device (ECCKD_MIXED)
      real(c_double), dimension(*), intent(inout) :: toa_src
      type(c_ptr), value :: stream
      integer(c_int) :: rc
    end function c_gas_optics_sw
    function c_lw_fluxes(model, ncol, nlay, plev, tlay, tsfc, tlev, ngas, gas_names, vmr, cs, ls, scalar, top_at_1, nmus, &
                         sfc_emis, inc_flux, flux_up, flux_dn, memspace, stream) bind(C, name="ecckd_lw_fluxes") result(rc)
      import c_ptr, c_int, c_double, c_char, c_long_long
      type(c_ptr), value :: model
      integer(c_int), value :: ncol, nlay, ngas, top_at_1, nmus, memspace
      real(c_double), dimension(*), intent(in) :: plev, tlay, tsfc, tlev, sfc_emis
      character(kind=c_char), dimension(*), intent(in) :: gas_names
      type(c_ptr), dimension(*), intent(in) :: vmr
      integer(c_long_long), dimension(*), intent(in) :: cs, ls
      real(c_double), dimension(*), intent(in) :: scalar
      type(c_ptr), value :: inc_flux
      real(c_double), dimension(*), intent(inout) :: flux_up, flux_dn
      type(c_ptr), value :: stream
      integer(c_int) :: rc
    end function c_lw_fluxes
    function c_planck_sfc_source_jac(model, ncol, tsfc, sfc_source_jac, memspace, stream) &
        bind(C, name="ecckd_planck_sfc_source_jac") result(rc)
      import c_ptr, c_int, c_double
      type(c_ptr), value :: model
      integer(c_int), value :: ncol, memspace
      real(c_double), dimension(*), intent(in) :: tsfc
      real(c_double), dimension(*), intent(inout) :: sfc_source_jac
      type(c_ptr), value :: stream
      integer(c_int) :: rc
    end function c_planck_sfc_source_jac
    ! the superset of the fused longwave calls with flux_up_jac; tau_p / ssa_p / cloud_mask / the clear-sky outputs may be null
    function c_lw_fluxes_jac(model, ncol, nlay, plev, tlay, tsfc, tlev, ngas, gas_names, vmr, cs, ls, scalar, top_at_1, nmus, &
                             sfc_emis, inc_flux, nband_p, tau_p, ssa_p, cloud_mask, flux_up, flux_dn, flux_up_clear, &
                             flux_dn_clear, flux_up_jac, memspace, stream) bind(C, name="ecckd_lw_fluxes_jac") result(rc)
      import c_ptr, c_int, c_double, c_char, c_long_long
      type(c_ptr), value :: model
      integer(c_int), value :: ncol, nlay, ngas, top_at_1, nmus, nband_p, memspace
      real(c_double), dimension(*), intent(in) :: plev, tlay, tsfc, tlev, sfc_emis
      character(kind=c_char), dimension(*), intent(in) :: gas_names
      type(c_ptr), dimension(*), intent(in) :: vmr
      integer(c_long_long), dimension(*), intent(in) :: cs, ls
      real(c_double), dimension(*), intent(in) :: scalar
      type(c_ptr), value :: inc_flux, tau_p, ssa_p, cloud_mask, flux_up_clear, flux_dn_clear
      real(c_double), dimension(*), intent(inout) :: flux_up, flux_dn, flux_up_jac
      type(c_ptr), value :: stream
      integer(c_int) :: rc
    end function c_lw_fluxes_jac
    function c_sw_fluxes(model, ncol, nlay, plev, tlay, ngas, gas_names, vmr, cs, ls, scalar, top_at_1, mu0, toa_scale, &
                         sfc_alb_dir, sfc_alb_dif, flux_up, flux_dn, flux_dir, memspace, stream) &
        bind(C, name="ecckd_sw_fluxes") result(rc)
      import c_ptr, c_int, c_double, c_char, c_long_long
      type(c_ptr), value :: model
      integer(c_int), value :: ncol, nlay, ngas, top_at_1, memspace
      real(c_double), dimension(*), intent(in) :: plev, tlay, mu0, sfc_alb_dir, sfc_alb_dif
      character(kind=c_char), dimension(*), intent(in) :: gas_names
      type(c_ptr), dimension(*), intent(in) :: vmr
      integer(c_long_long), dimension(*), intent(in) :: cs, ls
      real(c_double), dimension(*), intent(in) :: scalar
      type(c_ptr), value :: toa_scale, flux_dir
      real(c_double), dimension(*), intent(inout) :: flux_up, flux_dn
      type(c_ptr), value :: stream
      integer(c_int) :: rc
    end function c_sw_fluxes
    function c_lw_fluxes_allsky(model, ncol, nlay, plev, tlay, tsfc, tlev, ngas, gas_names, vmr, cs, ls, scalar, top_at_1, nmus, &
                                sfc_emis, inc_flux, nband_p, tau_p, ssa_p, flux_up, flux_dn, memspace, stream) &
        bind(C, name="ecckd_lw_fluxes_allsky") result(rc)
      import c_ptr, c_int, c_double, c_char, c_long_long
      type(c_ptr), value :: model
      integer(c_int), value :: ncol, nlay, ngas, top_at_1, nmus, nband_p, memspace
      real(c_double), dimension(*), intent(in) :: plev, tlay, tsfc, tlev, sfc_emis, tau_p
      character(kind=c_char), dimension(*), intent(in) :: gas_names
      type(c_ptr), dimension(*), intent(in) :: vmr
      integer(c_long_long), dimension(*), intent(in) :: cs, ls
      real(c_double), dimension(*), intent(in) :: scalar
      type(c_ptr), value :: inc_flux, ssa_p
      real(c_double), dimension(*), intent(inout) :: flux_up, flux_dn
      type(c_ptr), value :: stream
      integer(c_int) :: rc
    end function c_lw_fluxes_allsky
    function c_sw_fluxes_allsky(model, ncol, nlay, plev, tlay, ngas, gas_names, vmr, cs, ls, scalar, top_at_1, mu0, toa_scale, &
                                sfc_alb_dir, sfc_alb_dif, nband_p, tau_p, ssa_p, g_p, delta_scale, flux_up, flux_dn, flux_dir, &
                                memspace, stream) bind(C, name="ecckd_sw_fluxes_allsky") result(rc)
      import c_ptr, c_int, c_double, c_char, c_long_long
      type(c_ptr), value :: model
      integer(c_int), value :: ncol, nlay, ngas, top_at_1, nband_p, delta_scale, memspace
      real(c_double), dimension(*), intent(in) :: plev, tlay, mu0, sfc_alb_dir, sfc_alb_dif, tau_p, ssa_p, g_p
      character(kind=c_char), dimension(*), intent(in) :: gas_names
      type(c_ptr), dimension(*), intent(in) :: vmr
      integer(c_long_long), dimension(*), intent(in) :: cs, ls
      real(c_double), dimension(*), intent(in) :: scalar
      type(c_ptr), value :: toa_scale, flux_dir
      real(c_double), dimension(*), intent(inout) :: flux_up, flux_dn
      type(c_ptr), value :: stream
      integer(c_int) :: rc
    end function c_sw_fluxes_allsky
    function c_lw_fluxes_allsky_mcica(model, ncol, nlay, plev, tlay, tsfc, tlev, ngas, gas_names, vmr, cs, ls, scalar, top_at_1, &
                                      nmus, sfc_emis, inc_flux, nband_p, tau_p, ssa_p, cloud_mask, flux_up, flux_dn, memspace, &
                                      stream) bind(C, name="ecckd_lw_fluxes_allsky_mcica") result(rc)
      import c_ptr, c_int, c_double, c_char, c_long_long, c_int64_t
      type(c_ptr), value :: model
      integer(c_int), value :: ncol, nlay, ngas, top_at_1, nmus, nband_p, memspace
      real(c_double), dimension(*), intent(in) :: plev, tlay, tsfc, tlev, sfc_emis, tau_p
      character(kind=c_char), dimension(*), intent(in) :: gas_names
      type(c_ptr), dimension(*), intent(in) :: vmr
      integer(c_long_long), dimension(*), intent(in) :: cs, ls
      real(c_double), dimension(*), intent(in) :: scalar
      type(c_ptr), value :: inc_flux, ssa_p
      integer(c_int64_t), dimension(*), intent(in) :: cloud_mask
      real(c_double), dimension(*), intent(inout) :: flux_up, flux_dn
      type(c_ptr), value :: stream
      integer(c_int) :: rc
    end function c_lw_fluxes_allsky_mcica
    function c_sw_fluxes_allsky_mcica(model, ncol, nlay, plev, tlay, ngas, gas_names, vmr, cs, ls, scalar, top_at_1, mu0, &
                                      toa_scale, sfc_alb_dir, sfc_alb_dif, nband_p, tau_p, ssa_p, g_p, delta_scale, cloud_mask, &
                                      flux_up, flux_dn, flux_dir, memspace, stream) &
        bind(C, name="ecckd_sw_fluxes_allsky_mcica") result(rc)
      import c_ptr, c_int, c_double, c_char, c_long_long, c_int64_t
      type(c_ptr), value :: model
      integer(c_int), value :: ncol, nlay, ngas, top_at_1, nband_p, delta_scale, memspace
      real(c_double), dimension(*), intent(in) :: plev, tlay, mu0, sfc_alb_dir, sfc_alb_dif, tau_p, ssa_p, g_p
      character(kind=c_char), dimension(*), intent(in) :: gas_names
      type(c_ptr), dimension(*), intent(in) :: vmr
      integer(c_long_long), dimension(*), intent(in) :: cs, ls
      real(c_double), dimension(*), intent(in) :: scalar
      type(c_ptr), value :: toa_scale, flux_dir
      integer(c_int64_t), dimension(*), intent(in) :: cloud_mask
      real(c_double), dimension(*), intent(inout) :: flux_up, flux_dn
      type(c_ptr), value :: stream
      integer(c_int) :: rc
    end function c_sw_fluxes_allsky_mcica
    function c_lw_fluxes_clear_allsky(model, ncol, nlay, plev, tlay, tsfc, tlev, ngas, gas_names, vmr, cs, ls, scalar, top_at_1, &
                                      nmus, sfc_emis, inc_flux, nband_p, tau_p, ssa_p, cloud_mask, flux_up, flux_dn, &
                                      flux_up_clear, flux_dn_clear, memspace, stream) &
        bind(C, name="ecckd_lw_fluxes_clear_allsky") result(rc)
      import c_ptr, c_int, c_double, c_char, c_long_long
      type(c_ptr), value :: model
      integer(c_int), value :: ncol, nlay, ngas, top_at_1, nmus, nband_p, memspace
      real(c_double), dimension(*), intent(in) :: plev, tlay, tsfc, tlev, sfc_emis, tau_p
      character(kind=c_char), dimension(*), intent(in) :: gas_names
      type(c_ptr), dimension(*), intent(in) :: vmr
      integer(c_long_long), dimension(*), intent(in) :: cs, ls
      real(c_double), dimension(*), intent(in) :: scalar
      type(c_ptr), value :: inc_flux, ssa_p, cloud_mask
      real(c_double), dimension(*), intent(inout) :: flux_up, flux_dn, flux_up_clear, flux_dn_clear
      type(c_ptr), value :: stream
      integer(c_int) :: rc
    end function c_lw_fluxes_clear_allsky
    function c_sw_fluxes_clear_allsky(model, ncol, nlay, plev, tlay, ngas, gas_names, vmr, cs, ls, scalar, top_at_1, mu0, &
                                      toa_scale, sfc_alb_dir, sfc_alb_dif, nband_p, tau_p, ssa_p, g_p, delta_scale, cloud_mask, &
                                      flux_up, flux_dn, flux_dir, flux_up_clear, flux_dn_clear, flux_dir_clear, memspace, &
                                      stream) bind(C, name="ecckd_sw_fluxes_clear_allsky") result(rc)
      import c_ptr, c_int, c_double, c_char, c_long_long
      type(c_ptr), value :: model
      integer(c_int), value :: ncol, nlay, ngas, top_at_1, nband_p, delta_scale, memspace
      real(c_double), dimension(*), intent(in) :: plev, tlay, mu0, sfc_alb_dir, sfc_alb_dif, tau_p, ssa_p, g_p
      character(kind=c_char), dimension(*), intent(in) :: gas_names
      type(c_ptr), dimension(*), intent(in) :: vmr
      integer(c_long_long), dimension(*), intent(in) :: cs, ls
      real(c_double), dimension(*), intent(in) :: scalar
      type(c_ptr), value :: toa_scale, flux_dir, flux_dir_clear, cloud_mask
      real(c_double), dimension(*), intent(inout) :: flux_up, flux_dn, flux_up_clear, flux_dn_clear
      type(c_ptr), value :: stream
      integer(c_int) :: rc
    end function c_sw_fluxes_clear_allsky
    function c_daylit_columns(device, ncol, mu0, mu0_min, day_index, nday, memspace, stream) &
        bind(C, name="ecckd_daylit_columns") result(rc)
      import c_ptr, c_int, c_double
      integer(c_int), value :: device, ncol, memspace
      real(c_double), dimension(*), intent(in) :: mu0
      real(c_double), value :: mu0_min
      integer(c_int), dimension(*), intent(inout) :: day_index
      integer(c_int), intent(out) :: nday
      type(c_ptr), value :: stream
      integer(c_int) :: rc
    end function c_daylit_columns
    function c_sw_fluxes_daylit(model, ncol, nlay, nday, day_index, plev, tlay, ngas, gas_names, vmr, cs, ls, scalar, top_at_1, &
                                mu0, toa_scale, sfc_alb_dir, sfc_alb_dif, nband_p, tau_p, ssa_p, g_p, delta_scale, cloud_mask, &
                                flux_up, flux_dn, flux_dir, flux_up_clear, flux_dn_clear, flux_dir_clear, memspace, stream) &
        bind(C, name="ecckd_sw_fluxes_daylit") result(rc)
      import c_ptr, c_int, c_double, c_char, c_long_long
      type(c_ptr), value :: model
      integer(c_int), value :: ncol, nlay, nday, ngas, top_at_1, nband_p, delta_scale, memspace
      integer(c_int), dimension(*), intent(in) :: day_index
      real(c_double), dimension(*), intent(in) :: plev, tlay, mu0, sfc_alb_dir, sfc_alb_dif
      character(kind=c_char), dimension(*), intent(in) :: gas_names
      type(c_ptr), dimension(*), intent(in) :: vmr
      integer(c_long_long), dimension(*), intent(in) :: cs, ls
      real(c_double), dimension(*), intent(in) :: scalar
      type(c_ptr), value :: toa_scale, tau_p, ssa_p, g_p, cloud_mask, flux_dir, flux_up_clear, flux_dn_clear, flux_dir_clear
      real(c_double), dimension(*), intent(inout) :: flux_up, flux_dn
      type(c_ptr), value :: stream
      integer(c_int) :: rc
    end function c_sw_fluxes_daylit
    function c_gather_columns(device, ninner, ncol, nouter, elem_bytes, nday, day_index, src, dst, memspace, stream) &
        bind(C, name="ecckd_gather_columns") result(rc)
      import c_ptr, c_int, c_double
      integer(c_int), value :: device, ninner, ncol, nouter, elem_bytes, nday, memspace
      integer(c_int), dimension(*), intent(in) :: day_index
      real(c_double), dimension(*), intent(in) :: src      ! (8-byte elements: the binding serves the fp64 arrays)
      real(c_double), dimension(*), intent(inout) :: dst
      type(c_ptr), value :: stream
      integer(c_int) :: rc
    end function c_gather_columns
    function c_scatter_columns(device, ninner, ncol, nouter, elem_bytes, nday, day_index, src, dst, fill, memspace, stream) &
        bind(C, name="ecckd_scatter_columns") result(rc)
      import c_ptr, c_int, c_double
      integer(c_int), value :: device, ninner, ncol, nouter, elem_bytes, nday, memspace
      integer(c_int), dimension(*), intent(in) :: day_index
      real(c_double), dimension(*), intent(in) :: src
      real(c_double), dimension(*), intent(inout) :: dst
      real(c_double), value :: fill
      type(c_ptr), value :: stream
      integer(c_int) :: rc
    end function c_scatter_columns
    function c_rte_sw_host(device, ncol, nlay, ngpt, top_at_1, tau, ssa, g, mu0, toa, nband, band2gpt, alb_dir, alb_dif, &
                           flux_up, flux_dn, flux_dir, memspace, stream) bind(C, name="ecckd_rte_sw") result(rc)
      import c_ptr, c_int, c_double
      integer(c_int), value :: device, ncol, nlay, ngpt, top_at_1, nband, memspace
      type(c_ptr), value :: tau, ssa, g
      real(c_double), dimension(*), intent(in) :: mu0, toa, alb_dir, alb_dif
      integer(c_int), dimension(*), intent(in) :: band2gpt
      real(c_double), dimension(*), intent(inout) :: flux_up, flux_dn, flux_dir
      type(c_ptr), value :: stream
      integer(c_int) :: rc
    end function c_rte_sw_host
    function c_cloud_mask_sample(device, ncol, nlay, ngpt, overlap, cloud_frac, overlap_param, seed, col0, mask, memspace, &
                                 stream) bind(C, name="ecckd_cloud_mask_sample") result(rc)
      import c_ptr, c_int, c_double, c_int64_t
      integer(c_int), value :: device, ncol, nlay, ngpt, overlap, memspace
      real(c_double), dimension(*), intent(in) :: cloud_frac
      type(c_ptr), value :: overlap_param
      integer(c_int64_t), value :: seed, col0           ! (seed: the bits of the C unsigned 64-bit word)
      integer(c_int64_t), dimension(*), intent(inout) :: mask
      type(c_ptr), value :: stream
      integer(c_int) :: rc
    end function c_cloud_mask_sample
    function c_cloud_scaling_create(device, nfsd, fsd0, dfsd, nq, values, table) bind(C, name="ecckd_cloud_scaling_create") &
        result(rc)
      import c_ptr, c_int, c_double
      integer(c_int), value :: device, nfsd, nq
      real(c_double), value :: fsd0, dfsd
      real(c_double), dimension(*), intent(in) :: values
      type(c_ptr), intent(out) :: table
      integer(c_int) :: rc
    end function c_cloud_scaling_create
    subroutine c_cloud_scaling_destroy(table) bind(C, name="ecckd_cloud_scaling_destroy")
      import c_ptr
      type(c_ptr), value :: table
    end subroutine c_cloud_scaling_destroy
    function c_cloud_scaling_lognormal(nfsd, fsd0, dfsd, nq, values) bind(C, name="ecckd_cloud_scaling_lognormal") result(rc)
      import c_int, c_double
      integer(c_int), value :: nfsd, nq
      real(c_double), value :: fsd0, dfsd
      real(c_double), dimension(*), intent(inout) :: values
      integer(c_int) :: rc
    end function c_cloud_scaling_lognormal
    function c_cloud_scaling_sample(device, ncol, nlay, ngpt, overlap, cloud_frac, overlap_param, fsd, fsd_const, table, seed, &
                                    col0, scaling, mask, memspace, stream) bind(C, name="ecckd_cloud_scaling_sample") result(rc)
      import c_ptr, c_int, c_double, c_int64_t, c_float
      integer(c_int), value :: device, ncol, nlay, ngpt, overlap, memspace
      real(c_double), dimension(*), intent(in) :: cloud_frac
      type(c_ptr), value :: overlap_param, fsd, table, mask
      real(c_double), value :: fsd_const
      integer(c_int64_t), value :: seed, col0           ! (seed: the bits of the C unsigned 64-bit word)
      real(c_float), dimension(*), intent(inout) :: scaling
      type(c_ptr), value :: stream
      integer(c_int) :: rc
    end function c_cloud_scaling_sample
    function c_lw_flux_scaled(model, ncol, nlay, plev, tlay, tsfc, tlev, ngas, gas_names, vmr, cs, ls, scalar, top_at_1, nmus, &
                              sfc_emis, inc_flux, nband_p, tau_p, ssa_p, cloud_scaling, flux_up, flux_dn, memspace, stream) &
        bind(C, name="ecckd_lw_flux_scaled") result(rc)
      import c_ptr, c_int, c_double, c_char, c_long_long, c_float
      type(c_ptr), value :: model
      integer(c_int), value :: ncol, nlay, ngas, top_at_1, nmus, nband_p, memspace
      real(c_double), dimension(*), intent(in) :: plev, tlay, tsfc, tlev, sfc_emis, tau_p
      character(kind=c_char), dimension(*), intent(in) :: gas_names
      type(c_ptr), dimension(*), intent(in) :: vmr
      integer(c_long_long), dimension(*), intent(in) :: cs, ls
      real(c_double), dimension(*), intent(in) :: scalar
      type(c_ptr), value :: inc_flux, ssa_p
      real(c_float), dimension(*), intent(in) :: cloud_scaling
      real(c_double), dimension(*), intent(inout) :: flux_up, flux_dn
      type(c_ptr), value :: stream
      integer(c_int) :: rc
    end function c_lw_flux_scaled
    function c_sw_flux_scaled(model, ncol, nlay, plev, tlay, ngas, gas_names, vmr, cs, ls, scalar, top_at_1, mu0, toa_scale, &
                              sfc_alb_dir, sfc_alb_dif, nband_p, tau_p, ssa_p, g_p, delta_scale, cloud_scaling, flux_up, flux_dn, &
                              flux_dir, memspace, stream) bind(C, name="ecckd_sw_flux_scaled") result(rc)
      import c_ptr, c_int, c_double, c_char, c_long_long, c_float
      type(c_ptr), value :: model
      integer(c_int), value :: ncol, nlay, ngas, top_at_1, nband_p, delta_scale, memspace
      real(c_double), dimension(*), intent(in) :: plev, tlay, mu0, sfc_alb_dir, sfc_alb_dif, tau_p, ssa_p, g_p
      character(kind=c_char), dimension(*), intent(in) :: gas_names
      type(c_ptr), dimension(*), intent(in) :: vmr
      integer(c_long_long), dimension(*), intent(in) :: cs, ls
      real(c_double), dimension(*), intent(in) :: scalar
      type(c_ptr), value :: toa_scale, flux_dir
      real(c_float), dimension(*), intent(in) :: cloud_scaling
      real(c_double), dimension(*), intent(inout) :: flux_up, flux_dn
      type(c_ptr), value :: stream
      integer(c_int) :: rc
    end function c_sw_flux_scaled
    function c_model_device(model) bind(C, name="ecckd_model_get_device") result(dev)
      import c_ptr, c_int
      type(c_ptr), value :: model
      integer(c_int) :: dev
    end function c_model_device
    function c_lw_flux_bands(model, ncol, nlay, plev, tlay, tsfc, tlev, ngas, gas_names, vmr, cs, ls, scalar, top_at_1, nmus, &
                             sfc_emis, inc_flux, nband_p, tau_p, ssa_p, cloud_mask, bnd_flux_up, bnd_flux_dn, flux_up, flux_dn, &
                             memspace, stream) bind(C, name="ecckd_lw_flux_bands") result(rc)
      import c_ptr, c_int, c_double, c_char, c_long_long
      type(c_ptr), value :: model
      integer(c_int), value :: ncol, nlay, ngas, top_at_1, nmus, nband_p, memspace
      real(c_double), dimension(*), intent(in) :: plev, tlay, tsfc, tlev, sfc_emis
      character(kind=c_char), dimension(*), intent(in) :: gas_names
      type(c_ptr), dimension(*), intent(in) :: vmr
      integer(c_long_long), dimension(*), intent(in) :: cs, ls
      real(c_double), dimension(*), intent(in) :: scalar
      type(c_ptr), value :: inc_flux, tau_p, ssa_p, cloud_mask, flux_up, flux_dn
      real(c_double), dimension(*), intent(inout) :: bnd_flux_up, bnd_flux_dn
      type(c_ptr), value :: stream
      integer(c_int) :: rc
    end function c_lw_flux_bands
    function c_sw_flux_bands(model, ncol, nlay, plev, tlay, ngas, gas_names, vmr, cs, ls, scalar, top_at_1, mu0, toa_scale, &
                             sfc_alb_dir, sfc_alb_dif, nband_p, tau_p, ssa_p, g_p, delta_scale, cloud_mask, bnd_flux_up, &
                             bnd_flux_dn, bnd_flux_dir, flux_up, flux_dn, flux_dir, memspace, stream) &
        bind(C, name="ecckd_sw_flux_bands") result(rc)
      import c_ptr, c_int, c_double, c_char, c_long_long
      type(c_ptr), value :: model
      integer(c_int), value :: ncol, nlay, ngas, top_at_1, nband_p, delta_scale, memspace
      real(c_double), dimension(*), intent(in) :: plev, tlay, mu0, sfc_alb_dir, sfc_alb_dif
      character(kind=c_char), dimension(*), intent(in) :: gas_names
      type(c_ptr), dimension(*), intent(in) :: vmr
      integer(c_long_long), dimension(*), intent(in) :: cs, ls
      real(c_double), dimension(*), intent(in) :: scalar
      type(c_ptr), value :: toa_scale, tau_p, ssa_p, g_p, cloud_mask, bnd_flux_dir, flux_up, flux_dn, flux_dir
      real(c_double), dimension(*), intent(inout) :: bnd_flux_up, bnd_flux_dn
      type(c_ptr), value :: stream
      integer(c_int) :: rc
    end function c_sw_flux_bands
  end interface

  integer, parameter, public :: ECCKD_OVERLAP_MAX_RAN = 0, ECCKD_OVERLAP_EXP_RAN = 1

  !> Extension: the table of in-cloud water variability (ecckd_cloud_scaling_create; include/ecckd_hip.h, "In-cloud water
  !! variability"): values (nq, nfsd), row k (second index) the scalings of the nq equal-probability bins at the fractional
  !! standard deviation fsd0 + (k-1)*dfsd.  It lives on the device of the model it is loaded for.
  type, public :: ty_cloud_scaling
    type(c_ptr) :: handle = c_null_ptr
  contains
    procedure, public :: load_lognormal => cloud_scaling_load_lognormal
    procedure, public :: load_table => cloud_scaling_load_table
    procedure, public :: finalize => cloud_scaling_finalize
  end type ty_cloud_scaling

  public :: c_error_message, c_loc_3d, c_loc_2d

contains

  !> Message of the last failing C call, as the reference's character(len=128) error strings.
  function c_error_message() result(msg)
    character(len=128) :: msg
    character(kind=c_char), dimension(:), pointer :: p
    type(c_ptr) :: cp
    integer :: i
    msg = ""
    cp = c_last_error()
    if (.not. c_associated(cp)) return
    call c_f_pointer(cp, p, [128])
    do i = 1, 128
      if (p(i) == c_null_char) exit
      msg(i:i) = p(i)
    end do
    if (len_trim(msg) == 0) msg = "ecckd: unknown error"
  end function c_error_message

  !> load_and_init(ecckd, filename, available_gases) of mo_load_coefficients.F90:19-146 as a
  !! type-bound procedure; available_gases is accepted and ignored exactly as there (:19,:23).
  function load(this, filename, available_gases, device) result(error_msg)
    class(ty_gas_optics_ecckd), intent(inout) :: this
    character(len=*), intent(in) :: filename
    class(ty_gas_concs), intent(in), optional :: available_gases
    integer, intent(in), optional :: device
    character(len=128) :: error_msg
    integer(c_int) :: dev, rc, nband
    integer(c_int), dimension(:,:), allocatable :: b2g
    real(c_double), dimension(:,:), allocatable :: lims
    error_msg = ""
    dev = 0
    if (present(device)) dev = int(device, c_int)
    call this%finalize()
    rc = c_model_load(trim(filename) // c_null_char, dev, this%handle)
    if (rc /= 0) then
      error_msg = c_error_message()
      this%handle = c_null_ptr
      return
    end if
    ! ecckd%init(band_lims_wvn, band2gpt) of mo_load_coefficients.F90:74
    nband = c_get_nband(this%handle)
    allocate(b2g(2, nband), lims(2, nband))
    rc = c_get_band2gpt(this%handle, b2g)
    rc = c_get_band_lims(this%handle, lims)
    error_msg = this%init(lims, int(b2g))
  end function load

  subroutine finalize(this)
    class(ty_gas_optics_ecckd), intent(inout) :: this
    if (c_associated(this%handle)) call c_model_destroy(this%handle)
    this%handle = c_null_ptr
  end subroutine finalize

  pure function get_ngas(this)                                   ! src/gas_optics_ecckd.f90:477
    class(ty_gas_optics_ecckd), intent(in) :: this
    integer :: get_ngas
    get_ngas = int(c_get_ngas(this%handle))
  end function get_ngas

  pure function source_is_internal(this)                         ! :487
    class(ty_gas_optics_ecckd), intent(in) :: this
    logical :: source_is_internal
    source_is_internal = c_is_internal(this%handle) /= 0
  end function source_is_internal

  pure function source_is_external(this)                         ! :497
    class(ty_gas_optics_ecckd), intent(in) :: this
    logical :: source_is_external
    source_is_external = c_is_external(this%handle) /= 0
  end function source_is_external

  pure function get_gases(this)                                  ! :507
    class(ty_gas_optics_ecckd), intent(in) :: this
    character(len=32), dimension(this%get_ngas()) :: get_gases
    character(kind=c_char), dimension(name_len) :: buf
    integer :: i, k
    integer(c_int) :: rc
    do i = 1, size(get_gases)
      buf = c_null_char
      rc = c_get_gas_name(this%handle, int(i - 1, c_int), buf)
      get_gases(i) = ""
      do k = 1, name_len
        if (buf(k) == c_null_char) exit
        get_gases(i)(k:k) = buf(k)
      end do
    end do
  end function get_gases

  pure function get_press_min(this)                              ! :517
    class(ty_gas_optics_ecckd), intent(in) :: this
    real(wp) :: get_press_min
    get_press_min = c_press_min(this%handle)
  end function get_press_min

  pure function get_press_max(this)                              ! :527
    class(ty_gas_optics_ecckd), intent(in) :: this
    real(wp) :: get_press_max
    get_press_max = c_press_max(this%handle)
  end function get_press_max

  pure function get_temp_min(this)                               ! :537
    class(ty_gas_optics_ecckd), intent(in) :: this
    real(wp) :: get_temp_min
    get_temp_min = c_temp_min(this%handle)
  end function get_temp_min

  pure function get_temp_max(this)                               ! :547
    class(ty_gas_optics_ecckd), intent(in) :: this
    real(wp) :: get_temp_max
    get_temp_max = c_temp_max(this%handle)
  end function get_temp_max

  !> gas_desc -> the flat description the C ABI takes, without copying a concentration field: the C ABI takes a
  !! pointer and two strides per gas, which is exactly what ty_gas_concs stores -- concs(i)%conc is (1,1) for a
  !! scalar, (1,nlay) for a profile and (ncol,nlay) for a full field (RTE-RRTMGP's mo_gas_concentrations, same
  !! public components as the minimal type of mo_rte_min.F90), so the broadcast of get_vmr (:351) happens on the
  !! GPU through the strides.  Like the reference (:348-364) a concentration is only looked up for gases the
  !! k-distribution holds a table for: the others cross the boundary as a name with a null pointer (nothing is
  !! staged for them and an unset one is not an error); the get_vmr error texts are kept (:351-354).
  function marshal_gases(this, gas_desc, ncol, nlay, names, ptr, cs, ls, scalar) result(error_msg)
    class(ty_gas_optics_ecckd), intent(in) :: this
    type(ty_gas_concs), intent(in) :: gas_desc
    integer, intent(in) :: ncol, nlay
    character(kind=c_char), dimension(:), allocatable, intent(out) :: names
    type(c_ptr), dimension(:), allocatable, intent(out) :: ptr
    integer(c_long_long), dimension(:), allocatable, intent(out) :: cs, ls
    real(c_double), dimension(:), allocatable, intent(out) :: scalar
    character(len=128) :: error_msg
    character(len=32), dimension(:), allocatable :: gas_names, model_gases
    integer :: n, j, k, nm
    logical :: known
    error_msg = ""
    n = gas_desc%get_num_gases()
    nm = this%get_ngas()
    allocate(gas_names(n), model_gases(nm))
    gas_names = gas_desc%get_gas_names()
    model_gases = this%get_gases()
    allocate(names(max(1, n * name_len)), ptr(max(1, n)), cs(max(1, n)), ls(max(1, n)), scalar(max(1, n)))
    names = " "
    ptr = c_null_ptr
    cs = 0_c_long_long
    ls = 0_c_long_long
    scalar = 0._c_double
    do j = 1, n
      do k = 1, min(name_len, len_trim(gas_names(j)))
        names((j - 1) * name_len + k) = gas_names(j)(k:k)
      end do
      known = .false.
      do k = 1, nm
        if (trim(model_gases(k)) == trim(gas_names(j))) known = .true.
      end do
      if (.not. known) cycle                                  ! :358-364 silently skipped
      if (.not. allocated(gas_desc%concs(j)%conc)) then      ! (get_gas_names() returns gas_name(:): index j)
        error_msg = "ty_gas_concs%get_vmr; gas " // trim(gas_names(j)) // " not found"
        return
      end if
      associate (c => gas_desc%concs(j)%conc)
        if (size(c, 1) > 1 .and. size(c, 1) /= ncol) then
          error_msg = "ty_gas_concs%get_vmr; gas " // trim(gas_names(j)) // " array is inconsistent with ncol"
          return
        end if
        if (size(c, 2) > 1 .and. size(c, 2) /= nlay) then
          error_msg = "ty_gas_concs%get_vmr; gas " // trim(gas_names(j)) // " array is inconsistent with nlay"
          return
        end if
        if (size(c) == 1) then
          scalar(j) = c(1, 1)
        else
          ptr(j) = c_loc_2d(c)
          if (size(c, 1) > 1) cs(j) = 1_c_long_long
          if (size(c, 2) > 1) ls(j) = int(size(c, 1), c_long_long)
        end if
      end associate
    end do
  end function marshal_gases

  !> gas_optics_int, src/gas_optics_ecckd.f90:381-426 (same argument list).  Host containers: ECCKD_HOST
  !! (every array is staged through the GPU).  Device twins (mo_ecckd_device): ECCKD_MIXED -- tau and the
  !! sources stay in HBM for rte_lw.
  function gas_optics_int(this, play, plev, tlay, tsfc, gas_desc, optical_props, sources, col_dry, tlev) &
      result(error_msg)
    class(ty_gas_optics_ecckd), intent(in) :: this
    real(wp), dimension(:,:), intent(in) :: play, plev, tlay
    real(wp), dimension(:), intent(in) :: tsfc
    type(ty_gas_concs), intent(in) :: gas_desc
    class(ty_optical_props_arry), intent(inout) :: optical_props
    class(ty_source_func_lw), intent(inout) :: sources
    character(len=128) :: error_msg
    real(wp), dimension(:,:), intent(in), target, optional :: col_dry, tlev
    character(kind=c_char), dimension(:), allocatable :: names
    real(wp), dimension(:,:), allocatable, target :: tlev_c
    type(c_ptr), dimension(:), allocatable :: ptr
    integer(c_long_long), dimension(:), allocatable :: cs, ls
    real(c_double), dimension(:), allocatable :: scalar
    type(c_ptr) :: tlev_p, p_tau, p_lay, p_inc, p_dec, p_sfc
    integer :: ncol, nlay, n
    integer(c_int) :: rc, memspace
    ncol = size(tlay, 1)
    nlay = size(tlay, 2)
    error_msg = marshal_gases(this, gas_desc, ncol, nlay, names, ptr, cs, ls, scalar)
    if (trim(error_msg) /= "") return
    n = gas_desc%get_num_gases()
    tlev_p = c_null_ptr
    if (present(tlev)) then
      if (is_contiguous(tlev)) then
        tlev_p = c_loc_2d(tlev)
      else
        allocate(tlev_c(ncol, nlay + 1))
        tlev_c = tlev
        tlev_p = c_loc(tlev_c(1, 1))
      end if
    end if
    memspace = ECCKD_HOST
    select type (optical_props)
      class is (ty_optical_props_1scl_dev)
        select type (sources)
          class is (ty_source_func_lw_dev)
            if (optical_props%ncol /= ncol .or. optical_props%nlay /= nlay .or. sources%ncol /= ncol .or. &
                sources%nlay /= nlay) then
              error_msg = "gas_optics: device-resident optical_props / sources are inconsistently sized"
              return
            end if
            memspace = ECCKD_MIXED
            p_tau = optical_props%d_tau
            p_lay = sources%d_lay_source
            p_inc = sources%d_lev_source_inc
            p_dec = sources%d_lev_source_dec
            p_sfc = sources%d_sfc_source
          class default
            error_msg = "gas_optics: device-resident optical_props needs device-resident sources (ty_source_func_lw_dev)"
            return
        end select
      class default
        select type (sources)
          class is (ty_source_func_lw_dev)
            error_msg = "gas_optics: device-resident sources need device-resident optical_props (ty_optical_props_1scl_dev)"
            return
        end select
        p_tau = c_loc_3d(optical_props%tau)
        p_lay = c_loc_3d(sources%lay_source)
        p_inc = c_loc_3d(sources%lev_source_inc)
        p_dec = c_loc_3d(sources%lev_source_dec)
        p_sfc = c_loc_2d(sources%sfc_source)
    end select
    rc = c_gas_optics_lw(this%handle, int(ncol, c_int), int(nlay, c_int), plev, tlay, tsfc, tlev_p, &
                         int(n, c_int), names, ptr, cs, ls, scalar, p_tau, p_lay, p_inc, p_dec, p_sfc, memspace, &
                         c_null_ptr)
    if (rc /= 0) error_msg = c_error_message()
  end function gas_optics_int

  !> gas_optics_ext, src/gas_optics_ecckd.f90:431-473 (same argument list).
  function gas_optics_ext(this, play, plev, tlay, gas_desc, optical_props, toa_src, col_dry) result(error_msg)
    class(ty_gas_optics_ecckd), intent(in) :: this
    real(wp), dimension(:,:), intent(in) :: play, plev, tlay
    type(ty_gas_concs), intent(in) :: gas_desc
    class(ty_optical_props_arry), intent(inout) :: optical_props
    real(wp), dimension(:,:), intent(out) :: toa_src
    real(wp), dimension(:,:), intent(in), target, optional :: col_dry
    character(len=128) :: error_msg
    character(kind=c_char), dimension(:), allocatable :: names
    type(c_ptr), dimension(:), allocatable :: ptr
    integer(c_long_long), dimension(:), allocatable :: cs, ls
    real(c_double), dimension(:), allocatable :: scalar
    type(c_ptr) :: tau_p, ssa_p, g_p
    integer :: ncol, nlay, n
    integer(c_int) :: rc, memspace
    ncol = size(tlay, 1)
    nlay = size(tlay, 2)
    error_msg = marshal_gases(this, gas_desc, ncol, nlay, names, ptr, cs, ls, scalar)
    if (trim(error_msg) /= "") return
    n = gas_desc%get_num_gases()
    ssa_p = c_null_ptr
    g_p = c_null_ptr
    memspace = ECCKD_HOST
    select type (optical_props)                  ! :457-464
      class is (ty_optical_props_2str_dev)
        if (optical_props%ncol /= ncol .or. optical_props%nlay /= nlay) then
          error_msg = "gas_optics: device-resident optical_props is inconsistently sized"
          return
        end if
        memspace = ECCKD_MIXED
        tau_p = optical_props%d_tau
        ssa_p = optical_props%d_ssa
        g_p = optical_props%d_g
      class is (ty_optical_props_1scl_dev)
        memspace = ECCKD_MIXED
        tau_p = optical_props%d_tau
      class is (ty_optical_props_2str)
        tau_p = c_loc_3d(optical_props%tau)
        ssa_p = c_loc_3d(optical_props%ssa)
        g_p = c_loc_3d(optical_props%g)
      class default
        tau_p = c_loc_3d(optical_props%tau)
    end select
    rc = c_gas_optics_sw(this%handle, int(ncol, c_int), int(nlay, c_int), plev, tlay, int(n, c_int), names, &
                         ptr, cs, ls, scalar, tau_p, ssa_p, g_p, toa_src, memspace, c_null_ptr)
    if (rc /= 0) error_msg = c_error_message()
  end function gas_optics_ext

  !> Extension (no counterpart in the reference): broadband longwave fluxes in one call -- what the reference's block
  !! loop computes with ecckd%gas_optics(...) followed by rte_lw(...) (ecckd_rfmip_lw.F90:120-135) -- through the fused
  !! path of the library (ecckd_lw_fluxes: tau stays on the GPU, the Planck sources are recomputed inside the solver).
  !! Host arrays in, host fluxes out (60 layers take the fused kernels, other counts the general route).  flux_up / flux_dn are (ncol, nlay+1), sfc_emis (nband, ncol).
  !! flux_up_Jac (ncol, nlay+1): d(flux_up)/d(surface temperature), W m-2 K-1, from the same call (ecckd_lw_fluxes_jac);
  !! the fluxes are the same bits with and without it.
  function lw_fluxes(this, plev, tlay, tsfc, tlev, gas_desc, top_at_1, sfc_emis, flux_up, flux_dn, n_gauss_angles, flux_up_Jac) &
      result(error_msg)
    class(ty_gas_optics_ecckd), intent(in) :: this
    real(wp), dimension(:,:), intent(in) :: plev, tlay, tlev
    real(wp), dimension(:), intent(in) :: tsfc
    type(ty_gas_concs), intent(in) :: gas_desc
    logical, intent(in) :: top_at_1
    real(wp), dimension(:,:), intent(in) :: sfc_emis
    real(wp), dimension(:,:), intent(inout) :: flux_up, flux_dn
    integer, intent(in), optional :: n_gauss_angles
    real(wp), dimension(:,:), intent(inout), optional :: flux_up_Jac
    character(len=128) :: error_msg
    character(kind=c_char), dimension(:), allocatable :: names
    type(c_ptr), dimension(:), allocatable :: ptr
    integer(c_long_long), dimension(:), allocatable :: cs, ls
    real(c_double), dimension(:), allocatable :: scalar
    real(wp), dimension(:,:), allocatable :: up, dn, jac
    integer :: ncol, nlay, n, nmus
    integer(c_int) :: rc
    ncol = size(tlay, 1)
    nlay = size(tlay, 2)
    nmus = 1
    if (present(n_gauss_angles)) nmus = n_gauss_angles
    error_msg = marshal_gases(this, gas_desc, ncol, nlay, names, ptr, cs, ls, scalar)
    if (trim(error_msg) /= "") return
    if (size(sfc_emis, 1) /= this%get_nband() .or. size(sfc_emis, 2) /= ncol) then
      error_msg = "lw_fluxes: sfc_emis inconsistently sized"
      return
    end if
    n = gas_desc%get_num_gases()
    allocate(up(ncol, nlay + 1), dn(ncol, nlay + 1))
    if (present(flux_up_Jac)) then
      if (size(flux_up_Jac, 1) /= ncol .or. size(flux_up_Jac, 2) /= nlay + 1) then
        error_msg = "lw_fluxes: flux_up_Jac inconsistently sized"
        return
      end if
      allocate(jac(ncol, nlay + 1))
      rc = c_lw_fluxes_jac(this%handle, int(ncol, c_int), int(nlay, c_int), plev, tlay, tsfc, tlev, int(n, c_int), names, ptr, &
                           cs, ls, scalar, merge(1_c_int, 0_c_int, top_at_1), int(nmus, c_int), sfc_emis, c_null_ptr, 0_c_int, &
                           c_null_ptr, c_null_ptr, c_null_ptr, up, dn, c_null_ptr, c_null_ptr, jac, ECCKD_HOST, c_null_ptr)
      if (rc == 0) flux_up_Jac = jac
    else
    rc = c_lw_fluxes(this%handle, int(ncol, c_int), int(nlay, c_int), plev, tlay, tsfc, tlev, int(n, c_int), names, ptr, cs, &
                     ls, scalar, merge(1_c_int, 0_c_int, top_at_1), int(nmus, c_int), sfc_emis, c_null_ptr, up, dn, &
                     ECCKD_HOST, c_null_ptr)
    end if
    if (rc /= 0) then
      error_msg = c_error_message()
      return
    end if
    flux_up = up
    flux_dn = dn
  end function lw_fluxes

  !> Extension: sources%sfc_source_Jac(ncol, ngpt) = B(tsfc + 1) - B(tsfc) (ecckd_planck_sfc_source_jac), the surface term
  !! of rte_lw's flux_up_Jac: RRTMGP's convention, delta_Tsurf = 1 K.  Host arrays; sources must be allocated (alloc).
  function planck_sfc_source_jac(this, tsfc, sources) result(error_msg)
    class(ty_gas_optics_ecckd), intent(in) :: this
    real(wp), dimension(:), intent(in) :: tsfc
    class(ty_source_func_lw), intent(inout) :: sources
    character(len=128) :: error_msg
    error_msg = ""
    if (.not. allocated(sources%sfc_source_Jac)) then
      error_msg = "planck_sfc_source_jac: sources%sfc_source_Jac is not allocated (sources%alloc)"
      return
    end if
    if (size(sources%sfc_source_Jac, 1) /= size(tsfc) .or. size(sources%sfc_source_Jac, 2) /= this%get_ngpt()) then
      error_msg = "planck_sfc_source_jac: sources%sfc_source_Jac inconsistently sized"
      return
    end if
    if (c_planck_sfc_source_jac(this%handle, int(size(tsfc), c_int), tsfc, sources%sfc_source_Jac, ECCKD_HOST, c_null_ptr) /= 0) &
      error_msg = c_error_message()
  end function planck_sfc_source_jac

  !> Extension (no counterpart in the reference): broadband shortwave fluxes in one call -- what the reference's block
  !! loop computes with ecckd%gas_optics(...), the rescaling of toa_flux and rte_sw(...) (ecckd_rfmip_sw.F90:118-154) --
  !! through the fused path of the library (ecckd_sw_fluxes: only the total optical depth goes through GPU memory; the
  !! solver derives ssa, g = 0 and the incoming beam as gas_optics_ext does, src/gas_optics_ecckd.f90:455-472).  Host
  !! arrays in, host fluxes out; any layer count (the solver rte_sw takes for the shape: layer-systolic up to 60 layers,
  !! two-pass beyond).  flux_* are (ncol, nlay+1), the albedos (nband, ncol); toa_scale(ncol)
  !! multiplies the incoming beam of a column (the drivers' total-solar-irradiance rescaling); flux_dir is optional.
  function sw_fluxes(this, plev, tlay, gas_desc, top_at_1, mu0, sfc_alb_dir, sfc_alb_dif, flux_up, flux_dn, flux_dir, toa_scale) &
      result(error_msg)
    class(ty_gas_optics_ecckd), intent(in) :: this
    real(wp), dimension(:,:), intent(in) :: plev, tlay
    type(ty_gas_concs), intent(in) :: gas_desc
    logical, intent(in) :: top_at_1
    real(wp), dimension(:), intent(in) :: mu0
    real(wp), dimension(:,:), intent(in) :: sfc_alb_dir, sfc_alb_dif
    real(wp), dimension(:,:), intent(inout) :: flux_up, flux_dn
    real(wp), dimension(:,:), intent(inout), optional :: flux_dir
    real(wp), dimension(:), intent(in), optional, target :: toa_scale
    character(len=128) :: error_msg
    character(kind=c_char), dimension(:), allocatable :: names
    type(c_ptr), dimension(:), allocatable :: ptr
    integer(c_long_long), dimension(:), allocatable :: cs, ls
    real(c_double), dimension(:), allocatable :: scalar
    real(wp), dimension(:,:), allocatable, target :: up, dn, dir
    real(wp), dimension(:), allocatable, target :: scale
    type(c_ptr) :: scale_p, dir_p
    integer :: ncol, nlay, n
    integer(c_int) :: rc
    ncol = size(tlay, 1)
    nlay = size(tlay, 2)
    error_msg = marshal_gases(this, gas_desc, ncol, nlay, names, ptr, cs, ls, scalar)
    if (trim(error_msg) /= "") return
    if (size(sfc_alb_dir, 1) /= this%get_nband() .or. size(sfc_alb_dir, 2) /= ncol .or. &
        size(sfc_alb_dif, 1) /= this%get_nband() .or. size(sfc_alb_dif, 2) /= ncol) then
      error_msg = "sw_fluxes: surface albedos inconsistently sized"
      return
    end if
    n = gas_desc%get_num_gases()
    allocate(up(ncol, nlay + 1), dn(ncol, nlay + 1))
    scale_p = c_null_ptr
    dir_p = c_null_ptr
    if (present(toa_scale)) then
      allocate(scale(ncol))
      scale = toa_scale
      scale_p = c_loc(scale(1))
    end if
    if (present(flux_dir)) then
      allocate(dir(ncol, nlay + 1))
      dir_p = c_loc(dir(1, 1))
    end if
    rc = c_sw_fluxes(this%handle, int(ncol, c_int), int(nlay, c_int), plev, tlay, int(n, c_int), names, ptr, cs, ls, scalar, &
                     merge(1_c_int, 0_c_int, top_at_1), mu0, scale_p, sfc_alb_dir, sfc_alb_dif, up, dn, dir_p, ECCKD_HOST, &
                     c_null_ptr)
    if (rc /= 0) then
      error_msg = c_error_message()
      return
    end if
    flux_up = up
    flux_dn = dn
    if (present(flux_dir)) flux_dir = dir
  end function sw_fluxes

  !> Extension: sw_fluxes on the daylit columns only.  The arguments are those of sw_fluxes, every array with the full ncol,
  !! and mu0 is the true cosine of the solar zenith angle: the columns with mu0 > mu0_min (default 0; a NaN is night) are
  !! selected (ecckd_daylit_columns), compacted, computed and scattered back, and every other column of flux_up / flux_dn /
  !! flux_dir is zero at every level.  The caller handles no column list and sets no placeholder mu0 in the night columns.
  !!   toa_scale(ncol), or neither: the fused call ecckd_sw_fluxes_daylit -- what sw_fluxes computes for the daylit columns,
  !!     bit for bit, with the beam solar(g)*toa_scale(i).
  !!   tsi(ncol): the route of a host on the unfused calls, which is what the reference's block loop is: the inputs are
  !!     compacted with ecckd_gather_columns, gas_optics and rte_sw run on the daylit columns with the beam renormalised
  !!     between them exactly as the drivers do it, toa(i,:)*tsi(i)/sum(toa(i,:)) (ecckd_rfmip_sw.F90:126-133), and the fluxes
  !!     go back through ecckd_scatter_columns -- bit for bit what that block loop gives for the daylit columns.  (The beam
  !!     of that expression is an array per g-point; no toa_scale reproduces its bits.)
  function sw_fluxes_daylit(this, plev, tlay, gas_desc, top_at_1, mu0, sfc_alb_dir, sfc_alb_dif, flux_up, flux_dn, flux_dir, &
                            toa_scale, mu0_min, tsi) result(error_msg)
    class(ty_gas_optics_ecckd), intent(in) :: this
    real(wp), dimension(:,:), intent(in) :: plev, tlay
    type(ty_gas_concs), intent(in) :: gas_desc
    logical, intent(in) :: top_at_1
    real(wp), dimension(:), intent(in) :: mu0
    real(wp), dimension(:,:), intent(in) :: sfc_alb_dir, sfc_alb_dif
    real(wp), dimension(:,:), intent(inout) :: flux_up, flux_dn
    real(wp), dimension(:,:), intent(inout), optional :: flux_dir
    real(wp), dimension(:), intent(in), optional :: toa_scale, tsi
    real(wp), intent(in), optional :: mu0_min
    character(len=128) :: error_msg
    character(kind=c_char), dimension(:), allocatable :: names
    type(c_ptr), dimension(:), allocatable :: ptr
    integer(c_long_long), dimension(:), allocatable :: cs, ls
    real(c_double), dimension(:), allocatable :: scalar
    real(wp), dimension(:,:), allocatable, target :: up, dn, dir
    real(wp), dimension(:), allocatable, target :: scale
    integer(c_int), dimension(:), allocatable :: day_index
    type(c_ptr) :: scale_p, dir_p
    integer :: ncol, nlay, n
    integer(c_int) :: rc, nd
    real(c_double) :: limit
    ncol = size(tlay, 1)
    nlay = size(tlay, 2)
    error_msg = marshal_gases(this, gas_desc, ncol, nlay, names, ptr, cs, ls, scalar)
    if (trim(error_msg) /= "") return
    if (size(sfc_alb_dir, 1) /= this%get_nband() .or. size(sfc_alb_dir, 2) /= ncol .or. &
        size(sfc_alb_dif, 1) /= this%get_nband() .or. size(sfc_alb_dif, 2) /= ncol) then
      error_msg = "sw_fluxes_daylit: surface albedos inconsistently sized"
      return
    end if
    if (size(mu0) /= ncol) then
      error_msg = "sw_fluxes_daylit: mu0 inconsistently sized"
      return
    end if
    if (present(tsi)) then
      if (present(toa_scale)) then
        error_msg = "sw_fluxes_daylit: toa_scale and tsi exclude each other"
        return
      end if
      if (size(tsi) /= ncol) then
        error_msg = "sw_fluxes_daylit: tsi inconsistently sized"
        return
      end if
    end if
    limit = 0._c_double
    if (present(mu0_min)) limit = real(mu0_min, c_double)
    allocate(day_index(max(ncol, 1)))
    nd = 0
    rc = c_daylit_columns(c_model_device(this%handle), int(ncol, c_int), mu0, limit, day_index, nd, ECCKD_HOST, c_null_ptr)
    if (rc /= 0) then
      error_msg = c_error_message()
      return
    end if
    n = gas_desc%get_num_gases()
    allocate(up(ncol, nlay + 1), dn(ncol, nlay + 1))
    scale_p = c_null_ptr
    dir_p = c_null_ptr
    if (present(toa_scale)) then
      allocate(scale(ncol))
      scale = toa_scale
      scale_p = c_loc(scale(1))
    end if
    if (present(flux_dir)) then
      allocate(dir(ncol, nlay + 1))
      dir_p = c_loc(dir(1, 1))
    end if
    if (present(tsi) .and. nd > 0) then
      error_msg = daylit_unfused(this, ncol, nlay, nd, day_index, plev, tlay, gas_desc, top_at_1, mu0, sfc_alb_dir, sfc_alb_dif, &
                                 tsi, up, dn, dir)
      if (trim(error_msg) /= "") return
    else   ! (no daylit column: the fused call only zeroes the outputs)
      rc = c_sw_fluxes_daylit(this%handle, int(ncol, c_int), int(nlay, c_int), nd, day_index, plev, tlay, int(n, c_int), names, &
                              ptr, cs, ls, scalar, merge(1_c_int, 0_c_int, top_at_1), mu0, scale_p, sfc_alb_dir, sfc_alb_dif, &
                              0_c_int, c_null_ptr, c_null_ptr, c_null_ptr, 0_c_int, c_null_ptr, up, dn, dir_p, c_null_ptr, &
                              c_null_ptr, c_null_ptr, ECCKD_HOST, c_null_ptr)
      if (rc /= 0) then
        error_msg = c_error_message()
        return
      end if
    end if
    flux_up = up
    flux_dn = dn
    if (present(flux_dir)) flux_dir = dir
  end function sw_fluxes_daylit

  !> The tsi route of sw_fluxes_daylit: gather, gas_optics, the drivers' renormalisation of the beam, rte_sw, scatter.
  !! day_index(1:nd) is the 0-based ascending list; up / dn (and dir, if allocated) are (ncol, nlay+1).
  function daylit_unfused(this, ncol, nlay, nd, day_index, plev, tlay, gas_desc, top_at_1, mu0, sfc_alb_dir, sfc_alb_dif, tsi, &
                          up, dn, dir) result(error_msg)
    class(ty_gas_optics_ecckd), intent(in) :: this
    integer, intent(in) :: ncol, nlay
    integer(c_int), intent(in) :: nd
    integer(c_int), dimension(:), intent(in) :: day_index
    real(wp), dimension(:,:), intent(in) :: plev, tlay
    type(ty_gas_concs), intent(in) :: gas_desc
    logical, intent(in) :: top_at_1
    real(wp), dimension(:), intent(in) :: mu0, tsi
    real(wp), dimension(:,:), intent(in) :: sfc_alb_dir, sfc_alb_dif
    real(wp), dimension(:,:), intent(inout) :: up, dn
    real(wp), dimension(:,:), allocatable, intent(inout) :: dir
    character(len=128) :: error_msg
    type(ty_gas_concs) :: day_gases
    type(ty_optical_props_2str) :: optical_props
    real(wp), dimension(:,:), allocatable :: d_plev, d_tlay, d_ad, d_af, toa, d_up, d_dn, d_dir
    real(wp), dimension(:), allocatable :: d_mu0, d_tsi, def_tsi
    integer(c_int) :: dev, c, l, k, b, g
    integer :: i, j, nb, ng
    dev = c_model_device(this%handle)
    c = int(ncol, c_int)
    l = int(nlay, c_int)
    k = nd
    nb = this%get_nband()
    ng = this%get_ngpt()
    b = int(nb, c_int)
    g = int(ng, c_int)
    allocate(d_plev(nd, nlay + 1), d_tlay(nd, nlay), d_mu0(nd), d_tsi(nd), d_ad(nb, nd), d_af(nb, nd), toa(nd, ng), def_tsi(nd), &
             d_up(nd, nlay + 1), d_dn(nd, nlay + 1), d_dir(nd, nlay + 1))
    error_msg = ""
    ! arrays as (ninner, ncol, nouter): the (ncol, n) planes are (1, ncol, n), the albedos (nband, ncol, 1)
    if (c_gather_columns(dev, 1_c_int, c, l + 1_c_int, 8_c_int, k, day_index, plev, d_plev, ECCKD_HOST, c_null_ptr) /= 0 .or. &
        c_gather_columns(dev, 1_c_int, c, l, 8_c_int, k, day_index, tlay, d_tlay, ECCKD_HOST, c_null_ptr) /= 0 .or. &
        c_gather_columns(dev, 1_c_int, c, 1_c_int, 8_c_int, k, day_index, mu0, d_mu0, ECCKD_HOST, c_null_ptr) /= 0 .or. &
        c_gather_columns(dev, 1_c_int, c, 1_c_int, 8_c_int, k, day_index, tsi, d_tsi, ECCKD_HOST, c_null_ptr) /= 0 .or. &
        c_gather_columns(dev, b, c, 1_c_int, 8_c_int, k, day_index, sfc_alb_dir, d_ad, ECCKD_HOST, c_null_ptr) /= 0 .or. &
        c_gather_columns(dev, b, c, 1_c_int, 8_c_int, k, day_index, sfc_alb_dif, d_af, ECCKD_HOST, c_null_ptr) /= 0) then
      error_msg = c_error_message()
      return
    end if
    day_gases = gas_desc   ! the concentrations that differ between columns, on the daylit columns (the list is 0-based)
    do j = 1, gas_desc%get_num_gases()
      if (.not. allocated(gas_desc%concs(j)%conc)) cycle
      if (size(gas_desc%concs(j)%conc, 1) == ncol) day_gases%concs(j)%conc = gas_desc%concs(j)%conc(day_index(1:nd) + 1, :)
    end do
    error_msg = optical_props%alloc_2str(int(nd), nlay, this)
    if (trim(error_msg) /= "") return
    error_msg = this%gas_optics_ext(d_tlay, d_plev, d_tlay, day_gases, optical_props, toa)   ! (play is not read)
    if (trim(error_msg) /= "") return
    def_tsi = sum(toa, dim=2)                                               ! ecckd_rfmip_sw.F90:126-133
    do i = 1, nd
      toa(i, :) = toa(i, :) * d_tsi(i) / def_tsi(i)
    end do
    if (c_rte_sw_host(dev, k, l, g, merge(1_c_int, 0_c_int, top_at_1), c_loc_3d(optical_props%tau), c_loc_3d(optical_props%ssa), &
                      c_loc_3d(optical_props%g), d_mu0, toa, b, int(optical_props%get_band_lims_gpoint(), c_int), d_ad, d_af, &
                      d_up, d_dn, d_dir, ECCKD_HOST, c_null_ptr) /= 0) then
      error_msg = c_error_message()
      return
    end if
    if (c_scatter_columns(dev, 1_c_int, c, l + 1_c_int, 8_c_int, k, day_index, d_up, up, 0._c_double, ECCKD_HOST, c_null_ptr) /= 0 .or. &
        c_scatter_columns(dev, 1_c_int, c, l + 1_c_int, 8_c_int, k, day_index, d_dn, dn, 0._c_double, ECCKD_HOST, c_null_ptr) /= 0) then
      error_msg = c_error_message()
      return
    end if
    if (allocated(dir)) then
      if (c_scatter_columns(dev, 1_c_int, c, l + 1_c_int, 8_c_int, k, day_index, d_dir, dir, 0._c_double, ECCKD_HOST, c_null_ptr) /= 0) &
        error_msg = c_error_message()
    end if
  end function daylit_unfused

  !> Extension: lw_fluxes with the combined particulate (cloud, aerosol) optical properties on the model's bands,
  !! tau_p / ssa_p (ncol, nlay, nband), added to the gas optical depth inside the solver (ecckd_lw_fluxes_allsky):
  !! tau_gas + tau_p*(1 - ssa_p) with ssa_p [increment_1scalar_by_2stream, by band], tau_gas + tau_p without it
  !! [increment_1scalar_by_1scalar: one-stream particles].  Host arrays in, host fluxes out; the particulate arrays are
  !! never written.  flux_up / flux_dn are (ncol, nlay+1), sfc_emis (nband, ncol).
  !! cloud_mask (ncol, nlay), from sample_cloud_mask (ecckd_lw_fluxes_allsky_mcica): a g-point whose bit is clear sees no
  !! particles in that layer.
  !! flux_up_clear / flux_dn_clear (ncol, nlay+1), both or neither: the clear-sky fluxes of the same columns from the same
  !! gas-optics pass (ecckd_lw_fluxes_clear_allsky) -- what lw_fluxes returns, bit for bit.
  !! flux_up_Jac (ncol, nlay+1): d(flux_up)/d(surface temperature) of the all sky, W m-2 K-1, from the same call
  !! (ecckd_lw_fluxes_jac); every flux array holds the same bits with and without it.
  function lw_fluxes_allsky(this, plev, tlay, tsfc, tlev, gas_desc, top_at_1, sfc_emis, tau_p, flux_up, flux_dn, ssa_p, &
                            n_gauss_angles, cloud_mask, flux_up_clear, flux_dn_clear, flux_up_Jac) result(error_msg)
    class(ty_gas_optics_ecckd), intent(in) :: this
    real(wp), dimension(:,:), intent(in) :: plev, tlay, tlev
    real(wp), dimension(:), intent(in) :: tsfc
    type(ty_gas_concs), intent(in) :: gas_desc
    logical, intent(in) :: top_at_1
    real(wp), dimension(:,:), intent(in) :: sfc_emis
    real(wp), dimension(:,:,:), intent(in) :: tau_p
    real(wp), dimension(:,:), intent(inout) :: flux_up, flux_dn
    real(wp), dimension(:,:,:), intent(in), optional :: ssa_p
    integer, intent(in), optional :: n_gauss_angles
    integer(c_int64_t), dimension(:,:), intent(in), optional :: cloud_mask
    real(wp), dimension(:,:), intent(inout), optional :: flux_up_clear, flux_dn_clear
    real(wp), dimension(:,:), intent(inout), optional :: flux_up_Jac
    character(len=128) :: error_msg
    character(kind=c_char), dimension(:), allocatable :: names
    type(c_ptr), dimension(:), allocatable :: ptr
    integer(c_long_long), dimension(:), allocatable :: cs, ls
    real(c_double), dimension(:), allocatable :: scalar
    real(wp), dimension(:,:), allocatable :: up, dn, jac
    real(wp), dimension(:,:), allocatable, target :: upc, dnc
    real(wp), dimension(:,:,:), allocatable, target :: taup
    type(c_ptr) :: upc_c, dnc_c, taup_c
    real(wp), dimension(:,:,:), allocatable, target :: ssa
    integer(c_int64_t), dimension(:,:), allocatable, target :: mask
    type(c_ptr) :: ssa_c, mask_c
    integer :: ncol, nlay, n, nmus
    integer(c_int) :: rc
    ncol = size(tlay, 1)
    nlay = size(tlay, 2)
    nmus = 1
    if (present(n_gauss_angles)) nmus = n_gauss_angles
    error_msg = marshal_gases(this, gas_desc, ncol, nlay, names, ptr, cs, ls, scalar)
    if (trim(error_msg) /= "") return
    if (size(sfc_emis, 1) /= this%get_nband() .or. size(sfc_emis, 2) /= ncol) then
      error_msg = "lw_fluxes_allsky: sfc_emis inconsistently sized"
      return
    end if
    if (size(tau_p, 1) /= ncol .or. size(tau_p, 2) /= nlay) then
      error_msg = "lw_fluxes_allsky: tau_p inconsistently sized"
      return
    end if
    ssa_c = c_null_ptr
    if (present(ssa_p)) then
      if (any(shape(ssa_p) /= shape(tau_p))) then
        error_msg = "lw_fluxes_allsky: ssa_p inconsistently sized"
        return
      end if
      allocate(ssa(size(ssa_p, 1), size(ssa_p, 2), size(ssa_p, 3)))
      ssa = ssa_p
      if (size(ssa) > 0) ssa_c = c_loc(ssa(1, 1, 1))
    end if
    n = gas_desc%get_num_gases()
    allocate(up(ncol, nlay + 1), dn(ncol, nlay + 1))
    if (present(flux_up_clear) .neqv. present(flux_dn_clear)) then
      error_msg = "lw_fluxes_allsky: flux_up_clear and flux_dn_clear go together"
      return
    end if
    if (present(flux_up_Jac)) then   ! the superset call: any of mask and clear-sky outputs, plus the Jacobian
      if (size(flux_up_Jac, 1) /= ncol .or. size(flux_up_Jac, 2) /= nlay + 1) then
        error_msg = "lw_fluxes_allsky: flux_up_Jac inconsistently sized"
        return
      end if
      mask_c = c_null_ptr
      if (present(cloud_mask)) then
        if (size(cloud_mask, 1) /= ncol .or. size(cloud_mask, 2) /= nlay) then
          error_msg = "lw_fluxes_allsky: cloud_mask inconsistently sized"
          return
        end if
        allocate(mask(ncol, nlay))
        mask = cloud_mask
        if (size(mask) > 0) mask_c = c_loc(mask(1, 1))
      end if
      upc_c = c_null_ptr
      dnc_c = c_null_ptr
      if (present(flux_up_clear)) then
        allocate(upc(ncol, nlay + 1), dnc(ncol, nlay + 1))
        if (size(upc) > 0) then
          upc_c = c_loc(upc(1, 1))
          dnc_c = c_loc(dnc(1, 1))
        end if
      end if
      allocate(taup(ncol, nlay, size(tau_p, 3)), jac(ncol, nlay + 1))
      taup = tau_p
      taup_c = c_null_ptr
      if (size(taup) > 0) taup_c = c_loc(taup(1, 1, 1))
      rc = c_lw_fluxes_jac(this%handle, int(ncol, c_int), int(nlay, c_int), plev, tlay, tsfc, tlev, int(n, c_int), names, ptr, &
                           cs, ls, scalar, merge(1_c_int, 0_c_int, top_at_1), int(nmus, c_int), sfc_emis, c_null_ptr, &
                           int(size(tau_p, 3), c_int), taup_c, ssa_c, mask_c, up, dn, upc_c, dnc_c, jac, ECCKD_HOST, &
                           c_null_ptr)
      if (rc == 0) then
        flux_up_Jac = jac
        if (present(flux_up_clear)) then
          flux_up_clear = upc
          flux_dn_clear = dnc
        end if
      end if
    else if (present(flux_up_clear)) then   ! both skies from one gas-optics pass
      mask_c = c_null_ptr
      if (present(cloud_mask)) then
        if (size(cloud_mask, 1) /= ncol .or. size(cloud_mask, 2) /= nlay) then
          error_msg = "lw_fluxes_allsky: cloud_mask inconsistently sized"
          return
        end if
        allocate(mask(ncol, nlay))
        mask = cloud_mask
        if (size(mask) > 0) mask_c = c_loc(mask(1, 1))
      end if
      allocate(upc(ncol, nlay + 1), dnc(ncol, nlay + 1))
      rc = c_lw_fluxes_clear_allsky(this%handle, int(ncol, c_int), int(nlay, c_int), plev, tlay, tsfc, tlev, int(n, c_int), names, &
                                    ptr, cs, ls, scalar, merge(1_c_int, 0_c_int, top_at_1), int(nmus, c_int), sfc_emis, &
                                    c_null_ptr, int(size(tau_p, 3), c_int), tau_p, ssa_c, mask_c, up, dn, upc, dnc, ECCKD_HOST, &
                                    c_null_ptr)
      if (rc == 0) then
        flux_up_clear = upc
        flux_dn_clear = dnc
      end if
    else if (present(cloud_mask)) then
      if (size(cloud_mask, 1) /= ncol .or. size(cloud_mask, 2) /= nlay) then
        error_msg = "lw_fluxes_allsky: cloud_mask inconsistently sized"
        return
      end if
      rc = c_lw_fluxes_allsky_mcica(this%handle, int(ncol, c_int), int(nlay, c_int), plev, tlay, tsfc, tlev, int(n, c_int), names, &
                                    ptr, cs, ls, scalar, merge(1_c_int, 0_c_int, top_at_1), int(nmus, c_int), sfc_emis, &
                                    c_null_ptr, int(size(tau_p, 3), c_int), tau_p, ssa_c, cloud_mask, up, dn, ECCKD_HOST, &
                                    c_null_ptr)
    else
    rc = c_lw_fluxes_allsky(this%handle, int(ncol, c_int), int(nlay, c_int), plev, tlay, tsfc, tlev, int(n, c_int), names, ptr, &
                            cs, ls, scalar, merge(1_c_int, 0_c_int, top_at_1), int(nmus, c_int), sfc_emis, c_null_ptr, &
                            int(size(tau_p, 3), c_int), tau_p, ssa_c, up, dn, ECCKD_HOST, c_null_ptr)
    end if
    if (rc /= 0) then
      error_msg = c_error_message()
      return
    end if
    flux_up = up
    flux_dn = dn
  end function lw_fluxes_allsky

  !> Extension: sw_fluxes with the combined particulate optical properties on the model's bands, tau_p / ssa_p / g_p
  !! (ncol, nlay, nband), added to the gas optics inside the solver (ecckd_sw_fluxes_allsky) [increment_2stream_by_2stream];
  !! delta_scale: the library first delta-scales a copy of them with f = g*g.  Host arrays in, host fluxes out; the
  !! particulate arrays are never written.  The other arguments are those of sw_fluxes.
  !! cloud_mask (ncol, nlay), from sample_cloud_mask (ecckd_sw_fluxes_allsky_mcica): a g-point whose bit is clear sees no
  !! particles in that layer.
  !! flux_up_clear / flux_dn_clear (both or neither) and, optionally with them, flux_dir_clear: the clear-sky fluxes of the
  !! same columns from the same gas-optics pass (ecckd_sw_fluxes_clear_allsky) -- what sw_fluxes returns, bit for bit.
  function sw_fluxes_allsky(this, plev, tlay, gas_desc, top_at_1, mu0, sfc_alb_dir, sfc_alb_dif, tau_p, ssa_p, g_p, delta_scale, &
                            flux_up, flux_dn, flux_dir, toa_scale, cloud_mask, flux_up_clear, flux_dn_clear, flux_dir_clear) &
      result(error_msg)
    class(ty_gas_optics_ecckd), intent(in) :: this
    real(wp), dimension(:,:), intent(in) :: plev, tlay
    type(ty_gas_concs), intent(in) :: gas_desc
    logical, intent(in) :: top_at_1
    real(wp), dimension(:), intent(in) :: mu0
    real(wp), dimension(:,:), intent(in) :: sfc_alb_dir, sfc_alb_dif
    real(wp), dimension(:,:,:), intent(in) :: tau_p, ssa_p, g_p
    logical, intent(in) :: delta_scale
    real(wp), dimension(:,:), intent(inout) :: flux_up, flux_dn
    real(wp), dimension(:,:), intent(inout), optional :: flux_dir
    real(wp), dimension(:), intent(in), optional, target :: toa_scale
    integer(c_int64_t), dimension(:,:), intent(in), optional :: cloud_mask
    real(wp), dimension(:,:), intent(inout), optional :: flux_up_clear, flux_dn_clear, flux_dir_clear
    character(len=128) :: error_msg
    character(kind=c_char), dimension(:), allocatable :: names
    type(c_ptr), dimension(:), allocatable :: ptr
    integer(c_long_long), dimension(:), allocatable :: cs, ls
    real(c_double), dimension(:), allocatable :: scalar
    real(wp), dimension(:,:), allocatable, target :: up, dn, dir, upc, dnc, dirc
    real(wp), dimension(:), allocatable, target :: scale
    integer(c_int64_t), dimension(:,:), allocatable, target :: mask
    type(c_ptr) :: scale_p, dir_p, dirc_p, mask_c
    integer :: ncol, nlay, n
    integer(c_int) :: rc
    ncol = size(tlay, 1)
    nlay = size(tlay, 2)
    error_msg = marshal_gases(this, gas_desc, ncol, nlay, names, ptr, cs, ls, scalar)
    if (trim(error_msg) /= "") return
    if (size(sfc_alb_dir, 1) /= this%get_nband() .or. size(sfc_alb_dir, 2) /= ncol .or. &
        size(sfc_alb_dif, 1) /= this%get_nband() .or. size(sfc_alb_dif, 2) /= ncol) then
      error_msg = "sw_fluxes_allsky: surface albedos inconsistently sized"
      return
    end if
    if (size(tau_p, 1) /= ncol .or. size(tau_p, 2) /= nlay .or. any(shape(ssa_p) /= shape(tau_p)) .or. &
        any(shape(g_p) /= shape(tau_p))) then
      error_msg = "sw_fluxes_allsky: tau_p, ssa_p, g_p inconsistently sized"
      return
    end if
    n = gas_desc%get_num_gases()
    allocate(up(ncol, nlay + 1), dn(ncol, nlay + 1))
    scale_p = c_null_ptr
    dir_p = c_null_ptr
    if (present(toa_scale)) then
      allocate(scale(ncol))
      scale = toa_scale
      scale_p = c_loc(scale(1))
    end if
    if (present(flux_dir)) then
      allocate(dir(ncol, nlay + 1))
      dir_p = c_loc(dir(1, 1))
    end if
    if ((present(flux_up_clear) .neqv. present(flux_dn_clear)) .or. (present(flux_dir_clear) .and. .not. present(flux_up_clear))) then
      error_msg = "sw_fluxes_allsky: flux_up_clear and flux_dn_clear go together (flux_dir_clear with them)"
      return
    end if
    if (present(flux_up_clear)) then   ! both skies from one gas-optics pass
      mask_c = c_null_ptr
      if (present(cloud_mask)) then
        if (size(cloud_mask, 1) /= ncol .or. size(cloud_mask, 2) /= nlay) then
          error_msg = "sw_fluxes_allsky: cloud_mask inconsistently sized"
          return
        end if
        allocate(mask(ncol, nlay))
        mask = cloud_mask
        if (size(mask) > 0) mask_c = c_loc(mask(1, 1))
      end if
      allocate(upc(ncol, nlay + 1), dnc(ncol, nlay + 1))
      dirc_p = c_null_ptr
      if (present(flux_dir_clear)) then
        allocate(dirc(ncol, nlay + 1))
        dirc_p = c_loc(dirc(1, 1))
      end if
      rc = c_sw_fluxes_clear_allsky(this%handle, int(ncol, c_int), int(nlay, c_int), plev, tlay, int(n, c_int), names, ptr, cs, &
                                    ls, scalar, merge(1_c_int, 0_c_int, top_at_1), mu0, scale_p, sfc_alb_dir, sfc_alb_dif, &
                                    int(size(tau_p, 3), c_int), tau_p, ssa_p, g_p, merge(1_c_int, 0_c_int, delta_scale), &
                                    mask_c, up, dn, dir_p, upc, dnc, dirc_p, ECCKD_HOST, c_null_ptr)
      if (rc == 0) then
        flux_up_clear = upc
        flux_dn_clear = dnc
        if (present(flux_dir_clear)) flux_dir_clear = dirc
      end if
    else if (present(cloud_mask)) then
      if (size(cloud_mask, 1) /= ncol .or. size(cloud_mask, 2) /= nlay) then
        error_msg = "sw_fluxes_allsky: cloud_mask inconsistently sized"
        return
      end if
      rc = c_sw_fluxes_allsky_mcica(this%handle, int(ncol, c_int), int(nlay, c_int), plev, tlay, int(n, c_int), names, ptr, cs, &
                                    ls, scalar, merge(1_c_int, 0_c_int, top_at_1), mu0, scale_p, sfc_alb_dir, sfc_alb_dif, &
                                    int(size(tau_p, 3), c_int), tau_p, ssa_p, g_p, merge(1_c_int, 0_c_int, delta_scale), &
                                    cloud_mask, up, dn, dir_p, ECCKD_HOST, c_null_ptr)
    else
    rc = c_sw_fluxes_allsky(this%handle, int(ncol, c_int), int(nlay, c_int), plev, tlay, int(n, c_int), names, ptr, cs, ls, &
                            scalar, merge(1_c_int, 0_c_int, top_at_1), mu0, scale_p, sfc_alb_dir, sfc_alb_dif, &
                            int(size(tau_p, 3), c_int), tau_p, ssa_p, g_p, merge(1_c_int, 0_c_int, delta_scale), up, dn, dir_p, &
                            ECCKD_HOST, c_null_ptr)
    end if
    if (rc /= 0) then
      error_msg = c_error_message()
      return
    end if
    flux_up = up
    flux_dn = dn
    if (present(flux_dir)) flux_dir = dir
  end function sw_fluxes_allsky

  !> Extension: lw_fluxes / lw_fluxes_allsky with per-band output (ecckd_lw_flux_bands; include/ecckd_hip.h, "Fused
  !! per-band fluxes"): bnd_flux_up / bnd_flux_dn (ncol, nlay+1, nband) receive, per band of the model, the sum over the
  !! band's g-points -- what gas_optics + [increment by band] + rte_lw with a ty_fluxes_byband give.  tau_p (ncol, nlay,
  !! nband), optional: the particles, with ssa_p (absorption optical depth) or without (one-stream); cloud_mask (ncol, nlay)
  !! with tau_p only; inc_flux (ncol, ngpt).  flux_up / flux_dn (ncol, nlay+1), optional: the sum of the planes in band
  !! order.  Host arrays in, host fluxes out; no input is written.
  function lw_flux_bands(this, plev, tlay, tsfc, tlev, gas_desc, top_at_1, sfc_emis, bnd_flux_up, bnd_flux_dn, tau_p, ssa_p, &
                         n_gauss_angles, cloud_mask, inc_flux, flux_up, flux_dn) result(error_msg)
    class(ty_gas_optics_ecckd), intent(in) :: this
    real(wp), dimension(:,:), intent(in) :: plev, tlay, tlev
    real(wp), dimension(:), intent(in) :: tsfc
    type(ty_gas_concs), intent(in) :: gas_desc
    logical, intent(in) :: top_at_1
    real(wp), dimension(:,:), intent(in) :: sfc_emis
    real(wp), dimension(:,:,:), intent(inout) :: bnd_flux_up, bnd_flux_dn
    real(wp), dimension(:,:,:), intent(in), optional :: tau_p, ssa_p
    integer, intent(in), optional :: n_gauss_angles
    integer(c_int64_t), intent(in), optional :: cloud_mask(:,:)
    real(wp), dimension(:,:), intent(in), optional :: inc_flux
    real(wp), dimension(:,:), intent(inout), optional :: flux_up, flux_dn
    character(len=128) :: error_msg
    character(kind=c_char), dimension(:), allocatable :: names
    type(c_ptr), dimension(:), allocatable :: ptr
    integer(c_long_long), dimension(:), allocatable :: cs, ls
    real(c_double), dimension(:), allocatable :: scalar
    real(wp), dimension(:,:,:), allocatable :: bup, bdn
    real(wp), dimension(:,:,:), allocatable, target :: taup, ssa
    real(wp), dimension(:,:), allocatable, target :: incf, up, dn
    integer(c_int64_t), dimension(:,:), allocatable, target :: mask
    type(c_ptr) :: taup_c, ssa_c, mask_c, incf_c, up_c, dn_c
    integer :: ncol, nlay, n, nmus, nband, nbp
    integer(c_int) :: rc
    ncol = size(tlay, 1)
    nlay = size(tlay, 2)
    nband = this%get_nband()
    nmus = 1
    if (present(n_gauss_angles)) nmus = n_gauss_angles
    error_msg = marshal_gases(this, gas_desc, ncol, nlay, names, ptr, cs, ls, scalar)
    if (trim(error_msg) /= "") return
    if (size(sfc_emis, 1) /= nband .or. size(sfc_emis, 2) /= ncol) then
      error_msg = "lw_flux_bands: sfc_emis inconsistently sized"
      return
    end if
    if (any(shape(bnd_flux_up) /= [ncol, nlay + 1, nband]) .or. any(shape(bnd_flux_dn) /= [ncol, nlay + 1, nband])) then
      error_msg = "lw_flux_bands: bnd_flux_up, bnd_flux_dn inconsistently sized"
      return
    end if
    taup_c = c_null_ptr; ssa_c = c_null_ptr; mask_c = c_null_ptr; incf_c = c_null_ptr; up_c = c_null_ptr; dn_c = c_null_ptr
    nbp = 0
    if (present(tau_p)) then
      if (size(tau_p, 1) /= ncol .or. size(tau_p, 2) /= nlay) then
        error_msg = "lw_flux_bands: tau_p inconsistently sized"
        return
      end if
      nbp = size(tau_p, 3)
      allocate(taup(ncol, nlay, nbp))
      taup = tau_p
      if (size(taup) > 0) taup_c = c_loc(taup(1, 1, 1))
    end if
    if (present(ssa_p)) then
      if (.not. present(tau_p)) then
        error_msg = "lw_flux_bands: ssa_p and cloud_mask belong to tau_p"
        return
      else if (any(shape(ssa_p) /= shape(tau_p))) then
        error_msg = "lw_flux_bands: ssa_p inconsistently sized"
        return
      end if
      allocate(ssa(ncol, nlay, nbp))
      ssa = ssa_p
      if (size(ssa) > 0) ssa_c = c_loc(ssa(1, 1, 1))
    end if
    if (present(cloud_mask)) then
      if (.not. present(tau_p)) then
        error_msg = "lw_flux_bands: ssa_p and cloud_mask belong to tau_p"
        return
      else if (size(cloud_mask, 1) /= ncol .or. size(cloud_mask, 2) /= nlay) then
        error_msg = "lw_flux_bands: cloud_mask inconsistently sized"
        return
      end if
      allocate(mask(ncol, nlay))
      mask = cloud_mask
      if (size(mask) > 0) mask_c = c_loc(mask(1, 1))
    end if
    if (present(inc_flux)) then
      if (size(inc_flux, 1) /= ncol .or. size(inc_flux, 2) /= this%get_ngpt()) then
        error_msg = "lw_flux_bands: inc_flux inconsistently sized"
        return
      end if
      allocate(incf(ncol, size(inc_flux, 2)))
      incf = inc_flux
      if (size(incf) > 0) incf_c = c_loc(incf(1, 1))
    end if
    if (present(flux_up)) then
      allocate(up(ncol, nlay + 1))
      if (size(up) > 0) up_c = c_loc(up(1, 1))
    end if
    if (present(flux_dn)) then
      allocate(dn(ncol, nlay + 1))
      if (size(dn) > 0) dn_c = c_loc(dn(1, 1))
    end if
    n = gas_desc%get_num_gases()
    allocate(bup(ncol, nlay + 1, nband), bdn(ncol, nlay + 1, nband))
    rc = c_lw_flux_bands(this%handle, int(ncol, c_int), int(nlay, c_int), plev, tlay, tsfc, tlev, int(n, c_int), names, ptr, cs, &
                         ls, scalar, merge(1_c_int, 0_c_int, top_at_1), int(nmus, c_int), sfc_emis, incf_c, int(nbp, c_int), &
                         taup_c, ssa_c, mask_c, bup, bdn, up_c, dn_c, ECCKD_HOST, c_null_ptr)
    if (rc /= 0) then
      error_msg = c_error_message()
      return
    end if
    bnd_flux_up = bup
    bnd_flux_dn = bdn
    if (present(flux_up)) flux_up = up
    if (present(flux_dn)) flux_dn = dn
  end function lw_flux_bands

  !> Extension: sw_fluxes / sw_fluxes_allsky with per-band output (ecckd_sw_flux_bands): bnd_flux_up / bnd_flux_dn and,
  !! optionally, bnd_flux_dir (ncol, nlay+1, nband); tau_p / ssa_p / g_p (ncol, nlay, nband), all three or none, delta_scale
  !! as in sw_fluxes_allsky (default .true.); cloud_mask with particles only; toa_scale (ncol).  flux_up / flux_dn / flux_dir
  !! (ncol, nlay+1), optional: the sum of the planes in band order (flux_dir needs bnd_flux_dir).  Host arrays throughout.
  function sw_flux_bands(this, plev, tlay, gas_desc, top_at_1, mu0, sfc_alb_dir, sfc_alb_dif, bnd_flux_up, bnd_flux_dn, &
                         bnd_flux_dir, tau_p, ssa_p, g_p, delta_scale, toa_scale, cloud_mask, flux_up, flux_dn, flux_dir) &
      result(error_msg)
    class(ty_gas_optics_ecckd), intent(in) :: this
    real(wp), dimension(:,:), intent(in) :: plev, tlay
    type(ty_gas_concs), intent(in) :: gas_desc
    logical, intent(in) :: top_at_1
    real(wp), dimension(:), intent(in) :: mu0
    real(wp), dimension(:,:), intent(in) :: sfc_alb_dir, sfc_alb_dif
    real(wp), dimension(:,:,:), intent(inout) :: bnd_flux_up, bnd_flux_dn
    real(wp), dimension(:,:,:), intent(inout), optional :: bnd_flux_dir
    real(wp), dimension(:,:,:), intent(in), optional :: tau_p, ssa_p, g_p
    logical, intent(in), optional :: delta_scale
    real(wp), dimension(:), intent(in), optional :: toa_scale
    integer(c_int64_t), intent(in), optional :: cloud_mask(:,:)
    real(wp), dimension(:,:), intent(inout), optional :: flux_up, flux_dn, flux_dir
    character(len=128) :: error_msg
    character(kind=c_char), dimension(:), allocatable :: names
    type(c_ptr), dimension(:), allocatable :: ptr
    integer(c_long_long), dimension(:), allocatable :: cs, ls
    real(c_double), dimension(:), allocatable :: scalar
    real(wp), dimension(:,:,:), allocatable :: bup, bdn
    real(wp), dimension(:,:,:), allocatable, target :: bdir, taup, ssa, asy
    real(wp), dimension(:,:), allocatable, target :: up, dn, dir
    real(wp), dimension(:), allocatable, target :: scale
    integer(c_int64_t), dimension(:,:), allocatable, target :: mask
    type(c_ptr) :: taup_c, ssa_c, asy_c, mask_c, scale_c, bdir_c, up_c, dn_c, dir_c
    integer :: ncol, nlay, n, nband, nbp
    integer(c_int) :: rc, ds
    ncol = size(tlay, 1)
    nlay = size(tlay, 2)
    nband = this%get_nband()
    ds = 1_c_int
    if (present(delta_scale)) ds = merge(1_c_int, 0_c_int, delta_scale)
    error_msg = marshal_gases(this, gas_desc, ncol, nlay, names, ptr, cs, ls, scalar)
    if (trim(error_msg) /= "") return
    if (size(sfc_alb_dir, 1) /= nband .or. size(sfc_alb_dir, 2) /= ncol .or. &
        size(sfc_alb_dif, 1) /= nband .or. size(sfc_alb_dif, 2) /= ncol) then
      error_msg = "sw_flux_bands: surface albedos inconsistently sized"
      return
    end if
    if (any(shape(bnd_flux_up) /= [ncol, nlay + 1, nband]) .or. any(shape(bnd_flux_dn) /= [ncol, nlay + 1, nband])) then
      error_msg = "sw_flux_bands: bnd_flux_up, bnd_flux_dn inconsistently sized"
      return
    end if
    taup_c = c_null_ptr; ssa_c = c_null_ptr; asy_c = c_null_ptr; mask_c = c_null_ptr; scale_c = c_null_ptr
    bdir_c = c_null_ptr; up_c = c_null_ptr; dn_c = c_null_ptr; dir_c = c_null_ptr
    nbp = 0
    if (present(tau_p) .or. present(ssa_p) .or. present(g_p)) then
      if (.not. (present(tau_p) .and. present(ssa_p) .and. present(g_p))) then
        error_msg = "sw_flux_bands: tau_p, ssa_p and g_p go together"
        return
      else if (size(tau_p, 1) /= ncol .or. size(tau_p, 2) /= nlay .or. any(shape(ssa_p) /= shape(tau_p)) .or. &
               any(shape(g_p) /= shape(tau_p))) then
        error_msg = "sw_flux_bands: tau_p, ssa_p, g_p inconsistently sized"
        return
      end if
      nbp = size(tau_p, 3)
      allocate(taup(ncol, nlay, nbp), ssa(ncol, nlay, nbp), asy(ncol, nlay, nbp))
      taup = tau_p
      ssa = ssa_p
      asy = g_p
      if (size(taup) > 0) then
        taup_c = c_loc(taup(1, 1, 1))
        ssa_c = c_loc(ssa(1, 1, 1))
        asy_c = c_loc(asy(1, 1, 1))
      end if
    end if
    if (present(cloud_mask)) then
      if (nbp == 0) then
        error_msg = "sw_flux_bands: cloud_mask belongs to particles"
        return
      else if (size(cloud_mask, 1) /= ncol .or. size(cloud_mask, 2) /= nlay) then
        error_msg = "sw_flux_bands: cloud_mask inconsistently sized"
        return
      end if
      allocate(mask(ncol, nlay))
      mask = cloud_mask
      if (size(mask) > 0) mask_c = c_loc(mask(1, 1))
    end if
    if (present(toa_scale)) then
      allocate(scale(ncol))
      scale = toa_scale
      if (ncol > 0) scale_c = c_loc(scale(1))
    end if
    if (present(bnd_flux_dir)) then
      if (any(shape(bnd_flux_dir) /= [ncol, nlay + 1, nband])) then
        error_msg = "sw_flux_bands: bnd_flux_dir inconsistently sized"
        return
      end if
      allocate(bdir(ncol, nlay + 1, nband))
      if (size(bdir) > 0) bdir_c = c_loc(bdir(1, 1, 1))
    end if
    if (present(flux_up)) then
      allocate(up(ncol, nlay + 1))
      if (size(up) > 0) up_c = c_loc(up(1, 1))
    end if
    if (present(flux_dn)) then
      allocate(dn(ncol, nlay + 1))
      if (size(dn) > 0) dn_c = c_loc(dn(1, 1))
    end if
    if (present(flux_dir)) then
      allocate(dir(ncol, nlay + 1))
      if (size(dir) > 0) dir_c = c_loc(dir(1, 1))
    end if
    n = gas_desc%get_num_gases()
    allocate(bup(ncol, nlay + 1, nband), bdn(ncol, nlay + 1, nband))
    rc = c_sw_flux_bands(this%handle, int(ncol, c_int), int(nlay, c_int), plev, tlay, int(n, c_int), names, ptr, cs, ls, scalar, &
                         merge(1_c_int, 0_c_int, top_at_1), mu0, scale_c, sfc_alb_dir, sfc_alb_dif, int(nbp, c_int), taup_c, ssa_c, &
                         asy_c, ds, mask_c, bup, bdn, bdir_c, up_c, dn_c, dir_c, ECCKD_HOST, c_null_ptr)
    if (rc /= 0) then
      error_msg = c_error_message()
      return
    end if
    bnd_flux_up = bup
    bnd_flux_dn = bdn
    if (present(bnd_flux_dir)) bnd_flux_dir = bdir
    if (present(flux_up)) flux_up = up
    if (present(flux_dn)) flux_dn = dn
    if (present(flux_dir)) flux_dir = dir
  end function sw_flux_bands

  !> Extension: the McICA cloud mask of ecckd_cloud_mask_sample (the definition is in include/ecckd_hip.h; parity with
  !! RTE-RRTMGP's mo_cloud_sampling is unpinned) for this model's g-points: cloud_frac (ncol, nlay) in the layer order of
  !! tlay, overlap ECCKD_OVERLAP_MAX_RAN or ECCKD_OVERLAP_EXP_RAN (then overlap_param (ncol, nlay-1)), col0 the global
  !! 0-based index of the first column (a host that works in blocks passes its block offset, so that the mask of a column
  !! does not depend on the blocking).  cloud_mask (ncol, nlay): bit g-1 of a word set = g-point g sees the layer's cloud.
  function sample_cloud_mask(this, cloud_frac, overlap, seed, col0, cloud_mask, overlap_param) result(error_msg)
    class(ty_gas_optics_ecckd), intent(in) :: this
    real(wp), dimension(:,:), intent(in) :: cloud_frac
    integer, intent(in) :: overlap
    integer(c_int64_t), intent(in) :: seed, col0
    integer(c_int64_t), dimension(:,:), intent(inout) :: cloud_mask
    real(wp), dimension(:,:), intent(in), optional :: overlap_param
    character(len=128) :: error_msg
    real(wp), dimension(:,:), allocatable, target :: alpha
    integer(c_int64_t), dimension(:,:), allocatable :: words
    type(c_ptr) :: alpha_p
    integer :: ncol, nlay
    integer(c_int) :: rc
    error_msg = ""
    ncol = size(cloud_frac, 1)
    nlay = size(cloud_frac, 2)
    if (size(cloud_mask, 1) /= ncol .or. size(cloud_mask, 2) /= nlay) then
      error_msg = "sample_cloud_mask: cloud_mask inconsistently sized"
      return
    end if
    alpha_p = c_null_ptr
    if (present(overlap_param)) then
      if (size(overlap_param, 1) /= ncol .or. size(overlap_param, 2) /= nlay - 1) then
        error_msg = "sample_cloud_mask: overlap_param inconsistently sized"
        return
      end if
      allocate(alpha(ncol, max(nlay - 1, 1)))
      alpha(:, 1:nlay - 1) = overlap_param
      alpha_p = c_loc(alpha(1, 1))
    end if
    allocate(words(ncol, nlay))
    rc = c_cloud_mask_sample(c_model_device(this%handle), int(ncol, c_int), int(nlay, c_int), int(this%get_ngpt(), c_int), &
                             int(overlap, c_int), cloud_frac, alpha_p, seed, col0, words, ECCKD_HOST, c_null_ptr)
    if (rc /= 0) then
      error_msg = c_error_message()
      return
    end if
    cloud_mask = words
  end function sample_cloud_mask

  !> The lognormal table of ecckd_cloud_scaling_lognormal (bin means of the unit-mean distribution) on the device of `model`.
  function cloud_scaling_load_lognormal(this, model, nfsd, fsd0, dfsd, nq) result(error_msg)
    class(ty_cloud_scaling), intent(inout) :: this
    class(ty_gas_optics_ecckd), intent(in) :: model
    integer, intent(in) :: nfsd, nq
    real(wp), intent(in) :: fsd0, dfsd
    character(len=128) :: error_msg
    real(c_double), dimension(:,:), allocatable :: values
    error_msg = ""
    allocate(values(max(nq, 1), max(nfsd, 1)))
    if (c_cloud_scaling_lognormal(int(nfsd, c_int), real(fsd0, c_double), real(dfsd, c_double), int(nq, c_int), values) /= 0) then
      error_msg = c_error_message()
      return
    end if
    error_msg = this%load_table(model, values, fsd0, dfsd)
  end function cloud_scaling_load_lognormal

  !> A table of the host's own: values (nq, nfsd).
  function cloud_scaling_load_table(this, model, values, fsd0, dfsd) result(error_msg)
    class(ty_cloud_scaling), intent(inout) :: this
    class(ty_gas_optics_ecckd), intent(in) :: model
    real(wp), dimension(:,:), intent(in) :: values
    real(wp), intent(in) :: fsd0, dfsd
    character(len=128) :: error_msg
    real(c_double), dimension(:,:), allocatable :: v
    error_msg = ""
    call this%finalize()
    allocate(v(size(values, 1), size(values, 2)))
    v = values
    if (c_cloud_scaling_create(c_model_device(model%handle), int(size(v, 2), c_int), real(fsd0, c_double), real(dfsd, c_double), &
                               int(size(v, 1), c_int), v, this%handle) /= 0) then
      this%handle = c_null_ptr
      error_msg = c_error_message()
    end if
  end function cloud_scaling_load_table

  subroutine cloud_scaling_finalize(this)
    class(ty_cloud_scaling), intent(inout) :: this
    if (c_associated(this%handle)) call c_cloud_scaling_destroy(this%handle)
    this%handle = c_null_ptr
  end subroutine cloud_scaling_finalize

  !> Extension: the sampled optical-depth scaling of ecckd_cloud_scaling_sample (the definition is in include/ecckd_hip.h;
  !! parity with ecRad and RTE-RRTMGP is unpinned) for this model's g-points: cloud_frac, overlap, seed, col0, overlap_param
  !! as sample_cloud_mask; fsd (ncol, nlay), or fsd_const for every cell (fsd wins).  cloud_scaling (ncol, nlay, ngpt),
  !! single precision: 0 where the g-point does not see the layer's cloud.  cloud_mask (ncol, nlay), optional: the words of
  !! sample_cloud_mask.
  function sample_cloud_scaling(this, table, cloud_frac, overlap, seed, col0, cloud_scaling, fsd, fsd_const, overlap_param, &
                                cloud_mask) result(error_msg)
    class(ty_gas_optics_ecckd), intent(in) :: this
    type(ty_cloud_scaling), intent(in) :: table
    real(wp), dimension(:,:), intent(in) :: cloud_frac
    integer, intent(in) :: overlap
    integer(c_int64_t), intent(in) :: seed, col0
    real(c_float), dimension(:,:,:), intent(inout) :: cloud_scaling
    real(wp), dimension(:,:), intent(in), optional :: fsd
    real(wp), intent(in), optional :: fsd_const
    real(wp), dimension(:,:), intent(in), optional :: overlap_param
    integer(c_int64_t), dimension(:,:), intent(inout), optional :: cloud_mask
    character(len=128) :: error_msg
    real(wp), dimension(:,:), allocatable, target :: alpha, f
    integer(c_int64_t), dimension(:,:), allocatable, target :: words
    real(c_float), dimension(:,:,:), allocatable :: s
    type(c_ptr) :: alpha_p, f_p, words_p
    real(c_double) :: fc
    integer :: ncol, nlay, ng
    integer(c_int) :: rc
    error_msg = ""
    ncol = size(cloud_frac, 1)
    nlay = size(cloud_frac, 2)
    ng = this%get_ngpt()
    if (any(shape(cloud_scaling) /= [ncol, nlay, ng])) then
      error_msg = "sample_cloud_scaling: cloud_scaling inconsistently sized"
      return
    end if
    alpha_p = c_null_ptr; f_p = c_null_ptr; words_p = c_null_ptr
    fc = 0._c_double
    if (present(fsd_const)) fc = real(fsd_const, c_double)
    if (present(fsd)) then
      if (any(shape(fsd) /= shape(cloud_frac))) then
        error_msg = "sample_cloud_scaling: fsd inconsistently sized"
        return
      end if
      allocate(f(ncol, nlay))
      f = fsd
      if (size(f) > 0) f_p = c_loc(f(1, 1))
    else if (.not. present(fsd_const)) then
      error_msg = "sample_cloud_scaling: fsd or fsd_const is required"
      return
    end if
    if (present(overlap_param)) then
      if (size(overlap_param, 1) /= ncol .or. size(overlap_param, 2) /= nlay - 1) then
        error_msg = "sample_cloud_scaling: overlap_param inconsistently sized"
        return
      end if
      allocate(alpha(ncol, max(nlay - 1, 1)))
      alpha(:, 1:nlay - 1) = overlap_param
      alpha_p = c_loc(alpha(1, 1))
    end if
    if (present(cloud_mask)) then
      if (size(cloud_mask, 1) /= ncol .or. size(cloud_mask, 2) /= nlay) then
        error_msg = "sample_cloud_scaling: cloud_mask inconsistently sized"
        return
      end if
      allocate(words(ncol, nlay))
      if (size(words) > 0) words_p = c_loc(words(1, 1))
    end if
    allocate(s(ncol, nlay, ng))
    rc = c_cloud_scaling_sample(c_model_device(this%handle), int(ncol, c_int), int(nlay, c_int), int(ng, c_int), &
                                int(overlap, c_int), cloud_frac, alpha_p, f_p, fc, table%handle, seed, col0, s, words_p, &
                                ECCKD_HOST, c_null_ptr)
    if (rc /= 0) then
      error_msg = c_error_message()
      return
    end if
    cloud_scaling = s
    if (present(cloud_mask)) cloud_mask = words
  end function sample_cloud_scaling

  !> Extension: lw_fluxes_allsky with the particulate optical depth of every (layer, g-point) cell multiplied by
  !! cloud_scaling (ncol, nlay, ngpt), single precision (ecckd_lw_flux_scaled): what gas_optics + increment_scaled by band +
  !! rte_lw give, bit for bit.  tau_p (ncol, nlay, nband) with ssa_p (absorption optical depth) or without (one-stream).
  !! Host arrays in, host fluxes out; no input is written.
  function lw_flux_scaled(this, plev, tlay, tsfc, tlev, gas_desc, top_at_1, sfc_emis, tau_p, cloud_scaling, flux_up, flux_dn, &
                          ssa_p, n_gauss_angles, inc_flux) result(error_msg)
    class(ty_gas_optics_ecckd), intent(in) :: this
    real(wp), dimension(:,:), intent(in) :: plev, tlay, tlev
    real(wp), dimension(:), intent(in) :: tsfc
    type(ty_gas_concs), intent(in) :: gas_desc
    logical, intent(in) :: top_at_1
    real(wp), dimension(:,:), intent(in) :: sfc_emis
    real(wp), dimension(:,:,:), intent(in) :: tau_p
    real(c_float), dimension(:,:,:), intent(in) :: cloud_scaling
    real(wp), dimension(:,:), intent(inout) :: flux_up, flux_dn
    real(wp), dimension(:,:,:), intent(in), optional :: ssa_p
    integer, intent(in), optional :: n_gauss_angles
    real(wp), dimension(:,:), intent(in), optional :: inc_flux
    character(len=128) :: error_msg
    character(kind=c_char), dimension(:), allocatable :: names
    type(c_ptr), dimension(:), allocatable :: ptr
    integer(c_long_long), dimension(:), allocatable :: cs, ls
    real(c_double), dimension(:), allocatable :: scalar
    real(wp), dimension(:,:,:), allocatable, target :: ssa
    real(wp), dimension(:,:), allocatable, target :: incf
    real(wp), dimension(:,:), allocatable :: up, dn
    type(c_ptr) :: ssa_c, incf_c
    integer :: ncol, nlay, n, nmus
    integer(c_int) :: rc
    ncol = size(tlay, 1)
    nlay = size(tlay, 2)
    nmus = 1
    if (present(n_gauss_angles)) nmus = n_gauss_angles
    error_msg = marshal_gases(this, gas_desc, ncol, nlay, names, ptr, cs, ls, scalar)
    if (trim(error_msg) /= "") return
    if (size(sfc_emis, 1) /= this%get_nband() .or. size(sfc_emis, 2) /= ncol) then
      error_msg = "lw_flux_scaled: sfc_emis inconsistently sized"
      return
    end if
    if (size(tau_p, 1) /= ncol .or. size(tau_p, 2) /= nlay) then
      error_msg = "lw_flux_scaled: tau_p inconsistently sized"
      return
    end if
    if (any(shape(cloud_scaling) /= [ncol, nlay, this%get_ngpt()])) then
      error_msg = "lw_flux_scaled: cloud_scaling inconsistently sized"
      return
    end if
    if (any(shape(flux_up) /= [ncol, nlay + 1]) .or. any(shape(flux_dn) /= [ncol, nlay + 1])) then
      error_msg = "lw_flux_scaled: flux_up, flux_dn inconsistently sized"
      return
    end if
    ssa_c = c_null_ptr; incf_c = c_null_ptr
    if (present(ssa_p)) then
      if (any(shape(ssa_p) /= shape(tau_p))) then
        error_msg = "lw_flux_scaled: ssa_p inconsistently sized"
        return
      end if
      allocate(ssa(ncol, nlay, size(tau_p, 3)))
      ssa = ssa_p
      if (size(ssa) > 0) ssa_c = c_loc(ssa(1, 1, 1))
    end if
    if (present(inc_flux)) then
      if (size(inc_flux, 1) /= ncol .or. size(inc_flux, 2) /= this%get_ngpt()) then
        error_msg = "lw_flux_scaled: inc_flux inconsistently sized"
        return
      end if
      allocate(incf(ncol, size(inc_flux, 2)))
      incf = inc_flux
      if (size(incf) > 0) incf_c = c_loc(incf(1, 1))
    end if
    n = gas_desc%get_num_gases()
    allocate(up(ncol, nlay + 1), dn(ncol, nlay + 1))
    rc = c_lw_flux_scaled(this%handle, int(ncol, c_int), int(nlay, c_int), plev, tlay, tsfc, tlev, int(n, c_int), names, ptr, cs, &
                          ls, scalar, merge(1_c_int, 0_c_int, top_at_1), int(nmus, c_int), sfc_emis, incf_c, &
                          int(size(tau_p, 3), c_int), tau_p, ssa_c, cloud_scaling, up, dn, ECCKD_HOST, c_null_ptr)
    if (rc /= 0) then
      error_msg = c_error_message()
      return
    end if
    flux_up = up
    flux_dn = dn
  end function lw_flux_scaled

  !> Extension: sw_fluxes_allsky with the particulate optical depth of every (layer, g-point) cell -- after the delta
  !! scaling -- multiplied by cloud_scaling (ncol, nlay, ngpt), single precision (ecckd_sw_flux_scaled).  tau_p / ssa_p / g_p
  !! (ncol, nlay, nband); delta_scale as in sw_fluxes_allsky (default .true.); toa_scale (ncol); flux_dir optional.
  function sw_flux_scaled(this, plev, tlay, gas_desc, top_at_1, mu0, sfc_alb_dir, sfc_alb_dif, tau_p, ssa_p, g_p, cloud_scaling, &
                          flux_up, flux_dn, flux_dir, delta_scale, toa_scale) result(error_msg)
    class(ty_gas_optics_ecckd), intent(in) :: this
    real(wp), dimension(:,:), intent(in) :: plev, tlay
    type(ty_gas_concs), intent(in) :: gas_desc
    logical, intent(in) :: top_at_1
    real(wp), dimension(:), intent(in) :: mu0
    real(wp), dimension(:,:), intent(in) :: sfc_alb_dir, sfc_alb_dif
    real(wp), dimension(:,:,:), intent(in) :: tau_p, ssa_p, g_p
    real(c_float), dimension(:,:,:), intent(in) :: cloud_scaling
    real(wp), dimension(:,:), intent(inout) :: flux_up, flux_dn
    real(wp), dimension(:,:), intent(inout), optional :: flux_dir
    logical, intent(in), optional :: delta_scale
    real(wp), dimension(:), intent(in), optional :: toa_scale
    character(len=128) :: error_msg
    character(kind=c_char), dimension(:), allocatable :: names
    type(c_ptr), dimension(:), allocatable :: ptr
    integer(c_long_long), dimension(:), allocatable :: cs, ls
    real(c_double), dimension(:), allocatable :: scalar
    real(wp), dimension(:,:), allocatable, target :: dir
    real(wp), dimension(:,:), allocatable :: up, dn
    real(wp), dimension(:), allocatable, target :: scale
    type(c_ptr) :: scale_c, dir_c
    integer :: ncol, nlay, n, nband
    integer(c_int) :: rc, ds
    ncol = size(tlay, 1)
    nlay = size(tlay, 2)
    nband = this%get_nband()
    ds = 1_c_int
    if (present(delta_scale)) ds = merge(1_c_int, 0_c_int, delta_scale)
    error_msg = marshal_gases(this, gas_desc, ncol, nlay, names, ptr, cs, ls, scalar)
    if (trim(error_msg) /= "") return
    if (size(sfc_alb_dir, 1) /= nband .or. size(sfc_alb_dir, 2) /= ncol .or. &
        size(sfc_alb_dif, 1) /= nband .or. size(sfc_alb_dif, 2) /= ncol) then
      error_msg = "sw_flux_scaled: surface albedos inconsistently sized"
      return
    end if
    if (size(tau_p, 1) /= ncol .or. size(tau_p, 2) /= nlay .or. any(shape(ssa_p) /= shape(tau_p)) .or. &
        any(shape(g_p) /= shape(tau_p))) then
      error_msg = "sw_flux_scaled: tau_p, ssa_p, g_p inconsistently sized"
      return
    end if
    if (any(shape(cloud_scaling) /= [ncol, nlay, this%get_ngpt()])) then
      error_msg = "sw_flux_scaled: cloud_scaling inconsistently sized"
      return
    end if
    if (any(shape(flux_up) /= [ncol, nlay + 1]) .or. any(shape(flux_dn) /= [ncol, nlay + 1])) then
      error_msg = "sw_flux_scaled: flux_up, flux_dn inconsistently sized"
      return
    end if
    scale_c = c_null_ptr; dir_c = c_null_ptr
    if (present(toa_scale)) then
      allocate(scale(ncol))
      scale = toa_scale
      if (ncol > 0) scale_c = c_loc(scale(1))
    end if
    if (present(flux_dir)) then
      allocate(dir(ncol, nlay + 1))
      if (size(dir) > 0) dir_c = c_loc(dir(1, 1))
    end if
    n = gas_desc%get_num_gases()
    allocate(up(ncol, nlay + 1), dn(ncol, nlay + 1))
    rc = c_sw_flux_scaled(this%handle, int(ncol, c_int), int(nlay, c_int), plev, tlay, int(n, c_int), names, ptr, cs, ls, scalar, &
                          merge(1_c_int, 0_c_int, top_at_1), mu0, scale_c, sfc_alb_dir, sfc_alb_dif, int(size(tau_p, 3), c_int), &
                          tau_p, ssa_p, g_p, ds, cloud_scaling, up, dn, dir_c, ECCKD_HOST, c_null_ptr)
    if (rc /= 0) then
      error_msg = c_error_message()
      return
    end if
    flux_up = up
    flux_dn = dn
    if (present(flux_dir)) flux_dir = dir
  end function sw_flux_scaled

  function c_loc_3d(a) result(p)
    real(wp), dimension(:,:,:), intent(in), target, contiguous :: a
    type(c_ptr) :: p
    p = c_loc(a(1, 1, 1))
  end function c_loc_3d

  function c_loc_2d(a) result(p)
    real(wp), dimension(:,:), intent(in), target, contiguous :: a
    type(c_ptr) :: p
    p = c_loc(a(1, 1))
  end function c_loc_2d

end module gas_optics_ecckd
