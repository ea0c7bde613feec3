! mo_aerosol_optics.F90 -- type(ty_aerosol_optics): RTE-RRTMGP's ty_aerosol_optics_rrtmgp_merra
! (extensions/aerosols/mo_aerosol_optics_rrtmgp_merra.F90) with the type-bound procedures and argument lists spelt there,
! but the arithmetic runs on an MI355X through the C ABI of librte_ecckd_hip.so (include/ecckd_hip.h, "Aerosol optics":
! the definition, operation by operation, is there).  This file contains NO numerics: every procedure marshals its
! arguments and calls the library.
!
!   load(band_lims_wvn, merra_aero_bin_lims, aero_rh, aero_dust_tbl, aero_salt_tbl, aero_sulf_tbl, aero_bcar_tbl,
!        aero_bcar_rh_tbl, aero_ocar_tbl, aero_ocar_rh_tbl [, device])
!   finalize(), get_nbin(), get_nrh()
!   aerosol_optics(aero_type, aero_size, aero_mass, relhum, optical_props [, accumulate])
!
! aero_type, aero_size, aero_mass are (ncol,nlay) -- RTE-RRTMGP's call -- or (ncol,nlay,nspec): several species summed in
! one call; relhum is (ncol,nlay).  accumulate = .true. adds the aerosol onto what optical_props holds (the clouds) with
! the arithmetic of increment.  The type extends ty_optical_props with one g-point per band, as RTE-RRTMGP's does, so
!       call stop_on_err(aerosols%alloc_2str(ncol, nlay, aerosol_optics))
! makes the (ncol,nlay,nband) planes the all-sky calls take as tau_p, ssa_p, g_p.  optical_props: ty_optical_props_1scl
! (the absorption optical depth) or ty_optical_props_2str (tau, ssa, g) with host allocatables -- every array is staged
! through the GPU -- or their device twins of mo_ecckd_device, whose planes stay in HBM (ECCKD_MIXED: only the inputs
! cross PCIe).  Parity with RTE-RRTMGP is unpinned (the library is not part of the reference tree).
module mo_aerosol_optics
  use, intrinsic :: iso_c_binding
  use mo_rte_kind, only: wp
  use mo_optical_props, only: ty_optical_props, ty_optical_props_arry, ty_optical_props_1scl, ty_optical_props_2str
  use mo_ecckd_device, only: ty_optical_props_1scl_dev, ty_optical_props_2str_dev, ECCKD_HOST, ECCKD_MIXED
  implicit none
  private

  integer, parameter, public :: merra_aero_none = 0, merra_aero_dust = 1, merra_aero_salt = 2, merra_aero_sulf = 3, &
                                merra_aero_bcar_rh = 4, merra_aero_bcar = 5, merra_aero_ocar_rh = 6, merra_aero_ocar = 7

  type, extends(ty_optical_props), public :: ty_aerosol_optics
    private
    type(c_ptr) :: handle = c_null_ptr
  contains
    procedure, public :: load
    procedure, public :: finalize
    generic, public :: aerosol_optics => aerosol_optics_2d, aerosol_optics_3d
    procedure, public :: aerosol_optics_2d
    procedure, public :: aerosol_optics_3d
    procedure, public :: get_nbin
    procedure, public :: get_nrh
  end type ty_aerosol_optics

  interface
    function c_create_lut(nband, nbin, nrh, bin_lims, rh_levels, dust, salt, sulf, bcar, bcar_rh, ocar, ocar_rh, device, handle) &
        bind(C, name="ecckd_aerosol_optics_create_lut") result(rc)
      import c_int, c_double, c_ptr
      integer(c_int), value :: nband, nbin, nrh, device
      real(c_double), dimension(*), intent(in) :: bin_lims, rh_levels, dust, salt, sulf, bcar, bcar_rh, ocar, ocar_rh
      type(c_ptr), intent(out) :: handle
      integer(c_int) :: rc
    end function c_create_lut
    subroutine c_destroy(handle) bind(C, name="ecckd_aerosol_optics_destroy")
      import c_ptr
      type(c_ptr), value :: handle
    end subroutine c_destroy
    pure function c_get_nbin(handle) bind(C, name="ecckd_aerosol_optics_get_nbin") result(n)
      import c_int, c_ptr
      type(c_ptr), value :: handle
      integer(c_int) :: n
    end function c_get_nbin
    pure function c_get_nrh(handle) bind(C, name="ecckd_aerosol_optics_get_nrh") result(n)
      import c_int, c_ptr
      type(c_ptr), value :: handle
      integer(c_int) :: n
    end function c_get_nrh
    function c_aerosol_optics(handle, ncol, nlay, nspec, aero_type, aero_size, aero_mass, relhum, accumulate, tau, ssa, g, &
                              memspace, stream) bind(C, name="ecckd_aerosol_optics") result(rc)
      import c_int, c_double, c_ptr
      type(c_ptr), value :: handle, stream
      integer(c_int), value :: ncol, nlay, nspec, accumulate, memspace
      integer(c_int), dimension(*), intent(in) :: aero_type
      real(c_double), dimension(*), intent(in) :: aero_size, aero_mass, relhum
      type(c_ptr), value :: tau, ssa, g                                      ! host (ECCKD_HOST) or device (ECCKD_MIXED)
      integer(c_int) :: rc
    end function c_aerosol_optics
    function c_last_error_ao() bind(C, name="ecckd_last_error") result(msg)
      import c_ptr
      type(c_ptr) :: msg
    end function c_last_error_ao
  end interface

contains

  function c_error_message() result(msg)
    character(len=128) :: msg
    character(kind=c_char), dimension(:), pointer :: p
    type(c_ptr) :: cp
    integer :: i
    msg = "ecckd: unknown error"
    cp = c_last_error_ao()
    if (.not. c_associated(cp)) return
    call c_f_pointer(cp, p, [128])
    msg = ""
    do i = 1, 128
      if (p(i) == c_null_char) exit
      msg(i:i) = p(i)
    end do
  end function c_error_message

  !> load, RTE-RRTMGP's argument list.  device: the GPU that keeps the tables (default 0).
  function load(this, band_lims_wvn, merra_aero_bin_lims, aero_rh, aero_dust_tbl, aero_salt_tbl, aero_sulf_tbl, aero_bcar_tbl, &
                aero_bcar_rh_tbl, aero_ocar_tbl, aero_ocar_rh_tbl, device) result(error_msg)
    class(ty_aerosol_optics), intent(inout) :: this
    real(wp), dimension(:,:), intent(in) :: band_lims_wvn          !< (2, nband)
    real(wp), dimension(:,:), intent(in) :: merra_aero_bin_lims    !< (2, nbin)
    real(wp), dimension(:), intent(in) :: aero_rh                  !< (nrh)
    real(wp), dimension(:,:,:), intent(in) :: aero_dust_tbl        !< (nval, nbin, nband)
    real(wp), dimension(:,:,:,:), intent(in) :: aero_salt_tbl      !< (nval, nrh, nbin, nband)
    real(wp), dimension(:,:,:), intent(in) :: aero_sulf_tbl, aero_bcar_rh_tbl, aero_ocar_rh_tbl   !< (nval, nrh, nband)
    real(wp), dimension(:,:), intent(in) :: aero_bcar_tbl, aero_ocar_tbl                          !< (nval, nband)
    integer, intent(in), optional :: device
    character(len=128) :: error_msg
    integer, dimension(:,:), allocatable :: band2gpt
    integer :: nband, nbin, nrh, dev, i
    integer(c_int) :: rc
    call this%finalize()
    nband = size(band_lims_wvn, 2)
    allocate(band2gpt(2, nband))
    do i = 1, nband
      band2gpt(:, i) = i                                           ! one g-point per band
    end do
    error_msg = this%init(band_lims_wvn, band2gpt)
    if (error_msg /= "") return
    nbin = size(merra_aero_bin_lims, 2)
    nrh = size(aero_rh)
    if (size(merra_aero_bin_lims, 1) /= 2 .or. any(shape(aero_dust_tbl) /= [3, nbin, nband]) .or. &
        any(shape(aero_salt_tbl) /= [3, nrh, nbin, nband]) .or. any(shape(aero_sulf_tbl) /= [3, nrh, nband]) .or. &
        any(shape(aero_bcar_rh_tbl) /= [3, nrh, nband]) .or. any(shape(aero_ocar_rh_tbl) /= [3, nrh, nband]) .or. &
        any(shape(aero_bcar_tbl) /= [3, nband]) .or. any(shape(aero_ocar_tbl) /= [3, nband])) then
      error_msg = "aerosol_optics%load(): arrays sized inconsistently"
      return
    end if
    dev = 0
    if (present(device)) dev = device
    rc = c_create_lut(int(nband, c_int), int(nbin, c_int), int(nrh, c_int), merra_aero_bin_lims, aero_rh, aero_dust_tbl, &
                      aero_salt_tbl, aero_sulf_tbl, aero_bcar_tbl, aero_bcar_rh_tbl, aero_ocar_tbl, aero_ocar_rh_tbl, &
                      int(dev, c_int), this%handle)
    if (rc /= 0) then
      this%handle = c_null_ptr
      error_msg = c_error_message()
    end if
  end function load

  subroutine finalize(this)
    class(ty_aerosol_optics), intent(inout) :: this
    if (c_associated(this%handle)) call c_destroy(this%handle)
    this%handle = c_null_ptr
  end subroutine finalize

  function get_nbin(this) result(n)
    class(ty_aerosol_optics), intent(in) :: this
    integer :: n
    n = 0
    if (c_associated(this%handle)) n = int(c_get_nbin(this%handle))
  end function get_nbin

  function get_nrh(this) result(n)
    class(ty_aerosol_optics), intent(in) :: this
    integer :: n
    n = 0
    if (c_associated(this%handle)) n = int(c_get_nrh(this%handle))
  end function get_nrh

  !> aerosol_optics(aero_type, aero_size, aero_mass, relhum, optical_props): RTE-RRTMGP's call, one species per cell
  function aerosol_optics_2d(this, aero_type, aero_size, aero_mass, relhum, optical_props, accumulate) result(error_msg)
    class(ty_aerosol_optics), intent(in) :: this
    integer, dimension(:,:), intent(in) :: aero_type               !< (ncol, nlay), the merra_aero_* codes
    real(wp), dimension(:,:), intent(in) :: aero_size, aero_mass   !< microns, kg m-2
    real(wp), dimension(:,:), intent(in) :: relhum                 !< fraction
    class(ty_optical_props_arry), intent(inout), target :: optical_props
    logical, intent(in), optional :: accumulate
    character(len=128) :: error_msg
    error_msg = this%aerosol_optics_3d(reshape(aero_type, [size(aero_type, 1), size(aero_type, 2), 1]), &
                                       reshape(aero_size, [size(aero_size, 1), size(aero_size, 2), 1]), &
                                       reshape(aero_mass, [size(aero_mass, 1), size(aero_mass, 2), 1]), relhum, optical_props, &
                                       accumulate)
  end function aerosol_optics_2d

  !> the same with (ncol, nlay, nspec) species arrays: the species are summed in one call
  function aerosol_optics_3d(this, aero_type, aero_size, aero_mass, relhum, optical_props, accumulate) result(error_msg)
    class(ty_aerosol_optics), intent(in) :: this
    integer, dimension(:,:,:), intent(in) :: aero_type
    real(wp), dimension(:,:,:), intent(in) :: aero_size, aero_mass
    real(wp), dimension(:,:), intent(in) :: relhum
    class(ty_optical_props_arry), intent(inout), target :: optical_props
    logical, intent(in), optional :: accumulate
    character(len=128) :: error_msg
    type(c_ptr) :: tau, ssa, g
    integer(c_int) :: memspace, rc, acc
    integer(c_int), dimension(:,:,:), allocatable :: kinds
    integer :: ncol, nlay, nspec, nband
    error_msg = ""
    if (.not. c_associated(this%handle)) then
      error_msg = "aerosol_optics%aerosol_optics(): the tables have not been loaded"
      return
    end if
    ncol = size(aero_type, 1)
    nlay = size(aero_type, 2)
    nspec = size(aero_type, 3)
    nband = this%get_nband()
    if (any(shape(aero_size) /= shape(aero_type)) .or. any(shape(aero_mass) /= shape(aero_type)) .or. &
        any(shape(relhum) /= [ncol, nlay])) then
      error_msg = "aerosol optics: input arrays sized inconsistently"
      return
    end if
    if (optical_props%get_nband() /= nband .or. optical_props%get_ngpt() /= nband) then
      error_msg = "aerosol optics: optical properties are not on the bands of the tables"
      return
    end if
    tau = c_null_ptr
    ssa = c_null_ptr
    g = c_null_ptr
    memspace = ECCKD_HOST
    select type (optical_props)
    type is (ty_optical_props_1scl_dev)
      if (optical_props%ncol /= ncol .or. optical_props%nlay /= nlay) error_msg = "aerosol optics: optical_props sized inconsistently"
      tau = optical_props%d_tau
      memspace = ECCKD_MIXED
    type is (ty_optical_props_2str_dev)
      if (optical_props%ncol /= ncol .or. optical_props%nlay /= nlay) error_msg = "aerosol optics: optical_props sized inconsistently"
      tau = optical_props%d_tau
      ssa = optical_props%d_ssa
      g = optical_props%d_g
      memspace = ECCKD_MIXED
    class is (ty_optical_props_1scl)
      if (.not. allocated(optical_props%tau)) then
        error_msg = "aerosol optics: optical_props is not allocated"
      else if (size(optical_props%tau, 1) /= ncol .or. size(optical_props%tau, 2) /= nlay) then
        error_msg = "aerosol optics: optical_props sized inconsistently"
      else if (size(optical_props%tau) > 0) then
        tau = c_loc(optical_props%tau(1, 1, 1))
      end if
    class is (ty_optical_props_2str)
      if (.not. allocated(optical_props%tau)) then
        error_msg = "aerosol optics: optical_props is not allocated"
      else if (size(optical_props%tau, 1) /= ncol .or. size(optical_props%tau, 2) /= nlay) then
        error_msg = "aerosol optics: optical_props sized inconsistently"
      else if (size(optical_props%tau) > 0) then
        tau = c_loc(optical_props%tau(1, 1, 1))
        ssa = c_loc(optical_props%ssa(1, 1, 1))
        g = c_loc(optical_props%g(1, 1, 1))
      end if
    class default
      error_msg = "aerosol optics: optical_props must be ty_optical_props_1scl or ty_optical_props_2str"
    end select
    if (error_msg /= "") return
    if (ncol == 0) return
    acc = 0
    if (present(accumulate)) then
      if (accumulate) acc = 1
    end if
    allocate(kinds(ncol, nlay, nspec))
    kinds = int(aero_type, c_int)
    rc = c_aerosol_optics(this%handle, int(ncol, c_int), int(nlay, c_int), int(nspec, c_int), kinds, aero_size, aero_mass, relhum, &
                          acc, tau, ssa, g, memspace, c_null_ptr)
    if (rc /= 0) error_msg = c_error_message()
  end function aerosol_optics_3d

end module mo_aerosol_optics
