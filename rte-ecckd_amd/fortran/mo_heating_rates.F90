! mo_heating_rates.F90 -- compute_heating_rate of RTE-RRTMGP (extensions/mo_heating_rates.F90) with its argument order,
! but the arithmetic runs on an MI355X through the C ABI of librte_ecckd_hip.so (include/ecckd_hip.h, "Heating rates":
! the definition, operation by operation, is there).  This file contains NO numerics: every procedure marshals its
! arguments and calls the library.
!
!   error_msg = compute_heating_rate(flux_up, flux_dn, plev, heating_rate [, cp] [, grav] [, cp_dry] [, device])
!
! Generic over the rank of the fluxes -- (ncol,nlay+1) broadband, or (ncol,nlay+1,nouter): the bnd_flux_* arrays of
! ty_fluxes_byband, or any stack of flux sets -- and over where the result lives:
!   heating_rate a host array (ncol,nlay) / (ncol,nlay,nouter): every array is staged through the GPU (ECCKD_HOST);
!   heating_rate a type(ty_heating_rate_dev): the result stays in HBM (ECCKD_MIXED: only the inputs cross PCIe) until
!     copy_to_host() fills its host member, as the device twins of mo_ecckd_device do.
! plev is (ncol,nlay+1) and shared by every plane; for shortwave flux_dn is the total, direct beam included.  cp
! (ncol,nlay) is the host model's own specific heat per cell and replaces cp_dry.  grav and cp_dry default to the customary
! 9.80665 m s-2 and 1004.64 J kg-1 K-1; they are arguments of every call, not state.  There is no top_at_1: the expression
! does not depend on the orientation.  Parity with RTE-RRTMGP is unpinned (the library is not part of the reference tree).
module mo_heating_rates
  use, intrinsic :: iso_c_binding
  use mo_rte_kind, only: wp
  use mo_ecckd_device, only: ECCKD_HOST, ECCKD_MIXED
  implicit none
  private

  real(wp), parameter, public :: grav_default = 9.80665_wp, cp_dry_default = 1004.64_wp

  !> heating_rate(ncol,nlay,nouter) in device memory (nouter = 1: broadband)
  type, public :: ty_heating_rate_dev
    type(c_ptr) :: d_heating_rate = c_null_ptr
    integer :: ncol = 0, nlay = 0, nouter = 0, device = 0
    real(wp), dimension(:,:,:), allocatable :: heating_rate   !< host copy, filled by copy_to_host()
  contains
    procedure, public :: alloc => alloc_dev
    procedure, public :: free => free_dev
    procedure, public :: copy_to_host
  end type ty_heating_rate_dev

  interface compute_heating_rate
    module procedure compute_heating_rate_2d, compute_heating_rate_3d, compute_heating_rate_dev_2d, compute_heating_rate_dev_3d
  end interface compute_heating_rate
  public :: compute_heating_rate

  interface
    function c_heating_rate(device, ncol, nlay, nouter, flux_up, flux_dn, plev, grav, cp_dry, cp, heating_rate, memspace, &
                            stream) bind(C, name="ecckd_heating_rate") result(rc)
      import c_int, c_double, c_ptr
      integer(c_int), value :: device, ncol, nlay, nouter, memspace
      type(c_ptr), value :: flux_up, flux_dn, plev, cp                       ! host; cp may be null
      real(c_double), value :: grav, cp_dry
      type(c_ptr), value :: heating_rate, stream                             ! host (ECCKD_HOST) or device (ECCKD_MIXED)
      integer(c_int) :: rc
    end function c_heating_rate
    function c_hr_malloc(device, bytes, ptr) bind(C, name="ecckd_device_malloc") result(rc)
      import c_int, c_size_t, c_ptr
      integer(c_int), value :: device
      integer(c_size_t), value :: bytes
      type(c_ptr), intent(out) :: ptr
      integer(c_int) :: rc
    end function c_hr_malloc
    function c_hr_free(device, ptr) bind(C, name="ecckd_device_free") result(rc)
      import c_int, c_ptr
      integer(c_int), value :: device
      type(c_ptr), value :: ptr
      integer(c_int) :: rc
    end function c_hr_free
    function c_hr_memcpy(device, dst, src, bytes, to_device) bind(C, name="ecckd_device_memcpy") result(rc)
      import c_int, c_size_t, c_ptr
      integer(c_int), value :: device, to_device
      type(c_ptr), value :: dst, src
      integer(c_size_t), value :: bytes
      integer(c_int) :: rc
    end function c_hr_memcpy
    function c_last_error_hr() bind(C, name="ecckd_last_error") result(msg)
      import c_ptr
      type(c_ptr) :: msg
    end function c_last_error_hr
  end interface

contains

  function c_error_message() result(msg)
    character(len=128) :: msg
    character(kind=c_char), dimension(:), pointer :: p
    type(c_ptr) :: cp
    integer :: i
    msg = "ecckd: unknown error"
    cp = c_last_error_hr()
    if (.not. c_associated(cp)) return
    call c_f_pointer(cp, p, [128])
    msg = ""
    do i = 1, 128
      if (p(i) == c_null_char) exit
      msg(i:i) = p(i)
    end do
  end function c_error_message

  ! ---- ty_heating_rate_dev ----
  function alloc_dev(this, ncol, nlay, nouter, device) result(error_msg)
    class(ty_heating_rate_dev), intent(inout) :: this
    integer, intent(in) :: ncol, nlay
    integer, intent(in), optional :: nouter, device
    character(len=128) :: error_msg
    error_msg = ""
    call this%free()
    this%ncol = ncol
    this%nlay = nlay
    this%nouter = 1
    if (present(nouter)) this%nouter = nouter
    this%device = 0
    if (present(device)) this%device = device
    if (c_hr_malloc(int(this%device, c_int), int(ncol, c_size_t) * nlay * this%nouter * c_sizeof(1._wp), &
                    this%d_heating_rate) /= 0) then
      this%d_heating_rate = c_null_ptr
      error_msg = c_error_message()
    end if
  end function alloc_dev

  subroutine free_dev(this)
    class(ty_heating_rate_dev), intent(inout) :: this
    integer(c_int) :: rc
    if (c_associated(this%d_heating_rate)) rc = c_hr_free(int(this%device, c_int), this%d_heating_rate)
    this%d_heating_rate = c_null_ptr
  end subroutine free_dev

  function copy_to_host(this) result(error_msg)
    class(ty_heating_rate_dev), intent(inout), target :: this
    character(len=128) :: error_msg
    error_msg = ""
    if (.not. c_associated(this%d_heating_rate)) then
      error_msg = "heating_rate%copy_to_host(): not allocated"
      return
    end if
    if (allocated(this%heating_rate)) deallocate(this%heating_rate)
    allocate(this%heating_rate(this%ncol, this%nlay, this%nouter))
    if (c_hr_memcpy(int(this%device, c_int), c_loc(this%heating_rate), this%d_heating_rate, &
                    size(this%heating_rate, kind=c_size_t) * c_sizeof(1._wp), 0_c_int) /= 0) error_msg = c_error_message()
  end function copy_to_host

  ! ---- the call: explicit shapes, so every array is contiguous here whatever section the caller passed ----
  function heating_rate_call(ncol, nlay, nouter, flux_up, flux_dn, plev, out, memspace, device, cp, grav, cp_dry) &
      result(error_msg)
    integer, intent(in) :: ncol, nlay, nouter, device
    real(wp), dimension(ncol, nlay + 1, nouter), intent(in), target :: flux_up, flux_dn
    real(wp), dimension(ncol, nlay + 1), intent(in), target :: plev
    type(c_ptr), intent(in) :: out
    integer(c_int), intent(in) :: memspace
    real(wp), dimension(ncol, nlay), intent(in), target, optional :: cp
    real(wp), intent(in), optional :: grav, cp_dry
    character(len=128) :: error_msg
    type(c_ptr) :: cp_ptr
    real(c_double) :: g, c
    error_msg = ""
    g = real(grav_default, c_double)
    if (present(grav)) g = real(grav, c_double)
    c = real(cp_dry_default, c_double)
    if (present(cp_dry)) c = real(cp_dry, c_double)
    cp_ptr = c_null_ptr
    if (present(cp)) cp_ptr = c_loc(cp)
    if (c_heating_rate(int(device, c_int), int(ncol, c_int), int(nlay, c_int), int(nouter, c_int), c_loc(flux_up), &
                       c_loc(flux_dn), c_loc(plev), g, c, cp_ptr, out, memspace, c_null_ptr) /= 0) error_msg = c_error_message()
  end function heating_rate_call

  ! shapes of the inputs against (ncol, nlay+1 [, nouter]) taken from flux_up
  function check_shapes(ncol, nlev, shape_dn, shape_plev, cp_present, shape_cp) result(error_msg)
    integer, intent(in) :: ncol, nlev
    integer, dimension(2), intent(in) :: shape_dn, shape_plev, shape_cp
    logical, intent(in) :: cp_present
    character(len=128) :: error_msg
    error_msg = ""
    if (ncol < 1 .or. nlev < 2) then
      error_msg = "compute_heating_rate: fluxes need at least one column and two levels"
    else if (any(shape_dn /= [ncol, nlev]) .or. any(shape_plev /= [ncol, nlev])) then
      error_msg = "compute_heating_rate: flux_up, flux_dn and plev sized inconsistently"
    else if (cp_present) then
      if (any(shape_cp /= [ncol, nlev - 1])) error_msg = "compute_heating_rate: cp must be (ncol, nlay)"
    end if
  end function check_shapes

  !> broadband, host arrays
  function compute_heating_rate_2d(flux_up, flux_dn, plev, heating_rate, cp, grav, cp_dry, device) result(error_msg)
    real(wp), dimension(:,:), intent(in) :: flux_up, flux_dn, plev   !< (ncol, nlay+1)
    real(wp), dimension(:,:), intent(out), target, contiguous :: heating_rate   !< (ncol, nlay), K s-1
    real(wp), dimension(:,:), intent(in), optional :: cp             !< (ncol, nlay)
    real(wp), intent(in), optional :: grav, cp_dry
    integer, intent(in), optional :: device
    character(len=128) :: error_msg
    integer :: ncol, nlev, dev
    integer, dimension(2) :: shape_cp
    ncol = size(flux_up, 1)
    nlev = size(flux_up, 2)
    shape_cp = 0
    if (present(cp)) shape_cp = shape(cp)
    error_msg = check_shapes(ncol, nlev, shape(flux_dn), shape(plev), present(cp), shape_cp)
    if (error_msg /= "") return
    if (any(shape(heating_rate) /= [ncol, nlev - 1])) then
      error_msg = "compute_heating_rate: heating_rate must be (ncol, nlay)"
      return
    end if
    dev = 0
    if (present(device)) dev = device
    error_msg = heating_rate_call(ncol, nlev - 1, 1, flux_up, flux_dn, plev, c_loc(heating_rate), ECCKD_HOST, dev, cp, grav, &
                                  cp_dry)
  end function compute_heating_rate_2d

  !> by band (or any stack of flux sets), host arrays
  function compute_heating_rate_3d(flux_up, flux_dn, plev, heating_rate, cp, grav, cp_dry, device) result(error_msg)
    real(wp), dimension(:,:,:), intent(in) :: flux_up, flux_dn       !< (ncol, nlay+1, nouter)
    real(wp), dimension(:,:), intent(in) :: plev                     !< (ncol, nlay+1)
    real(wp), dimension(:,:,:), intent(out), target, contiguous :: heating_rate   !< (ncol, nlay, nouter), K s-1
    real(wp), dimension(:,:), intent(in), optional :: cp             !< (ncol, nlay)
    real(wp), intent(in), optional :: grav, cp_dry
    integer, intent(in), optional :: device
    character(len=128) :: error_msg
    integer :: ncol, nlev, nouter, dev
    integer, dimension(2) :: shape_cp
    ncol = size(flux_up, 1)
    nlev = size(flux_up, 2)
    nouter = size(flux_up, 3)
    shape_cp = 0
    if (present(cp)) shape_cp = shape(cp)
    error_msg = check_shapes(ncol, nlev, [size(flux_dn, 1), size(flux_dn, 2)], shape(plev), present(cp), shape_cp)
    if (error_msg == "" .and. (nouter < 1 .or. size(flux_dn, 3) /= nouter)) &
      error_msg = "compute_heating_rate: flux_up, flux_dn and plev sized inconsistently"
    if (error_msg /= "") return
    if (any(shape(heating_rate) /= [ncol, nlev - 1, nouter])) then
      error_msg = "compute_heating_rate: heating_rate must be (ncol, nlay, nouter)"
      return
    end if
    dev = 0
    if (present(device)) dev = device
    error_msg = heating_rate_call(ncol, nlev - 1, nouter, flux_up, flux_dn, plev, c_loc(heating_rate), ECCKD_HOST, dev, cp, &
                                  grav, cp_dry)
  end function compute_heating_rate_3d

  !> broadband, the result in a device container (alloc(ncol, nlay))
  function compute_heating_rate_dev_2d(flux_up, flux_dn, plev, heating_rate, cp, grav, cp_dry) result(error_msg)
    real(wp), dimension(:,:), intent(in) :: flux_up, flux_dn, plev   !< (ncol, nlay+1)
    type(ty_heating_rate_dev), intent(inout) :: heating_rate
    real(wp), dimension(:,:), intent(in), optional :: cp             !< (ncol, nlay)
    real(wp), intent(in), optional :: grav, cp_dry
    character(len=128) :: error_msg
    integer :: ncol, nlev
    integer, dimension(2) :: shape_cp
    ncol = size(flux_up, 1)
    nlev = size(flux_up, 2)
    shape_cp = 0
    if (present(cp)) shape_cp = shape(cp)
    error_msg = check_shapes(ncol, nlev, shape(flux_dn), shape(plev), present(cp), shape_cp)
    if (error_msg /= "") return
    if (.not. c_associated(heating_rate%d_heating_rate) .or. heating_rate%ncol /= ncol .or. heating_rate%nlay /= nlev - 1 .or. &
        heating_rate%nouter /= 1) then
      error_msg = "compute_heating_rate: heating_rate is not allocated as (ncol, nlay)"
      return
    end if
    error_msg = heating_rate_call(ncol, nlev - 1, 1, flux_up, flux_dn, plev, heating_rate%d_heating_rate, ECCKD_MIXED, &
                                  heating_rate%device, cp, grav, cp_dry)
  end function compute_heating_rate_dev_2d

  !> by band (or any stack of flux sets), the result in a device container (alloc(ncol, nlay, nouter))
  function compute_heating_rate_dev_3d(flux_up, flux_dn, plev, heating_rate, cp, grav, cp_dry) result(error_msg)
    real(wp), dimension(:,:,:), intent(in) :: flux_up, flux_dn       !< (ncol, nlay+1, nouter)
    real(wp), dimension(:,:), intent(in) :: plev                     !< (ncol, nlay+1)
    type(ty_heating_rate_dev), intent(inout) :: heating_rate
    real(wp), dimension(:,:), intent(in), optional :: cp             !< (ncol, nlay)
    real(wp), intent(in), optional :: grav, cp_dry
    character(len=128) :: error_msg
    integer :: ncol, nlev, nouter
    integer, dimension(2) :: shape_cp
    ncol = size(flux_up, 1)
    nlev = size(flux_up, 2)
    nouter = size(flux_up, 3)
    shape_cp = 0
    if (present(cp)) shape_cp = shape(cp)
    error_msg = check_shapes(ncol, nlev, [size(flux_dn, 1), size(flux_dn, 2)], shape(plev), present(cp), shape_cp)
    if (error_msg == "" .and. (nouter < 1 .or. size(flux_dn, 3) /= nouter)) &
      error_msg = "compute_heating_rate: flux_up, flux_dn and plev sized inconsistently"
    if (error_msg /= "") return
    if (.not. c_associated(heating_rate%d_heating_rate) .or. heating_rate%ncol /= ncol .or. heating_rate%nlay /= nlev - 1 .or. &
        heating_rate%nouter /= nouter) then
      error_msg = "compute_heating_rate: heating_rate is not allocated as (ncol, nlay, nouter)"
      return
    end if
    error_msg = heating_rate_call(ncol, nlev - 1, nouter, flux_up, flux_dn, plev, heating_rate%d_heating_rate, ECCKD_MIXED, &
                                  heating_rate%device, cp, grav, cp_dry)
  end function compute_heating_rate_dev_3d

end module mo_heating_rates
