! mo_cloud_optics.F90 -- type(ty_cloud_optics) of RTE-RRTMGP (extensions/cloud_optics/mo_cloud_optics.F90), look-up-table
! form, with the type-bound procedures and argument lists spelt there, but the arithmetic runs on an MI355X through the C
! ABI of librte_ecckd_hip.so (include/ecckd_hip.h, "Cloud optics": the definition, operation by operation, is there).
! This file contains NO numerics: every procedure marshals its arguments and calls the library.
!
!   load(band_lims_wvn, radliq_lwr, radliq_upr, radliq_fac, radice_lwr, radice_upr, radice_fac,
!        lut_extliq, lut_ssaliq, lut_asyliq, lut_extice, lut_ssaice, lut_asyice [, device])     the LUT form
!   finalize(), set_ice_roughness(icergh), get_num_ice_roughness_types(),
!   get_min_radius_liq() / get_max_radius_liq() / get_min_radius_ice() / get_max_radius_ice()
!   cloud_optics(clwp, ciwp, reliq, reice, optical_props)
!
! The type extends ty_optical_props with one g-point per band, as RTE-RRTMGP's does, so
!       call stop_on_err(clouds%alloc_2str(ncol, nlay, cloud_optics))
! makes the (ncol,nlay,nband) planes the all-sky calls take as tau_p, ssa_p, g_p.  optical_props: ty_optical_props_1scl
! (the absorption optical depth) or ty_optical_props_2str (tau, ssa, g) with host allocatables -- every array is staged
! through the GPU -- or their device twins of mo_ecckd_device, whose planes stay in HBM (ECCKD_MIXED: only the four
! (ncol,nlay) inputs cross PCIe).  The ice roughness is held here and passed with every call: per-call state is explicit
! in the C ABI.  The Pade form of RTE-RRTMGP's type is not provided.  Parity with RTE-RRTMGP is unpinned (the library is
! not part of the reference tree).
module mo_cloud_optics
  use, intrinsic :: iso_c_binding
  use mo_rte_kind, only: wp
  use mo_optical_props, only: ty_optical_props, ty_optical_props_arry, ty_optical_props_1scl, ty_optical_props_2str
  use mo_ecckd_device, only: ty_optical_props_1scl_dev, ty_optical_props_2str_dev, ECCKD_HOST, ECCKD_MIXED
  implicit none
  private

  type, extends(ty_optical_props), public :: ty_cloud_optics
    private
    type(c_ptr) :: handle = c_null_ptr
    integer :: icergh = 0
  contains
    generic, public :: load => load_lut
    procedure, public :: load_lut
    procedure, public :: finalize
    procedure, public :: cloud_optics
    procedure, public :: set_ice_roughness
    procedure, public :: get_num_ice_roughness_types
    procedure, public :: get_min_radius_liq
    procedure, public :: get_max_radius_liq
    procedure, public :: get_min_radius_ice
    procedure, public :: get_max_radius_ice
  end type ty_cloud_optics

  interface
    function c_create_lut(nband, nsize_liq, nsize_ice, nrghice, radliq_lwr, radliq_upr, radice_lwr, radice_upr, extliq, ssaliq, &
                          asyliq, extice, ssaice, asyice, device, handle) bind(C, name="ecckd_cloud_optics_create_lut") result(rc)
      import c_int, c_double, c_ptr
      integer(c_int), value :: nband, nsize_liq, nsize_ice, nrghice, device
      real(c_double), value :: radliq_lwr, radliq_upr, radice_lwr, radice_upr
      real(c_double), dimension(*), intent(in) :: extliq, ssaliq, asyliq, extice, ssaice, asyice
      type(c_ptr), intent(out) :: handle
      integer(c_int) :: rc
    end function c_create_lut
    subroutine c_destroy(handle) bind(C, name="ecckd_cloud_optics_destroy")
      import c_ptr
      type(c_ptr), value :: handle
    end subroutine c_destroy
    pure function c_get_nrghice(handle) bind(C, name="ecckd_cloud_optics_get_nrghice") result(n)
      import c_int, c_ptr
      type(c_ptr), value :: handle
      integer(c_int) :: n
    end function c_get_nrghice
    pure function c_min_radius_liq(handle) bind(C, name="ecckd_cloud_optics_get_min_radius_liq") result(v)
      import c_double, c_ptr
      type(c_ptr), value :: handle
      real(c_double) :: v
    end function c_min_radius_liq
    pure function c_max_radius_liq(handle) bind(C, name="ecckd_cloud_optics_get_max_radius_liq") result(v)
      import c_double, c_ptr
      type(c_ptr), value :: handle
      real(c_double) :: v
    end function c_max_radius_liq
    pure function c_min_radius_ice(handle) bind(C, name="ecckd_cloud_optics_get_min_radius_ice") result(v)
      import c_double, c_ptr
      type(c_ptr), value :: handle
      real(c_double) :: v
    end function c_min_radius_ice
    pure function c_max_radius_ice(handle) bind(C, name="ecckd_cloud_optics_get_max_radius_ice") result(v)
      import c_double, c_ptr
      type(c_ptr), value :: handle
      real(c_double) :: v
    end function c_max_radius_ice
    function c_cloud_optics(handle, ncol, nlay, clwp, ciwp, reliq, reice, icergh, tau, ssa, g, memspace, stream) &
        bind(C, name="ecckd_cloud_optics") result(rc)
      import c_int, c_double, c_ptr
      type(c_ptr), value :: handle, stream
      integer(c_int), value :: ncol, nlay, icergh, memspace
      real(c_double), dimension(*), intent(in) :: clwp, ciwp, reliq, reice
      type(c_ptr), value :: tau, ssa, g                                      ! host (ECCKD_HOST) or device (ECCKD_MIXED)
      integer(c_int) :: rc
    end function c_cloud_optics
    function c_last_error_co() bind(C, name="ecckd_last_error") result(msg)
      import c_ptr
      type(c_ptr) :: msg
    end function c_last_error_co
  end interface

contains

  function c_error_message() result(msg)
    character(len=128) :: msg
    character(kind=c_char), dimension(:), pointer :: p
    type(c_ptr) :: cp
    integer :: i
    msg = "ecckd: unknown error"
    cp = c_last_error_co()
    if (.not. c_associated(cp)) return
    call c_f_pointer(cp, p, [128])
    msg = ""
    do i = 1, 128
      if (p(i) == c_null_char) exit
      msg(i:i) = p(i)
    end do
  end function c_error_message

  !> load (LUT form), RTE-RRTMGP's argument list; radliq_fac / radice_fac are accepted and unused, as there.  device: the
  !! GPU that keeps the tables (default 0).
  function load_lut(this, band_lims_wvn, radliq_lwr, radliq_upr, radliq_fac, radice_lwr, radice_upr, radice_fac, &
                    lut_extliq, lut_ssaliq, lut_asyliq, lut_extice, lut_ssaice, lut_asyice, device) result(error_msg)
    class(ty_cloud_optics), intent(inout) :: this
    real(wp), dimension(:,:), intent(in) :: band_lims_wvn          !< (2, nband)
    real(wp), intent(in) :: radliq_lwr, radliq_upr, radliq_fac, radice_lwr, radice_upr, radice_fac
    real(wp), dimension(:,:), intent(in) :: lut_extliq, lut_ssaliq, lut_asyliq       !< (nsize_liq, nband)
    real(wp), dimension(:,:,:), intent(in) :: lut_extice, lut_ssaice, lut_asyice     !< (nsize_ice, nband, nrghice)
    integer, intent(in), optional :: device
    character(len=128) :: error_msg
    integer, dimension(:,:), allocatable :: band2gpt
    integer :: nband, nsize_liq, nsize_ice, nrghice, dev, i
    integer(c_int) :: rc
    call this%finalize()
    nband = size(band_lims_wvn, 2)
    error_msg = ""
    allocate(band2gpt(2, nband))
    do i = 1, nband
      band2gpt(:, i) = i                                           ! one g-point per band
    end do
    error_msg = this%init(band_lims_wvn, band2gpt)
    if (error_msg /= "") return
    nsize_liq = size(lut_extliq, 1)
    nsize_ice = size(lut_extice, 1)
    nrghice = size(lut_extice, 3)
    if (size(lut_extliq, 2) /= nband .or. any(shape(lut_ssaliq) /= shape(lut_extliq)) .or. &
        any(shape(lut_asyliq) /= shape(lut_extliq)) .or. size(lut_extice, 2) /= nband .or. &
        any(shape(lut_ssaice) /= shape(lut_extice)) .or. any(shape(lut_asyice) /= shape(lut_extice))) then
      error_msg = "cloud_optics%init(): arrays sized inconsistently"
      return
    end if
    dev = 0
    if (present(device)) dev = device
    rc = c_create_lut(int(nband, c_int), int(nsize_liq, c_int), int(nsize_ice, c_int), int(nrghice, c_int), radliq_lwr, &
                      radliq_upr, radice_lwr, radice_upr, lut_extliq, lut_ssaliq, lut_asyliq, lut_extice, lut_ssaice, &
                      lut_asyice, int(dev, c_int), this%handle)
    if (rc /= 0) then
      this%handle = c_null_ptr
      error_msg = c_error_message()
      return
    end if
    this%icergh = 1
  end function load_lut

  subroutine finalize(this)
    class(ty_cloud_optics), intent(inout) :: this
    if (c_associated(this%handle)) call c_destroy(this%handle)
    this%handle = c_null_ptr
    this%icergh = 0
  end subroutine finalize

  function set_ice_roughness(this, icergh) result(error_msg)
    class(ty_cloud_optics), intent(inout) :: this
    integer, intent(in) :: icergh
    character(len=128) :: error_msg
    error_msg = ""
    if (.not. c_associated(this%handle)) then
      error_msg = "cloud_optics%set_ice_roughness(): can't set before initialization"
    else if (icergh < 1 .or. icergh > this%get_num_ice_roughness_types()) then
      error_msg = "cloud_optics%set_ice_roughness(): must be > 0 and <= nrghice"
    else
      this%icergh = icergh
    end if
  end function set_ice_roughness

  function get_num_ice_roughness_types(this) result(n)
    class(ty_cloud_optics), intent(in) :: this
    integer :: n
    n = 0
    if (c_associated(this%handle)) n = int(c_get_nrghice(this%handle))
  end function get_num_ice_roughness_types

  function get_min_radius_liq(this) result(r)
    class(ty_cloud_optics), intent(in) :: this
    real(wp) :: r
    r = real(c_min_radius_liq(this%handle), wp)
  end function get_min_radius_liq

  function get_max_radius_liq(this) result(r)
    class(ty_cloud_optics), intent(in) :: this
    real(wp) :: r
    r = real(c_max_radius_liq(this%handle), wp)
  end function get_max_radius_liq

  function get_min_radius_ice(this) result(r)
    class(ty_cloud_optics), intent(in) :: this
    real(wp) :: r
    r = real(c_min_radius_ice(this%handle), wp)
  end function get_min_radius_ice

  function get_max_radius_ice(this) result(r)
    class(ty_cloud_optics), intent(in) :: this
    real(wp) :: r
    r = real(c_max_radius_ice(this%handle), wp)
  end function get_max_radius_ice

  !> cloud_optics(clwp, ciwp, reliq, reice, optical_props): water paths (g m-2) and effective radii (microns), (ncol,nlay),
  !! to optical_props on the bands (alloc_1scl / alloc_2str with this object as the spectral description).
  function cloud_optics(this, clwp, ciwp, reliq, reice, optical_props) result(error_msg)
    class(ty_cloud_optics), intent(in) :: this
    real(wp), dimension(:,:), intent(in) :: clwp, ciwp, reliq, reice
    class(ty_optical_props_arry), intent(inout), target :: optical_props
    character(len=128) :: error_msg
    type(c_ptr) :: tau, ssa, g
    integer(c_int) :: memspace, rc
    integer :: ncol, nlay, nband
    error_msg = ""
    if (.not. c_associated(this%handle)) then
      error_msg = "cloud_optics%cloud_optics(): the tables have not been loaded"
      return
    end if
    ncol = size(clwp, 1)
    nlay = size(clwp, 2)
    nband = this%get_nband()
    if (any(shape(ciwp) /= shape(clwp)) .or. any(shape(reliq) /= shape(clwp)) .or. any(shape(reice) /= shape(clwp))) then
      error_msg = "cloud optics: input arrays sized inconsistently"
      return
    end if
    if (optical_props%get_nband() /= nband .or. optical_props%get_ngpt() /= nband) then
      error_msg = "cloud optics: optical properties are not on the bands of the tables"
      return
    end if
    tau = c_null_ptr
    ssa = c_null_ptr
    g = c_null_ptr
    memspace = ECCKD_HOST
    select type (optical_props)
    type is (ty_optical_props_1scl_dev)
      if (optical_props%ncol /= ncol .or. optical_props%nlay /= nlay) error_msg = "cloud optics: optical_props sized inconsistently"
      tau = optical_props%d_tau
      memspace = ECCKD_MIXED
    type is (ty_optical_props_2str_dev)
      if (optical_props%ncol /= ncol .or. optical_props%nlay /= nlay) error_msg = "cloud optics: optical_props sized inconsistently"
      tau = optical_props%d_tau
      ssa = optical_props%d_ssa
      g = optical_props%d_g
      memspace = ECCKD_MIXED
    class is (ty_optical_props_1scl)
      if (.not. allocated(optical_props%tau)) then
        error_msg = "cloud optics: optical_props is not allocated"
      else if (size(optical_props%tau, 1) /= ncol .or. size(optical_props%tau, 2) /= nlay) then
        error_msg = "cloud optics: optical_props sized inconsistently"
      else if (size(optical_props%tau) > 0) then
        tau = c_loc(optical_props%tau(1, 1, 1))
      end if
    class is (ty_optical_props_2str)
      if (.not. allocated(optical_props%tau)) then
        error_msg = "cloud optics: optical_props is not allocated"
      else if (size(optical_props%tau, 1) /= ncol .or. size(optical_props%tau, 2) /= nlay) then
        error_msg = "cloud optics: optical_props sized inconsistently"
      else if (size(optical_props%tau) > 0) then
        tau = c_loc(optical_props%tau(1, 1, 1))
        ssa = c_loc(optical_props%ssa(1, 1, 1))
        g = c_loc(optical_props%g(1, 1, 1))
      end if
    class default
      error_msg = "cloud optics: optical_props must be ty_optical_props_1scl or ty_optical_props_2str"
    end select
    if (error_msg /= "") return
    if (ncol == 0) return
    rc = c_cloud_optics(this%handle, int(ncol, c_int), int(nlay, c_int), clwp, ciwp, reliq, reice, int(this%icergh, c_int), &
                        tau, ssa, g, memspace, c_null_ptr)
    if (rc /= 0) error_msg = c_error_message()
  end function cloud_optics

end module mo_cloud_optics
