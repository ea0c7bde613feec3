! Stand-ins for the five RTE-RRTMGP modules the reference's gas-optics module `use`s
! (src/gas_optics_ecckd.f90:3-7).  TEST INFRASTRUCTURE ONLY: they let that module be compiled
! unmodified into oracle/_ref/libecckd_ref.so, against which the C oracle is checked bit for bit
! (tests/test_oracle_vs_reference.py).  Each declares only what the module touches; nothing here
! is RTE-RRTMGP's code.

module mo_rte_kind
  use, intrinsic :: iso_c_binding, only: c_double
  implicit none
  integer, parameter, public :: wp = c_double
end module mo_rte_kind


module mo_optical_props
  use mo_rte_kind, only: wp
  implicit none
  private

  type, public :: ty_optical_props
    integer :: unused = 0
  end type ty_optical_props

  type, abstract, extends(ty_optical_props), public :: ty_optical_props_arry
    real(wp), dimension(:,:,:), allocatable :: tau      ! (ncol, nlay, ngpt)
  end type ty_optical_props_arry

  type, extends(ty_optical_props_arry), public :: ty_optical_props_1scl
  end type ty_optical_props_1scl

  type, extends(ty_optical_props_arry), public :: ty_optical_props_2str
    real(wp), dimension(:,:,:), allocatable :: ssa      ! (ncol, nlay, ngpt)
    real(wp), dimension(:,:,:), allocatable :: g        ! (ncol, nlay, ngpt)
  end type ty_optical_props_2str
end module mo_optical_props


module mo_source_functions
  use mo_rte_kind, only: wp
  use mo_optical_props, only: ty_optical_props
  implicit none
  private

  type, extends(ty_optical_props), public :: ty_source_func_lw
    real(wp), dimension(:,:,:), allocatable :: lay_source      ! (ncol, nlay, ngpt)
    real(wp), dimension(:,:,:), allocatable :: lev_source_inc  ! (ncol, nlay, ngpt)
    real(wp), dimension(:,:,:), allocatable :: lev_source_dec  ! (ncol, nlay, ngpt)
    real(wp), dimension(:,:),   allocatable :: sfc_source      ! (ncol, ngpt)
  end type ty_source_func_lw
end module mo_source_functions


! Every gas holds a full (ncol, nlay) field: RTE-RRTMGP's get_vmr broadcasts scalar and
! per-column values to that shape, and a broadcast is an exact copy.
module mo_gas_concentrations
  use mo_rte_kind, only: wp
  implicit none
  private

  type, public :: ty_gas_concs
    character(len=32), allocatable :: names(:)
    real(wp), dimension(:,:,:), allocatable :: vmr        ! (ncol, nlay, ngas)
  contains
    procedure, public :: get_num_gases
    procedure, public :: get_gas_names
    procedure, public :: get_vmr
  end type ty_gas_concs

contains

  pure function get_num_gases(this)
    class(ty_gas_concs), intent(in) :: this
    integer :: get_num_gases
    get_num_gases = size(this%names)
  end function get_num_gases

  pure function get_gas_names(this)
    class(ty_gas_concs), intent(in) :: this
    character(len=32), dimension(size(this%names)) :: get_gas_names
    get_gas_names = this%names
  end function get_gas_names

  function get_vmr(this, gas, array) result(error_msg)
    class(ty_gas_concs), intent(in) :: this
    character(len=*), intent(in) :: gas
    real(wp), dimension(:,:), intent(out) :: array
    character(len=128) :: error_msg
    integer :: i
    error_msg = ""
    do i = 1, size(this%names)
      if (trim(this%names(i)) == trim(gas)) then
        array(:,:) = this%vmr(:,:,i)
        return
      endif
    enddo
    error_msg = "gas " // trim(gas) // " not found"
  end function get_vmr
end module mo_gas_concentrations


module mo_gas_optics
  use mo_rte_kind, only: wp
  use mo_optical_props, only: ty_optical_props, ty_optical_props_arry
  use mo_source_functions, only: ty_source_func_lw
  use mo_gas_concentrations, only: ty_gas_concs
  implicit none
  private

  type, abstract, extends(ty_optical_props), public :: ty_gas_optics
  contains
    generic, public :: gas_optics => gas_optics_int, gas_optics_ext
    procedure(gas_optics_int_abstract), deferred, public :: gas_optics_int
    procedure(gas_optics_ext_abstract), deferred, public :: gas_optics_ext
  end type ty_gas_optics

  abstract interface
    function gas_optics_int_abstract(this, play, plev, tlay, tsfc, gas_desc, &
                                     optical_props, sources, col_dry, tlev) result(error_msg)
      import ty_gas_optics, wp, ty_gas_concs, ty_optical_props_arry, ty_source_func_lw
      class(ty_gas_optics), intent(in) :: this
      real(wp), dimension(:,:), intent(in) :: play
      real(wp), dimension(:,:), intent(in) :: plev
      real(wp), dimension(:,:), intent(in) :: tlay
      real(wp), dimension(:), intent(in) :: tsfc
      type(ty_gas_concs), intent(in) :: gas_desc
      class(ty_optical_props_arry), intent(inout)    :: optical_props
      class(ty_source_func_lw), intent(inout) :: sources
      character(len=128) :: error_msg
      real(wp), dimension(:,:), intent(in), target, optional :: col_dry
      real(wp), dimension(:,:), intent(in), target, optional :: tlev
    end function gas_optics_int_abstract

    function gas_optics_ext_abstract(this, play, plev, tlay, gas_desc, optical_props, &
                                     toa_src, col_dry) result(error_msg)
      import ty_gas_optics, wp, ty_gas_concs, ty_optical_props_arry
      class(ty_gas_optics), intent(in) :: this
      real(wp), dimension(:,:), intent(in) :: play
      real(wp), dimension(:,:), intent(in) :: plev
      real(wp), dimension(:,:), intent(in) :: tlay
      type(ty_gas_concs), intent(in) :: gas_desc
      class(ty_optical_props_arry), intent(inout)    :: optical_props
      real(wp), dimension(:,:), intent(out) :: toa_src
      real(wp), dimension(:,:), intent(in), target, optional :: col_dry
      character(len=128) :: error_msg
    end function gas_optics_ext_abstract
  end interface
end module mo_gas_optics
