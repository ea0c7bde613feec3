! ecckd_aerosol_driver.F90 -- the all-sky chain from what a host model carries for its aerosols: species types, particle
! sizes, layer masses and relative humidity go through type(ty_aerosol_optics) (mo_aerosol_optics.F90) to the particulate
! properties on the model's bands, and those, with the atmosphere, through ecckd%lw_fluxes_allsky to fluxes -- the calls
! an all-sky RTE-RRTMGP driver makes between gas_optics and the solver, with the k-distribution of ecCKD.
!
!   ecckd_aerosol_driver  <ecckd_lw_file.nc>  <input.bin>  <aerosols.bin>  <output.bin>  [device_resident 0|1]
!
! device_resident = 1: the planes are the device twin ty_optical_props_2str_dev (they are written in HBM; only the inputs
! cross PCIe) and are copied back for the flux call and the output file.
! input.bin: the layout ecckd_driver reads for the longwave (ecckd_driver.F90): int32 ncol, nlay, ngas; per gas a 32-char
! name; float64 plev(ncol,nlay+1), tlev(ncol,nlay+1), tlay(ncol,nlay), tsfc(ncol), sfc_emis(ncol), then per gas vmr(ncol,nlay).
! aerosols.bin (little-endian): int32 nband, nbin, nrh, nspec; float64 bin_lims(2,nbin), rh_levels(nrh), dust_tbl(3,nbin,nband),
! salt_tbl(3,nrh,nbin,nband), sulf_tbl(3,nrh,nband), bcar_tbl(3,nband), bcar_rh_tbl(3,nrh,nband), ocar_tbl(3,nband),
! ocar_rh_tbl(3,nrh,nband); int32 aero_type(ncol,nlay,nspec); float64 aero_size, aero_mass (ncol,nlay,nspec), relhum(ncol,nlay).
! output.bin: float64 tau, ssa, g (ncol,nlay,nband), flux_up, flux_dn (ncol,nlay+1).
program ecckd_aerosol_driver
  use, intrinsic :: iso_fortran_env, only: error_unit, int32
  use gas_optics_ecckd, only: ty_gas_optics_ecckd
  use mo_aerosol_optics, only: ty_aerosol_optics
  use mo_gas_concentrations, only: ty_gas_concs
  use mo_optical_props, only: ty_optical_props_2str
  use mo_ecckd_device, only: ty_optical_props_2str_dev
  use mo_rte_kind, only: wp
  implicit none
  character(len=512) :: ecckd_path, in_path, aer_path, out_path, arg
  integer(int32) :: ncol, nlay, ngas, nband, nbin, nrh, nspec
  integer :: u, i, ibnd, dev_flag
  logical :: top_at_1
  character(len=32), dimension(:), allocatable :: gas_names
  real(wp), dimension(:,:), allocatable :: plev, tlev, tlay, relhum, sfc_spec, flux_up, flux_dn, bin_lims, bcar, ocar
  real(wp), dimension(:), allocatable :: tsfc, emis, rh_levels
  real(wp), dimension(:,:,:), allocatable :: vmr, dust, sulf, bcar_rh, ocar_rh, aero_size, aero_mass
  real(wp), dimension(:,:,:,:), allocatable :: salt
  integer(int32), dimension(:,:,:), allocatable :: aero_type
  type(ty_gas_optics_ecckd) :: ecckd
  type(ty_aerosol_optics) :: aerosol_optics
  type(ty_gas_concs) :: gas_concs
  class(ty_optical_props_2str), allocatable :: aerosols

  if (command_argument_count() < 4) then
    write(error_unit, "(a)") " usage: ecckd_aerosol_driver ecckd_lw_file input.bin aerosols.bin output.bin [device_resident 0|1]"
    stop 1
  end if
  call get_command_argument(1, ecckd_path)
  call get_command_argument(2, in_path)
  call get_command_argument(3, aer_path)
  call get_command_argument(4, out_path)
  dev_flag = 0
  if (command_argument_count() >= 5) then
    call get_command_argument(5, arg)
    read(arg, *) dev_flag
  end if

  open(newunit=u, file=trim(in_path), access="stream", form="unformatted", status="old")
  read(u) ncol, nlay, ngas
  allocate(gas_names(ngas))
  read(u) gas_names
  allocate(plev(ncol, nlay + 1), tlev(ncol, nlay + 1), tlay(ncol, nlay), tsfc(ncol), emis(ncol), vmr(ncol, nlay, ngas))
  read(u) plev, tlev, tlay, tsfc, emis, vmr
  close(u)

  open(newunit=u, file=trim(aer_path), access="stream", form="unformatted", status="old")
  read(u) nband, nbin, nrh, nspec
  allocate(bin_lims(2, nbin), rh_levels(nrh), dust(3, nbin, nband), salt(3, nrh, nbin, nband), sulf(3, nrh, nband), &
           bcar(3, nband), bcar_rh(3, nrh, nband), ocar(3, nband), ocar_rh(3, nrh, nband))
  allocate(aero_type(ncol, nlay, nspec), aero_size(ncol, nlay, nspec), aero_mass(ncol, nlay, nspec), relhum(ncol, nlay))
  read(u) bin_lims, rh_levels, dust, salt, sulf, bcar, bcar_rh, ocar, ocar_rh
  read(u) aero_type
  read(u) aero_size, aero_mass, relhum
  close(u)

  call stop_on_err(ecckd%load(trim(ecckd_path)))
  if (.not. ecckd%source_is_internal()) call stop_on_err("ecckd_aerosol_driver: a longwave k-distribution file is needed")
  if (ecckd%get_nband() /= nband) call stop_on_err("ecckd_aerosol_driver: the aerosol tables are not on the bands of the k-distribution")
  call stop_on_err(aerosol_optics%load(ecckd%get_band_lims_wavenumber(), bin_lims, rh_levels, dust, salt, sulf, bcar, bcar_rh, &
                                       ocar, ocar_rh))
  if (aerosol_optics%get_nbin() /= nbin .or. aerosol_optics%get_nrh() /= nrh) &
    call stop_on_err("ecckd_aerosol_driver: the getters disagree with the file")

  call stop_on_err(gas_concs%init(gas_names))
  do i = 1, ngas
    if (all(vmr(:, :, i) == vmr(1, 1, i))) then
      call stop_on_err(gas_concs%set_vmr(trim(gas_names(i)), vmr(1, 1, i)))
    else
      call stop_on_err(gas_concs%set_vmr(trim(gas_names(i)), vmr(:, :, i)))
    end if
  end do

  ! species, sizes, masses, humidity -> band properties (between gas_optics and increment in an all-sky RTE-RRTMGP driver)
  if (dev_flag /= 0) then
    allocate(ty_optical_props_2str_dev :: aerosols)
  else
    allocate(ty_optical_props_2str :: aerosols)
  end if
  call stop_on_err(aerosols%alloc_2str(int(ncol), int(nlay), aerosol_optics))
  if (nspec == 1) then   ! RTE-RRTMGP's call
    call stop_on_err(aerosol_optics%aerosol_optics(int(aero_type(:, :, 1)), aero_size(:, :, 1), aero_mass(:, :, 1), relhum, aerosols))
  else
    call stop_on_err(aerosol_optics%aerosol_optics(int(aero_type), aero_size, aero_mass, relhum, aerosols))
  end if
  select type (aerosols)
  type is (ty_optical_props_2str_dev)
    call stop_on_err(aerosols%copy_to_host())
  end select

  ! ... -> fluxes
  top_at_1 = plev(1, 1) < plev(1, nlay + 1)
  allocate(sfc_spec(nband, ncol), flux_up(ncol, nlay + 1), flux_dn(ncol, nlay + 1))
  do i = 1, ncol
    do ibnd = 1, nband
      sfc_spec(ibnd, i) = emis(i)
    end do
  end do
  call stop_on_err(ecckd%lw_fluxes_allsky(plev, tlay, tsfc, tlev, gas_concs, top_at_1, sfc_spec, aerosols%tau, flux_up, flux_dn, &
                                          ssa_p=aerosols%ssa))

  open(newunit=u, file=trim(out_path), access="stream", form="unformatted", status="replace")
  write(u) aerosols%tau, aerosols%ssa, aerosols%g, flux_up, flux_dn
  close(u)
  select type (aerosols)
  type is (ty_optical_props_2str_dev)
    call aerosols%free()
  end select
  call aerosol_optics%finalize()
  call ecckd%finalize()
  write(error_unit, *) "ecckd_aerosol_driver: ", ncol, " columns done"

contains
  subroutine stop_on_err(msg)
    character(len=*), intent(in) :: msg
    if (len_trim(msg) > 0) then
      write(error_unit, *) trim(msg)
      stop 1
    end if
  end subroutine stop_on_err
end program ecckd_aerosol_driver
