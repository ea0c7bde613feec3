! ecckd_heating_driver.F90 -- a radiation step to its end: the atmosphere goes through ecckd%lw_fluxes to fluxes, and
! those, with the level pressures, through compute_heating_rate (mo_heating_rates.F90) to the temperature tendency in
! K s-1 -- the call every all-sky RTE-RRTMGP driver makes after rte_lw / rte_sw.
!
!   ecckd_heating_driver  <ecckd_lw_file.nc>  <input.bin>  <output.bin>  [device_resident 0|1]
!
! device_resident = 1: the heating rate is written into the device container ty_heating_rate_dev (it stays in HBM; only
! the fluxes and pressures cross PCIe) and is copied back for the output file.
! input.bin: the layout ecckd_driver reads for the longwave (ecckd_driver.F90): int32 ncol, nlay, ngas; per gas a 32-char
! name; float64 plev(ncol,nlay+1), tlev(ncol,nlay+1), tlay(ncol,nlay), tsfc(ncol), sfc_emis(ncol), then per gas vmr(ncol,nlay).
! output.bin: float64 flux_up, flux_dn (ncol,nlay+1), heating_rate (ncol,nlay).
program ecckd_heating_driver
  use, intrinsic :: iso_fortran_env, only: error_unit, int32
  use gas_optics_ecckd, only: ty_gas_optics_ecckd
  use mo_gas_concentrations, only: ty_gas_concs
  use mo_heating_rates, only: compute_heating_rate, ty_heating_rate_dev
  use mo_rte_kind, only: wp
  implicit none
  character(len=512) :: ecckd_path, in_path, out_path, arg
  integer(int32) :: ncol, nlay, ngas
  integer :: u, i, ibnd, nband, dev_flag
  logical :: top_at_1
  character(len=32), dimension(:), allocatable :: gas_names
  real(wp), dimension(:,:), allocatable :: plev, tlev, tlay, sfc_spec, flux_up, flux_dn, heating_rate
  real(wp), dimension(:), allocatable :: tsfc, emis
  real(wp), dimension(:,:,:), allocatable :: vmr
  type(ty_gas_optics_ecckd) :: ecckd
  type(ty_gas_concs) :: gas_concs
  type(ty_heating_rate_dev) :: heating_dev

  if (command_argument_count() < 3) then
    write(error_unit, "(a)") " usage: ecckd_heating_driver ecckd_lw_file input.bin output.bin [device_resident 0|1]"
    stop 1
  end if
  call get_command_argument(1, ecckd_path)
  call get_command_argument(2, in_path)
  call get_command_argument(3, out_path)
  dev_flag = 0
  if (command_argument_count() >= 4) then
    call get_command_argument(4, arg)
    read(arg, *) dev_flag
  end if

  open(newunit=u, file=trim(in_path), access="stream", form="unformatted", status="old")
  read(u) ncol, nlay, ngas
  allocate(gas_names(ngas))
  read(u) gas_names
  allocate(plev(ncol, nlay + 1), tlev(ncol, nlay + 1), tlay(ncol, nlay), tsfc(ncol), emis(ncol), vmr(ncol, nlay, ngas))
  read(u) plev, tlev, tlay, tsfc, emis, vmr
  close(u)

  call stop_on_err(ecckd%load(trim(ecckd_path)))
  if (.not. ecckd%source_is_internal()) call stop_on_err("ecckd_heating_driver: a longwave k-distribution file is needed")
  nband = ecckd%get_nband()
  call stop_on_err(gas_concs%init(gas_names))
  do i = 1, ngas
    if (all(vmr(:, :, i) == vmr(1, 1, i))) then
      call stop_on_err(gas_concs%set_vmr(trim(gas_names(i)), vmr(1, 1, i)))
    else
      call stop_on_err(gas_concs%set_vmr(trim(gas_names(i)), vmr(:, :, i)))
    end if
  end do

  ! the atmosphere -> fluxes
  top_at_1 = plev(1, 1) < plev(1, nlay + 1)
  allocate(sfc_spec(nband, ncol), flux_up(ncol, nlay + 1), flux_dn(ncol, nlay + 1), heating_rate(ncol, nlay))
  do i = 1, ncol
    do ibnd = 1, nband
      sfc_spec(ibnd, i) = emis(i)
    end do
  end do
  call stop_on_err(ecckd%lw_fluxes(plev, tlay, tsfc, tlev, gas_concs, top_at_1, sfc_spec, flux_up, flux_dn))

  ! ... -> heating rates (after rte_lw / rte_sw in an RTE-RRTMGP driver)
  if (dev_flag /= 0) then
    call stop_on_err(heating_dev%alloc(int(ncol), int(nlay)))
    call stop_on_err(compute_heating_rate(flux_up, flux_dn, plev, heating_dev))
    call stop_on_err(heating_dev%copy_to_host())
    heating_rate = heating_dev%heating_rate(:, :, 1)
    call heating_dev%free()
  else
    call stop_on_err(compute_heating_rate(flux_up, flux_dn, plev, heating_rate))
  end if

  open(newunit=u, file=trim(out_path), access="stream", form="unformatted", status="replace")
  write(u) flux_up, flux_dn, heating_rate
  close(u)
  call ecckd%finalize()
  write(error_unit, *) "ecckd_heating_driver: ", ncol, " columns done"

contains
  subroutine stop_on_err(msg)
    character(len=*), intent(in) :: msg
    if (len_trim(msg) > 0) then
      write(error_unit, *) trim(msg)
      stop 1
    end if
  end subroutine stop_on_err
end program ecckd_heating_driver
