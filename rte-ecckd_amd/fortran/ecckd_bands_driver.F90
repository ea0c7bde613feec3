! ecckd_bands_driver.F90 -- per-band fluxes of one block of columns from the fused path: the atmosphere and the
! particulate optical properties on the model's bands go through ecckd%lw_flux_bands or ecckd%sw_flux_bands
! (ecckd_lw_flux_bands / ecckd_sw_flux_bands; include/ecckd_hip.h, "Fused per-band fluxes") and the band planes are
! written out -- what a host binds for surface shortwave by band or outgoing longwave by band.
!
!   ecckd_bands_driver  lw|sw  <ecckd_file.nc>  <input.bin>  <output.bin>  [particles.bin]
!
! input.bin: the layout ecckd_driver reads (ecckd_driver.F90): int32 ncol, nlay, ngas; per gas a 32-char name; float64
! plev(ncol,nlay+1), tlev(ncol,nlay+1), tlay(ncol,nlay), tsfc(ncol), then sfc_emis(ncol) [lw] or mu0(ncol), albedo(ncol) [sw],
! then per gas vmr(ncol,nlay).
! particles.bin (absent: clear sky): int32 nband, with_ssa_g, delta_scale; float64 tau(ncol,nlay,nband) and, with_ssa_g = 1,
! ssa and g of the same shape (the shortwave needs all three; the longwave ignores g).
! output.bin: float64 bnd_flux_up, bnd_flux_dn (ncol,nlay+1,nband) [sw: bnd_flux_dir too], then the broadband flux_up,
! flux_dn (ncol,nlay+1) [sw: flux_dir too].
program ecckd_bands_driver
  use, intrinsic :: iso_fortran_env, only: error_unit, int32
  use gas_optics_ecckd, only: ty_gas_optics_ecckd
  use mo_gas_concentrations, only: ty_gas_concs
  use mo_rte_kind, only: wp
  implicit none
  character(len=512) :: mode, ecckd_path, in_path, out_path, part_path
  integer(int32) :: ncol, nlay, ngas, nband_p, with_ssa_g, delta
  integer :: u, i, ibnd, nband
  logical :: top_at_1, shortwave, particles
  character(len=32), dimension(:), allocatable :: gas_names
  real(wp), dimension(:,:), allocatable :: plev, tlev, tlay, sfc_spec, flux_up, flux_dn, flux_dir
  real(wp), dimension(:), allocatable :: tsfc, sfc, mu0
  real(wp), dimension(:,:,:), allocatable :: vmr, tau_p, ssa_p, g_p, bnd_up, bnd_dn, bnd_dir
  type(ty_gas_optics_ecckd) :: ecckd
  type(ty_gas_concs) :: gas_concs

  if (command_argument_count() < 4) then
    write(error_unit, "(a)") " usage: ecckd_bands_driver lw|sw ecckd_file input.bin output.bin [particles.bin]"
    stop 1
  end if
  call get_command_argument(1, mode)
  call get_command_argument(2, ecckd_path)
  call get_command_argument(3, in_path)
  call get_command_argument(4, out_path)
  shortwave = trim(mode) == "sw"
  if (.not. shortwave .and. trim(mode) /= "lw") call stop_on_err("ecckd_bands_driver: the first argument is lw or sw")
  particles = command_argument_count() >= 5
  if (particles) call get_command_argument(5, part_path)

  open(newunit=u, file=trim(in_path), access="stream", form="unformatted", status="old")
  read(u) ncol, nlay, ngas
  allocate(gas_names(ngas))
  read(u) gas_names
  allocate(plev(ncol, nlay + 1), tlev(ncol, nlay + 1), tlay(ncol, nlay), tsfc(ncol), sfc(ncol), mu0(ncol), vmr(ncol, nlay, ngas))
  read(u) plev, tlev, tlay, tsfc
  if (shortwave) read(u) mu0
  read(u) sfc, vmr
  close(u)

  call stop_on_err(ecckd%load(trim(ecckd_path)))
  if (ecckd%source_is_internal() .eqv. shortwave) call stop_on_err("ecckd_bands_driver: the file does not belong to the mode")
  nband = ecckd%get_nband()
  if (particles) then
    open(newunit=u, file=trim(part_path), access="stream", form="unformatted", status="old")
    read(u) nband_p, with_ssa_g, delta
    allocate(tau_p(ncol, nlay, nband_p))
    read(u) tau_p
    if (with_ssa_g /= 0) then
      allocate(ssa_p(ncol, nlay, nband_p), g_p(ncol, nlay, nband_p))
      read(u) ssa_p, g_p
    end if
    close(u)
    if (shortwave .and. with_ssa_g == 0) call stop_on_err("ecckd_bands_driver: the shortwave needs tau, ssa and g")
  end if
  call stop_on_err(gas_concs%init(gas_names))
  do i = 1, ngas
    if (all(vmr(:, :, i) == vmr(1, 1, i))) then
      call stop_on_err(gas_concs%set_vmr(trim(gas_names(i)), vmr(1, 1, i)))
    else
      call stop_on_err(gas_concs%set_vmr(trim(gas_names(i)), vmr(:, :, i)))
    end if
  end do

  top_at_1 = plev(1, 1) < plev(1, nlay + 1)
  allocate(sfc_spec(nband, ncol), flux_up(ncol, nlay + 1), flux_dn(ncol, nlay + 1), flux_dir(ncol, nlay + 1))
  allocate(bnd_up(ncol, nlay + 1, nband), bnd_dn(ncol, nlay + 1, nband), bnd_dir(ncol, nlay + 1, nband))
  do i = 1, ncol
    do ibnd = 1, nband
      sfc_spec(ibnd, i) = sfc(i)
    end do
  end do
  if (shortwave) then
    if (particles) then
      call stop_on_err(ecckd%sw_flux_bands(plev, tlay, gas_concs, top_at_1, mu0, sfc_spec, sfc_spec, bnd_up, bnd_dn, bnd_dir, &
                                           tau_p=tau_p, ssa_p=ssa_p, g_p=g_p, delta_scale=(delta /= 0), flux_up=flux_up, &
                                           flux_dn=flux_dn, flux_dir=flux_dir))
    else
      call stop_on_err(ecckd%sw_flux_bands(plev, tlay, gas_concs, top_at_1, mu0, sfc_spec, sfc_spec, bnd_up, bnd_dn, bnd_dir, &
                                           flux_up=flux_up, flux_dn=flux_dn, flux_dir=flux_dir))
    end if
  else if (particles .and. with_ssa_g /= 0) then
    call stop_on_err(ecckd%lw_flux_bands(plev, tlay, tsfc, tlev, gas_concs, top_at_1, sfc_spec, bnd_up, bnd_dn, tau_p=tau_p, &
                                         ssa_p=ssa_p, flux_up=flux_up, flux_dn=flux_dn))
  else if (particles) then
    call stop_on_err(ecckd%lw_flux_bands(plev, tlay, tsfc, tlev, gas_concs, top_at_1, sfc_spec, bnd_up, bnd_dn, tau_p=tau_p, &
                                         flux_up=flux_up, flux_dn=flux_dn))
  else
    call stop_on_err(ecckd%lw_flux_bands(plev, tlay, tsfc, tlev, gas_concs, top_at_1, sfc_spec, bnd_up, bnd_dn, flux_up=flux_up, &
                                         flux_dn=flux_dn))
  end if

  open(newunit=u, file=trim(out_path), access="stream", form="unformatted", status="replace")
  write(u) bnd_up, bnd_dn
  if (shortwave) write(u) bnd_dir
  write(u) flux_up, flux_dn
  if (shortwave) write(u) flux_dir
  close(u)
  call ecckd%finalize()
  write(error_unit, *) "ecckd_bands_driver: ", ncol, " columns, ", nband, " bands done"

contains
  subroutine stop_on_err(msg)
    character(len=*), intent(in) :: msg
    if (len_trim(msg) > 0) then
      write(error_unit, *) trim(msg)
      stop 1
    end if
  end subroutine stop_on_err
end program ecckd_bands_driver
