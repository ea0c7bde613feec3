! ecckd_scaling_driver.F90 -- all-sky fluxes of one block of columns with in-cloud water variability: a lognormal scaling
! table is built (ty_cloud_scaling%load_lognormal), the optical-depth scaling of every (column, layer, g-point) is sampled
! from the cloud fractions (ecckd%sample_cloud_scaling; include/ecckd_hip.h, "In-cloud water variability") and handed to
! ecckd%lw_flux_scaled or ecckd%sw_flux_scaled with the particulate optical properties on the model's bands.
!
!   ecckd_scaling_driver  lw|sw  <ecckd_file.nc>  <input.bin>  <output.bin>  <particles.bin>  <scaling.bin>
!
! input.bin: the layout ecckd_driver reads (ecckd_driver.F90): int32 ncol, nlay, ngas; per gas a 32-char name; float64
! plev(ncol,nlay+1), tlev(ncol,nlay+1), tlay(ncol,nlay), tsfc(ncol), then sfc_emis(ncol) [lw] or mu0(ncol), albedo(ncol) [sw],
! then per gas vmr(ncol,nlay).
! particles.bin: int32 nband, with_ssa_g, delta_scale; float64 tau(ncol,nlay,nband) and, with_ssa_g = 1, ssa and g of the
! same shape (the shortwave needs all three; the longwave ignores g).
! scaling.bin: int32 overlap; int64 seed; int32 nfsd, nq; float64 fsd0, dfsd; float64 cloud_frac(ncol,nlay),
! fsd(ncol,nlay) and, with overlap = 1, overlap_param(ncol,nlay-1).
! output.bin: float64 flux_up, flux_dn (ncol,nlay+1), then float32 cloud_scaling(ncol,nlay,ngpt).
program ecckd_scaling_driver
  use, intrinsic :: iso_fortran_env, only: error_unit, int32, int64, real32
  use gas_optics_ecckd, only: ty_gas_optics_ecckd, ty_cloud_scaling
  use mo_gas_concentrations, only: ty_gas_concs
  use mo_rte_kind, only: wp
  implicit none
  character(len=512) :: mode, ecckd_path, in_path, out_path, part_path, scal_path
  integer(int32) :: ncol, nlay, ngas, nband_p, with_ssa_g, delta, overlap, nfsd, nq
  integer(int64) :: seed
  real(wp) :: fsd0, dfsd
  integer :: u, i, ibnd, nband
  logical :: top_at_1, shortwave
  character(len=32), dimension(:), allocatable :: gas_names
  real(wp), dimension(:,:), allocatable :: plev, tlev, tlay, sfc_spec, flux_up, flux_dn, cloud_frac, fsd, alpha
  real(wp), dimension(:), allocatable :: tsfc, sfc, mu0
  real(wp), dimension(:,:,:), allocatable :: vmr, tau_p, ssa_p, g_p
  real(real32), dimension(:,:,:), allocatable :: scaling
  type(ty_gas_optics_ecckd) :: ecckd
  type(ty_cloud_scaling) :: table
  type(ty_gas_concs) :: gas_concs

  if (command_argument_count() < 6) then
    write(error_unit, "(a)") " usage: ecckd_scaling_driver lw|sw ecckd_file input.bin output.bin particles.bin scaling.bin"
    stop 1
  end if
  call get_command_argument(1, mode)
  call get_command_argument(2, ecckd_path)
  call get_command_argument(3, in_path)
  call get_command_argument(4, out_path)
  call get_command_argument(5, part_path)
  call get_command_argument(6, scal_path)
  shortwave = trim(mode) == "sw"
  if (.not. shortwave .and. trim(mode) /= "lw") call stop_on_err("ecckd_scaling_driver: the first argument is lw or sw")

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
  if (ecckd%source_is_internal() .eqv. shortwave) call stop_on_err("ecckd_scaling_driver: the file does not belong to the mode")
  nband = ecckd%get_nband()
  open(newunit=u, file=trim(part_path), access="stream", form="unformatted", status="old")
  read(u) nband_p, with_ssa_g, delta
  allocate(tau_p(ncol, nlay, nband_p))
  read(u) tau_p
  if (with_ssa_g /= 0) then
    allocate(ssa_p(ncol, nlay, nband_p), g_p(ncol, nlay, nband_p))
    read(u) ssa_p, g_p
  end if
  close(u)
  if (shortwave .and. with_ssa_g == 0) call stop_on_err("ecckd_scaling_driver: the shortwave needs tau, ssa and g")
  open(newunit=u, file=trim(scal_path), access="stream", form="unformatted", status="old")
  read(u) overlap, seed, nfsd, nq, fsd0, dfsd
  allocate(cloud_frac(ncol, nlay), fsd(ncol, nlay), alpha(ncol, max(nlay - 1, 0)))
  read(u) cloud_frac, fsd
  if (overlap == 1) read(u) alpha
  close(u)

  call stop_on_err(gas_concs%init(gas_names))
  do i = 1, ngas
    if (all(vmr(:, :, i) == vmr(1, 1, i))) then
      call stop_on_err(gas_concs%set_vmr(trim(gas_names(i)), vmr(1, 1, i)))
    else
      call stop_on_err(gas_concs%set_vmr(trim(gas_names(i)), vmr(:, :, i)))
    end if
  end do

  call stop_on_err(table%load_lognormal(ecckd, int(nfsd), fsd0, dfsd, int(nq)))
  allocate(scaling(ncol, nlay, ecckd%get_ngpt()))
  if (overlap == 1) then
    call stop_on_err(ecckd%sample_cloud_scaling(table, cloud_frac, int(overlap), seed, 0_int64, scaling, fsd=fsd, overlap_param=alpha))
  else
    call stop_on_err(ecckd%sample_cloud_scaling(table, cloud_frac, int(overlap), seed, 0_int64, scaling, fsd=fsd))
  end if

  top_at_1 = plev(1, 1) < plev(1, nlay + 1)
  allocate(sfc_spec(nband, ncol), flux_up(ncol, nlay + 1), flux_dn(ncol, nlay + 1))
  do i = 1, ncol
    do ibnd = 1, nband
      sfc_spec(ibnd, i) = sfc(i)
    end do
  end do
  if (shortwave) then
    call stop_on_err(ecckd%sw_flux_scaled(plev, tlay, gas_concs, top_at_1, mu0, sfc_spec, sfc_spec, tau_p, ssa_p, g_p, scaling, &
                                          flux_up, flux_dn, delta_scale=(delta /= 0)))
  else if (with_ssa_g /= 0) then
    call stop_on_err(ecckd%lw_flux_scaled(plev, tlay, tsfc, tlev, gas_concs, top_at_1, sfc_spec, tau_p, scaling, flux_up, flux_dn, &
                                          ssa_p=ssa_p))
  else
    call stop_on_err(ecckd%lw_flux_scaled(plev, tlay, tsfc, tlev, gas_concs, top_at_1, sfc_spec, tau_p, scaling, flux_up, flux_dn))
  end if

  open(newunit=u, file=trim(out_path), access="stream", form="unformatted", status="replace")
  write(u) flux_up, flux_dn
  write(u) scaling
  close(u)
  call table%finalize()
  call ecckd%finalize()
  write(error_unit, *) "ecckd_scaling_driver: ", ncol, " columns done"

contains
  subroutine stop_on_err(msg)
    character(len=*), intent(in) :: msg
    if (len_trim(msg) > 0) then
      write(error_unit, *) trim(msg)
      stop 1
    end if
  end subroutine stop_on_err
end program ecckd_scaling_driver
