! ecckd_cloud_driver.F90 -- the all-sky chain from what a host model carries: liquid and ice water paths and effective
! radii go through type(ty_cloud_optics) (mo_cloud_optics.F90) to the particulate properties on the model's bands, and
! those, with the atmosphere, through ecckd%lw_fluxes_allsky to fluxes -- the calls an all-sky RTE-RRTMGP driver makes
! between gas_optics and the solver, with the k-distribution of ecCKD.
!
!   ecckd_cloud_driver  <ecckd_lw_file.nc>  <input.bin>  <clouds.bin>  <output.bin>  [device_resident 0|1]
!
! device_resident = 1: the planes are the device twin ty_optical_props_2str_dev (they are written in HBM; only the four
! (ncol,nlay) inputs cross PCIe) and are copied back for the flux call and the output file.
! input.bin: the layout ecckd_driver reads for the longwave (ecckd_driver.F90): int32 ncol, nlay, ngas; per gas a 32-char
! name; float64 plev(ncol,nlay+1), tlev(ncol,nlay+1), tlay(ncol,nlay), tsfc(ncol), sfc_emis(ncol), then per gas vmr(ncol,nlay).
! clouds.bin (little-endian): int32 nband, nsize_liq, nsize_ice, nrghice, icergh; float64 radliq_lwr, radliq_upr,
! radice_lwr, radice_upr; float64 lut_extliq, lut_ssaliq, lut_asyliq (nsize_liq,nband), lut_extice, lut_ssaice, lut_asyice
! (nsize_ice,nband,nrghice); float64 clwp, ciwp, reliq, reice (ncol,nlay).
! output.bin: float64 tau, ssa, g (ncol,nlay,nband), flux_up, flux_dn (ncol,nlay+1).
program ecckd_cloud_driver
  use, intrinsic :: iso_fortran_env, only: error_unit, int32
  use gas_optics_ecckd, only: ty_gas_optics_ecckd
  use mo_cloud_optics, only: ty_cloud_optics
  use mo_gas_concentrations, only: ty_gas_concs
  use mo_optical_props, only: ty_optical_props_2str
  use mo_ecckd_device, only: ty_optical_props_2str_dev
  use mo_rte_kind, only: wp
  implicit none
  character(len=512) :: ecckd_path, in_path, cloud_path, out_path, arg
  integer(int32) :: ncol, nlay, ngas, nband, nsize_liq, nsize_ice, nrghice, icergh
  integer :: u, i, ibnd, dev_flag
  logical :: top_at_1
  character(len=32), dimension(:), allocatable :: gas_names
  real(wp), dimension(:,:), allocatable :: plev, tlev, tlay, clwp, ciwp, reliq, reice, sfc_spec, flux_up, flux_dn
  real(wp), dimension(:), allocatable :: tsfc, emis
  real(wp), dimension(:,:,:), allocatable :: vmr, extice, ssaice, asyice
  real(wp), dimension(:,:), allocatable :: extliq, ssaliq, asyliq
  real(wp) :: radliq_lwr, radliq_upr, radice_lwr, radice_upr
  type(ty_gas_optics_ecckd) :: ecckd
  type(ty_cloud_optics) :: cloud_optics
  type(ty_gas_concs) :: gas_concs
  class(ty_optical_props_2str), allocatable :: clouds

  if (command_argument_count() < 4) then
    write(error_unit, "(a)") " usage: ecckd_cloud_driver ecckd_lw_file input.bin clouds.bin output.bin [device_resident 0|1]"
    stop 1
  end if
  call get_command_argument(1, ecckd_path)
  call get_command_argument(2, in_path)
  call get_command_argument(3, cloud_path)
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

  open(newunit=u, file=trim(cloud_path), access="stream", form="unformatted", status="old")
  read(u) nband, nsize_liq, nsize_ice, nrghice, icergh
  read(u) radliq_lwr, radliq_upr, radice_lwr, radice_upr
  allocate(extliq(nsize_liq, nband), ssaliq(nsize_liq, nband), asyliq(nsize_liq, nband))
  allocate(extice(nsize_ice, nband, nrghice), ssaice(nsize_ice, nband, nrghice), asyice(nsize_ice, nband, nrghice))
  allocate(clwp(ncol, nlay), ciwp(ncol, nlay), reliq(ncol, nlay), reice(ncol, nlay))
  read(u) extliq, ssaliq, asyliq, extice, ssaice, asyice
  read(u) clwp, ciwp, reliq, reice
  close(u)

  call stop_on_err(ecckd%load(trim(ecckd_path)))
  if (.not. ecckd%source_is_internal()) call stop_on_err("ecckd_cloud_driver: a longwave k-distribution file is needed")
  if (ecckd%get_nband() /= nband) call stop_on_err("ecckd_cloud_driver: the cloud tables are not on the bands of the k-distribution")
  call stop_on_err(cloud_optics%load(ecckd%get_band_lims_wavenumber(), radliq_lwr, radliq_upr, 1._wp, radice_lwr, radice_upr, &
                                     1._wp, extliq, ssaliq, asyliq, extice, ssaice, asyice))
  call stop_on_err(cloud_optics%set_ice_roughness(int(icergh)))
  if (cloud_optics%get_min_radius_liq() /= radliq_lwr .or. cloud_optics%get_max_radius_ice() /= radice_upr .or. &
      cloud_optics%get_num_ice_roughness_types() /= nrghice) call stop_on_err("ecckd_cloud_driver: the getters disagree with the file")

  call stop_on_err(gas_concs%init(gas_names))
  do i = 1, ngas
    if (all(vmr(:, :, i) == vmr(1, 1, i))) then
      call stop_on_err(gas_concs%set_vmr(trim(gas_names(i)), vmr(1, 1, i)))
    else
      call stop_on_err(gas_concs%set_vmr(trim(gas_names(i)), vmr(:, :, i)))
    end if
  end do

  ! water paths and radii -> band properties (between gas_optics and increment in an all-sky RTE-RRTMGP driver)
  if (dev_flag /= 0) then
    allocate(ty_optical_props_2str_dev :: clouds)
  else
    allocate(ty_optical_props_2str :: clouds)
  end if
  call stop_on_err(clouds%alloc_2str(int(ncol), int(nlay), cloud_optics))
  call stop_on_err(cloud_optics%cloud_optics(clwp, ciwp, reliq, reice, clouds))
  select type (clouds)
  type is (ty_optical_props_2str_dev)
    call stop_on_err(clouds%copy_to_host())
  end select

  ! ... -> fluxes
  top_at_1 = plev(1, 1) < plev(1, nlay + 1)
  allocate(sfc_spec(nband, ncol), flux_up(ncol, nlay + 1), flux_dn(ncol, nlay + 1))
  do i = 1, ncol
    do ibnd = 1, nband
      sfc_spec(ibnd, i) = emis(i)
    end do
  end do
  call stop_on_err(ecckd%lw_fluxes_allsky(plev, tlay, tsfc, tlev, gas_concs, top_at_1, sfc_spec, clouds%tau, flux_up, flux_dn, &
                                          ssa_p=clouds%ssa))

  open(newunit=u, file=trim(out_path), access="stream", form="unformatted", status="replace")
  write(u) clouds%tau, clouds%ssa, clouds%g, flux_up, flux_dn
  close(u)
  select type (clouds)
  type is (ty_optical_props_2str_dev)
    call clouds%free()
  end select
  call cloud_optics%finalize()
  call ecckd%finalize()
  write(error_unit, *) "ecckd_cloud_driver: ", ncol, " columns done"

contains
  subroutine stop_on_err(msg)
    character(len=*), intent(in) :: msg
    if (len_trim(msg) > 0) then
      write(error_unit, *) trim(msg)
      stop 1
    end if
  end subroutine stop_on_err
end program ecckd_cloud_driver
