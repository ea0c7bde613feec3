! ecckd_driver.F90 -- Fortran host program over the drop-in module, shaped like the block loop of
! example/rfmip-rad-irf/ecckd_rfmip_lw.F90:107-136 and ecckd_rfmip_sw.F90:112-162: load the ecCKD
! file, then per column block gas_optics() followed by rte_lw()/rte_sw(), fluxes out.
!
!   ecckd_driver lw|sw  <ecckd_file.nc>  <input.bin>  <output.bin>  [block_size] [n_quad_angles] [device_resident 0|1] [repeats] [byband 0|1] [fused 0|1] [particles.bin] [cloudfrac.bin] [clear.bin] [jac.bin]
!
! device_resident = 1: optical_props / source are the device twins of mo_ecckd_device (tau and the sources stay in
! HBM between gas_optics and the solver; ECCKD_MIXED memory space of the C ABI).
! repeats: the block loop is run that many times and the best wall time is printed ("loop_seconds", bench.py reads it).
! fused = 1: one call ecckd%lw_fluxes(...) / ecckd%sw_fluxes(...) per block instead of gas_optics + rte_lw / rte_sw (the library's
!            fused paths).
! particles.bin (needs fused = 1): all-sky -- the combined cloud / aerosol optical properties on the model's bands; one
!            call ecckd%lw_fluxes_allsky(...) / ecckd%sw_fluxes_allsky(...) per block on a contiguous copy of its columns.
!            Little-endian: int32 nband, has_ssa_g, delta_scale; then float64 tau(ncol,nlay,nband) and, if has_ssa_g /= 0,
!            ssa and g of the same shape (the longwave ignores g and delta_scale; without ssa the particles are one-stream,
!            longwave only).
! cloudfrac.bin (needs particles.bin): McICA -- per block, ecckd%sample_cloud_mask(...) with col0 = the block's 0-based
!            column offset, and the mask goes to the all-sky call (cloud_mask=).  Little-endian: int32 overlap (0 maximum-
!            random, 1 exponential-random), int64 seed, float64 cloud_frac(ncol,nlay) and, for overlap 1,
!            overlap_param(ncol,nlay-1).
! clear.bin (needs fused = 1 and particles.bin): a second output file, in the layout of output.bin, with the clear-sky fluxes
!            of the same columns -- the all-sky call is made with flux_up_clear / flux_dn_clear, so both skies come from one
!            gas-optics pass per block (ecckd_lw_fluxes_clear_allsky / ecckd_sw_fluxes_clear_allsky).  An empty string for
!            cloudfrac.bin (or any file argument) means "none".
! jac.bin (longwave, host containers: device_resident = 0): a further output file with flux_up_jac(ncol,nlay+1), the derivative
!            of flux_up with respect to the surface temperature (W m-2 K-1), in the layout of an array of output.bin.
!            fused = 1: the fused call of the block is made with flux_up_Jac; fused = 0: ecckd%planck_sfc_source_jac fills
!            sources%sfc_source_Jac behind gas_optics and rte_lw is called with flux_up_Jac.
! byband = 1: fluxes go through ty_fluxes_byband (per-band arrays; their sum over bands must reproduce the broadband
! fluxes, which are what output.bin holds either way).
!
! input.bin (little-endian, written by tests/test_fortran_shim.py): int32 ncol, nlay, ngas; per gas
! a 32-char name; then float64 arrays in Fortran order: plev(ncol,nlay+1), tlev(ncol,nlay+1),
! tlay(ncol,nlay), tsfc(ncol), sfc_emis(ncol) [lw] or mu0(ncol), albedo(ncol) [sw], then per gas
! vmr(ncol,nlay).  output.bin: flux_up(ncol,nlay+1), flux_dn(ncol,nlay+1).
! (The RFMIP netCDF files the reference drivers read are an FTP download and not available here.)
program ecckd_driver
  use, intrinsic :: iso_fortran_env, only: error_unit, int32, int64
  use gas_optics_ecckd, only: ty_gas_optics_ecckd, ECCKD_OVERLAP_EXP_RAN
  use mo_fluxes, only: ty_fluxes_broadband
  use mo_fluxes_byband, only: ty_fluxes_byband
  use mo_gas_concentrations, only: ty_gas_concs
  use mo_optical_props, only: ty_optical_props_1scl, ty_optical_props_2str
  use mo_ecckd_device, only: ty_optical_props_1scl_dev, ty_optical_props_2str_dev, ty_source_func_lw_dev
  use mo_rte_kind, only: wp
  use mo_rte_lw, only: rte_lw, rte_set_solver_option
  use mo_rte_sw, only: rte_sw
  use mo_source_functions, only: ty_source_func_lw
  implicit none
  character(len=512) :: mode, ecckd_path, in_path, out_path, arg
  integer(int32) :: ncol, nlay, ngas
  integer :: block_size, n_quad_angles, nblocks, b, c0, c1, nc, i, ibnd, nbnd, u, dev_flag, repeats, rep, byband
  integer(kind=8) :: t0, t1, rate
  integer :: nc_alloc = -1, fused = 0
  real(wp) :: best, secs
  real(wp), dimension(:,:,:), allocatable, target :: bnd_up, bnd_dn
  logical :: top_at_1, lw
  character(len=32), dimension(:), allocatable :: gas_names
  real(wp), dimension(:,:), allocatable :: plev, tlev, tlay, play
  real(wp), dimension(:), allocatable :: tsfc, bc1, bc2
  real(wp), dimension(:,:,:), allocatable :: vmr
  real(wp), dimension(:,:), allocatable, target :: flux_up, flux_dn
  real(wp), dimension(:,:), allocatable :: sfc_spec, sfc_spec2, toa
  character(len=512) :: part_path
  logical :: allsky = .false.
  character(len=512) :: frac_path
  logical :: mcica = .false.
  character(len=512) :: clear_path
  logical :: both = .false.
  real(wp), dimension(:,:), allocatable :: clear_up, clear_dn
  character(len=512) :: jac_path
  logical :: with_jac = .false.
  real(wp), dimension(:,:), allocatable :: jac_up
  real(wp), dimension(:,:), allocatable :: jac_b   ! the block's Jacobian; unallocated (= absent) without jac.bin
  integer(int32) :: overlap
  integer(int64) :: seed
  real(wp), dimension(:,:), allocatable :: cloud_frac, overlap_param
  integer(int64), dimension(:,:), allocatable :: mask_b   ! the block's mask; unallocated (= absent) without cloudfrac.bin
  integer(int32) :: nband_p, has_ssa_g, delta_flag
  real(wp), dimension(:,:,:), allocatable :: tau_p, ssa_p, g_p
  type(ty_gas_optics_ecckd) :: ecckd
  type(ty_gas_concs), dimension(:), allocatable :: gas_concs   ! one per block, filled before the loop (mo_rfmip_io.F90:177-263)
  class(ty_source_func_lw), allocatable :: source
  class(ty_optical_props_1scl), allocatable :: op1
  class(ty_optical_props_2str), allocatable :: op2
  type(ty_fluxes_broadband), target :: fluxes_bb
  type(ty_fluxes_byband), target :: fluxes_band
  class(ty_fluxes_broadband), pointer :: fluxes

  if (command_argument_count() < 4) then
    call usage()
    stop 1
  end if
  ! ECCKD_SOLVER_OPTION=name=value in the environment: one solver option set through the Fortran binding
  call get_environment_variable("ECCKD_SOLVER_OPTION", arg, status=i)
  if (i == 0 .and. len_trim(arg) > 0) then
    u = index(arg, "=")
    if (u < 2) call stop_on_err("ecckd_driver: ECCKD_SOLVER_OPTION must be name=value")
    read(arg(u + 1:), *, iostat=i) secs
    if (i /= 0) call stop_on_err("ecckd_driver: ECCKD_SOLVER_OPTION must be name=value")
    call stop_on_err(rte_set_solver_option(arg(1:u - 1), secs))
  end if
  call get_command_argument(1, mode)
  call get_command_argument(2, ecckd_path)
  call get_command_argument(3, in_path)
  call get_command_argument(4, out_path)
  block_size = 0
  n_quad_angles = 1
  if (command_argument_count() >= 5) then
    call get_command_argument(5, arg)
    read(arg, *) block_size
  end if
  if (command_argument_count() >= 6) then
    call get_command_argument(6, arg)
    read(arg, *) n_quad_angles
  end if
  dev_flag = 0
  if (command_argument_count() >= 7) then
    call get_command_argument(7, arg)
    read(arg, *) dev_flag
  end if
  repeats = 1
  if (command_argument_count() >= 8) then
    call get_command_argument(8, arg)
    read(arg, *) repeats
  end if
  byband = 0
  if (command_argument_count() >= 9) then
    call get_command_argument(9, arg)
    read(arg, *) byband
  end if
  if (command_argument_count() >= 10) then
    call get_command_argument(10, arg)
    read(arg, *) fused
  end if
  if (command_argument_count() >= 11) then
    call get_command_argument(11, part_path)
    allsky = len_trim(part_path) > 0
  end if
  if (command_argument_count() >= 12) then
    call get_command_argument(12, frac_path)
    mcica = len_trim(frac_path) > 0
  end if
  if (command_argument_count() >= 13) then
    call get_command_argument(13, clear_path)
    both = len_trim(clear_path) > 0
  end if
  if (command_argument_count() >= 14) then
    call get_command_argument(14, jac_path)
    with_jac = len_trim(jac_path) > 0
  end if
  if (with_jac .and. (trim(mode) /= "lw" .or. dev_flag /= 0)) then
    write(error_unit, "(a)") " ecckd_driver: a Jacobian output file needs the longwave and device_resident = 0"
    call usage()
    stop 1
  end if
  if (both .and. .not. (allsky .and. fused /= 0)) then
    write(error_unit, "(a)") " ecckd_driver: a clear-sky output file needs fused = 1 and a particle file (particles.bin)"
    call usage()
    stop 1
  end if
  if (mcica .and. .not. allsky) then
    write(error_unit, "(a)") " ecckd_driver: a cloud-fraction file needs a particle file (particles.bin)"
    call usage()
    stop 1
  end if
  if (allsky .and. fused == 0) then
    write(error_unit, "(a)") " ecckd_driver: a particle file needs fused = 1 (lw_fluxes_allsky / sw_fluxes_allsky)"
    call usage()
    stop 1
  end if
  if (byband /= 0) then
    fluxes => fluxes_band
  else
    fluxes => fluxes_bb
  end if
  lw = trim(mode) == "lw"
  if (dev_flag /= 0) then
    allocate(ty_source_func_lw_dev :: source)
    allocate(ty_optical_props_1scl_dev :: op1)
    allocate(ty_optical_props_2str_dev :: op2)
  else
    allocate(ty_source_func_lw :: source)
    allocate(ty_optical_props_1scl :: op1)
    allocate(ty_optical_props_2str :: op2)
  end if

  open(newunit=u, file=trim(in_path), access="stream", form="unformatted", status="old")
  read(u) ncol, nlay, ngas
  allocate(gas_names(ngas))
  read(u) gas_names
  allocate(plev(ncol, nlay + 1), tlev(ncol, nlay + 1), tlay(ncol, nlay), play(ncol, nlay), tsfc(ncol), &
           bc1(ncol), bc2(ncol), vmr(ncol, nlay, ngas))
  read(u) plev, tlev, tlay, tsfc
  if (lw) then
    read(u) bc1
  else
    read(u) bc1, bc2
  end if
  read(u) vmr
  close(u)
  play = 0.5_wp * (plev(:, 1:nlay) + plev(:, 2:nlay + 1))
  if (allsky) then
    open(newunit=u, file=trim(part_path), access="stream", form="unformatted", status="old")
    read(u) nband_p, has_ssa_g, delta_flag
    allocate(tau_p(ncol, nlay, nband_p))
    read(u) tau_p
    if (has_ssa_g /= 0) then
      allocate(ssa_p(ncol, nlay, nband_p), g_p(ncol, nlay, nband_p))
      read(u) ssa_p, g_p
    else if (.not. lw) then
      call stop_on_err("ecckd_driver: shortwave particles need ssa and g (has_ssa_g = 1)")
    end if
    close(u)
  end if
  if (mcica) then
    open(newunit=u, file=trim(frac_path), access="stream", form="unformatted", status="old")
    read(u) overlap, seed
    allocate(cloud_frac(ncol, nlay))
    read(u) cloud_frac
    if (overlap == ECCKD_OVERLAP_EXP_RAN) then
      allocate(overlap_param(ncol, max(nlay - 1, 0)))
      read(u) overlap_param
    end if
    close(u)
  end if
  if (block_size <= 0) block_size = ncol

  call stop_on_err(ecckd%load(trim(ecckd_path)))
  if (lw .neqv. ecckd%source_is_internal()) call stop_on_err("ecckd_driver: k-distribution file doesn't match lw/sw")
  nbnd = ecckd%get_nband()
  top_at_1 = play(1, 1) < play(1, nlay)                   ! ecckd_rfmip_lw.F90:85
  allocate(flux_up(ncol, nlay + 1), flux_dn(ncol, nlay + 1))
  if (both) allocate(clear_up(ncol, nlay + 1), clear_dn(ncol, nlay + 1))
  if (with_jac) allocate(jac_up(ncol, nlay + 1))
  nblocks = (ncol + block_size - 1) / block_size

  ! gas concentrations per block, as read_and_block_gases_ty prepares them before the reference's loop
  ! (mo_rfmip_io.F90:177-263); a field that is uniform goes in as a scalar, as RFMIP's well-mixed gases do
  allocate(gas_concs(nblocks))
  do b = 1, nblocks
    c0 = (b - 1) * block_size + 1
    c1 = min(ncol, b * block_size)
    call stop_on_err(gas_concs(b)%init(gas_names))
    do i = 1, ngas
      if (all(vmr(c0:c1, :, i) == vmr(c0, 1, i))) then
        call stop_on_err(gas_concs(b)%set_vmr(trim(gas_names(i)), vmr(c0, 1, i)))
      else
        call stop_on_err(gas_concs(b)%set_vmr(trim(gas_names(i)), vmr(c0:c1, :, i)))
      end if
    end do
  end do
  best = huge(1._wp)
  do rep = 1, max(1, repeats)
  call system_clock(t0, rate)
  do b = 1, nblocks
    c0 = (b - 1) * block_size + 1
    c1 = min(ncol, b * block_size)
    nc = c1 - c0 + 1
    fluxes%flux_up => flux_up(c0:c1, :)
    fluxes%flux_dn => flux_dn(c0:c1, :)
    if (byband /= 0) then
      if (allocated(bnd_up)) deallocate(bnd_up, bnd_dn)
      allocate(bnd_up(nc, nlay + 1, nbnd), bnd_dn(nc, nlay + 1, nbnd))
      fluxes_band%bnd_flux_up => bnd_up
      fluxes_band%bnd_flux_dn => bnd_dn
    end if
    if (allocated(sfc_spec)) deallocate(sfc_spec)
    allocate(sfc_spec(nbnd, nc))
    do i = 1, nc                                             ! ecckd_rfmip_lw.F90:112-116
      do ibnd = 1, nbnd
        sfc_spec(ibnd, i) = bc1(c0 + i - 1)
      end do
    end do
    if (mcica) then   ! the mask of a column depends on its global index, not on the blocking: col0 = c0 - 1
      if (allocated(mask_b)) deallocate(mask_b)
      allocate(mask_b(nc, nlay))
      if (overlap == ECCKD_OVERLAP_EXP_RAN) then
        call stop_on_err(ecckd%sample_cloud_mask(cloud_frac(c0:c1, :), int(overlap), seed, int(c0 - 1, int64), mask_b, &
                                                 overlap_param=overlap_param(c0:c1, :)))
      else
        call stop_on_err(ecckd%sample_cloud_mask(cloud_frac(c0:c1, :), int(overlap), seed, int(c0 - 1, int64), mask_b))
      end if
    end if
    if (with_jac) then
      if (allocated(jac_b)) deallocate(jac_b)
      allocate(jac_b(nc, nlay + 1))
    end if
    if (lw .and. both) then
      if (has_ssa_g /= 0) then
        call stop_on_err(ecckd%lw_fluxes_allsky(plev(c0:c1, :), tlay(c0:c1, :), tsfc(c0:c1), tlev(c0:c1, :), gas_concs(b), &
                                                top_at_1, sfc_spec, tau_p(c0:c1, :, :), flux_up(c0:c1, :), flux_dn(c0:c1, :), &
                                                ssa_p=ssa_p(c0:c1, :, :), n_gauss_angles=n_quad_angles, cloud_mask=mask_b, &
                                                flux_up_clear=clear_up(c0:c1, :), flux_dn_clear=clear_dn(c0:c1, :), &
                                                flux_up_Jac=jac_b))
      else
        call stop_on_err(ecckd%lw_fluxes_allsky(plev(c0:c1, :), tlay(c0:c1, :), tsfc(c0:c1), tlev(c0:c1, :), gas_concs(b), &
                                                top_at_1, sfc_spec, tau_p(c0:c1, :, :), flux_up(c0:c1, :), flux_dn(c0:c1, :), &
                                                n_gauss_angles=n_quad_angles, cloud_mask=mask_b, &
                                                flux_up_clear=clear_up(c0:c1, :), flux_dn_clear=clear_dn(c0:c1, :), &
                                                flux_up_Jac=jac_b))
      end if
    else if (lw .and. allsky) then
      if (has_ssa_g /= 0) then
        call stop_on_err(ecckd%lw_fluxes_allsky(plev(c0:c1, :), tlay(c0:c1, :), tsfc(c0:c1), tlev(c0:c1, :), gas_concs(b), &
                                                top_at_1, sfc_spec, tau_p(c0:c1, :, :), flux_up(c0:c1, :), flux_dn(c0:c1, :), &
                                                ssa_p=ssa_p(c0:c1, :, :), n_gauss_angles=n_quad_angles, cloud_mask=mask_b, &
                                                flux_up_Jac=jac_b))
      else
        call stop_on_err(ecckd%lw_fluxes_allsky(plev(c0:c1, :), tlay(c0:c1, :), tsfc(c0:c1), tlev(c0:c1, :), gas_concs(b), &
                                                top_at_1, sfc_spec, tau_p(c0:c1, :, :), flux_up(c0:c1, :), flux_dn(c0:c1, :), &
                                                n_gauss_angles=n_quad_angles, cloud_mask=mask_b, flux_up_Jac=jac_b))
      end if
    else if (lw .and. fused /= 0) then
      call stop_on_err(ecckd%lw_fluxes(plev(c0:c1, :), tlay(c0:c1, :), tsfc(c0:c1), tlev(c0:c1, :), gas_concs(b), top_at_1, &
                                       sfc_spec, flux_up(c0:c1, :), flux_dn(c0:c1, :), n_gauss_angles=n_quad_angles, &
                                       flux_up_Jac=jac_b))
    else if (lw) then
      if (nc /= nc_alloc) then                                 ! (the reference allocates once, before its loop: :102-103)
        call stop_on_err(source%alloc(nc, nlay, ecckd))
        call stop_on_err(op1%alloc_1scl(nc, nlay, ecckd))
        nc_alloc = nc
      end if
      call stop_on_err(ecckd%gas_optics(play(c0:c1, :), plev(c0:c1, :), tlay(c0:c1, :), tsfc(c0:c1), gas_concs(b), &
                                        op1, source, tlev=tlev(c0:c1, :)))
      ! ecckd level sources hold one value per level (src/gas_optics_ecckd.f90:419-424): each level is read once
      if (with_jac) call stop_on_err(ecckd%planck_sfc_source_jac(tsfc(c0:c1), source))
      call stop_on_err(rte_lw(op1, top_at_1, source, sfc_spec, fluxes, n_gauss_angles=n_quad_angles, &
                              lev_sources_shared=.true., flux_up_Jac=jac_b))
    else if (fused /= 0) then
      if (allocated(sfc_spec2)) deallocate(sfc_spec2)
      allocate(sfc_spec2(nbnd, nc))
      do i = 1, nc
        sfc_spec(:, i) = bc2(c0 + i - 1)                     ! albedo, direct = diffuse (ecckd_rfmip_sw.F90:136-141)
        sfc_spec2(:, i) = bc2(c0 + i - 1)
      end do
      if (both) then
        call stop_on_err(ecckd%sw_fluxes_allsky(plev(c0:c1, :), tlay(c0:c1, :), gas_concs(b), top_at_1, bc1(c0:c1), sfc_spec, &
                                                sfc_spec2, tau_p(c0:c1, :, :), ssa_p(c0:c1, :, :), g_p(c0:c1, :, :), &
                                                delta_flag /= 0, flux_up(c0:c1, :), flux_dn(c0:c1, :), cloud_mask=mask_b, &
                                                flux_up_clear=clear_up(c0:c1, :), flux_dn_clear=clear_dn(c0:c1, :)))
      else if (allsky) then
        call stop_on_err(ecckd%sw_fluxes_allsky(plev(c0:c1, :), tlay(c0:c1, :), gas_concs(b), top_at_1, bc1(c0:c1), sfc_spec, &
                                                sfc_spec2, tau_p(c0:c1, :, :), ssa_p(c0:c1, :, :), g_p(c0:c1, :, :), &
                                                delta_flag /= 0, flux_up(c0:c1, :), flux_dn(c0:c1, :), cloud_mask=mask_b))
      else
      call stop_on_err(ecckd%sw_fluxes(plev(c0:c1, :), tlay(c0:c1, :), gas_concs(b), top_at_1, bc1(c0:c1), sfc_spec, sfc_spec2, &
                                       flux_up(c0:c1, :), flux_dn(c0:c1, :)))
      end if
    else
      if (allocated(sfc_spec2)) deallocate(sfc_spec2)
      if (allocated(toa)) deallocate(toa)
      allocate(sfc_spec2(nbnd, nc), toa(nc, ecckd%get_ngpt()))
      do i = 1, nc
        sfc_spec(:, i) = bc2(c0 + i - 1)                     ! albedo, direct = diffuse (ecckd_rfmip_sw.F90:136-141)
        sfc_spec2(:, i) = bc2(c0 + i - 1)
      end do
      if (nc /= nc_alloc) then
        call stop_on_err(op2%alloc_2str(nc, nlay, ecckd))
        nc_alloc = nc
      end if
      call stop_on_err(ecckd%gas_optics(play(c0:c1, :), plev(c0:c1, :), tlay(c0:c1, :), gas_concs(b), op2, toa))
      call stop_on_err(rte_sw(op2, top_at_1, bc1(c0:c1), toa, sfc_spec, sfc_spec2, fluxes))
    end if
    if (with_jac) jac_up(c0:c1, :) = jac_b
    if (byband /= 0) then
      if (maxval(abs(sum(bnd_up, dim=3) - flux_up(c0:c1, :))) > 1.e-9_wp .or. &
          maxval(abs(sum(bnd_dn, dim=3) - flux_dn(c0:c1, :))) > 1.e-9_wp) &
        call stop_on_err("ecckd_driver: per-band fluxes do not add up to the broadband fluxes")
    end if
  end do
  call system_clock(t1)
  secs = real(t1 - t0, wp) / real(rate, wp)
  best = min(best, secs)
  end do
  write(error_unit, "(a,es12.5)") " ecckd_driver: loop_seconds ", best

  open(newunit=u, file=trim(out_path), access="stream", form="unformatted", status="replace")
  write(u) flux_up, flux_dn
  close(u)
  if (both) then
    open(newunit=u, file=trim(clear_path), access="stream", form="unformatted", status="replace")
    write(u) clear_up, clear_dn
    close(u)
  end if
  if (with_jac) then
    open(newunit=u, file=trim(jac_path), access="stream", form="unformatted", status="replace")
    write(u) jac_up
    close(u)
  end if
  call ecckd%finalize()
  write(error_unit, *) "ecckd_driver: ", ncol, " columns in ", nblocks, " blocks done"

contains
  subroutine usage()
    write(error_unit, "(a)") " usage: ecckd_driver lw|sw ecckd_file input.bin output.bin [block_size] [n_quad_angles]"
    write(error_unit, "(a)") "        [device_resident 0|1] [repeats] [byband 0|1] [fused 0|1] [particles.bin] [cloudfrac.bin]"
    write(error_unit, "(a)") "        [clear.bin: clear-sky fluxes of the same columns; needs fused = 1 and particles.bin]"
    write(error_unit, "(a)") "        [jac.bin: flux_up_jac of the same columns; longwave, device_resident = 0]"
  end subroutine usage

  subroutine stop_on_err(msg)                                ! mo_simple_netcdf.F90:331-339
    character(len=*), intent(in) :: msg
    if (len_trim(msg) > 0) then
      write(error_unit, *) trim(msg)
      stop 1
    end if
  end subroutine stop_on_err
end program ecckd_driver
