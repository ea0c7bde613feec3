! C entry points into the reference's gas-optics module, built unmodified against
! oracle/ref/rte_stubs.f90 (oracle/Makefile, target _ref/libecckd_ref.so).  TEST INFRASTRUCTURE
! ONLY: loaded by oracle/oracle.py (ref_gas_optics_int / ref_gas_optics_ext) and nothing else.
!
! One saved ty_gas_optics_ecckd is filled member by member with what load_and_init would leave
! in it (oracle.CkdModel restates that loader: netcdf-fortran is not needed), then driven through
! the type-bound generic gas_optics, exactly as a host program calls it.  Arrays are passed in
! Fortran order; every output is copied back to the caller, because the module reallocates the
! source arrays it is handed (calculate_planck_function's allocatable, intent(inout) argument).
module ecckd_ref_harness
  use, intrinsic :: iso_c_binding, only: c_int, c_double, c_char, c_null_char
  use mo_rte_kind, only: wp
  use mo_optical_props, only: ty_optical_props_1scl, ty_optical_props_2str
  use mo_source_functions, only: ty_source_func_lw
  use mo_gas_concentrations, only: ty_gas_concs
  use gas_optics_ecckd, only: ty_gas_optics_ecckd
  implicit none
  private

  type(ty_gas_optics_ecckd), save :: k

contains

  ! Start a model: grids, then Planck (longwave, ntp > 0) or solar and Rayleigh (shortwave, ntp = 0)
  ! tables.  Gases follow with ecckd_ref_add_gas, in the model's gas order.
  subroutine ecckd_ref_init(ng, np, nt, ntp, log_pressure, temperature, planck_function, &
                            temperature_planck, solar_irradiance, rayleigh) bind(C, name="ecckd_ref_init")
    integer(c_int), value, intent(in) :: ng, np, nt, ntp
    real(c_double), intent(in) :: log_pressure(np), temperature(np, nt)
    real(c_double), intent(in) :: planck_function(ng, *), temperature_planck(*)
    real(c_double), intent(in) :: solar_irradiance(*), rayleigh(*)
    integer :: i

    do i = 1, size(k%absorption)
      if (allocated(k%absorption(i)%coefficient)) deallocate(k%absorption(i)%coefficient)
      if (allocated(k%absorption(i)%mole_fraction)) deallocate(k%absorption(i)%mole_fraction)
    enddo
    if (allocated(k%gpoint_fraction)) deallocate(k%gpoint_fraction)
    if (allocated(k%planck_function)) deallocate(k%planck_function)
    if (allocated(k%temperature_planck)) deallocate(k%temperature_planck)
    if (allocated(k%solar_irradiance)) deallocate(k%solar_irradiance)
    if (allocated(k%rayleigh_molar_scattering_coeff)) deallocate(k%rayleigh_molar_scattering_coeff)
    k%gas(:) = ""
    k%num_gases = 0
    k%num_composite_gases = 0
    allocate(k%gpoint_fraction(1, ng))        ! only its second extent is read
    k%gpoint_fraction(:,:) = 0._wp
    k%log_pressure = log_pressure(1:np)
    k%temperature = temperature(1:np, 1:nt)
    k%shortwave = ntp == 0
    if (k%shortwave) then
      k%solar_irradiance = solar_irradiance(1:ng)
      k%rayleigh_molar_scattering_coeff = rayleigh(1:ng)
      k%total_solar_irradiance = sum(k%solar_irradiance)
    else
      k%planck_function = planck_function(1:ng, 1:ntp)
      k%temperature_planck = temperature_planck(1:ntp)
      k%total_solar_irradiance = 0._wp
    endif
  end subroutine ecckd_ref_init

  ! Append one AbsorptionTable.  coefficient is (ng, np, nt, nv); mole_fraction (nv) is read only
  ! for the look-up-table code.
  subroutine ecckd_ref_add_gas(name, ng, np, nt, nv, code, composite_only, coefficient, &
                               mole_fraction, reference_mole_fraction) bind(C, name="ecckd_ref_add_gas")
    character(kind=c_char), intent(in) :: name(32)
    integer(c_int), value, intent(in) :: ng, np, nt, nv, code, composite_only
    real(c_double), intent(in) :: coefficient(ng, np, nt, nv), mole_fraction(*)
    real(c_double), value, intent(in) :: reference_mole_fraction
    integer :: n

    n = k%num_gases + 1
    k%num_gases = n
    k%gas(n) = c_name(name)
    k%absorption(n)%coefficient = coefficient
    k%absorption(n)%composite_only = composite_only /= 0
    k%absorption(n)%concentration_dependence_code = code
    if (code == 2) k%absorption(n)%mole_fraction = mole_fraction(1:nv)
    k%absorption(n)%reference_mole_fraction = reference_mole_fraction
    if (composite_only /= 0) k%num_composite_gases = k%num_composite_gases + 1
  end subroutine ecckd_ref_add_gas

  ! get_press_min, get_press_max, get_temp_min, get_temp_max
  subroutine ecckd_ref_limits(out) bind(C, name="ecckd_ref_limits")
    real(c_double), intent(out) :: out(4)
    out = [k%get_press_min(), k%get_press_max(), k%get_temp_min(), k%get_temp_max()]
  end subroutine ecckd_ref_limits

  ! k%gas_optics(play, plev, tlay, tsfc, gas_desc, optical_props, sources[, tlev=tlev]).
  ! names is ngas blank- or NUL-padded 32-character names, vmr (ncol, nlay, ngas).
  subroutine ecckd_ref_gas_optics_int(ncol, nlay, ngas, names, vmr, plev, tlay, tsfc, has_tlev, tlev, &
                                      tau, lay_source, lev_source_inc, lev_source_dec, sfc_source, errmsg) &
                                      bind(C, name="ecckd_ref_gas_optics_int")
    integer(c_int), value, intent(in) :: ncol, nlay, ngas, has_tlev
    character(kind=c_char), intent(in) :: names(32, ngas)
    real(c_double), intent(in) :: vmr(ncol, nlay, ngas), plev(ncol, nlay + 1), tlay(ncol, nlay), tsfc(ncol)
    real(c_double), intent(in) :: tlev(ncol, nlay + 1)
    real(c_double), intent(inout) :: tau(ncol, nlay, *), lay_source(ncol, nlay, *)
    real(c_double), intent(inout) :: lev_source_inc(ncol, nlay, *), lev_source_dec(ncol, nlay, *)
    real(c_double), intent(inout) :: sfc_source(ncol, *)
    character(kind=c_char), intent(out) :: errmsg(129)
    type(ty_gas_concs) :: gc
    type(ty_optical_props_1scl) :: op
    type(ty_source_func_lw) :: src
    character(len=128) :: err
    integer :: ng

    ng = size(k%gpoint_fraction, 2)
    call fill_concs(gc, ncol, nlay, ngas, names, vmr)
    allocate(op%tau(ncol, nlay, ng))
    allocate(src%lay_source(ncol, nlay, ng), src%lev_source_inc(ncol, nlay, ng), &
             src%lev_source_dec(ncol, nlay, ng), src%sfc_source(ncol, ng))
    op%tau(:,:,:) = tau(:,:,1:ng)
    src%lay_source(:,:,:) = lay_source(:,:,1:ng)
    src%lev_source_inc(:,:,:) = lev_source_inc(:,:,1:ng)
    src%lev_source_dec(:,:,:) = lev_source_dec(:,:,1:ng)
    src%sfc_source(:,:) = sfc_source(:,1:ng)
    if (has_tlev /= 0) then
      err = k%gas_optics(play_of(plev), plev, tlay, tsfc, gc, op, src, tlev=tlev)
    else
      err = k%gas_optics(play_of(plev), plev, tlay, tsfc, gc, op, src)
    endif
    tau(:,:,1:ng) = op%tau
    lay_source(:,:,1:ng) = src%lay_source
    lev_source_inc(:,:,1:ng) = src%lev_source_inc
    lev_source_dec(:,:,1:ng) = src%lev_source_dec
    sfc_source(:,1:ng) = src%sfc_source
    call c_string(err, errmsg)
  end subroutine ecckd_ref_gas_optics_int

  ! k%gas_optics(play, plev, tlay, gas_desc, optical_props, toa_src) with a two-stream
  ! (two_stream /= 0) or a one-scalar optical_props.
  subroutine ecckd_ref_gas_optics_ext(ncol, nlay, ngas, names, vmr, plev, tlay, two_stream, &
                                      tau, ssa, g, toa_src, errmsg) bind(C, name="ecckd_ref_gas_optics_ext")
    integer(c_int), value, intent(in) :: ncol, nlay, ngas, two_stream
    character(kind=c_char), intent(in) :: names(32, ngas)
    real(c_double), intent(in) :: vmr(ncol, nlay, ngas), plev(ncol, nlay + 1), tlay(ncol, nlay)
    real(c_double), intent(inout) :: tau(ncol, nlay, *), ssa(ncol, nlay, *), g(ncol, nlay, *)
    real(c_double), intent(inout) :: toa_src(ncol, *)
    character(kind=c_char), intent(out) :: errmsg(129)
    type(ty_gas_concs) :: gc
    type(ty_optical_props_1scl) :: op1
    type(ty_optical_props_2str) :: op2
    real(wp), allocatable :: toa(:,:)
    character(len=128) :: err
    integer :: ng

    ng = size(k%gpoint_fraction, 2)
    call fill_concs(gc, ncol, nlay, ngas, names, vmr)
    toa = toa_src(:,1:ng)
    if (two_stream /= 0) then
      allocate(op2%tau(ncol, nlay, ng), op2%ssa(ncol, nlay, ng), op2%g(ncol, nlay, ng))
      op2%tau(:,:,:) = tau(:,:,1:ng)
      op2%ssa(:,:,:) = ssa(:,:,1:ng)
      op2%g(:,:,:) = g(:,:,1:ng)
      err = k%gas_optics(play_of(plev), plev, tlay, gc, op2, toa)
      tau(:,:,1:ng) = op2%tau
      ssa(:,:,1:ng) = op2%ssa
      g(:,:,1:ng) = op2%g
    else
      allocate(op1%tau(ncol, nlay, ng))
      op1%tau(:,:,:) = tau(:,:,1:ng)
      err = k%gas_optics(play_of(plev), plev, tlay, gc, op1, toa)
      tau(:,:,1:ng) = op1%tau
    endif
    toa_src(:,1:ng) = toa
    call c_string(err, errmsg)
  end subroutine ecckd_ref_gas_optics_ext

  subroutine fill_concs(gc, ncol, nlay, ngas, names, vmr)
    type(ty_gas_concs), intent(out) :: gc
    integer(c_int), intent(in) :: ncol, nlay, ngas
    character(kind=c_char), intent(in) :: names(32, ngas)
    real(c_double), intent(in) :: vmr(ncol, nlay, ngas)
    integer :: i
    allocate(gc%names(ngas))
    do i = 1, ngas
      gc%names(i) = c_name(names(:, i))
    enddo
    gc%vmr = vmr
  end subroutine fill_concs

  ! Layer pressures, which the module accepts and never reads.
  function play_of(plev) result(play)
    real(wp), intent(in) :: plev(:,:)
    real(wp) :: play(size(plev, 1), size(plev, 2) - 1)
    play = 0.5_wp*(plev(:, 1:size(plev, 2) - 1) + plev(:, 2:))
  end function play_of

  function c_name(s) result(name)
    character(kind=c_char), intent(in) :: s(32)
    character(len=32) :: name
    integer :: i
    name = ""
    do i = 1, 32
      if (s(i) == c_null_char) exit
      name(i:i) = s(i)
    enddo
  end function c_name

  subroutine c_string(s, out)
    character(len=*), intent(in) :: s
    character(kind=c_char), intent(out) :: out(len(s) + 1)
    integer :: i, n
    n = len_trim(s)
    do i = 1, n
      out(i) = s(i:i)
    enddo
    out(n + 1:) = c_null_char
  end subroutine c_string
end module ecckd_ref_harness
