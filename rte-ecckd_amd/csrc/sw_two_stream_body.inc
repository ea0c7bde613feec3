// body of two_stream (sw_two_stream.hpp): sw_two_stream of RTE-RRTMGP for one cell, every product and sum rounded on its
// own in the order the reference spells.
  const real gq = G0 ? real(0) : gq_in;
  const real eps = sw_eps<real>();
  const real gamma1 = (real(8) - w0 * (real(5) + real(3) * gq)) * real(.25);
  const real gamma2 = real(3) * (w0 * (real(1) - gq)) * real(.25);
  const real gamma3 = G0 ? real(.5) : (real(2) - real(3) * mu0 * gq) * real(.25);
  const real gamma4 = G0 ? real(.5) : real(1) - gamma3;
  const real alpha1 = gamma1 * gamma4 + gamma2 * gamma3;
  const real alpha2 = G0 ? alpha1 : gamma1 * gamma3 + gamma2 * gamma4;   // (G0: the same products, the sum commutes)
  const real kk0 = (gamma1 - gamma2) * (gamma1 + gamma2);
  // k_floor = 1e-12 unless ecckd_set_solver_option moved it.  Single precision with the default (k_floor_tau > 0; capi.cpp,
  // rte_sw_impl): the bound of a cell is min(k_floor, k_floor_tau / tau^2), at least 1e-12 -- k tau stays at 1e-2 in a thick
  // cell instead of growing with tau.  (tau = 0 or NaN: k_floor; tau^2 = inf: 1e-12.)
  real kf = k_floor;
  if (sizeof(real) == 4 && k_floor_tau > real(0)) kf = fmax(real(1e-12), fmin(k_floor, k_floor_tau / (tau * tau)));
  const real k = sw_sqrt<FAST>(kk0 > kf ? kk0 : kf);
  const real exp_minusktau = sw_exp<FAST>(-tau * k);
  const real exp_minus2ktau = exp_minusktau * exp_minusktau;
  real RT_term = rcp<FAST>(k * (real(1) + exp_minus2ktau) + gamma1 * (real(1) - exp_minus2ktau));
  TwoStreamT<real> r;
  r.Rdif = RT_term * gamma2 * (real(1) - exp_minus2ktau);
  r.Tdif = RT_term * real(2) * k * exp_minusktau;
  r.Tnoscat = sw_exp<FAST>(-tau * mu0_inv);
  const real k_mu = k * mu0, k_gamma3 = k * gamma3, k_gamma4 = G0 ? k_gamma3 : k * gamma4;
  const real d = real(1) - k_mu * k_mu;
  if (FAST) RT_term = w0 * RT_term * rcp<true>(fabs(d) >= eps ? d : eps);
  else RT_term = w0 * RT_term / (fabs(d) >= eps ? d : eps);
  r.Rdir = RT_term * ((real(1) - k_mu) * (alpha2 + k_gamma3) - (real(1) + k_mu) * (alpha2 - k_gamma3) * exp_minus2ktau -
                      real(2) * (k_gamma3 - alpha2 * k_mu) * exp_minusktau * r.Tnoscat);
  r.Tdir = -RT_term * ((real(1) + k_mu) * (alpha1 + k_gamma4) * r.Tnoscat -
                       (real(1) - k_mu) * (alpha1 - k_gamma4) * exp_minus2ktau * r.Tnoscat -
                       real(2) * (k_gamma4 + alpha1 * k_mu) * exp_minusktau);
  if (CLAMP) {   // later RTE-RRTMGP releases: the direct beam can neither gain energy nor go negative
    const real lim = real(1) - r.Tnoscat;
    r.Rdir = fmax(real(0), fmin(r.Rdir, lim));
    r.Tdir = fmax(real(0), fmin(r.Tdir, lim - r.Rdir));
  }
  return r;
