// rte_lw_body.inc -- the body of the register-resident longwave solver, included into its kernels (kernels_rte_lw.hip:
// rte_lw_kernel, rte_lw_allsky_f32_kernel), which define `a`, real, NL, CW, EXACT, OVER, SHARED, SER3, OFF32 and ALLSKY.
  static_assert(NL > 0 && !(EXACT && OVER), "unrolled layer count; overflow only in the padded form");
  static_assert(!ALLSKY || (sizeof(real) == 4 && !SHARED), "the in-solver addition: single precision, two level arrays");
  static_assert(!OFF32 || EXACT, "32-bit offsets: exact layer count only");
  constexpr int kPF = prefetch_depth(NL);
  static_assert(kPF <= NL, "prefetch ring deeper than the unrolled layer count");
  constexpr int GW = 64 / CW;
  extern __shared__ __attribute__((aligned(16))) unsigned char acc_raw[];
  double *acc = reinterpret_cast<double *>(acc_raw);   // [2][nlay+1][CW], double in both precisions
  // RteLwArgs carries `double` pointers; in the single-precision instantiation they address float data
  auto P = [](const double *p) { return reinterpret_cast<const real *>(p); };
  auto Q = [](double *p) { return reinterpret_cast<real *>(p); };
  const int lane = threadIdx.x;
  const int cl = lane % CW, gs = lane / CW;
  const bool owner = gs == 0;
  const int ncol = a.ncol, nlay = a.nlay, ng = a.ng;
  const int nlev = nlay + 1;
  // (padded variants: one extra row per array, index nlev, swallows the absent layers' adds)
  constexpr bool PAD = !EXACT;
  const int nover = OVER ? (nlay > NL ? nlay - NL : 0) : 0;   // layers above the register-resident ones
  double *acc_dn = acc, *acc_up = acc + (nlev + (PAD ? 1 : 0)) * CW;
  // s < nlay with nlay read through an opaque asm (see the header comment)
  // index of the s_-th register-resident layer among all layers (opaque for the same reason)
  auto abs_layer = [&](int s_) {
    if (!OVER) return s_;
    int no = nover;
    asm volatile("" : "+s"(no));
    return no + s_;
  };
  auto present = [&](int s_) {
    int nl = nlay;
    asm volatile("" : "+s"(nl));
    return s_ < nl;
  };
  const real pi = (real)acos(-1.);
  const real tau_thresh = (real)a.tau_thresh;   // sqrt(epsilon(1._wp)) unless ecckd_set_solver_option moved it
  // layer / level walked s-th from the top lives at index l0 + s*lstep
  const long lay0 = a.top_at_1 ? 0 : nlay - 1, lev0 = a.top_at_1 ? 0 : nlay;
  const long lstep = a.top_at_1 ? 1 : -1;
  const real *Bdn = P(a.top_at_1 ? a.lev_source_inc : a.lev_source_dec);
  const real *Bup = P(a.top_at_1 ? a.lev_source_dec : a.lev_source_inc);
  [[maybe_unused]] const long lgs = a.lev_gstride ? (long)a.lev_gstride : (long)ncol * nlay;   // g-plane stride of Bdn / Bup (SHARED)
  const int ngroups = (ng + GW - 1) / GW;
  const int niter = ngroups * a.nmus;
  const long ntiles = ((long)ncol + CW - 1) / CW;

  // Work units: blocks [0, tail_first) take one whole tile (all g-pairs); beyond that a block takes ONE g-pair
  // iteration of a tail tile and leaves its sums in `partials` for rte_lw_tail_reduce (see launch_ser).
  const long tail_first = (OVER || a.tail_first < 0) ? ntiles : a.tail_first;
  const long nunits = tail_first + (ntiles - tail_first) * niter;
  for (long unit = blockIdx.x; unit < nunits; unit += gridDim.x) {
    long tile = unit;
    int it0 = 0, it1 = niter;
    if (!OVER && unit >= tail_first) {
      const long u = unit - tail_first;
      tile = tail_first + u / niter;
      it0 = (int)(u - (tile - tail_first) * niter);
      it1 = it0 + 1;
    }
    const long col = tile * CW + cl;
    const bool valid = col < ncol;
    const long cc = valid ? col : (long)ncol - 1;
    for (int i = lane; i < 2 * (nlev + (PAD ? 1 : 0)) * CW; i += 64) acc[i] = 0.;

    real T[NL], SU[NL];
    [[maybe_unused]] real *sT = nullptr, *sSU = nullptr;
    if constexpr (OVER) {
      sT = Q(a.scratch) + ((long)blockIdx.x * 2 * nover) * 64 + lane;
      sSU = sT + (long)nover * 64;
    }
    real ptau[kPF], play[kPF], pbdn[kPF];
    [[maybe_unused]] real pbup[SHARED ? 1 : kPF];
    [[maybe_unused]] real bup_first = real(0);   // SHARED: near-edge source of the first register-resident layer
    // ALLSKY: the band's tau_p / ssa_p and the mask half of the layers in flight, beside ptau.  Their element offsets are
    // tau's plus a constant of the pair: dqp to the band plane (dvp: the same in bytes, modulo 2^32, for OFF32), and for the
    // mask half 2 * (tau's offset) + dqm (dvm).  part_bit: the g-point's bit in its half.
    [[maybe_unused]] real pptau[ALLSKY ? kPF : 1], ppssa[ALLSKY ? kPF : 1];
    [[maybe_unused]] unsigned ppmk[ALLSKY ? kPF : 1];
    [[maybe_unused]] long dqp = 0, dqm = 0;
    [[maybe_unused]] unsigned dvp = 0, dvm = 0;
    [[maybe_unused]] const bool has_ssa = ALLSKY && a.part_ssa != nullptr, has_mask = ALLSKY && a.part_mask != nullptr;
    [[maybe_unused]] const unsigned *mask_b = reinterpret_cast<const unsigned *>(a.part_mask);

    // Element offset of the next layer to prefetch.  It is advanced step by step and made
    // opaque to the optimiser after every advance: otherwise the fully unrolled layer loop is
    // rewritten as base + s*step with 60 loop-invariant scalar offsets that spill the SGPR file.
    long qn = 0;
    const long qstep = (long)ncol * lstep;
    typedef __attribute__((address_space(1))) const char gcchar_t;
    typedef __attribute__((address_space(1))) const real greal_t;
    [[maybe_unused]] unsigned vo = 0;                                           // OFF32: byte offset of this lane's next request
    [[maybe_unused]] const unsigned vstep = (unsigned)((long)sizeof(real) * qstep);   // (wraps for bottom-up storage)
    [[maybe_unused]] const real *tau_b = nullptr, *lay_b = nullptr, *bdn_b = nullptr, *bup_b = nullptr;   // first plane of the group
    // SHARED: the level arrays have a g-plane stride of their own (RteLwArgs::lev_gstride: the two views of one level buffer
    // are (nlay+1)*ncol apart from plane to plane), so they get their own plane base and their own lane offset: `vol` beside
    // `vo`, or -- 64-bit form -- `ql` added to qn where a level is read.  Both advance by a layer like the others.
    [[maybe_unused]] unsigned vol = 0;
    [[maybe_unused]] long ql = 0;
    auto at32 = [&](const real *plane, unsigned off) -> real {
      return __builtin_nontemporal_load((greal_t *)((gcchar_t *)plane + off));
    };
    auto pair_start = [&](int it) {
      const int gb = (it / a.nmus) * GW;
      const int g = gb + gs;
      const int gg = g < ng ? g : ng - 1;
      if constexpr (ALLSKY) {
        const long band = a.gpt2band[gg];
        if constexpr (OFF32) {
          dvp = (unsigned)sizeof(real) * (unsigned)((long)ncol * nlay * (band - (gg - gb)));
          dvm = 4u * (unsigned)(gg >> 5) - 2u * (unsigned)sizeof(real) * (unsigned)((long)ncol * nlay * (gg - gb));
          asm volatile("" : "+v"(dvp), "+v"(dvm));
        } else {
          dqp = (long)ncol * nlay * (band - gg);
          dqm = (long)(gg >> 5) - 2 * (long)ncol * nlay * gg;
          asm volatile("" : "+v"(dqp), "+v"(dqm));
        }
      }
      if constexpr (OFF32) {
        const long pl = (long)ncol * nlay * gb;
        const long pll = SHARED ? lgs * gb : pl;
        tau_b = P(a.tau) + pl; lay_b = P(a.lay_source) + pl; bdn_b = Bdn + pll; bup_b = Bup + pll;
        vo = (unsigned)sizeof(real) * (unsigned)(cc + (long)ncol * nlay * (gg - gb) + (long)ncol * lay0);
        asm volatile("" : "+v"(vo));
        if (SHARED) {
          vol = (unsigned)sizeof(real) * (unsigned)(cc + lgs * (gg - gb) + (long)ncol * lay0);
          asm volatile("" : "+v"(vol));
          bup_first = at32(bup_b, vol);
        }
        return;
      }
      qn = cc + (long)ncol * nlay * gg + (long)ncol * (lay0 + lstep * nover);
      asm volatile("" : "+v"(qn));
      if (SHARED) {
        ql = (lgs - (long)ncol * nlay) * gg;
        asm volatile("" : "+v"(ql));
      }
      if (SHARED && !OVER) bup_first = __builtin_nontemporal_load(Bup + qn + ql);
    };
    // `sl` = layer being requested (compile-time in the unrolled code); in the padded variants the
    // offset stops advancing at the last real layer, so absent layers re-read it (finite data).
    auto issue = [&](int slot, int sl) {
      if constexpr (OFF32) {
        ptau[slot] = at32(tau_b, vo);
        play[slot] = at32(lay_b, vo);
        pbdn[slot] = at32(bdn_b, SHARED ? vol : vo);
        if (!SHARED) pbup[slot] = at32(bup_b, vo);
        if constexpr (ALLSKY) {
          // (plain loads, not nontemporal: the band planes are read by every g-point of the band)
          typedef __attribute__((address_space(1))) const unsigned guns_t;
          pptau[slot] = *(greal_t *)((gcchar_t *)P(a.part_tau) + (unsigned)(vo + dvp));
          ppssa[slot] = has_ssa ? *(greal_t *)((gcchar_t *)P(a.part_ssa) + (unsigned)(vo + dvp)) : real(0);
          ppmk[slot] = has_mask ? *(guns_t *)((gcchar_t *)mask_b + (unsigned)(2u * vo + dvm)) : ~0u;
        }
        vo += vstep;
        asm volatile("" : "+v"(vo));
        if (SHARED) {
          vol += vstep;
          asm volatile("" : "+v"(vol));
        }
        return;
      }
      // nontemporal: read-once streams
      ptau[slot] = __builtin_nontemporal_load(P(a.tau) + qn);
      play[slot] = __builtin_nontemporal_load(P(a.lay_source) + qn);
      pbdn[slot] = __builtin_nontemporal_load(Bdn + qn + (SHARED ? ql : 0L));
      if (!SHARED) pbup[slot] = __builtin_nontemporal_load(Bup + qn);
      if constexpr (ALLSKY) {   // (not nontemporal: the band planes are read by every g-point of the band)
        pptau[slot] = P(a.part_tau)[qn + dqp];
        ppssa[slot] = has_ssa ? P(a.part_ssa)[qn + dqp] : real(0);
        ppmk[slot] = has_mask ? mask_b[2 * qn + dqm] : ~0u;
      }
      if (!PAD || present(abs_layer(sl + 1))) qn += qstep;
      asm volatile("" : "+v"(qn));
    };
    // Same, but pinned into the recurrence: the empty asm also "modifies" the running
    // intensity, so the loads for layer s+kPF cannot be hoisted above layer s-1 (without this
    // the scheduler issues dozens of layers of loads up front and spills the register file).
    auto issue_after = [&](int slot, int sl, real &pin) {
      if constexpr (OFF32 && SHARED) asm volatile("" : "+v"(vo), "+v"(vol), "+v"(pin));
      else if constexpr (OFF32) asm volatile("" : "+v"(vo), "+v"(pin));
      else asm volatile("" : "+v"(qn), "+v"(pin));
      issue(slot, sl);
    };

    pair_start(it0);
#pragma unroll
    for (int s = 0; s < kPF; ++s) issue(s, s);

    for (int it = it0; it < it1; ++it) {
      const int gi = it / a.nmus, k = it - gi * a.nmus;
      const int g = gi * GW + gs;
      const bool gact = g < ng;
      const int gg = gact ? g : ng - 1;
      const long base = cc + (long)ncol * nlay * gg;
      const real D = (real)a.Ds[k];
      const real wfac = gact ? real(2) * pi * (real)a.wts[k] : real(0);
      const real eps = P(a.sfc_emis)[a.gpt2band[gg] + (long)a.nband * cc];
      const real sfc_src = P(a.sfc_source)[cc + (long)ncol * gg];
      // ALLSKY: the cell's optical depth -- tau + tp * (1 - sp), tp = 0 where the g-point's mask bit is clear
      [[maybe_unused]] const unsigned part_bit = 1u << (gg & 31);
      [[maybe_unused]] auto with_particles = [&](real tau, real tp, real sp, unsigned half) {
        const real t2 = (half & part_bit) ? tp : real(0);
        const real tabs = t2 * (real(1) - sp);
        return tau + tabs;
      };

      // ---------------- down sweep ----------------
      // radn_dn(top): no incident diffuse flux, or inc_flux turned into an intensity (SURVEY Appendix B.1)
      real I = real(0);
      if (a.inc_flux) {
        const real f = P(a.inc_flux)[cc + (long)ncol * gg];
        I = a.inc_isotropic ? f / pi : f / (real(2) * pi * (real)a.wts[k]);
      }
      auto layer = [&](int s, real tau, real lay, real bdn, real bup, real &t_out,
                       real &su_out) {
        const bool act = !PAD || present(s);
        if (PAD) tau = act ? tau : real(0);   // absent layer: trans = 1, both sources 0
        const real tl = tau * D;
        real t, sdn, su;
        lw_layer_source<SER3>(tl, tau_thresh, lay, bdn, bup, t, sdn, su);   // (lw_layer.hpp; source_up is materialised there)
        su_out = su;
        t_out = t;
        const real v = gsum<real, CW>(wfac * I);
        acc_add(&acc_dn[(act ? s : nlev) * CW + cl], v, owner);
        I = t * I + sdn;
      };
      [[maybe_unused]] real carry = bup_first;   // SHARED: far-edge source of the layer above
      if constexpr (OVER) {   // the layers above the register-resident ones: plain loads, scratch ring
        for (int s = 0; s < nover; ++s) {
          const long q = base + (long)ncol * (lay0 + lstep * s);
          const long qlev = SHARED ? q + (lgs - (long)ncol * nlay) * gg : q;
          const real bdn = Bdn[qlev];
          const real bup = (SHARED && s > 0) ? carry : Bup[qlev];
          real t, su;
          real tau_q = P(a.tau)[q];
          if constexpr (ALLSKY)
            tau_q = with_particles(tau_q, P(a.part_tau)[q + dqp], has_ssa ? P(a.part_ssa)[q + dqp] : real(0),
                                   has_mask ? mask_b[2 * q + dqm] : ~0u);
          layer(s, tau_q, P(a.lay_source)[q], bdn, bup, t, su);
          carry = bdn;
          sT[(long)s * 64] = t;
          sSU[(long)s * 64] = su;
        }
      }
#pragma unroll
      for (int s = 0; s < NL; ++s) {
        real tau = ptau[s % kPF];
        const real lay = play[s % kPF], bdn = pbdn[s % kPF];
        const real bup = SHARED ? carry : pbup[s % kPF];
        if constexpr (ALLSKY) tau = with_particles(tau, pptau[s % kPF], ppssa[s % kPF], ppmk[s % kPF]);
        if (s + kPF < NL) issue_after(s % kPF, s + kPF, I);
        layer(abs_layer(s), tau, lay, bdn, bup, T[s], SU[s]);
        if (SHARED) carry = bdn;
        if (s % kSchedSpan == kSchedSpan - 1) __builtin_amdgcn_sched_barrier(0);
      }
      // the next pair's first register-resident layers start streaming while the up sweep runs
      if (it + 1 < it1) {
        pair_start(it + 1);
#pragma unroll
        for (int s = 0; s < kPF; ++s) issue(s, s);
      }
      {
        const real v = gsum<real, CW>(wfac * I);
        acc_add(&acc_dn[nlay * CW + cl], v, owner);
      }
      // ---------------- surface + up sweep ----------------
      real U = I * (real(1) - eps) + eps * sfc_src;
      auto up = [&](int s, real t, real su) {
        const real v = gsum<real, CW>(wfac * U);
        acc_add(&acc_up[((!PAD || present(s)) ? s + 1 : nlev) * CW + cl], v, owner);
        U = t * U + su;
      };
#pragma unroll
      for (int s = NL - 1; s >= 0; --s) up(abs_layer(s), T[s], SU[s]);
      if constexpr (OVER) {
        for (int s = nover - 1; s >= 0; --s) up(s, sT[(long)s * 64], sSU[(long)s * 64]);
      }
      {
        const real v = gsum<real, CW>(wfac * U);
        acc_add(&acc_up[cl], v, owner);
      }
    }

    if (!OVER && unit >= tail_first) {   // one g-pair iteration of a tail tile: [unit][dn, up][nlev][CW]
      double *pp = a.partials + (unit - tail_first) * 2 * nlev * CW;
      for (int s = gs; s < nlev; s += GW) {
        pp[s * CW + cl] = acc_dn[s * CW + cl];
        pp[(nlev + s) * CW + cl] = acc_up[s * CW + cl];
      }
    } else
    // broadband fluxes: level s-th from the top -> lev0 + lstep*s
    if (valid) {
      for (int s = gs; s < nlev; s += GW) {
        const long q = col + (long)ncol * (lev0 + lstep * s);
        Q(a.flux_dn)[q] = (real)acc_dn[s * CW + cl];
        Q(a.flux_up)[q] = (real)acc_up[s * CW + cl];
      }
    }
  }
