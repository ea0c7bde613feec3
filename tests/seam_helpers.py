"""Clouds and McICA masks on the layers where the flux solvers change hands (numpy only).

synthetic.clouds puts particles into two slabs in the middle of the grid, so the first and the last layer of every column
and most of the layers listed below never see a particle or a cleared mask bit.  The generators here put them there and
nowhere else.

The seam layers, as read from the kernels (rte-ecckd_amd/csrc; "walked s" = the s-th layer in the solver's walking order):

  "lw_register"  rte_lw_body.inc (rte_lw_kernel, rte_lw_allsky_f32_kernel).  helpers.lw_seam_layers: the first walked layer,
                 the last present layer of a padded form (kernels_rte_lw.hip:191-197: NL = 32, 48, 64, 80, 96; 60 is exact),
                 walked nover - 1 | nover of the overflow form (rte_lw_body.inc:21, nover = nlay - 96; the ring loop :240-249
                 adds the particles by its own expression).  The prefetch prologue `for s < kPF: issue(s, s)`
                 (rte_lw_body.inc:188) hands over to issue_after (:262) between walked kPF - 1 and kPF, kPF =
                 prefetch_depth(NL) = 4 for NL = 96, else ECCKD_LW_PF = 8 (kernels_rte_lw.hip:49-60); in the overflow form the
                 prologue loads the register layers, walked nover .. nover + kPF - 1.
  "lw_split60"   kernels_rte_lw_split.hip: every form that takes particles is the Planck-recomputing one, 15 layers per
                 wave and 4 waves (launch_seg :735-742, launch_both :767-771, launch_jac_inline :777-785, kRescSeg = 15 :603),
                 kSplitPF = split_pf(true) = ECCKD_SPLIT_PF_PLANCK = 2 layers in flight (:37-41, :118; prologue :233, refill
                 :295-297).  Per segment: its first layer, walked s0 + kSplitPF - 1 | s0 + kSplitPF, and its last layer.
  "sw_systolic"  kernels_rte_sw_sys.hip: wave w owns the layers walked 5 w .. 5 w + 4 (kSysLPW = ECCKD_SYS_LPW = 5 :42-46,
                 s0 = w * LPW and nl :176-178); the last owning wave holds 1 .. 5 layers.  First and last layer of every wave.
  "sw_two_pass"  kernels_rte_sw.hip, rte_sw_body: two passes over the layers, each with a prologue of PF layers in flight
                 and a refill behind it.  PF = 2 in every all-sky (and every float32 fused) instantiation, PF = kPF =
                 ECCKD_SW_PF = 3 in the plain rte_sw of the composed route (:57-59, :96).  Pass 1 walks surface -> top: its
                 prologue fetches the PF lowest layers (:196) and the refill the layer PF above the one at hand (:204; the
                 partial group :217-219).  Pass 2 walks top -> surface: prologue on the PF topmost layers (:235-239), refill
                 clamped at the last layer (:246-248).  The hand-overs are PF - 1 | PF from either end: counted from the
                 top 0, 1 | 2 and 2 | 3, and nlay-4 | nlay-3, nlay-3 | nlay-2, nlay-1.
  "lw_2stream"   kernels_rte_lw_2str.hip, rte_lw_2str_body: the same two passes; PF = 2 with particles (the fused
                 lw_fluxes_allsky(use_2stream=True)), 3 without (the composed route's solver) (:56); prologues :128-131
                 (surface end) and :166-170 (top), refills :136 and :176-178.  The same layers as "sw_two_pass".
  "lw_jac"       kernels_rte_lw_jac.hip: walks upwards from the surface (:59-61) with kJacPF = 4 layers in flight (:40; prologue
                 :130, blocks of PF :133-137): walked 0, PF - 1 | PF, the first layer of the last block of PF, and the last.

Every kind includes the first and the last array layer."""
import numpy as np

import allsky_helpers as ah
import helpers
import mcica_helpers as mh

LW_PF, LW_PF_96 = 8, 4
SPLIT_SEG, SPLIT_WAVES, SPLIT_PF = 15, 4, 2
SYS_LPW, SYS_WAVES = 5, 12
TWO_PASS_PF = (2, 3)   # with particles in the prefetch slot, without
JAC_PF = 4
KINDS = ("lw_register", "lw_split60", "sw_systolic", "sw_two_pass", "lw_jac", "lw_2stream")
MASK_PATTERNS = ("ones", "zero", "bit0", "last_bit", "upper_half", "alternating")


def seam_layers(kind, nlay, top_at_1):
    """Sorted array indices of the seam layers of the solver form `kind` at `nlay` layers (module docstring)."""
    assert kind in KINDS, kind
    down = lambda s: s if top_at_1 else nlay - 1 - s        # walked s-th from the top -> array index
    walked = [0, nlay - 1]
    at = down
    if kind == "lw_register":
        out = list(helpers.lw_seam_layers(nlay, top_at_1))
        over = nlay > helpers.LW_MAX_REGISTER_LAYERS
        pf = LW_PF_96 if nlay > 80 else LW_PF
        walked += [pf - 1, pf]
        if over:
            nover = nlay - helpers.LW_MAX_REGISTER_LAYERS
            walked += [nover + pf - 1, nover + pf]
        return sorted(set(out) | {at(s) for s in walked if 0 <= s < nlay})
    if kind == "lw_split60":
        assert nlay == SPLIT_SEG * SPLIT_WAVES
        for w in range(SPLIT_WAVES):
            s0 = w * SPLIT_SEG
            walked += [s0, s0 + SPLIT_PF - 1, s0 + SPLIT_PF, s0 + SPLIT_SEG - 1]
    elif kind == "sw_systolic":
        assert nlay <= SYS_LPW * SYS_WAVES
        for s0 in range(0, nlay, SYS_LPW):
            walked += [s0, min(s0 + SYS_LPW, nlay) - 1]
    elif kind in ("sw_two_pass", "lw_2stream"):
        for pf in TWO_PASS_PF:                              # pass 2 from the top, pass 1 from the surface
            walked += [pf - 1, pf, nlay - pf, nlay - 1 - pf]
    else:
        at = lambda s: nlay - 1 - down(s)                   # walked s-th from the surface
        walked += [JAC_PF - 1, JAC_PF, (nlay - 1) // JAC_PF * JAC_PF]
    return sorted({at(s) for s in walked if 0 <= s < nlay})


def seam_clouds(nband, nlay, ncol, seams, pattern, seed):
    """dict tau, ssa, g (nband, nlay, ncol) float64 and cloudy (ncol,) bool.  tau_p ~ U(0.5, 3) on seam layers and +0
    elsewhere; ssa_p in [0.6, 1) and g_p in [0.7, 0.9) are random in every cell.  "all": every seam layer of every odd column
    (even columns are clear; a single column is cloudy); "one": column c has its cloud on seams[c % len(seams)] only."""
    assert pattern in ("all", "one") and len(seams) > 0
    rng = np.random.default_rng(seed)
    seams = np.asarray(seams)
    on = np.zeros((nlay, ncol), bool)
    col = np.arange(ncol)
    if pattern == "all":
        cloudy = (col % 2 == 1) | (ncol == 1)
        on[np.ix_(seams, np.nonzero(cloudy)[0])] = True
    else:
        cloudy = np.ones(ncol, bool)
        on[seams[col % len(seams)], col] = True
    tau = np.where(on[None], rng.uniform(0.5, 3.0, (nband, nlay, ncol)), 0.0)
    ssa = rng.uniform(0.6, 0.999, (nband, nlay, ncol))
    g = rng.uniform(0.7, 0.9, (nband, nlay, ncol))
    return dict(tau=np.ascontiguousarray(tau), ssa=ssa, g=g, cloudy=cloudy)


def signal_pattern(seams):
    """The cloud pattern under which every seam layer keeps a signal in a quantity that has to cross all the clouds -- the
    shortwave fluxes below them, the surface-temperature Jacobian above them: "all" up to 8 seam layers; beyond (the
    layer-systolic solver from 21 layers up has two seams per wave, the 60-layer longwave kernels 17) "one", because
    twenty-odd layers of tau_p ~ 1.75 leave the far side in the dark (removing the lowest cloud moves the shortwave oracle
    by 5e-9 W m-2 at 59 layers, removing the highest one the Jacobian at the top by 9e-9 W m-2 K-1 at 60)."""
    return "all" if len(seams) <= 8 else "one"


def mask_word(pattern, ngpt):
    """The 64-bit word of one of MASK_PATTERNS for a table of ngpt g-points (no bit at or above ngpt is set; with at most
    32 g-points "upper_half" is the zero word)."""
    full = 2 ** ngpt - 1
    return {"ones": full, "zero": 0, "bit0": 1, "last_bit": 1 << (ngpt - 1), "upper_half": full & ~(2 ** 32 - 1),
            "alternating": full & 0x5555555555555555}[pattern]


def seam_pattern(i, c):
    """Index into MASK_PATTERNS of column c on the i-th seam layer: pairs of columns share a pattern, so the odd columns
    (the cloudy ones of pattern "all") walk through all six, and every seam layer starts at another one; the c // 13 term
    keeps the columns i, i + n, i + 2 n, ... (the cloudy ones of seam i under pattern "one") from meeting one pattern only
    when 12 divides n."""
    return (c // 2 + c // 13 + i) % len(MASK_PATTERNS)


def seam_masks(nlay, ncol, ngpt, seams, seed):
    """(nlay, ncol) uint64, a function of its arguments alone: random words (bits below ngpt) off the seam layers; on the
    i-th seam layer column c holds mask_word(MASK_PATTERNS[seam_pattern(i, c)])."""
    rng = np.random.default_rng(seed)
    hi = rng.integers(0, 2 ** 32, (nlay, ncol), dtype=np.uint64)
    lo = rng.integers(0, 2 ** 32, (nlay, ncol), dtype=np.uint64)
    mask = ((hi << np.uint64(32)) | lo) & np.uint64(2 ** ngpt - 1)
    for i, l in enumerate(seams):
        for c in range(ncol):
            mask[l, c] = np.uint64(mask_word(MASK_PATTERNS[seam_pattern(i, c)], ngpt))
    return mask


def coverage(cloud, mask, ngpt):
    """Per layer (three bool arrays of nlay): a cloudy cell; a cloudy cell with a cleared bit below ngpt; a cloudy cell with a
    set bit.  mask None: no bit is ever cleared, every bit is set."""
    cell = cloud["tau"][0] > 0
    if mask is None:
        return cell.any(axis=1), np.zeros(cell.shape[0], bool), cell.any(axis=1)
    full = np.uint64(2 ** ngpt - 1)
    m = np.asarray(mask, dtype=np.uint64) & full
    return cell.any(axis=1), (cell & (m != full)).any(axis=1), (cell & (m != 0)).any(axis=1)


def half_seen(mask, ngpt):
    """bool, the mask's shape: at least half of the ngpt g-points have their bit set."""
    nset = ((np.asarray(mask, dtype=np.uint64)[..., None] >> np.arange(ngpt, dtype=np.uint64)) & np.uint64(1)).sum(axis=-1)
    return 2 * nset >= ngpt


def without_layer(cloud, l):
    """The cloud with the particles of array layer l removed."""
    tau = cloud["tau"].copy()
    tau[:, l, :] = 0.0
    return dict(cloud, tau=tau)


def layer_signals(run, cloud, seams, mask=None, ngpt=None, ref=None):
    """Condition 1: for every seam layer, the smallest over the columns that carry a cloud there of the largest flux
    change (over levels and flux arrays) when that layer's particles are removed.  run(cloud) -> list of (nlay+1, ncol)
    reference fluxes.  With a mask the columns are those in which at least half of the g-points see the layer's cloud (the
    words "ones" and "alternating").  The other words probe the choice of the bit: a cell whose word is zero equals its clear
    cell, and under a one-bit word a single g-point of 27 to 36 carries the cloud, which moves the broadband flux by as
    little as 1e-8 W m-2 -- but a kernel that picks another bit, word half or layer for that cell turns the cloud on in the
    other g-points, and that error is the removal signal measured here on the neighbouring columns.
    Returns {layer: W m-2}."""
    ref = run(cloud) if ref is None else ref
    out = {}
    for l in seams:
        has = cloud["tau"][0, l] > 0
        if mask is not None:
            has = has & half_seen(mask, ngpt)[l]
        if not has.any():
            continue
        other = run(without_layer(cloud, l))
        change = np.max([np.abs(a - b).max(axis=0) for a, b in zip(ref, other)], axis=0)
        out[int(l)] = float(change[has].min())
    return out


# ------------------------------------------------------------------------------------------------
# references: the C oracle (passed in as `oracle_mod`) on gas optics computed once and incremented in numpy
# ------------------------------------------------------------------------------------------------
def lw_reference(oracle_mod, m, cols, mask=None, one_stream=False, top_at_1=True, nmus=1, inc_flux=None, options=None):
    """run(cloud) -> [up, dn] of oracle.rte_lw on the oracle's gas optics (computed once) incremented in numpy."""
    items = helpers.oracle_gas_items(cols)
    tau, lay, inc, dec, sfc, oerr = oracle_mod.gas_optics_int(m, cols["plev"], cols["tlay"], cols["tsfc"], items, cols["tlev"])
    assert oerr == ""
    emis = np.repeat(cols["sfc_emis"][None, :], m.ng, 0)

    def run(cloud):
        t = tau
        if cloud is not None:
            tp = ah.spread(cloud["tau"], m.band2gpt, m.ng) if mask is None else mh.masked_tau(cloud["tau"], mask, m.band2gpt, m.ng)
            op2 = (tp,) if one_stream else (tp, ah.spread(cloud["ssa"], m.band2gpt, m.ng), ah.spread(cloud["g"], m.band2gpt, m.ng))
            t, = ah.increment((tau,), op2)
        return list(oracle_mod.rte_lw(t, lay, inc, dec, emis, sfc, top_at_1=top_at_1, nmus=nmus, inc_flux=inc_flux,
                                      options=options))
    run.tau = tau
    return run


def sw_reference(oracle_mod, m, cols, delta=True, mask=None, top_at_1=True, scale=None):
    """run(cloud) -> [up, dn, dir] of oracle.rte_sw on the oracle's gas optics (computed once) incremented in numpy by the
    (delta-scaled, masked) band optics: ah.oracle_sw_allsky / test_gpu_mcica.py's oracle_sw_masked."""
    items = helpers.oracle_gas_items(cols, helpers.SW_NAMES)
    otau, ossa, og, otoa, oerr = oracle_mod.gas_optics_ext(m, cols["plev"], cols["tlay"], items)
    assert oerr == ""
    if scale is not None:
        otoa = otoa * scale[None, :]
    g2b = m.gpt2band - 1
    alb = [np.ascontiguousarray(cols[n][:, g2b].T) for n in ("alb_dir", "alb_dif")]

    def run(cloud):
        op = (otau, ossa, og)
        if cloud is not None:
            part = (cloud["tau"], cloud["ssa"], cloud["g"])
            if delta:
                part = ah.delta_scale(*part)
            tp = ah.spread(part[0], m.band2gpt, m.ng) if mask is None else mh.masked_tau(part[0], mask, m.band2gpt, m.ng)
            op = ah.increment(op, (tp, ah.spread(part[1], m.band2gpt, m.ng), ah.spread(part[2], m.band2gpt, m.ng)))
        return list(oracle_mod.rte_sw(op[0], op[1], op[2], cols["mu0"], otoa, alb[0], alb[1], top_at_1=top_at_1))
    return run
