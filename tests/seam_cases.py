"""The case tables of tests/test_gpu_allsky_seams.py and what can be said about them without a GPU (numpy and the oracle
only): layer counts, switch walks, the clouds and masks of a case, condition 1 (check_signal) and condition 2
(check_every_seam_is_covered).  tests/test_allsky_seams_host.py runs the same tables on the CPU."""
import numpy as np

import allsky_helpers as ah
import helpers
import seam_helpers as sh
from helpers import r32
from rte_ecckd_amd import synthetic

LW_NLAY = (1, 2, 3, 4, 5, 31, 32, 33, 48, 49, 59, 61, 64, 65, 80, 81, 96, 97, 98, 137)
SW_NLAY = (1, 2, 4, 5, 6, 9, 10, 11, 55, 56, 59, 60, 61, 62, 137)
JAC_NLAY = (1, 2, 3, 4, 5, 7, 61)
SCAT_NLAY = (60, 59, 61, 5)
TABLES = {"fsck": "lw_fsck", "rrtmgp": "lw_rrtmgp", "sw_wide": "sw_wide"}
NCOLS = (33, 65, 130)

_TABLES = {}


def table(which):
    """(band2gpt, ngpt) of the file, without a GPU."""
    if not _TABLES:
        _TABLES.update(ah.band_tables())
    return _TABLES[TABLES[which]]


def seams_of(kinds, nlay, top_at_1):
    return sorted(set().union(*[sh.seam_layers(kind, nlay, top_at_1) for kind in kinds]))


def seam_case(which, kinds, nlay, ncol, top_at_1, pattern="all"):
    """(seams, cloud, mask) of a case: a function of its arguments alone, so seam_coverage can rebuild it."""
    b2g, ng = table(which)
    seams = seams_of(kinds, nlay, top_at_1)
    seed = 1000 * nlay + 2 * ncol + int(top_at_1)
    return seams, sh.seam_clouds(b2g.shape[0], nlay, ncol, seams, pattern, seed), sh.seam_masks(nlay, ncol, ng, seams, seed + 1)


def differ_columns(cloud, mask, ngpt):
    """The columns whose all-sky fluxes have to differ from the clear sky: cloudy, and with a mask at least half of the
    g-points see one of the column's cloudy cells."""
    cell = cloud["tau"][0] > 0
    return (cell if mask is None else cell & sh.half_seen(mask, ngpt)).any(axis=0)


def check_signal(run, ref, cloud, seams, mask, ngpt, bar, what):
    """Condition 1; returns the smallest signal.  Every seam layer that carries a cloud in the case is measured; with a mask,
    every one on which at least half of the g-points of some column see the cloud (seam_helpers.layer_signals says why;
    check_every_seam_is_covered holds the union)."""
    sig = sh.layer_signals(run, cloud, seams, mask, ngpt, ref=ref)
    cell = cloud["tau"][0] > 0
    carried = [l for l in seams if (cell[l] if mask is None else cell[l] & sh.half_seen(mask, ngpt)[l]).any()]
    assert sorted(sig) == carried and (carried or cloud["tau"].shape[2] == 1), (what, sorted(sig), carried)
    low = min(sig.values()) if sig else np.inf
    assert low >= 20 * bar, (what, bar, sig)
    return low


# ------------------------------------------------------------------------------------------------
# the switch walks: every switch flips at least once per kernel form
# ------------------------------------------------------------------------------------------------
# (top_at_1, one_stream, n_gauss_angles, inc_flux, mask, "lw_series_terms", "lw_inc_flux_isotropic", "lw_tail_split")
LW_WALK = ((True, False, 1, False, False, 2, 0, 1), (False, True, 3, True, True, 3, 1, 0),
           (True, True, 1, True, True, 2, 0, 0), (False, False, 3, False, False, 3, 0, 1))
# (top_at_1, mask, inc_flux, n_gauss_angles) of the solvers with scattering; the two-stream solver runs where the angle is 1
SCAT_WALK = ((True, True, True, 1), (False, True, False, 1), (True, False, True, 3), (False, False, True, 1),
             (True, False, False, 1))
SPLIT_KINDS = ("lw_split60", "lw_jac")
JAC_KINDS = ("lw_jac", "lw_register")


def lw_general_cases(f32):
    """(nlay, ncol) of the register-resident solver; a single column once per form (padded 33, overflow 137, exact 60)."""
    for i, nlay in enumerate(LW_NLAY + ((60,) if f32 else ())):
        yield nlay, NCOLS[i % 3]
        if nlay in (33, 137, 60):
            yield nlay, 1


def scat_kinds(nlay):
    """One cloud serves both solvers.  The two-stream solver is rte_lw_2str_body at every layer count ("lw_2stream").  The
    rescaled solver runs in the layer-split kernels at 60 layers; elsewhere it is the per-g-point kernel of
    kernels_rte_gpt.hip on arrays already incremented, which reads no particles itself -- the register-resident
    solver's layers stand in there, so that first, last and a pair of inner layers stay cloudy."""
    return ("lw_split60" if nlay == 60 else "lw_register", "lw_2stream")


# (delta_scale, toa_scale, mask, "sw_tail_split", "sw_solver", top_at_1)
def sw_cases(nlay):
    walk = [(1, 0, 0, 1, 0, True), (0, 1, 1, 0, 0, True), (1, 1, 1, 1, 0, False), (0, 0, 0, 0, 0, False)]
    if nlay in (4, 10, 56, 60):   # the two-pass solver below 61 layers
        walk += [(1, 1, 1, 1, 1, True), (0, 0, 0, 0, 1, True), (0, 1, 1, 0, 1, False), (1, 0, 0, 1, 1, False)]
    return walk


def sw_ncol(nlay):
    """130 columns where the layer-systolic solver has more than 8 seam layers (one cloud per column: five per seam)."""
    return 130 if 21 <= nlay <= 60 else NCOLS[SW_NLAY.index(nlay) % 3]


SW_SHAPES = [(nlay, sw_ncol(nlay)) for nlay in SW_NLAY] + [(6, 1), (62, 1)]   # a single column once per solver
JAC_SHAPES = [(nlay, NCOLS[i % 3]) for i, nlay in enumerate(JAC_NLAY)] + [(7, 1)]
SCAT_SHAPES = [(nlay, NCOLS[i % 3]) for i, nlay in enumerate(SCAT_NLAY)] + [(59, 1)]


def sw_kind(nlay, solver):
    return "sw_systolic" if nlay <= 60 and solver == 0 else "sw_two_pass"


def sw_seam_case(nlay, ncol, solver, top_at_1, pattern=None):
    kind = sw_kind(nlay, solver)
    pattern = sh.signal_pattern(sh.seam_layers(kind, nlay, top_at_1)) if pattern is None else pattern
    seams, cloud, mask = seam_case("sw_wide", (kind,), nlay, ncol, top_at_1, pattern)
    return seams, {n: (r32(v) if v.dtype == np.float64 else v) for n, v in cloud.items()}, mask


# ------------------------------------------------------------------------------------------------
# float32 longwave against the oracle
# ------------------------------------------------------------------------------------------------
# one case per kernel form: padded to 32, 48, 64, 80 and 96 layers, the exact 60-layer form, the overflow form
F32_ORACLE = [("fsck", 31, True), ("rrtmgp", 33, False), ("fsck", 61, False), ("rrtmgp", 65, True), ("fsck", 81, True),
              ("rrtmgp", 60, False), ("fsck", 137, True), ("rrtmgp", 137, False)]


def f32_oracle_case(oracle_mod, m, press_min, which, nlay, top_at_1, ncol=33):
    """The case, its oracle reference on the float32-rounded inputs, the helpers.lw_f32_bar bar and the smallest seam-layer
    signal -- all without a GPU."""
    cols = synthetic.columns(3 + nlay, ncol, press_min, nlay=nlay)
    cols["emis"] = np.repeat(cols["sfc_emis"][:, None], m.band2gpt.shape[0], 1)
    seams, cloud, _ = seam_case(which, ("lw_register",), nlay, ncol, top_at_1)
    rc = {n: (r32(v) if isinstance(v, np.ndarray) and v.dtype == np.float64 else v) for n, v in cols.items()}
    rcl = {n: (r32(v) if v.dtype == np.float64 else v) for n, v in cloud.items()}
    run = sh.lw_reference(oracle_mod, m, rc, top_at_1=top_at_1)
    ref = run(rcl)
    items = helpers.oracle_gas_items(rc)
    tau, lay, inc, dec, sfc, _ = oracle_mod.gas_optics_int(m, rc["plev"], rc["tlay"], rc["tsfc"], items, rc["tlev"])
    tau, = ah.increment((tau,), (rcl["tau"], rcl["ssa"], rcl["g"]), m.band2gpt)
    case = dict(tau=tau, lay=lay, inc=inc, dec=dec, emis_gpt=np.repeat(rc["sfc_emis"][None, :], m.ng, 0), sfc=sfc)
    bar = helpers.lw_f32_bar(case, top_at_1, 1, ref)
    low = check_signal(run, ref, rcl, seams, None, m.ng, bar, (which, nlay, top_at_1))
    return cols, cloud, ref, bar, low


# ------------------------------------------------------------------------------------------------
# condition 2: every seam gets tested
# ------------------------------------------------------------------------------------------------
def module_cases():
    """(form, kind, which, kinds of the case, nlay, ncol, top_at_1, pattern, masked) of every case of the GPU module."""
    for f32 in (False, True):
        for nlay, ncol in lw_general_cases(f32):
            for which in ("fsck", "rrtmgp"):
                for v in LW_WALK:
                    yield ("lw f32" if f32 else "lw fp64", "lw_register", which, ("lw_register",), nlay, ncol, v[0], "all", v[4])
    for which in ("fsck", "rrtmgp"):
        for v in LW_WALK:
            for ncol in (1, 65):
                for kind in SPLIT_KINDS:
                    yield ("lw fp64 split", kind, which, SPLIT_KINDS, 60, ncol, v[0], "all", v[4])
                    yield ("lw fp64 split jacobian", kind, which, SPLIT_KINDS, 60, ncol, v[0], "one", v[4])
            for nlay, ncol in JAC_SHAPES:
                yield ("lw jacobian", "lw_jac", which, JAC_KINDS, nlay, ncol, v[0], "all", v[4])
    for nlay, ncol in SCAT_SHAPES:
        for top, masked, inc, nmus in SCAT_WALK:
            yield ("lw rescaled", scat_kinds(nlay)[0], "fsck", scat_kinds(nlay), nlay, ncol, top, "all", masked)
            if nmus == 1:
                yield ("lw two-stream", "lw_2stream", "fsck", scat_kinds(nlay), nlay, ncol, top, "all", masked)
    for nlay, ncol in SW_SHAPES:
        for delta, scale, masked, split, solver, top in sw_cases(nlay):
            kind = sw_kind(nlay, solver)
            yield ("sw fp64", kind, "sw_wide", (kind,), nlay, ncol, top, None, bool(masked))
            if ncol > 1:
                yield ("sw f32", kind, "sw_wide", (kind,), nlay, ncol, top, "one", bool(masked))


def seam_coverage():
    """{(form, kind, nlay, top_at_1): [seam layers, layers with a cloudy cell, ... a cleared bit, ... a set bit]} over
    module_cases()."""
    out = {}
    for form, kind, which, kinds, nlay, ncol, top, pattern, masked in module_cases():
        ng = table(which)[1]
        want = sh.seam_layers(kind, nlay, top)
        if pattern is None:
            pattern = sh.signal_pattern(want)
        seams, cloud, mask = seam_case(which, kinds, nlay, ncol, top, pattern)
        assert set(want) <= set(seams)
        got = sh.coverage(cloud, mask if masked else None, ng)
        entry = out.setdefault((form, kind, nlay, top), [want, set(), set(), set()])
        for s, layers in zip(entry[1:], got):
            s |= set(np.nonzero(layers)[0].tolist())
    return out


def check_every_seam_is_covered():
    """Condition 2, from the case tables alone: for every form, layer count and orientation the GPU module runs, the union
    over its cases puts a cloudy cell, a cleared mask bit on a cloudy cell and a set mask bit on a cloudy cell on every
    layer seam_helpers.seam_layers returns.  Returns seam_coverage()."""
    cov = seam_coverage()
    assert {k[1] for k in cov} == set(sh.KINDS)
    for key, (want, cell, cleared, kept) in cov.items():
        assert set(want) <= cell, (key, sorted(set(want) - cell))
        assert set(want) <= cleared, (key, "no cleared bit", sorted(set(want) - cleared))
        assert set(want) <= kept, (key, "no set bit", sorted(set(want) - kept))
    return cov
