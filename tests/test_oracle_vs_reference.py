"""CPU tests: the C oracle (oracle/ecckd_oracle.c) against the reference's own gas-optics module,
src/gas_optics_ecckd.f90 compiled unmodified into oracle/_ref/libecckd_ref.so by
oracle.build_ref() (oracle/Makefile; stand-ins for the RTE-RRTMGP modules it uses in
oracle/ref/rte_stubs.f90, entry points in oracle/ref/ref_harness.f90).

Both sides are fp64 with contraction off and call the same libm exp/log, so they must agree
bit for bit: every output is compared on its uint64 view, NaN cells included.  A mismatch is a
misreading of the reference by the oracle -- and, through the oracle, possibly by the HIP kernels.

What this does not pin: the loader.  Both sides are filled from oracle.CkdModel, the Python
restatement of load_and_init (mo_load_coefficients.F90), because that routine needs
netcdf-fortran; test_capi_host.py::test_load_matches_reference_loader_restatement checks the
product's loader against the same restatement.  The solvers stay unpinned (RTE-RRTMGP is absent).

NaN inputs are left out on purpose: the reference turns 1 + max(0, min(NaN, ...)) into a table
index with no guard and may read outside its tables.  The oracle-versus-GPU tests cover NaN.
"""
import json
import math
import os

import numpy as np
import pytest

import helpers
from conftest import LW_FSCK, LW_RRTMGP, SW_WIDE
from rte_ecckd_amd import synthetic
from test_oracle import kat_inputs

HERE = os.path.dirname(os.path.abspath(__file__))
LW_OUT = ("tau", "lay_source", "lev_source_inc", "lev_source_dec", "sfc_source")
SW_OUT = ("tau", "ssa", "g", "toa_src")
LW_FILES = {"lw_fsck": LW_FSCK, "lw_rrtmgp": LW_RRTMGP}
ALL_FILES = dict(LW_FILES, sw_wide=SW_WIDE)


@pytest.fixture(scope="module", autouse=True)
def ref(oracle_mod):
    """The reference module's library; every test here skips without it (and only then)."""
    if not os.path.exists(oracle_mod.REF_LIB):
        pytest.skip("oracle/_ref/libecckd_ref.so is absent: build() makes it from a reference checkout "
                    "(src/gas_optics_ecckd.f90) and an amdflang")
    oracle_mod.ref_lib()
    return oracle_mod


_models = {}


def model(oracle_mod, path):
    if path not in _models:
        _models[path] = oracle_mod.CkdModel(path)
    return _models[path]


def same_bits(a, b, what):
    """a and b identical to the bit: same shape, NaN at the same cells, equal uint64 views."""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    assert a.shape == b.shape, what
    assert np.array_equal(np.isnan(a), np.isnan(b)), "%s: NaN at different cells" % what
    diff = a.view(np.uint64) != b.view(np.uint64)
    if diff.any():
        i = tuple(int(x) for x in np.argwhere(diff)[0])
        pytest.fail("%s: %d of %d cells differ from the reference, first at %s: oracle %r, reference %r"
                    % (what, int(diff.sum()), diff.size, i, a[i], b[i]))


def check_lw(ora, m, cols, gases, tlev=True):
    tl = cols["tlev"] if tlev else None
    o = ora.gas_optics_int(m, cols["plev"], cols["tlay"], cols["tsfc"], gases, tl)
    r = ora.ref_gas_optics_int(m, cols["plev"], cols["tlay"], cols["tsfc"], gases, tl)
    assert o[5] == r[5]
    for name, a, b in zip(LW_OUT, o[:5], r[:5]):
        if tlev or name not in ("lev_source_inc", "lev_source_dec"):    # written only with tlev (:414-424)
            same_bits(a, b, name)
    return r


def check_sw(ora, m, cols, gases, two_stream=True):
    o = ora.gas_optics_ext(m, cols["plev"], cols["tlay"], gases, two_stream)
    r = ora.ref_gas_optics_ext(m, cols["plev"], cols["tlay"], gases, two_stream)
    assert o[4] == r[4]
    for name, a, b in zip(SW_OUT, o[:4], r[:4]):
        if two_stream or name == "tau":                  # the 1scl case returns after tau (:456-463)
            same_bits(a, b, name)
    return r


def check(ora, m, cols, gases):
    return check_sw(ora, m, cols, gases) if m.shortwave else check_lw(ora, m, cols, gases)


# ------------------------------------------------------------------------------------------------
def test_harness_reproduces_known_answers(ref):
    """The six values SURVEY §8(a) recorded from a run of the reference module: the harness fills
    ty_gas_optics_ecckd the way that run did."""
    kat = json.load(open(os.path.join(HERE, "golden", "kat_survey.json")))
    m = model(ref, LW_FSCK)
    plev, tlev, tlay, tsfc, gases = kat_inputs()
    tau, lay, inc, dec, sfc, err = ref.ref_gas_optics_int(m, plev, tlay, tsfc, gases, tlev)
    assert err == ""
    assert tau[0, 0, 0] == kat["tau(1,1,1)"]
    assert tau[0, 59, 0] == kat["tau(1,60,1)"]
    assert tau[16, 29, 0] == kat["tau(1,30,17)"]
    assert lay[4, 29, 0] == kat["lay_source(1,30,5)"]
    assert sfc[4, 0] == kat["sfc_source(1,5)"]
    assert inc[4, 59, 0] == kat["lev_source_inc(1,60,5)"]
    assert abs(np.pi * sfc.sum() - kat["pi_times_sum_sfc_source"]) < 1e-3
    check_lw(ref, m, dict(plev=plev, tlev=tlev, tlay=tlay, tsfc=tsfc), gases)


@pytest.mark.parametrize("key", sorted(ALL_FILES))
def test_synthetic_2000_columns(ref, key):
    m = model(ref, ALL_FILES[key])
    cols = synthetic.columns(0, 2000, float(np.exp(m.log_pressure[0])), shortwave=m.shortwave)
    check(ref, m, cols, synthetic.gas_items(cols))


@pytest.mark.parametrize("key", sorted(ALL_FILES))
def test_edge_columns_and_orography(ref, key):
    m = model(ref, ALL_FILES[key])
    pmin = float(np.exp(m.log_pressure[0]))
    for cols in (helpers.edge_columns(pmin), helpers.orography_ramp(pmin)):
        check(ref, m, cols, synthetic.gas_items(cols))


@pytest.mark.parametrize("key", sorted(ALL_FILES))
@pytest.mark.parametrize("ncol,nlay", [(1, 60), (7, 1), (33, 60), (9, 137), (1, 137), (1, 1)])
def test_column_and_layer_counts(ref, key, ncol, nlay):
    m = model(ref, ALL_FILES[key])
    cols = synthetic.columns(500, ncol, float(np.exp(m.log_pressure[0])), nlay=nlay)
    check(ref, m, cols, synthetic.gas_items(cols))


@pytest.mark.parametrize("key", sorted(ALL_FILES))
@pytest.mark.parametrize("nlay", [1, 60, 137])
@pytest.mark.parametrize("bottom_first", [False, True])
def test_branch_columns(ref, key, nlay, bottom_first):
    """Every branch in helpers.branch_columns, top-first and bottom-first (negative weights)."""
    m = model(ref, ALL_FILES[key])
    cols = helpers.branch_columns(m, nlay=nlay, bottom_first=bottom_first)
    r = check(ref, m, cols, helpers.oracle_gas_items(cols))
    tau = r[0]
    z = helpers.BRANCH_COLUMNS.index("zero_thickness")
    lz = nlay - 1 if bottom_first else 0                 # the zero-thickness top layer
    assert np.all(tau[:, lz, z] == 0.0)
    if m.shortwave:
        assert np.all(np.isnan(r[1][:, lz, z]))          # ssa = 0/0 (:459)
    else:
        assert not np.isnan(tau).any()


def test_branch_columns_reach_their_branches(ref):
    """The columns take the branches they are named after (guards helpers.branch_columns itself)."""
    m = model(ref, LW_FSCK)
    c = helpers.branch_columns(m)
    col = {n: i for i, n in enumerate(helpers.BRANCH_COLUMNS)}
    pmid = 0.5 * (c["plev"][1:] + c["plev"][:-1])
    assert np.all(pmid[:, col["p_below_grid"]] < np.exp(m.log_pressure[0]))
    assert np.any(pmid[:, col["p_above_110kPa"]] > np.exp(m.log_pressure[-1]))
    assert np.all(c["tsfc"][[col["planck_below_120K"], col["planck_above_350K"]]] != m.temperature_planck[[0, -1]])
    assert c["tsfc"][col["planck_at_120K"]] == m.temperature_planck[0] == 120.0
    assert c["tsfc"][col["planck_at_350K"]] == m.temperature_planck[-1] == 350.0
    assert c["tlay"][:, col["planck_below_120K"]].max() < 120.0 < 350.0 < c["tlay"][:, col["planck_above_350K"]].min()
    lp0, dlp = m.log_pressure[0], m.log_pressure[1] - m.log_pressure[0]      # temperature index, :120-137
    pidx = 1.0 + np.clip((np.log(pmid) - lp0) / dlp, 0.0, m.np_ - 1.0001)
    ip0 = pidx.astype(int)
    t0 = (1.0 - (pidx - ip0)) * m.temperature[0, ip0 - 1] + (pidx - ip0) * m.temperature[0, ip0]
    tidx = (c["tlay"] - t0) / (m.temperature[1, 0] - m.temperature[0, 0])
    assert np.all(tidx[:, col["t_above_grid"]] > m.nt - 1) and np.all(tidx[:, col["t_below_grid"]] < 0)
    mf = m.tables[m.gas.index("h2o")]["mole_fraction"]
    assert c["h2o"][:, col["h2o_below_lut"]].max() < mf[0] and c["h2o"][:, col["h2o_above_lut"]].min() > mf[-1]
    assert c["ch4"][col["rel_lin_at_ref"]] == m.tables[m.gas.index("ch4")]["reference_mole_fraction"]
    assert np.sum(np.diff(c["plev"][:, col["zero_thickness"]]) == 0) == 4


@pytest.mark.parametrize("key", ["lw_fsck", "sw_wide"])
@pytest.mark.parametrize("names", [
    ["co2", "ch4", "n2o", "cfc11", "cfc12", "h2o", "o3"],
    ["co2", "ch4", "n2o", "o2", "cfc11", "cfc12", "h2o", "o3"],
    ["co2", "ch4", "n2o", "n2", "cfc11", "cfc12", "h2o", "o3"],
    ["co2", "ch4", "n2o", "o2", "n2", "cfc11", "cfc12", "h2o", "o3", "no2"],
    ["n2", "o2", "h2o"],
], ids=["no_o2_n2", "o2_only", "n2_only", "both_and_no2", "composite_first"])
def test_gas_lists(ref, key, names):
    """Which composite constituent comes first decides whether the other one counts (:365-373)."""
    m = model(ref, ALL_FILES[key])
    cols = helpers.branch_columns(m)
    check(ref, m, cols, helpers.oracle_gas_items(cols, names, overrides={"n2": 0.781}))


@pytest.mark.parametrize("key", ["lw_fsck", "sw_wide"])
def test_gas_order_permutations(ref, key):
    """tau accumulates gas by gas in gas_desc order (:348,370): the order decides the bits."""
    m = model(ref, ALL_FILES[key])
    cols = helpers.branch_columns(m)
    names = synthetic.GAS_ORDER + ["n2"]
    rng = np.random.default_rng(20240611)
    taus = set()
    for _ in range(20):
        perm = [names[i] for i in rng.permutation(len(names))]
        r = check(ref, m, cols, helpers.oracle_gas_items(cols, perm, overrides={"n2": 0.781}))
        taus.add(r[0].tobytes())
    assert len(taus) > 1, "the permutations must reach different accumulation orders"


@pytest.mark.parametrize("key", ["lw_fsck", "sw_wide"])
def test_vmr_shapes(ref, key):
    """Scalar, per-column, per-layer and full vmr fields, all broadcast by get_vmr."""
    m = model(ref, ALL_FILES[key])
    cols = synthetic.columns(77, 24, float(np.exp(m.log_pressure[0])), nlay=60)
    nlay = 60
    over = {"co2": 4.1e-4,                                              # scalar
            "ch4": np.linspace(1.0e-6, 3.0e-6, 24),                     # per column
            "n2o": np.linspace(2.0e-7, 5.0e-7, nlay),                   # per layer
            "o3": cols["o3"], "o2": np.full(24, 0.209)}                 # full, per column
    items = helpers.oracle_gas_items(cols, overrides=over)
    assert [(cs, ls) for _, _, cs, ls in items[:3]] == [(0, 0), (1, 0), (0, 1)]
    check(ref, m, cols, items)


@pytest.mark.parametrize("key", sorted(LW_FILES))
def test_error_without_tlev(ref, key):
    """"tlev is required for ecckd" after tau, lay_source and sfc_source are written (:407-417)."""
    m = model(ref, LW_FILES[key])
    cols = helpers.branch_columns(m)
    r = check_lw(ref, m, cols, helpers.oracle_gas_items(cols), tlev=False)
    assert r[5] == "tlev is required for ecckd"


def test_error_one_scalar_shortwave(ref):
    """"shortwave must use ty_optical_props_2str" after tau (gas + Rayleigh) is written (:455-463)."""
    m = model(ref, SW_WIDE)
    cols = helpers.branch_columns(m)
    r = check_sw(ref, m, cols, helpers.oracle_gas_items(cols), two_stream=False)
    assert r[4] == "shortwave must use ty_optical_props_2str"


@pytest.mark.parametrize("key", sorted(ALL_FILES))
def test_getters(ref, pkg, key):
    """get_press_min/max, get_temp_min/max (:517-553) against CkdModel and the C ABI's host model."""
    m = model(ref, ALL_FILES[key])
    lim = ref.ref_limits(m)
    assert lim == (math.exp(m.log_pressure[0]), math.exp(m.log_pressure[-1]),
                   float(m.temperature.min()), float(m.temperature.max()))
    k = pkg.GasOpticsEcckd()
    assert k.load(ALL_FILES[key], device=-1) == ""
    assert (k.get_press_min(), k.get_press_max(), k.get_temp_min(), k.get_temp_max()) == lim


# ------------------------------------------------------------------------------------------------
# committed fixtures
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key,nlay", helpers.REF_FIXTURE_SETS)
def test_reference_fixtures_match_live_reference(ref, key, nlay):
    """tests/golden/ref_*.npz are what this build of the reference module computes on their inputs."""
    m = model(ref, ALL_FILES[key])
    cols, fixture, _ = helpers.load_ref_fixture(key, nlay)
    items = helpers.oracle_gas_items(cols, helpers.REF_FIXTURE_GASES)
    if m.shortwave:
        live = ref.ref_gas_optics_ext(m, cols["plev"], cols["tlay"], items)
        names = SW_OUT
    else:
        live = ref.ref_gas_optics_int(m, cols["plev"], cols["tlay"], cols["tsfc"], items, cols["tlev"])
        names = LW_OUT
    assert live[-1] == ""
    for name, a, b in zip(names, fixture, live):
        same_bits(a, b, name)


def test_synth16_fixture_matches_reference(ref):
    """The gas-optics arrays of tests/golden/lw_fsck_synth16.npz (written from the oracle by
    make_golden.py) are the reference module's output for the same inputs."""
    z = np.load(os.path.join(HERE, "golden", "lw_fsck_synth16.npz"))
    m = model(ref, LW_FSCK)
    cols = synthetic.columns(0, 16, float(np.exp(m.log_pressure[0])))
    tau, lay, inc, dec, sfc, err = ref.ref_gas_optics_int(m, cols["plev"], cols["tlay"], cols["tsfc"],
                                                          synthetic.gas_items(cols), cols["tlev"])
    assert err == ""
    for name, a in (("tau", tau), ("lay_source", lay), ("lev_source_inc", inc), ("sfc_source", sfc)):
        same_bits(z[name], a, name)
