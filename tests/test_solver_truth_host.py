"""The oracle's RTE solvers (oracle/ecckd_oracle.c) against independent multi-digit solutions of the two-stream and
Schwarzschild equations and against the Gauss-Jacobi rule derived from its moments (tests/solver_truth.py; the
expected values travel in tests/golden/solver_truth_{sw,lw}.npz).  tests/test_gpu_solver_truth.py holds the HIP
solvers to the same fixtures."""
import importlib.util
import os

import numpy as np
import pytest

import helpers
import truth_fixture as tf

ORACLE_ATOL = 1e-10      # W m-2: a tenth of helpers.FLUX_ATOL, so the GPU bar is never spent on the oracle
SPLIT_ATOL = 1e-12       # W m-2: layer-splitting invariance
RESONANCE_FACTOR = 64.0  # x 2^-53 / |1 - (k mu0)^2| of the incident flux

SW_PLAIN = [n for n, s in tf.sw_meta().items() if s["kind"] in ("main", "thin", "thick", "diffuse_in")]
SW_CONSERVATIVE = [n for n, s in tf.sw_meta().items() if s["kind"] == "conservative"]
LW_CASES = [(n, v) for n, s in tf.lw_meta().items() for v in s["variants"] if v.split()[0] == "tab" and v.endswith("f64")]


def sw_oracle(oracle_mod, inp, top_at_1=True, **options):
    """Oracle spectral fluxes (up, dn, dir) of a shortwave fixture set, levels top first whatever the orientation."""
    a = [inp["tau"], inp["ssa"], inp["g"]]
    if not top_at_1:
        a = [tf.flip(x, 1) for x in a]
    out = oracle_mod.rte_sw_gpt(*a, inp["mu0"], inp["toa"], tf.per_gpt(inp["alb_dir"]), tf.per_gpt(inp["alb_dif"]),
                                top_at_1=top_at_1, inc_flux_dif=inp.get("inc_dif"),
                                options=oracle_mod.solver_options(**options))
    return out if top_at_1 else tuple(tf.flip(x, 1) for x in out)


def sw_distance(out, exp):
    """Largest distance per column over up, dn, dir: broadband, and band / g-point fluxes where the set stores them."""
    d = np.zeros(exp["up"].shape[-1])
    for o, n in zip(out, ("up", "dn", "dir")):
        d = np.maximum(d, np.abs(o.sum(axis=0) - exp[n]).max(axis=0))
        if "gpt_" + n in exp:
            d = np.maximum(d, np.abs(o - exp["gpt_" + n]).max(axis=(0, 1)))
        if "bnd_" + n in exp:
            bnd = np.stack([o[b0 - 1:b1].sum(axis=0) for b0, b1 in tf.BAND2GPT])
            d = np.maximum(d, np.abs(bnd - exp["bnd_" + n]).max(axis=(0, 1)))
    return d


def incident(inp):
    inc = (inp["toa"] * inp["mu0"][None, :]).sum(axis=0)
    return inc + inp["inc_dif"].sum(axis=0) if "inc_dif" in inp else inc


def lw_oracle(oracle_mod, inp, variant, top_at_1=True, **options):
    _, nmus, inc, _ = variant.split()
    a = [inp["tau"], inp["lay"], inp["inc"], inp["dec"]]
    if not top_at_1:   # level l + 1 of the flipped grid is level nlay - 1 - l: inc and dec change places
        a = [tf.flip(inp["tau"], 1), tf.flip(inp["lay"], 1), tf.flip(inp["dec"], 1), tf.flip(inp["inc"], 1)]
    opt = oracle_mod.solver_options(lw_inc_flux_isotropic=int(inc == "isotropic"), **options)
    out = oracle_mod.rte_lw(*a, inp["emis_gpt"], inp["sfc_source"], top_at_1=top_at_1, nmus=int(nmus),
                            inc_flux=None if inc == "none" else inp["inc_flux"], options=opt)
    return out if top_at_1 else tuple(tf.flip(x, 0) for x in out)


# ------------------------------------------------------------------------------------------------
# the oracle against every set
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("top_at_1", [True, False])
@pytest.mark.parametrize("name", SW_PLAIN)
def test_sw_oracle_against_truth(oracle_mod, name, top_at_1):
    """sw_two_stream + adding against the boundary-value solve: main, thin, thick, diffuse_in, both orientations, to
    1e-10 W m-2.  Measured, band and g-point fluxes included, the same in both orientations: main 1.6e-12 (1 layer; 1.4e-13
    at 60, 1.1e-13 at 61 layers, 5.7e-14 / 2.8e-14 in the one-column sets at 60 / 61 layers), thin 1.32e-11, thick 1.0e-12,
    diffuse_in 3.3e-12 W m-2.  The `main` sets are built so that no layer leaves 0 <= Rdir <= 1 - Tnoscat,
    0 <= Tdir <= 1 - Tnoscat - Rdir: there "sw_dir_clamp" = 1 must stay inside the same bar."""
    inp, exp = tf.sw_set(name)
    assert incident(inp).max() <= 1400.0
    d = sw_distance(sw_oracle(oracle_mod, inp, top_at_1), exp).max()
    print("%s top_at_1=%d: oracle distance %.3e W m-2" % (name, top_at_1, d))
    assert d < ORACLE_ATOL
    if tf.sw_meta()[name]["kind"] == "main":
        assert tf.sw_meta()[name]["clamp_conditions_hold"]
        assert sw_distance(sw_oracle(oracle_mod, inp, top_at_1, sw_dir_clamp=1), exp).max() < ORACLE_ATOL


@pytest.mark.parametrize("name", SW_CONSERVATIVE)
def test_sw_oracle_conservative(oracle_mod, name):
    """ssa = 1 exactly in about 40 % of the layers.  The truth solves the k = 0 equations; the solvers floor k^2 at
    sw_k_floor = 1e-12, which perturbs the fluxes.  Measured distance of the oracle over the final sets: 3.1e-8 W m-2
    (8 layers) and 1.9e-8 W m-2 (60 layers); the bars are 4 x that, 1.24e-7 and 7.7e-8 W m-2 (the fixture's metadata
    holds both numbers; the GPU test uses the same bars).  The distance is rounding more than perturbation: with
    k = 1e-6 the solvers' 1 - exp(-2 k tau) keeps ten digits.  A floor of 1e-10 gives 3.6e-8 and 1.2e-7 W m-2, one of
    1e-16 gives 2.9e-6 W m-2 (60 layers): neither neighbour of the default is closer to the k = 0 solution."""
    inp, exp = tf.sw_set(name)
    m = tf.sw_meta()[name]
    assert m["bar"] == 4.0 * m["oracle_distance"] and m["bar"] < 2e-7
    assert np.any(inp["ssa"] == 1.0) and np.any(inp["ssa"] < 1.0)
    d = sw_distance(sw_oracle(oracle_mod, inp), exp).max()
    print("%s: oracle distance %.3e W m-2, bar %.3e" % (name, d, m["bar"]))
    assert d < m["bar"]
    assert sw_distance(sw_oracle(oracle_mod, inp, top_at_1=False), exp).max() < m["bar"]


def resonance_bar(inp):
    return RESONANCE_FACTOR * 2.0 ** -53 / inp["d_min"] * incident(inp)


def test_sw_oracle_resonance(oracle_mod):
    """Layers with |1 - (k mu0)^2| = 1e-1 .. 1e-4 (column i: 10^-(1 + i % 4)).  The equations are smooth there; the
    closed forms divide by it, so rounding is amplified by 1 / |d|.  Bar: 64 x 2^-53 / |d_min| of the column's incident
    flux.  Largest constant seen over the set (in place of the 64): 1.43 for the oracle."""
    inp, exp = tf.sw_set("resonance")
    for i in range(inp["mu0"].shape[0]):
        assert abs(inp["d_min"][i] / 10.0 ** -(1 + i % 4) - 1.0) < 1e-6
    for top_at_1 in (True, False):
        d = sw_distance(sw_oracle(oracle_mod, inp, top_at_1), exp)
        const = (d * inp["d_min"] / (2.0 ** -53 * incident(inp))).max()
        print("resonance top_at_1=%d: largest constant %.3f (bar %g), distance %.3e W m-2" % (top_at_1, const, RESONANCE_FACTOR, d.max()))
        assert np.all(d < resonance_bar(inp))


LW_SWITCHES = [{}, dict(lw_series_terms=3), dict(lw_series_terms=3, lw_tau_thresh=helpers.EPS32_THRESH),
               dict(lw_tau_thresh=1e-6), dict(lw_tau_thresh=helpers.EPS32_THRESH)]


@pytest.mark.parametrize("name,variant", LW_CASES)
def test_lw_oracle_against_truth(oracle_mod, name, variant):
    """lw_solver_noscat (linear-in-tau source, transport, quadrature with the published table) against the per-angle
    Schwarzschild solve, both orientations, both forms of the incident flux, to 1e-10 W m-2 (measured: at most 5.2e-13
    over every set and the first four switches).  The series switches change only rounding against the truth: 3 terms,
    the single-precision threshold (3.45e-4) with 3 and with 2 terms, and a threshold of 1e-6 with 2 terms each stay
    inside the same bar.  2 terms at the single-precision threshold drop x^3 / 8 <= 5.1e-12 of twice the source step,
    which the sets keep below 1e3 tau <= 0.35 W m-2 sr-1 in such a layer: 1.1e-11 W m-2 per layer at the most, measured
    3.0e-12 over a column."""
    inp, exp = tf.lw_set(name, variant)
    assert max(exp["up"].max(), exp["dn"].max()) <= 500.0
    below = inp["tau"] * helpers.GAUSS_DS[0][0] < np.sqrt(np.finfo(np.float64).eps)
    assert below.any() and not below.all()                       # both sides of the series threshold
    for top_at_1 in (True, False):
        for sw in LW_SWITCHES if top_at_1 else LW_SWITCHES[:1]:
            fu, fd = lw_oracle(oracle_mod, inp, variant, top_at_1, **sw)
            d = max(np.abs(fu - exp["up"]).max(), np.abs(fd - exp["dn"]).max())
            print("%s %s top_at_1=%d %s: oracle distance %.3e W m-2" % (name, variant, top_at_1, sw, d))
            assert d < ORACLE_ATOL


@pytest.mark.parametrize("name", sorted(tf.lw_meta()))
def test_lw_oracle_exact_nodes(oracle_mod, name):
    """The published table against the exact Gauss-Jacobi nodes: fluxes computed with the table differ from the
    exact-node truth by the table's own precision (nine digits of the secants) and no more -- 1e-8 of the largest
    flux -- for 2 to 4 angles."""
    for variant in tf.lw_meta()[name]["variants"]:
        q, nmus, inc, im = variant.split()
        if q != "exact" or nmus == "1":       # (one exact node is secant 1.5: the table's 1.66 is a convention)
            continue
        inp, exp = tf.lw_set(name, variant)
        gu, gd = oracle_mod.rte_lw_gpt(inp["tau"], inp["lay"], inp["inc"], inp["dec"], inp["emis_gpt"], inp["sfc_source"],
                                       nmus=int(nmus), inc_flux=inp["inc_flux"])
        big = max(exp["gpt_up"].max(), exp["gpt_dn"].max())
        d = max(np.abs(gu - exp["gpt_up"]).max(), np.abs(gd - exp["gpt_dn"]).max())
        print("%s %s: table against exact nodes %.3e of the largest flux" % (name, variant, d / big))
        assert 0 < d < 1e-8 * big


# ------------------------------------------------------------------------------------------------
# quadrature
# ------------------------------------------------------------------------------------------------
def test_quadrature_table_is_gauss_jacobi():
    """helpers.GAUSS_DS / GAUSS_WTS (the constants of the oracle and of the kernels) against the Gauss rule for the
    weight mu on [0, 1] derived from its moments (the fixture holds the derived nodes rounded to float64;
    test_fixture_regenerates ties them to solver_truth.gauss_jacobi)."""
    assert helpers.GAUSS_DS[0] == (1.66,) and helpers.GAUSS_WTS[0] == (0.5,)      # the conventional single angle
    D1, w1 = tf.exact_quadrature(1)
    assert D1[0] == 1.5 and w1[0] == 0.5
    for n in (2, 3, 4):
        D, w = tf.exact_quadrature(n)
        tD, tw = np.array(helpers.GAUSS_DS[n - 1]), np.array(helpers.GAUSS_WTS[n - 1])
        assert np.all(np.diff(D) > 0)
        assert np.array_equal(np.round(w, 10), tw)                                 # all ten printed decimals
        assert np.max(np.abs(tD / D - 1.0)) <= 2.0 ** -23
        assert abs(tw.sum() - 0.5) < 1e-10                                         # zeroth moment
        assert abs(np.sum(tw / tD) - 1.0 / 3.0) < 2e-9                             # first moment: sum w_k mu_k = 1/3
        assert abs(np.sum(w) - 0.5) < 1e-15 and abs(np.sum(w / D) - 1.0 / 3.0) < 1e-15


def test_generator_table_is_helpers_table():
    """The generator computes the `tab` fluxes with its own copy of the published constants."""
    gen = load_generator()
    assert gen.GAUSS_DS == helpers.GAUSS_DS and gen.GAUSS_WTS == helpers.GAUSS_WTS
    assert np.array_equal(gen.BAND2GPT, tf.BAND2GPT)


# ------------------------------------------------------------------------------------------------
# layer splitting
# ------------------------------------------------------------------------------------------------
def split_layer(a, l):
    """(ng, nlay, ncol) -> (ng, nlay + 1, ncol) with layer l repeated."""
    return np.ascontiguousarray(np.concatenate([a[:, :l + 1], a[:, l:]], axis=1))


def sw_split_inputs(inp, l):
    out = dict(inp)
    tau = split_layer(inp["tau"], l)
    tau[:, l:l + 2] *= 0.5
    out.update(tau=tau, ssa=split_layer(inp["ssa"], l), g=split_layer(inp["g"], l))
    return out


def lw_split_inputs(inp, l):
    """Layer l cut into two of half the optical depth, the interpolated source at the new level (exact: the level
    sources sit on a grid of 2^-20)."""
    tau = split_layer(inp["tau"], l)
    tau[:, l:l + 2] *= 0.5
    lev = inp["lev_source"]
    mid = 0.5 * (lev[:, l] + lev[:, l + 1])
    assert np.array_equal(2.0 * mid, lev[:, l] + lev[:, l + 1])
    lev = np.ascontiguousarray(np.concatenate([lev[:, :l + 1], mid[:, None], lev[:, l + 1:]], axis=1))
    out = dict(inp, tau=tau, lev_source=lev, inc=np.ascontiguousarray(lev[:, 1:]), dec=np.ascontiguousarray(lev[:, :-1]))
    out["lay"] = 0.5 * (out["inc"] + out["dec"])
    assert np.array_equal(2.0 * out["lay"], out["inc"] + out["dec"])
    return out


def drop_level(f, l):
    """Fluxes (..., nlay + 2, ncol) of a grid with layer l split -> the original levels."""
    return np.delete(f, l + 1, axis=-2)


SPLIT_D_MIN = 0.3
SPLIT_FACTOR = 8.0       # x 2^-53 / |1 - (k mu0)^2| of the incident flux, for columns nearer the resonance


def resonance_distance(inp):
    """min over layers and g-points of |1 - (k mu0)^2|, per column."""
    w, g = inp["ssa"], inp["g"]
    g1, g2 = (8.0 - w * (5.0 + 3.0 * g)) / 4.0, 3.0 * w * (1.0 - g) / 4.0
    k2 = np.maximum((g1 - g2) * (g1 + g2), 0.0)
    return np.min(np.abs(1.0 - k2 * inp["mu0"][None, None, :] ** 2), axis=(0, 1))


def split_bar(inp):
    """Per-column bar of the layer-splitting test.  sw_two_stream divides the direct-beam terms by d = 1 - (k mu0)^2, and
    the rounding it amplifies differs between a layer and its halves: 2^-53 / |d| of an incident flux of up to
    1400 W m-2 is 1.6e-11 W m-2 at the 0.01 the `main` sets allow and 5e-13 at 0.3.  So 1e-12 W m-2 holds as it stands
    in every column whose layers all keep |d| >= 0.3; a column nearer the resonance is held to
    max(1e-12, 8 x 2^-53 / |d_col| x incident): the constant of the resonance test's bar measured at a probe point is
    about 4 for one evaluation against the truth, and here two evaluations are compared.  Largest constant seen over
    the cases below: 2.25 (main_n1)."""
    d = resonance_distance(inp)
    near = SPLIT_FACTOR * 2.0 ** -53 / d * incident(inp)
    return np.where(d >= SPLIT_D_MIN, SPLIT_ATOL, np.maximum(SPLIT_ATOL, near))


SW_SPLITS = [("main_n1", 0), ("diffuse_in", 0), ("diffuse_in", 3), ("main_n60", 0), ("main_n61", 1), ("main_c1", 0),
             ("main_n60_c1", 0), ("thin", 59), ("thick", 2)]


@pytest.mark.parametrize("name,l", SW_SPLITS)
def test_sw_oracle_layer_splitting(oracle_mod, name, l):
    """Cutting a layer into two of half the optical depth changes no flux at the original levels: trivial for the
    equations, a real condition on the two-stream coefficients and the adding recurrences with a source.  Layers near
    the top, where the fluxes are large.  Every column is asserted: 1e-12 W m-2 away from the resonance, the amplified
    bar of split_bar nearer to it."""
    inp, _ = tf.sw_set(name)
    a = sw_oracle(oracle_mod, inp)
    b = sw_oracle(oracle_mod, sw_split_inputs(inp, l))
    bar = split_bar(inp)
    flat = bar == SPLIT_ATOL
    assert flat.sum() >= 3 or flat.size == 1
    d = np.max([np.abs(drop_level(y, l) - x).max(axis=(0, 1)) for x, y in zip(a, b)], axis=0)
    const = (d * resonance_distance(inp) / (2.0 ** -53 * incident(inp))).max()
    print("%s layer %d: %.3e W m-2 over all %d columns (%d at 1e-12; largest constant %.3f, bar %g)"
          % (name, l, d.max(), d.size, flat.sum(), const, SPLIT_FACTOR))
    assert np.all(d < bar), (np.flatnonzero(d >= bar), d[d >= bar], bar[d >= bar])


@pytest.mark.parametrize("name,l,nmus", [("n1", 0, 1), ("n33", 0, 2), ("n33", 17, 4), ("n60s", 59, 2), ("n97", 96, 3)])
def test_lw_oracle_layer_splitting(oracle_mod, name, l, nmus):
    """The same for the longwave source formula, with the interpolated source at the new level."""
    inp = tf.lw_set(name)
    v = "tab %d weighted f64" % nmus
    a = lw_oracle(oracle_mod, inp, v)
    b = lw_oracle(oracle_mod, lw_split_inputs(inp, l), v)
    d = max(np.abs(drop_level(y, l) - x).max() for x, y in zip(a, b))
    print("%s layer %d: %.3e W m-2" % (name, l, d))
    assert d < SPLIT_ATOL


# ------------------------------------------------------------------------------------------------
# the fixtures are what the generator writes
# ------------------------------------------------------------------------------------------------
def load_generator():
    spec = importlib.util.spec_from_file_location("make_golden_solver_truth", os.path.join(tf.GOLDEN, "make_golden_solver_truth.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    return gen


def test_fixture_inputs_regenerate():
    """The stored inputs are the generator's (no mpmath needed), every set is present with the shapes the generator
    lists, and the files stay well inside the limit for a committed file."""
    gen = load_generator()
    assert sorted(gen.SW_SETS) == sorted(tf.sw_meta()) and sorted(gen.LW_SETS) == sorted(tf.lw_meta())
    for name, s in gen.SW_SETS.items():
        inp, _ = tf.sw_set(name)
        for k, v in gen.sw_inputs(name).items():
            assert np.array_equal(inp[k], v), (name, k)
        assert inp["tau"].shape == (3, s["nlay"], s["ncol"])
    for name, s in gen.LW_SETS.items():
        inp = tf.lw_set(name)
        for k, v in gen.lw_inputs(name).items():
            assert np.array_equal(inp[k], v), (name, k)
        assert inp["tau"].shape == (3, s["nlay"], s["ncol"])
        assert [" ".join(v) for v in s["variants"]] == tf.lw_meta()[name]["variants"]
    for p in (gen.SW_PATH, gen.LW_PATH):
        assert os.path.getsize(p) < 768 * 1024


def test_fixture_regenerates():
    """With mpmath: four columns of every set recomputed from solver_truth give the fixture's bits (deep shortwave sets:
    the float64 image; every other image and every second longwave variant as well), and the stored Gauss-Jacobi
    nodes are solver_truth.gauss_jacobi's.  The only test of this file that may skip (without mpmath)."""
    pytest.importorskip("mpmath")
    gen = load_generator()
    for n in (1, 2, 3, 4):
        D, w = gen.exact_quadrature(n)
        eD, ew = tf.exact_quadrature(n)
        assert np.array_equal(D, eD) and np.array_equal(w, ew)
    for name, s in gen.SW_SETS.items():
        inp = gen.sw_inputs(name)
        for image in ("f64", "f32") if s["f32"] and s["nlay"] <= 8 else ("f64",):
            _, exp = tf.sw_set(name, image)
            for i in sorted({0, s["ncol"] // 3, 2 * s["ncol"] // 3, s["ncol"] - 1}):
                out = gen.sw_expected_column(name, inp, i, image, check=False)[0]
                assert sorted(out) == sorted(exp)
                for k, v in out.items():
                    assert np.array_equal(v, exp[k][..., i]), (name, image, i, k)
    for name, s in gen.LW_SETS.items():
        inp = gen.lw_inputs(name)
        for v in s["variants"][::2]:
            _, exp = tf.lw_set(name, " ".join(v))
            for i in sorted({0, s["ncol"] // 3, 2 * s["ncol"] // 3, s["ncol"] - 1}):
                out = gen.lw_expected_column(name, inp, i, v, check=False)[0]
                for k, a in out.items():
                    assert np.array_equal(a, exp[k][..., i]), (name, v, i, k)
