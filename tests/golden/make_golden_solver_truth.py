"""Writes tests/golden/solver_truth_sw.npz and solver_truth_lw.npz: inputs of the flux solvers and the fluxes that
tests/solver_truth.py (multi-digit solutions of the two-stream and Schwarzschild equations, independent of the oracle
and of the product) gives for them, rounded once to float64.

    python tests/golden/make_golden_solver_truth.py        (needs mpmath; a few minutes on 8 cores)

Run twice it writes identical files: the inputs come from seeded generators, every (set, column) is solved on its own,
and the archives are written with fixed time stamps.  The inputs and the expected fluxes are the same bits wherever it
runs; the metadata's `oracle_distance`, `oracle_constant` and `bar` are measured with the C oracle as compiled where the
generator runs, so another compiler or libm may write other last digits there (and with them another `conservative`
bar, which the host and the GPU tests both read from the metadata).

Every shortwave (column, g-point) is solved at DPS digits (plus the digits linear shooting loses, see solver_truth)
and again at 2 DPS; the two must agree to 1e-25 of the column's incident flux.  The longwave likewise (1e-25 of the
largest flux of the column).  The oracle is used here only to MEASURE: its distance from every set goes into the
metadata, the `conservative` and `resonance` bars of tests/test_solver_truth_host.py are taken from it.

Sets (3 g-points in two bands, band2gpt = [[1, 2], [3, 3]]; albedos / emissivity per band):
  shortwave  main_*        tau 1e-3..5 (log-uniform), ssa 0.05..0.999, g -0.3..0.9, albedos 0..1 (direct != diffuse).
                           mu0 0.05..1 is redrawn until every layer has |1 - (k mu0)^2| >= 0.01 AND mu0 g <= 0.6: with
                           the latter every layer has 0 <= Rdir <= 1 - Tnoscat and 0 <= Tdir <= 1 - Tnoscat - Rdir (checked
                           below on the multi-digit single-layer values), so "sw_dir_clamp" = 1 must not change a flux.
             thin          tau 1e-12..1e-6
             thick         three layers of tau 30..200 under five thin ones (the direct beam underflows)
             diffuse_in    non-zero diffuse flux at the top (kernel-level interface); per-g-point fluxes stored
             conservative  ssa = 1 exactly in about 40 % of the layers (the solvers floor k^2 at 1e-12, the truth has k = 0)
             resonance     column i: every layer has |1 - (k mu0)^2| = 10^-(1 + i % 4), alternating sign
  longwave   n1, n33, n60, n60s, n97, and one column at 60 and at 97 layers (n60_c1, n97_c1; shortwave: main_c1 at 61
             and main_n60_c1 at 60 layers): tau 1e-10..30 (log-uniform), level sources on a grid of 2^-20 W m-2 sr-1, so
             that lay = (lev_a + lev_b) / 2 is exact in float64.  Values up to 60 on that grid need 26 bits: the float32
             image rounds the level values (by up to 2e-6 W m-2 sr-1), its layer source is the float32 mean of the rounded
             levels (one more rounding), and its truth is linear between the rounded levels -- a mismatch of about
             2e-6 W m-2 sr-1, far inside the single-precision bar (at least 1e-4 W m-2).
             The source changes across a layer by at most min(8, 1e3 tau) W m-2 sr-1: the solvers' (1 - T) / tau - T
             cancels to 1.1e-16 / tau (absolute) just above the series threshold, which a source step dB turns into a
             flux error of pi 1.1e-16 dB / tau per layer -- 3e-8 W m-2 for steps of 20 across layers of tau 1e-6 (measured
             on a first draw with independent level values), 1e-11 with steps of 3e4 tau.  That is rounding of the
             published algorithm, not a defect, and no atmosphere has such steps across transparent layers; with the
             bound it is 3.5e-13 W m-2 per layer, under the 1e-12 of the layer-splitting test.
The 65-column sets at 60 layers cycle through 13 profiles of optical properties and level sources (column i has
profile i % 13) so that the archive compresses; boundary values and mu0 differ in every column.
"""
import io
import json
import multiprocessing
import os
import sys
import zipfile
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for _p in (ROOT, os.path.join(ROOT, "oracle"), os.path.dirname(HERE)):
    if _p not in sys.path:
        sys.path.insert(0, _p)

DPS = 40
AGREE = 1e-25
BAND2GPT = np.array([[1, 2], [3, 3]])
GPT2BAND = np.array([0, 0, 1])
NG = 3
SW_PATH = os.path.join(HERE, "solver_truth_sw.npz")
LW_PATH = os.path.join(HERE, "solver_truth_lw.npz")
# published secants and weights (the same constants as helpers.GAUSS_DS / GAUSS_WTS; tests/test_solver_truth_host.py
# ties them to solver_truth.gauss_jacobi)
GAUSS_DS = ((1.66,), (1.18350343, 2.81649655), (1.09719858, 1.69338507, 4.70941630),
            (1.06056257, 1.38282560, 2.40148179, 7.15513024))
GAUSS_WTS = ((0.5,), (0.3180413817, 0.1819586183), (0.2009319137, 0.2292411064, 0.0698269799),
             (0.1355069134, 0.2034645680, 0.1298475476, 0.0311809710))

# name: kind, nlay, ncol, nprof (0: one profile per column), float32 image too, stored outputs
SW_SETS = {
    "main_n1": dict(kind="main", nlay=1, ncol=65, nprof=0, f32=True, out="bnd"),
    "main_n60": dict(kind="main", nlay=60, ncol=65, nprof=13, f32=True, out="bb"),
    "main_n61": dict(kind="main", nlay=61, ncol=12, nprof=0, f32=True, out="bnd"),
    "main_c1": dict(kind="main", nlay=61, ncol=1, nprof=0, f32=True, out="bb"),
    "main_n60_c1": dict(kind="main", nlay=60, ncol=1, nprof=0, f32=True, out="bb"),
    "thin": dict(kind="thin", nlay=60, ncol=8, nprof=0, f32=True, out="bb"),
    "thick": dict(kind="thick", nlay=8, ncol=9, nprof=0, f32=True, out="bb"),
    "diffuse_in": dict(kind="diffuse_in", nlay=8, ncol=65, nprof=0, f32=False, out="gpt"),
    "conservative_n8": dict(kind="conservative", nlay=8, ncol=9, nprof=0, f32=True, out="bb"),
    "conservative_n60": dict(kind="conservative", nlay=60, ncol=9, nprof=0, f32=True, out="bb"),
    "resonance": dict(kind="resonance", nlay=4, ncol=8, nprof=0, f32=False, out="bb"),
}


def _variants(spec):
    return [tuple(v.split()) for v in spec]


# variant: quadrature (tab: published table, broadband fluxes; exact: Gauss-Jacobi nodes rounded to float64, per-g-point
# fluxes; sets with bnd: the band fluxes of the tab variants without incident flux too), angles, incident flux (none / weighted: I = F / (2 pi w_k) / isotropic: I = F / pi), image (f64 / f32)
_ALL = ["tab %d %s f64" % (n, i) for n in (1, 2, 3, 4) for i in ("none", "weighted", "isotropic")] + \
       ["exact %d weighted f64" % n for n in (1, 2, 3, 4)] + \
       ["tab %d %s f32" % (n, i) for n in (1, 2, 3, 4) for i in ("none", "weighted")]
LW_SETS = {
    "n1": dict(nlay=1, ncol=65, nprof=0, bnd=True, variants=_variants(_ALL)),
    "n33": dict(nlay=33, ncol=6, nprof=0, bnd=True, variants=_variants(
        ["tab 2 none f64", "tab 3 weighted f64", "exact 1 weighted f64", "tab 2 none f32", "tab 4 weighted f32"])),
    "n60": dict(nlay=60, ncol=65, nprof=13, bnd=False, variants=_variants(
        ["tab 1 none f64", "tab 4 none f64", "tab 2 weighted f64", "tab 3 isotropic f64", "tab 1 none f32"])),
    "n60s": dict(nlay=60, ncol=6, nprof=0, bnd=True, variants=_variants(
        ["tab 2 none f64", "tab 3 none f64", "exact 3 weighted f64", "tab 2 weighted f32", "tab 4 none f32"])),
    "n97": dict(nlay=97, ncol=6, nprof=0, bnd=True, variants=_variants(
        ["tab 1 none f64", "tab 3 none f64", "tab 4 weighted f64", "tab 2 isotropic f64", "exact 4 weighted f64",
         "tab 3 none f32", "tab 1 weighted f32"])),
    "n60_c1": dict(nlay=60, ncol=1, nprof=0, bnd=True, variants=_variants(
        ["tab 2 none f64", "tab 3 weighted f64", "tab 1 isotropic f64", "exact 2 weighted f64", "tab 4 none f32",
         "tab 2 weighted f32"])),
    "n97_c1": dict(nlay=97, ncol=1, nprof=0, bnd=True, variants=_variants(
        ["tab 4 none f64", "tab 1 weighted f64", "exact 3 weighted f64", "tab 2 none f32"])),
}


def r32(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32), dtype=np.float64)


def _rng(name, what):
    return np.random.default_rng([20240607, zlib.crc32((what + "/" + name).encode())])


def _k(ssa, g):
    g1 = (8.0 - ssa * (5.0 + 3.0 * g)) / 4.0
    g2 = 3.0 * ssa * (1.0 - g) / 4.0
    return np.sqrt(np.maximum((g1 - g2) * (g1 + g2), 0.0))


def resonance_distance(ssa, g, mu0):
    """min over layers and g-points of |1 - (k mu0)^2| per column (layers with ssa = 1 have k = 0: distance 1)."""
    return np.min(np.abs(1.0 - (_k(ssa, g) * mu0[None, None, :]) ** 2), axis=(0, 1))


# ------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------
def sw_inputs(name):
    s = SW_SETS[name]
    kind, nlay, ncol = s["kind"], s["nlay"], s["ncol"]
    rng = _rng(name, "sw")
    npf = s["nprof"] or ncol
    shape = (NG, nlay, npf)
    logu = lambda lo, hi, sh: np.exp(rng.uniform(np.log(lo), np.log(hi), sh))
    tau = logu(1e-3, 5.0, shape)
    ssa = rng.uniform(0.05, 0.999, shape)
    g = rng.uniform(-0.3, 0.9, shape)
    if kind == "thin":
        tau = logu(1e-12, 1e-6, shape)
    elif kind == "thick":
        tau[:, :nlay - 3] = logu(1e-3, 0.5, (NG, nlay - 3, npf))
        tau[:, nlay - 3:] = logu(30.0, 200.0, (NG, 3, npf))
    elif kind == "conservative":
        ssa[rng.uniform(size=shape) < 0.4] = 1.0
    pick = np.arange(ncol) % npf
    tau, ssa, g = (np.ascontiguousarray(a[:, :, pick]) for a in (tau, ssa, g))
    mu0 = np.empty(ncol)
    if kind == "resonance":
        mu0 = rng.uniform(0.55, 1.0, ncol)
        for i in range(ncol):
            for k in range(NG):
                for l in range(nlay):
                    d = 10.0 ** -(1 + i % 4) * (1.0 if l % 2 == 0 else -1.0)
                    want = np.sqrt(1.0 - d) / mu0[i]
                    lo, hi = 0.0, 1.0                      # k falls from 2 (ssa = 0) to 0 (ssa = 1)
                    for _ in range(200):
                        mid = 0.5 * (lo + hi)
                        if _k(np.float64(mid), g[k, l, i]) > want:
                            lo = mid
                        else:
                            hi = mid
                    ssa[k, l, i] = lo
    else:
        for i in range(ncol):
            while True:
                m = rng.uniform(0.05, 1.0)
                one = np.array([m])
                ok = resonance_distance(ssa[:, :, i:i + 1], g[:, :, i:i + 1], one)[0] >= 0.01
                if kind == "main":
                    ok = ok and m * g[:, :, i].max() <= 0.6
                if ok:
                    mu0[i] = m
                    break
    total = rng.uniform(600.0, 1400.0 / 1.0001, ncol) * (0.9 if kind == "diffuse_in" else 1.0)
    frac = rng.uniform(0.2, 1.0, (NG, ncol))
    toa = total[None, :] * frac / frac.sum(axis=0)[None, :]
    alb_dir = rng.uniform(0.0, 1.0, (ncol, 2))
    alb_dif = rng.uniform(0.0, 1.0, (ncol, 2))
    assert not np.any(alb_dir == alb_dif)
    out = dict(tau=tau, ssa=ssa, g=g, mu0=mu0, toa=toa, alb_dir=alb_dir, alb_dif=alb_dif)
    if kind == "diffuse_in":
        out["inc_dif"] = rng.uniform(0.0, 30.0, (NG, ncol))
    return out


def lw_inputs(name):
    s = LW_SETS[name]
    nlay, ncol = s["nlay"], s["ncol"]
    rng = _rng(name, "lw")
    npf = s["nprof"] or ncol
    tau = np.exp(rng.uniform(np.log(1e-10), np.log(30.0), (NG, nlay, npf)))
    grid = 2.0 ** 20
    lev = np.empty((NG, nlay + 1, npf))
    lev[:, 0] = np.round(rng.uniform(5.0, 55.0, (NG, npf)) * grid) / grid
    step = rng.uniform(0.25, 1.0, (NG, nlay, npf)) * np.minimum(8.0, 1e3 * tau)
    sign = np.where(rng.uniform(size=(NG, nlay, npf)) < 0.5, -1.0, 1.0)
    for l in range(nlay):
        sg = np.where(lev[:, l] < 10.0, 1.0, np.where(lev[:, l] > 50.0, -1.0, sign[:, l]))
        lev[:, l + 1] = lev[:, l] + np.round(sg * step[:, l] * grid) / grid
    assert lev.min() >= 1.0 and lev.max() <= 60.0
    pick = np.arange(ncol) % npf
    tau, lev = np.ascontiguousarray(tau[:, :, pick]), np.ascontiguousarray(lev[:, :, pick])
    return dict(tau=tau, lev_source=lev, sfc_emis=rng.uniform(0.7, 1.0, (ncol, 2)),
                sfc_source=rng.uniform(1.0, 60.0, (NG, ncol)), inc_flux=rng.uniform(0.5, 30.0, (NG, ncol)))


def exact_quadrature(n):
    """Gauss-Jacobi secants and weights rounded to float64 (what ecckd_lw_solver_noscat_gpt is handed)."""
    import solver_truth as st
    D, w = st.gauss_jacobi(n)
    return [float(x) for x in D], [float(x) for x in w]


# ------------------------------------------------------------------------------------------------
# expected values, one column at a time
# ------------------------------------------------------------------------------------------------
def _col(a, i):
    a = np.asarray(a)
    return np.ascontiguousarray(a[..., i:i + 1])


def sw_expected_column(name, inp, i, image, check=True):
    """Expected fluxes of column i of a shortwave set: dict of float64 arrays (without the column axis), the largest
    disagreement between the DPS and the 2 DPS solve (relative to the incident flux; None without `check`), the
    working digits, and whether the clamp conditions hold in every layer."""
    import mpmath as mp
    import solver_truth as st
    conv = r32 if image == "f32" else (lambda a: np.asarray(a, dtype=np.float64))
    tau, ssa, g = (conv(_col(inp[n], i)) for n in ("tau", "ssa", "g"))
    mu0, toa = conv(inp["mu0"][i:i + 1]), conv(_col(inp["toa"], i))
    ad = conv(inp["alb_dir"][i:i + 1, GPT2BAND].T)
    af = conv(inp["alb_dif"][i:i + 1, GPT2BAND].T)
    dif = conv(_col(inp["inc_dif"], i)) if "inc_dif" in inp else None
    a = st.sw_truth(tau, ssa, g, mu0, toa, ad, af, dif, dps=DPS)
    agree = None
    if check:
        b = st.sw_truth(tau, ssa, g, mu0, toa, ad, af, dif, dps=2 * DPS)
        with mp.workdps(30):
            agree = 0.0
            for k in range(NG):
                inc = mp.mpf(float(toa[k, 0])) * mp.mpf(float(mu0[0])) + (0 if dif is None else mp.mpf(float(dif[k, 0])))
                for n in ("up", "dn", "dir"):
                    agree = max(agree, max(float(abs(x - y) / inc) for x, y in zip(a[n][k, :, 0], b[n][k, :, 0])))
    out = {}
    kind = SW_SETS[name]["out"]
    for n in ("up", "dn", "dir"):
        f = a[n][:, :, 0]
        out[n] = st.to_f64(st.sum_gpts(f))
        if kind == "bnd":
            out["bnd_" + n] = np.stack([st.to_f64(st.sum_gpts(f, b0 - 1, b1)) for b0, b1 in BAND2GPT])
        if kind == "gpt":
            out["gpt_" + n] = st.to_f64(f)
    r, t, tn = a["rdir"], a["tdir"], a["tnoscat"]
    clamp_ok = all(0 <= x <= 1 - z and 0 <= y <= 1 - z - x for x, y, z in zip(r.ravel(), t.ravel(), tn.ravel()))
    digits = DPS + 5 + int(max(st.sw_digits_lost(tau[k, :, 0], ssa[k, :, 0], g[k, :, 0]) for k in range(NG)))
    return out, agree, digits, clamp_ok


def lw_expected_column(name, inp, i, variant, check=True):
    import mpmath as mp
    import solver_truth as st
    quad, nmus, inc, image = variant
    nmus = int(nmus)
    conv = r32 if image == "f32" else (lambda a: np.asarray(a, dtype=np.float64))
    tau, lev = conv(_col(inp["tau"], i)), conv(_col(inp["lev_source"], i))
    emis = conv(inp["sfc_emis"][i:i + 1, GPT2BAND].T)
    sfc = conv(_col(inp["sfc_source"], i))
    incf = None if inc == "none" else conv(_col(inp["inc_flux"], i))
    Ds, wts = exact_quadrature(nmus) if quad == "exact" else (GAUSS_DS[nmus - 1], GAUSS_WTS[nmus - 1])
    res = [st.lw_truth(tau, lev, emis, sfc, Ds, wts, incf, inc == "isotropic", dps=d) for d in ((DPS, 2 * DPS) if check else (DPS,))]
    agree = None
    if check:
        with mp.workdps(30):
            big = max(abs(x) for x in list(res[0][0].ravel()) + list(res[0][1].ravel()))
            agree = max(float(abs(x - y) / big) for a, b in zip(res[0], res[1]) for x, y in zip(a.ravel(), b.ravel()))
    up, dn = res[0][0][:, :, 0], res[0][1][:, :, 0]
    if quad == "exact":
        return dict(gpt_up=st.to_f64(up), gpt_dn=st.to_f64(dn)), agree
    out = dict(up=st.to_f64(st.sum_gpts(up)), dn=st.to_f64(st.sum_gpts(dn)))
    if LW_SETS[name]["bnd"] and inc == "none":
        for n, f in (("up", up), ("dn", dn)):
            out["bnd_" + n] = np.stack([st.to_f64(st.sum_gpts(f, b0 - 1, b1)) for b0, b1 in BAND2GPT])
    return out, agree


def _sw_task(t):
    name, i, image = t
    return t, sw_expected_column(name, sw_inputs(name), i, image)


def _lw_task(t):
    name, i, variant = t
    return t, lw_expected_column(name, lw_inputs(name), i, variant)


def vkey(variant):
    return "%s%s.%s.%s" % variant


# ------------------------------------------------------------------------------------------------
# measuring the oracle (metadata only)
# ------------------------------------------------------------------------------------------------
def sw_oracle_distance(oracle, name, arrays, **options):
    """Largest |oracle - truth| over the broadband fluxes of a shortwave set, per column (W m-2)."""
    a = lambda n: arrays["%s.%s" % (name, n)]
    ad = np.ascontiguousarray(a("alb_dir")[:, GPT2BAND].T)
    af = np.ascontiguousarray(a("alb_dif")[:, GPT2BAND].T)
    dif = arrays.get(name + ".inc_dif")
    gu, gd, gr = oracle.rte_sw_gpt(a("tau"), a("ssa"), a("g"), a("mu0"), a("toa"), ad, af, inc_flux_dif=dif,
                                   options=oracle.solver_options(**options) if options else None)
    d = np.zeros(a("mu0").shape[0])
    for o, n in ((gu, "up"), (gd, "dn"), (gr, "dir")):
        d = np.maximum(d, np.abs(o.sum(axis=0) - a("f64." + n)).max(axis=0))
    return d


def incident(arrays, name):
    a = lambda n: arrays["%s.%s" % (name, n)]
    inc = (a("toa") * a("mu0")[None, :]).sum(axis=0)
    if name + ".inc_dif" in arrays:
        inc = inc + arrays[name + ".inc_dif"].sum(axis=0)
    return inc


def write_npz(path, arrays):
    """np.load-able archive with fixed time stamps and a fixed member order."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue(), compresslevel=9)


def main():
    import oracle
    oracle.build()
    pool = multiprocessing.Pool(min(8, os.cpu_count() or 1))
    # ---- shortwave ----
    arrays, meta = {}, {}
    tasks = [(n, i, im) for n, s in SW_SETS.items() for i in range(s["ncol"]) for im in (("f64", "f32") if s["f32"] else ("f64",))]
    tasks.sort(key=lambda t: -SW_SETS[t[0]]["nlay"] * (20 if SW_SETS[t[0]]["kind"] == "thick" else 1))
    results = dict(pool.imap_unordered(_sw_task, tasks, chunksize=1))
    for name, s in SW_SETS.items():
        inp = sw_inputs(name)
        for k, v in inp.items():
            arrays["%s.%s" % (name, k)] = v
        agree, digits, clamp = 0.0, 0, True
        for im in ("f64", "f32") if s["f32"] else ("f64",):
            cols = [results[(name, i, im)] for i in range(s["ncol"])]
            for k in cols[0][0]:
                arrays["%s.%s.%s" % (name, im, k)] = np.ascontiguousarray(np.stack([c[0][k] for c in cols], axis=-1))
            agree = max(agree, max(c[1] for c in cols))
            digits = max(digits, max(c[2] for c in cols))
            clamp = clamp and all(c[3] for c in cols)
        assert agree <= AGREE, (name, agree)
        if s["kind"] == "main":
            assert clamp, name + ": a layer leaves 0 <= Rdir <= 1 - Tnoscat, 0 <= Tdir <= 1 - Tnoscat - Rdir"
        assert incident(arrays, name).max() <= 1400.0
        dist = sw_oracle_distance(oracle, name, arrays)
        dmin = resonance_distance(inp["ssa"], inp["g"], inp["mu0"])
        meta[name] = dict(s, digits=digits, dps_agreement=agree, clamp_conditions_hold=bool(clamp),
                          resonance_distance_min=float(dmin.min()), oracle_distance=float(dist.max()))
        if s["kind"] == "resonance":
            arrays[name + ".d_min"] = dmin
            meta[name]["oracle_constant"] = float((dist * dmin / (2.0 ** -53 * incident(arrays, name))).max())
        if s["kind"] == "conservative":
            meta[name]["bar"] = 4.0 * float(dist.max())
        print("sw", name, json.dumps(meta[name]))
    arrays["meta"] = np.array(json.dumps(dict(dps=DPS, band2gpt=BAND2GPT.tolist(), sets=meta), sort_keys=True))
    write_npz(SW_PATH, arrays)
    # ---- longwave ----
    arrays, meta = {}, {}
    tasks = [(n, i, v) for n, s in LW_SETS.items() for i in range(s["ncol"]) for v in s["variants"]]
    tasks.sort(key=lambda t: -LW_SETS[t[0]]["nlay"] * int(t[2][1]))
    results = dict(pool.imap_unordered(_lw_task, tasks, chunksize=4))
    for name, s in LW_SETS.items():
        inp = lw_inputs(name)
        for k, v in inp.items():
            arrays["%s.%s" % (name, k)] = v
        agree, dist = 0.0, 0.0
        lev = inp["lev_source"]
        lay = 0.5 * (lev[:, 1:] + lev[:, :-1])
        assert np.array_equal(lay * 2.0, lev[:, 1:] + lev[:, :-1])
        emis = np.ascontiguousarray(inp["sfc_emis"][:, GPT2BAND].T)
        for v in s["variants"]:
            cols = [results[(name, i, v)] for i in range(s["ncol"])]
            for k in cols[0][0]:
                arrays["%s.%s.%s" % (name, vkey(v), k)] = np.ascontiguousarray(np.stack([c[0][k] for c in cols], axis=-1))
            agree = max(agree, max(c[1] for c in cols))
            if v[0] == "tab" and v[3] == "f64":
                opt = oracle.solver_options(lw_inc_flux_isotropic=int(v[2] == "isotropic"))
                fu, fd = oracle.rte_lw(inp["tau"], lay, np.ascontiguousarray(lev[:, 1:]), np.ascontiguousarray(lev[:, :-1]), emis,
                                       inp["sfc_source"], nmus=int(v[1]), inc_flux=None if v[2] == "none" else inp["inc_flux"],
                                       options=opt)
                eu, ed = arrays["%s.%s.up" % (name, vkey(v))], arrays["%s.%s.dn" % (name, vkey(v))]
                assert max(eu.max(), ed.max()) <= 500.0
                dist = max(dist, float(np.abs(fu - eu).max()), float(np.abs(fd - ed).max()))
        assert agree <= AGREE, (name, agree)
        meta[name] = dict(nlay=s["nlay"], ncol=s["ncol"], nprof=s["nprof"], bnd=s["bnd"], variants=[" ".join(v) for v in s["variants"]],
                          digits=DPS, dps_agreement=agree, oracle_distance=dist)
        print("lw", name, json.dumps({k: v for k, v in meta[name].items() if k != "variants"}))
    for n in (1, 2, 3, 4):
        D, w = exact_quadrature(n)
        arrays["exact_Ds_%d" % n], arrays["exact_wts_%d" % n] = np.array(D), np.array(w)
    arrays["meta"] = np.array(json.dumps(dict(dps=DPS, band2gpt=BAND2GPT.tolist(), sets=meta), sort_keys=True))
    write_npz(LW_PATH, arrays)
    pool.close()
    print("wrote", SW_PATH, os.path.getsize(SW_PATH), LW_PATH, os.path.getsize(LW_PATH))


if __name__ == "__main__":
    main()
