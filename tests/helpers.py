"""Shared test plumbing: product-side objects built from the synthetic generator."""
import math
import os

import numpy as np

from rte_ecckd_amd import synthetic

SW_NAMES = ["co2", "ch4", "n2o", "o2", "h2o", "o3"]     # gases of the shortwave tests
FLUX_ATOL = 1e-9                                         # fp64 flux tolerance against the oracle, W m-2
EPS32_THRESH = float(np.sqrt(np.float64(np.finfo(np.float32).eps)))   # rte_lw's tau_thresh in single precision


def r32(a):
    """float32-rounded copy, held in float64 (what the oracle is given in the single-precision tests)."""
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32), dtype=np.float64)


def product_gas_concs(pkg, cols, to=lambda a: a, names=None, overrides=None):
    """GasConcs in RFMIP order from synthetic columns; `to` moves arrays (e.g. to the GPU)."""
    names = list(synthetic.GAS_ORDER if names is None else names)
    gc = pkg.GasConcs(names)
    for n in names:
        v = (overrides or {}).get(n, cols.get(n, 0.0))
        if np.isscalar(v):
            assert gc.set_vmr(n, float(v)) == ""
        elif v.ndim == 1 and v.shape[0] == cols["plev"].shape[1]:
            assert gc.set_vmr_column(n, to(v)) == ""
        else:
            assert gc.set_vmr(n, to(v)) == ""
    return gc


def oracle_gas_items(cols, names=None, overrides=None):
    names = list(synthetic.GAS_ORDER if names is None else names)
    ncol = cols["plev"].shape[1]
    nlay = cols["tlay"].shape[0]
    items = []
    for n in names:
        v = (overrides or {}).get(n, cols.get(n, 0.0))
        if np.isscalar(v):
            items.append((n, np.array([v], dtype=np.float64), 0, 0))
        elif v.ndim == 1 and v.shape[0] == ncol:
            items.append((n, np.ascontiguousarray(v), 1, 0))
        elif v.ndim == 1 and v.shape[0] == nlay:
            items.append((n, np.ascontiguousarray(v), 0, 1))
        else:
            items.append((n, np.ascontiguousarray(v), 1, ncol))
    return items


def max_rel(a, b, floor=1e-300):
    a = np.asarray(a)
    b = np.asarray(b)
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), floor)))


def run_lw_gas_optics(pkg, k, cols, device=None, names=None, overrides=None, tlev=True, dtype=np.float64):
    """Product LW gas optics on numpy (host memspace) or torch (device memspace) arrays.
    Returns (err, tau, lay, inc, dec, sfc) as numpy arrays.  dtype float32: every array is passed in single
    precision (the _f32 entry points)."""
    ncol = cols["plev"].shape[1]
    nlay = cols["tlay"].shape[0]
    if device is None:
        to = lambda a: np.ascontiguousarray(a, dtype=dtype)
        like = np.empty(0, dtype)
        back = lambda a: a
    else:
        import torch
        to = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(device)
        like = to(np.zeros(1))
        back = lambda a: a.cpu().numpy()
    gc = product_gas_concs(pkg, cols, to, names, overrides)
    op = pkg.OpticalProps1scl()
    op.alloc_1scl(ncol, nlay, k, like=like)
    src = pkg.SourceFuncLW()
    src.alloc(ncol, nlay, k, like=like)
    err = k.gas_optics(None, to(cols["plev"]), to(cols["tlay"]), to(cols["tsfc"]), gc, op, src,
                       tlev=to(cols["tlev"]) if tlev else None)
    if device is not None:
        import torch
        torch.cuda.synchronize()
    return err, back(op.tau), back(src.lay_source), back(src.lev_source_inc), back(src.lev_source_dec), back(src.sfc_source)


# ------------------------------------------------------------------------------------------------
# Input columns shared by the fp64 and fp32 gas-optics tests
# ------------------------------------------------------------------------------------------------
def edge_columns(press_min, ncol=96):
    """Synthetic columns pushed through every branch of the gas optics."""
    c = synthetic.columns(1000, ncol, press_min)
    c = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in c.items()}
    c["h2o"][:, 0:8] = 1e-9                       # below the first h2o LUT node
    c["h2o"][:, 8:12] = 0.2                       # above the last node
    c["ch4"][12:20] = 1e-7                        # below reference -> negative -> clamped
    c["n2o"][12:20] = 1e-8
    c["tlev"][:, 20:24] = 100.0; c["tlay"][:, 20:24] = 100.0; c["tsfc"][20:24] = 110.0   # below Planck table
    c["tlev"][:, 24:28] = 400.0; c["tlay"][:, 24:28] = 400.0; c["tsfc"][24:28] = 360.0   # above it (extrapolates)
    c["plev"][:, 28:32] *= 1e-3                   # far below the pressure grid
    c["plev"][:, 32:36] *= 3.0                    # above it
    c["plev"][:, 36:40] *= np.linspace(0.3, 1.0, 4)[None, :]   # wide pressure spread inside one tile
    c["tlay"][:, 40:44] += 80.0                   # outside the 6-node T grid
    c["tlay"][:, 44:48] -= 80.0
    c["cfc11"][48:52] = 0.0
    return c


def orography_ramp(press_min, ncol=2048, c0=40):
    """Surface pressure ramps smoothly from 50 to 103 kPa across the columns: at the lower layers a
    4096-column segment spans more pressure rows than the LDS slab holds, so the fused kernel walks it once
    per slab position; most waves sit in one position, a few straddle two."""
    c = synthetic.columns(c0, ncol, press_min)
    c = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in c.items()}
    ps = np.linspace(50000.0, 103000.0, ncol)
    eta = (np.arange(61, dtype=np.float64) / 60) ** 2
    ptop = c["plev"][0, 0]
    c["plev"] = np.ascontiguousarray(ptop + (ps[None, :] - ptop) * eta[:, None])
    return c


# ------------------------------------------------------------------------------------------------
# Node-identity known answers from data the reference DOES hold: the three LUT files.
# These do not pin the code path (parity stays "unpinned"); they tie the oracle and the HIP path to
# reference-held numbers instead of to each other.
# ------------------------------------------------------------------------------------------------
PI_F32 = float(np.float32(3.14159265359))          # src/gas_optics_ecckd.f90:53
GLOBAL_WEIGHT = 1.0 / (float(np.float32(9.80665)) * float(np.float32(0.001)) * float(np.float32(28.970)))   # :107


def planck_node_case(m):
    """Temperatures that sit exactly on temperature_planck(k): the interpolation weights are (1, 0), so every
    source must equal planck_function(:,k)/pi (pi the f32-rounded literal), bit for bit (:275-288).
    Returns (cols-like dict with ncol = ntp, expected (ng, ntp))."""
    ntp, ng = m.ntp, m.ng
    T = m.temperature_planck.copy()
    nlay = 3
    p = np.exp(m.log_pressure[20]) * np.array([1.0, 1.1, 1.2, 1.3])
    cols = dict(plev=np.repeat(p[:, None], ntp, 1), tlay=np.repeat(T[None], nlay, 0),
                tlev=np.repeat(T[None], nlay + 1, 0), tsfc=T.copy())
    return cols, np.ascontiguousarray(m.planck_function.T) / PI_F32


def tau_node_cases(m, names=("co2", "ch4", "h2o")):
    """One gas at a time, layer pressure and temperature on table nodes where the index arithmetic is exact
    (pressure nodes 1 and 2: (lp - lp0)/dlp is 0 or 1 by construction; every temperature node but the last: the
    grid is exactly 20 K apart; h2o at its first mole-fraction node): tau must equal weight * coefficient(:,ip,it[,iv])
    with weight = global_weight*(p1-p0)*vmr (linear, look-up table) or *(vmr - ref) (relative-linear)
    (src/gas_optics_ecckd.f90:143-149,167-221), bit for bit.  Yields (gas, cols, gas item, expected (ng, 1, ncol))."""
    out = []
    for name in names:
        t = m.tables[m.gas.index(name)]
        cases = [(ip, it) for ip in (0, 1) for it in range(m.nt - 1)]   # (the last node is clamped to nt - 1.0001: :137)
        ncol = len(cases)
        plev = np.empty((2, ncol)); tlay = np.empty((1, ncol)); exp = np.empty((m.ng, 1, ncol))
        vmr = {"co2": 4e-4, "ch4": 2.5e-6}.get(name)     # (ch4 above its reference mole fraction: below it the per-gas clamp zeroes tau, :234-238)
        if t["code"] == 2:
            vmr = float(t["mole_fraction"][0])
        for c, (ip, it) in enumerate(cases):
            P = float(np.exp(m.log_pressure[ip]))
            if np.log(P) != m.log_pressure[ip]:            # exp/log round trip not exact: take the file's pressure
                from scipy.io import netcdf_file
                P = float(netcdf_file(m.path, mmap=False).variables["pressure"].data[ip])
            d = 2.0 ** np.floor(np.log2(P / 4))
            plev[0, c], plev[1, c] = P - d, P + d
            assert 0.5 * (plev[0, c] + plev[1, c]) == P
            tlay[0, c] = m.temperature[it, ip]
            sw = GLOBAL_WEIGHT * (plev[1, c] - plev[0, c])
            w = sw * (vmr - t["reference_mole_fraction"]) if t["code"] == 3 else sw * vmr
            exp[:, 0, c] = w * t["coefficient"][0, it, ip, :]
        cols = dict(plev=plev, tlay=tlay, tlev=np.repeat(tlay, 2, 0), tsfc=tlay[0].copy())
        out.append((name, cols, (name, np.array([vmr]), 0, 0), exp))
    return out


# ------------------------------------------------------------------------------------------------
# Longwave solver restated in numpy, in the operation order of rte_lw_kernel (kernels_rte_lw.hip), for a chosen
# precision: the float32 run predicts how far the single-precision kernel may sit from the fp64 oracle, the float64
# run shows that it restates the same solver (tests/test_oracle.py).
# ------------------------------------------------------------------------------------------------
GAUSS_DS = ((1.66,), (1.18350343, 2.81649655), (1.09719858, 1.69338507, 4.70941630),
            (1.06056257, 1.38282560, 2.40148179, 7.15513024))
GAUSS_WTS = ((0.5,), (0.3180413817, 0.1819586183), (0.2009319137, 0.2292411064, 0.0698269799),
             (0.1355069134, 0.2034645680, 0.1298475476, 0.0311809710))
LW_MAX_REGISTER_LAYERS = 96     # kMaxRegisterLayers: deeper grids take the overflow form
LW_PADDED_FORMS = (32, 48, 64, 80, 96)


def lw_group_width(nlay):
    """g-points one wave sums per shuffle: 64 / CW, CW = 32 (register forms) or 16 (overflow form)."""
    return 4 if nlay > LW_MAX_REGISTER_LAYERS else 2


def lw_emulate(tau, lay, inc, dec, emis_gpt, sfc, top_at_1=True, nmus=1, dtype=np.float32, series3=False,
               tau_thresh=None, inc_flux=None, inc_isotropic=False, gw=None, per_gpt=False):
    """Fluxes (up, dn) of rte_lw_kernel's per-(column, g-point, angle) recurrence -- the `layer` / `up` lambdas -- with
    every operation in `dtype`, and the broadband sums in float64 as the kernel's LDS accumulators hold them: the
    weighted intensities of one group of `gw` g-points are summed in `dtype` (the shuffle butterfly), the group sums
    are added into float64 in the kernel's iteration order (group-major, angle-minor).  Lanes beyond ng repeat the
    last g-point with weight 0, as the kernel's do.  tau_thresh None: sqrt(epsilon) of `dtype`.  per_gpt: also the
    spectral fluxes (ng, nlay+1, ncol) summed over angles in float64 (what oracle rte_lw_gpt returns)."""
    dt = np.dtype(dtype).type
    c = lambda a: np.asarray(a, dtype=dt)
    # float64: the C library's exp, as the oracle calls it (numpy's vectorised exp differs from it by up to a few ulp,
    # which the cancellation in (1 - t) / tl - t turns into 1e-10 W m-2)
    exp = np.exp if dt is not np.float64 else np.vectorize(math.exp, otypes=[np.float64])
    tau, lay, inc, dec, emis, sfc = map(c, (tau, lay, inc, dec, emis_gpt, sfc))
    ng, nlay, ncol = tau.shape
    gw = lw_group_width(nlay) if gw is None else gw
    thresh = dt(np.sqrt(np.finfo(dt).eps)) if tau_thresh is None else dt(tau_thresh)
    pi = dt(np.pi)                          # (real)acos(-1.)
    one, two, half, third, eighth = dt(1), dt(2), dt(0.5), dt(1) / dt(3), dt(1) / dt(8)
    walk = np.arange(nlay) if top_at_1 else np.arange(nlay - 1, -1, -1)    # layer walked s-th from the top
    bdn_a, bup_a = (inc, dec) if top_at_1 else (dec, inc)
    acc_dn = np.zeros((nlay + 1, ncol)); acc_up = np.zeros((nlay + 1, ncol))
    gacc_dn = np.zeros((ng, nlay + 1, ncol)) if per_gpt else None
    gacc_up = np.zeros((ng, nlay + 1, ncol)) if per_gpt else None

    lanes = np.arange(gw)

    def add(acc, gacc, s, v, g):
        """acc[s] += gsum(v) (butterfly over the lanes that share a column, in dtype), per g-point into gacc."""
        if gacc is not None:
            real = g < ng
            gacc[g[real], s] += v[real]
        o = 1
        while o < gw:
            v = v + v[lanes ^ o]
            o <<= 1
        acc[s] += v[0]

    with np.errstate(all="ignore"):
        for gb in range(0, ng, gw):
            g = gb + lanes
            gg = np.minimum(g, ng - 1)
            for k in range(nmus):
                D = dt(GAUSS_DS[nmus - 1][k])
                wk = dt(GAUSS_WTS[nmus - 1][k])
                wfac = np.where(g < ng, two * pi * wk, dt(0)).astype(dt)[:, None]
                if inc_flux is None:
                    I = np.zeros((gw, ncol), dt)
                else:
                    f = c(inc_flux)[gg]
                    I = f / pi if inc_isotropic else f / (two * pi * wk)
                T = np.empty((nlay, gw, ncol), dt); SU = np.empty((nlay, gw, ncol), dt)
                for s in range(nlay):
                    l = walk[s]
                    tl = tau[gg, l] * D
                    t = exp(-tl)
                    omt = one - t
                    big = omt / tl - t
                    small = tl * (half + tl * (-third + tl * eighth)) if series3 else tl * (half - third * tl)
                    fact = np.where(tl > thresh, big, small)
                    ly, bd, bu = lay[gg, l], bdn_a[gg, l], bup_a[gg, l]
                    sdn = omt * bd + two * fact * (ly - bd)
                    SU[s] = omt * bu + two * fact * (ly - bu)
                    T[s] = t
                    add(acc_dn, gacc_dn, s, wfac * I, g)
                    I = t * I + sdn
                add(acc_dn, gacc_dn, nlay, wfac * I, g)
                eps = emis[gg]
                U = I * (one - eps) + eps * sfc[gg]
                for s in range(nlay - 1, -1, -1):
                    add(acc_up, gacc_up, s + 1, wfac * U, g)
                    U = T[s] * U + SU[s]
                add(acc_up, gacc_up, 0, wfac * U, g)
    lev = slice(None) if top_at_1 else slice(None, None, -1)   # level s-th from the top -> array level
    out = (acc_up[lev], acc_dn[lev])
    if per_gpt:
        out += (gacc_up[:, lev], gacc_dn[:, lev])
    return out


def lw_seam_layers(nlay, top_at_1):
    """Array indices of the layers where rte_lw_kernel's forms change hands: the first layer walked; the last present
    layer of a padded form (every depth but the exact 60-layer form, up to 96 layers); the two layers on either side
    of the ring/register boundary of the overflow form (walked nover - 1 and nover, nover = nlay - 96)."""
    at = lambda s: s if top_at_1 else nlay - 1 - s
    seams = [at(0)]
    if nlay != 60 and nlay <= LW_MAX_REGISTER_LAYERS:
        seams.append(at(nlay - 1))
    if nlay > LW_MAX_REGISTER_LAYERS:
        nover = nlay - LW_MAX_REGISTER_LAYERS
        seams += [at(nover - 1), at(nover)]
    return sorted(set(seams))


def lw_f32_bar(case, top_at_1, nmus, ref, **emu):
    """Flux bar of a single-precision solver case: 4 x the float32 restatement's largest distance from the fp64 oracle
    (`ref` = (up, dn) of the oracle), at least 1e-4 W m-2.  `case` holds tau, lay, inc, dec, emis_gpt, sfc."""
    eu, ed = lw_emulate(case["tau"], case["lay"], case["inc"], case["dec"], case["emis_gpt"], case["sfc"], top_at_1,
                        nmus, np.float32, **emu)
    ok_u, ok_d = np.isfinite(ref[0]), np.isfinite(ref[1])
    dev = max(np.max(np.abs(eu - ref[0])[ok_u], initial=0.0), np.max(np.abs(ed - ref[1])[ok_d], initial=0.0))
    return max(4.0 * dev, 1e-4)


def lw_flux_changes(oracle_mod, case, top_at_1, nmus, ref, seams, **oracle_kw):
    """The oracle's flux changes (largest over all levels and columns) when one seam layer is made transparent
    (tau = 0 in every g-point and column) and when top_at_1 is flipped: a bar must stay far below each."""
    def run(tau, t1):
        return oracle_mod.rte_lw(tau, case["lay"], case["inc"], case["dec"], case["emis_gpt"], case["sfc"],
                                 top_at_1=t1, nmus=nmus, **oracle_kw)

    def change(out):
        ok = np.isfinite(ref[0]) & np.isfinite(ref[1])
        return max(np.max(np.abs(out[0] - ref[0])[ok], initial=0.0), np.max(np.abs(out[1] - ref[1])[ok], initial=0.0))
    out = {}
    for l in seams:
        t = case["tau"].copy()
        t[:, l, :] = 0.0
        out["tau0@%d" % l] = change(run(t, top_at_1))
    out["flip"] = change(run(case["tau"], not top_at_1))
    return out


# ------------------------------------------------------------------------------------------------
# Columns that take every branch of the reference's gas optics once (tests/test_oracle_vs_reference.py,
# tests/golden/make_golden_ref.py).  Each column is named after the branch it takes.
# ------------------------------------------------------------------------------------------------
BRANCH_COLUMNS = ("synthetic0", "synthetic1", "p_below_grid", "p_above_110kPa", "t_above_grid", "t_below_grid",
                  "planck_below_120K", "planck_at_120K", "planck_at_350K", "planck_above_350K", "h2o_below_lut",
                  "h2o_above_lut", "h2o_zero", "rel_lin_below_ref", "rel_lin_at_ref", "rel_lin_above_ref",
                  "zero_thickness", "wide_p_spread", "synthetic2", "synthetic3")


def branch_columns(m, nlay=60, bottom_first=False, c0=3000):
    """One synthetic column per name in BRANCH_COLUMNS, altered to take that branch of
    src/gas_optics_ecckd.f90 in `m` (a CkdModel): the p and T clamps (:122-140, 1.0001), the h2o
    mole-fraction clamps (:153-160, 1.001) and h2o = 0, the relative-linear gases below, exactly at
    and above their reference mole fraction (:145-146; below it the per-gas clamp :234-238 zeroes
    them), Planck temperatures below, at both ends of and above temperature_planck (:275-285),
    zero-thickness layers (simple_weight = 0: tau = 0, and ssa = 0/0 in the shortwave).
    bottom_first: levels stored surface first (simple_weight < 0).  No NaN anywhere: the reference
    would index its tables with int(NaN)."""
    press_min = float(np.exp(m.log_pressure[0]))
    ncol = len(BRANCH_COLUMNS)
    c = synthetic.columns(c0, ncol, press_min, nlay=nlay)
    c = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in c.items()}
    col = {n: i for i, n in enumerate(BRANCH_COLUMNS)}
    for n in ("ch4", "n2o", "cfc11", "cfc12", "co2"):
        c[n] = np.full(ncol, c[n]) if np.isscalar(c[n]) else c[n]
    c["plev"][:, col["p_below_grid"]] *= 5e-6       # the whole column above the grid top
    c["plev"][:, col["p_above_110kPa"]] *= 1.5
    c["tlay"][:, col["t_above_grid"]] += 120.0      # the T grid is 5 x 20 K wide
    c["tlay"][:, col["t_below_grid"]] -= 120.0
    if m.temperature_planck is not None:
        tp0, tp1 = float(m.temperature_planck[0]), float(m.temperature_planck[-1])
        for name, t, ts in (("planck_below_120K", 100.0, 110.0), ("planck_at_120K", tp0, tp0),
                            ("planck_at_350K", tp1, tp1), ("planck_above_350K", 400.0, 360.0)):
            c["tlev"][:, col[name]] = t
            c["tlay"][:, col[name]] = t
            c["tsfc"][col[name]] = ts
    h2o = m.tables[m.gas.index("h2o")]["mole_fraction"]
    c["h2o"][:, col["h2o_below_lut"]] = 0.1 * h2o[0]
    c["h2o"][:, col["h2o_above_lut"]] = 4.0 * h2o[-1]
    c["h2o"][:, col["h2o_zero"]] = 0.0
    for name, t in zip(m.gas, m.tables):
        if t["code"] == 3 and name in c:
            ref = t["reference_mole_fraction"]
            c[name][col["rel_lin_below_ref"]] = 0.5 * ref
            c[name][col["rel_lin_at_ref"]] = ref
            c[name][col["rel_lin_above_ref"]] = 2.0 * ref
    z = col["zero_thickness"]
    c["plev"][1, z] = c["plev"][0, z]                         # the top layer
    c["plev"][nlay // 3 + 1:nlay // 3 + 4, z] = c["plev"][nlay // 3, z]   # three layers in the middle
    c["plev"][:, col["wide_p_spread"]] *= np.linspace(0.3, 1.4, nlay + 1)
    c["plev"][:, col["wide_p_spread"]] = np.maximum.accumulate(c["plev"][:, col["wide_p_spread"]])
    if bottom_first:
        for k in ("plev", "tlev", "tlay", "h2o", "o3"):
            c[k] = np.ascontiguousarray(c[k][::-1])
    return c


# ------------------------------------------------------------------------------------------------
# Reference fixtures: inputs and outputs of the reference's own gas-optics module on the branch columns
# (tests/golden/make_golden_ref.py writes them; the GPU suite reads them without the reference tree).
# ------------------------------------------------------------------------------------------------
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
REF_FIXTURE_SETS = (("lw_fsck", 60), ("lw_rrtmgp", 30), ("sw_wide", 60), ("lw_fsck", 137))
REF_FIXTURE_GASES = synthetic.GAS_ORDER + ["n2"]     # RFMIP order, no2 (unknown to the tables), then n2
WELL_MIXED = dict(co2=420e-6, ch4=1.9e-6, n2o=3.3e-7, cfc11=2.3e-10, cfc12=5.2e-10, o2=0.209)   # ch4 below its reference


def ref_fixture_path(key, nlay):
    return os.path.join(GOLDEN, "ref_%s_%d.npz" % (key, nlay))


def load_ref_fixture(key, nlay):
    """(cols, outputs, column names) of one reference fixture.  cols as synthetic.columns gives them (scalar gases
    as floats); outputs in the shapes and order gas_optics returns them: longwave (tau, lay_source, lev_source_inc,
    lev_source_dec, sfc_source), shortwave (tau, ssa, g, toa_src)."""
    z = np.load(ref_fixture_path(key, nlay))
    cols = {}
    for k in ("plev", "tlev", "tlay", "tsfc", "h2o", "o3") + tuple(REF_FIXTURE_GASES):
        if k in z.files:
            v = z[k]
            cols[k] = float(v) if v.ndim == 0 else np.ascontiguousarray(v)
    if key.startswith("sw"):
        out = tuple(z[k] for k in ("tau", "ssa", "g", "toa_src"))
    else:
        lev = z["lev_source"]
        out = (z["tau"], z["lay_source"], np.ascontiguousarray(lev[:, 1:]), np.ascontiguousarray(lev[:, :-1]),
               z["sfc_source"])
    return cols, out, [str(n) for n in z["columns"]]
