"""Writes tests/golden/lw_2stream_truth.npz: inputs of the two-stream longwave solver and the fluxes that
tests/lw_2stream_ref.truth (a multi-digit boundary-value solution, independent of the product and of the numpy
restatement) gives for them, rounded once to float64.

    python tests/golden/make_golden_lw_2stream.py        (needs mpmath; about a minute)

Run twice it writes identical files: seeded generators, fixed time stamps in the archive.  3 g-points in two bands
(truth_fixture.BAND2GPT), 9 columns, emissivity per band in [0.8, 1], an incident flux in columns 1, 4 and 7.  Arrays are
stored top first (top_at_1); lw_2stream_ref.flip_orientation gives the other orientation.

Sets
  cloudy_n1, _n2, _n8, _n61   tau log-uniform in [1e-2, 30], ssa in [0, 0.999], g in [-0.2, 0.9]; a few tau = 0 layers;
                              ssa = 0 in columns 2 and 6; lev_source_inc(l) != lev_source_dec(l+1) at interior levels in
                              the odd columns (the geometric mean is exercised)
  thin_n8                     tau log-uniform in [1e-6, 1e-2], temperature steps of 3..8 K between levels
  near_conservative_n8        ssa = 1 - 10^-u, u in [3, 6] (up to 0.999999); ssa = 1 exactly in about 40 % of the layers
  cutoff_n8                   cloudy, with layers of 0 < tau <= 1e-8 (the solver drops their sources by definition, the
                              truth does not): expected fluxes are the RESTATEMENT's; bar helpers.FLUX_ATOL

Metadata per set: `restate_distance`, the largest distance (W m-2, broadband and per g-point, both orientations) of the
numpy restatement from the truth, and `bar` = 4 x that -- the rule of the shortwave `conservative` sets: the factor
covers the device's exp / sqrt / reciprocal and the order of the g-point sum.  Every `cloudy` bar must be at most
helpers.FLUX_ATOL (asserted below).
"""
import io
import json
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import lw_2stream_ref as ref   # noqa: E402

FLUX_ATOL = 1e-9               # helpers.FLUX_ATOL (helpers imports the package; the generator needs none of it)
BAND2GPT = [[1, 2], [3, 3]]
GPT2BAND = np.array([0, 0, 1])
NG, NCOL = 3, 9
PATH = os.path.join(HERE, "lw_2stream_truth.npz")
SETS = (("cloudy_n1", "cloudy", 1), ("cloudy_n2", "cloudy", 2), ("cloudy_n8", "cloudy", 8), ("cloudy_n61", "cloudy", 61),
        ("thin_n8", "thin", 8), ("near_conservative_n8", "near_conservative", 8), ("cutoff_n8", "cutoff", 8))


def planck_like(T, scale):
    """A smooth source (W m-2 sr-1) of the level temperature; pi B is about 13 W m-2 at 250 K for scale 4."""
    return scale * (T / 250.0) ** 4


def make_inputs(kind, nlay, seed):
    rng = np.random.default_rng(seed)
    shape = (NG, nlay, NCOL)
    if kind == "thin":
        tau = 10.0 ** rng.uniform(-6.0, -2.0, shape)
    else:
        tau = 10.0 ** rng.uniform(-2.0, np.log10(30.0), shape)
    ssa = rng.uniform(0.0, 0.999, shape)
    g = rng.uniform(-0.2, 0.9, shape)
    if kind == "near_conservative":
        ssa = 1.0 - 10.0 ** -rng.uniform(3.0, 6.0, shape)
        ssa[rng.uniform(size=shape) < 0.4] = 1.0
    ssa[:, :, 2] = 0.0
    ssa[:, :, 6] = 0.0
    if kind in ("cloudy", "cutoff") and nlay >= 2:
        tau[rng.uniform(size=shape) < 0.06] = 0.0
    if kind == "cutoff":
        pick = rng.uniform(size=shape)
        tau[pick < 0.15] = 1e-8
        tau[(pick >= 0.15) & (pick < 0.3)] = 10.0 ** rng.uniform(-14.0, -8.5, shape)[(pick >= 0.15) & (pick < 0.3)]
    step = rng.uniform(3.0, 8.0, (nlay + 1, NCOL)) if kind == "thin" else rng.uniform(0.2, 80.0 / (nlay + 1), (nlay + 1, NCOL))
    step *= rng.choice([1.0, 1.0, 1.0, -1.0], size=step.shape)                 # mostly warmer downwards, some inversions
    T = 215.0 + np.cumsum(step, axis=0)
    scale = np.array([3.0, 4.0, 5.0])[:, None, None]
    lev = planck_like(T[None], scale)                                            # (NG, nlay + 1, NCOL)
    inc, dec = np.ascontiguousarray(lev[:, 1:]), np.ascontiguousarray(lev[:, :-1])
    if nlay >= 2:   # odd columns: the two arrays disagree at the interior levels by up to 2 %
        inc[:, :-1, 1::2] *= 1.0 + rng.uniform(-0.02, 0.02, (NG, nlay - 1, NCOL))[:, :, 1::2]
    sfc_emis = rng.uniform(0.8, 1.0, (NCOL, 2))
    sfc_emis[0] = 1.0
    tsfc = T[-1] + rng.uniform(-3.0, 3.0, NCOL)
    sfc_source = np.ascontiguousarray(planck_like(tsfc[None], scale[:, 0]))
    inc_flux = np.zeros((NG, NCOL))
    inc_flux[:, 1::3] = rng.uniform(0.5, 20.0, (NG, NCOL))[:, 1::3]
    return dict(tau=tau, ssa=ssa, g=g, inc=inc, dec=dec, sfc_emis=sfc_emis, sfc_source=sfc_source, inc_flux=inc_flux)


def per_gpt(a):
    return np.ascontiguousarray(a[:, GPT2BAND].T)


def solve(fn, a, top_at_1):
    return fn(a["tau"], a["ssa"], a["g"], a["inc"], a["dec"], per_gpt(a["sfc_emis"]), a["sfc_source"], a["inc_flux"], top_at_1)


def main():
    arrays, meta = {}, {}
    for k, (name, kind, nlay) in enumerate(SETS):
        a = make_inputs(kind, nlay, 20260 + k)
        for key, v in a.items():
            arrays["%s.%s" % (name, key)] = v
        ru, rd = solve(ref.restate, a, True)
        rec = dict(nlay=nlay, kind=kind)
        if kind == "cutoff":
            assert np.any((a["tau"] > 0) & (a["tau"] <= ref.TAU_MIN))
            gu, gd = ru, rd
            up, dn = ref.broadband(ru), ref.broadband(rd)
            rec.update(against="restate", bar=FLUX_ATOL)
        else:
            tu, td = solve(ref.truth, a, True)
            gu, gd = ref.to_f64(tu), ref.to_f64(td)
            up, dn = ref.to_f64(ref.sum_gpts(tu)), ref.to_f64(ref.sum_gpts(td))
            # the other orientation solves the same problem: the truth must not care, the restatement is measured in both
            b = ref.flip_orientation(a)
            fu, fd = solve(ref.truth, b, False)
            assert np.array_equal(ref.to_f64(fu)[:, ::-1], gu) and np.array_equal(ref.to_f64(fd)[:, ::-1], gd), name
            qu, qd = solve(ref.restate, b, False)
            dist = max(np.max(np.abs(ru - gu)), np.max(np.abs(rd - gd)), np.max(np.abs(ref.broadband(ru) - up)),
                       np.max(np.abs(ref.broadband(rd) - dn)), np.max(np.abs(ref.broadband(qu)[::-1] - up)),
                       np.max(np.abs(ref.broadband(qd)[::-1] - dn)))
            rec.update(against="truth", restate_distance=float(dist), bar=float(4.0 * dist))
            if kind == "cloudy":
                assert rec["bar"] <= FLUX_ATOL, (name, rec)
        arrays[name + ".up"], arrays[name + ".dn"] = up, dn
        arrays[name + ".gpt_up"], arrays[name + ".gpt_dn"] = gu, gd
        meta[name] = rec
        print(name, rec, "max flux %.2f" % float(np.max(up)), flush=True)
    arrays["meta"] = np.array(json.dumps(dict(band2gpt=BAND2GPT, sets=meta), sort_keys=True))
    with zipfile.ZipFile(PATH, "w") as z:   # fixed time stamps: the same bytes on every run
        for key in sorted(arrays):
            buf = io.BytesIO()
            np.save(buf, arrays[key] if arrays[key].ndim == 0 else np.ascontiguousarray(arrays[key]))
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())
    print("wrote", PATH, os.path.getsize(PATH), "bytes")


if __name__ == "__main__":
    main()
