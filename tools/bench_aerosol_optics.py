#!/usr/bin/env python3
"""Aerosol-optics timings (ecckd_aerosol_optics / _f32, device arrays) at 60 layers with synthetic.aerosols and
synthetic.aerosol_lut(nband, 5, 36) (MERRA-sized: LDS route at 1 band, L2 route at 5 and 16 bands in fp64), fp64 and
float32, 1e5 and 1e6 columns, 1 / 5 / 16 bands, nspec 1 / 5 / 15.  The inputs are generated for 1e5 columns; the 1e6-column
case repeats them ten times along the columns.  Per case, in one process, every variant timed five times (min-max kept):
  call              one two-stream call, nspec species          4*nspec + (2*nspec + 1 + 3*nband) reals per cell
  copy              a torch copy_ of as many bytes (read + written) as `call` moves: the copy yardstick of the cloud-optics row
  chained           nspec single-species calls: the first into the result planes, each other one into a second set of planes
                    and then the band-grid increment onto the result (what a host has to do without nspec and accumulate)
  accumulate        one call with accumulate=1 onto planes that hold the clouds
  plain_increment   the plain call into a second set of planes, then the band-grid increment
and, in fp64 with nspec = 5, the call in front of the fused all-sky calls:
  lw_allsky / aerosol_lw_allsky   lw_fluxes_allsky alone / after an accumulating aerosol call   (1-band and 16-band files)
  sw_allsky / aerosol_sw_allsky   sw_fluxes_allsky alone / after an accumulating aerosol call   (5-band file)
HIP-event timing: 3 warm-up calls per variant, then the variants interleaved round-robin.
Usage: python tools/bench_aerosol_optics.py [--sizes 100000,1000000] [--repeats 5] [--out profiles/aerosol_optics.json]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = os.path.join(ROOT, "data")
LW_FILES = {1: os.path.join(DATA, "ecckd-1.2_lw_ckd-definition_climate_fsck-tol0.0161.nc"),
            16: os.path.join(DATA, "ecckd-1.2_lw_ckd-definition_climate_rrtmgp-tol0.061.nc")}
SW_FILE = os.path.join(DATA, "ecckd-1.2_sw_ckd-definition_climate_wide-tol0.05.nc")
NBANDS, NSPECS, NLAY, NBIN, NRH, BASE_COLS = (1, 5, 16), (1, 5, 15), 60, 5, 36, 100000
TABLE_NAMES = ("merra_aero_bin_lims", "aero_rh", "aero_dust_tbl", "aero_salt_tbl", "aero_sulf_tbl", "aero_bcar_tbl",
               "aero_bcar_rh_tbl", "aero_ocar_tbl", "aero_ocar_rh_tbl")


def stats(ms):
    ms = sorted(ms)
    return {"median_ms": ms[len(ms) // 2], "min_ms": ms[0], "max_ms": ms[-1], "n": len(ms)}


def interleaved(variants, repeats):
    """{name: stats}: every variant warmed up three times, then timed `repeats` times round-robin with HIP events."""
    import torch
    for fn in variants.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    out = {n: [] for n in variants}
    for _ in range(repeats):
        for n, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            out[n].append(e0.elapsed_time(e1))
    return {n: stats(v) for n, v in out.items()}


def check(msg):
    if msg:
        raise SystemExit(msg)


def apart(a, b):
    """the min-max ranges of two variants do not overlap"""
    return a["max_ms"] < b["min_ms"] or b["max_ms"] < a["min_ms"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="100000,1000000")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sizes = sorted(int(s) for s in args.sizes.split(",") if s)

    import torch
    sys.path.insert(0, ROOT)
    import rte_ecckd_amd as pkg
    from rte_ecckd_amd import synthetic
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    base = min(BASE_COLS, sizes[-1])
    aer_np = synthetic.aerosols(0, base, NLAY, max(NSPECS))
    none_fraction = float((aer_np[0] == 0).mean())
    clear_cell_fraction = float((aer_np[0] == 0).all(axis=0).mean())
    cld_np = synthetic.clouds(0, base, NLAY, max(NBANDS))
    luts = {nband: synthetic.aerosol_lut(nband, NBIN, NRH) for nband in NBANDS}
    objs = {}
    for nband, lut in luts.items():
        objs[nband] = pkg.AerosolOptics()
        check(objs[nband].load(None, *[lut[n] for n in TABLE_NAMES], device=0))
    cases, chain = [], []
    for f32 in (False, True):
        tdt, es = (torch.float32, 4) if f32 else (torch.float64, 8)
        for ncol in sizes:
            reps = -(-ncol // base)
            wide = lambda a: t(a).repeat(*([1] * (a.ndim - 1)), reps)[..., :ncol].contiguous()
            kind = wide(aer_np[0])
            size, mass, rh = (wide(a).to(tdt) for a in aer_np[1:])
            ncell = ncol * NLAY
            for nband in NBANDS:
                ao = objs[nband]
                cld = [wide(cld_np[n][:nband]).to(tdt) for n in ("tau", "ssa", "g")]
                op, tmp = pkg.OpticalProps2str(), pkg.OpticalProps2str()
                op.tau, op.ssa, op.g = (c.clone() for c in cld)
                tmp.tau, tmp.ssa, tmp.g = (torch.empty_like(c) for c in cld)
                for nspec in NSPECS:
                    k3, s3, m3 = kind[:nspec], size[:nspec], mass[:nspec]
                    nbytes = ncell * (4 * nspec + es * (2 * nspec + 1 + 3 * nband))
                    src, dst = (torch.empty(nbytes // 2 // es, dtype=tdt, device=dev) for _ in range(2))

                    def call():
                        check(ao.aerosol_optics(k3, s3, m3, rh, op))

                    def chained():
                        check(ao.aerosol_optics(k3[0], s3[0], m3[0], rh, op))
                        for s in range(1, nspec):
                            check(ao.aerosol_optics(k3[s], s3[s], m3[s], rh, tmp))
                            check(op.increment(tmp))

                    def accumulate():
                        check(ao.aerosol_optics(k3, s3, m3, rh, op, accumulate=True))

                    def plain_increment():
                        check(ao.aerosol_optics(k3, s3, m3, rh, tmp))
                        check(op.increment(tmp))

                    res = interleaved({"call": call, "copy": lambda: dst.copy_(src), "chained": chained,
                                       "accumulate": accumulate, "plain_increment": plain_increment}, args.repeats)
                    entry = {"dtype": "f32" if f32 else "f64", "ncol": ncol, "nlay": NLAY, "nband": nband, "nspec": nspec,
                             "bytes": nbytes, "results": res,
                             "call_TB_per_s": nbytes / (res["call"]["median_ms"] * 1e-3) / 1e12,
                             "call_fraction_of_copy": res["copy"]["median_ms"] / res["call"]["median_ms"],
                             "chained_over_call": res["chained"]["median_ms"] / res["call"]["median_ms"],
                             "chained_and_call_ranges_apart": apart(res["chained"], res["call"]),
                             "plain_increment_over_accumulate": res["plain_increment"]["median_ms"] / res["accumulate"]["median_ms"],
                             "plain_increment_and_accumulate_ranges_apart": apart(res["plain_increment"], res["accumulate"])}
                    cases.append(entry)
                    print(json.dumps(entry), flush=True)
                    del src, dst
                if not f32:   # the call in front of the fused all-sky calls, nspec = 5
                    files = ([("lw", LW_FILES[nband])] if nband in LW_FILES else []) + ([("sw", SW_FILE)] if nband == 5 else [])
                    for which, path in files:
                        k = pkg.GasOpticsEcckd()
                        check(k.load(path, device=0))
                        assert k.get_nband() == nband
                        cols = synthetic.columns(0, ncol, k.get_press_min(), nlay=NLAY, shortwave=which == "sw")
                        names = synthetic.GAS_ORDER if which == "lw" else ["co2", "ch4", "n2o", "o2", "h2o", "o3"]
                        gc = pkg.GasConcs(names)
                        for n in names:
                            v = cols[n]
                            if np.isscalar(v):
                                gc.set_vmr(n, float(v))
                            elif v.ndim == 1:
                                gc.set_vmr_column(n, t(v))
                            else:
                                gc.set_vmr(n, t(v))
                        plev, tlay = t(cols["plev"]), t(cols["tlay"])
                        fl = pkg.FluxesBroadband(*(torch.empty((NLAY + 1, ncol), dtype=torch.float64, device=dev)
                                                   for _ in range(2 if which == "lw" else 3)))
                        if which == "lw":
                            tlev, tsfc = t(cols["tlev"]), t(cols["tsfc"])
                            emis = t(np.repeat(cols["sfc_emis"][:, None], nband, 1))
                            allsky = lambda: check(k.lw_fluxes_allsky(plev, tlay, tsfc, tlev, gc, True, emis, op, fl))
                        else:
                            mu0, alb = t(cols["mu0"]), t(np.repeat(cols["albedo"][:, None], nband, 1))
                            alb2 = alb.clone()
                            allsky = lambda: check(k.sw_fluxes_allsky(plev, tlay, gc, True, mu0, alb, alb2, op, fl, delta_scale=True))

                        def both():
                            for a, c in zip((op.tau, op.ssa, op.g), cld):
                                a.copy_(c)
                            check(ao.aerosol_optics(kind[:5], size[:5], mass[:5], rh, op, accumulate=True))
                            allsky()

                        def reset_and_allsky():   # the same plane refresh, so that the ratio isolates the aerosol call
                            for a, c in zip((op.tau, op.ssa, op.g), cld):
                                a.copy_(c)
                            allsky()

                        res = interleaved({which + "_allsky": reset_and_allsky, "aerosol_" + which + "_allsky": both}, args.repeats)
                        entry = {"ncol": ncol, "nlay": NLAY, "nband": nband, "ngpt": k.get_ngpt(), "nspec": 5, "results": res,
                                 "chain_over_allsky_alone": res["aerosol_" + which + "_allsky"]["median_ms"]
                                 / res[which + "_allsky"]["median_ms"]}
                        chain.append(entry)
                        print(json.dumps(entry), flush=True)
                        del k, gc, allsky, both, reset_and_allsky, fl
                        pkg.release_scratch(0)
                del op, tmp, cld
                torch.cuda.empty_cache()
    out = {"device": torch.cuda.get_device_name(0), "build": pkg.lib().ecckd_build_info().decode(), "repeats": args.repeats,
           "timing": "HIP events, 3 warm-up calls, variants interleaved; min-max of `repeats` calls",
           "tables": "synthetic.aerosol_lut(nband, 5, 36)", "inputs": "synthetic.aerosols(0, %d, 60, 15), repeated along the columns" % base,
           "none_fraction": none_fraction, "clear_cell_fraction": clear_cell_fraction, "aerosol_optics": cases, "chain": chain}
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
