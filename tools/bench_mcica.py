#!/usr/bin/env python3
"""McICA timings, fp64, synthetic.clouds / synthetic.cloud_fraction, per shape
(sw | lw_fsck | lw_rrtmgp, ncol, 60 layers):
  (a) the existing calls -- clear-sky fused fluxes and the unmasked fused all-sky call -- on this build and, with
      --parent-lib, on another build of the library (the parent commit's), in fresh child processes that alternate, so
      the two builds are compared on the same box in one job;
  (b) on this build, interleaved in one process: the unmasked fused all-sky call, the masked one (cloud_mask=), the
      general route with a mask (longwave: gas_optics_tau + increment(cloud_mask=) + rte_lw_fused; shortwave:
      gas_optics + delta_scale of a copy + increment(cloud_mask=) + rte_sw), ecckd_cloud_mask_sample alone for both
      overlaps (ms and GB/s of mask written), and ecckd_increment by band with and without a mask.
HIP-event timing: 3 warm-up calls, then --repeats timed calls per variant, the variants interleaved round-robin; median
and min-max.  Usage: python tools/bench_mcica.py [--shapes sw:100000,lw_fsck:100000,...] [--parent-lib lib.so] [--out f.json]"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_allsky import interleaved, stats  # noqa: E402

DATA = os.path.join(ROOT, "data")
FILES = {"sw": "ecckd-1.2_sw_ckd-definition_climate_wide-tol0.05.nc", "lw_fsck": "ecckd-1.2_lw_ckd-definition_climate_fsck-tol0.0161.nc",
         "lw_rrtmgp": "ecckd-1.2_lw_ckd-definition_climate_rrtmgp-tol0.061.nc"}
SW_NAMES = ["co2", "ch4", "n2o", "o2", "h2o", "o3"]


def child(kind, ncol, nlay, repeats, existing_only):
    import torch
    sys.path.insert(0, ROOT)
    import rte_ecckd_amd as pkg
    from rte_ecckd_amd import synthetic
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)

    def check(msg):
        if msg:
            raise SystemExit(msg)

    sw = kind == "sw"
    k = pkg.GasOpticsEcckd()
    check(k.load(os.path.join(DATA, FILES[kind]), device=0))
    ng, nb = k.get_ngpt(), k.get_nband()
    cols = synthetic.columns(0, ncol, k.get_press_min(), nlay=nlay, shortwave=sw)
    cloud = synthetic.clouds(0, ncol, nlay, nb)
    names = SW_NAMES if sw else synthetic.GAS_ORDER
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
    part = pkg.OpticalProps2str()
    part.tau, part.ssa, part.g = t(cloud["tau"]), t(cloud["ssa"]), t(cloud["g"])
    fl = pkg.FluxesBroadband(*(torch.empty((nlay + 1, ncol), dtype=torch.float64, device=dev) for _ in range(3 if sw else 2)))
    if sw:
        rng = np.random.default_rng(nlay)
        mu0, ad, af = t(cols["mu0"]), t(rng.uniform(0.02, 0.6, (ncol, nb))), t(rng.uniform(0.02, 0.6, (ncol, nb)))
        clear = lambda: check(k.sw_fluxes(plev, tlay, gc, True, mu0, ad, af, fl))
        allsky = lambda **kw: check(k.sw_fluxes_allsky(plev, tlay, gc, True, mu0, ad, af, part, fl, delta_scale=True, **kw))
    else:
        tsfc, tlev = t(cols["tsfc"]), t(cols["tlev"])
        emis = t(np.repeat(cols["sfc_emis"][:, None], nb, 1))
        clear = lambda: check(k.lw_fluxes(plev, tlay, tsfc, tlev, gc, True, emis, fl))
        allsky = lambda **kw: check(k.lw_fluxes_allsky(plev, tlay, tsfc, tlev, gc, True, emis, part, fl, **kw))
    variants = {"clear_fused": clear, "allsky_fused": allsky}
    fits = ncol * nlay * ng * 8 * (3 if sw else 1) < 40e9
    if existing_only and fits:   # ecckd_increment by band on the build under ECCKD_LIB (the parent's, for the masked one's yardstick)
        b2g = k.get_band2gpt()
        if sw:
            op = pkg.OpticalProps2str(); op.alloc_2str(ncol, nlay, k, like=plev)
            check(k.gas_optics(None, plev, tlay, gc, op, torch.empty((ng, ncol), dtype=torch.float64, device=dev)))
        else:
            op = pkg.OpticalProps1scl(); op.alloc_1scl(ncol, nlay, k, like=plev)
            check(k.gas_optics_tau(plev, tlay, gc, op))
        variants["increment_by_band"] = lambda: check(op.increment(part, band2gpt=b2g))
    if not existing_only:
        cf = t(synthetic.cloud_fraction(0, ncol, nlay))
        alpha = torch.full((nlay - 1, ncol), 0.7, dtype=torch.float64, device=dev)
        mask = pkg.sample_cloud_mask(cf, ng, seed=1)
        variants["allsky_fused_masked"] = lambda: allsky(cloud_mask=mask)
        b2g = k.get_band2gpt()
        if fits:
            if sw:
                op = pkg.OpticalProps2str(); op.alloc_2str(ncol, nlay, k, like=plev)
                work = pkg.OpticalProps2str(); work.alloc_2str_bands(ncol, nlay, k, like=plev)
                toa = torch.empty((ng, ncol), dtype=torch.float64, device=dev)

                def general():
                    check(k.gas_optics(None, plev, tlay, gc, op, toa))
                    work.tau.copy_(part.tau); work.ssa.copy_(part.ssa); work.g.copy_(part.g)
                    check(work.delta_scale())
                    check(op.increment(work, band2gpt=b2g, cloud_mask=mask))
                    check(pkg.rte_sw(op, True, mu0, toa, ad, af, fl))
            else:
                op = pkg.OpticalProps1scl(); op.alloc_1scl(ncol, nlay, k, like=plev)

                def general():
                    check(k.gas_optics_tau(plev, tlay, gc, op))
                    check(op.increment(part, band2gpt=b2g, cloud_mask=mask))
                    check(k.rte_lw_fused(op, True, tlay, tlev, tsfc, emis, fl))
            check(k.gas_optics(None, plev, tlay, gc, op, toa) if sw else k.gas_optics_tau(plev, tlay, gc, op))
            variants["general_route_masked"] = general
            variants["increment_by_band"] = lambda: check(op.increment(part, band2gpt=b2g))
            variants["increment_by_band_masked"] = lambda: check(op.increment(part, band2gpt=b2g, cloud_mask=mask))
        variants["sample_max_ran"] = lambda: pkg.sample_cloud_mask(cf, ng, seed=1)
        variants["sample_exp_ran"] = lambda: pkg.sample_cloud_mask(cf, ng, "exp_ran", alpha, seed=1)
    res = {n: stats(v) for n, v in interleaved(variants, repeats).items()}
    out = {"kind": kind, "ncol": ncol, "nlay": nlay, "ngpt": ng, "nband": nb, "device": torch.cuda.get_device_name(0),
           "build": pkg.lib().ecckd_build_info().decode(), "results": res}
    if not existing_only:
        for n in ("sample_max_ran", "sample_exp_ran"):
            res[n]["mask_GBps"] = 8.0 * ncol * nlay / (res[n]["median_ms"] * 1e-3) / 1e9
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="sw:100000,lw_fsck:100000,lw_rrtmgp:100000,lw_fsck:1000000")
    ap.add_argument("--nlay", type=int, default=60)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=2, help="fresh processes per build and shape, alternating")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, help="(child mode) kind:ncol")
    ap.add_argument("--existing-only", action="store_true", help="(child mode) time the calls that exist on the parent alone")
    args = ap.parse_args()
    if args.child:
        kind, ncol = args.child.split(":")
        child(kind, int(ncol), args.nlay, args.repeats, args.existing_only)
        return

    def run(shape, lib, existing_only):
        env = dict(os.environ)
        env.pop("ECCKD_LIB", None)
        if lib:
            env["ECCKD_LIB"] = os.path.abspath(lib)
        cmd = [sys.executable, os.path.abspath(__file__), "--child", shape, "--nlay", str(args.nlay), "--repeats", str(args.repeats)]
        r = subprocess.run(cmd + (["--existing-only"] if existing_only else []), env=env, capture_output=True, text=True, timeout=900)
        if r.returncode != 0:   # (a failed child ends the job: nothing more is started on the GPU)
            raise SystemExit("child failed (%s): %s" % (shape, r.stderr[-2000:]))
        return json.loads(r.stdout.strip().splitlines()[-1])

    out = {"timing": "HIP events, 3 warm-up calls, variants interleaved; builds in alternating fresh processes", "repeats": args.repeats,
           "shapes": []}
    for shape in args.shapes.split(","):
        entry = {"shape": shape, "existing_calls": {"parent": [], "branch": []}}
        if args.parent_lib:
            for _ in range(args.rounds):
                for name, lib in (("parent", args.parent_lib), ("branch", None)):
                    entry["existing_calls"][name].append(run(shape, lib, True))
            overlap = {}
            for call in ("clear_fused", "allsky_fused", "increment_by_band"):
                if any(call not in c["results"] for b in ("parent", "branch") for c in entry["existing_calls"][b]):
                    continue
                lo = {b: min(c["results"][call]["min_ms"] for c in entry["existing_calls"][b]) for b in ("parent", "branch")}
                hi = {b: max(c["results"][call]["max_ms"] for c in entry["existing_calls"][b]) for b in ("parent", "branch")}
                overlap[call] = {"parent_ms": [lo["parent"], hi["parent"]], "branch_ms": [lo["branch"], hi["branch"]],
                                 "ranges_overlap": lo["parent"] <= hi["branch"] and lo["branch"] <= hi["parent"]}
            entry["existing_calls_min_max"] = overlap
        entry["mcica"] = run(shape, None, False)
        r = entry["mcica"]["results"]
        entry["masked_over_unmasked_fused"] = r["allsky_fused_masked"]["median_ms"] / r["allsky_fused"]["median_ms"]
        if "general_route_masked" in r:
            entry["general_route_over_masked_fused"] = r["general_route_masked"]["median_ms"] / r["allsky_fused_masked"]["median_ms"]
        out["shapes"].append(entry)
        print(json.dumps({k: v for k, v in entry.items() if k != "existing_calls"}), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
