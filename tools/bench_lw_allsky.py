#!/usr/bin/env python3
"""All-sky longwave timings at 60 layers, fp64, synthetic.clouds, on the 32-g / 1-band file at 1e6
and 1e5 columns and on the 36-g / 16-band file (the only one where the band of a lane changes inside a tile) at 1e5:
  (a)  clear-sky ecckd_lw_fluxes -- on this build and, with --parent-lib, on another build of the library (the parent
       commit's), each in fresh child processes that alternate, so the two are compared on the same box;
  (b)  the unfused all-sky composition gas_optics + increment (1scl += band 2str) + rte_lw, default solver options;
  (b') gas_optics_tau + increment + rte_lw_fused (the composition the fused call equals bit for bit; 32-g file);
  (c)  the fused lw_fluxes_allsky with two-stream particles;
  (c1) the fused lw_fluxes_allsky with one-stream particles (32-g file).
HIP-event timing: 3 warm-up calls, then `--repeats` (default 30) timed calls per variant, the variants interleaved
round-robin; median and min-max spread.
Usage: python tools/bench_lw_allsky.py [--sizes 1000000,100000] [--parent-lib lib.so] [--out file.json]"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILES = {"fsck_32g_1band": os.path.join(ROOT, "data", "ecckd-1.2_lw_ckd-definition_climate_fsck-tol0.0161.nc"),
         "rrtmgp_36g_16band": os.path.join(ROOT, "data", "ecckd-1.2_lw_ckd-definition_climate_rrtmgp-tol0.061.nc")}
NLAY = 60


def stats(ms):
    ms = sorted(ms)
    return {"median_ms": ms[len(ms) // 2], "min_ms": ms[0], "max_ms": ms[-1], "n": len(ms)}


def interleaved(variants, repeats):
    """{name: [ms]}: every variant warmed up three times, then timed `repeats` times round-robin with HIP events."""
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
    return out


def check(msg):
    if msg:
        raise SystemExit(msg)


def below(x, y):
    """x's min-max range lies wholly below y's."""
    return x["max_ms"] < y["min_ms"]


def workload(pkg, which, ncol, clear_only=False):
    """The variants of one (file, column count) as {name: callable}, plus its shape; clear_only: (a) alone (the parent's
    library has no all-sky call)."""
    import torch
    from rte_ecckd_amd import synthetic
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    k = pkg.GasOpticsEcckd()
    check(k.load(FILES[which], device=0))
    ng, nb = k.get_ngpt(), k.get_nband()
    cols = synthetic.columns(0, ncol, k.get_press_min(), nlay=NLAY)
    cloud = synthetic.clouds(0, ncol, NLAY, nb)
    gc = pkg.GasConcs(synthetic.GAS_ORDER)
    for n in synthetic.GAS_ORDER:
        v = cols[n]
        if np.isscalar(v):
            gc.set_vmr(n, float(v))
        elif v.ndim == 1:
            gc.set_vmr_column(n, t(v))
        else:
            gc.set_vmr(n, t(v))
    plev, tlay, tlev, tsfc = t(cols["plev"]), t(cols["tlay"]), t(cols["tlev"]), t(cols["tsfc"])
    emis = t(np.repeat(cols["sfc_emis"][:, None], nb, 1))
    fl = pkg.FluxesBroadband(*(torch.empty((NLAY + 1, ncol), dtype=torch.float64, device=dev) for _ in range(2)))
    clear = lambda: check(k.lw_fluxes(plev, tlay, tsfc, tlev, gc, True, emis, fl))
    if clear_only:
        return k, {"a_clear_lw_fluxes": clear}, (ng, nb)
    b2g = k.get_band2gpt()
    two = pkg.OpticalProps2str(); two.alloc_2str_bands(ncol, NLAY, k, like=plev)
    two.tau.copy_(t(cloud["tau"])); two.ssa.copy_(t(cloud["ssa"])); two.g.copy_(t(cloud["g"]))
    one = pkg.OpticalProps1scl(); one.alloc_1scl_bands(ncol, NLAY, k, like=plev)
    one.tau.copy_(two.tau)
    op = pkg.OpticalProps1scl(); op.alloc_1scl(ncol, NLAY, k, like=plev)
    src = pkg.SourceFuncLW(); src.alloc(ncol, NLAY, k, like=plev)

    def unfused():
        check(k.gas_optics(None, plev, tlay, tsfc, gc, op, src, tlev=tlev))
        check(op.increment(two, band2gpt=b2g))
        check(pkg.rte_lw(op, True, src, emis, fl))

    def unfused_tau():
        check(k.gas_optics_tau(plev, tlay, gc, op))
        check(op.increment(two, band2gpt=b2g))
        check(k.rte_lw_fused(op, True, tlay, tlev, tsfc, emis, fl))

    variants = {"a_clear_lw_fluxes": clear, "b_unfused_gas_optics_increment_rte_lw": unfused,
                "b1_gas_optics_tau_increment_rte_lw_fused": unfused_tau,
                "c_fused_allsky_two_stream": lambda: check(k.lw_fluxes_allsky(plev, tlay, tsfc, tlev, gc, True, emis, two, fl)),
                "c1_fused_allsky_one_stream": lambda: check(k.lw_fluxes_allsky(plev, tlay, tsfc, tlev, gc, True, emis, one, fl))}
    if nb > 1:   # the 36-g file: (a), (b), (c)
        del variants["b1_gas_optics_tau_increment_rte_lw_fused"], variants["c1_fused_allsky_one_stream"]
    return k, variants, (ng, nb)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1000000,100000", help="column counts of the 32-g file")
    ap.add_argument("--ncol-36g", type=int, default=100000)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--clear-only", type=int, default=0, help="(child mode) time ecckd_lw_fluxes alone at this column count, print one JSON line")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sizes = [int(s) for s in args.sizes.split(",") if s]

    clear_children = None
    if args.parent_lib and not args.clear_only:   # fresh processes, alternating, before this one opens the GPU
        clear_children = {"ncol": sizes[0], "parent": [], "branch": []}
        for _ in range(2):
            for name, lib in (("parent", args.parent_lib), ("branch", None)):
                env = dict(os.environ)
                if lib:
                    env["ECCKD_LIB"] = os.path.abspath(lib)
                else:
                    env.pop("ECCKD_LIB", None)
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--clear-only", str(sizes[0]), "--repeats", str(args.repeats)],
                                   env=env, capture_output=True, text=True, timeout=400)
                if r.returncode != 0:
                    raise SystemExit("child failed: " + r.stderr[-2000:])
                clear_children[name].append(json.loads(r.stdout.strip().splitlines()[-1]))

    import torch
    sys.path.insert(0, ROOT)
    import rte_ecckd_amd as pkg

    if args.clear_only:
        _, variants, _ = workload(pkg, "fsck_32g_1band", args.clear_only, clear_only=True)
        print(json.dumps(stats(interleaved({"clear": variants["a_clear_lw_fluxes"]}, args.repeats)["clear"])))
        return

    cases = []
    for which, ncol in [("fsck_32g_1band", n) for n in sizes] + [("rrtmgp_36g_16band", args.ncol_36g)]:
        k, variants, (ng, nb) = workload(pkg, which, ncol)
        res = {n: stats(v) for n, v in interleaved(variants, args.repeats).items()}
        a, b, c = res["a_clear_lw_fluxes"], res["b_unfused_gas_optics_increment_rte_lw"], res["c_fused_allsky_two_stream"]
        entry = {"file": which, "ncol": ncol, "nlay": NLAY, "ngpt": ng, "nband": nb, "results": res,
                 "unfused_over_fused": b["median_ms"] / c["median_ms"], "fused_range_below_unfused": below(c, b),
                 "cost_of_clouds_fused_over_clear": c["median_ms"] / a["median_ms"],
                 # whole-call figure, not a kernel's share of peak: tau written and read once (16 B per cell) plus the two band
                 # planes if every band value comes from HBM once and from L2 for the other g-points of its band
                 "fused_call_bytes_per_cell": 16.0 + 16.0 * nb / ng}
        if "b1_gas_optics_tau_increment_rte_lw_fused" in res:
            b1 = res["b1_gas_optics_tau_increment_rte_lw_fused"]
            entry["tau_composition_over_fused"] = b1["median_ms"] / c["median_ms"]
            entry["fused_range_below_tau_composition"] = below(c, b1)
        cases.append(entry)
        del k, variants
        pkg.release_scratch(0)
        torch.cuda.empty_cache()
    out = {"device": torch.cuda.get_device_name(0), "build": pkg.lib().ecckd_build_info().decode(), "dtype": "f64",
           "repeats": args.repeats, "timing": "HIP events, 3 warm-up calls, variants interleaved", "cases": cases,
           "clear_lw_fluxes_fresh_processes": clear_children}
    if clear_children:
        par = sorted(x for r in clear_children["parent"] for x in (r["min_ms"], r["max_ms"]))
        med = lambda rs: sorted(r["median_ms"] for r in rs)[len(rs) // 2]
        out["clear_sky_unchanged"] = {"parent_median_ms": med(clear_children["parent"]), "branch_median_ms": med(clear_children["branch"]),
                                      "parent_min_ms": par[0], "parent_max_ms": par[-1],
                                      "branch_median_within_parent_spread": par[0] <= med(clear_children["branch"]) <= par[-1]}
    line = json.dumps(out, indent=1)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
