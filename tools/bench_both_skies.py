#!/usr/bin/env python3
"""Clear-sky + all-sky fluxes from one call (ecckd_*_fluxes_clear_allsky), fp64, synthetic.clouds /
synthetic.cloud_fraction.  Per shape kind:ncol:nlay (kind = sw | lw_fsck | lw_rrtmgp) and per configuration -- two-stream
or (longwave) one-stream particles, with and without a cloud mask -- on this build, interleaved in one process:
  (a) the two existing calls back to back: *_fluxes, then *_fluxes_allsky(cloud_mask=);
  (b) the new call with "lw_both_skies" = 0 (two solver launches behind one gas-optics pass);
  (c) longwave at 60 layers: the new call with "lw_both_skies" = 1 (the dual-sky kernel);
and, with --parent-lib,
  (d) each existing fused call (clear, all-sky, all-sky masked) on this build and on another build of the library (the
      parent commit's), in fresh child processes that alternate: their min-max ranges must overlap.
The decision rule for the default of "lw_both_skies" is evaluated per configuration over the 60-layer longwave shapes: 1
only if the min-max range of (c) lies wholly below that of (b) at every one of them.
HIP-event timing: 3 warm-up calls, then --repeats timed calls per variant, the variants interleaved round-robin; median
and min-max.  Usage: python tools/bench_both_skies.py [--shapes lw_fsck:100000:60,...] [--parent-lib lib.so] [--out f.json]"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_allsky import interleaved, stats  # noqa: E402
from bench_mcica import DATA, FILES, SW_NAMES  # noqa: E402

DEFAULT_SHAPES = "lw_fsck:100000:60,lw_fsck:1000000:60,lw_rrtmgp:100000:60,lw_fsck:100000:137,sw:100000:60"


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
    two = pkg.OpticalProps2str()
    two.tau, two.ssa, two.g = t(cloud["tau"]), t(cloud["ssa"]), t(cloud["g"])
    one = pkg.OpticalProps1scl()
    one.tau = two.tau
    empty = lambda: torch.empty((nlay + 1, ncol), dtype=torch.float64, device=dev)
    fl = pkg.FluxesBroadband(*(empty() for _ in range(3 if sw else 2)))
    fc = pkg.FluxesBroadband(*(empty() for _ in range(3 if sw else 2)))
    mask = pkg.sample_cloud_mask(t(synthetic.cloud_fraction(0, ncol, nlay)), ng, seed=1)
    if sw:
        rng = np.random.default_rng(nlay)
        mu0, ad, af = t(cols["mu0"]), t(rng.uniform(0.02, 0.6, (ncol, nb))), t(rng.uniform(0.02, 0.6, (ncol, nb)))
        clear = lambda: check(k.sw_fluxes(plev, tlay, gc, True, mu0, ad, af, fc))
        allsky = lambda part, m: check(k.sw_fluxes_allsky(plev, tlay, gc, True, mu0, ad, af, part, fl, delta_scale=True, cloud_mask=m))
        both = lambda part, m: check(k.sw_fluxes_clear_allsky(plev, tlay, gc, True, mu0, ad, af, part, fl, fc, delta_scale=True,
                                                              cloud_mask=m))
    else:
        tsfc, tlev = t(cols["tsfc"]), t(cols["tlev"])
        emis = t(np.repeat(cols["sfc_emis"][:, None], nb, 1))
        clear = lambda: check(k.lw_fluxes(plev, tlay, tsfc, tlev, gc, True, emis, fc))
        allsky = lambda part, m: check(k.lw_fluxes_allsky(plev, tlay, tsfc, tlev, gc, True, emis, part, fl, cloud_mask=m))
        both = lambda part, m: check(k.lw_fluxes_clear_allsky(plev, tlay, tsfc, tlev, gc, True, emis, part, fl, fc, cloud_mask=m))

    configs = [("two_stream", two, None), ("two_stream_masked", two, mask)]
    if not sw:
        configs += [("one_stream", one, None), ("one_stream_masked", one, mask)]
    variants = {}
    if existing_only:
        variants["clear_fused"] = clear
        variants["allsky_fused"] = lambda: allsky(two, None)
        variants["allsky_fused_masked"] = lambda: allsky(two, mask)
    else:
        def form(v, fn):
            def run():
                pkg.set_solver_option("lw_both_skies", v)
                fn()
            return run

        for name, part, m in configs:
            def a(part=part, m=m):
                clear()
                allsky(part, m)
            variants[name + ":a_two_calls"] = a
            variants[name + ":b_one_call_two_launches"] = form(0, lambda part=part, m=m: both(part, m))
            if not sw and nlay == 60:
                variants[name + ":c_one_call_dual_sky_kernel"] = form(1, lambda part=part, m=m: both(part, m))
    res = {n: stats(v) for n, v in interleaved(variants, repeats).items()}
    print(json.dumps({"kind": kind, "ncol": ncol, "nlay": nlay, "ngpt": ng, "nband": nb, "device": torch.cuda.get_device_name(0),
                      "build": pkg.lib().ecckd_build_info().decode(), "results": res}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=DEFAULT_SHAPES)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=2, help="fresh processes per build and shape, alternating")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, help="(child mode) kind:ncol:nlay")
    ap.add_argument("--existing-only", action="store_true", help="(child mode) time the calls that exist on the parent alone")
    args = ap.parse_args()
    if args.child:
        kind, ncol, nlay = args.child.split(":")
        child(kind, int(ncol), int(nlay), args.repeats, args.existing_only)
        return

    def run(shape, lib, existing_only):
        env = dict(os.environ)
        env.pop("ECCKD_LIB", None)
        if lib:
            env["ECCKD_LIB"] = os.path.abspath(lib)
        cmd = [sys.executable, os.path.abspath(__file__), "--child", shape, "--repeats", str(args.repeats)]
        r = subprocess.run(cmd + (["--existing-only"] if existing_only else []), env=env, capture_output=True, text=True, timeout=600)
        if r.returncode != 0:   # (a failed child ends the job: nothing more is started on the GPU)
            raise SystemExit("child failed (%s): %s" % (shape, r.stderr[-2000:]))
        return json.loads(r.stdout.strip().splitlines()[-1])

    out = {"timing": "HIP events, 3 warm-up calls, variants interleaved; builds in alternating fresh processes", "repeats": args.repeats,
           "shapes": []}
    below = {}   # configuration -> [range of (c) wholly below range of (b), per 60-layer longwave shape]
    for shape in args.shapes.split(","):
        entry = {"shape": shape}
        if args.parent_lib:
            runs = {"parent": [], "branch": []}
            for _ in range(args.rounds):
                for name, lib in (("parent", args.parent_lib), ("branch", None)):
                    runs[name].append(run(shape, lib, True)["results"])
            overlap = {}
            for call in ("clear_fused", "allsky_fused", "allsky_fused_masked"):
                lo = {b: min(c[call]["min_ms"] for c in runs[b]) for b in runs}
                hi = {b: max(c[call]["max_ms"] for c in runs[b]) for b in runs}
                med = {b: sorted(c[call]["median_ms"] for c in runs[b])[len(runs[b]) // 2] for b in runs}
                overlap[call] = {"parent_ms": [lo["parent"], hi["parent"]], "branch_ms": [lo["branch"], hi["branch"]],
                                 "parent_median_ms": med["parent"], "branch_median_ms": med["branch"],
                                 "ranges_overlap": lo["parent"] <= hi["branch"] and lo["branch"] <= hi["parent"]}
            entry["d_existing_calls_min_max"] = overlap
        new = run(shape, None, False)
        entry.update({n: new[n] for n in ("kind", "ncol", "nlay", "ngpt", "device", "build")})
        r = new["results"]
        entry["results"] = r
        ratios = {}
        for cfg in sorted({n.split(":")[0] for n in r}):
            a, b = r[cfg + ":a_two_calls"], r[cfg + ":b_one_call_two_launches"]
            ratios[cfg] = {"a_over_b": a["median_ms"] / b["median_ms"],
                           "a_over_b_range": [a["min_ms"] / b["max_ms"], a["max_ms"] / b["min_ms"]]}
            c = r.get(cfg + ":c_one_call_dual_sky_kernel")
            if c:
                ratios[cfg].update({"a_over_c": a["median_ms"] / c["median_ms"],
                                    "a_over_c_range": [a["min_ms"] / c["max_ms"], a["max_ms"] / c["min_ms"]],
                                    "c_wholly_below_b": c["max_ms"] < b["min_ms"]})
                below.setdefault(cfg, []).append(c["max_ms"] < b["min_ms"])
        entry["ratios"] = ratios
        out["shapes"].append(entry)
        print(json.dumps({k: v for k, v in entry.items() if k != "results"}), flush=True)
    out["lw_both_skies_default_by_rule"] = {cfg: int(all(v)) for cfg, v in below.items()}
    print(json.dumps({"lw_both_skies_default_by_rule": out["lw_both_skies_default_by_rule"]}), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
