#!/usr/bin/env python3
"""The rescaled longwave solver's clear-sky outputs and Jacobian next to what a host had to call without them (DESIGN section
5.5c), fp64, fast arithmetic mode.  Per shape kind:ncol:nlay (kind = lw_fsck | lw_rrtmgp), on this build, interleaved in one
process, on synthetic.columns / synthetic.clouds:
  both skies  ecckd_lw_fluxes_rescaled_jac with clear-sky outputs beside ecckd_lw_fluxes + ecckd_lw_fluxes_allsky_rescaled back
              to back (two gas-optics passes);
  Jacobian    the same call with flux_up_jac, "lw_jac_inline" = 1 and 0, beside the call without it and beside
              ecckd_lw_fluxes_allsky_rescaled run twice (what a finite difference costs); and with every output;
  solver      ecckd_rte_lw_rescaled_jac beside ecckd_rte_lw_rescaled on random arrays of the same size;
and, with --parent-lib,
  existing    ecckd_lw_fluxes, ecckd_lw_fluxes_allsky_rescaled, ecckd_lw_fluxes_jac and ecckd_rte_lw_rescaled on this build and
              on another build of the library (the parent commit's), in fresh child processes that alternate: their min-max
              ranges must overlap.
HIP-event timing: 3 warm-up calls, then --repeats timed calls per variant, the variants interleaved round-robin; median and
min-max.  Usage: python tools/bench_lw_rescaled_jac.py [--shapes lw_fsck:100000:60,...] [--parent-lib lib.so] [--out f.json]"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_allsky import interleaved, stats  # noqa: E402
from bench_mcica import DATA, FILES  # noqa: E402

DEFAULT_SHAPES = "lw_fsck:100000:60,lw_fsck:1000000:60,lw_fsck:100000:137"
EXISTING = ("existing:lw_fluxes", "existing:lw_fluxes_allsky_rescaled", "existing:lw_fluxes_jac", "existing:rte_lw_rescaled")


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

    k = pkg.GasOpticsEcckd()
    check(k.load(os.path.join(DATA, FILES[kind]), device=0))
    ng, nb = k.get_ngpt(), k.get_nband()
    cols = synthetic.columns(0, ncol, k.get_press_min(), nlay=nlay)
    cloud = synthetic.clouds(0, ncol, nlay, nb)
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
    two = pkg.OpticalProps2str()
    two.tau, two.ssa, two.g = t(cloud["tau"]), t(cloud["ssa"]), t(cloud["g"])
    empty = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)
    fl = pkg.FluxesBroadband(empty(nlay + 1, ncol), empty(nlay + 1, ncol))
    flc = pkg.FluxesBroadband(empty(nlay + 1, ncol), empty(nlay + 1, ncol))
    jac = empty(nlay + 1, ncol)
    atm = (plev, tlay, tsfc, tlev, gc, True, emis)

    # the solver alone, on random arrays of the same size
    op = pkg.OpticalProps2str()
    op.alloc_2str(ncol, nlay, k, like=plev)
    src = pkg.SourceFuncLW()
    src.alloc(ncol, nlay, k, like=plev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    rand = lambda: torch.rand(op.tau.shape, generator=gen, device=dev, dtype=torch.float64)
    op.tau.copy_(10.0 ** (rand() * 3.0 - 2.0))
    op.ssa.copy_(rand() * 0.999)
    op.g.copy_(rand() * 0.9)
    src.lev_source_dec.copy_(3.0 + rand())
    src.lev_source_inc.copy_(src.lev_source_dec * 1.01)
    src.lay_source.copy_(src.lev_source_dec * 1.005)
    src.sfc_source.fill_(4.0)
    src.sfc_source_jac.fill_(0.05)

    def rescaled_allsky():
        check(k.lw_fluxes_allsky(*atm, two, fl, rescaled=True))

    def with_inline(value, **kw):
        def call():
            pkg.set_solver_option("lw_jac_inline", value)
            check(k.lw_fluxes_rescaled(*atm, two, fl, **kw))
        return call

    variants, solvers = {}, {}
    variants["existing:lw_fluxes"] = lambda: check(k.lw_fluxes(*atm, flc))
    variants["existing:lw_fluxes_allsky_rescaled"] = rescaled_allsky
    variants["existing:lw_fluxes_jac"] = lambda: check(k.lw_fluxes(*atm, flc, flux_up_jac=jac))
    solvers["existing:rte_lw_rescaled"] = lambda: check(pkg.rte_lw(op, True, src, emis, fl, n_gauss_angles=1, rescaled=True))
    if not existing_only:
        solvers["solver:rte_lw_rescaled_jac"] = lambda: check(pkg.rte_lw_rescaled_jac(op, True, src, emis, fl, jac))

        def back_to_back():
            check(k.lw_fluxes(*atm, flc))
            rescaled_allsky()

        def twice():
            rescaled_allsky()
            rescaled_allsky()
        variants["parent:lw_fluxes_then_allsky_rescaled"] = back_to_back
        variants["parent:allsky_rescaled_twice"] = twice
        variants["new:lw_fluxes_rescaled"] = lambda: check(k.lw_fluxes_rescaled(*atm, two, fl))
        variants["new:both_skies"] = lambda: check(k.lw_fluxes_rescaled(*atm, two, fl, fluxes_clear=flc))
        variants["new:jac_inline1"] = with_inline(1, flux_up_jac=jac)
        variants["new:jac_inline0"] = with_inline(0, flux_up_jac=jac)
        variants["new:both_skies_jac_inline1"] = with_inline(1, fluxes_clear=flc, flux_up_jac=jac)
    default_inline = pkg.get_solver_option("lw_jac_inline") if not existing_only else None
    res = {n: stats(v) for n, v in interleaved(solvers, repeats).items()}
    res.update({n: stats(v) for n, v in interleaved(variants, repeats).items()})
    print(json.dumps({"kind": kind, "ncol": ncol, "nlay": nlay, "ngpt": ng, "nband": nb, "device": torch.cuda.get_device_name(0),
                      "build": pkg.lib().ecckd_build_info().decode(), "lw_jac_inline_default": default_inline, "results": res}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=DEFAULT_SHAPES)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=2, help="fresh processes per build and shape, alternating")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--parent-commit", default=None, help="recorded beside the parent's figures")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lw_rescaled_jac.json"))
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
        print("bench_lw_rescaled_jac: %s, %s" % (shape, "another build, existing calls" if lib else "this build"), file=sys.stderr, flush=True)
        r = subprocess.run(cmd + (["--existing-only"] if existing_only else []), env=env, capture_output=True, text=True, timeout=600)
        if r.returncode != 0:   # (a failed child ends the job: nothing more is started on the GPU)
            raise SystemExit("child failed (%s): %s" % (shape, r.stderr[-2000:]))
        return json.loads(r.stdout.strip().splitlines()[-1])

    out = {"timing": "HIP events, 3 warm-up calls, variants interleaved; builds in alternating fresh processes", "repeats": args.repeats,
           "parent_commit": args.parent_commit, "shapes": []}
    for shape in args.shapes.split(","):
        entry = {"shape": shape}
        if args.parent_lib:
            runs = {"parent": [], "branch": []}
            for _ in range(args.rounds):
                for name, lib in (("parent", args.parent_lib), ("branch", None)):
                    runs[name].append(run(shape, lib, True)["results"])
            overlap = {}
            for call in EXISTING:
                lo = {b: min(c[call]["min_ms"] for c in runs[b]) for b in runs}
                hi = {b: max(c[call]["max_ms"] for c in runs[b]) for b in runs}
                med = {b: sorted(c[call]["median_ms"] for c in runs[b])[len(runs[b]) // 2] for b in runs}
                overlap[call] = {"parent_ms": [lo["parent"], hi["parent"]], "branch_ms": [lo["branch"], hi["branch"]],
                                 "parent_median_ms": med["parent"], "branch_median_ms": med["branch"],
                                 "ranges_overlap": lo["parent"] <= hi["branch"] and lo["branch"] <= hi["parent"]}
            entry["existing_calls_min_max"] = overlap
        new = run(shape, None, False)
        entry.update({n: new[n] for n in ("kind", "ncol", "nlay", "ngpt", "device", "build", "lw_jac_inline_default")})
        r = new["results"]
        entry["results"] = r
        plain, both, pair = r["new:lw_fluxes_rescaled"], r["new:both_skies"], r["parent:lw_fluxes_then_allsky_rescaled"]
        j1, j0 = r["new:jac_inline1"], r["new:jac_inline0"]
        entry["ratios"] = {"both_skies_over_back_to_back": both["median_ms"] / pair["median_ms"],
                           "both_skies_saves_ms": pair["median_ms"] - both["median_ms"],
                           "both_skies_wholly_below_back_to_back": both["max_ms"] < pair["min_ms"],
                           "jac_inline1_over_plain": j1["median_ms"] / plain["median_ms"],
                           "jac_inline0_over_plain": j0["median_ms"] / plain["median_ms"],
                           "jac_inline1_wholly_below_inline0": j1["max_ms"] < j0["min_ms"],
                           "jac_inline1_over_allsky_twice": j1["median_ms"] / r["parent:allsky_rescaled_twice"]["median_ms"],
                           "rte_lw_rescaled_jac_over_rte_lw_rescaled":
                               r["solver:rte_lw_rescaled_jac"]["median_ms"] / r["existing:rte_lw_rescaled"]["median_ms"]}
        out["shapes"].append(entry)
        print(json.dumps({k: v for k, v in entry.items() if k != "results"}), flush=True)
        if args.out:   # (rewritten after every shape: a job cut short keeps what it measured)
            with open(args.out, "w") as f:
                f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
