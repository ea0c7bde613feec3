#!/usr/bin/env python3
"""Solver option "gas_wave_roles" (gas_roles_kernel: tau waves and source waves share a block; DESIGN section 5.1, "Wave
roles") against the parent commit's build, in fresh child processes that alternate: every round runs each point on the
parent's library, on this build with the option at 0, with the option at 1 and as shipped (the option at its default, -1:
per shape).  Points:
  lw_f64_1e6         python bench.py --steps 10 --warmup 2                   (the headline)    kernel gas_lw_fused
  lw_f64_1e5         ... --ncol 100000                                                          kernel gas_lw_fused
  lw_36g_f64_1e6     ... --lut rrtmgp                      (chunks of 4 g-points, the Planck window)   kernel gas_lw_fused
  lw_slab32_f64_1e6  ... --solver-option gas_slab_f32=1    (the float32 image keeps its own kernel)    kernel gas_lw_fused
  lw_f32_1e6         ... --dtype f32                                         (must not move)   kernel gas_lw_fused_f32
  sw_f64_1e5         ... --mode sw --ncol 100000                             (must not move)   kernel tau
  lw_fluxes_f64_1e6  ecckd_lw_fluxes on device arrays at 1e6 columns: the tau-only mode (must not move)
Per point and variant: ms_per_step and the gas-optics HIP-event time (gas_lw_fused spans the edge kernel too), every
sample, min, max and median.  The rule (decided per point): a setting wins when its whole ms_per_step range lies below the
parent's range and its median is lower by more than twice the parent's own min-max spread of this run; it loses when the
same holds the other way round.  The option's default is 1 exactly for the shapes whose points win.
Usage: python tools/bench_gas_wave_roles.py (--parent-lib lib.so | --parent-ref HEAD~1) [--rounds 3] [--points a,b]
           [--variants parent,option_0,option_1,default] [--out profiles/gas_wave_roles.json]
--parent-ref builds the library of that commit from `git archive` in a temporary directory (needs the repository's .git).
--out: a file that exists already is extended by the points of this run (one job per group of points)."""
import argparse
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bench_gas_tile_sync as base   # noqa: E402  (child runner, statistics, the ecckd_lw_fluxes child)

OPTION = "gas_wave_roles"
BENCH = ["bench.py", "--steps", "10", "--warmup", "2"]
POINTS = (("lw_f64_1e6", BENCH, "gas_lw_fused"),
          ("lw_f64_1e5", BENCH + ["--ncol", "100000"], "gas_lw_fused"),
          ("lw_36g_f64_1e6", BENCH + ["--lut", "rrtmgp"], "gas_lw_fused"),
          ("lw_slab32_f64_1e6", BENCH + ["--solver-option", "gas_slab_f32=1"], "gas_lw_fused"),
          ("lw_f32_1e6", BENCH + ["--dtype", "f32"], "gas_lw_fused_f32"),
          ("sw_f64_1e5", BENCH + ["--mode", "sw", "--ncol", "100000"], "tau"),
          ("lw_fluxes_f64_1e6", None, "tau"))
VARIANTS = {"parent": None, "option_0": 0, "option_1": 1, "default": None}


def fluxes_child(option):
    if option is not None:
        sys.path.insert(0, ROOT)
        import rte_ecckd_amd as pkg
        pkg.set_solver_option(OPTION, option)
    base.fluxes_child(None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--parent-ref", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--points", default=None, help="comma-separated subset of the points")
    ap.add_argument("--variants", default="parent,option_0,option_1,default", help="comma-separated subset; parent is always run")
    ap.add_argument("--out", default=None)
    ap.add_argument("--fluxes-child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.fluxes_child is not None:
        return fluxes_child(None if args.fluxes_child == "none" else float(args.fluxes_child))
    tmp = None
    if not args.parent_lib:
        if not args.parent_ref:
            raise SystemExit("--parent-lib or --parent-ref is required")
        tmp = tempfile.TemporaryDirectory()
        args.parent_lib = base.build_parent(args.parent_ref, tmp.name)
    points = [p for p in POINTS if args.points is None or p[0] in args.points.split(",")]
    names = [n for n in VARIANTS if n == "parent" or n in args.variants.split(",")]
    py = sys.executable
    rounds = max(args.rounds, 3)
    ms, kms = {}, {}
    for r in range(rounds):
        for point, cmd, kernel in points:
            for name in names:
                lib, opt = (args.parent_lib if name == "parent" else None), VARIANTS[name]
                if cmd is None:
                    c = [py, os.path.abspath(__file__), "--fluxes-child", "none" if opt is None else str(opt)]
                else:
                    c = [py] + cmd + ([] if opt is None else ["--solver-option", "%s=%d" % (OPTION, opt)])
                line = base.run(c, lib, 600)
                ms.setdefault(point, {}).setdefault(name, []).append(line["ms_per_step"])
                kms.setdefault(point, {}).setdefault(name, []).append(line["kernels"][kernel]["avg_ms"])
                if args.out:   # (every sample so far: a run that is cut short still leaves its numbers)
                    with open(args.out + ".partial", "w") as f:
                        json.dump({"ms_per_step": ms, "kernel_ms": kms}, f)
                print("round %d %-18s %-9s %8.3f ms/step  %s %7.3f ms" % (r, point, name, line["ms_per_step"], kernel,
                                                                          line["kernels"][kernel]["avg_ms"]), flush=True)
    report = {"rounds": rounds, "option": OPTION, "points": {}}
    if args.out and os.path.exists(args.out):
        with open(args.out) as f:
            report["points"] = json.load(f).get("points", {})
    for point, _, kernel in points:
        e = {n: {"ms_per_step": base.stats(ms[point][n]), kernel + "_ms": base.stats(kms[point][n])} for n in ms[point]}
        par = e["parent"]["ms_per_step"]
        spread = par["max"] - par["min"]
        e["parent_spread_ms"] = spread
        for n in names[1:]:
            s = e[n]["ms_per_step"]
            e[n]["overlaps_parent"] = s["min"] <= par["max"] and par["min"] <= s["max"]
            e[n]["wins"] = s["max"] < par["min"] and par["median"] - s["median"] > 2 * spread
            e[n]["loses"] = s["min"] > par["max"] and s["median"] - par["median"] > 2 * spread
            e[n]["median_vs_parent"] = s["median"] / par["median"]
        report["points"][point] = e
        print(point, {n: (round(e[n]["ms_per_step"]["min"], 3), round(e[n]["ms_per_step"]["median"], 3), round(e[n]["ms_per_step"]["max"], 3))
                      for n in ms[point]}, {n: ("wins" if e[n]["wins"] else "loses" if e[n]["loses"] else "-") for n in names[1:]},
              flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(report, f, indent=1)
        os.remove(args.out + ".partial")
    if tmp:
        tmp.cleanup()


if __name__ == "__main__":
    main()
