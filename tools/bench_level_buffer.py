#!/usr/bin/env python3
"""The longwave level sources as one buffer (include/ecckd_hip.h, "Level buffer") against the
parent commit's build, in fresh child processes that alternate: every round runs each point on the parent's library
(ECCKD_LIB) and on this build.  SourceFuncLW.alloc falls back to two separate arrays for a library without
ecckd_has_level_buffer, so the parent is measured as it is.  Points:
  lw_f64_1e6        python bench.py --steps 10 --warmup 2                 (the headline: the gain)
  lw_f64_1e5        ... --ncol 100000                                     (the gain at the small size)
  lw_36g_f64_1e6    ... --lut rrtmgp                                      (the 36-g table, Planck window)
  lw_ref_f64_1e6    ... --arithmetic reference                            (reference-order arithmetic: planck_kernel)
  lw_f32_1e6        ... --dtype f32                                       (unchanged path: must not lose)
  sw_f64_1e5        ... --mode sw --ncol 100000                           (unchanged path: must not lose)
  lw_fluxes_f64_1e6 ecckd_lw_fluxes on device arrays at 1e6 columns       (unchanged path: must not lose)
Per point and build: ms_per_step and the HIP-event times of the kernels named beside the point, every sample, min, max
and median.  The rule (decided per point): this build wins when its whole ms_per_step range lies below the parent's range
and its median is lower by more than twice the parent's own min-max spread of this run; it loses when the same holds the
other way round.
Usage: python tools/bench_level_buffer.py (--parent-lib lib.so | --parent-ref HEAD~1) [--rounds 3] [--points a,b]
       [--out profiles/level_buffer.json]
--parent-ref builds the library of that commit from `git archive` in a temporary directory (needs the repository's .git);
with --parent-lib, --parent-commit records which commit the library was built from."""
import argparse
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bench_gas_tile_sync as base   # noqa: E402  (child runner, statistics, the ecckd_lw_fluxes child)

BENCH = ["bench.py", "--steps", "10", "--warmup", "2"]
POINTS = (("lw_f64_1e6", BENCH, ("gas_lw_fused", "rte_lw")),
          ("lw_f64_1e5", BENCH + ["--ncol", "100000"], ("gas_lw_fused", "rte_lw")),
          ("lw_36g_f64_1e6", BENCH + ["--lut", "rrtmgp"], ("gas_lw_fused", "rte_lw")),
          ("lw_ref_f64_1e6", BENCH + ["--arithmetic", "reference"], ("planck", "rte_lw")),
          ("lw_f32_1e6", BENCH + ["--dtype", "f32"], ("gas_lw_fused_f32", "rte_lw")),
          ("sw_f64_1e5", BENCH + ["--mode", "sw", "--ncol", "100000"], ("tau",)),
          ("lw_fluxes_f64_1e6", None, ("tau",)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--parent-ref", default=None)
    ap.add_argument("--parent-commit", default=None, help="the commit --parent-lib was built from (recorded in the report)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--points", default=None, help="comma-separated subset of the points")
    ap.add_argument("--out", default=None)
    ap.add_argument("--fluxes-child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.fluxes_child is not None:
        return base.fluxes_child(None)
    tmp = None
    if not args.parent_lib:
        if not args.parent_ref:
            raise SystemExit("--parent-lib or --parent-ref is required")
        tmp = tempfile.TemporaryDirectory()
        args.parent_lib = base.build_parent(args.parent_ref, tmp.name)
        args.parent_commit = subprocess.run(["git", "rev-parse", args.parent_ref], capture_output=True, text=True, check=True,
                                            cwd=ROOT).stdout.strip()
    points = [p for p in POINTS if args.points is None or p[0] in args.points.split(",")]
    py = sys.executable
    variants = (("parent", args.parent_lib), ("this", None))
    rounds = max(args.rounds, 3)
    ms, kms = {}, {}
    for r in range(rounds):
        for point, cmd, kernels in points:
            for name, lib in variants:
                c = [py, os.path.abspath(__file__), "--fluxes-child", "none"] if cmd is None else [py] + cmd
                line = base.run(c, lib, 600)
                ms.setdefault(point, {}).setdefault(name, []).append(line["ms_per_step"])
                for kn in kernels:
                    kms.setdefault(point, {}).setdefault(name, {}).setdefault(kn, []).append(line["kernels"][kn]["avg_ms"])
                if args.out:   # (every sample so far: a run that is cut short still leaves its numbers)
                    with open(args.out + ".partial", "w") as f:
                        json.dump({"ms_per_step": ms, "kernel_ms": kms}, f)
                print("round %d %-18s %-7s %8.3f ms/step  %s" % (r, point, name, line["ms_per_step"], "  ".join(
                    "%s %7.3f ms" % (kn, line["kernels"][kn]["avg_ms"]) for kn in kernels)), flush=True)
    report = {"rounds": rounds, "parent_commit": args.parent_commit, "points": {}}
    for point, _, kernels in points:
        e = {n: dict({"ms_per_step": base.stats(ms[point][n])}, **{kn + "_ms": base.stats(kms[point][n][kn]) for kn in kernels})
             for n in ms[point]}
        par, s = e["parent"]["ms_per_step"], e["this"]["ms_per_step"]
        spread = par["max"] - par["min"]
        e["parent_spread_ms"] = spread
        e["this"]["overlaps_parent"] = s["min"] <= par["max"] and par["min"] <= s["max"]
        e["this"]["wins"] = s["max"] < par["min"] and par["median"] - s["median"] > 2 * spread
        e["this"]["loses"] = s["min"] > par["max"] and s["median"] - par["median"] > 2 * spread
        e["this"]["median_vs_parent"] = s["median"] / par["median"]
        report["points"][point] = e
        print(point, {n: (round(e[n]["ms_per_step"]["min"], 3), round(e[n]["ms_per_step"]["median"], 3),
                          round(e[n]["ms_per_step"]["max"], 3)) for n in ms[point]},
              "wins" if e["this"]["wins"] else "loses" if e["this"]["loses"] else "-", flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(report, f, indent=1)
        os.remove(args.out + ".partial")
    if tmp:
        tmp.cleanup()


if __name__ == "__main__":
    main()
