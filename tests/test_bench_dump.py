"""bench.py --dump-outputs: what the timed path computed in its last step, written as .npy files that two builds can be
compared by.  Inputs come from the counter-based synthetic generator, so the same arguments give the same files."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import LW_FSCK, ROOT

pytestmark = pytest.mark.gpu

LW_NAMES = ("tau", "lay_source", "lev_source_inc", "lev_source_dec", "sfc_source", "flux_up", "flux_dn")
SW_NAMES = ("tau", "ssa", "g", "toa_src", "flux_up", "flux_dn")


def run_bench(out_dir, *extra):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
           "--cpu-seconds", "0", "--no-side", "--dump-outputs", str(out_dir)] + list(extra)
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, cwd=str(out_dir.parent), timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    files = sorted(os.listdir(str(out_dir)))
    assert all(f.endswith(".npy") for f in files), files
    return json.loads(lines[0]), {f[:-4]: np.load(str(out_dir / f)) for f in files}


def test_lw_dump_is_reproducible_and_matches_the_oracle(pkg, gpu, oracle_mod, tmp_path):
    import bench
    from rte_ecckd_amd import synthetic
    ncol = 2000                                   # above bench.DUMP_COLUMNS: the seeded column sample is exercised
    d1, a = run_bench(tmp_path / "a", "--ncol", str(ncol))
    d2, b = run_bench(tmp_path / "b", "--ncol", str(ncol))
    assert d1["steps"] == 2 and d1["ms_per_step"] > 0 and d2["ms_per_step"] > 0
    assert sorted(a) == sorted(LW_NAMES) and sorted(b) == sorted(LW_NAMES)
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    cols = bench.dump_columns(ncol)
    assert len(cols) == bench.DUMP_COLUMNS
    for n in LW_NAMES:
        assert a[n].dtype == np.float64 and a[n].shape[-1] == len(cols), n
        assert np.array_equal(a[n], b[n]), n     # same arguments, same inputs, same results

    m = oracle_mod.CkdModel(LW_FSCK)
    c = synthetic.columns(0, ncol, float(np.exp(m.log_pressure[0])))
    tau, lay, inc, dec, sfc, _ = oracle_mod.gas_optics_int(m, c["plev"], c["tlay"], c["tsfc"], synthetic.gas_items(c), c["tlev"])
    fu, fd = oracle_mod.rte_lw(tau, lay, inc, dec, np.repeat(c["sfc_emis"][None, :], tau.shape[0], 0), sfc)
    assert np.max(np.abs(a["tau"] - tau[..., cols]) / np.maximum(np.abs(tau[..., cols]), 1e-300)) < 1e-12
    assert np.array_equal(a["lay_source"], lay[..., cols])
    assert np.max(np.abs(a["flux_up"] - fu[:, cols])) < 1e-6
    assert np.max(np.abs(a["flux_dn"] - fd[:, cols])) < 1e-6


def test_sw_dump_small_run_keeps_every_column(pkg, gpu, tmp_path):
    d, a = run_bench(tmp_path / "sw", "--mode", "sw", "--ncol", "300")
    assert d["steps"] == 2 and d["ms_per_step"] > 0
    assert sorted(a) == sorted(SW_NAMES)
    for n in SW_NAMES:
        assert a[n].dtype == np.float64 and a[n].shape[-1] == 300 and np.all(np.isfinite(a[n])), n


@pytest.mark.parametrize("mode", ["lw", "sw"])
def test_plain_run_leaves_the_extras_to_full(pkg, gpu, tmp_path, mode):
    """Without --full a run times its steps and prints the line: no oracle spot check, no CPU baseline, no side
    measurement (the bench tests that read those pass --full)."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--mode", mode,
           "--ncol", "2000"]
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, cwd=str(tmp_path), timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["full"] is False and d["steps"] == 2 and d["ms_per_step"] > 0 and d["value"] > 0 and d["kernels"]
    assert d["check_max_abs_flux_diff_vs_oracle_Wm2"] is None and d["cpu_baseline"] is None
    extras = ("fused_sw",) if mode == "sw" else ("rte_lw_shared_levels", "lw_solver_variants", "well_mixed_scalars", "fused_lw",
                                                 "host_memspace", "fortran_device_resident")
    assert all(d[key] is None for key in extras), {key: d[key] for key in extras}
