"""Writes tests/golden/ref_<file>_<nlay>.npz: inputs and outputs of the reference's own gas-optics
module (src/gas_optics_ecckd.f90, built unmodified into oracle/_ref/libecckd_ref.so by
oracle.build_ref()) on a compact edge set of each model file, for the GPU suite
(tests/test_gpu_reference_fixtures.py), which must not need the reference tree.

Columns: helpers.branch_columns (one per branch group, plus synthetic ones) followed by four of
them stored bottom first (negative layer weights).  Gases: RFMIP order with no2, which the tables
do not know, and n2.  One set per file (the 36-g model at 30 layers, the others at 60) and eight
of the columns at 137 layers on the FSCK model, whose well-mixed gases are scalars
(helpers.WELL_MIXED: the product's merged-table path): 2.8 MB in all, as fp64 outputs hardly
compress.
Longwave sets hold tau, lay_source, sfc_source and the level sources as one (ng, nlay+1, ncol)
`lev_source` (lev_source_inc is its levels 1.., lev_source_dec its levels ..nlay-1: :423-424);
shortwave sets tau, ssa, g and toa_src.  helpers.load_ref_fixture reads them back.

    python tests/golden/make_golden_ref.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.dirname(HERE)]
import oracle  # noqa: E402
import helpers  # noqa: E402

FILES = {"lw_fsck": "ecckd-1.2_lw_ckd-definition_climate_fsck-tol0.0161.nc",
         "lw_rrtmgp": "ecckd-1.2_lw_ckd-definition_climate_rrtmgp-tol0.061.nc",
         "sw_wide": "ecckd-1.2_sw_ckd-definition_climate_wide-tol0.05.nc"}
BOTTOM_FIRST = ("synthetic0", "rel_lin_below_ref", "planck_above_350K", "zero_thickness")
DEEP = ("synthetic0", "p_above_110kPa", "t_below_grid", "planck_above_350K", "h2o_above_lut", "planck_at_350K",
        "zero_thickness", "synthetic0_bottom_first")
SETS = [("lw_fsck", 60, None), ("lw_rrtmgp", 30, None), ("sw_wide", 60, None), ("lw_fsck", 137, DEEP)]
N2 = 0.781
PROFILES = ("plev", "tlev", "tlay", "h2o", "o3")          # (nlev or nlay, ncol)
PER_COLUMN = ("tsfc", "co2", "ch4", "n2o", "cfc11", "cfc12")


def fixture_columns(m, nlay, subset=None):
    """Inputs of one set (the columns named in `subset`, or all of column_names()): every vmr a
    full (nlay, ncol) field or one value per column, but o2, no2 and n2 (scalars)."""
    top = helpers.branch_columns(m, nlay=nlay)
    bot = helpers.branch_columns(m, nlay=nlay, bottom_first=True)
    pick = [helpers.BRANCH_COLUMNS.index(n) for n in BOTTOM_FIRST]
    cols = {}
    for k in PROFILES:
        cols[k] = np.ascontiguousarray(np.concatenate([top[k], bot[k][:, pick]], axis=1))
    for k in PER_COLUMN:
        cols[k] = np.ascontiguousarray(np.concatenate([top[k], bot[k][pick]]))
    if subset is not None:
        keep = [column_names().index(n) for n in subset]
        for k in PROFILES:
            cols[k] = np.ascontiguousarray(cols[k][:, keep])
        for k in PER_COLUMN:
            cols[k] = np.ascontiguousarray(cols[k][keep])
    cols.update(o2=top["o2"], no2=top["no2"], n2=N2)
    return cols


def column_names(subset=None):
    return list(subset) if subset is not None else list(helpers.BRANCH_COLUMNS) + [n + "_bottom_first" for n in BOTTOM_FIRST]


def reference_outputs(m, cols):
    items = helpers.oracle_gas_items(cols, helpers.REF_FIXTURE_GASES)
    if m.shortwave:
        tau, ssa, g, toa, err = oracle.ref_gas_optics_ext(m, cols["plev"], cols["tlay"], items)
        assert err == ""
        return dict(tau=tau, ssa=ssa, g=g, toa_src=toa)
    tau, lay, inc, dec, sfc, err = oracle.ref_gas_optics_int(m, cols["plev"], cols["tlay"], cols["tsfc"], items,
                                                             cols["tlev"])
    assert err == ""
    lev = np.concatenate([dec[:, :1], inc], axis=1)
    assert np.array_equal(lev[:, :-1], dec)
    return dict(tau=tau, lay_source=lay, lev_source=lev, sfc_source=sfc)


def main():
    assert oracle.build_ref() or os.path.exists(oracle.REF_LIB), "needs the reference module (oracle.build_ref)"
    assert [(k, n) for k, n, _ in SETS] == list(helpers.REF_FIXTURE_SETS)
    total = 0
    for key, nlay, subset in SETS:
        m = oracle.CkdModel(os.path.join(ROOT, "data", FILES[key]))
        cols = fixture_columns(m, nlay, subset)
        if subset is not None:
            cols.update(helpers.WELL_MIXED)
        out = reference_outputs(m, cols)
        ins = {k: np.asarray(v, dtype=np.float64) for k, v in cols.items()}
        np.savez_compressed(helpers.ref_fixture_path(key, nlay), columns=np.array(column_names(subset)), **ins, **out)
        total += os.path.getsize(helpers.ref_fixture_path(key, nlay))
        print("wrote", os.path.basename(helpers.ref_fixture_path(key, nlay)), os.path.getsize(helpers.ref_fixture_path(key, nlay)), "bytes")
    print("total", total, "bytes")


if __name__ == "__main__":
    main()
