#!/usr/bin/env python3
"""Times the multi-column solver against the single-column paths it can replace (DESIGN.md "Several right-hand sides in one
PCG pass").  One process, one GPU; every shape gets one warm-up and --reps timed repetitions, the two legs of a row alternating.
Wall times are taken around the Python call (which ends in a device synchronise), device times are pl_stats_t.ms_solve.

    python tools/time_solve_multi.py --out profiles/r08_solve_multi
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pylatticedso_amd import _capi                                     # noqa: E402
from pylatticedso_amd.homogenization_cell import HomogenizedCell       # noqa: E402
from pylatticedso_amd.lattice_sim import LatticeSim                    # noqa: E402
from pylatticedso_amd.utils_schur import node_order_to_simulate        # noqa: E402

E, NU = 1013.0, 0.3


def _cell(geoms, radii):
    return LatticeSim({"geometry": {"cell_size": {"x": 1, "y": 1, "z": 1}, "number_of_cells": {"x": 1, "y": 1, "z": 1},
                                    "radii": radii, "geom_types": geoms},
                       "simulation_parameters": {"enable": True, "material": "VeroClear", "periodicity": True}})


def _wall(fn):
    t0 = time.perf_counter()
    out = fn()
    return 1e3 * (time.perf_counter() - t0), out


def _summary(ms):
    return {"min_ms": min(ms), "max_ms": max(ms), "median_ms": float(np.median(ms)), "all_ms": ms}


def schur_row(reps):
    L = _cell(["Diamond", "Kelvin"], [0.03, 0.03])
    lat, pen = L.lattice, L.penalized
    order = node_order_to_simulate(L, 0)
    blocks = [None, 1, 2, 4, 8, 16, 32, 64]
    times = {b: [] for b in blocks}
    with _capi.HipLattice(lat.node_xyz, lat.beam_conn, lat.beam_radius, pen.seg_len, pen.seg_nsub, E, NU, reorder=0,
                          precond=5) as dev:
        dev.assemble()
        ref = dev.schur(order, rtol=1e-13, max_iter=200000)
        err = {}
        for b in blocks[1:]:
            err[b] = float(np.linalg.norm(dev.schur(order, rtol=1e-13, max_iter=200000, block=b) - ref) / np.linalg.norm(ref))
        for _ in range(reps):
            for b in blocks:
                times[b].append(_wall(lambda: dev.schur(order, rtol=1e-13, max_iter=200000, block=b))[0])
    base = _summary(times[None])
    rows = {str(b): dict(_summary(times[b]), rel_diff_to_pl_schur=err[b], wins=max(times[b]) < base["min_ms"],
                         speedup_median=base["median_ms"] / float(np.median(times[b]))) for b in blocks[1:]}
    return {"what": "Diamond + Kelvin Schur complement (38 boundary nodes, 228 columns), rtol 1e-13, precond = 5 handle",
            "pl_schur": base, "pl_schur_block": rows}


def homogenisation_row(reps):
    out = {False: [], True: []}
    H = {}
    for rep in range(reps + 1):
        for batched in (False, True):
            L = _cell(["Octet"], [0.04])
            a = HomogenizedCell(L, batched=batched)
            a.prepare_simulation()
            a.apply_dirichlet_for_homogenization()
            a.periodic_boundary_condition()
            ms, H[batched] = _wall(a.solve_full_homogenization)
            if rep:
                out[batched].append(ms)
            L._device.close()
    base, bat = _summary(out[False]), _summary(out[True])
    return {"what": "six-case homogenisation of an Octet cell (solve_full_homogenization, wall)", "batched_false": base,
            "batched_true": dict(bat, wins=bat["max_ms"] < base["min_ms"], speedup_median=base["median_ms"] / bat["median_ms"],
                                 rel_diff=float(np.linalg.norm(H[True] - H[False]) / np.linalg.norm(H[False])))}


def iteration_row(reps, iters=200):
    """Device time of one PCG iteration with k columns: a solve cut off after `iters` iterations, ms_solve / iters."""
    L = LatticeSim({"geometry": {"cell_size": {"x": 1, "y": 1, "z": 1}, "number_of_cells": {"x": 3, "y": 2, "z": 2},
                                 "radii": [0.05, 0.04, 0.03], "geom_types": ["BCC", "Hybrid1", "Hybrid4"]},
                    "simulation_parameters": {"enable": True, "material": "VeroClear", "periodicity": False},
                    "boundary_conditions": {
                        "Displacement": {"Fixed": {"Surface": ["Xmin"], "DOF": ["X", "Y", "Z", "RX", "RY", "RZ"],
                                                   "Value": [0, 0, 0, 0, 0, 0]}},
                        "Force": {"Load": {"Surface": ["Xmax"], "DOF": ["Z"], "Value": [-0.1]}}}})
    lat, pen = L.lattice, L.penalized
    rng = np.random.default_rng(0)
    res = {}
    with _capi.HipLattice(lat.node_xyz, lat.beam_conn, lat.beam_radius, pen.seg_len, pen.seg_nsub, E, NU, precond=1) as dev:
        dev.set_bc(L.fixed_DOF)
        dev.assemble()
        res["single_iteration_us_pl_time_kernel_3"] = [1e3 * dev.time_kernel(3, 200) for _ in range(reps)]
        for k in (1, 2, 4, 8, 16, 32, 64):
            f = np.where(L.fixed_DOF, 0.0, rng.standard_normal((k,) + L.fixed_DOF.shape))
            us = []
            for rep in range(reps + 1):
                _, st = dev.solve_multi(None, f, rtol=1e-30, max_iter=iters, raise_on_noconv=False)
                if rep:
                    us.append(1e3 * st[0]["ms_solve"] / iters)
            res[f"k={k}"] = {"iteration_us": us, "per_column_us": [u / k for u in us]}
    return {"what": f"one Jacobi-PCG iteration with k columns, 3 x 2 x 2 BCC + Hybrid1 + Hybrid4 ({lat.n_nodes} nodes), "
                    f"ms_solve / {iters} iterations (includes the status look every 16 iterations)", "rows": res}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/r08_solve_multi")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    res = {"schur": schur_row(a.reps), "homogenisation": homogenisation_row(a.reps), "iteration": iteration_row(a.reps)}
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out + ".json", "w") as fh:
        json.dump(res, fh, indent=1)
    lines = [res["schur"]["what"], f"  pl_schur             min {res['schur']['pl_schur']['min_ms']:9.2f}  median "
             f"{res['schur']['pl_schur']['median_ms']:9.2f}  max {res['schur']['pl_schur']['max_ms']:9.2f} ms"]
    for b, r in res["schur"]["pl_schur_block"].items():
        lines.append(f"  pl_schur_block b={b:>2}  min {r['min_ms']:9.2f}  median {r['median_ms']:9.2f}  max {r['max_ms']:9.2f} ms  "
                     f"x{r['speedup_median']:.1f}  wins={r['wins']}  diff {r['rel_diff_to_pl_schur']:.1e}")
    h = res["homogenisation"]
    lines += [h["what"]] + [f"  batched={k[8:]:5}  min {h[k]['min_ms']:9.2f}  median {h[k]['median_ms']:9.2f}  max {h[k]['max_ms']:9.2f} ms"
                            for k in ("batched_false", "batched_true")]
    lines.append(f"  wins={h['batched_true']['wins']}  x{h['batched_true']['speedup_median']:.2f}  diff {h['batched_true']['rel_diff']:.1e}")
    it = res["iteration"]
    lines += [it["what"], f"  single column (pl_time_kernel 3): {np.median(it['rows']['single_iteration_us_pl_time_kernel_3']):.1f} us"]
    for k, r in it["rows"].items():
        if k.startswith("k="):
            lines.append(f"  {k:>5}: {np.median(r['iteration_us']):8.1f} us per iteration, {np.median(r['per_column_us']):7.2f} us per column")
    with open(a.out + ".txt", "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
