#!/usr/bin/env python3
"""Times the conduction gather (pl_cond_spmv) on the 50^3 Octet lattice of bench.py beside its yardstick,
k_thermal_load of pl_thermal_load in the same run: both walk the same sliced-ELL incidence, one thread per node.  Then one
pl_cond_solve between a hot and a cold face.  One process, one GPU; one warm-up and --reps timed repetitions per row.  Kernel
times are HIP events around the launches of one call (the library prints them when PL_TIMING is set; the last line of a call is
the stage that ends it - for pl_cond_solve the whole PCG with its status downloads).  The rows under convection (DESIGN.md
section 10m) follow in the same process, after the plain ones: the convective gather beside the plain gather of the same run,
pl_cond_film (k_cond_film and its fold), the temperature p-norm pass and one pl_cond_solve with convection.
Last, the transient (pl_cond_transient): --steps backward-Euler steps between the hot and the cold face,
without and with the film, with the iterations per step, the device time per step and per iteration, k_heat_begin and k_heat_end
of the last step beside one plain k_cond_gather of the same run, and the host synchronisations per step; they go to
<out>_transient.json / .txt (--only-transient skips the rows above).

    python tools/time_conduction.py --out profiles/r20_heat                     (r19_convection: the record of section 10m)
    python tools/time_conduction.py --out profiles/r20_heat --only-transient
"""
import argparse
import json
import os
import re
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
os.environ["PL_TIMING"] = "1"

from time_stress import _summary, _timed                               # noqa: E402
from pylatticedso_amd.lattice_sim import LatticeSim                    # noqa: E402


def _captured(fn):
    """(wall ms, the library's PL_TIMING lines of the call as {label: value}, result)."""
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile(mode="w+b") as tmp:
        os.dup2(tmp.fileno(), 2)
        try:
            t0 = time.perf_counter()
            out = fn()
            wall = 1e3 * (time.perf_counter() - t0)
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        tmp.seek(0)
        text = tmp.read().decode(errors="replace")
    return wall, {m[0]: float(m[1]) for m in re.findall(r"\[pl_cond_transient\]\s+(\S+)\s+([0-9.]+)", text)}, out


def transient_rows(a, dev, fixed, t_bar, T):
    """The transient with and without the film on the handle's lattice: medians and spreads of a.reps warm repetitions."""
    res = {"steps": a.steps, "dt": a.dt, "rho_c": a.rho_c, "rtol": a.rtol, "theta": 1.0, "reps": a.reps, "cases": {}}
    for name, film in (("no film", None), (f"film {a.film:g}", a.film)):
        dev.set_conduction(0.2)
        if film is not None:
            dev.set_convection(film, a.ambient)
        dev.set_heat_capacity(a.rho_c)
        t0 = np.full(dev.n_nodes, a.ambient)
        keep = {}
        for rep in range(a.reps + 1):
            wall, lines, out = _captured(lambda: dev.cond_transient(a.dt, a.steps, 1.0, fixed, t_bar, t0=t0, rtol=a.rtol,
                                                                    max_iter=200000))
            _, gather, _ = _timed(lambda: dev.cond_spmv(T))
            if rep:
                its = int(out["iters"].sum())
                row = {"wall_ms": wall, "time_loop_ms": lines["time_loop_hip_event"], "refresh_ms": lines["refresh_hip_event"],
                       "device_ms_per_step": lines["time_loop_hip_event"] / a.steps,
                       "device_ms_per_iteration": lines["time_loop_hip_event"] / max(its, 1),
                       "k_heat_begin_ms": lines["k_heat_begin_last_step"], "k_heat_end_ms": lines["k_heat_end_last_step"],
                       "k_cond_gather_ms": gather, "host_syncs_per_step": lines["host_syncs_per_step"],
                       "iterations_per_step": its / a.steps}
                for k, v in row.items():
                    keep.setdefault(k, []).append(v)
        res["cases"][name] = {k: _summary(v) for k, v in keep.items()}
        res["cases"][name]["iterations_of_every_step"] = out["iters"].tolist()
    return res


def transient_report(a, res, head):
    lines = [f"{head}; pl_cond_transient, {res['steps']} backward-Euler steps of dt {res['dt']:g}, rho_c {res['rho_c']:g}, "
             f"rtol {res['rtol']:g}, hot Zmin and cold Zmax from the ambient; medians [min, max] of {a.reps} warm repetitions"]
    for name, c in res["cases"].items():
        lines.append(f"  {name}:")
        for k, r in c.items():
            if isinstance(r, dict):
                lines.append(f"    {k:28} {r['median_ms']:10.4f}   [{r['min_ms']:.4f}, {r['max_ms']:.4f}]")
        lines.append(f"    iterations of every step     {c['iterations_of_every_step']}")
    with open(a.out + "_transient.json", "w") as fh:
        json.dump(res, fh, indent=1)
    with open(a.out + "_transient.txt", "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--dt", type=float, default=0.5)
    ap.add_argument("--rho-c", dest="rho_c", type=float, default=2.0)
    ap.add_argument("--only-transient", action="store_true")
    ap.add_argument("--out", default="profiles/r20_heat")
    ap.add_argument("--film", type=float, default=0.05)
    ap.add_argument("--ambient", type=float, default=20.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cells", type=int, default=50)
    ap.add_argument("--geom", default="Octet")
    ap.add_argument("--rtol", type=float, default=1e-8)
    a = ap.parse_args()
    n = a.cells
    L = LatticeSim({"geometry": {"cell_size": {"x": 1, "y": 1, "z": 1}, "number_of_cells": {"x": n, "y": n, "z": n},
                                 "radii": [0.05], "geom_types": [a.geom]},
                    "simulation_parameters": {"enable": True, "material": "VeroClear", "periodicity": False},
                    "boundary_conditions": {
                        "Displacement": {"Fixed": {"Surface": ["Xmin"], "DOF": ["X", "Y", "Z", "RX", "RY", "RZ"],
                                                   "Value": [0, 0, 0, 0, 0, 0]}},
                        "Force": {"Load": {"Surface": ["Xmax"], "DOF": ["Z"], "Value": [-0.1]}}}})
    lat = L.lattice
    dev = L.device_model()
    dev.set_bc(L.fixed_DOF)
    dev.assemble()
    rng = np.random.default_rng(0)
    T = 20.0 + 60.0 * rng.random(lat.n_nodes)
    mu = rng.standard_normal(lat.n_nodes)
    lam = np.ascontiguousarray((rng.standard_normal((lat.n_nodes, 6)) * 1e-3).ravel())
    fixed = np.zeros(lat.n_nodes, bool)
    hot, cold = L.find_point_on_lattice_surface(["Zmin"]), L.find_point_on_lattice_surface(["Zmax"])
    fixed[hot] = fixed[cold] = True
    t_bar = np.zeros(lat.n_nodes)
    t_bar[hot], t_bar[cold] = 90.0, 20.0
    dev.set_conduction(0.2)
    dev.set_thermal(7e-5, 40.0 + 10.0 * (2.0 * rng.random(lat.n_nodes) - 1.0))
    res = {"lattice": f"{n}^3 {a.geom}", "n_nodes": int(lat.n_nodes), "n_beams": int(lat.n_beams), "reps": a.reps,
           "rtol": a.rtol, "rows": {}}
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    head = f"{res['lattice']}: {res['n_nodes']} nodes, {res['n_beams']} struts"
    if a.only_transient:
        transient_report(a, transient_rows(a, dev, fixed, t_bar, T), head)
        dev.close()
        return
    solves = []

    def solve():
        solves.append(dev.cond_solve(fixed, t_bar, None, rtol=a.rtol, max_iter=200000)[1])

    rows = {"pl_thermal_load, f_th and n_free (last stage: k_thermal_load)": lambda: dev.thermal_load(),
            "pl_cond_spmv (last stage: k_cond_gather<false>)": lambda: dev.cond_spmv(T),
            "pl_cond_spmv masked (last stage: k_cond_gather<true>)": lambda: dev.cond_spmv(T, fixed),
            "pl_cond_flux (last stage: k_cond_flux)": lambda: dev.cond_flux(T),
            "pl_cond_sens (last stage: k_cond_sens)": lambda: dev.cond_sens(T, mu),
            "pl_thermal_load_adjoint (last stage: k_thermal_load_adjoint)": lambda: dev.thermal_load_adjoint(lam),
            f"pl_cond_solve rtol {a.rtol:g}, hot Zmin and cold Zmax (last stage: the PCG)": solve}
    conv_solves = []

    def conv_solve():
        conv_solves.append(dev.cond_solve(fixed, t_bar, None, rtol=a.rtol, max_iter=200000)[1])

    plain_gather = "pl_cond_spmv (last stage: k_cond_gather<false>)"
    conv_gather = "convection: pl_cond_spmv (last stage: k_cond_gather<false, true>)"
    conv_rows = {conv_gather: lambda: dev.cond_spmv(T),
                 "convection: pl_cond_spmv masked (last stage: k_cond_gather<true, true>)": lambda: dev.cond_spmv(T, fixed),
                 "convection: pl_cond_sens (last stage: k_cond_sens<true>)": lambda: dev.cond_sens(T, mu),
                 "convection: pl_cond_film, Qc and P (last stage: k_cond_film + fold)": lambda: dev.cond_film(T, total=True),
                 "pl_temp_pnorm p 8 with dphi_dT (last stage: values, fold, p-sum, fold, grad)":
                     lambda: dev.temp_pnorm(T, 8.0, a.ambient, ~fixed, gradient=True),
                 f"convection: pl_cond_solve rtol {a.rtol:g}, hot Zmin and cold Zmax (last stage: the PCG)": conv_solve}
    first_conv = next(iter(conv_rows))
    rows.update(conv_rows)
    for name, fn in rows.items():
        if name == first_conv:                    # the plain rows are done: from here on the CONV kernels run
            dev.set_convection(a.film, a.ambient)
        walls, kernels = [], []
        for rep in range(a.reps + 1):
            w, k, _ = _timed(fn)
            if rep:
                walls.append(w)
                kernels.append(k)
        res["rows"][name] = {"wall": _summary(walls), "kernel_hip_events": _summary(kernels)}
    k = {name: r["kernel_hip_events"]["median_ms"] for name, r in res["rows"].items()}
    st = solves[-1]
    res["cond_solve"] = {"iterations": int(st["iterations"]), "rel_residual": float(st["rel_residual"]),
                         "converged": int(st["converged"]), "iterations_of_every_repetition": [int(s["iterations"]) for s in solves]}
    # what the gather has to move: per strut visit (two per strut) the 8-byte incidence entry, 8 bytes of g and 8 bytes of the
    # other node's x; per node 8 bytes of x read and 8 bytes of y written
    res["k_cond_gather_model_bytes"] = int(2 * lat.n_beams * (8 + 8 + 8) + 16 * lat.n_nodes)
    t = k["pl_cond_spmv (last stage: k_cond_gather<false>)"]
    res["k_cond_gather_model_GB_per_s"] = res["k_cond_gather_model_bytes"] / (t * 1e-3) / 1e9
    # the convective gather reads H once per node on top of that
    st = conv_solves[-1]
    res["convection"] = {"film": a.film, "ambient": a.ambient,
                         "cond_solve": {"iterations": int(st["iterations"]), "rel_residual": float(st["rel_residual"]),
                                        "converged": int(st["converged"])},
                         "k_cond_gather_conv_model_bytes": int(res["k_cond_gather_model_bytes"] + 8 * lat.n_nodes),
                         "k_cond_gather_conv_over_plain": k[conv_gather] / k[plain_gather]}
    with open(a.out + ".json", "w") as fh:
        json.dump(res, fh, indent=1)
    lines = [f"{res['lattice']}: {res['n_nodes']} nodes, {res['n_beams']} struts; medians of {a.reps} warm repetitions"]
    for name, r in res["rows"].items():
        kk = r["kernel_hip_events"]
        lines.append(f"  {name:82} wall {r['wall']['median_ms']:9.2f} ms" +
                     (f"   last stage (HIP events) {kk['median_ms']:8.4f} ms" if kk else ""))
    lines.append(f"  pl_cond_solve: {res['cond_solve']['iterations']} iterations, rel_residual "
                 f"{res['cond_solve']['rel_residual']:.2e}")
    lines.append(f"  k_cond_gather: {res['k_cond_gather_model_bytes']} model bytes, "
                 f"{res['k_cond_gather_model_GB_per_s']:.0f} GB/s at the measured time")
    cv = res["convection"]
    lines.append(f"  pl_cond_solve under convection: {cv['cond_solve']['iterations']} iterations, rel_residual "
                 f"{cv['cond_solve']['rel_residual']:.2e}")
    lines.append(f"  k_cond_gather<false, true>: {cv['k_cond_gather_conv_model_bytes']} model bytes, "
                 f"{cv['k_cond_gather_conv_over_plain']:.3f} x the plain gather of this run")
    with open(a.out + ".txt", "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    transient_report(a, transient_rows(a, dev, fixed, t_bar, T), head)
    dev.close()


if __name__ == "__main__":
    main()
