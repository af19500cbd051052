#!/usr/bin/env python3
"""Times the frequency response (pl_harm_spmv, pl_harmonic) on the 20^3 Octet column of section 10f,
clamped at its base, beside the work it replaces, in one run on one GPU:

  - the complex product of 1 and 8 frequencies against two pl_dyn_spmv_multi calls of two columns per frequency (the real and
    the imaginary coefficients on the pair (Re x, Im x)), HIP events around the launches (PL_TIMING), the calls alternating,
    the first repetition left out;
  - one COCG iteration of 1, 8 and 32 frequencies: the host clock around a pass of --iters iterations that ends in the
    status look, divided by the iterations;
  - a sweep of 32 frequencies through the first resonances with the damping (0.05 w_1, 0.002 / w_1), and pl_transient driven
    at one of these frequencies until the start-up transient has decayed to 1e-3, as the order-of-magnitude comparison.

    python tools/time_harmonic.py --out profiles/r14_harmonic
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
os.environ["PL_TIMING"] = "1"

from pylatticedso_amd.lattice_sim import LatticeSim                    # noqa: E402


def _captured(fn):
    """(wall ms, the library's PL_TIMING lines on stderr, result)."""
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
    return wall, text, out


def _stage(text, name):
    return [float(v) for v in re.findall(re.escape(name) + r"\s+([0-9.]+)", text)]


def _summary(ms):
    return {"min_ms": min(ms), "median_ms": float(np.median(ms)), "max_ms": max(ms), "all_ms": ms}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/r14_harmonic")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cells", type=int, default=20)
    ap.add_argument("--iters", type=int, default=192)
    ap.add_argument("--max-iter", type=int, default=60000)
    a = ap.parse_args()
    n = a.cells
    L = LatticeSim({"geometry": {"cell_size": {"x": 1, "y": 1, "z": 1}, "number_of_cells": {"x": n, "y": n, "z": n},
                                 "radii": [0.05], "geom_types": ["Octet"]},
                    "simulation_parameters": {"enable": True, "material": "VeroClear", "periodicity": False},
                    "boundary_conditions": {
                        "Displacement": {"Fixed": {"Surface": ["Zmin"], "DOF": ["X", "Y", "Z", "RX", "RY", "RZ"],
                                                   "Value": [0, 0, 0, 0, 0, 0]}},
                        "Force": {"Load": {"Surface": ["Zmax"], "DOF": ["X"], "Value": [0.01]}}}})
    lat = L.lattice
    N = lat.n_nodes
    dev = L.device_model()
    dev.set_bc(L.fixed_DOF)
    dev.assemble()
    dev.set_mass(1.0)
    res = {"lattice": f"{n}^3 Octet column", "n_nodes": int(N), "n_beams": int(lat.n_beams), "reps": a.reps}
    rng = np.random.default_rng(0)

    # 1. the product
    res["product"] = {}
    for nf in (1, 8):
        X = rng.standard_normal((nf, N, 6)) + 1j * rng.standard_normal((nf, N, 6))
        coef = np.column_stack([1.0 + 0.1j * (1 + np.arange(nf)), -0.5 * (1 + np.arange(nf)) + 0.2j])
        pairs = [np.stack([X[k].real, X[k].imag]) for k in range(nf)]
        for masked in (False, True):
            fused, split = [], []
            for rep in range(a.reps + 1):
                t = _stage(_captured(lambda: dev.harm_spmv(coef, X, masked=masked))[1], "kernel_hip_event")[-1]
                s = 0.0
                for k in range(nf):
                    for c_K, c_M in ((coef[k, 0].real, coef[k, 1].real), (coef[k, 0].imag, coef[k, 1].imag)):
                        s += _stage(_captured(lambda: dev.dyn_spmv_multi(c_K, c_M, pairs[k], masked=masked))[1],
                                    "kernel_hip_event")[-1]
                if rep:
                    fused.append(t)
                    split.append(s)
            row = {"harm_spmv": _summary(fused), "two_dyn_spmv_multi_of_two_columns_per_frequency": _summary(split)}
            row["ratio_of_medians"] = row["harm_spmv"]["median_ms"] / row["two_dyn_spmv_multi_of_two_columns_per_frequency"]["median_ms"]
            res["product"][f"{nf} frequencies{', masked' if masked else ''}"] = row

    # 2. the first natural frequencies, then one iteration of 1 / 8 / 32 frequencies
    fixed = np.asarray(L.fixed_DOF).reshape(N, 6) != 0
    load = np.zeros((N, 6))
    load[:, :3] = np.asarray(L.applied_force)[:N, :3]
    load[fixed] = 0.0
    modes = dev.vibration_modes(6, n_sub=16, raise_on_noconv=False)
    w = np.sqrt(modes["omega2"])
    res["omega"] = [float(v) for v in w]
    damping = (0.05 * w[0], 0.002 / w[0])
    band = np.linspace(0.5 * w[0], 1.1 * w[5], 32)
    top = np.flatnonzero(lat.node_xyz[:, 2] > lat.node_xyz[:, 2].max() - 1e-9)[:4]
    res["iteration"] = {}
    for nf in (1, 8, 32):
        per = []
        for rep in range(a.reps + 1):
            text = _captured(lambda: dev.harmonic(band[:nf] + 0.3 * w[0], load, *damping, probes=top, rtol=1e-30,
                                                  max_iter=a.iters, raise_on_noconv=False))[1]
            if rep:
                per.append(_stage(text, "iteration_mean_host_clock")[-1])
        res["iteration"][f"{nf} frequencies"] = _summary(per)

    # 3. the sweep, and one of its frequencies by time stepping
    wall, text, out = _captured(lambda: dev.harmonic(band, load, *damping, probes=top, rtol=1e-8, max_iter=a.max_iter,
                                                     raise_on_noconv=False))
    res["sweep"] = {"frequencies": 32, "band_over_w1": [float(band[0] / w[0]), float(band[-1] / w[0])], "rtol": 1e-8,
                    "wall_ms": wall, "whole_call_host_clock_ms": _stage(text, "whole_call_host_clock")[-1],
                    "iteration_mean_ms": _stage(text, "iteration_mean_host_clock")[-1],
                    "iterations": out["iters"].tolist(), "status": out["status"].tolist(),
                    "peak_amplitude": [float(v) for v in np.linalg.norm(out["probe"][:, 0, :3], axis=1)]}
    k = 8
    zeta = 0.5 * (damping[0] / w[0] + damping[1] * w[0])
    dt = 2.0 * np.pi / band[k] / 40.0
    n_steps = int(np.ceil(np.log(1e3) / (zeta * w[0]) / dt))
    amp = np.cos(band[k] * dt * np.arange(n_steps + 1))[:, None]
    wall_t, text_t, tr = _captured(lambda: dev.transient(dt, n_steps, load[None], amp, ray_m=damping[0], ray_k=damping[1],
                                                         rtol=1e-8, probes=top))
    tail = tr["probe"][-80:, 0, 0, :3]                   # the last two periods of the first probe
    res["transient_to_steady_state"] = {
        "omega_over_w1": float(band[k] / w[0]), "steps": n_steps, "wall_ms": wall_t,
        "iterations_per_step": _stage(text_t, "iterations_per_step")[-1],
        "amplitude_last_two_periods": float(np.abs(tail).max(axis=0).max()),
        "amplitude_frequency_response": float(np.abs(out["probe"][k, 0, :3]).max())}
    res["sweep_wall_per_frequency_over_transient_wall"] = wall / 32 / wall_t

    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out + ".json", "w") as fh:
        json.dump(res, fh, indent=1)
    lines = [f"{res['lattice']}: {res['n_nodes']} nodes, {res['n_beams']} struts; {a.reps} warm repetitions, medians"]
    for name, r in res["product"].items():
        lines.append(f"  product, {name:24} harm_spmv {r['harm_spmv']['median_ms']:.4f} ms, 2 x dyn_spmv_multi(2) per frequency "
                     f"{r['two_dyn_spmv_multi_of_two_columns_per_frequency']['median_ms']:.4f} ms, ratio {r['ratio_of_medians']:.2f}")
    for name, r in res["iteration"].items():
        lines.append(f"  one COCG iteration, {name:16} {r['median_ms']:.4f} ms ({r['min_ms']:.4f} - {r['max_ms']:.4f})")
    s = res["sweep"]
    lines.append(f"  sweep of 32 frequencies, {s['band_over_w1'][0]:.2f} - {s['band_over_w1'][1]:.2f} w_1, rtol 1e-8: {s['wall_ms']:.1f} ms, "
                 f"iterations {min(s['iterations'])} - {max(s['iterations'])}, status {sorted(set(s['status']))}, "
                 f"{s['iteration_mean_ms']:.4f} ms per iteration")
    t = res["transient_to_steady_state"]
    lines.append(f"  pl_transient at {t['omega_over_w1']:.2f} w_1 to steady state: {t['steps']} steps, {t['wall_ms']:.1f} ms, "
                 f"{t['iterations_per_step']:.1f} iterations per step; amplitude {t['amplitude_last_two_periods']:.4e} against "
                 f"{t['amplitude_frequency_response']:.4e}")
    lines.append(f"  sweep wall per frequency / transient wall: {res['sweep_wall_per_frequency_over_transient_wall']:.4f}")
    with open(a.out + ".txt", "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    dev.close()


if __name__ == "__main__":
    main()
