#!/usr/bin/env python3
"""Times the frequency-response sensitivities (pl_harmonic_sens) on the 20^3 Octet column of section
10f, clamped at its base, in one run on one GPU: 32 frequencies from 0.5 to 3.0 w_1 with the damping (0.05 w_1, 0.002 / w_1),
rtol = 1e-8, one warm-up left out, medians of --reps calls:

  - pl_harmonic of this library beside pl_harmonic of another build (--parent-tree: a checkout of the parent commit with its
    library built), each in a child process of its own that imports the package of its tree, the parent's first and last:
    the load stride of k_harm_init must cost nothing, so the three must agree within the run's own spread;
  - pl_harmonic_sens with a generic output vector (twice the column blocks: about twice the sweep expected) and with
    out_vec = NULL (about the sweep alone expected);
  - k_harmonic_sens by HIP events (PL_TIMING), and its share of the call.

    python tools/time_harmonic_sens.py --parent-tree /path/to/parent/checkout --out profiles/r15_harmonic_sens
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (a child process measures the package of another checkout: the sweep uses nothing that checkout lacks)
sys.path.insert(0, os.environ.get("PL_TIME_TREE") or ROOT)
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


def _column(n):
    L = LatticeSim({"geometry": {"cell_size": {"x": 1, "y": 1, "z": 1}, "number_of_cells": {"x": n, "y": n, "z": n},
                                 "radii": [0.05], "geom_types": ["Octet"]},
                    "simulation_parameters": {"enable": True, "material": "VeroClear", "periodicity": False},
                    "boundary_conditions": {
                        "Displacement": {"Fixed": {"Surface": ["Zmin"], "DOF": ["X", "Y", "Z", "RX", "RY", "RZ"],
                                                   "Value": [0, 0, 0, 0, 0, 0]}},
                        "Force": {"Load": {"Surface": ["Zmax"], "DOF": ["X"], "Value": [0.01]}}}})
    N = L.lattice.n_nodes
    dev = L.device_model()
    dev.set_bc(L.fixed_DOF)
    dev.assemble()
    dev.set_mass(1.0)
    fixed = np.asarray(L.fixed_DOF).reshape(N, 6) != 0
    load = np.zeros((N, 6))
    load[:, :3] = np.asarray(L.applied_force)[:N, :3]
    load[fixed] = 0.0
    return L, dev, load


def _sweep(dev, load, w1, reps, max_iter):
    """pl_harmonic over the band: wall ms of reps calls after one warm-up, and the iteration counts"""
    band = np.linspace(0.5, 3.0, 32) * w1
    damping = (0.05 * w1, 0.002 / w1)
    walls, out = [], None
    for rep in range(reps + 1):
        wall, _, out = _captured(lambda: dev.harmonic(band, load, *damping, rtol=1e-8, max_iter=max_iter, raise_on_noconv=False))
        if rep:
            walls.append(wall)
    return {"wall": _summary(walls), "iterations": out["iters"].tolist(), "status": out["status"].tolist()}


def _child(tree, a, w1):
    env = dict(os.environ)
    env.pop("PYLATTICE_HIP_LIB", None)
    env["PL_TIME_TREE"] = os.path.abspath(tree or ROOT)
    cmd = [sys.executable, os.path.abspath(__file__), "--sweep-only", "--w1", repr(w1), "--reps", str(a.reps), "--cells",
           str(a.cells), "--max-iter", str(a.max_iter)]
    text = subprocess.run(cmd, env=env, check=True, stdout=subprocess.PIPE, timeout=600).stdout.decode()
    return json.loads(text.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/r15_harmonic_sens")
    ap.add_argument("--parent-tree", default=None, help="a checkout of the parent commit with its library built")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cells", type=int, default=20)
    ap.add_argument("--max-iter", type=int, default=60000)
    ap.add_argument("--sweep-only", action="store_true", help="(the child processes) pl_harmonic alone, one JSON line")
    ap.add_argument("--w1", type=float, default=None)
    a = ap.parse_args()
    L, dev, load = _column(a.cells)
    if a.sweep_only:
        print(json.dumps(_sweep(dev, load, a.w1, a.reps, a.max_iter)))
        dev.close()
        return
    lat = L.lattice
    N = lat.n_nodes
    res = {"lattice": f"{a.cells}^3 Octet column", "n_nodes": int(N), "n_beams": int(lat.n_beams), "reps": a.reps}
    w1 = float(np.sqrt(dev.vibration_modes(2, n_sub=8, raise_on_noconv=False)["omega2"][0]))
    res["omega_1"] = w1
    band = np.linspace(0.5, 3.0, 32) * w1
    damping = (0.05 * w1, 0.002 / w1)

    res["pl_harmonic"] = {}
    if a.parent_tree:
        res["pl_harmonic"]["parent, first"] = _child(a.parent_tree, a, w1)
    res["pl_harmonic"]["this library"] = _child(None, a, w1)
    if a.parent_tree:
        res["pl_harmonic"]["parent, last"] = _child(a.parent_tree, a, w1)

    l = np.random.default_rng(7).standard_normal((N, 6)) * np.array([1, 1, 1, 0.1, 0.1, 0.1])
    res["pl_harmonic_sens"] = {}
    for name, out_vec in (("generic l", l), ("out_vec = NULL", None)):
        walls, kern, share, out = [], [], [], None
        for rep in range(a.reps + 1):
            wall, text, out = _captured(lambda: dev.harmonic_sens(band, load, out_vec, 2, 8.0, ray_m=damping[0], ray_k=damping[1],
                                                                  rtol=1e-8, max_iter=a.max_iter, raise_on_noconv=False))
            if rep:
                walls.append(wall)
                kern.append(_stage(text, "k_harmonic_sens ")[-1])
                share.append(_stage(text, "k_harmonic_sens_share")[-1])
        res["pl_harmonic_sens"][name] = {"wall": _summary(walls), "k_harmonic_sens": _summary(kern),
                                         "k_harmonic_sens_share_percent": float(np.median(share)),
                                         "iterations_forward": out["iters"][0].tolist(),
                                         "iterations_adjoint": out["iters"][1].tolist(), "status": out["status"].tolist(),
                                         "J": out["J"]}
    own = res["pl_harmonic"]["this library"]["wall"]["median_ms"]
    for r in res["pl_harmonic_sens"].values():
        r["wall_over_pl_harmonic"] = r["wall"]["median_ms"] / own

    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out + ".json", "w") as fh:
        json.dump(res, fh, indent=1)
    lines = [f"{res['lattice']}: {res['n_nodes']} nodes, {res['n_beams']} struts; 32 frequencies 0.5 - 3.0 w_1, rtol 1e-8; "
             f"one warm-up left out, medians of {a.reps}"]
    for name, r in res["pl_harmonic"].items():
        w = r["wall"]
        lines.append(f"  pl_harmonic, {name:16} {w['median_ms']:.1f} ms ({w['min_ms']:.1f} - {w['max_ms']:.1f}), iterations "
                     f"{min(r['iterations'])} - {max(r['iterations'])}, status {sorted(set(r['status']))}")
    for name, r in res["pl_harmonic_sens"].items():
        w, k = r["wall"], r["k_harmonic_sens"]
        it = r["iterations_adjoint"] if any(r["iterations_adjoint"]) else r["iterations_forward"]
        lines.append(f"  pl_harmonic_sens, {name:16} {w['median_ms']:.1f} ms ({w['min_ms']:.1f} - {w['max_ms']:.1f}) = "
                     f"{r['wall_over_pl_harmonic']:.2f} x pl_harmonic; iterations {min(it)} - {max(it)}; k_harmonic_sens "
                     f"{k['median_ms']:.4f} ms ({k['min_ms']:.4f} - {k['max_ms']:.4f}), {r['k_harmonic_sens_share_percent']:.2f} % of "
                     f"the call")
    with open(a.out + ".txt", "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    dev.close()


if __name__ == "__main__":
    main()
