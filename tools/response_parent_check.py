#!/usr/bin/env python3
"""One-off checks of the response refactor, each mode in a process of its own:

  bits TREE OUT.npz      the four response entry points on case A of the four GPU test files, every output array saved
  compare A.npz B.npz    == on every array, one verdict line per call
  time TREE              whole_call_host_clock of pl_transient and pl_transient_sens (PL_TIMING) on the 20^3 Octet column
"""
import os
import re
import sys
import tempfile

import numpy as np

mode = sys.argv[1]
if mode in ("bits", "time"):
    TREE = os.path.abspath(sys.argv[2])
    sys.path.insert(0, os.path.join(TREE, "tests"))
    sys.path.insert(0, TREE)
    os.environ.pop("PYLATTICE_HIP_LIB", None)


def captured(fn):
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile(mode="w+b") as tmp:
        os.dup2(tmp.fileno(), 2)
        try:
            out = fn()
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        tmp.seek(0)
        text = tmp.read().decode(errors="replace")
    return text, out


def bits(out_path):
    import pylatticedso_amd
    from pylatticedso_amd import _capi
    assert os.path.abspath(pylatticedso_amd.__file__).startswith(TREE), pylatticedso_amd.__file__
    assert os.path.abspath(_capi.LIB_PATH).startswith(TREE), _capi.LIB_PATH
    import test_gpu_harmonic_sens as HS
    import test_gpu_transient_sens as TS
    res = {}

    def keep(call, out):
        for k, v in out.items():
            if v is not None:
                res[f"{call}/{k}"] = np.asarray(v)

    t = TS._get("A")
    dev = t.devs[1]
    T = _capi.TRANSIENT_SENS_CHUNK
    top = [int(v) for v in t.top[:2]]
    keep("pl_transient", dev.transient(t.dt, 40, t.load[None], np.ones((41, 1)), u0=t.u0, v0=t.v0, ray_m=t.damping[0],
                                       ray_k=t.damping[1], rtol=1e-12, max_iter=5000, probes=[top[0], top[1], top[0]],
                                       snap_every=2))
    keep("pl_transient_sens", dev.transient_sens(rtol=1e-12, max_iter=5000, **t.args(kind=2, n_steps=T + 1, base=True)))
    h = HS._get("A")
    dev = h.devs[1]
    W = h.W[:5]
    keep("pl_harmonic", dev.harmonic(W, h.load, *h.D, probes=[int(h.top[1]), int(h.top[0]), int(h.top[1])], fields=True,
                                     rtol=1e-10, max_iter=4000, block=2))
    keep("pl_harmonic_sens out_vec", dev.harmonic_sens(rtol=1e-10, max_iter=4000, block=2, **h.args("dead", 2, W)))
    keep("pl_harmonic_sens out_vec=NULL base_dir", dev.harmonic_sens(rtol=1e-10, max_iter=4000, block=2,
                                                                      **h.args("self_base", 2, W)))
    np.savez(out_path, **res)
    print(f"saved {len(res)} arrays to {out_path}")


def compare(a_path, b_path):
    a, b = np.load(a_path), np.load(b_path)
    assert sorted(a.files) == sorted(b.files), (a.files, b.files)
    calls = sorted({k.split("/")[0] for k in a.files})
    ok = True
    for call in calls:
        keys = [k for k in a.files if k.split("/")[0] == call]
        diff = [k.split("/")[1] for k in keys
                if not (a[k].shape == b[k].shape and a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]))]
        names = ", ".join(f"{k.split('/')[1]}{list(a[k].shape)}" for k in keys)
        nonzero = all(np.asarray(a[k]).any() for k in keys if k.split("/")[1] in ("dJ_dr", "y", "probe", "fields", "energy"))
        ok = ok and not diff
        print(f"  {call}: {'identical to the parent' if not diff else 'DIFFERS in ' + ', '.join(diff)} ({names})"
              f"{'' if nonzero else '  [an output is all zero]'}")
    return 0 if ok else 1


def timing():
    os.environ["PL_TIMING"] = "1"
    from pylatticedso_amd.lattice_sim import LatticeSim
    n = 20
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
    w1 = float(np.sqrt(dev.vibration_modes(2, n_sub=8, raise_on_noconv=False)["omega2"][0]))
    dt, n_steps = 2.0 * np.pi / w1 / 40.0, 50
    amp = np.ones((n_steps + 1, 1))
    l = np.random.default_rng(7).standard_normal((N, 6)) * np.array([1, 1, 1, 0.1, 0.1, 0.1])
    damping = dict(ray_m=0.05 * w1, ray_k=0.002 / w1)
    calls = {"pl_transient": lambda: dev.transient(dt, n_steps, load[None], amp, rtol=1e-8, **damping),
             "pl_transient_sens": lambda: dev.transient_sens(dt, n_steps, l, 2, 8.0, patterns=load[None], amp=amp, rtol=1e-8,
                                                             **damping)}
    for name, fn in calls.items():
        ms = []
        for rep in range(6):
            text, _ = captured(fn)
            if rep:
                ms.append(float(re.findall(r"whole_call_host_clock\s+([0-9.]+)", text)[-1]))
        print(f"TIME {name} whole_call_host_clock median {np.median(ms):.3f} ms ({min(ms):.3f} - {max(ms):.3f}), 50 steps, 5 reps")
    dev.close()


if mode == "bits":
    bits(sys.argv[3])
elif mode == "compare":
    sys.exit(compare(sys.argv[2], sys.argv[3]))
elif mode == "time":
    timing()
