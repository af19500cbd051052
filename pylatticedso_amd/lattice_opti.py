"""Host-side mirror of the reference's ``LatticeOpti`` for the sensitivity pass of the hot path.

Mirrors ``src/pyLatticeOpti/lattice_opti.py``: preset block ``optimization_informations`` (:228-256), the
parameterisations ``constant`` / ``constant+hybrid`` / ``unit_cell`` / ``linear`` (:467-560, :1468-1485),
normalisation (:1318-1400), ``objective`` (:430-465), ``compute_compliance`` (:645-663), ``gradient`` (:701-731) with
its sign flip and ``(r_max − r_min)/C0`` scaling, and the SciPy SLSQP driver (:141-195, stays SciPy).

What runs on the GPU: the equilibrium solve (``solve_FEM_FenicsX``), the adjoint solve for displacement objectives and
the per-strut contraction ``λ_eᵀ (∂K_e/∂r) u_e`` (``pl_sens``) — the reference obtains the same quantity as
``u_cellᵀ (∂S/∂r) u_cell`` with a finite-differenced cell Schur complement (``lattice_sim.py:1020-1054``), at fixed
penalised-segment geometry (convention (i) of SURVEY.md appendix A).

``simulation_type: "DDM"`` (what most of the reference's optimisation presets use): the equilibrium goes through
``solve_DDM`` on the device with surrogate cell Schur complements, the gradient contracts their spline derivatives
(``schur_surrogate.py``) cell by cell.

Out of scope here: the kriging relative-density surrogate; the density constraint uses the
direct strut-volume formula instead.
"""
from __future__ import annotations

import time
from typing import Callable, NamedTuple

import numpy as np

from . import geometric_host as GH
from .lattice_sim import LatticeSim, open_lattice_parameters
from .utils_simulation import solve_FEM_FenicsX

_DOF = {"X": 0, "Y": 1, "Z": 2, "RX": 3, "RY": 4, "RZ": 5}


class _ResponseConstraint(NamedTuple):
    """One response constraint of the preset (FEM mode).  `stem` names its methods and attributes: _<stem>_settings (whose first
    entry is the limit), <stem>_constraint, <stem>_constraint_gradient and _last_<stem>, the (aggregate, peak) of the last
    evaluation, whose peak goes into _history[history] per iteration.  The aggregate method returns (q, peak, ...); the
    constraint is scale(q, limit) - 1 <= 0 and its gradient scale(dq/dtheta, limit).  gradient: "partials" - aggregate(want_grad)
    ends with (dq/du, dq/dr at fixed u) for _aggregate_gradient; "total" - it ends with dq/dr_b for
    _strut_gradient_to_parameters; "shared" - aggregate() gives the value and dq/dr_b in one call.  reason: why DDM mode refuses."""
    key: str
    stem: str
    history: str
    reason: str
    aggregate: str
    scale: Callable
    gradient: str


def _over(q, limit):
    return q / limit


def _times(q, limit):
    return limit * q


def _times_circular_squared(q, limit):
    return (2.0 * np.pi * limit) ** 2 * q


def _equilibrium_load(model):
    """The load of the model's equilibrium problem: its external forces plus, under a temperature, the thermal loads
    solve_problem composed (K u = f_ext + f_th)."""
    f_th = getattr(model, "_f_th", None)
    return model._f if f_th is None else model._f + f_th


_INTERIORS = "the recovered interiors of DDM cells"
# in the order they are handed to SLSQP
_RESPONSE_CONSTRAINTS = (
    _ResponseConstraint("max_stress", "stress", "max_stress", f"strut stresses on {_INTERIORS} are not implemented",
                        "strut_stress_aggregate", _over, "partials"),
    _ResponseConstraint("buckling", "buckling", "max_buckling", f"strut forces on {_INTERIORS} are not implemented",
                        "strut_buckling_aggregate", _over, "partials"),
    _ResponseConstraint("global_buckling", "global_buckling", "min_load_factor",
                        f"the geometric stiffness of {_INTERIORS} is not implemented", "global_buckling_aggregate", _times, "total"),
    _ResponseConstraint("frequency", "frequency", "min_frequency", f"the mass of {_INTERIORS} is not implemented",
                        "frequency_aggregate", _times_circular_squared, "total"),
    _ResponseConstraint("peak_displacement", "peak_displacement", "peak_displacement",
                        f"the transient response of {_INTERIORS} is not implemented", "peak_displacement_aggregate", _over, "shared"),
    _ResponseConstraint("resonance_peak", "resonance_peak", "resonance_peak",
                        f"the frequency response of {_INTERIORS} is not implemented", "resonance_peak_aggregate", _over, "shared"),
    _ResponseConstraint("max_temperature", "max_temperature", "max_temperature",
                        "DDM handles carry no strut graph to conduct heat on", "max_temperature_aggregate", _over, "total"),
)
# objectives of the conduction problem alone: no mechanical equilibrium, no mechanical adjoint
_THERMAL_OBJECTIVES = ("thermal_compliance", "heat_dissipation")


class LatticeOpti(LatticeSim):
    def __init__(self, name_file, mesh_trimmer=None, verbose: int = 0, convergence_plotting: bool = False,
                 data_roots=None, reference_compat=None, ddm_gradient=None, paired_adjoint=False):
        """``ddm_gradient``: how the exact-DDM gradient is formed - "finite_difference" (default: central differences of
        whole cell Schur complements, the reference's way) or "analytic" (exact cell matrices only: every cell is condensed
        once, the adjoint and the state are recovered on the whole cell and the per-strut sensitivities summed,
        LatticeSim.recover_cell_interiors).  None: the preset's
        ``simulation_parameters.DDM.schur_complement_computation.gradient``, else "finite_difference".  The two agree to
        the finite differences' own error when the preset has no radius gradient (``_cell_gfac`` = 1, every test and
        timing of this repository).  With one they differ: the central differences perturb the representative's strut
        radii as (r +- h) gfac[rep], so dS/dr already carries gfac[rep], and _ddm_cell_sensitivities multiplies by gfac[c]
        once more (kept as it was: the default path is unchanged); the analytic mode applies the chain rule
        d(strut radius)/d(cell radius) = gfac[c] once.

        ``paired_adjoint`` (FEM mode, displacement / displacement_ratio objectives; opt-in): the gradient solves the state and
        its adjoint right-hand sides as the columns of ONE pl_solve_multi pass under the equilibrium's Dirichlet mask instead
        of one pl_solve per right-hand side with the boundary data re-installed in between.

        ``reference_compat`` (one switch with LatticeSim's): the reference's behaviour where it differs from the consistent
        one - its model of struts shared by several cells (lattice_sim.py docstring here), and for the "linear"
        parameterisation its gradient exactly as it computes it (lattice_opti.py:787-841, 719-720) instead of the
        derivative of the objective (see calculate_gradient)."""
        params = open_lattice_parameters(name_file)
        info = params.get("optimization_informations", {})
        # lattice_opti.py:96-103: simulation_type "DDM" runs every equilibrium through solve_DDM with the cell Schur
        # complements (exact or surrogate) and contracts their derivatives dS/dr for the gradient
        self._ddm_mode = info.get("simulation_type", None) == "DDM"
        for c in _RESPONSE_CONSTRAINTS:
            if self._ddm_mode and c.key in (info.get("constraints") or {}):
                raise NotImplementedError(f'the "{c.key}" constraint needs simulation_type "FEM": {c.reason}')
        if self._ddm_mode and info.get("objective_type", None) in _THERMAL_OBJECTIVES:
            raise NotImplementedError(f'the "{info["objective_type"]}" objective needs simulation_type "FEM": DDM handles carry no '
                                      "strut graph to conduct heat on")
        comp = ((params.get("simulation_parameters", {}).get("DDM") or {}).get("schur_complement_computation") or {})
        if ddm_gradient is None:
            ddm_gradient = comp.get("gradient", "finite_difference") if self._ddm_mode else "finite_difference"
        if ddm_gradient not in ("finite_difference", "analytic"):
            raise ValueError('ddm_gradient must be "finite_difference" or "analytic"')
        if ddm_gradient == "analytic" and not self._ddm_mode:
            raise ValueError('ddm_gradient="analytic" applies to simulation_type "DDM" only (the FEM gradient is analytic '
                             "already)")
        if ddm_gradient == "analytic" and comp.get("type", None) != "exact":
            raise ValueError('ddm_gradient="analytic" needs exact Schur complements '
                             '(schur_complement_computation.type = "exact"): a surrogate has no strut model to differentiate')
        if self._ddm_mode and (params.get("simulation_parameters", {}).get("thermal") is not None):
            raise ValueError('the "thermal" block needs simulation_type "FEM": the cell matrices of DDM mode carry no strut '
                             "temperatures")
        super().__init__(params, mesh_trimmer, verbose, self._ddm_mode, data_roots=data_roots,
                         reference_compat=reference_compat, ddm_gradient=ddm_gradient)
        self.paired_adjoint = bool(paired_adjoint)
        self.solution = None
        self.actual_objective = None
        self.denorm_objective = None
        self.initial_value_objective = None
        self.actualGradient = None
        self.initial_parameters = None
        self.bounds = None
        self.constraints = []
        self.iteration = 0
        self.optim_ftol = 1e-6
        self.optim_disp = True
        self.optim_eps = 1e-3
        self.actual_optimization_parameters = []
        self._sim_is_current = False
        self.min_radius = 0.01
        self.max_radius = 0.1
        self._history = {"iteration": [], "objective_norm": [], "objective": [], "relative_density": [],
                         "parameters": [], "timestamp": []}
        lat = self.lattice
        self._get_optimization_parameters(name_file)
        if self.objective_type in _THERMAL_OBJECTIVES or "max_temperature" in self.constraints_dict:
            if self.conduction is None:
                raise ValueError('thermal objectives and the "max_temperature" constraint need a conduction problem '
                                 '(simulation_parameters["thermal"]["conduction"])')
            if self.objective_type == "heat_dissipation" and self.conduction.get("convection", None) is None:
                raise ValueError('the "heat_dissipation" objective needs the "Convection" block of the conduction problem')
        for c in _RESPONSE_CONSTRAINTS:
            setattr(self, "_last_" + c.stem, None)
            if c.key in self.constraints_dict:
                self._history[c.history] = []
        # (parameters, aggregate) of peak_displacement and resonance_peak: the value and the gradient of one design share one call
        self._peak_cache = self._resonance_cache = None
        self._set_number_parameters_optimization()
        # strut -> (cell, type) of the LAST cell that holds it: Cell.change_beam_radius (cell.py:896-917) is called
        # cell after cell, so a strut shared by several cells ends with the last one's radius
        cell_of = np.repeat(np.arange(lat.n_cells), np.diff(lat.cell_beam_ptr))
        self._beam_cell = np.zeros(lat.n_beams, np.int64)
        self._beam_cell[lat.cell_beam_idx] = cell_of          # later cells overwrite earlier ones
        gr = self.grad_radius if self.grad_radius is not None else np.ones((max(self.num_cells_x, self.num_cells_y,
                                                                                self.num_cells_z), 3))
        pos = lat.cell_pos
        self._cell_gfac = gr[pos[:, 0], 0] * gr[pos[:, 1], 1] * gr[pos[:, 2], 2]     # Cell.get_radius (cell.py:385-412)
        self._cell_center = lat.cell_coord + 0.5 * lat.cell_size
        self._x0 = self._y0 = self._z0 = 0.0

    # -- preset ----------------------------------------------------------------------------------------
    def _get_optimization_parameters(self, name_file):
        info = open_lattice_parameters(name_file).get("optimization_informations", {})
        self.objective_function = info.get("objective_function", None)
        self.objective_type = info.get("objective_type", None)
        self.objectif_data = info.get("objective_data", None)
        self.optim_max_iteration = info.get("max_iterations", 20)
        self.constraints_dict = info.get("constraints", {})
        self.optimization_parameters = info.get("optimization_parameters", None)
        if self.optimization_parameters is None:
            raise ValueError("No optimization parameters defined.")
        self._simulation_type = info.get("simulation_type", None)
        if self._simulation_type not in {"FEM", "DDM"}:
            raise ValueError("Invalid simulation type for optimization. Choose 'FEM' or 'DDM'.")
        self.enable_normalization = info.get("enable_parameter_normalization", False)
        self.enable_gradient_computing = info.get("enable_gradient_computing", False)

    def _set_number_parameters_optimization(self):
        t = self.optimization_parameters["type"]
        if t == "unit_cell":
            self.number_parameters = self.lattice.n_cells * len(self.geom_types)
        elif t == "linear":
            dirs = self.optimization_parameters.get("direction", [])
            if not dirs:
                raise ValueError("No directions provided for linear optimization.")
            if any(d not in {"x", "y", "z"} for d in dirs):
                raise ValueError(f"Invalid direction in {dirs}; valid are 'x', 'y', 'z'.")
            self.number_parameters = len(dirs) + 1
        elif t == "constant":
            self.number_parameters = len(self.geom_types) if self.optimization_parameters.get("hybrid", False) else 1
        else:
            raise ValueError("Invalid optimization parameters type.")

    def redefine_optim_parameters(self, max_iteration=None, ftol=None, disp=None, eps=None):
        if max_iteration is not None:
            self.optim_max_iteration = max_iteration
        if ftol is not None:
            self.optim_ftol = ftol
        if disp is not None:
            self.optim_disp = disp
        if eps is not None:
            self.optim_eps = eps

    # -- normalisation (lattice_opti.py:1318-1400) ---------------------------------------------------------
    def _clamp_radius(self, v):
        return max(self.min_radius, min(self.max_radius, float(v)))

    def denormalize_optimization_parameters(self, r_norm):
        if not self.enable_normalization:
            return list(r_norm)
        r = np.asarray(r_norm, dtype=float) * (self.max_radius - self.min_radius) + self.min_radius
        return np.minimum(self.max_radius, np.maximum(self.min_radius, r)).tolist()       # (_clamp_radius, vectorised)

    def normalize_optimization_parameters(self, r):
        if not self.enable_normalization:
            return list(r)
        out = []
        for v in r:
            if v < self.min_radius or v > self.max_radius:
                raise ValueError("Optimization parameter out of bounds.")
            out.append((v - self.min_radius) / (self.max_radius - self.min_radius))
        return out

    def normalize_objective(self, value):
        if not self.enable_normalization:
            return float(value)
        if self.initial_value_objective is None:
            s = abs(float(value))
            self.initial_value_objective = s if s != 0.0 else 1.0
        return float(value) / self.initial_value_objective

    def _to_normalized_theta_space(self, grad_dr):
        if not self.enable_normalization:
            return grad_dr
        if self.initial_value_objective in (None, 0.0):
            raise RuntimeError("Normalization scale not initialized; call objective() once before grad.")
        return grad_dr * (self.max_radius - self.min_radius) / self.initial_value_objective

    # -- parameters -> radii --------------------------------------------------------------------------------
    def _cell_radii_from_parameters(self, theta):
        """(C, G) base radii per cell and geometry + d r_cell / d theta as a sparse description."""
        t = self.optimization_parameters["type"]
        C, G = self.lattice.n_cells, len(self.geom_types)
        theta = list(map(float, theta))
        if t == "constant":
            if self.optimization_parameters.get("hybrid", False):
                if len(theta) != G:
                    raise ValueError(f"Expected {G} parameters for hybrid constant mode, got {len(theta)}.")
                per = self.denormalize_optimization_parameters(theta)
                return np.tile(np.asarray(per), (C, 1))
            r = self.denormalize_optimization_parameters([theta[0]])[0]
            return np.full((C, G), r)
        if t == "unit_cell":
            return np.asarray(self.denormalize_optimization_parameters(theta)).reshape(C, G)
        if t == "linear":
            dirs = self.optimization_parameters.get("direction", [])
            d_phys = self.denormalize_optimization_parameters([theta[-1]])[0]
            span = self.max_radius - self.min_radius
            L = np.maximum([self.size_x, self.size_y, self.size_z], 1e-16)
            h = (self._cell_center - [self._x0, self._y0, self._z0]) / L
            s = np.zeros(C)
            for i, dkey in enumerate(dirs):
                s += theta[i] * h[:, "xyz".index(dkey)]
            val = np.clip(d_phys + span * s, self.min_radius, self.max_radius)
            return np.tile(val[:, None], (1, G))
        raise ValueError("Invalid optimization parameters type.")

    def set_optimization_parameters(self, optimization_parameters_actual):
        """lattice_opti.py:467-560: map the optimiser's vector to strut radii (device update, topology untouched)."""
        # (this runs once per design variable and SLSQP iteration - the finite-difference density constraint - so it stays in
        #  numpy: the list conversions and np.allclose of the first version were 10 ms per iteration at 192 variables)
        th = np.array(optimization_parameters_actual, dtype=float).ravel()
        if len(th) != self.number_parameters:
            raise ValueError("Invalid number of optimization parameters.")
        prev = getattr(self, "_theta_arr", None)
        if (self.actual_optimization_parameters is not None and prev is not None
                and len(self.actual_optimization_parameters) == len(th) == len(prev)
                and bool(np.all(np.abs(th - prev) <= 1e-10 + 1e-10 * np.abs(prev)))):      # (np.allclose, rtol = atol = 1e-10)
            return
        self._sim_is_current = False
        theta = th.tolist()
        self._theta_arr = th
        self.actual_optimization_parameters = theta
        self.cell_radii = self._cell_radii_from_parameters(theta)
        lat = self.lattice
        lat.beam_radius = (self.cell_radii[self._beam_cell, lat.beam_type] * self._cell_gfac[self._beam_cell])
        if self._ddm_mode:
            # reset_cell_with_new_radii (lattice_sim.py:1421-1497): new cell radii -> new Schur complements (+ dS/dr)
            lat.cell_radii = self.cell_radii * self._cell_gfac[:, None]
            # exact: one device condensation per distinct radius set (+ central differences for dS/dr when gradients
            # are on, as lattice_sim.py:1020-1054 does with dolfinx solves); surrogates: one batched evaluation - made when
            # the matrices are next asked for (_flush_schur): SLSQP's finite-difference density constraint sets one vector per
            # design variable and iteration that is never simulated (round 5, 12 x 4 x 4 cells: 197 evaluations of all cell
            # matrices per SLSQP iteration, 146 of its 186 ms)
            self._schur_stale = True
            return
        # the device gets the new radii when it is next asked for (device_model): SLSQP differentiates the density constraint by
        # finite differences - 54 parameter vectors per iteration on the reference's 6x3x3 preset, none of which is simulated
        # (round 5: 1 174 of 1 253 calls of this method in a 20-iteration run uploaded radii nobody used)
        self._device_radii_stale = True

    def _flush_schur(self):
        """Cell matrices (and dS/dr) for the radii set last: evaluated here, not in set_optimization_parameters."""
        if getattr(self, "_schur_stale", False):
            self._schur_stale = False
            self.calculate_schur_complement_cells()

    def ddm_model(self):
        self._flush_schur()
        return super().ddm_model()

    def device_model(self, **kw):
        """As LatticeSim.device_model; a design loop solves ONE slowly changing system over and over, so its handle starts every
        solve from the best combination of its last six solutions for the system at hand (pl_opts_t.warm_start = 4, the Galerkin
        start; round 5 - until then the previous solution, and for compliance only: an objective with an adjoint solve alternates
        two right-hand sides on the handle, which a projection does not mind - the states and the adjoints of the last design
        iterations are all candidates).  Radii set since the last call are uploaded here."""
        if self._device is None:
            kw.setdefault("warm_start", 4)
        fresh = self._device is None
        dev = super().device_model(**kw)
        if getattr(self, "_device_radii_stale", False) and not self._ddm_mode:
            if not fresh:                      # (a handle created just now was built from the current radii)
                dev.update_radii(self.lattice.beam_radius)
            self._device_radii_stale = False
        return dev

    # -- equilibrium / objective ------------------------------------------------------------------------------
    def _initialize_simulation_parameters(self):
        self.reaction_force_vector[:] = 0.0
        self.displacement_vector[:] = 0.0
        self.fixed_DOF[:] = False
        self.applied_force[:] = 0.0
        self.set_boundary_conditions()

    def _simulate_lattice_equilibrium(self):
        self._initialize_simulation_parameters()
        if self._ddm_mode:
            xsol, info, _, _ = self.solve_DDM()
            if xsol is None:
                raise RuntimeError("solve_DDM: zero right-hand side")
        else:
            if self._needs_mechanics:
                _, self._model = solve_FEM_FenicsX(self)
            if self._needs_temperature and not (self._needs_mechanics and self.conduction_driven):
                # (under a conduction-driven temperature the mechanical solve has just solved the conduction problem)
                dev = self.device_model()
                self._assemble_for_conduction(dev)
                self._solve_conduction(dev)
        self._sim_is_current = True

    @property
    def _needs_mechanics(self):
        """False when neither the objective nor a constraint reads the displacements: only the conduction problem is solved."""
        return (self.objective_type not in _THERMAL_OBJECTIVES or
                any(c.key in self.constraints_dict for c in _RESPONSE_CONSTRAINTS if c.key != "max_temperature"))

    @property
    def _needs_temperature(self):
        return self.objective_type in _THERMAL_OBJECTIVES or "max_temperature" in self.constraints_dict

    def _ambient(self):
        cv = self.conduction.get("convection", None)
        return self.conduction["reference"] if cv is None else cv["ambient"]

    def _thermal_adjoint_sens(self, dJ_dT):
        """mu^T d[(K_T + H) T - H T_inf]/dr_b with (K_T + H) mu = dJ/dT on the free thermal nodes, mu = 0 on the others
        (pl_cond_solve_adjoint, pl_cond_sens): what every functional of the temperature subtracts from its partial derivative."""
        dev = self.device_model()
        fixed = self.conduction["fixed"]
        mu, _ = dev.cond_solve(fixed, None, np.where(fixed, 0.0, dJ_dT), rtol=1e-10, max_iter=200000, adjoint=True)
        return dev.cond_sens(self.temperature_field, mu, convective=self.convection_chain)

    def _equilibrium_at(self, r):
        """The design r set and its equilibrium solved, unless the last solve is already that of r."""
        self.set_optimization_parameters(r)
        if not self._sim_is_current:
            self._simulate_lattice_equilibrium()

    def compute_compliance(self):
        """C = sum_k f_k u_k over loaded dofs (lattice_opti.py:645-663)."""
        return float((self.applied_force * self.displacement_vector).sum())

    def _objective_nodes(self, surfaces):
        return self.find_point_on_lattice_surface(surfaces)

    def calculate_objective(self):
        if self.objective_type == "thermal_compliance":     # q . (T - T_inf) over the free nodes
            q = self.conduction["heat_flow"]
            if q is None:
                return 0.0
            return float((q * (self.temperature_field - self._ambient()))[~self.conduction["fixed"]].sum())
        if self.objective_type == "heat_dissipation":       # P = sum_i H_i (T_i - T_inf)
            return self.dissipated_power()
        if self.objective_type == "compliance":
            return self.compute_compliance()
        if self.objective_type == "displacement":
            nodes = self._objective_nodes(self.objectif_data["Surface"])
            vals = [self.displacement_vector[n, _DOF[d]] for n in nodes for d in self.objectif_data["DOF"]]
            mean_disp = float(np.mean(vals))
            if self.objective_function == "max":
                return -mean_disp
            if self.objective_function == "min":
                return mean_disp
            raise ValueError("objective_function must be 'min' or 'max'")
        if self.objective_type == "displacement_ratio":
            u_in, u_out, _ = self._ratio_terms()
            return -(u_out * u_in)                 # lattice_opti.py:616-636 (inverse mechanism: u_out ~ -u_in)
        if self.objective_type == "stiffness":
            raise NotImplementedError("Stiffness objective not implemented yet.")     # as the reference (:638)
        raise ValueError("Invalid objective function type.")

    def _ratio_terms(self):
        """displacement_ratio (lattice_opti.py:616-636, 1560-1621): mean displacement of the loaded dofs (the boundary
        condition named "Load", under "Force" if there is a force block, else under "Displacement"), mean displacement of
        the objective's dofs, and q = dJ/du of J = -(u_out u_in) on the nodes.  For one DOF per set - what the reference's
        presets use - these are the reference's own coefficients (-u_in / n_out on the output nodes, -u_out / n_in on the
        loaded ones); with several DOFs the reference divides by the node count only, which is not the derivative of its
        mean over nodes x DOFs: here q is the derivative."""
        bd = self.boundary_conditions
        if bd.get("Force", None) is not None:
            bd = bd["Force"]
        elif bd.get("Displacement", None) is not None:
            bd = bd["Displacement"]
        else:
            raise ValueError("No boundary conditions defined for displacement ratio objective.")
        if "Load" not in bd:
            raise ValueError('displacement_ratio needs a boundary condition named "Load" (lattice_opti.py:625)')
        nodes_in = np.asarray(self._objective_nodes(bd["Load"]["Surface"]), dtype=np.int64)
        nodes_out = np.asarray(self._objective_nodes(self.objectif_data["Surface"]), dtype=np.int64)
        c_in = [_DOF[d] for d in bd["Load"]["DOF"]]
        c_out = [_DOF[d] for d in self.objectif_data["DOF"]]
        u = self.displacement_vector
        u_in = float(np.mean(u[np.ix_(nodes_in, c_in)]))
        u_out = float(np.mean(u[np.ix_(nodes_out, c_out)]))
        q = np.zeros_like(u)
        for k in c_out:
            np.add.at(q, (nodes_out, k), -u_in / (len(nodes_out) * len(c_out)))
        for k in c_in:
            np.add.at(q, (nodes_in, k), -u_out / (len(nodes_in) * len(c_in)))
        return u_in, u_out, q

    def objective(self, r):
        self._equilibrium_at(r)
        objective = self.calculate_objective()
        self.denorm_objective = objective
        val = self.normalize_objective(objective)
        if self.objective_function == "max":
            val = -val
        elif self.objective_function != "min":
            raise ValueError("objective_function must be 'min' or 'max'")
        self.actual_objective = val
        return val

    # -- sensitivities ------------------------------------------------------------------------------------------
    def _adjoint(self, q):
        """Solve K lam = q on the free dofs (lam = 0 on constrained ones) with the device PCG."""
        dev = self.device_model()
        fixed = self._model._fixed
        dev.set_bc(fixed, None, np.where(fixed, 0.0, q))
        lam, _ = dev.solve(rtol=1e-10, max_iter=200000)
        dev.set_bc(fixed, self._model._ubar, _equilibrium_load(self._model))     # restore the equilibrium problem
        return lam

    def _paired_state_adjoints(self, qs):
        """The state and the adjoints of the loads qs as the columns of one solve_multi under the equilibrium's mask:
        column 0 carries the prescribed values and loads of the equilibrium, the others zero values and their q on the
        free dofs.  Returns (u, [lam ...])."""
        dev = self.device_model()
        fixed = np.asarray(self._model._fixed, dtype=bool).reshape(-1, 6)
        ubar = np.zeros((1 + len(qs),) + fixed.shape)
        ubar[0] = np.asarray(self._model._ubar).reshape(fixed.shape)
        f = np.stack([np.asarray(_equilibrium_load(self._model), dtype=float).reshape(fixed.shape)] +
                     [np.where(fixed, 0.0, np.asarray(q).reshape(fixed.shape)) for q in qs])
        U, _ = dev.solve_multi(ubar, f, rtol=1e-10, max_iter=200000)
        return U[0], list(U[1:])

    def _unit_mean_load(self, nodes, dofs):
        """d(mean displacement over nodes x dofs)/du as a nodal field."""
        q = np.zeros_like(self._model.u)
        for k in dofs:
            np.add.at(q, (np.asarray(nodes, dtype=np.int64), k), 1.0 / (len(nodes) * len(dofs)))
        return q

    def _sens(self, u, lam):
        """lam^T (dK/dr_b) u minus, under a temperature, lam^T d f_th / d r_b (pl_sens, pl_thermal_sens): the per-strut term
        every adjoint gradient subtracts, since K du/dr = -dK/dr u + d f_th / dr."""
        dev = self.device_model()
        s = dev.sens(u, lam)
        if self.thermal is not None:
            s = s - dev.thermal_sens(u if lam is None else lam)
        if self.conduction_driven and self.conduction_chain:
            # the temperature follows the radii through g = k kappa pi r^2 / L: with c = (d f_th / d dT)^T lam and
            # K_T mu = c on the free thermal nodes, lam^T (d f_th / d dT) dT/dr_b = -mu^T (dK_T/dr_b) T
            cd = self.conduction
            c = dev.thermal_load_adjoint(u if lam is None else lam)
            # (under convection the adjoint operator is K_T + H and cond_sens carries the convective bracket, section 10m)
            mu, _ = dev.cond_solve(cd["fixed"], None, np.where(cd["fixed"], 0.0, c), rtol=1e-10, max_iter=200000, adjoint=True)
            s = s + dev.cond_sens(self.temperature_field, mu, convective=self.convection_chain)
        return s

    conduction_chain = True     # False leaves dT/dr out of the gradients (tests show what that costs)
    convection_chain = True     # False leaves the convective bracket of cond_sens out (the same kind of switch)

    def _no_conduction_driven(self, key):
        if key in ("max_stress", "buckling") and self.conduction_driven:
            raise ValueError(f'the "{key}" constraint under a conduction-driven temperature needs dphi/dT of the p-norm '
                             "kernels (the section force depends on T directly), which is not implemented; give the "
                             "temperature to set_temperature as an array instead")

    def strut_sensitivities(self):
        """s_b such that d(objective)/d r_b = −s_b at fixed segment geometry (compliance: s_b = u_eᵀ ∂K_e/∂r u_e)."""
        dev = self.device_model()
        if self.objective_type == "thermal_compliance":     # dJ/dT = q, no explicit dependence on r
            q = self.conduction["heat_flow"]
            return self._thermal_adjoint_sens(np.zeros(self.lattice.n_nodes) if q is None else q)
        if self.objective_type == "heat_dissipation":       # dJ/dT = H on the free nodes, dJ/dr_b at fixed T = k_b Qc_b / r_b
            Qc = dev.cond_film(self.temperature_field)
            k = 1.0 if dev._mult is None else np.asarray(dev._mult, dtype=float)
            return self._thermal_adjoint_sens(dev._H_host()[0]) - k * Qc / dev._radius
        u = self._model.u
        if self.paired_adjoint and self.objective_type == "displacement":
            nodes = self._objective_nodes(self.objectif_data["Surface"])
            sign = -1.0 if self.objective_function == "max" else 1.0
            q = sign * self._unit_mean_load(nodes, [_DOF[d] for d in self.objectif_data["DOF"]])
            u2, (lam,) = self._paired_state_adjoints([q])
            return self._sens(u2, lam)
        if self.paired_adjoint and self.objective_type == "displacement_ratio":
            # q = -u_in e_out - u_out e_in is linear in two loads that do not depend on the state: three columns
            bd = self.boundary_conditions
            bd = bd["Force"] if bd.get("Force", None) is not None else bd["Displacement"]
            u_in, u_out, _ = self._ratio_terms()
            e_out = self._unit_mean_load(self._objective_nodes(self.objectif_data["Surface"]),
                                         [_DOF[d] for d in self.objectif_data["DOF"]])
            e_in = self._unit_mean_load(self._objective_nodes(bd["Load"]["Surface"]), [_DOF[d] for d in bd["Load"]["DOF"]])
            u2, (l_out, l_in) = self._paired_state_adjoints([e_out, e_in])
            return self._sens(u2, -u_in * l_out - u_out * l_in)
        if self.objective_type == "compliance":
            lam = u
            # prescribed displacements or a thermal load: the adjoint of J = f_ext . u solves K lam = f_ext, the mechanical
            # loads only, and is not u itself
            if np.any(self._model._ubar != 0.0) or self.thermal is not None:
                lam = self._adjoint(self._model._f)
            return self._sens(u, None if lam is u else lam)
        if self.objective_type == "displacement":
            nodes = self._objective_nodes(self.objectif_data["Surface"])
            q = np.zeros_like(u)
            cnt = len(nodes) * len(self.objectif_data["DOF"])
            sign = -1.0 if self.objective_function == "max" else 1.0
            for d in self.objectif_data["DOF"]:
                q[nodes, _DOF[d]] += sign / cnt
            return self._sens(u, self._adjoint(q))
        if self.objective_type == "displacement_ratio":
            return self._sens(u, self._adjoint(self._ratio_terms()[2]))
        raise NotImplementedError(f"Gradient for objective '{self.objective_type}' not implemented yet.")

    def _ddm_adjoint(self, q_nodes):
        """S lam = q on the free cell-boundary dofs (lattice_opti.py:1560-1650: CG to 1e-10, no preconditioner)."""
        dev = self.ddm_model()
        bn = self._boundary_nodes_by_index()
        fixed = self.fixed_DOF[bn]
        dev.set_bc(fixed, None, np.where(fixed, 0.0, q_nodes[bn]))
        if getattr(self, "_ddm_precond", 0) in (2, 3, 4):
            # pl_set_bc drops what depends on the Dirichlet mask: the factorised assembled-Schur preconditioner (2) and the
            # inverted node blocks (3; with their dense level: 4) - the handle is then "not assembled" and pl_solve refuses
            dev.assemble()
        lam_b, _ = dev.solve(rtol=1e-10, max_iter=max(2000, self.number_iteration_max or 0))
        lam = np.zeros_like(self.displacement_vector)
        lam[bn] = lam_b
        return lam

    def _ddm_cell_sensitivities(self):
        """(C, G):  lam_c^T (dS_c/dr_j) u_c per cell and geometry, u_c / lam_c on the cell's boundary nodes in
        Cell.define_node_order_to_simulate order (lattice_opti.py:746-760, 866-890)."""
        self._flush_schur()
        analytic = self.ddm_gradient == "analytic"
        if self.schur_gradients is None and not analytic:
            raise RuntimeError("Schur complement gradients are not available: enable_gradient_computing must be true")
        cb = self.cell_boundary_nodes()
        U = self.displacement_vector[cb].reshape(len(cb), -1)
        lam_nodes = None                          # (rows x 6) adjoint; None: the state itself
        if self.objective_type == "compliance":
            Lam = U
        elif self.objective_type == "displacement":
            nodes = self._objective_nodes(self.objectif_data["Surface"])
            q = np.zeros_like(self.displacement_vector)
            cnt = len(nodes) * len(self.objectif_data["DOF"])
            sign = -1.0 if self.objective_function == "max" else 1.0
            for d in self.objectif_data["DOF"]:
                q[nodes, _DOF[d]] += sign / cnt
            lam_nodes = self._ddm_adjoint(q)
            Lam = lam_nodes[cb].reshape(len(cb), -1)
        elif self.objective_type == "displacement_ratio":
            lam_nodes = self._ddm_adjoint(self._ratio_terms()[2])
            Lam = lam_nodes[cb].reshape(len(cb), -1)
        else:
            raise NotImplementedError(f"Gradient for objective '{self.objective_type}' not implemented yet.")
        G = len(self.geom_types)
        if analytic:
            # lam_c^T (dS_c/dr_j) u_c = sum over the cell's struts of type j of lam_e^T (dK_e/dr) u_e, u and lam recovered on
            # the whole cell (E = [I; -K_II^-1 K_IB]: dS/dr = E^T (dK/dr) E at fixed segment geometry) - no step length
            self.recover_cell_interiors(lam=lam_nodes, want_sens=True)
            btype = self.lattice.beam_type
            s_cell = np.stack([np.bincount(btype[beams], weights=s, minlength=G)[:G]
                               for beams, s in self.cell_strut_sens])
            return s_cell * self._cell_gfac[:, None]
        GA = getattr(self, "_schur_gradients_array", None)
        if GA is not None and GA.shape[1] == G:
            # every cell at once: t = dS[idx[c], j] u_c (batched matrix-vector products), then lam_c . t  (a design with one
            # radius set per cell has as many distinct matrices as cells: the loop below made 4 096 einsum calls at 16^3 cells)
            idx = self.cell_schur_index
            T = np.matmul(GA[idx], U[:, None, :, None])[..., 0]          # (C, G, n)
            s_cell = np.einsum("cgn,cn->cg", T, Lam)
            return s_cell * self._cell_gfac[:, None]
        s_cell = np.zeros((len(cb), G))
        for k, dS_list in enumerate(self.schur_gradients):            # one batched contraction per distinct matrix
            sel = np.flatnonzero(self.cell_schur_index == k)
            for j, dS in enumerate(dS_list):
                s_cell[sel, j] = np.einsum("ci,ij,cj->c", Lam[sel], dS, U[sel])
        return s_cell * self._cell_gfac[:, None]

    def calculate_gradient(self):
        """Raw gradient in the reference's sign convention (lattice_opti.py:735-907): sum over the struts driven by
        each parameter of λ_eᵀ (∂K_e/∂r) u_e (FEM) or over the cells of λ_cᵀ (∂S_c/∂r) u_c (DDM), chained through
        Cell.get_radius and the parameterisation."""
        if self._ddm_mode:
            s_cell = self._ddm_cell_sensitivities()
        else:
            s_cell = self._strut_to_cell(self.strut_sensitivities())
        return self._chain_cell_sensitivities(s_cell, self.reference_compat)

    def _strut_to_cell(self, s):
        """(C, G) sums of a per-strut derivative over the struts every (cell, geometry) radius drives, times the cells'
        gradient factor (Cell.get_radius)."""
        lat = self.lattice
        s_cell = np.zeros((lat.n_cells, len(self.geom_types)))
        np.add.at(s_cell, (self._beam_cell, lat.beam_type), s * self._cell_gfac[self._beam_cell])
        return s_cell

    def _chain_cell_sensitivities(self, s_cell, reference_chain=False):
        """(C, G) derivatives with respect to the cell radii -> the parameterisation's variables (physical units; the
        normalisation of the variables is the caller's).  reference_chain: the reference's own chain rule for "linear"."""
        t = self.optimization_parameters["type"]
        if t == "unit_cell":
            return s_cell.ravel()
        if t == "constant":
            if self.optimization_parameters.get("hybrid", False):
                return s_cell.sum(axis=0)
            return np.array([s_cell.sum()])
        if t == "linear" and reference_chain:
            # The reference's chain rule, verbatim in effect (lattice_opti.py:787-841): slopes are de-normalised like
            # radii (clamped into [r_min, r_max]), the "unclamped radius" r = sum a_k c_k + d is formed with the ABSOLUTE
            # cell-centre coordinates and only decides which cells count; d r / d a_k = c_k, d r / d d = 1.  This is not
            # the derivative of the objective (whose field is r = d + span * sum theta_k (c_k - c0_k) / L_k, :467-560);
            # kept behind this switch so that runs can be compared with the reference number for number.
            dirs = self.optimization_parameters.get("direction", [])
            theta = self.actual_optimization_parameters
            a = [self.denormalize_optimization_parameters([float(theta[i])])[0] for i in range(len(dirs))]
            d0 = self.denormalize_optimization_parameters([float(theta[-1])])[0]
            cen = self._cell_center
            r_un = d0 + sum(a[i] * cen[:, "xyz".index(k)] for i, k in enumerate(dirs))
            active = (r_un > self.min_radius + 1e-12) & (r_un < self.max_radius - 1e-12)
            sc = (s_cell / self._cell_gfac[:, None]).sum(axis=1) * active
            grad = np.zeros(self.number_parameters)
            for i, k in enumerate(dirs):
                grad[i] = (sc * cen[:, "xyz".index(k)]).sum()
            grad[-1] = sc.sum()
            return grad
        if t == "linear":
            dirs = self.optimization_parameters.get("direction", [])
            theta = self.actual_optimization_parameters
            span = self.max_radius - self.min_radius
            L = np.maximum([self.size_x, self.size_y, self.size_z], 1e-16)
            h = (self._cell_center - [self._x0, self._y0, self._z0]) / L
            d_phys = self.denormalize_optimization_parameters([theta[-1]])[0]
            r_un = d_phys + span * sum(theta[i] * h[:, "xyz".index(k)] for i, k in enumerate(dirs))
            active = (r_un > self.min_radius + 1e-12) & (r_un < self.max_radius - 1e-12)
            sc = s_cell.sum(axis=1) * active
            grad = np.zeros(self.number_parameters)
            for i, k in enumerate(dirs):
                grad[i] = (sc * span * h[:, "xyz".index(k)]).sum()
            grad[-1] = sc.sum()
            return grad
        raise NotImplementedError(f"Gradient for optimization type '{t}' not implemented yet.")

    def gradient(self, r):
        """d(normalised objective)/d(theta) (lattice_opti.py:701-731)."""
        self._equilibrium_at(r)
        g = -self.calculate_gradient()
        if self.objective_function == "max":
            g = -g        # objective() negates the (normalised) value for 'max'; keep the pair consistent
        if self.optimization_parameters["type"] == "linear" and not self.reference_compat:
            # slopes act on the physical radius directly (span already applied); only the intercept is normalised
            scale = np.ones(self.number_parameters)
            if self.enable_normalization:
                scale[:] = 1.0 / self.initial_value_objective
                scale[-1] *= (self.max_radius - self.min_radius)
            g = g * scale
        else:
            g = self._to_normalized_theta_space(g)
        self.actualGradient = g.copy()
        return g

    # -- density constraint (direct strut-volume formula) ---------------------------------------------------------
    def relative_density(self):
        lat = self.lattice
        geo = getattr(self, "_density_geometry", None)
        if geo is None or geo[0] is not lat.beam_conn:          # strut lengths and the cells' volume: fixed by the topology
            d = lat.node_xyz[lat.beam_conn[:, 1]] - lat.node_xyz[lat.beam_conn[:, 0]]
            geo = self._density_geometry = (lat.beam_conn, np.pi * np.linalg.norm(d, axis=1),
                                            float(lat.cell_size.prod(axis=1).sum()))
        r = lat.beam_radius
        return float((geo[1] * r * r).sum() / geo[2])

    def density_constraint(self, r):
        self.set_optimization_parameters(r)
        return self.relative_density() - float(self.constraints_dict["relative_density"]["value"])

    # -- stress constraint (FEM mode): p-norm of the strut von Mises stresses, pl_stress_pnorm -----------------------------
    def _stress_settings(self):
        c = self.constraints_dict["max_stress"]
        return float(c["value"]), float(c.get("p", 8)), int(c.get("where", 1))

    def strut_stress_aggregate(self, want_grad=False):
        """(Phi_p, sigma_max, dPhi/du, dPhi/dr at fixed u) of the current equilibrium with the constraint's p and where."""
        _, p, where = self._stress_settings()
        out = self.device_model().stress_pnorm(p, self._model.u, where=where, want_grad=want_grad)
        self._last_stress = (out[0], out[1])
        return out

    def stress_constraint(self, r):
        """Phi_p / s_allow - 1 (<= 0 when feasible; Phi_p >= the largest von Mises stress of any strut station)."""
        return self._constraint_value("max_stress", r)

    def stress_constraint_gradient(self, r):
        """d(stress_constraint)/d(theta): dPhi/dr_b = dPhi/dr_b at fixed u - lam^T (dK/dr_b) u with K lam = dPhi/du on the free
        dofs (lam = 0 on prescribed ones, which take no load), chained through Cell.get_radius and the parameterisation
        as the objective's gradient is."""
        return self._constraint_gradient("max_stress", r)

    # -- what the response constraints share (_RESPONSE_CONSTRAINTS) -------------------------------------------------------
    def _constraint_limit(self, c):
        return getattr(self, f"_{c.stem}_settings")()[0]

    def _constraint_value(self, key, r):
        c = next(c for c in _RESPONSE_CONSTRAINTS if c.key == key)
        self._no_conduction_driven(key)
        self._equilibrium_at(r)
        return c.scale(getattr(self, c.aggregate)()[0], self._constraint_limit(c)) - 1.0

    def _constraint_gradient(self, key, r):
        c = next(c for c in _RESPONSE_CONSTRAINTS if c.key == key)
        self._no_conduction_driven(key)
        self._equilibrium_at(r)
        aggregate =getattr(self, c.aggregate)
        out = aggregate() if c.gradient == "shared" else aggregate(want_grad=True)
        g = self._aggregate_gradient(out[2], out[3]) if c.gradient == "partials" else self._strut_gradient_to_parameters(out[2])
        return c.scale(g, self._constraint_limit(c))

    def _cached_aggregate(self, cache, compute):
        """compute() for the current design, unless the one-entry cache (an attribute's name) already holds it."""
        key = tuple(map(float, self.actual_optimization_parameters)) if len(self.actual_optimization_parameters) else None
        hit = getattr(self, cache)
        if hit is not None and key is not None and hit[0] == key:
            return hit[1]
        res = compute()
        setattr(self, cache, (key, res))
        return res

    def _aggregate_gradient(self, dq_du, dq_dr):
        """dq/d(theta) of a scalar q(u(r), r) of the equilibrium from its partial derivatives: dq/dr_b = dq/dr_b at fixed u -
        lam^T (dK/dr_b) u (+ lam^T d f_th / dr_b under a temperature, _sens) with K lam = dq/du on the free dofs, through
        _strut_to_cell, the parameterisation's chain and the normalisation of the variables."""
        lam = self._adjoint(dq_du)
        return self._strut_gradient_to_parameters(dq_dr - self._sens(self._model.u, lam))

    def _strut_gradient_to_parameters(self, s):
        """dq/d(theta) from the total per-strut derivatives dq/dr_b: _strut_to_cell, the parameterisation's chain and the
        normalisation of the variables."""
        g = self._chain_cell_sensitivities(self._strut_to_cell(s))
        scale = np.ones(self.number_parameters)          # d(physical variable)/d(theta)
        if self.enable_normalization:
            span = self.max_radius - self.min_radius
            if self.optimization_parameters["type"] == "linear":
                scale[-1] = span                          # the slopes act on the physical radius directly
            else:
                scale[:] = span
        return g * scale

    # -- buckling constraint (FEM mode): p-norm of the struts' Euler utilisations, pl_buckling_pnorm ------------------------
    def _buckling_settings(self):
        c = self.constraints_dict["buckling"]
        return float(c.get("value", 1.0)), float(c.get("p", 8)), dict(length=int(c.get("length", 1)),
                                                                        k_eff=float(c.get("k_eff", 1.0)),
                                                                        shear=int(c.get("shear", 0)))

    def strut_buckling_aggregate(self, want_grad=False):
        """(B_p, util_max, dB/du, dB/dr at fixed u) of the current equilibrium with the constraint's p and column model."""
        _, p, kw = self._buckling_settings()
        out = self.device_model().buckling_pnorm(p, self._model.u, want_grad=want_grad, **kw)
        self._last_buckling = (out[0], out[1])
        return out

    def buckling_constraint(self, r):
        """B_p / beta_allow - 1 (<= 0 when feasible; B_p >= the largest utilisation max(0, -N) / N_cr of any strut)."""
        return self._constraint_value("buckling", r)

    def buckling_constraint_gradient(self, r):
        """d(buckling_constraint)/d(theta) by the adjoint chain of stress_constraint_gradient: dB/dr_b at fixed u -
        lam^T (dK/dr_b) u with K lam = dB/du on the free dofs."""
        return self._constraint_gradient("buckling", r)

    # -- temperature constraint (FEM mode): p-norm of the nodal temperature over the free thermal nodes, pl_temp_pnorm ------------
    def _max_temperature_settings(self):
        c = self.constraints_dict["max_temperature"]
        ref = c.get("reference", None)
        return float(c["limit"]), float(c.get("p", 8)), float(self._ambient() if ref is None else ref)

    def max_temperature_aggregate(self, want_grad=False):
        """(Phi_p, peak, dPhi/dr_b or None) of T - reference over the free nodes of the conduction problem at the current
        design (Phi_p >= the peak).  dPhi/dr_b is total: Phi depends on r through T alone, -mu^T d[(K_T + H) T - H T_inf]/dr_b."""
        _, p, ref = self._max_temperature_settings()
        res = self.device_model().temp_pnorm(self.temperature_field, p, ref, ~self.conduction["fixed"], gradient=want_grad)
        self._last_max_temperature = (res["phi"], res["max"])
        return res["phi"], res["max"], (-self._thermal_adjoint_sens(res["dphi_dT"]) if want_grad else None)

    def max_temperature_constraint(self, r):
        """Phi_p / limit - 1 (<= 0 when feasible: Phi_p >= max(T - reference) over the free thermal nodes)."""
        return self._constraint_value("max_temperature", r)

    def max_temperature_constraint_gradient(self, r):
        """d(max_temperature_constraint)/d(theta): dPhi/dr_b / limit through _strut_gradient_to_parameters."""
        return self._constraint_gradient("max_temperature", r)

    # -- global buckling constraint (FEM mode): p-norm of 1 / lambda_i, pl_buckling_modes + pl_buckling_modes_sens ------------
    def _global_buckling_settings(self):
        c = self.constraints_dict["global_buckling"]
        kw = {k: c[k] for k in ("n_sub", "rtol", "max_iter", "tol", "max_outer") if k in c}
        return float(c.get("value", 1.0)), int(c.get("n_modes", 4)), float(c.get("p", 8)), kw

    def global_buckling_aggregate(self, want_grad=False):
        """(J_p, lambda_1, dJ/dr_b or None) of the current equilibrium: J_p = (sum_i lambda_i^-p)^(1/p) over the constraint's
        n_modes smallest positive load factors (J_p >= 1 / lambda_1; 0 and lambda_1 = inf when none exists).  dJ/dr_b is the
        device's weighted sum of the rows of pl_buckling_modes_sens and is total: the adjoint for u(r) is inside that call."""
        _, n_modes, p, kw = self._global_buckling_settings()
        self.global_buckling(n_modes, **kw)
        out = self.global_buckling_sensitivity(p, want_rows=False) if want_grad else None
        lam = self.buckling_load_factors
        lam1 = float(lam[0]) if np.isfinite(lam[0]) else float("inf")
        J = out["aggregate"] if want_grad else GH.load_factor_aggregate(lam, p)[0]
        self._last_global_buckling = (J, lam1)
        return J, lam1, (out["dJ_dr"] if want_grad else None)

    def global_buckling_constraint(self, r):
        """lambda_min J_p - 1 (<= 0 when feasible: J_p >= 1 / lambda_1, so lambda_1 >= lambda_min then; -1 when no positive load
        factor exists)."""
        return self._constraint_value("global_buckling", r)

    def global_buckling_constraint_gradient(self, r):
        """d(global_buckling_constraint)/d(theta): lambda_min dJ/dr_b through the tail of _aggregate_gradient."""
        return self._constraint_gradient("global_buckling", r)

    # -- frequency constraint (FEM mode): p-norm of 1 / omega_i^2, pl_vibration_modes + pl_vibration_modes_sens -------------------
    def _frequency_settings(self):
        c = self.constraints_dict["frequency"]
        kw = {k: c[k] for k in ("n_sub", "rtol", "max_iter", "tol", "max_outer") if k in c}
        mass = dict(density=float(c.get("density", 1.0)), rotary=bool(c.get("rotary", True)), node_mass=c.get("node_mass", None))
        return float(c["value"]), int(c.get("n_modes", 4)), float(c.get("p", 8)), mass, kw

    def frequency_aggregate(self, want_grad=False):
        """(J_p, f_1 in Hz, dJ/dr_b or None) of the current design: J_p = (sum_i (omega_i^2)^-p)^(1/p) over the constraint's
        n_modes lowest natural frequencies (J_p >= 1 / omega_1^2).  dJ/dr_b is the device's weighted sum of the rows of
        pl_vibration_modes_sens; it needs no adjoint solve."""
        _, n_modes, p, mass, kw = self._frequency_settings()
        self.natural_frequencies(n_modes, **mass, **kw)
        out = self.natural_frequency_sensitivity(p, want_rows=False) if want_grad else None
        J = out["aggregate"] if want_grad else GH.load_factor_aggregate(self.vibration_omega2, p)[0]
        self._last_frequency = (J, float(self.natural_frequencies_hz[0]))
        return J, self._last_frequency[1], (out["dJ_dr"] if want_grad else None)

    def frequency_constraint(self, r):
        """(2 pi f_min)^2 J_p - 1 (<= 0 when feasible: J_p >= 1 / omega_1^2, so f_1 >= f_min then)."""
        return self._constraint_value("frequency", r)

    def frequency_constraint_gradient(self, r):
        """d(frequency_constraint)/d(theta): (2 pi f_min)^2 dJ/dr_b through _strut_gradient_to_parameters."""
        return self._constraint_gradient("frequency", r)

    # -- peak displacement constraint (FEM mode): p-norm over time of one output of the transient response, pl_transient_sens ------
    def _peak_displacement_settings(self):
        c = self.constraints_dict["peak_displacement"]
        run = dict(dt=float(c["dt"]), n_steps=int(c["n_steps"]), density=float(c["density"]), amplitude=c.get("amplitude", None),
                   base_acceleration=c.get("base_acceleration", None), damping=tuple(c.get("damping", (0.0, 0.0))),
                   rotary=bool(c.get("rotary", True)), node_mass=c.get("node_mass", None))
        kw = {k: c[k] for k in ("beta", "gamma", "rtol", "max_iter") if k in c}
        return float(c["max_displacement"]), run, kw, c.get("output", None), float(c.get("p", 8))

    def peak_displacement_aggregate(self):
        """(J_p, max_n |y_n|, dJ/dr_b) of the current design under the constraint's transient run: y_n = l . u_n the output of
        row n, J_p = (sum_n |y_n|^p)^(1/p) >= max_n |y_n|.  One pl_transient_sens call gives all three (the forward pass and
        the adjoint sweep); the value and the gradient of one design share it."""
        def run_once():
            _, run, kw, output, p = self._peak_displacement_settings()
            self._transient_settings = self._transient_setup("peak_displacement", kw=kw, **run)
            out = self.transient_sensitivity(output, kind=2, p=p)
            res = (out["J"], float(np.abs(out["y"]).max()), out["dJ_dr"])
            self._last_peak_displacement = res[:2]
            return res
        return self._cached_aggregate("_peak_cache", run_once)

    def peak_displacement_constraint(self, r):
        """J_p / max_displacement - 1 (<= 0 when feasible: J_p >= max_n |y_n|, so the peak stays below max_displacement then)."""
        return self._constraint_value("peak_displacement", r)

    def peak_displacement_constraint_gradient(self, r):
        """d(peak_displacement_constraint)/d(theta): dJ/dr_b / max_displacement through _strut_gradient_to_parameters."""
        return self._constraint_gradient("peak_displacement", r)

    # -- resonance peak constraint (FEM mode): p-norm over a band of one output of the frequency response, pl_harmonic_sens ---------
    def _resonance_peak_settings(self):
        c = self.constraints_dict["resonance_peak"]
        run = dict(frequencies_hz=np.asarray(c["frequencies_hz"], float).reshape(-1), density=float(c["density"]),
                   damping=tuple(c.get("damping", (0.0, 0.0))), base_acceleration=c.get("base_acceleration", None),
                   rotary=bool(c.get("rotary", True)), node_mass=c.get("node_mass", None))
        kw = {k: c[k] for k in ("rtol", "max_iter") if k in c}
        return float(c["max_amplitude"]), run, kw, c.get("output", None), float(c.get("p", 8))

    def resonance_peak_aggregate(self):
        """(J_p, max_k |y_k|, dJ/dr_b) of the current design over the constraint's frequencies: y_k = l^T u_k the output at
        frequency k, J_p = (sum_k |y_k|^p)^(1/p) >= max_k |y_k|.  One pl_harmonic_sens call gives all three (the fields and
        the adjoint fields in the same passes); the value and the gradient of one design share it."""
        def run_once():
            _, run, kw, output, p = self._resonance_peak_settings()
            self._dynamics_guard("resonance_peak")
            self._frf_settings = self._frf_setup(kw=kw, **run)
            out = self.frequency_response_sensitivity(output, kind=2, p=p)
            res = (out["J"], float(np.abs(out["y"]).max()), out["dJ_dr"])
            self._last_resonance_peak = res[:2]
            return res
        return self._cached_aggregate("_resonance_cache", run_once)

    def resonance_peak_constraint(self, r):
        """J_p / max_amplitude - 1 (<= 0 when feasible: J_p >= max_k |y_k|, so the peak stays below max_amplitude then)."""
        return self._constraint_value("resonance_peak", r)

    def resonance_peak_constraint_gradient(self, r):
        """d(resonance_peak_constraint)/d(theta): dJ/dr_b / max_amplitude through _strut_gradient_to_parameters."""
        return self._constraint_gradient("resonance_peak", r)

    # -- driver (SciPy SLSQP, as the reference) ---------------------------------------------------------------------
    def _initialize_optimization_solver(self):
        from scipy.optimize import Bounds
        lo, hi = (0.0, 1.0) if self.enable_normalization else (self.min_radius, self.max_radius)
        t = self.optimization_parameters["type"]
        init = float(np.mean(self.normalize_optimization_parameters(self.radii)))
        if t == "linear":
            self.bounds = Bounds(lb=[-1.0] * (self.number_parameters - 1) + [lo],
                                 ub=[1.0] * (self.number_parameters - 1) + [hi])
            self.initial_parameters = [0.0] * (self.number_parameters - 1) + [init]
        else:
            self.bounds = Bounds(lb=[lo] * self.number_parameters, ub=[hi] * self.number_parameters)
            if t == "constant" and self.optimization_parameters.get("hybrid", False):
                self.initial_parameters = self.normalize_optimization_parameters(self.radii)
            else:
                self.initial_parameters = [init] * self.number_parameters

    def callback_function(self, r):
        self._opt_iteration = getattr(self, "_opt_iteration", 0) + 1   # (solve_DDM keeps its CG count in .iteration)
        self.iteration = self._opt_iteration
        self._history["iteration"].append(self.iteration)
        self._history["objective_norm"].append(self.actual_objective)
        self._history["objective"].append(self.denorm_objective)
        self._history["relative_density"].append(self.relative_density())
        for c in _RESPONSE_CONSTRAINTS:
            if c.history in self._history:
                last = getattr(self, "_last_" + c.stem)
                self._history[c.history].append(None if last is None else last[1])
        self._history["parameters"].append(list(map(float, r)))
        self._history["timestamp"].append(time.time())

    def optimize_lattice(self):
        from scipy.optimize import NonlinearConstraint, minimize
        self.initial_value_objective = None
        self.iteration = 0
        self._opt_iteration = 0
        self._sim_is_current = False
        self.actual_optimization_parameters = []
        self._initialize_optimization_solver()
        self.constraints = []
        if "relative_density" in self.constraints_dict:
            mode = self.constraints_dict["relative_density"].get("mode", "upper")
            lb, ub = {"upper": (-np.inf, 0.0), "lower": (0.0, np.inf), "eq": (0.0, 0.0)}.get(mode, (-np.inf, 0.0))
            self.constraints.append(NonlinearConstraint(self.density_constraint, lb, ub))
        for c in _RESPONSE_CONSTRAINTS:
            if c.key in self.constraints_dict:
                jac = {"jac": getattr(self, c.stem + "_constraint_gradient")} if self.enable_gradient_computing else {}
                self.constraints.append(NonlinearConstraint(getattr(self, c.stem + "_constraint"), -np.inf, 0.0, **jac))
        kw = dict(fun=self.objective, x0=self.initial_parameters, method="SLSQP", bounds=self.bounds,
                  constraints=self.constraints, callback=self.callback_function,
                  options={"maxiter": self.optim_max_iteration, "ftol": self.optim_ftol, "disp": self.optim_disp,
                           "eps": self.optim_eps})
        if self.enable_gradient_computing:
            kw["jac"] = self.gradient
        self.solution = minimize(**kw)
        self.set_optimization_parameters(self.solution.x)
        return self.solution
