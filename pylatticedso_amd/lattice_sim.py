"""Host-side mirror of the reference's ``LatticeSim`` for the FEM hot path, backed by arrays.

Mirrors (same names, argument meaning and error behaviour) the parts of
``src/pyLatticeSim/lattice_sim.py`` and ``src/pyLatticeDesign/lattice.py`` that feed
``solve_FEM_FenicsX``: preset parsing (lattice.py:212-311, lattice_sim.py:201-238), joint penalisation
(lattice_sim.py:245-308), boundary conditions (lattice_sim.py:405-494, lattice.py:1320-1411) and the
``xsol`` packing (lattice_sim.py:502-542).  Node data live in (N,6) arrays instead of ``Point`` lists:

    fixed_DOF, displacement_vector, applied_force, reaction_force_vector, index_boundary

Struts shared by several cells (lattices with struts in cell faces or on cell edges: Octet, Cubic, Kelvin, Auxetic ...):
the reference splits such a strut once PER OWNER CELL (lattice_sim.py:250-303) and keeps every copy, gives the
penalisation points lying in a cell face a boundary index, boundary conditions and a place in ``xsol``
(lattice_sim.py:405-458,502-563).  Two models are offered:

* ``reference_compat=False`` (default): every strut is penalised exactly once and only design nodes carry boundary
  data - the physical lattice;
* ``reference_compat=True`` (or environment ``PYLATTICE_REFERENCE_COMPAT=1``): the reference's own state - strut
  multiplicity = number of owner cells, every per-node array has one row per REFERENCE node (design nodes, then
  penalisation points, in the reference's index order), boundary data and ``xsol`` entries on penalisation points.
  Bit-exact against the states dumped from the running reference for all 29 golden lattices; the solve treats the
  copies of a strut as parallel chains between the same points (see ``compat_device.py`` for the one thing that cannot
  be pinned here: what the reference's gmsh model makes of them).
"""
from __future__ import annotations

import json
import os
from pathlib import Path

import numpy as np

from . import lattice_arrays as LA
from .timing import timing
from .views import LatticeViews

DDM_DENSE_MAX = 16384      # PL_DDM_DENSE_MAX of include/pylattice_hip.h
DDM_LARGE_PRECOND = 4       # above it: 4 = node blocks + dense level on node aggregates (3 = the node blocks alone)
DDM_COARSE_MAX_DOFS = 0     # size of that dense level (pl_opts_t.coarse_max_dofs; 0 = the library's default, 1 536)
# device_model(): lattice sizes from which the handle is asked for the multi-level preconditioner + record palette, and for
# fp32-stored PCG vectors with fp64 refinement (measured crossovers, DESIGN.md sections 7 / 7a)
MULTILEVEL_MIN_NODES = 600
DIRECT_MAX_NODES = 200        # up to here: dense factorisation of K as the preconditioner (opts.precond = 5), see device_model
SMALL_TILES_MAX_NODES = 5000  # multi-level PCG below this size: 32-node tiles and 12-mode dense level
FP32_VECTORS_MIN_NODES = 2_000_000

_ROOT = Path(__file__).resolve().parents[1]
PRESET_DIR = _ROOT / "data" / "inputs" / "preset_lattice"

# E, nu of the reference's material cards (src/pyLatticeDesign/materials/*.json)
MATERIALS = {"VeroClear": (1013.0, 0.3), "TPU": (20000.0, 0.3), "Ti-6Al-4V": (104000.0, 0.35)}
_SURFACES = ["Xmin", "Xmax", "Ymin", "Ymax", "Zmin", "Zmax", "Xmid", "Ymid", "Zmid"]
_DOF_MAP = {"X": 0, "Y": 1, "Z": 2, "RX": 3, "RY": 4, "RZ": 5}


def open_lattice_parameters(file_name):
    """utils.open_lattice_parameters (utils.py:111-130): preset name relative to data/inputs/preset_lattice,
    or an absolute path; '.json' appended when missing.  A dict is passed through (extension)."""
    if isinstance(file_name, dict):
        return file_name
    json_path = PRESET_DIR / file_name
    if json_path.suffix != ".json":
        json_path = json_path.with_suffix(".json")
    try:
        with open(json_path, "r") as fh:
            return json.load(fh)
    except FileNotFoundError:
        raise FileNotFoundError(f"The file {json_path} does not exist.")


def material_properties(name):
    if name in MATERIALS:
        return MATERIALS[name]
    p = os.environ.get("PYLATTICE_MATERIAL_PATH")
    if p and os.path.exists(os.path.join(p, f"{name}.json")):
        with open(os.path.join(p, f"{name}.json")) as fh:
            d = json.load(fh)
        return float(d["Young_modulus"]), float(d["Poisson_ratio"])
    raise FileNotFoundError(f"Material file not found: {name}.json")


class LatticeSim(LatticeViews):
    _design_mult_note_done = False      # the "strut copies" warning is given once per process

    def __init__(self, name_file, mesh_trimmer=None, verbose: int = 0,
                 enable_domain_decomposition_solver: bool = False, data_roots=None, reference_compat=None,
                 ddm_gradient="finite_difference"):
        """Same arguments as the reference (lattice_sim.py:44-47) plus ``data_roots``: extra directories in which the
        reduced-basis files of the surrogate DDM modes are looked up (the reference finds them in its own checkout),
        ``reference_compat`` (module docstring; None = environment PYLATTICE_REFERENCE_COMPAT, else False) and
        ``ddm_gradient``: what the exact branch of calculate_schur_complement_cells builds when
        ``enable_gradient_computing`` is on - "finite_difference": the central differences dS/dr of every representative
        (the reference's way); "analytic": nothing beyond the matrices, the sensitivities come from
        recover_cell_interiors (LatticeOpti)."""
        if ddm_gradient not in ("finite_difference", "analytic"):
            raise ValueError('ddm_gradient must be "finite_difference" or "analytic"')
        self.ddm_gradient = ddm_gradient
        if mesh_trimmer is not None:
            raise NotImplementedError("mesh_trimmer is outside the accelerated path")
        if reference_compat is None:
            reference_compat = os.environ.get("PYLATTICE_REFERENCE_COMPAT", "0") not in ("", "0")
        self.reference_compat = bool(reference_compat)
        self._verbose = verbose
        self.data_roots = list(data_roots or [])
        self.used_schur_preconditioner = None
        self._ddm_precond = 0
        self.domain_decomposition_solver = enable_domain_decomposition_solver
        self.n_DOF_per_node = 6
        self.penalization_coefficient = LA.PENALIZATION_COEFFICIENT
        self.is_penalized = False
        params = open_lattice_parameters(name_file)
        self._extract_geometry(params)
        self.define_simulation_parameters(params)
        self._base_radii = [float(r) for r in self.radii]
        self._cell_radii_override = None
        self._device = self._ddm_device = None
        self.thermal = None                        # (alpha, delta_T, beam_alpha) of set_temperature, None without one
        self.conduction = None                     # the conduction problem of solve_temperature, None without one
        self.temperature_field = None              # (n_nodes,) T of its last solve
        self.temperature_history = None            # the dict of the last transient_temperature
        self._generate_and_prepare()
        if self._conduction_preset is not None:    # simulation_parameters["thermal"]["conduction"]
            c = self._conduction_preset
            self._set_conduction_problem(c["conductivity"], c.get("Temperature", None), c.get("HeatFlow", None),
                                         c.get("beam_conductivity", None), c.get("reference", 0.0), c.get("Convection", None))
        if self._thermal_preset is not None:       # simulation_parameters["thermal"]
            self.set_temperature(*self._thermal_preset)
        self.cell_schur_index = None       # (C,) index into self.schur_complements
        self.schur_complements = None      # (n_S, 6 n_b, 6 n_b)
        self.iteration = 0
        self.enable_gradient_computing = False     # lattice_sim.py:114: also keep dS/dr per unique cell
        self.schur_gradients = None                # [n_S] lists of dS/dr_j
        self._schur_cell_data = None               # [n_S] strut data every exact cell matrix was condensed from
        self.schur_surrogate = None
        if self.domain_decomposition_solver:
            if self.type_schur_complement_computation == "FE2":
                raise NotImplementedError("FE2 Schur complements are outside the accelerated path")
            if self.type_schur_complement_computation != "exact":
                # reduced basis + surrogate for its coefficients (lattice_sim.py:126-135); the .npz is looked up
                # like the reference does, below <root>/data/outputs/schur_complement/reduced_basis/
                from .schur_surrogate import SchurSurrogate
                self.schur_surrogate = SchurSurrogate.load(self.geom_types, self.precision_greedy,
                                                           self.type_schur_complement_computation,
                                                           search_dirs=data_roots)
                self.reduce_basis_dict = {"basis_reduced_ortho": self.schur_surrogate.basis,
                                          "alpha_ortho": self.schur_surrogate.alpha_train.T,
                                          "list_elements": self.schur_surrogate.points}
                self.alpha_coefficients_greedy = self.schur_surrogate.alpha_train
                self.shape_schur_complement = self.schur_surrogate.n
            if self.enable_preconditioner and self.preconditioner_type not in ("mean", "nearest_reference", "exact"):
                raise NotImplementedError("Not implemented preconditioner approximation method.")   # lattice_sim.py:1323
            self.calculate_schur_complement_cells()

    # ------------------------------------------------------------------------------------------------
    def _extract_geometry(self, p):
        geometry = p.get("geometry", {})
        cs, nc = geometry.get("cell_size", {}), geometry.get("number_of_cells", {})
        self.cell_size_x, self.cell_size_y, self.cell_size_z = cs.get("x"), cs.get("y"), cs.get("z")
        self.num_cells_x, self.num_cells_y, self.num_cells_z = nc.get("x"), nc.get("y"), nc.get("z")
        self.radii = geometry.get("radii")
        self.geom_types = geometry.get("geom_types")
        if None in [self.cell_size_x, self.cell_size_y, self.cell_size_z, self.num_cells_x, self.num_cells_y,
                    self.num_cells_z, self.radii, self.geom_types]:
            raise ValueError("Missing geometry parameters in JSON file.")
        # lattice.py:236-238
        self.enable_randomness = bool(geometry.get("enable_randomness", False))
        self.range_radius = geometry.get("range_radius", [0.01, 0.1])
        self.randomness_hybrid = bool(geometry.get("randomness_hybrid", False))
        grad = p.get("gradient", {})

        def table(block, keys):
            if not block:
                return None
            return LA.gradient_table(self.num_cells_x, self.num_cells_y, self.num_cells_z,
                                     block.get("rule", "constant"),
                                     [block.get(f"direction_{a}", False) for a in "xyz"],
                                     [block.get(f"parameter_{a}", 0.0) for a in "xyz"])

        self.grad_radius = table(grad.get("radii", {}), None)
        self.grad_dim = table(grad.get("cell_dimension", {}), None)
        sup = p.get("supplementary", {})
        blocks = []
        for blk in sup.get("erased_blocks", {}).values():
            s, d = blk.get("start_point", {}), blk.get("dimensions_block", {})
            blocks.append([s.get("x", 0.0), s.get("y", 0.0), s.get("z", 0.0), d.get("x", 0.0), d.get("y", 0.0),
                           d.get("z", 0.0)])
        self.eraser_blocks = blocks or None
        self.symmetry_lattice = None                    # lattice.py:294-303
        sym = sup.get("symmetries", {})
        if sym:
            pt = sym.get("reference_point", {})
            self.symmetry_lattice = {"sym_plane": sym.get("plane", None),
                                     "sym_point": (pt.get("x", 0.0), pt.get("y", 0.0), pt.get("z", 0.0))}

    def define_simulation_parameters(self, name_file):
        """lattice_sim.py:201-238."""
        p = open_lattice_parameters(name_file)
        sim = p.get("simulation_parameters", {})
        self.enable_simulation_properties = bool(sim.get("enable", False))
        self.material_name = sim.get("material", "VeroClear")
        self.enable_periodicity = sim.get("periodicity", False)
        ddm = sim.get("DDM", None)
        self.enable_preconditioner = None
        self.preconditioner_type = None
        self.number_iteration_max = None
        self.type_schur_complement_computation = None
        self.precision_greedy = None
        if ddm is not None:
            self.enable_preconditioner = ddm.get("enable_preconditioner", False)
            self.preconditioner_type = ddm.get("preconditioner_type", None)
            if self.preconditioner_type is None and self.enable_preconditioner:
                raise ValueError("Preconditioner type must be defined in the input file.")
            self.number_iteration_max = ddm.get("max_iterations", 1000)
            comp = ddm.get("schur_complement_computation", None)
            if comp is None:
                raise ValueError("Schur complement computation method must be defined in the input file.")
            self.type_schur_complement_computation = comp.get("type", None)
            if self.type_schur_complement_computation not in ["exact", "FE2"]:
                self.precision_greedy = comp.get("precision_greedy", None)
                if self.precision_greedy is None:
                    raise ValueError("Precision for greedy algorithm must be defined in the input file.")
        elif self.domain_decomposition_solver:
            raise ValueError("Schur complement computation method must be defined in the input file.")
        self.boundary_conditions = p.get("boundary_conditions", {})
        th = sim.get("thermal", None)              # {"alpha": a, "delta_T": scalar}: a uniform temperature rise
        self._thermal_preset = self._conduction_preset = None
        if th is not None and th.get("conduction", None) is not None:
            # {"alpha": a, "conduction": {"conductivity", "reference", "Temperature": {...}, "HeatFlow": {...}}}: the
            # temperature is the solution of the conduction problem on the struts (solve_temperature)
            if self.domain_decomposition_solver:
                raise ValueError('the "conduction" block needs simulation_type "FEM": DDM handles carry no strut graph')
            self._conduction_preset = dict(th["conduction"])
            self._thermal_preset = ("conduction", float(th["alpha"]))
        elif th is not None:
            self._thermal_preset = (float(th["delta_T"]), float(th["alpha"]))
        self.young_modulus, self.poisson_ratio = material_properties(self.material_name)

    # ------------------------------------------------------------------------------------------------
    @timing.category("simulation")
    @timing.timeit
    def reset_cell_with_new_radii(self, new_radii, index_cell: int = 0):
        """lattice_sim.py:1421-1497: give one cell new base radii and redo everything that depends on them - the
        struts of that cell, the penalisation lengths (L_zone depends on the neighbours' radii), boundary indices and
        boundary conditions.  Array-backed: the lattice is regenerated with a per-cell radius override."""
        if len(new_radii) != len(self.radii):
            raise ValueError("Invalid hybrid radii data.")
        if not (0 <= index_cell < self.lattice.n_cells):
            raise IndexError("Invalid cell index.")
        self.radii = [float(r) for r in new_radii]
        if getattr(self, "_cell_radii_override", None) is None:
            self._cell_radii_override = np.tile(np.asarray(self._base_radii, dtype=float), (self.lattice.n_cells, 1))
        self._cell_radii_override[index_cell] = self.radii
        self._generate_and_prepare()

    @timing.category("simulation")
    @timing.timeit
    def set_cell_radii(self, radii):
        """Give every cell its own radii, (C, n_geometries) in the cell order of ``lattice.cell_pos`` - what a loop of
        ``Cell.change_beam_radius`` (cell.py:896-917) does in the reference (LatticeOpti works this way).  The lattice
        arrays are regenerated once; in DDM mode the cell Schur complements are re-evaluated."""
        radii = np.asarray(radii, dtype=float).reshape(self.lattice.n_cells, len(self._base_radii))
        self._cell_radii_override = radii.copy()
        self._generate_and_prepare()
        if self.domain_decomposition_solver:
            self.calculate_schur_complement_cells()

    @timing.category("design")
    @timing.timeit
    def _generate_and_prepare(self):
        """Lattice arrays + penalisation + boundary indices + boundary conditions from the current parameters."""
        for dev in (getattr(self, "_device", None), getattr(self, "_ddm_device", None)):
            if dev is not None:
                dev.close()
        self._device = self._ddm_device = None
        if self.enable_randomness and self._cell_radii_override is None:
            # lattice.py:458-465: every cell draws its radii from the reference's seeded stream.  The position in that
            # stream depends on how many points the earlier cells created (LA.random_cell_radii): a geometry-only pass
            # first, then the lattice with those radii
            geo = LA.generate((self.cell_size_x, self.cell_size_y, self.cell_size_z),
                              (self.num_cells_x, self.num_cells_y, self.num_cells_z), self.geom_types,
                              self._base_radii, grad_radius=self.grad_radius, grad_dim=self.grad_dim,
                              erased_blocks=self.eraser_blocks, want_creator=True)
            self._cell_gfac = geo.cell_radii[:, 0] / self._base_radii[0]
            self._cell_radii_override = LA.random_cell_radii(geo.extras["node_creator"], geo.n_cells,
                                                             len(self._base_radii), self.range_radius,
                                                             self.randomness_hybrid)
        self.__dict__.pop("_surface_points_cache", None)      # (tables derived from the old topology)
        self.__dict__.pop("_gdi_cache", None)
        self.lattice = LA.generate((self.cell_size_x, self.cell_size_y, self.cell_size_z),
                                   (self.num_cells_x, self.num_cells_y, self.num_cells_z), self.geom_types,
                                   self._base_radii, grad_radius=self.grad_radius, grad_dim=self.grad_dim,
                                   erased_blocks=self.eraser_blocks,
                                   cell_radii_override=(None if self._cell_radii_override is None else
                                                        self._cell_radii_override * self._cell_gfac[:, None]))
        if self._cell_radii_override is None:      # gradient factor of Cell.get_radius (cell.py:385-412), per cell
            self._cell_gfac = self.lattice.cell_radii[:, 0] / self._base_radii[0]
        if self.symmetry_lattice is not None:      # lattice.py:90-91
            plane, point = self.symmetry_lattice["sym_plane"], self.symmetry_lattice["sym_point"]
            if plane is None or point is None:
                raise ValueError("Both symmetry_plane and reference_point must be provided.")
            self.lattice = LA.apply_symmetry(self.lattice, self.geom_types, plane, point)
            if len(self._cell_gfac) != self.lattice.n_cells:
                self._cell_gfac = np.concatenate([self._cell_gfac, self._cell_gfac])
        lat = self.lattice
        self.x_min, self.x_max, self.y_min, self.y_max, self.z_min, self.z_max = map(float, lat.bbox)
        self.penalized = None
        self.is_penalized = False
        self.beam_mult = None
        # lattice_sim.py:119-122: joints are penalised for the FEM path and for DDM with exact Schur complements;
        # with a surrogate the penalisation lives inside the stored Schur matrices
        if self.enable_simulation_properties and (not self.domain_decomposition_solver
                                                  or self.type_schur_complement_computation == "exact"):
            self.define_angles_between_beams()
            self.set_penalized_beams()
        else:
            self.lzone = np.zeros((lat.n_beams, 2))
            self.penalized = LA.penalize(lat, None)
        # rows of the per-node arrays: the design nodes; in reference_compat mode the reference's whole node list
        # (design nodes, then the penalisation points in coordinate order = Point.index, lattice.py:687-696)
        self._compat_rows = self.reference_compat and self.is_penalized
        if self._compat_rows:
            self._define_strut_multiplicity()
        # Struts the reference would hold several copies of at DESIGN level (hybrid collision on a strut shared by several
        # cells, apply_symmetry twins): the default model keeps each once - say so once, and leave a flag on the object
        dm = lat.extras.get("design_mult")
        self.differs_from_reference_by_strut_copies = bool(dm is not None and (np.asarray(dm) > 1).any()
                                                           and not self.reference_compat)
        if self.differs_from_reference_by_strut_copies and not LatticeSim._design_mult_note_done:
            LatticeSim._design_mult_note_done = True
            import warnings
            warnings.warn(f"{int((np.asarray(dm) > 1).sum())} struts of this lattice exist in several copies in the reference's "
                          "model (hybrid collision on struts shared by several cells / symmetry twins); the default "
                          "LatticeSim keeps each strut once.  Pass reference_compat=True (or PYLATTICE_REFERENCE_COMPAT=1) "
                          "for the reference's own model (INTEGRATION.md).", stacklevel=2)
        R = self.get_number_nodes() if self._compat_rows else lat.n_nodes
        self.fixed_DOF = np.zeros((R, 6), dtype=bool)
        self.displacement_vector = np.zeros((R, 6))
        self.applied_force = np.zeros((R, 6))
        self.reaction_force_vector = np.zeros((R, 6))
        self._cell_points = None
        self.define_node_index_boundary()
        self.set_boundary_conditions()

    def get_number_cells(self):
        return self.lattice.n_cells

    def get_lattice_boundary_box(self):
        return [self.x_min, self.x_max, self.y_min, self.y_max, self.z_min, self.z_max]

    # ------------------------------------------------------------------------------------------------
    @timing.category("design")
    @timing.timeit
    def define_angles_between_beams(self):
        """lattice.py:805-904.  Large non-periodic lattices take the device kernel (pl_lzone: the valence^2 angle search
        is 10^7-10^8 pair evaluations at 10^6 struts); small ones and periodic single cells the numpy restatement."""
        if not self.enable_periodicity and self.lattice.n_nodes >= 20000:
            from ._capi import lzone
            self.lzone = lzone(self.lattice.node_xyz, self.lattice.beam_conn, self.lattice.beam_radius)
        else:
            self.lzone = LA.compute_lzone(self.lattice, bool(self.enable_periodicity))

    @timing.category("simulation")
    @timing.timeit
    def set_penalized_beams(self):
        self.penalized = LA.penalize(self.lattice, self.lzone)
        self.is_penalized = True

    def _define_strut_multiplicity(self):
        """reference_compat: how many copies of every strut the reference's model holds.  set_penalized_beams loops
        ``for cell: for beam in cell.beams_cell`` and replaces a strut with a penalised end by NEW segment objects in that
        cell only (lattice_sim.py:250-303), so a strut shared by k cells ends up as k copies of each segment; a strut
        without penalised ends stays one shared object.  (Copies made by check_hybrid_collision come on top:
        ``lattice.extras["design_mult"]``.)"""
        lat, pen = self.lattice, self.penalized
        owners = np.bincount(lat.cell_beam_idx, minlength=lat.n_beams)
        split = (pen.seg_len[:, 0] > 0) | (pen.seg_len[:, 2] > 0)
        mult = np.where(split, owners, 1).astype(np.int64)
        dm = lat.extras.get("design_mult")
        if dm is not None and lat.extras.get("design_mult_kind") == "per_cell":
            # twins of apply_symmetry: every copy sits in one cell's beams_cell and is penalised there once - as many
            # segment copies as owner cells (counted by the cell -> strut table), dm objects when nothing is split
            mult = np.where(split, owners, dm)
        elif dm is not None:
            # every design copy is a separate object in every owner cell's beams_cell (lattice.py:1188-1195): each is
            # penalised once per owner cell
            mult = np.where(split, owners * dm, dm)
        self.beam_mult = mult

    def cell_points(self):
        """CSR cell -> rows of the per-node arrays: ``Cell.points_cell`` of the reference.  Design nodes of the cell; in
        reference_compat mode also the penalisation points of the cell's struts (cell.add_point, lattice_sim.py:301)."""
        if self._cell_points is None:
            lat = self.lattice
            if not self._compat_rows:
                self._cell_points = (lat.cell_node_ptr, lat.cell_node_idx)
            else:
                from .views import _tables
                t = _tables(self)
                cell_of_b = np.repeat(np.arange(lat.n_cells), np.diff(lat.cell_beam_ptr))
                pens = t.pen_id[lat.cell_beam_idx]                    # (n_pairs, 2)
                ok = pens >= 0
                rows = np.concatenate([np.repeat(np.arange(lat.n_cells), np.diff(lat.cell_node_ptr)),
                                       np.repeat(cell_of_b, 2).reshape(-1, 2)[ok]])
                cols = np.concatenate([lat.cell_node_idx, pens[ok]])
                self._cell_points = LA._csr_from_pairs(rows, cols, lat.n_cells)
        return self._cell_points

    def node_coordinates(self):
        """(rows, 3) coordinates of the rows of the per-node arrays."""
        if self._compat_rows:
            from .views import _tables
            return _tables(self).node_xyz
        return self.lattice.node_xyz

    def reset_penalized_beams(self) -> None:
        """lattice_sim.py:313-400: undo set_penalized_beams - every strut is one segment again, the penalisation points
        go away (the design struts and nodes were never replaced here, so nothing has to be rewired); a device handle
        built for the penalised model is dropped."""
        if not self.is_penalized:
            print("Warning: lattice does not appear to be penalized.")
            return
        self.lzone = np.zeros((self.lattice.n_beams, 2))
        self.penalized = LA.penalize(self.lattice, None)
        self.is_penalized = False
        if self._device is not None:
            self._device.close()
            self._device = None
        for name in ("_view_tables", "_node_mod_store"):
            if hasattr(self, name):
                delattr(self, name)

    @timing.category("simulation")
    @timing.timeit
    def define_node_index_boundary(self):
        """Boundary index of every node lying on the box of one of its cells (lattice_sim.py:546-563), numbered in
        the order get_global_displacement visits them (cells in order, nodes by rounded coordinates)."""
        lat = self.lattice
        ptr, idx = self.cell_points()
        node_xyz = self.node_coordinates()
        N = len(node_xyz)
        if N >= 20000:   # large lattices: the same rule in multi-threaded C++ (pl_boundary_index / pl_boundary_index_rows)
            from ._capi import boundary_index
            self.index_boundary, visit = boundary_index(ptr, idx, node_xyz, lat.cell_coord, lat.cell_size,
                                                        by_coordinates=bool(self._compat_rows))
            self.max_index_boundary = len(visit) - 1
            self._boundary_visit_order = visit
            return
        self.index_boundary = np.full(N, -1, np.int64)
        on_box = np.zeros(N, bool)
        cell_of = np.repeat(np.arange(lat.n_cells), np.diff(ptr))
        xyz = node_xyz[idx]
        lo, hi = lat.cell_coord[cell_of], lat.cell_coord[cell_of] + lat.cell_size[cell_of]
        on = ((xyz == lo) | (xyz == hi)).any(axis=1)
        on_box[idx[on]] = True
        # visit order: cell-major, then (round(x,9), round(y,9), round(z,9), index); node index already sorts by xyz
        inside = np.ones(len(idx), bool)
        inside[ptr[1:-1]] = False                           # first entry of every cell but the first
        if self._compat_rows:
            # rows inside a cell come in (round(x, 9), round(y, 9), round(z, 9), index) order (_sorted_nodes,
            # lattice_sim.py:193-199): design nodes and penalisation points interleave
            key = np.round(xyz, 9)
            idx = idx[np.lexsort((idx, key[:, 2], key[:, 1], key[:, 0], cell_of))]
        elif len(idx) > 1 and not np.all((np.diff(idx) > 0) | ~inside[1:]):
            idx = idx[np.lexsort((idx, cell_of))]           # rows not yet ascending inside their cell
        seq = idx[on_box[idx]]
        # first visit of every node, without sorting: of duplicate targets of a fancy assignment the last one written
        # stays, so writing the positions in reverse leaves the first one
        pos = np.arange(len(seq))
        first = np.full(N, -1, np.int64)
        first[seq[::-1]] = pos[::-1]
        visit = seq[first[seq] == pos]
        self.index_boundary[visit] = np.arange(len(visit))
        self.max_index_boundary = len(visit) - 1
        self._boundary_visit_order = visit

    # ------------------------------------------------------------------------------------------------
    def get_cells_on_surfaces(self, surfaces):
        """lattice.py:1363-1411: iterative extrema filter on the integer cell positions."""
        pos = self.lattice.cell_pos
        cand = np.arange(len(pos))
        for token in surfaces:
            t = token.strip().lower()
            if not t:
                continue
            ax = {"x": 0, "y": 1, "z": 2}.get(t[0])
            if ax is None:
                raise ValueError(f"Invalid axis in constraint '{token}', expected X/Y/Z with min/max.")
            if "min" in t:
                ext = pos[cand, ax].min()
            elif "max" in t:
                ext = pos[cand, ax].max()
            else:
                raise ValueError(f"Invalid extrema in constraint '{token}', expected 'min' or 'max'.")
            cand = cand[pos[cand, ax] == ext]
            if len(cand) == 0:
                return cand
        return cand

    def find_point_on_lattice_surface(self, surfaceNames, surface_cells=None):
        """Node ids on the given surfaces (lattice.py:1320-1359)."""
        if not all(s in _SURFACES for s in surfaceNames):
            raise ValueError("Invalid surface name_lattice(s).")
        lat = self.lattice
        # (the node sets of a lattice's surfaces do not change while its topology stands: an optimisation re-applies the same
        #  boundary conditions before every simulation - 4.5 ms of an 18-ms objective + gradient at 24^3 cells went here)
        cache = self.__dict__.setdefault("_surface_points_cache", {})
        ckey = (id(lat), lat.n_nodes, tuple(surfaceNames), None if surface_cells is None else tuple(surface_cells))
        if ckey in cache:
            return cache[ckey].copy()
        cells = self.get_cells_on_surfaces(surfaceNames)
        names = surface_cells if surface_cells is not None else surfaceNames
        ptr, idx = self.cell_points()
        node_xyz = self.node_coordinates()
        # every (surface cell, point of that cell) pair at once (a Python loop over the cells cost 0.1 s at 50^3 cells)
        cells = np.asarray(cells, dtype=np.int64)
        if len(cells):
            cnt = (ptr[cells + 1] - ptr[cells]).astype(np.int64)
            owner = np.repeat(np.arange(len(cells)), cnt)
            first = np.repeat(np.asarray(ptr)[cells].astype(np.int64) - np.concatenate(([0], np.cumsum(cnt)[:-1])), cnt)
            nodes = np.asarray(idx)[first + np.arange(int(cnt.sum()))]
            keep = np.ones(len(nodes), bool)
            for s in names:
                ax = "XYZ".index(s[0])
                val = lat.cell_coord[cells, ax] + (lat.cell_size[cells, ax] if s.endswith("max") else 0.0)
                # (min and mid both refer to the cell's lower corner, cell.py:451-462)
                keep &= node_xyz[nodes, ax] == val[owner]
            pts = np.unique(nodes[keep])
        else:
            pts = np.zeros(0, np.int64)
        if len(pts) == 0:
            raise ValueError("No points found on the specified surfaces.")
        cache[ckey] = pts
        return pts.copy()

    def apply_constraints_nodes(self, surfaces, value, DOF, type_constraint="Displacement", surface_cells=None):
        """lattice_sim.py:405-458: displacement -> value + fixed flag; force -> total / number of target nodes
        whose dof is free."""
        pts = self.find_point_on_lattice_surface(surfaces, surface_cells)
        pts = pts[self.index_boundary[pts] >= 0]
        if len(pts) == 0:
            raise ValueError("No nodes found on the specified surfaces for constraint application.")
        targets = {d: int((~self.fixed_DOF[pts, d]).sum()) for d in DOF}
        for val, d in zip(value, DOF):
            if type_constraint == "Displacement":
                self.displacement_vector[pts, d] = val
                self.fixed_DOF[pts, d] = True
            elif type_constraint == "Force":
                self.applied_force[pts, d] = val / max(1, targets[d])
            else:
                raise ValueError("Invalid type of constraint. Use 'Displacement' or 'Force'.")

    @timing.category("simulation")
    @timing.timeit
    def set_boundary_conditions(self):
        """lattice_sim.py:460-494."""
        for key, block in self.boundary_conditions.items():
            if key not in ["Force", "Displacement"]:
                raise ValueError(f"Invalid boundary condition type: {key}. Must be 'Force' or 'Displacement'.")
            for _name, data in block.items():
                if "Surface" not in data or "Value" not in data or "DOF" not in data:
                    raise ValueError("Invalid boundary condition data. 'Surface', 'Value' and 'DOF' are required.")
                if not isinstance(data["Surface"], list):
                    raise ValueError("Surface must be a list of strings.")
                if not isinstance(data["Value"], list):
                    raise ValueError("Value must be a list of floats.")
                if not isinstance(data["DOF"], list):
                    raise ValueError("DOF must be a list of strings.")
                if len(data["Value"]) != len(data["DOF"]):
                    raise ValueError("Value and DOF must have the same length.")
                if not all(d in _DOF_MAP for d in data["DOF"]):
                    raise ValueError("DOF must be one of 'X', 'Y', 'Z', 'RX', 'RY', 'RZ'.")
                if not all(s in _SURFACES for s in data["Surface"]):
                    raise ValueError("Surface must be one of 'Xmin', 'Xmax', 'Ymin', 'Ymax', 'Zmin', 'Zmax', "
                                     "'Xmid', 'Ymid', 'Zmid'.")
                self.apply_constraints_nodes(data["Surface"], data["Value"], [_DOF_MAP[d] for d in data["DOF"]],
                                             key, data.get("SurfaceCells", None))

    # ------------------------------------------------------------------------------------------------
    @timing.category("simulation")
    @timing.timeit
    def get_global_displacement(self, withFixed: bool = False, OnlyImposed: bool = False):
        """lattice_sim.py:502-542: free dofs of the cell-boundary nodes in visit order."""
        V = np.asarray(self._boundary_visit_order, dtype=np.int64)
        U, fixed = self.displacement_vector[V], self.fixed_DOF[V]
        idx6 = np.repeat(self.index_boundary[V].astype(np.int64)[:, None], 6, axis=1)
        if not OnlyImposed:                       # free dofs (+ the constrained ones if asked for), node-major
            take = ~fixed | bool(withFixed)
            disp, index = U[take], idx6[take]
        else:                                     # every dof: 0 for unloaded free ones (no index entry for those)
            silent = ~fixed & (self.applied_force[V] == 0)
            disp, index = np.where(silent, 0.0, U).ravel(), idx6[~silent]
        # a Python list, as in the reference, whatever the size (one type for every caller: `index + other`, `.index()`,
        # JSON ...; 3 M entries cost ~50 ms at 50^3 cells); the int64 array stays available beside it
        self.global_displacement_index_array = index if not OnlyImposed else getattr(self, "global_displacement_index_array", None)
        prev = getattr(self, "_gdi_cache", None)      # (the list only changes with the Dirichlet mask: a design loop asks
        if prev is not None and prev[0].shape == index.shape and np.array_equal(prev[0], index):   # for the same one again)
            index = list(prev[1])
        else:
            arr = index
            index = index.tolist()
            self._gdi_cache = (arr.copy(), list(index))
        if not OnlyImposed:
            self.global_displacement_index = index
        return np.asarray(disp, dtype=float), index

    # ------------------------------------------------------------------------------------------------
    def device_model(self, **kw):
        """The HIP handle for this lattice (created on first use; no CPU fallback)."""
        from ._capi import HipLattice
        if self._device is None:
            pen = self.penalized
            if self.lattice.n_nodes <= DIRECT_MAX_NODES:
                # the sizes of the reference's own presets (6x3x3 cells = 166 nodes): a slender cantilever of a few hundred nodes
                # needs 200 - 300 PCG iterations whatever the preconditioner (3.3 ms), the dense Cholesky factor of its ~1 000
                # dofs takes 16 launches; the PCG then converges in one or two steps (tools/experiments/small_lattice_precond.py)
                # (measured, profiles/r05_g_small_precond.txt: BCC 6x3x3 3.05 -> 1.66 ms per assembly + solve, 8x4x4 4.5 -> 3.2;
                # beyond ~350 nodes the factorisation chain of n / 64 links overtakes the PCG, and Octet lattices, which
                # converge in 60 - 100 iterations, are served better by the PCG from 300 nodes on)
                kw.setdefault("precond", 5)
            if self.lattice.n_nodes >= MULTILEVEL_MIN_NODES:
                # multi-level preconditioner + record palette (what bench.py measures).  Round 5: from 600 nodes instead of
                # 20 000 - with the short iteration (pl_small.h) and small tiles it beats Jacobi from there on (BCC 16x8x8:
                # 10.3 -> 5.2 ms, Octet 10x5x5 2.9 -> 1.8, 12^3 Octet 4.8 -> 2.1, 16^3 BCC 11.9 -> 5.8 ms per assembly + solve)
                kw.setdefault("precond", 3)
                kw.setdefault("palette", 1)
                if self.lattice.n_nodes < SMALL_TILES_MAX_NODES:
                    kw.setdefault("tile_nodes", 32)
                    kw.setdefault("coarse_modes", 12)
            if self.lattice.n_nodes >= FP32_VECTORS_MIN_NODES:
                # from ~2 M nodes the PCG vectors no longer fit the caches and stream from HBM: fp32 inner solves with fp64
                # refinement (rtol still refers to the TRUE fp64 residual).  Measured: 100^3 Octet 284 against 234 M
                # beams/s, 100^3 BCC 80.8 against 76.3; 50^3 Octet (0.77 M nodes) 220 against 230 - hence the threshold
                kw.setdefault("precision", 1)
            if self._compat_rows:
                from .compat_device import CompatDevice
                self._device = CompatDevice(self, **kw)
                return self._device
            self._device = HipLattice(self.lattice.node_xyz, self.lattice.beam_conn, self.lattice.beam_radius,
                                      pen.seg_len, pen.seg_nsub, self.young_modulus, self.poisson_ratio,
                                      pen_coef=self.penalization_coefficient, **kw)
        return self._device

    # -- temperature (FEM mode; pl_set_thermal) ------------------------------------------------
    def set_temperature(self, delta_T, alpha, beam_alpha=None):
        """Temperature rise of the nodes for the solves that follow: delta_T a scalar, an (n_nodes,) array, or a callable of the
        node coordinates (n_nodes, 3); alpha the expansion coefficient of every strut, or beam_alpha (n_beams,) per strut.  The
        temperature is linear along a strut and uniform over its section.  solve_FEM_FenicsX then solves K u = f_ext + f_th,
        the reactions are K u - f_th, and strut_stress / strut_buckling report the mechanical force; global_buckling and
        solve_DDM refuse while a temperature is set."""
        n = self.lattice.n_nodes
        ba = None if beam_alpha is None else np.array(np.broadcast_to(np.asarray(beam_alpha, dtype=float),
                                                                      (self.lattice.n_beams,)))
        if isinstance(delta_T, str):
            # delta_T = "conduction": T - reference of the conduction problem of solve_temperature (or of the preset's
            # "conduction" block), solved again before every mechanical solve so that it follows the radii
            if delta_T != "conduction":
                raise ValueError('set_temperature: delta_T must be a number, an array, a callable or "conduction"')
            if self.conduction is None:
                raise RuntimeError('set_temperature("conduction"): define the conduction problem first (solve_temperature)')
            if not (np.isfinite(alpha) and (ba is None or np.isfinite(ba).all())):
                raise ValueError("set_temperature: alpha and beam_alpha must be finite")
            self.thermal = (float(alpha), "conduction", ba)
            return
        dT = delta_T(np.asarray(self.lattice.node_xyz, dtype=float)) if callable(delta_T) else delta_T
        dT = np.array(np.broadcast_to(np.asarray(dT, dtype=float), (n,)))
        if not (np.isfinite(dT).all() and np.isfinite(alpha) and (ba is None or np.isfinite(ba).all())):
            raise ValueError("set_temperature: delta_T, alpha and beam_alpha must be finite")
        self.thermal = (float(alpha), dT, ba)
        if self._device is not None and not getattr(self, "_compat_rows", False):
            self._apply_temperature(self._device)

    def clear_temperature(self):
        """Removes the temperature of set_temperature (and of the preset's "thermal" block)."""
        self.thermal = None
        if self._device is not None and not getattr(self, "_compat_rows", False):
            self._device.clear_thermal()

    def _apply_temperature(self, dev):
        if getattr(self, "_compat_rows", False):
            raise NotImplementedError("thermal loads are not available in the reference_compat strut model")
        alpha, dT, ba = self.thermal
        if self.conduction_driven:
            dT = self._solve_conduction(dev) - self.conduction["reference"]
        dev.set_thermal(alpha, dT, ba)

    # -- steady heat conduction on the struts (FEM mode; pl_set_conduction) --------------------
    @property
    def conduction_driven(self):
        """True when the temperature of set_temperature is the solution of the conduction problem."""
        return self.thermal is not None and isinstance(self.thermal[1], str)

    def _thermal_nodes(self, spec, what, share):
        """(mask (n,), values (n,)) of a boundary description of the conduction problem: a block {"Surface": [...], "Value": v}
        or a dict of named blocks, as the presets' boundary conditions are written; share: the value is a total, divided
        equally over the nodes of its surface."""
        n = self.lattice.n_nodes
        mask, val = np.zeros(n, bool), np.zeros(n)
        blocks = [spec] if "Surface" in spec else list(spec.values())
        for b in blocks:
            if "Surface" not in b or "Value" not in b:
                raise ValueError(f"solve_temperature: a {what} block needs 'Surface' and 'Value'")
            pts = self.find_point_on_lattice_surface(list(b["Surface"]), b.get("SurfaceCells", None))
            v = float(np.asarray(b["Value"], dtype=float).reshape(-1)[0])
            mask[pts] = True
            if share:
                val[pts] += v / len(pts)
            else:
                val[pts] = v
        return mask, val

    def _set_conduction_problem(self, conductivity, fixed, heat_flow, beam_conductivity, reference, convection=None):
        n = self.lattice.n_nodes
        if self.domain_decomposition_solver:
            raise ValueError("solve_temperature: heat conduction needs the FEM strut model (DDM handles carry no strut graph)")
        conv = None
        if convection is not None:     # {"film": h, "ambient": T_inf, "beam_film": optional (n_beams,)}
            if "ambient" not in convection or ("film" not in convection and convection.get("beam_film", None) is None):
                raise ValueError('solve_temperature: convection needs "film" (or "beam_film") and "ambient"')
            bf = convection.get("beam_film", None)
            bf = None if bf is None else np.array(np.broadcast_to(np.asarray(bf, dtype=float), (self.lattice.n_beams,)))
            film, amb = float(convection.get("film", 0.0)), float(convection["ambient"])
            if not (np.isfinite(amb) and ((bf is None and film > 0 and np.isfinite(film)) or
                                          (bf is not None and (bf >= 0).all() and np.isfinite(bf).all() and bf.any()))):
                raise ValueError("solve_temperature: film coefficients must be non-negative, finite and not all zero, "
                                 "the ambient temperature finite")
            conv = {"film": film, "ambient": amb, "beam_film": bf}
        if fixed is None:              # (the caller has checked that convection makes this a valid problem)
            mask, t_bar = np.zeros(n, bool), np.zeros(n)
        elif isinstance(fixed, dict):
            mask, t_bar = self._thermal_nodes(fixed, "Temperature", False)
        elif isinstance(fixed, (tuple, list)) and len(fixed) == 2:
            mask = np.array(np.broadcast_to(np.asarray(fixed[0]).reshape(-1) != 0, (n,)))
            t_bar = np.where(mask, np.broadcast_to(np.asarray(fixed[1], dtype=float), (n,)), 0.0)
        else:                                      # (n,) temperatures, NaN on the free nodes
            t = np.array(np.broadcast_to(np.asarray(fixed, dtype=float), (n,)))
            mask, t_bar = ~np.isnan(t), np.nan_to_num(t)
        if heat_flow is None:
            q = None
        elif isinstance(heat_flow, dict):
            q = self._thermal_nodes(heat_flow, "HeatFlow", True)[1]
        else:
            q = np.array(np.broadcast_to(np.asarray(heat_flow, dtype=float), (n,)))
        bk = None if beam_conductivity is None else np.array(np.broadcast_to(np.asarray(beam_conductivity, dtype=float),
                                                                             (self.lattice.n_beams,)))
        if not mask.any() and conv is None:
            raise ValueError("solve_temperature: no node has a prescribed temperature")
        if not (np.isfinite(t_bar).all() and (q is None or np.isfinite(q).all()) and np.isfinite(reference)):
            raise ValueError("solve_temperature: temperatures, heat flows and the reference must be finite")
        if not ((bk is None and conductivity > 0 and np.isfinite(conductivity)) or
                (bk is not None and (bk > 0).all() and np.isfinite(bk).all())):
            raise ValueError("solve_temperature: conductivities must be positive and finite")
        self.conduction = {"conductivity": float(conductivity), "beam_conductivity": bk, "fixed": mask, "t_bar": t_bar,
                           "heat_flow": None if q is None else np.where(mask, 0.0, q), "reference": float(reference),
                           "convection": conv}

    def _assemble_for_conduction(self, dev):
        """The conduction calls need an assembled handle (the strut records); a handle that never saw boundary conditions
        gets the lattice's mask first, which the next mechanical solve installs again with its values and loads."""
        if not dev._assembled:
            dev.set_bc(self.fixed_DOF)
            dev.assemble()

    def _conduction_states(self, dev):
        """The conduction and convection states of the kept problem on the handle, set where they differ."""
        c = self.conduction
        want = c["conductivity"] if c["beam_conductivity"] is None else c["beam_conductivity"]
        if dev._conduction is None or not np.array_equal(np.asarray(dev._conduction), np.asarray(want)):
            dev.set_conduction(c["conductivity"], c["beam_conductivity"])
        cv = c.get("convection", None)
        if cv is None:
            if dev._convection is not None:
                dev.clear_convection()
        else:
            want = cv["film"] if cv["beam_film"] is None else cv["beam_film"]
            have = dev._convection
            if have is None or have[1] != cv["ambient"] or not np.array_equal(np.asarray(have[0]), np.asarray(want)):
                dev.set_convection(cv["film"], cv["ambient"], cv["beam_film"])

    def _solve_conduction(self, dev):
        """T of the conduction problem on the handle's current radii (pl_cond_solve); the handle must be assembled."""
        c = self.conduction
        self._conduction_states(dev)
        T, self.conduction_stats = dev.cond_solve(c["fixed"], c["t_bar"], c["heat_flow"], rtol=1e-12, max_iter=200000)
        self.temperature_field = T
        return T

    def solve_temperature(self, conductivity=None, fixed=None, heat_flow=None, beam_conductivity=None, reference=0.0,
                          convection=None):
        """Steady temperatures of the lattice nodes, each strut one conductor g = k kappa pi r^2 / L between its nodes:
        K_T T = q on the free nodes, T prescribed on the others.  conductivity: kappa of every strut, or beam_conductivity
        (n_beams,) per strut.  fixed: the prescribed temperatures - a block {"Surface": [...], "Value": T} or a dict of named
        blocks, as the presets' boundary conditions name surfaces; or (mask, values); or an (n_nodes,) array with NaN on the
        free nodes.  heat_flow: the heat inflow - blocks whose "Value" is the TOTAL of the surface, shared equally over its
        nodes, or an (n_nodes,) array of nodal inflows.  reference: the stress-free temperature that
        set_temperature("conduction", alpha) subtracts.  Returns T (n_nodes,); the problem is kept, and solved again before
        every mechanical solve under a conduction-driven temperature.  Without arguments: the problem kept last (that of the
        preset's "conduction" block, for instance) on the current radii.
        convection = {"film": h, "ambient": T_inf, "beam_film": optional (n_beams,)}: every strut end also exchanges with
        an ambient at T_inf through c = k h pi r L (lumped: (K_T + diag H) T = q + H T_inf); ``fixed`` may then be None -
        the convection alone makes the problem well posed."""
        if getattr(self, "_compat_rows", False):
            raise NotImplementedError("heat conduction is not available in the reference_compat strut model")
        if conductivity is None and fixed is None:
            if self.conduction is None:
                raise RuntimeError("solve_temperature: no conduction problem is defined (give conductivity and fixed)")
        elif (conductivity is None and beam_conductivity is None) or (fixed is None and convection is None):
            raise ValueError("solve_temperature needs a conductivity and the prescribed temperatures")
        else:
            self._set_conduction_problem(0.0 if conductivity is None else conductivity, fixed, heat_flow, beam_conductivity,
                                         reference, convection)
        dev = self.device_model()
        self._assemble_for_conduction(dev)
        return self._solve_conduction(dev).copy()

    def transient_temperature(self, dt, n_steps, heat_capacity, theta=1.0, initial=None, amplitude=None, fixed_amplitude=None,
                              probes=None, snap_every=0, beam_heat_capacity=None, node_capacity=None, rtol=1e-10,
                              max_iter=100000):
        """Temperatures in time of the conduction problem kept by the last ``solve_temperature`` - its mask, prescribed values,
        heat flow and convection - on the device (pl_set_heat_capacity, pl_cond_transient): n_steps implicit theta steps
        (theta = 1 backward Euler, 1/2 Crank-Nicolson) of C dT/dt + (K_T + H) T = a(t) q + H T_inf, C the lumped capacity of the
        struts at the volumetric heat capacity ``heat_capacity`` (or beam_heat_capacity (n_beams,) per strut) plus
        node_capacity (n_nodes,).  initial: the start field, (n_nodes,) or a scalar; None = the ambient of the convection,
        else the problem's reference.  The heat flow is load pattern 0 with the factor ``amplitude``; the prescribed nodes go
        from the start field to their values with the factor ``fixed_amplitude`` (None = at their values from the first row
        on: a thermal shock).  Both: a callable of the time, an array (n_steps + 1,), or None = 1 throughout, as in
        ``transient_response``.  probes: node indices (default: every node).  Returns the device call's dict - times, probe,
        heat (U, Q_in, Q_c, Q_R), iters, state, snaps - and keeps it as ``temperature_history``; ``temperature_field`` is left
        alone, and ``set_temperature`` takes any row of the history."""
        if getattr(self, "_compat_rows", False) or self.domain_decomposition_solver:
            raise NotImplementedError("heat conduction is not available in the reference_compat strut model or on a "
                                      "domain-decomposition lattice")
        if self.conduction is None:
            raise RuntimeError("transient_temperature: no conduction problem is defined (solve_temperature)")
        c = self.conduction
        n, rows = self.lattice.n_nodes, int(n_steps) + 1
        time = float(dt) * np.arange(rows)

        def factor(a, what):
            if a is None:
                return None
            if callable(a):
                return np.array([float(a(t)) for t in time])
            a = np.asarray(a, float).reshape(-1)
            if a.size != rows:
                raise ValueError(f"{what} must have {rows} entries")
            return a

        amp0, bar_amp = factor(amplitude, "amplitude"), factor(fixed_amplitude, "fixed_amplitude")
        cv = c.get("convection", None)
        if initial is None:
            initial = cv["ambient"] if cv is not None else c["reference"]
        t0 = np.array(np.broadcast_to(np.asarray(initial, dtype=float), (n,)))
        dev = self.device_model()
        self._assemble_for_conduction(dev)
        self._conduction_states(dev)
        bh = None if beam_heat_capacity is None else np.array(np.broadcast_to(np.asarray(beam_heat_capacity, dtype=float),
                                                                              (self.lattice.n_beams,)))
        nc = None if node_capacity is None else np.array(np.broadcast_to(np.asarray(node_capacity, dtype=float), (n,)))
        have = dev._heat_capacity
        if have is None or not np.array_equal(np.asarray(have[0]), np.asarray(float(heat_capacity) if bh is None else bh)) or \
                (have[1] is None) != (nc is None) or (nc is not None and not np.array_equal(have[1], nc)):
            dev.set_heat_capacity(0.0 if bh is not None else heat_capacity, bh, nc)
        q = c["heat_flow"]
        out = dev.cond_transient(dt, n_steps, theta, c["fixed"], c["t_bar"], bar_amp, None if q is None else q[None],
                                 None if q is None else (np.ones(rows) if amp0 is None else amp0)[:, None], t0, rtol=rtol,
                                 max_iter=max_iter, probes=np.arange(n) if probes is None else np.asarray(probes, int).reshape(-1),
                                 snap_every=snap_every)
        self.temperature_history = out
        return out

    def clear_conduction(self):
        """Removes the conduction problem (and a temperature that is driven by it)."""
        if self.conduction_driven:
            self.clear_temperature()
        self.conduction = None
        self.temperature_field = None
        if self._device is not None and not getattr(self, "_compat_rows", False):
            self._device.clear_conduction()

    def strut_heat_flow(self):
        """(n_beams,) heat flow Q_b = g (T_A - T_B) / k of one copy of every strut, from its first node to its second, for
        the temperatures of the last conduction solve (pl_cond_flux)."""
        if self.conduction is None or self.temperature_field is None:
            raise RuntimeError("strut_heat_flow: no temperature field (solve_temperature)")
        dev = self.device_model()
        self._assemble_for_conduction(dev)
        return dev.cond_flux(self.temperature_field)

    def _convective_field(self, who):
        if self.conduction is None or self.temperature_field is None:
            raise RuntimeError(f"{who}: no temperature field (solve_temperature)")
        if self.conduction.get("convection", None) is None:
            raise RuntimeError(f"{who}: the conduction problem has no convection")
        dev = self.device_model()
        self._assemble_for_conduction(dev)
        if dev._convection is None:              # (a handle made after the last solve)
            self._solve_conduction(dev)
        return dev

    def strut_heat_loss(self):
        """(n_beams,) convective loss Qc_b = c [(T_A - T_inf) + (T_B - T_inf)] / k of one copy of every strut for the
        temperatures of the last conduction solve (pl_cond_film)."""
        return self._convective_field("strut_heat_loss").cond_film(self.temperature_field)

    def dissipated_power(self):
        """P = sum_i H_i (T_i - T_inf), what the lattice gives to the ambient at the temperatures of the last conduction
        solve, summed on the device in a fixed order (pl_cond_film)."""
        return self._convective_field("dissipated_power").cond_film(self.temperature_field, total=True)[1]

    def max_temperature(self, p=None, reference=None):
        """Peak of T - reference over the free nodes of the conduction problem for the temperatures of its last solve; with
        p: (peak, p-norm) of pl_temp_pnorm.  reference: default the ambient of the convection, else the problem's reference."""
        if self.conduction is None or self.temperature_field is None:
            raise RuntimeError("max_temperature: no temperature field (solve_temperature)")
        c = self.conduction
        if reference is None:
            reference = c["convection"]["ambient"] if c.get("convection", None) is not None else c["reference"]
        dev = self.device_model()
        self._assemble_for_conduction(dev)
        res = dev.temp_pnorm(self.temperature_field, 1.0 if p is None else p, reference, ~c["fixed"])
        return res["max"] if p is None else (res["max"], res["phi"])

    def thermal_strut_forces(self):
        """(n_beams,) restrained thermal force n_free of one copy of every strut (pl_thermal_load): what a strut heated and
        held at both ends pushes with, ka alpha L mean(dT) / k."""
        if self.thermal is None:
            raise RuntimeError("thermal_strut_forces: no temperature is set (set_temperature)")
        if self._device is None:
            raise RuntimeError("thermal_strut_forces needs a solve_FEM_FenicsX on this lattice first")
        return self._device.thermal_load()[1]

    def _no_temperature(self, who):
        if self.thermal is not None:
            raise RuntimeError(f"{who}: K_g is built from K_e u_e and would ignore the thermal prestress; "
                               "clear_temperature() first")

    def strut_stress(self, where=0):
        """Section forces and von Mises stress of every strut for the displacements of the last solve_FEM_FenicsX, on the
        device (pl_stress; the reference: generalized_stress / calculate_forces / calculate_moments,
        simulation_base.py:116-174): dict with N, V, T, Mb, sigma_vm of shape (n_beams, 4) - the stations [A, q1, q2, B] of
        every strut, NaN where absent - and peak (n_beams,).  where = 1: the two ends of the un-penalised middle segment only."""
        if self._device is None or getattr(self, "_compat_rows", False):
            raise RuntimeError("strut_stress needs a solve_FEM_FenicsX on this lattice first (default strut model; the "
                               "reference_compat model has no device stress pass)")
        # (LatticeOpti solves adjoint systems on the same handle: its equilibrium field is passed explicitly; otherwise the
        #  solution of the last solve is still on the device)
        model = getattr(self, "_model", None)
        return self._device.stress(None if model is None else model._u_solver, where=where)

    def max_strut_stress(self, where=0):
        """Largest von Mises stress of any strut station (what the reference's extract_stress_field prints,
        simulation_base.py:776-806)."""
        return float(self.strut_stress(where)["peak"].max())

    def strut_buckling(self, length=1, k_eff=1.0, shear=0):
        """Euler buckling utilisation of every strut for the displacements of the last solve_FEM_FenicsX, on the device
        (pl_buckling): dict with util = max(0, -N) / N_cr (buckling predicted at 1; 0 in tension), n_axial (signed axial force
        of one copy) and n_crit, each (n_beams,).  length = 1: the un-penalised middle segment is the buckling length (NaN on a
        strut without one), 0: the node-to-node length; k_eff: effective-length factor (1 pinned-pinned, 0.5 clamped-clamped);
        shear = 1: Engesser's shear-reduced load."""
        if self._device is None or getattr(self, "_compat_rows", False):
            raise RuntimeError("strut_buckling needs a solve_FEM_FenicsX on this lattice first (default strut model; the "
                               "reference_compat model has no device buckling pass)")
        model = getattr(self, "_model", None)       # (as strut_stress: LatticeOpti's equilibrium field is passed explicitly)
        return self._device.buckling(None if model is None else model._u_solver, length=length, k_eff=k_eff, shear=shear)

    def max_strut_buckling(self, length=1, k_eff=1.0, shear=0):
        """Largest buckling utilisation of any present strut (0 when no strut is compressed or none is present)."""
        util = self.strut_buckling(length, k_eff, shear)["util"]
        util = util[~np.isnan(util)]                 # (length = 1: struts without a middle segment are absent)
        return float(util.max()) if util.size else 0.0

    def global_buckling(self, n_modes=4, **kw):
        """Global linear buckling for the displacements of the last solve_FEM_FenicsX, on the device (pl_buckling_modes):
        the n_modes smallest positive factors lambda by which the applied loads may grow before cells or the whole lattice
        buckle together, (K + lambda K_g(u)) phi = 0, and their modes.  Every strut enters K_g as one element between its two
        joints: a strut buckling on its own is the business of ``strut_buckling``.  Keyword arguments (n_sub, rtol, max_iter,
        tol, max_outer) go to ``HipLattice.buckling_modes``.  Sets ``buckling_load_factors`` (n_modes,) and
        ``buckling_modes`` (n_modes, n_nodes, 6) - NaN beyond the factors that exist - and returns the device call's dict."""
        if self._device is None or getattr(self, "_compat_rows", False):
            raise RuntimeError("global_buckling needs a solve_FEM_FenicsX on this lattice first (default strut model; the "
                               "reference_compat model has no device buckling pass)")
        self._no_temperature("global_buckling")
        model = getattr(self, "_model", None)       # (as strut_stress: LatticeOpti's equilibrium field is passed explicitly)
        out = self._device.buckling_modes(n_modes, None if model is None else model._u_solver, **kw)
        self.buckling_load_factors = out["load_factor"]
        self.buckling_modes = out["modes"]
        return out

    def global_buckling_sensitivity(self, p=8, want_rows=True, **kw):
        """Derivatives of the load factors of the last ``global_buckling`` to the strut radii, on the device
        (pl_buckling_modes_sens), and of their aggregate J = (sum_i lambda_i^-p)^(1/p) >= 1 / lambda_1
        (geometric_host.load_factor_aggregate): dict with aggregate, dJ_dr (n_beams,) - the device's weighted sum with the
        weights dJ/dlambda_i - and dlam_dr (n_modes, n_beams) (want_rows=False leaves it out).  All are total derivatives at
        fixed segment geometry: the displacements follow the radii.  The rows of a repeated factor are not derivatives one by
        one; J weighs equal factors equally, so dJ_dr is - as long as the aggregate holds whole clusters.  Keyword arguments
        (rtol, max_iter) go to ``HipLattice.buckling_modes_sens``."""
        if self._device is None or getattr(self, "_compat_rows", False):
            raise RuntimeError("global_buckling needs a solve_FEM_FenicsX on this lattice first (default strut model; the "
                               "reference_compat model has no device buckling pass)")
        self._no_temperature("global_buckling_sensitivity")
        if getattr(self, "buckling_load_factors", None) is None:
            raise RuntimeError("global_buckling_sensitivity needs a global_buckling on this lattice first")
        from .geometric_host import load_factor_aggregate
        lam = self.buckling_load_factors
        J, wts = load_factor_aggregate(lam, p)
        model = getattr(self, "_model", None)       # (as global_buckling)
        out = self._device.buckling_modes_sens(lam, self.buckling_modes, None if model is None else model._u_solver,
                                               weights=wts, want_rows=want_rows, **kw)
        res = {"aggregate": J, "dJ_dr": out["dsum_dr"]}
        if want_rows:
            res["dlam_dr"] = out["dlam_dr"]
        return res

    def natural_frequencies(self, n_modes=4, density=1.0, rotary=True, node_mass=None, **kw):
        """Natural frequencies of the lattice under the supports of the last solve_FEM_FenicsX, on the device
        (pl_set_mass, pl_vibration_modes): the n_modes smallest omega^2 of K phi = omega^2 M phi and their modes, M the
        consistent mass of the struts at ``density`` (every strut one element between its two joints, its plain radius over
        the whole length; ``rotary``: with the rotary inertia of bending), plus translational point masses node_mass
        (n_nodes,).  The loads play no part.  Keyword arguments (n_sub, rtol, max_iter, tol, max_outer) go to
        ``HipLattice.vibration_modes``.  Sets ``natural_frequencies_hz`` = sqrt(omega^2) / 2 pi and ``vibration_omega2``
        (n_modes,), ``vibration_modes`` (n_modes, n_nodes, 6) with phi^T M phi = 1 - NaN beyond the modes that exist - and
        returns the device call's dict with ``frequency`` (Hz) added."""
        if self._device is None or getattr(self, "_compat_rows", False):
            raise RuntimeError("natural_frequencies needs a solve_FEM_FenicsX on this lattice first (default strut model; "
                               "the reference_compat model has no device mass)")
        self._device.set_mass(density, rotary, node_mass)
        out = self._device.vibration_modes(n_modes, **kw)
        out["frequency"] = np.sqrt(out["omega2"]) / (2.0 * np.pi)
        self.natural_frequencies_hz = out["frequency"]
        self.vibration_omega2 = out["omega2"]
        self.vibration_modes = out["modes"]
        return out

    def transient_response(self, dt, n_steps, density, amplitude=None, base_acceleration=None, damping=(0.0, 0.0),
                           probes=None, rotary=True, node_mass=None, **kw):
        """Response in time under the supports and the force set of the last solve_FEM_FenicsX, on the device (pl_set_mass,
        pl_transient): implicit Newmark steps of M a + C v + K u = f(t) from rest, M the consistent mass of the struts at
        ``density`` (as ``natural_frequencies``), C = damping[0] M + damping[1] K.  The force set is load pattern 0 with the
        factor ``amplitude``: a callable of the time, an array (n_steps + 1,), or None = 1 throughout (a suddenly applied
        load).  ``base_acceleration`` = (direction (3,), a_g (n_steps + 1,)) adds the inertia load -M e_direction a_g[n] of a
        moving base, the response then being relative to it.  probes: node indices (default: the loaded nodes).  Keyword
        arguments (beta, gamma, rtol, max_iter, u0, v0, snap_every) go to ``HipLattice.transient``.  Sets ``transient_time``
        (n_steps + 1,), ``transient_probe`` (n_steps + 1, 3, n_probe, 6) = u, v, a of the probes, ``transient_energy``
        (n_steps + 1, 3) = kinetic, strain, external work, ``transient_state`` (3, n_nodes, 6) and returns the device call's
        dict."""
        s = self._transient_setup("transient_response", dt, n_steps, density, amplitude, base_acceleration, damping, rotary,
                                  node_mass, kw)
        dev, n = self._device, self.lattice.n_nodes
        force, amp0 = s["force"], s["amp0"]
        patterns, amps = [force], [amp0]
        if base_acceleration is not None:
            direction, a_g = s["base_acceleration"]
            e = np.zeros((1, n, 6))
            e[0, :, :3] = np.asarray(direction, float).reshape(3)
            patterns.append(-dev.mass_spmv_multi(e)[0])
            amps.append(a_g)
        if probes is None:
            probes = np.flatnonzero(np.abs(force).sum(axis=1) > 0)
        probes = np.asarray(probes, int).reshape(-1)
        out = dev.transient(dt, n_steps, np.stack(patterns), np.stack(amps, axis=1), ray_m=damping[0], ray_k=damping[1],
                            probes=probes, **kw)
        self.transient_time, self.transient_probe = out["time"], out["probe"]
        self.transient_energy, self.transient_state = out["energy"], out["state"]
        self._transient_probes = probes
        self._transient_settings = s
        return out

    def _dynamics_guard(self, who):
        """What the dynamic responses ask of the lattice: the default strut model, a FEM handle, a solve behind it."""
        if getattr(self, "_compat_rows", False) or self.domain_decomposition_solver:
            raise NotImplementedError(f"{who}: the default strut model on a FEM lattice only (no reference_compat "
                                      "rows, no domain decomposition)")
        if self._device is None:
            raise RuntimeError(f"{who} needs a solve_FEM_FenicsX on this lattice first")

    def _transient_setup(self, who, dt, n_steps, density, amplitude, base_acceleration, damping, rotary, node_mass, kw):
        """The checks of ``transient_response``, the mass model on the device, and the settings of the run as a dict: what
        ``transient_sensitivity`` runs again."""
        self._dynamics_guard(who)
        n, rows = self.lattice.n_nodes, int(n_steps) + 1
        self._device.set_mass(density, rotary, node_mass)
        time = float(dt) * np.arange(rows)
        force = np.zeros((n, 6))
        force[:, :3] = np.asarray(self.applied_force)[:n, :3]      # (only the translational components are loads)
        if amplitude is None:
            amp0 = np.ones(rows)
        elif callable(amplitude):
            amp0 = np.array([float(amplitude(t)) for t in time])
        else:
            amp0 = np.asarray(amplitude, float).reshape(-1)
            if amp0.size != rows:
                raise ValueError(f"amplitude must have {rows} entries")
        if base_acceleration is not None:
            direction, a_g = base_acceleration
            a_g = np.asarray(a_g, float).reshape(-1)
            if a_g.size != rows:
                raise ValueError(f"base_acceleration needs {rows} accelerations")
            base_acceleration = (np.asarray(direction, float).reshape(3), a_g)
        run = {q: kw[q] for q in ("beta", "gamma", "rtol", "max_iter", "u0", "v0") if q in kw}
        return dict(dt=float(dt), n_steps=int(n_steps), density=density, rotary=rotary, node_mass=node_mass, force=force,
                    amp0=amp0, base_acceleration=base_acceleration, damping=(float(damping[0]), float(damping[1])), run=run)

    def transient_sensitivity(self, output=None, kind=2, p=8, weight=None):
        """Radius derivatives of an objective of the last ``transient_response``, on the device (pl_transient_sens: the run
        again with the same time step, density, amplitude, base acceleration, damping and scheme, then the discrete adjoint
        of the scheme backwards in time).  One output per row y_n = l . u_n: ``output`` is l as an (n_nodes, 6) array, a
        (node, dof) pair, or None = the force pattern scaled to unit norm.  J of the outputs with the weights ``weight``
        (n_steps + 1,) or None = 1: kind 0 sum w y, 1 1/2 sum w y^2, 2 (sum w |y|^p)^(1/p) >= max |y| for w = 1.  Returns a
        dict with J, y (n_steps + 1,) and dJ_dr (n_beams,) at fixed segment geometry, plus the iterations of both passes."""
        if getattr(self, "_compat_rows", False) or self.domain_decomposition_solver:
            raise NotImplementedError("transient_sensitivity: the default strut model on a FEM lattice only (no "
                                      "reference_compat rows, no domain decomposition)")
        s = getattr(self, "_transient_settings", None)
        if s is None or self._device is None:
            raise RuntimeError("transient_sensitivity needs a transient_response on this lattice first")
        n = self.lattice.n_nodes
        if output is None:
            norm = float(np.linalg.norm(s["force"]))
            if norm == 0.0:
                raise ValueError("transient_sensitivity: no force pattern to take the output from; give output")
            l = s["force"] / norm
        elif np.ndim(output) == 1 and np.size(output) == 2:
            l = np.zeros((n, 6))
            l[int(output[0]), int(output[1])] = 1.0
        else:
            l = np.asarray(output, float).reshape(n, 6)
        base = s["base_acceleration"]
        self._device.set_mass(s["density"], s["rotary"], s["node_mass"])
        return self._device.transient_sens(s["dt"], s["n_steps"], l, kind, p, weight, s["force"][None], s["amp0"][:, None],
                                           None if base is None else base[0], None if base is None else base[1],
                                           ray_m=s["damping"][0], ray_k=s["damping"][1], **s["run"])

    def dynamic_amplification(self):
        """max_t |u| / |u_static| of every probe of the last ``transient_response``, |.| the norm of the three translations and
        u_static the displacements of the last solve_FEM_FenicsX (n_probe,); 2 is the undamped one-degree-of-freedom value
        for a suddenly applied load."""
        if getattr(self, "transient_probe", None) is None:
            raise RuntimeError("dynamic_amplification needs a transient_response on this lattice first")
        u_dyn = np.linalg.norm(self.transient_probe[:, 0, :, :3], axis=2).max(axis=0)
        u_static = np.linalg.norm(np.asarray(self.displacement_vector)[self._transient_probes, :3], axis=1)
        return u_dyn / u_static

    def frequency_response(self, frequencies_hz, density, damping=(0.0, 0.0), probes=None, base_acceleration=None,
                           rotary=True, node_mass=None, **kw):
        """Steady-state response to a harmonic load under the supports of the last solve_FEM_FenicsX, on the device
        (pl_set_mass, pl_harmonic): for every frequency f (Hz), w = 2 pi f, the complex amplitudes u of
        (K + i w C - w^2 M) u = load, M the consistent mass of the struts at ``density`` (as ``natural_frequencies``),
        C = damping[0] M + damping[1] K.  The load is the force set of the solve; with ``base_acceleration`` = direction (3,)
        or an axis 0 / 1 / 2 it is the inertia load -M e_direction of a base shaken with unit acceleration amplitude, the
        response then being relative to the base.  probes: node indices (default: the nodes of the force set).  Keyword
        arguments (rtol, max_iter, block, fields, raise_on_noconv) go to ``HipLattice.harmonic``.  Sets ``frf_frequency`` (n_freq,) in Hz, ``frf_probe``
        (n_freq, n_probe, 6) complex, ``frf_power`` (n_freq, 4) = Re f^T u, Im f^T u, u^H K u, u^H M u, ``frf_iterations``
        (n_freq,), with a base acceleration ``frf_transmissibility`` (n_freq, n_probe, 3) = absolute over base displacement
        (else None), and returns the device call's dict."""
        self._dynamics_guard("frequency_response")
        dev, n = self._device, self.lattice.n_nodes
        hz = np.atleast_1d(np.asarray(frequencies_hz, float)).reshape(-1)
        dev.set_mass(density, rotary, node_mass)
        if base_acceleration is None:
            load = np.zeros((n, 6))
            load[:, :3] = np.asarray(self.applied_force)[:n, :3]      # (only the translational components are loads)
            if probes is None:
                probes = np.flatnonzero(np.abs(load).sum(axis=1) > 0)
        else:
            direction = (np.eye(3)[int(base_acceleration)] if np.ndim(base_acceleration) == 0
                         else np.asarray(base_acceleration, float).reshape(3))
            e = np.zeros((1, n, 6))
            e[0, :, :3] = direction
            load = -dev.mass_spmv_multi(e)[0]
            if probes is None:
                probes = np.flatnonzero(np.abs(np.asarray(self.applied_force)[:n, :3]).sum(axis=1) > 0)
        probes = np.asarray(probes, int).reshape(-1)
        out = dev.harmonic(2.0 * np.pi * hz, load, ray_m=float(damping[0]), ray_k=float(damping[1]), probes=probes, **kw)
        self.frf_frequency, self.frf_probe = hz, out["probe"]
        self.frf_power, self.frf_iterations = out["power"], out["iters"]
        self._frf_probes = probes
        self._frf_settings = self._frf_setup(hz, density, damping, base_acceleration, rotary, node_mass, kw)
        # a base moving with x_b e^{iwt}, -w^2 x_b = 1: absolute over base displacement, e_direction - w^2 u (the rigid
        # value e_direction at w = 0)
        self.frf_transmissibility = None
        if base_acceleration is not None:
            w2 = (2.0 * np.pi * hz) ** 2
            self.frf_transmissibility = direction[None, None, :] - w2[:, None, None] * out["probe"][:, :, :3]
        return out

    def _frf_setup(self, frequencies_hz, density, damping, base_acceleration, rotary, node_mass, kw):
        """The settings of a ``frequency_response`` as a dict: what ``frequency_response_sensitivity`` runs again.  The load
        is the force set of the last solve, or (base_acceleration: a direction (3,) or an axis 0 / 1 / 2) that of a base
        shaken with unit acceleration, which the device forms itself because it follows the design."""
        n = self.lattice.n_nodes
        load = direction = None
        if base_acceleration is None:
            load = np.zeros((n, 6))
            load[:, :3] = np.asarray(self.applied_force)[:n, :3]      # (only the translational components are loads)
        else:
            direction = (np.eye(3)[int(base_acceleration)] if np.ndim(base_acceleration) == 0
                         else np.asarray(base_acceleration, float).reshape(3))
        return dict(hz=np.atleast_1d(np.asarray(frequencies_hz, float)).reshape(-1), density=density, rotary=rotary,
                    node_mass=node_mass, damping=(float(damping[0]), float(damping[1])), load=load, base_dir=direction,
                    run={q: kw[q] for q in ("rtol", "max_iter", "block") if q in kw})

    def frequency_response_sensitivity(self, output=None, kind=2, p=8, weight=None):
        """Radius derivatives of an objective of the last ``frequency_response``, on the device (pl_harmonic_sens: the sweep
        again with the same frequencies, density, load or base acceleration, damping and solver settings, the adjoint fields
        in the same passes).  One complex output per frequency y_k = l^T u_k: ``output`` is l as an (n_nodes, 6) array, a
        (node, dof) pair, or None = the load itself (the dynamic compliance: no second solve).  J of the outputs with the
        weights ``weight`` (n_freq,) or None = 1: kind 0 -sum w Im y, 1 1/2 sum w |y|^2, 2 (sum w |y|^p)^(1/p) >= max |y| for
        w = 1.  Returns a dict with J, y (n_freq,) complex and dJ_dr (n_beams,) at fixed segment geometry, plus iters, relres
        and status (2, n_freq) of the forward and the adjoint solves."""
        if getattr(self, "_compat_rows", False) or self.domain_decomposition_solver:
            raise NotImplementedError("frequency_response_sensitivity: the default strut model on a FEM lattice only (no "
                                      "reference_compat rows, no domain decomposition)")
        s = getattr(self, "_frf_settings", None)
        if s is None or self._device is None:
            raise RuntimeError("frequency_response_sensitivity needs a frequency_response on this lattice first")
        n = self.lattice.n_nodes
        if output is None:
            l = None
        elif np.ndim(output) == 1 and np.size(output) == 2:
            l = np.zeros((n, 6))
            l[int(output[0]), int(output[1])] = 1.0
        else:
            l = np.asarray(output, float).reshape(n, 6)
        self._device.set_mass(s["density"], s["rotary"], s["node_mass"])
        return self._device.harmonic_sens(2.0 * np.pi * s["hz"], s["load"], l, kind, p, weight, s["base_dir"],
                                          ray_m=s["damping"][0], ray_k=s["damping"][1], **s["run"])

    def dynamic_stiffness_peaks(self):
        """The resonance peaks of the last ``frequency_response``: for every probe the local maxima of |u| over the
        frequencies, |.| the norm of the three complex translations - a list (one entry per probe) of dicts with index,
        frequency (Hz) and amplitude arrays.  The ends of the band count only if they lie above their one neighbour."""
        if getattr(self, "frf_probe", None) is None:
            raise RuntimeError("dynamic_stiffness_peaks needs a frequency_response on this lattice first")
        amp = np.linalg.norm(self.frf_probe[:, :, :3], axis=2)           # (n_freq, n_probe)
        pad = np.vstack([np.full((1, amp.shape[1]), -np.inf), amp, np.full((1, amp.shape[1]), -np.inf)])
        top = (pad[1:-1] > pad[:-2]) & (pad[1:-1] >= pad[2:]) if amp.shape[0] > 1 else np.zeros_like(amp, bool)
        peaks = []
        for j in range(amp.shape[1]):
            idx = np.flatnonzero(top[:, j])
            peaks.append({"index": idx, "frequency": self.frf_frequency[idx], "amplitude": amp[idx, j]})
        return peaks

    def natural_frequency_sensitivity(self, p=8, want_rows=True):
        """Derivatives of the omega^2 of the last ``natural_frequencies`` to the strut radii, on the device
        (pl_vibration_modes_sens: one pass over the struts, no solve), and of their aggregate
        J = (sum_i (omega_i^2)^-p)^(1/p) >= 1 / omega_1^2 (geometric_host.load_factor_aggregate): dict with aggregate, dJ_dr
        (n_beams,) - the device's weighted sum with the weights dJ/d(omega_i^2) - and domega2_dr (n_modes, n_beams)
        (want_rows=False leaves it out), at fixed segment geometry.  The rows of a repeated frequency are not derivatives one
        by one; J weighs equal frequencies equally, so dJ_dr is - as long as the aggregate holds whole clusters."""
        if getattr(self, "vibration_omega2", None) is None or self._device is None:
            raise RuntimeError("natural_frequency_sensitivity needs a natural_frequencies on this lattice first")
        from .geometric_host import load_factor_aggregate
        J, wts = load_factor_aggregate(self.vibration_omega2, p)
        out = self._device.vibration_modes_sens(self.vibration_omega2, self.vibration_modes, weights=wts, want_rows=want_rows)
        res = {"aggregate": J, "dJ_dr": out["dsum_dr"]}
        if want_rows:
            res["domega2_dr"] = out["domega2_dr"]
        return res

    # ------------------------------------------------------------------------------------------------
    # Domain decomposition (lattice_sim.py:846-919, 1111-1252)
    # ------------------------------------------------------------------------------------------------
    def cell_boundary_nodes(self):
        """(C, n_b) node ids of every cell in the order of Cell.define_node_order_to_simulate (cell.py:611-680)."""
        from .utils_schur import node_order_all_cells
        rows = node_order_all_cells(self)
        if rows is None:
            raise NotImplementedError("cells with different numbers of boundary nodes")
        return rows

    def set_schur_complements(self, S, cell_index=None):
        """Install cell Schur complements: one (6n_b)^2 matrix for every cell, or a stack plus a per-cell index.
        (The reference fills Cell.schur_complement from dolfinx or from its reduced-basis surrogates,
        lattice_sim.py:846-978; the surrogate files are outside this repository.)"""
        S = np.asarray(S, dtype=np.float64)
        if S.ndim == 2:
            S = S[None]
        self.schur_complements = S
        self._schur_cell_data = None       # (calculate_schur_complement_cells sets it again for its own matrices)
        self.cell_schur_index = (np.zeros(self.lattice.n_cells, np.int32) if cell_index is None
                                 else np.asarray(cell_index, np.int32))
        dev = self._ddm_device
        if dev is not None:
            if S.shape[1] == dev._m and len(self.cell_schur_index) == dev._n_cells:
                # same cells, other matrices (every iteration of a design loop): the handle takes them (round 5; it used to be
                # destroyed and created again - 10 ms per solve_DDM on a 12 x 4 x 4 lattice against 2 ms of device work)
                dev.update_ddm_matrices(S, self.cell_schur_index)
                if getattr(self, "_ddm_precond", 0) == 2:
                    self.define_preconditioner()
            else:
                dev.close()
                self._ddm_device = None

    @timing.category("simulation")
    @timing.timeit
    def calculate_schur_complement_cells(self):
        """Exact Schur complement of one representative cell per (geometry, radii) group (lattice_sim.py:846-919),
        condensed from that cell's own struts with their penalised segments.  The representatives - and, with gradients
        on, their central-difference variants - of one cell topology (connectivity + boundary order) go to the device
        in ONE batched condensation (pl_schur_cells); a topology beyond that kernel's size takes pl_schur per cell."""
        from . import _capi
        if self.type_schur_complement_computation != "exact":
            return self._surrogate_schur_complement_cells()
        lat, pen = self.lattice, self.penalized
        cb = self.cell_boundary_nodes()
        par = self._cell_parameter_radii()       # the reference groups by Cell.radii, which ignores the preset gradient
        keys = [tuple(np.round(par[c], 8)) for c in range(lat.n_cells)]
        groups, reps, idx = {}, [], np.zeros(lat.n_cells, np.int32)
        for c, k in enumerate(keys):
            if k not in groups:
                groups[k] = len(reps)
                reps.append(c)
            idx[c] = groups[k]
        mats, grads, data = [None] * len(reps), [None] * len(reps), [None] * len(reps)
        fd_gradients = self._schur_fd_gradients()
        by_topology = {}
        for q, c in enumerate(reps):
            beams = lat.cell_beam_idx[lat.cell_beam_ptr[c]:lat.cell_beam_ptr[c + 1]]
            nodes = np.unique(lat.beam_conn[beams])
            remap = np.full(lat.n_nodes, -1, np.int64)
            remap[nodes] = np.arange(len(nodes))
            conn, order = remap[lat.beam_conn[beams]], remap[cb[c]]
            key = (len(nodes), conn.tobytes(), order.tobytes())
            by_topology.setdefault(key, []).append((q, c, beams, nodes, conn, order))
            # what recover_cell_interiors sends for every cell that uses this matrix
            data[q] = {"cell": c, "key": key, "conn": conn, "order": order, "xyz": lat.node_xyz[nodes].copy(),
                       "radius": lat.beam_radius[beams].copy(), "seg_len": pen.seg_len[beams].copy(),
                       "seg_nsub": pen.seg_nsub[beams].copy()}
        for (n_nodes, _, _), members in by_topology.items():
            _, _, beams0, _, conn, order = members[0]
            if not _capi.schur_cells_fits(n_nodes, len(beams0), len(order)):
                for q, c, beams, nodes, conn, order in members:
                    mats[q], grads[q] = self._schur_cell_by_columns(c, beams, nodes, conn, order, par[c])
                continue
            # instances: every representative, then (gradients on) its +h / -h variants per radius parameter - the
            # reference's _compute_schur_gradients (lattice_sim.py:1020-1054): h = max(1e-8, 1e-6 max(1, |r|)), radii
            # changed at FIXED penalised segment lengths (Cell.change_beam_radius, cell.py:896-917)
            xyz, rad, slen, nsub, steps = [], [], [], [], []
            for q, c, beams, nodes, _, _ in members:
                base = lat.beam_radius[beams]
                variants = [base]
                if fd_gradients:
                    for j, rj in enumerate(par[c]):
                        h = max(1e-8, 1e-6 * max(1.0, abs(rj)))
                        rp, rm = rj + h, max(1e-12, rj - h)
                        steps.append(rp - rm)
                        sel = lat.beam_type[beams] == j
                        for rv in (rp, rm):
                            r = base.copy()
                            r[sel] = rv * self._cell_gfac[c]
                            variants.append(r)
                for r in variants:
                    xyz.append(lat.node_xyz[nodes])
                    rad.append(r)
                    slen.append(pen.seg_len[beams])
                    nsub.append(pen.seg_nsub[beams])
            S, info = _capi.schur_cells(np.stack(xyz), conn, order, np.stack(rad), np.stack(slen), np.stack(nsub),
                                        self.young_modulus, self.poisson_ratio, pen_coef=self.penalization_coefficient)
            bad = np.flatnonzero(info != 0)
            if len(bad):
                raise RuntimeError(f"exact Schur complement: cell {members[bad[0] // len(variants)][1]} cannot be condensed "
                                   f"(pl_schur_cells info {int(info[bad[0]])}: a mechanism or bad strut data)")
            per = len(variants)                   # instances per representative (the same for every member)
            for i, (q, c, *_rest) in enumerate(members):
                mats[q] = S[i * per]
                if fd_gradients:
                    st = steps[i * len(par[c]):(i + 1) * len(par[c])]
                    grads[q] = [(S[i * per + 1 + 2 * j] - S[i * per + 2 + 2 * j]) / st[j] for j in range(len(par[c]))]
        self.schur_gradients = grads if fd_gradients else None
        self._schur_gradients_array = None
        self.set_schur_complements(np.stack(mats), idx)
        self._schur_cell_data = data

    def _schur_fd_gradients(self):
        """Whether the exact branch also builds the central differences dS/dr (gradients on, not the analytic mode)."""
        return bool(self.enable_gradient_computing) and self.ddm_gradient != "analytic"

    # Opt-in for cells beyond the batched kernels' size: an int makes _schur_cell_by_columns condense that many columns per
    # PCG pass (pl_schur_block; 0 = the library's choice) and _recover_cell_by_solve solve u and lam as two columns of one
    # pl_solve_multi.  None: one pl_solve per column / field.
    schur_column_block = None

    def _schur_cell_by_columns(self, c, beams, nodes, conn, order, radii):
        """Exact Schur complement (and, with gradients on, its central differences) of cell c by pl_schur: one PCG solve
        per boundary dof on a handle of the cell's struts - for cells beyond the batched kernel's size."""
        blk = self.schur_column_block
        from ._capi import HipLattice
        lat, pen = self.lattice, self.penalized
        with HipLattice(lat.node_xyz[nodes], conn, lat.beam_radius[beams],
                        pen.seg_len[beams], pen.seg_nsub[beams], self.young_modulus, self.poisson_ratio,
                        pen_coef=self.penalization_coefficient, reorder=0,
                        **({"precond": 5} if 6 * len(nodes) <= DDM_DENSE_MAX else {})) as dev:   # (see cell_device)
            dev.assemble()
            S = dev.schur(order, rtol=1e-13, max_iter=200000, block=blk)
            if not self._schur_fd_gradients():
                return S, None
            gl = []
            for j, rj in enumerate(radii):
                h = max(1e-8, 1e-6 * max(1.0, abs(rj)))
                rp, rm = rj + h, max(1e-12, rj - h)
                S_pm = []
                for rv in (rp, rm):
                    rad = lat.beam_radius[beams].copy()
                    sel = lat.beam_type[beams] == j
                    rad[sel] = rv * self._cell_gfac[c]
                    dev.update_radii(rad)
                    dev.assemble()
                    S_pm.append(dev.schur(order, rtol=1e-13, max_iter=200000, block=blk))
                gl.append((S_pm[0] - S_pm[1]) / (rp - rm))
            return S, gl

    def _surrogate_schur_complement_cells(self):
        """Surrogate branch of lattice_sim.py:846-919: one batched evaluation S(r) = B alpha(r) for the distinct
        radius sets of the lattice (keys rounded to 8 decimals like the reference's cache), plus dS/dr when
        enable_gradient_computing is set."""
        if self.schur_surrogate is None:
            raise NotImplementedError("Not implemented schur complement computation method.")
        par = np.asarray(self._cell_parameter_radii(), dtype=float)
        # distinct radius sets, rounded to 8 decimals like the reference's cache keys (one numpy pass; the per-cell tuples and the
        # dictionary of the first version were 10 ms at 4 096 cells)
        uniq, idx = np.unique(np.round(par.reshape(len(par), -1), 8), axis=0, return_inverse=True)
        idx = np.asarray(idx, dtype=np.int32).ravel()
        radii_batch = uniq.tolist()
        S = self.schur_surrogate.schur_batch(radii_batch)
        self.schur_gradients, self._schur_gradients_array = None, None
        if self.enable_gradient_computing:
            G = self.schur_surrogate.schur_gradients_batch(radii_batch)          # (n_q, d, n, n) in one go, or None
            if G is not None:
                self._schur_gradients_array = G
                self.schur_gradients = [list(g) for g in G]                      # (views)
            else:
                self.schur_gradients = [self.schur_surrogate.schur_gradients(r) for r in radii_batch]
        if self._verbose > 1:
            print("Number of unique Schur complements computed:", len(radii_batch))
        self.set_schur_complements(S, idx)

    def get_schur_complement_from_reduced_basis_batch(self, geometric_params_list):
        """lattice_sim.py:919-977."""
        if self.schur_surrogate is None:
            raise NotImplementedError("Not implemented schur complement computation method.")
        return self.schur_surrogate.schur_batch(geometric_params_list)

    def get_schur_complement_from_reduced_basis(self, geometric_params):
        """lattice_sim.py:979-1018."""
        return self.get_schur_complement_from_reduced_basis_batch([list(geometric_params)])[0]

    # ------------------------------------------------------------------------------------------------
    # Backward half of the exact DDM: cell interiors and exact strut sensitivities (pl_cells_recover)
    # ------------------------------------------------------------------------------------------------
    @timing.category("simulation")
    @timing.timeit
    def recover_cell_interiors(self, lam=None, want_sens=False):
        """Fill the interior rows of ``displacement_vector`` from its cell-boundary rows: u_I = -K_II^-1 K_IB u_B per cell
        (no load and no Dirichlet dof on interior nodes, as the DDM assumes).  The cells of one topology (connectivity +
        boundary order) go to the device in ONE call (pl_cells_recover), each with the strut data of its REPRESENTATIVE -
        the cell its Schur complement was condensed from - so that the recovered field belongs to the operator
        ``solve_DDM`` solved: u_full^T K u_full = u_B^T S u_B per cell.  With one radius set per cell this is the cell's
        own data and the field is the FEM field.  Cells beyond the kernel's size are solved one by one on a handle.

        ``lam`` (rows x 6, like ``displacement_vector``; None: lam = u): a second field recovered the same way from its
        boundary rows, for the sensitivities.  ``want_sens``: return the per-strut sensitivities
        lam_e^T (dK_e/dr) u_e as an (n_beams,) array on the lattice's strut indices (a strut held by several cells gets
        their sum); per cell they stay in ``cell_strut_sens`` as (strut indices, values).  Summed over the struts of one
        radius parameter of a cell they are lam_B^T (dS/dr) u_B, exactly and at fixed segment geometry.  They are
        derivatives with respect to the STRUT radius; a preset radius gradient (``_cell_gfac``) is the caller's chain
        rule."""
        from . import _capi
        if self.type_schur_complement_computation != "exact":
            raise NotImplementedError("recover_cell_interiors: surrogate Schur complements have no strut model behind "
                                      "their matrices; only the exact mode can recover cell interiors")
        if getattr(self, "_compat_rows", False):
            raise NotImplementedError("recover_cell_interiors: not available with reference_compat rows")
        data = self._schur_cell_data
        if data is None or self.cell_schur_index is None:
            raise ValueError("recover_cell_interiors: the cell matrices were not condensed by "
                             "calculate_schur_complement_cells() (set_schur_complements() installs matrices only)")
        lat, pen = self.lattice, self.penalized
        cb = self.cell_boundary_nodes()
        U = self.displacement_vector
        lam = None if lam is None else np.asarray(lam, dtype=float).reshape(U.shape)
        groups = {}
        for c in range(lat.n_cells):
            beams = lat.cell_beam_idx[lat.cell_beam_ptr[c]:lat.cell_beam_ptr[c + 1]]
            nodes = np.unique(lat.beam_conn[beams])
            conn, order = np.searchsorted(nodes, lat.beam_conn[beams]), np.searchsorted(nodes, cb[c])
            key = (len(nodes), conn.tobytes(), order.tobytes())
            src = data[self.cell_schur_index[c]]
            if src["key"] != key:
                # struts or nodes numbered differently from the representative's: the cell's own strut data
                src = {"xyz": lat.node_xyz[nodes], "radius": lat.beam_radius[beams], "seg_len": pen.seg_len[beams],
                       "seg_nsub": pen.seg_nsub[beams]}
            groups.setdefault(key, []).append((c, beams, nodes, conn, order, src))
        want = ("u", "sens") if want_sens else ("u",)
        sens = np.zeros(lat.n_beams) if want_sens else None
        self.cell_strut_sens = [None] * lat.n_cells if want_sens else None
        for (n_nodes, _, _), members in groups.items():
            _, beams0, _, conn, order, _ = members[0]
            ub = np.stack([U[cb[m[0]]].reshape(-1) for m in members])
            lb = None if lam is None else np.stack([lam[cb[m[0]]].reshape(-1) for m in members])
            if _capi.schur_cells_fits(n_nodes, len(beams0), len(order)):
                out = _capi.cells_recover(np.stack([m[5]["xyz"] for m in members]), conn, order,
                                          np.stack([m[5]["radius"] for m in members]),
                                          np.stack([m[5]["seg_len"] for m in members]),
                                          np.stack([m[5]["seg_nsub"] for m in members]), ub, self.young_modulus,
                                          self.poisson_ratio, lam_b=lb, want=want,
                                          pen_coef=self.penalization_coefficient)
                bad = np.flatnonzero(out["info"] != 0)
                if len(bad):
                    raise RuntimeError(f"recover_cell_interiors: cell {members[bad[0]][0]} cannot be recovered "
                                       f"(pl_cells_recover info {int(out['info'][bad[0]])}: a mechanism or bad strut data)")
            else:
                res = [self._recover_cell_by_solve(m[5], conn, order, ub[i], None if lb is None else lb[i], want_sens)
                       for i, m in enumerate(members)]
                out = {"u": np.stack([r[0] for r in res])}
                if want_sens:
                    out["sens"] = np.stack([r[2] for r in res])
            interior = np.setdiff1d(np.arange(n_nodes), order)
            for i, (c, beams, nodes, *_rest) in enumerate(members):
                U[nodes[interior]] = out["u"][i][interior]
                if want_sens:
                    self.cell_strut_sens[c] = (beams, out["sens"][i])
                    np.add.at(sens, beams, out["sens"][i])
        return sens

    def _recover_cell_by_solve(self, src, conn, order, ub, lb, want_sens):
        """recover_cell_interiors for one cell beyond the batched kernel's size: a handle of the cell's struts with every
        boundary dof fixed at its value, one solve per field, then pl_sens (the pattern of _schur_cell_by_columns).
        Returns (u_full, lam_full or None, sens or None)."""
        from ._capi import HipLattice
        n = len(src["xyz"])
        fixed = np.zeros((n, 6), bool)
        fixed[order] = True
        with HipLattice(src["xyz"], conn, src["radius"], src["seg_len"], src["seg_nsub"], self.young_modulus,
                        self.poisson_ratio, pen_coef=self.penalization_coefficient, reorder=0,
                        **({"precond": 5} if 6 * n <= DDM_DENSE_MAX else {})) as dev:
            fields = []
            if self.schur_column_block is not None:      # u and lam as the columns of one pass
                ubar = np.zeros((1 if lb is None else 2, n, 6))
                ubar[0, order] = np.asarray(ub).reshape(-1, 6)
                if lb is not None:
                    ubar[1, order] = np.asarray(lb).reshape(-1, 6)
                dev.set_bc(fixed)
                dev.assemble()
                fields = list(dev.solve_multi(ubar, None, rtol=1e-13, max_iter=200000)[0])
            for vb in () if fields else ((ub,) if lb is None else (ub, lb)):
                ubar = np.zeros((n, 6))
                ubar[order] = np.asarray(vb).reshape(-1, 6)
                if not ubar.any():
                    fields.append(ubar)
                    continue
                dev.set_bc(fixed, ubar, None)
                dev.assemble()
                fields.append(dev.solve(rtol=1e-13, max_iter=200000)[0])
            s = None
            if want_sens:
                dev.assemble()
                s = dev.sens(fields[0], None if lb is None else fields[1])
        return fields[0], (None if lb is None else fields[1]), s

    def ddm_result_model(self):
        """What ``solve_FEM_FenicsX`` hands back as its model, for a DDM result whose interiors were recovered
        (``solve_DDM(recover_interior=True)``): the whole field ``u``, the lattice and an assembled handle of its struts -
        what ``exportSimulationResults`` and the per-strut post-processing read."""
        from .utils_simulation import FullScaleLatticeSimulation
        dev = self.device_model()
        dev.update_radii(self.lattice.beam_radius)       # (a design loop in DDM mode changes radii without a new handle)
        dev.assemble()
        model = FullScaleLatticeSimulation(self, dev)
        model.u = model._u_solver = self.displacement_vector.copy()
        return model

    def ddm_model(self):
        from ._capi import HipLattice
        if self.schur_complements is None:
            raise ValueError("Schur complements are not defined: call calculate_schur_complement_cells() or "
                             "set_schur_complements()")
        if self._ddm_device is None:
            cb = self.cell_boundary_nodes()
            n_nodes = self.max_index_boundary + 1
            # enable_preconditioner: the reference factorises the assembled Schur matrix (lattice_sim.py:1333-1415).
            # The device does the same (dense Cholesky, precond = 2) up to DDM_DENSE_MAX dofs; beyond that the CG gets
            # the node-block Jacobi preconditioner of the same matrix (its 6 x 6 diagonal blocks, inverted: same solution,
            # more iterations - a quarter fewer than with the diagonal alone).
            # Round 5: above the dense limit the node blocks get a dense level on top (precond = 4: 12 rigid / strain modes
            # per aggregate of boundary nodes, Galerkin operator from the cell matrices) - the iteration count then stops
            # growing with the lattice (32^3 BCC cells: 2.2 x fewer iterations than the node blocks alone).
            self._ddm_precond = 0
            xyz = None
            if self.enable_preconditioner:
                self._ddm_precond = 2 if 6 * n_nodes <= DDM_DENSE_MAX else DDM_LARGE_PRECOND
                if self._ddm_precond == 4:
                    xyz = self.lattice.node_xyz[self._boundary_nodes_by_index()]
            # CG parameters of the reference's solve_DDM (lattice_sim.py:1156-1159): alpha clamp 100, direction-norm
            # stop 1e-12, restart every 500 000 iterations
            self._ddm_device = HipLattice.ddm(n_nodes, self.index_boundary[cb], self.schur_complements,
                                              self.cell_schur_index, precond=self._ddm_precond, alpha_max=100.0,
                                              mintol=1e-12, restart_every=500000, node_xyz=xyz,
                                              coarse_max_dofs=DDM_COARSE_MAX_DOFS)
            if self._ddm_precond == 2:
                self.define_preconditioner()
        return self._ddm_device

    def _define_preconditioner_approximation(self):
        """lattice_sim.py:1312-1329: the dataset the approximate preconditioners are built from -
        ``Schur_complement_mean_<geoms>.npz`` ("mean") or ``Schur_complement_<geoms>.npz`` ("nearest_reference") under
        ``data/outputs/schur_complement/`` of a data root; nothing for "exact"."""
        if self.preconditioner_type == "exact":
            return None
        if self.preconditioner_type not in ("mean", "nearest_reference"):
            raise NotImplementedError("Not implemented preconditioner approximation method.")
        stem = "Schur_complement_mean_" if self.preconditioner_type == "mean" else "Schur_complement_"
        name = stem + "_".join(str(g) for g in self.geom_types) + ".npz"
        roots = list(self.data_roots or [])
        if os.environ.get("PYLATTICE_DATA_ROOT"):
            roots.append(os.environ["PYLATTICE_DATA_ROOT"])
        roots.append(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        for root in roots:
            for sub in (os.path.join("data", "outputs", "schur_complement"), ""):
                path = os.path.join(root, sub, name)
                if os.path.isfile(path):
                    self.used_schur_preconditioner = np.load(path, allow_pickle=True)
                    return path
        if self.preconditioner_type == "mean":
            # the reference's checkout does not carry its Schur_complement_mean_*.npz files: build the mean matrix from
            # the radius dataset of the same geometries, else from this lattice's own cell matrices
            full = "Schur_complement_" + "_".join(str(g) for g in self.geom_types) + ".npz"
            for root in roots:
                for sub in (os.path.join("data", "outputs", "schur_complement"), ""):
                    path = os.path.join(root, sub, full)
                    if os.path.isfile(path):
                        mats = np.asarray(np.load(path, allow_pickle=True)["schur_matrices"], dtype=float)
                        self.used_schur_preconditioner = {"schur_matrices": mats.mean(axis=0)}
                        return path
            self._mean_of_own_cells = True      # re-evaluated whenever the cell matrices change (define_preconditioner)
            return None
        raise FileNotFoundError(f"Schur complement dataset for the '{self.preconditioner_type}' preconditioner not "
                                f"found: {name} (looked under {roots})")

    @timing.category("simulation")
    @timing.timeit
    def define_preconditioner(self):
        """lattice_sim.py:1333-1415 (define_preconditioner + build_preconditioner): choose the cell matrices the
        assembled preconditioner is made of and hand them to the device, which assembles and factorises
        ``sum_c B_c^T Shat_c B_c`` at the next ``assemble()``.  "exact": the cells' own Schur complements; "mean": the one
        matrix of the mean dataset for every cell; "nearest_reference": for every cell the dataset matrix whose radii
        are nearest (Euclidean, first on ties - sklearn's NearestNeighbors(n_neighbors=1) in the reference) to
        Cell.radii."""
        dev = self._ddm_device
        if dev is None or not self.enable_preconditioner or getattr(self, "_ddm_precond", 0) != 2:
            return
        if self.preconditioner_type == "exact" or self.preconditioner_type is None:
            dev.set_ddm_preconditioner(None)
            return
        if self.used_schur_preconditioner is None and not getattr(self, "_mean_of_own_cells", False):
            self._define_preconditioner_approximation()
        if self.used_schur_preconditioner is None:          # "mean" without any dataset: mean over this lattice's cells
            w = np.bincount(self.cell_schur_index, minlength=len(self.schur_complements)).astype(float)
            dev.set_ddm_preconditioner(np.tensordot(w / w.sum(), self.schur_complements, axes=(0, 0)))
            return
        data = self.used_schur_preconditioner
        mats = np.asarray(data["schur_matrices"], dtype=float)
        if self.preconditioner_type == "mean":
            dev.set_ddm_preconditioner(mats.reshape(-1, mats.shape[-2], mats.shape[-1])[:1])
            return
        pts = np.asarray(data["radius_values"], dtype=float)
        if pts.ndim == 1:
            pts = pts[:, None]
        radii = self._cell_parameter_radii()
        d2 = ((radii[:, None, :] - pts[None, :, :]) ** 2).sum(axis=2)
        dev.set_ddm_preconditioner(mats, np.argmin(d2, axis=1).astype(np.int32))

    def _cell_parameter_radii(self):
        """``Cell.radii`` of the reference for every cell: the radii the cell was GIVEN (preset value,
        reset_cell_with_new_radii, LatticeOpti), which the preset's radius gradient does not touch - it only scales
        the struts (cell.py:86,407-412).  The key of the reference's Schur-complement cache and the argument of its
        surrogates and of the nearest-reference preconditioner."""
        return self.lattice.cell_radii / self._cell_gfac[:, None]

    @timing.category("simulation")
    @timing.timeit
    def solve_DDM(self, recover_interior=False):
        """Domain-decomposition solve on the cell-boundary nodes (lattice_sim.py:1111-1176): right-hand side
        b = f_free - (S u_imposed)_free, plain CG with the reference's parameters (tol 1e-6, alpha clamp 100,
        max_iterations from the preset), results written back to displacement_vector; returns
        (xsol, info, global_displacement_index, b) or four None when b == 0.

        ``recover_interior`` (exact Schur complements only): afterwards fill the interior nodes of every cell too
        (recover_cell_interiors), so that what the FEM path offers after a solve - the penalisation-point rows, per-strut
        results, the VTU export - works on the result."""
        if not self.domain_decomposition_solver:
            raise ValueError("LatticeSim was not created with enable_domain_decomposition_solver=True")
        if self.thermal is not None:
            raise ValueError("solve_DDM: thermal loads need the FEM strut model (the cell matrices carry no strut "
                             "temperatures); clear_temperature() first")
        dev = self.ddm_model()
        if self._ddm_precond in (1, 3, 4) and not getattr(self, "_precond_note_done", False):
            print(f"solve_DDM: {6 * (self.max_index_boundary + 1)} boundary dofs exceed the {DDM_DENSE_MAX} the device "
                  "factorises densely for the assembled-Schur preconditioner; running CG preconditioned by its node blocks"
                  + (" and a dense level on aggregates of nodes" if self._ddm_precond == 4 else "") +
                  " to the same tolerance (max_iterations of the preset then only applies if larger than 20000)")
            self._precond_note_done = True
        bn = self._boundary_nodes_by_index()
        fixed = self.fixed_DOF[bn]
        if (~fixed).sum() == 0:
            raise ValueError("No free DOF in the lattice. Process aborted.")
        ubar = np.where(fixed, self.displacement_vector[bn], 0.0)
        f = self.applied_force[bn]
        dev.set_bc(fixed, ubar, f)
        dev.assemble()
        b = np.where(fixed, 0.0, f - dev.spmv(ubar))
        if not b.any():       # (not np.linalg.norm: a threaded BLAS dot whose spinning worker threads starve the HIP runtime's
                              #  helper threads - measured at 32^3 cells: 12 ms in the norm and +70 ms in every other solve)
            print("No external forces or imposed displacements in the lattice. Process aborted.")
            return None, None, None, None
        maxit = self.number_iteration_max or 1000
        if self._ddm_precond in (1, 3, 4):
            # presets written for the LU-preconditioned CG cap it at a handful of iterations; the block-Jacobi CG that
            # replaces it above the dense limit needs O(sqrt(cond)) of them to reach the same 1e-6
            maxit = max(maxit, 20000)
        u, st = dev.solve(rtol=1e-6, max_iter=maxit, raise_on_noconv=False)
        if self._ddm_precond == 2 and int(st["precond_used"]) != 2:
            # the assembled matrix was not positive definite (surrogate matrices far from their training points can be
            # indefinite): the device ran Jacobi CG; give it the room the factorised preconditioner would not need
            if not getattr(self, "_spd_note_done", False):
                print("solve_DDM: the assembled Schur preconditioner is not positive definite (indefinite surrogate "
                      "matrix?); Jacobi-preconditioned CG instead")
                self._spd_note_done = True
            if not st["converged"] and maxit < 20000:
                u, st = dev.solve(rtol=1e-6, max_iter=20000, raise_on_noconv=False)
        self.iteration = st["iterations"]
        info = int(st["info"])               # 0 converged, 1 not, 2 not and a step fell below 1e-6 (the reference's codes)
        if info and self._verbose > -1:
            print(f"Conjugate Gradient did not converge ({self.iteration} iterations, relative residual "
                  f"{st['rel_residual']:.2e}).")
        self.displacement_vector[bn] = u
        self.reaction_force_vector[bn] = dev.reactions(u)
        if recover_interior:
            self.recover_cell_interiors()
            if self.is_penalized:
                # penalisation points: back-substituted now, on a handle of the struts as they are at this moment (a
                # deferred evaluation could meet radii or segments changed since the solve)
                from ._capi import HipLattice
                lat, pen = self.lattice, self.penalized
                with HipLattice(lat.node_xyz, lat.beam_conn, lat.beam_radius, pen.seg_len, pen.seg_nsub,
                                self.young_modulus, self.poisson_ratio, pen_coef=self.penalization_coefficient) as fem:
                    fem.assemble()
                    per_strut = fem.node_mod(self.displacement_vector)
                self._node_mod_pending, self._node_mod_stale = None, False
                self.set_node_mod_displacement(per_strut)
        xsol, idx = self.get_global_displacement()
        return xsol, info, self.global_displacement_index, b[~fixed]

    def _boundary_nodes_by_index(self):
        bn = np.empty(self.max_index_boundary + 1, np.int64)
        nodes = np.flatnonzero(self.index_boundary >= 0)
        bn[self.index_boundary[nodes]] = nodes
        return bn


# -- design-side attributes of the reference's base class (lattice.py:58-60, 346-385), for every class on the array model
def _design_properties(cls):
    from statistics import mean
    cls.size_x = property(lambda self: float(self.x_max - self.x_min))
    cls.size_y = property(lambda self: float(self.y_max - self.y_min))
    cls.size_z = property(lambda self: float(self.z_max - self.z_min))

    def get_relative_density(self) -> float:
        """Mean of the cells' relative densities (lattice.py:346-360)."""
        return float(mean(c.relative_density for c in self.cells))

    def get_beam_radius_min_max(self):
        r = self.lattice.beam_radius
        return float(r.max()), float(r.min())

    def getName(self):
        return getattr(self, "name_lattice", "lattice")
    cls.get_relative_density = get_relative_density
    cls.get_beam_radius_min_max = get_beam_radius_min_max
    cls.getName = getName


_design_properties(LatticeSim)
