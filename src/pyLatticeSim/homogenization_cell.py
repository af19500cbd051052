"""``from pyLatticeSim.homogenization_cell import HomogenizedCell`` (reference: src/pyLatticeSim/homogenization_cell.py:60);
``fit_cell_radii`` has no counterpart in the reference."""
from pylatticedso_amd.homogenization_cell import HomogenizedCell, directional_modulus, fit_cell_radii  # noqa: F401
