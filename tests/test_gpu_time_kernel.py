"""pl_time_kernel runs what the solve runs: ids 10 and 11 (and 7, 8, 9 on the fp32-stored vectors) call the same operator
apply and the same iteration as pl_solve, on the handle's own buffers.  So a handle that has been timed must still solve as
before: the same plan (preconditioner, storage width, form of the iteration, eliminated nodes), the same iteration count
up to the run-to-run spread of the atomic sums (+-3, as tests/test_gpu_ddm.py allows) and the same displacements.

The iteration count is not compared in precision = 2: there the count is a sum of whole chunks of the look schedule
(pl_schedule.h), and repeated solves on one handle give 289 ... 295 iterations whether or not the handle is timed in between
(measured on an MI355X, 16 solves in a row, before and after the solver's host side was restructured: consecutive solves
differ by up to 5).  precision = 0 gives 220 / 221, precision = 1 always 248.

Lattice: bcc_6x3x3 with boundary set b, the recorded partition (oracle/precond_cases.py) - the smallest case here with at
least 4 tiles and 2 aggregates."""
import pytest

pytestmark = pytest.mark.gpu

from oracle import precond_cases as C, precond_oracle as P      # noqa: E402

NAME, BSET, TM, CM = "bcc_6x3x3", "b", 12, 6


@pytest.mark.parametrize("short_iteration", [-1, 1])
@pytest.mark.parametrize("precision", [0, 1, 2])
@pytest.mark.parametrize("condense", [-1, 1])
def test_a_timed_handle_solves_as_before(condense, precision, short_iteration):
    lat = C.Lattice(NAME)
    fixed, ubar, f, _ = C.boundary_set(BSET, lat, C.recorded_partition(NAME, CM))
    opts = dict(precond=3, coarse_max_dofs=C.COARSE_MAX_DOFS[CM], tile_modes=TM, coarse_modes=CM, coarse_storage=32,
                tile_nodes=C.TILE_NODES[NAME], condense=condense, precision=precision, short_iteration=short_iteration,
                warm_start=0)
    if short_iteration == 1:
        opts["palette"] = 1
    with lat.device(**opts) as dev:
        dev.set_bc(fixed, ubar, f)
        dev.assemble()
        u1, st1 = dev.solve(rtol=1e-8)
        ids = [0, 3, 10, 11] + ([7, 8, 9] if int(st1["precond_used"]) >= 2 else [])
        times = {i: dev.time_kernel(i, 2) for i in ids}
        u2, st2 = dev.solve(rtol=1e-8)
    keys = ("precond_used", "precision_used", "short_iteration_used", "condensed_nodes")
    dev_u = P.rel(u2, u1)
    print(f"TIMED_HANDLE condense={condense} precision={precision} short={short_iteration} "
          f"plan={[st1[k] for k in keys]} iterations={st1['iterations']}/{st2['iterations']} rel={dev_u:.3e} "
          f"ms={' '.join(f'{i}:{t:.4f}' for i, t in times.items())}")
    assert st1["converged"] and st2["converged"]
    assert all(t > 0.0 for t in times.values()), times
    assert [st2[k] for k in keys] == [st1[k] for k in keys], ([st1[k] for k in keys], [st2[k] for k in keys])
    if precision != 2:
        assert abs(int(st2["iterations"]) - int(st1["iterations"])) <= 3, (st1["iterations"], st2["iterations"])
    assert dev_u < 1e-6, dev_u
