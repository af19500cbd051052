"""Kernel averages of one rocprofv3 kernel trace, per kernel AND grid size (the headline lattice and the large one of
bench.py --full launch the same kernels on different grids).  usage: trace_by_grid.py TRACE.csv"""
import csv, sys, collections
rows = list(csv.DictReader(open(sys.argv[1])))
gk = [k for k in rows[0] if k.startswith("Grid_Size")]
acc = collections.defaultdict(list)
for r in rows:
    n = r["Kernel_Name"]
    if not any(s in n for s in ("k_pcg_direction_flat", "k_pcg_update_tile", "k_spmv_tile_lds<", "k_full_gemv", "k_pcg_direction_coarse")):
        continue
    acc[(n[:78], "x".join(r[k] for k in gk))].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
print(f"{'kernel':78s} {'grid':>14s} {'calls':>6s} {'avg us':>9s} {'median':>9s} {'max':>9s}")
for (n, g), v in sorted(acc.items(), key=lambda kv: -len(kv[1])):
    v.sort()
    print(f"{n:78s} {g:>14s} {len(v):6d} {sum(v) / len(v):9.2f} {v[len(v) // 2]:9.2f} {v[-1]:9.2f}")
