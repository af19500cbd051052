set -o pipefail
O=${1:-.exp/r05_r}; mkdir -p "$O"
python -m pytest tests/test_gpu_parity.py -q -x -k "float_lever or assembly_schedules or strain_mode or lds_resident" > $O/pytest.log 2>&1; tail -3 $O/pytest.log
for rep in 1 2; do
PL_NO_REL32=1 python bench.py --gpus 1 --steps 20 --warmup 5 --full --no-other --no-e2e --no-streaming > $O/off$rep.json 2>/dev/null
python bench.py --gpus 1 --steps 20 --warmup 5 --full --no-other --no-e2e --no-streaming > $O/on$rep.json 2>/dev/null
done
PL_NO_REL32=1 python bench.py --config 2 --steps 3 --warmup 1 --full --no-other --no-e2e --no-streaming > $O/c2off.json 2>/dev/null
python bench.py --config 2 --steps 3 --warmup 1 --full --no-other --no-e2e --no-streaming > $O/c2on.json 2>/dev/null
python - "$O" <<PY
import json,glob,sys
for f in sorted(glob.glob(sys.argv[1] + "/*.json")):
    try:
        d=json.loads(open(f).read().strip().splitlines()[-1])
        print(f, round(d["value"]/1e6,2), round(d["ms_per_step"],3), d["kernels_ms"].get("pcg_iteration"), d["kernels_ms"].get("spmv"))
    except Exception as e:
        print(f, "failed", e)
PY
