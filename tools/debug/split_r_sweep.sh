# cfg2 at per-GPU batch 8 / 16 / 64 with conv_split strips of 8 / 16 / 32 rows (DL4DS_SPLIT_R, a test hook) -> OUT_DIR (round 6: 16 rows only where 32 leave CUs idle)
# Usage: tools/debug/split_r_sweep.sh OUT_DIR
O=${1:?usage: tools/debug/split_r_sweep.sh OUT_DIR}
mkdir -p $O
export DL4DS_TEST_HOOKS=1
for B in 8 16 64; do for R in 8 16 32; do
  DL4DS_SPLIT_R=$R DL4DS_BENCH_BREAKDOWN=1 python bench.py --full --batch $B --no-cpu-baseline --no-unfolded --no-b16 > $O/b${B}_r$R.json 2> $O/b${B}_r$R.err
done; done
python - "$O" <<'PY'
import json,glob,os,sys
for f in sorted(glob.glob(os.path.join(sys.argv[1], '*.json'))):
    try:
        j=json.loads(open(f).read().strip().splitlines()[-1]); b=j['breakdown']
        print(f, round(j['value'],1), round(j['ms_per_step'],3), {k:round(v['ms_per_step'],3) for k,v in b.items() if k.startswith(('conv_split','conv_wino<3,3>'))})
    except Exception as e: print(f,'ERR',e)
PY
