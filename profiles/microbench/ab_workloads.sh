# A/B on one box beyond the headline's step: the full bench line (sensitivity legs, resident re-run, one-shot stream), the
# 2x150 shape (the WIDE instantiation) or config4 on one GPU, for the product build and build_var/lib_<name>.so variants, three
# rounds interleaved, every run a process of its own.
#     bash profiles/microbench/ab_workloads.sh full|2x150|config4 <name> [<name> ...]
R=$(cd "$(dirname "$0")/../.." && pwd); cd $R
leg=$1; shift
case $leg in
  full)    args="--steps 60" ;;
  2x150)   args="--steps 60 --no-sensitivity --lq 150 --lr 590 --reads 100 --fusions 5000" ;;
  config4) args="--steps 10 --no-sensitivity --workload config4 --gpus 1" ;;
  *) echo "unknown leg $leg"; exit 2 ;;
esac
for round in 1 2 3; do
  for v in product "$@"; do
    if [ $v = product ]; then unset DEFUSE_DSA_LIB; else export DEFUSE_DSA_LIB=$R/build_var/lib_$v.so; fi
    timeout -k 10 400 python bench.py --no-cpu-baseline --warmup 3 $args 2>/dev/null | python -c "
import sys, json
d = json.loads(sys.stdin.readline())
s = '$leg $round %-9s step %.4f fill %.4f finish %.4f rerun_step %.4f' % ('$v', d['ms_per_step'], d['stage_ms']['fill'], d['stage_ms']['finish'], d['resident_rerun']['ms_per_step'])
if 'one_shot' in d:
    s += ' one_shot ' + ' '.join('%s %.3f' % (k, v) for k, v in d['one_shot'].items() if k.startswith('ms_per'))
for k, v in d.get('sensitivity', {}).items():
    if isinstance(v, dict) and 'ms_per_step' in v:
        s += ' %s %.4f' % (k, v['ms_per_step'])
print(s)" || exit 1
  done
done
