set -o pipefail
out=${OUT:-bench_out}/rpd
mkdir -p $out
for v in product rpd4 rpd8 product rpd4 rpd8; do
  lib=deep-rawburst-sr_amd/libdbsr_hip.so; [ "$v" != product ] && lib=deep-rawburst-sr_amd/libdbsr_hip_$v.so
  DBSR_HIP_LIB=$lib timeout -k 10 200 python bench.py --full --mode train --kernel-breakdown --no-cpu-baseline --steps 10 > $out/$v.json 2> $out/$v.err || { echo "$v failed"; tail $out/$v.err; exit 1; }
  echo "$v $(python -c "import json;print(json.load(open('$out/$v.json'))['ms_per_step'])") $(grep -E '^bwd.proj.oth ' $out/$v.err)"
done
