#!/bin/bash
# A/B developer bench on ONE box: ab.sh "<bench args>" lib1 lib2 ...   (boxes differ by several %, never compare across calls)
# AB_JSON=<file>: every run's result line is appended there behind its library's name (ray counts, checksums, kernel times).
# A run that fails or passes its time limit ends the series: nothing more is started on that GPU.
args=$1; shift
for lib in "$@"; do
  echo "== $lib $args"
  RUSTRAY_HIP_LIB=$PWD/$lib timeout -k 10 ${AB_TIMEOUT:-300} python bench.py --steps 3 --warmup 1 --no-cpu-baseline --no-extras $args 2> /tmp/ab_err.txt > /tmp/ab_out.txt || { echo "bench failed:"; tail -n 3 /tmp/ab_err.txt; exit 1; }
  [ -n "$AB_JSON" ] && echo "$lib $(tail -n 1 /tmp/ab_out.txt)" >> "$AB_JSON"
  python -c "
import json; r=json.loads(open('/tmp/ab_out.txt').read().strip().splitlines()[-1]); print(round(r['value']), round(r['ms_per_step'],3), {k: round(v,2) for k,v in r['kernel_ms_per_frame'].items()}, r['frame_checksum'])"
done
