#!/bin/bash
# tools/pmc_detector_lp.sh OUTDIR [PRECISION] — what bounds the dense stage's 16-bit kernel: counter-only rocprofv3 --pmc
# passes (never together with a trace domain, the program right behind `--`) over tools/pmc_detector_lp.py run, summed
# per kernel instance into OUTDIR/pmc_conv2d_lp.json (copied to profiles/pmc_conv2d_lp.json). Run ON the GPU box.
# Every pass runs under its own time limit; a pass that fails, faults or times out ends the script (no stale summary).
set -u
R=$(cd "$(dirname "$0")/.." && pwd)
O=${1:?OUTDIR}; PREC=${2:-fp16}
rm -rf "$O"; mkdir -p "$O"
n=0
while read -r counters; do
  n=$((n + 1))
  # shellcheck disable=SC2086
  timeout -k 10 300 rocprofv3 --pmc $counters --output-format csv -d "$O/p$n" -o c -- python3 "$R/tools/pmc_detector_lp.py" run "$PREC" > "$O/p$n.log" 2>&1 < /dev/null
  e=$?
  if [ $e -ne 0 ] || [ -z "$(find "$O/p$n" -name '*counter_collection.csv' 2>/dev/null | head -1)" ]; then
    echo "pmc_detector_lp.sh: pass p$n FAILED (rc $e; see $O/p$n.log); stopping"; exit 1
  fi
done < <(python3 "$R/tools/pmc_detector_lp.py" passes)
python3 "$R/tools/pmc_detector_lp.py" sum "$O" "$O/pmc_conv2d_lp.json"
