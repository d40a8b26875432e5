#!/bin/bash
# A/B timing of two builds of libgrlx.so on the SAME GPU box (box-to-box spread is ~6 %, run-to-run on one
# box ~0.1 %): ab_bench.sh <libA.so> <libB.so> [rounds] [bench args...]   -- alternates A, B, A, B, ...
# Every run has a time limit of its own (AB_TIMEOUT seconds, default 300) and the first run that fails, faults or
# runs into it ends the script: nothing more is started on a device that may be in trouble.
set -o pipefail
A=$1; B=$2; N=${3:-3}; shift; shift; shift || true
for i in $(seq 1 $N); do
  for L in "$A" "$B"; do
    GRLX_LIB=$(realpath $L) timeout -k 10 ${AB_TIMEOUT:-300} python bench.py --no-cpu-baseline "$@" | python -c "import sys,json; d=json.loads(sys.stdin.read()); print('$L  %.1f M env-steps/s  %.3f ms  learn_steps %s/%s  served %s' % (d['value']/1e6, d['ms_per_step'], d.get('learn_steps'), d.get('learn_steps_expected'), d.get('env_server')))" || exit 1
  done
done
