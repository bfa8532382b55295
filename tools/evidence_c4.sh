#!/bin/bash
# c4 evidence in the order that lets the graded line carry the counters of THIS tree: PMC passes first (they rewrite
# profiles/<tag>_{traffic,valu}_c4.json, which bench.py attaches), then the bench command with --full; everything copied to $RESULTS/prof/ (default results/prof/)
T=${1:-r04}
RESULTS=${RESULTS:-results}
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
mkdir -p $RESULTS/prof profiles
bash tools/pmc_profile.sh c4 $T 1 > $RESULTS/prof/pmc_c4.log 2>&1
tail -25 $RESULTS/prof/pmc_c4.log
( time timeout -k 5 2400 python bench.py --gpus 1 --steps 20 --warmup 5 --full > $RESULTS/prof/bench_c4_default.json ) 2> $RESULTS/prof/bench_c4_default.log
tail -6 $RESULTS/prof/bench_c4_default.log
cp profiles/${T}_*c4* $RESULTS/prof/
