#!/bin/bash
# Round 6's one-call experiments as modes of ONE script (no more r<N>_*.sh files):   bash profiles/experiments.sh <mode>
# Every mode is what ran in one call; results and readings are under profiles/r06/ (a_ ... f_).  Some modes load variant libraries that are
# not part of the product build (python profiles/build_variant.py <name> <-D flags>: see the mode).  The modes of the retired kernel forms
# (in-wave fan-out of split parts, TAA inside the trace launch) went with those forms; the parent of their removal still has them.
# Modes: suite, resolve, split2, costframes, zerolast
REPO=${GRAFT_REPO_ROOT:-/root/repo}; cd $REPO; mkdir -p gpurun_out
L=$REPO/yetanotherconsolegameengine_amd/lib

# round 6: the GPU suite on the build of the hour + the heaviest blocks in TWO parts (YCGE_SPLIT_TOP_LG=1), same call
mode_suite() {
  timeout 2700 python -m pytest tests -m gpu -q > gpurun_out/r6_suite_pytest.log 2>&1; echo "pytest rc=$?"; tail -6 gpurun_out/r6_suite_pytest.log
  for cfg in 4 3; do
    echo "== config $cfg"
    for spec in "32 2" "64 1" "128 1" "256 1" "512 1" "32 2"; do set -- $spec
      YCGE_SPLIT_TOP=$1 YCGE_SPLIT_TOP_LG=$2 timeout 200 python profiles/sync_ms.py $cfg 300 "split_top=$1 parts=2^$2" 2>&1 | tail -1; done
  done
}

# round 6: the tile-resident resolve as ONE launch (k_resolve_tiles) against round 5's two; hardware queues per stream; a rank's period frame by frame
mode_resolve() {
  timeout 900 python -m pytest tests/test_gpu_parity.py -m gpu -x -q -k "tile_resident" 2>&1 | tail -3
  run() { echo -n "$1 | world $2 K=$3: "; ( for kv in $1; do export "$kv"; done; timeout 300 python profiles/rank_flight.py 4 $2 residentc $3 2>&1 | tail -1 | cut -c75-210 ); }
  for w in 8 4; do
    run "A=one_launch" $w 4
    run "YCGE_RES_SPLIT_RESOLVE=1" $w 4
    run "GPU_MAX_HW_QUEUES=8" $w 4
    run "GPU_MAX_HW_QUEUES=8 YCGE_RES_SPLIT_RESOLVE=1" $w 4
    run "GPU_MAX_HW_QUEUES=8" $w 6
    run "GPU_MAX_HW_QUEUES=8" $w 8
    run "GPU_MAX_HW_QUEUES=16" $w 8
    run "A=one_launch" $w 6
    run "YCGE_RES_LOOP_COMM=slot" $w 4
    run "GPU_MAX_HW_QUEUES=8 YCGE_RES_LOOP_COMM=slot" $w 4
    run "GPU_MAX_HW_QUEUES=8 YCGE_RES_LOOP_COMM=slot" $w 8
  done
  echo "== ring 1 (latency 1: the synchronous form of a rank)"; run "A=one_launch" 8 2
}

# round 6: the new split default (two parts, count by block count) against round 5's (32 blocks in four), the spread of frame times with the SAME frame
# number every frame (same rays) against consecutive frames, the GPU suite on this build
mode_split2() {
  timeout 2700 python -m pytest tests -m gpu -q > gpurun_out/r6_split2_pytest.log 2>&1; echo "pytest rc=$?"; tail -4 gpurun_out/r6_split2_pytest.log
  for cfg in 4 3; do
    echo "== config $cfg"
    YCGE_SPLIT_TOP=32 YCGE_SPLIT_TOP_LG=2 timeout 200 python profiles/sync_ms.py $cfg 300 "round 5: 32 x 4 parts" 2>&1 | tail -1
    timeout 200 python profiles/sync_ms.py $cfg 300 "default" 2>&1 | tail -1
    YCGE_SPLIT_TOP=32 YCGE_SPLIT_TOP_LG=2 timeout 200 python profiles/sync_ms.py $cfg 300 "round 5: 32 x 4 parts" 2>&1 | tail -1
    timeout 200 python profiles/sync_ms.py $cfg 300 "default" 2>&1 | tail -1
    SAME_FRAME=40 timeout 200 python profiles/sync_ms.py $cfg 300 "default, frame 40 every time" 2>&1 | tail -1
    SAME_FRAME=41 timeout 200 python profiles/sync_ms.py $cfg 300 "default, frame 41 every time" 2>&1 | tail -1
    SAME_FRAME=42 timeout 200 python profiles/sync_ms.py $cfg 300 "default, frame 42 every time" 2>&1 | tail -1
  done
}

# round 6: frames of history behind a block's schedule cost (maximum over the last n frames; 4 in the product), synchronous frames, same call
mode_costframes() {
  for cfg in 4 3; do
    echo "== config $cfg"
    timeout 200 python profiles/sync_ms.py $cfg 300 "history 4 (product)" 2>&1 | tail -1
    for n in 2 3 6 8; do YCGE_LIB=$L/var_cost$n.so timeout 200 python profiles/sync_ms.py $cfg 300 "history $n" 2>&1 | tail -1; done
    timeout 200 python profiles/sync_ms.py $cfg 300 "history 4 (product)" 2>&1 | tail -1
  done
}

# round 6: the schedule's last class is cost ZERO alone (sky) - against round 5's classes (var_order5.so: -DYCGE_ORDER_ZERO_LAST=0); timing events only with statistics
mode_zerolast() {
  for cfg in 4 3; do
    echo "== config $cfg"
    for rep in 1 2; do
      YCGE_LIB=$L/var_order5.so timeout 200 python profiles/sync_ms.py $cfg 300 "round 5's order classes" 2>&1 | tail -1
      timeout 200 python profiles/sync_ms.py $cfg 300 "zero-cost blocks last" 2>&1 | tail -1
    done
    NO_STATS=1 timeout 200 python profiles/sync_ms.py $cfg 300 "zero-cost blocks last, no statistics asked for (no timing events)" 2>&1 | tail -1
    timeout 200 python profiles/sync_ms.py $cfg 300 "zero-cost blocks last" 2>&1 | tail -1
  done
  timeout 300 python profiles/mega_prof.py 4 2>&1 | grep -v amdgpu.ids > gpurun_out/r6_mega_prof_zerolast.txt; grep -E "trace_ms|span|slot time|>= 256|blocks split" gpurun_out/r6_mega_prof_zerolast.txt; sed -n 7,16p gpurun_out/r6_mega_prof_zerolast.txt
  timeout 600 python -m pytest tests/test_gpu_timed_variants.py -m gpu -x -q -k "steady or mesh or frames_in_flight" 2>&1 | tail -2
}

case "$1" in
  suite|resolve|split2|costframes|zerolast) mode_$1 ;;
  *) echo "usage: bash profiles/experiments.sh <suite|resolve|split2|costframes|zerolast>"; exit 2 ;;
esac
