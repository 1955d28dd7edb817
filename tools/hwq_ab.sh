#!/bin/bash
# A/B of the pipelined step against the size of the runtime's hardware-queue pool: bench.py at 1 and at 64 streams with GPU_MAX_HW_QUEUES as
# the machine has it (unset = the runtime's 4) and with 8 exported, alternated three times.  One line per run is appended to the report.
#
#   tools/hwq_ab.sh [-o REPORT] [-n REPS] [-s "1 64"] [-t SECONDS] [NAME="VAR=value VAR=value" ...]
#
# Every NAME=... argument is one leg: the assignments are put in front of the bench.py command (empty: the environment as it is).  Default legs:
#   default=""  q8="GPU_MAX_HW_QUEUES=8"
# Other uses: another checkout with its own build (SVA_BENCH=/path/to/checkout/bench.py: that bench.py is run instead), another way of creating the chain streams
# (SVA_DEBUG=stream_queues=0|1|2, csrc/engine.hip get_streams).  Each run has its own time limit; the script stops at the first run that fails.
cd "$(dirname "$0")/.." || exit 1
OUT=profiles/hw_queues_report.txt
REPS=3
STREAMS="1 64"
LIMIT=240
while getopts "o:n:s:t:" opt; do
    case $opt in
        o) OUT=$OPTARG ;;
        n) REPS=$OPTARG ;;
        s) STREAMS=$OPTARG ;;
        t) LIMIT=$OPTARG ;;
        *) exit 2 ;;
    esac
done
shift $((OPTIND - 1))
LEGS=("$@")
[ ${#LEGS[@]} -eq 0 ] && LEGS=("default=" "q8=GPU_MAX_HW_QUEUES=8")
mkdir -p "$(dirname "$OUT")"
LOG=$(mktemp)
trap 'rm -f "$LOG"' EXIT
for B in $STREAMS; do
    for rep in $(seq 1 "$REPS"); do
        for leg in "${LEGS[@]}"; do
            name=${leg%%=*}
            assign=${leg#*=}
            # shellcheck disable=SC2086
            bench=$(env $assign sh -c 'echo ${SVA_BENCH:-bench.py}')
            # shellcheck disable=SC2086
            env $assign timeout -k 10 "$LIMIT" python "$bench" --gpus 1 --streams "$B" > "$LOG" 2>&1
            rc=$?
            if [ $rc -ne 0 ]; then
                echo "hwq_ab streams=$B rep=$rep leg=$name [$assign] FAILED rc=$rc" | tee -a "$OUT"
                tail -n 15 "$LOG"
                exit $rc
            fi
            value=$(grep '^{' "$LOG" | tail -n 1 | python -c 'import json, sys; print(json.loads(sys.stdin.readline())["value"])')
            queues=$(env $assign sh -c 'echo ${GPU_MAX_HW_QUEUES:-unset}')
            echo "hwq_ab streams=$B rep=$rep leg=$name GPU_MAX_HW_QUEUES=$queues [$assign] frames/s=$value" | tee -a "$OUT"
        done
    done
done
