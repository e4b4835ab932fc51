# Counters of the fast film's gather kernel on the headline, before / after style (run on the GPU box):
#   [OUT_DIR=dir] bash tools/profile_film_gather.sh <tag> [rounds]     -> <dir, default build/profile>/prof_<tag>/<tag>_film_gather_counters.json
# `rounds` sets NORI_HIP_FILM_GATHER=rounds (film_gather_kernel for every border: the "before").  Like tools/profile_round.sh:
# each counter pass is its own rocprofv3 run (--kernel-trace --pmc only) of ONE render pass (tools/wf_probe.py, REPS=1); a pass
# that fails ends the script.
set -u
TAG=${1:-film}
[ "${2:-}" = "rounds" ] && export NORI_HIP_FILM_GATHER=rounds
ROOT=$(cd $(dirname $0)/.. && pwd)
cd $ROOT && export TMPDIR=/tmp
OUT=$(mkdir -p ${OUT_DIR:-build/profile} && cd ${OUT_DIR:-build/profile} && pwd)/prof_$TAG
mkdir -p $OUT
export REPS=1 WORKLOAD=${WORKLOAD:-pa4-cbox-path_mis} ENGINE=wavefront
run_pass() {
  local NAME=$1; shift
  timeout -k 10 600 rocprofv3 --kernel-trace --pmc "$@" --output-format csv -d /tmp/prof_$NAME -o c -- python tools/wf_probe.py > $OUT/${NAME}.log 2>&1 || { tail -20 $OUT/${NAME}.log; echo "pass $NAME failed"; exit 1; }
  find /tmp/prof_$NAME -name '*counter_collection.csv' -exec cp {} $OUT/${NAME}_counter_collection.csv \;
  rm -rf /tmp/prof_$NAME
}
run_pass lds SQ_INSTS_VALU SQ_INSTS_LDS SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_WAVE_CYCLES SQ_BUSY_CYCLES
run_pass elapsed GRBM_GUI_ACTIVE FETCH_SIZE
python tools/summarize_film_gather.py $OUT $TAG | tee $OUT/${TAG}_film_gather_counters.json
