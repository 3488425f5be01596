# usage: bash tools/gpu_env_ab.sh "<VAR=a VAR2=b>" "<VAR=c>" ... — same-box A/B of environment settings on the headline config, 3 alternating rounds.
# Stops at the first run that fails or times out: after a fault nothing more is started on that card.
set -o pipefail
mkdir -p gpurun_out
for r in $(seq 1 ${ROUNDS:-3}); do
  for v in "$@"; do
    env $v timeout -k 10 200 python bench.py --config ${CFG:-pong-canonical-b32} --steps 1000 --warmup 200 --no-cpu-baseline --no-profile 2>/dev/null | tail -1 | python -c "import sys,json; d=json.loads(sys.stdin.read()); print('[$v] round $r: %.2f us/step  %.0f steps/s' % (d['ms_per_step']*1e3, d['value']))"
    rc=$?
    if [ $rc -ne 0 ]; then echo "[$v] round $r: FAILED (exit status $rc), stopping" >&2; exit $rc; fi
  done
done
