# A/B of the BiLSTM forward-step k-loop pipeline (PPO_LSTM_STEP_PIPE 1 / 2), alternating
set -o pipefail
export PPO_BENCH_FULL=1  # = bench.py --full: the per-kernel figures and legs read below are measured only then
for rep in 1 2; do
for c in 1 2; do
  PPO_LSTM_STEP_PIPE=$c timeout -k 10 300 python bench.py --model lstm --steps 3 --warmup 1 --no-cpu-baseline \
    > gpurun_out/lstm_pipe_${TAG}_${c}_$rep.json 2> gpurun_out/lstm_pipe_${TAG}_${c}_$rep.err || exit 1
  python -c "import json;d=json.load(open('gpurun_out/lstm_pipe_${TAG}_${c}_$rep.json'));k=d['kernels_ms_per_step'];print($c, round(d['ms_per_step'],1), {n:round(v,1) for n,v in k.items() if 'step_fwd' in n})"
done
done
