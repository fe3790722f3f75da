# A/B of the Humanoid shard's paired WGRAD / DGRAD launch LDS stages (PPO_WIDE_PAIR_NS 2 / 4 / 5)
set -o pipefail
export PPO_BENCH_FULL=1  # = bench.py --full: the per-kernel figures and legs read below are measured only then
A="--num-envs 1024 --obs-dim 376 --act-dim 17 --hidden 512,512,512 --batch 8192 --steps 3 --warmup 1 --no-cpu-baseline --no-legs"
for rep in 1 2; do
for c in 2 4 5; do
  PPO_WIDE_PAIR_NS=$c timeout -k 10 300 python bench.py $A > gpurun_out/hum_pair_${TAG}_${c}_$rep.json 2> gpurun_out/hum_pair_${TAG}_${c}_$rep.err || exit 1
  python -c "import json;d=json.load(open('gpurun_out/hum_pair_${TAG}_${c}_$rep.json'));k=d['kernels_ms_per_step'];print($c, round(d['ms_per_step'],2), {n:round(v,2) for n,v in k.items() if 'pair' in n})"
done
done
