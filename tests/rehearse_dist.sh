# Multi-rank rehearsal on a one-GPU box: two ranks share the GPU, the exchanges go over gloo
# (bench.py --dist-backend gloo), then the N=1 bench line.
set -o pipefail
BENCH_OUT=${BENCH_OUT:-bench_out}   # where the two bench lines go
mkdir -p "$BENCH_OUT"
timeout -k 10 300 python -m torch.distributed.run --nnodes=1 --nproc-per-node 2 --master-addr 127.0.0.1 --master-port 29517 bench.py --full --gpus 2 --steps 3 --warmup 1 --batch 32 --dist-backend gloo > "$BENCH_OUT/rehearse2.json" 2> "$BENCH_OUT/rehearse2.err" && echo rehearse ok && \
timeout -k 10 600 python bench.py --full > "$BENCH_OUT/bench.json" 2> "$BENCH_OUT/bench.err" && echo bench ok
