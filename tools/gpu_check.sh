# Parity + N>1 rehearsal on one MI355X (run through gpurun from the repo root).
set -o pipefail
mkdir -p gpurun_out
timeout -k 10 600 python -m pytest tests -m gpu -x -q > gpurun_out/pytest_gpu.log 2>&1 || exit 1
bash tools/gpu_steps.sh -x "300 bench_torchrun1.log python -m torch.distributed.run --nnodes=1 --nproc-per-node 1 --master-addr 127.0.0.1 --master-port 29511 bench.py --full --gpus 1 --steps 10 --warmup 2 --cpu-seconds 0 --no-pcie" || exit 2
bash tools/gpu_steps.sh -x "300 bench_gloo2.log python -m torch.distributed.run --nnodes=1 --nproc-per-node 2 --master-addr 127.0.0.1 --master-port 29512 bench.py --full --gpus 2 --steps 10 --warmup 2 --dist-backend gloo --records 4194304" || exit 3
