#!/bin/bash
# first halo ring in 64 bytes: invariants, parity subset, noisy search times, transient
cd "$(dirname "$0")/.."; mkdir -p out
timeout 900 python -m pytest tests/test_gpu_tree_invariants.py tests/test_gpu_seeded.py tests/test_gpu_fuzz.py tests/test_gpu_parity.py -m gpu -x -q 2>&1 | tail -5 > out/h_tests.log
timeout 300 python scripts/measure_noisy.py > out/h_noisy.log 2>&1
timeout 300 python scripts/dev/transient_census.py > out/h_transient.log 2>&1
timeout 300 python bench.py --full --steps 100 --warmup 20 > out/h_bench.log 2>&1
tail -3 out/h_tests.log; tail -8 out/h_noisy.log; tail -5 out/h_transient.log; tail -1 out/h_bench.log
