#!/bin/bash
# Build the kernels' host code with ASan + UBSan (host side only) and run the shape sweep on the CPU
# (arguments go to the program: --dw-plans prints the depthwise launch plans instead).
set -euo pipefail
ROOT="$(cd "$(dirname "$0")/../.." && pwd)"
OUT="$ROOT/build/asan"
mkdir -p "$OUT"
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
SAN="-Xarch_host -fsanitize=address -Xarch_host -fsanitize=undefined -Xarch_host -fno-omit-frame-pointer"
SRCS="dw_plan dw_fwd dw_bwd_s1 dw_bwd_s2 pwgemm pwtall pwbwd block stem se head tokenlearner transformer gradnorm adam"
pids=()
objs=("$OUT/host_checks.o")
for s in $SRCS; do
  src="$ROOT/pytorch_rt1_for_distributed_training_amd/csrc/kernels/$s.hip"
  obj="$OUT/$s.o"
  objs+=("$obj")
  stale=0
  for dep in "$src" "$ROOT"/pytorch_rt1_for_distributed_training_amd/csrc/kernels/common.h "$ROOT"/pytorch_rt1_for_distributed_training_amd/csrc/kernels/dw/*.h; do
    if [ ! -f "$obj" ] || [ "$dep" -nt "$obj" ]; then stale=1; fi
  done
  if [ "$stale" = 1 ]; then
    $HIPCC --offload-arch=gfx950 -std=c++17 -O1 -g $SAN -c "$src" -o "$obj" &
    pids+=($!)
  fi
done
for p in "${pids[@]}"; do wait "$p"; done
$HIPCC -std=c++17 -O1 -g $SAN -c "$ROOT/tools/host_asan/host_checks.cpp" -o "$OUT/host_checks.o"
$HIPCC --offload-arch=gfx950 -fsanitize=address,undefined -fno-gpu-sanitize -o "$OUT/host_checks" "${objs[@]}"
ASAN_OPTIONS=detect_leaks=0:abort_on_error=1 UBSAN_OPTIONS=halt_on_error=1:print_stacktrace=1 "$OUT/host_checks" "$@"
