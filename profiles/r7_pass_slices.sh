#!/bin/bash
# Pass slices of the megakernel (profiles/r7_pass_slices.md): step 0 on any library, then the slice sweep on the headline run and on an
# eighth of the frame. HYDRA_HIP_LIB selects the library (a parent build for the A/B); HPT_PASS_SLICE (diagnostic) sets the passes per work
# item, since bench.py sets no options. Every step has its own time limit and the first failure ends the script.
# --no-cpu-baseline / --no-also are not passed: they only act with --full, which these runs do not use.
# Usage: profiles/r7_pass_slices.sh [parent-library.so]
set -eu
cd "$(dirname "$0")/.."
B="timeout -k 10 150 python bench.py --gpus 1 --steps 3 --warmup 1 --no-build"
for round in 1 2; do
  $B
  $B --width 2048 --height 2048 --spp 256
  $B --width 512 --height 512 --spp 4096
  for k in 2 4 8; do $B --emulate-share $k; done
done
for share in 1 4 8; do
  if [ -n "${1:-}" ]; then HYDRA_HIP_LIB="$1" $B --emulate-share $share; fi
  for s in 0 16 32 64 128 256 512; do HPT_PASS_SLICE=$s $B --emulate-share $share; done
done
for s in 0 128 256; do HPT_PASS_SLICE=$s $B --spp 512; done
