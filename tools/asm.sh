#!/bin/bash
# tools/asm.sh <name> [extra hipcc flags...] -> /tmp/kyasm/<name>.s: device assembly of ky_launch.hip (KY_SRC overrides the source; KY_ASM_DEBUG= leaves the line
# tables out: listings of two trees then differ only where their code does, which is what tools/asm_same.py compares)
NAME=$1; shift
BASE="--offload-arch=gfx950 -O3 -std=c++17 -Wno-unused-function -Wno-bitwise-instead-of-logical -fno-slp-vectorize -fno-hip-fp32-correctly-rounded-divide-sqrt"
SRC=${KY_SRC:-ky_amd/csrc/ky_launch.hip}
mkdir -p /tmp/kyasm
hipcc $BASE "$@" -S --cuda-device-only ${KY_ASM_DEBUG--gline-tables-only} -o /tmp/kyasm/$NAME.s $SRC
