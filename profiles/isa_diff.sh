#!/bin/bash
# Are the kernels of two builds the same code? Compares the gfx950 disassembly of translation units of two object directories with the symbol
# names removed (a template parameter added to a kernel changes every mangled name and nothing else).
#   profiles/isa_diff.sh <build dir A> <build dir B> [unit ...]      e.g.  profiles/isa_diff.sh ../parent/hydracore3_amd/build hydracore3_amd/build pt1 pt2 wf_trace
# Prints one line per unit: "same" or "DIFFERENT"; exit status 1 if any differs.
set -o pipefail
LLVM=${LLVM:-/opt/rocm/llvm/bin}
A=$1; B=$2; shift 2
UNITS=${*:-pt1 pt2 pt6 pt9 pt14 pt16 wf_shade wf_trace stream bw_fwd bw_dr}
TMP=$(mktemp -d); trap 'rm -rf "$TMP"' EXIT
dis() {   # object file -> name-free disassembly of its gfx950 code object
  "$LLVM/llvm-objcopy" -O binary --only-section=.hip_fatbin "$1" "$TMP/x.fatbin" &&
  "$LLVM/clang-offload-bundler" --unbundle --type=o --targets=hipv4-amdgcn-amd-amdhsa--gfx950 --input="$TMP/x.fatbin" --output="$TMP/x.co" &&
  "$LLVM/llvm-objdump" -d --no-show-raw-insn "$TMP/x.co" | grep -v "file format" | sed 's/<[^>]*>//g; s/^ *[0-9a-f]*://; s/\/\/.*//; s/^[0-9a-f]* *$//'
}
rc=0
for u in $UNITS; do
  a=$(dis "$A/$u.o" | md5sum) || exit 2
  b=$(dis "$B/$u.o" | md5sum) || exit 2
  if [ "$a" = "$b" ]; then echo "$u same"; else echo "$u DIFFERENT"; rc=1; fi
done
exit $rc
