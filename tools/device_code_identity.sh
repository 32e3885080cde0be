#!/bin/bash
# Is the gfx950 device code of the working tree the same as a revision's?
#   [FILES="pt_abi pt_megakernel ..."] bash tools/device_code_identity.sh REV
# For host-side refactors and added translation units: compiles the
# translation units whose kernels such a change must leave alone (FILES, names
# without .hip; by default the render kernels' four, pt_denoise and pt_guide)
# device-only from REV's csrc/ and include/ and from the working tree's, in the
# shipped and the register-stress build (-DPTMI_STRESS_WAVES=8), and
# compares each code object's disassembly, ELF notes (kernel metadata:
# registers, LDS, scratch, arguments) and sorted kernel descriptor symbols,
# which also pins the order the kernels were instantiated in. (pt_denoise.hip
# is not part of the stress library; it is compiled both ways all the same.)
# The raw code objects are not compared: they differ in the __hip_cuid_<hash>
# symbol, a hash of the source text. Prints a markdown table; exit 0 iff all
# comparisons (three per file and build) are identical. Needs no GPU.
set -eu
REV=$1
ROOT=$(cd "$(dirname "$0")/.." && pwd)
ROCM=${ROCM_PATH:-/opt/rocm}
HIPCC=${HIPCC:-$ROCM/bin/hipcc}
LLVM=$ROCM/lib/llvm/bin
# the Makefile's FLAGS
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -fhip-fp32-correctly-rounded-divide-sqrt -fno-fast-math -fno-slp-vectorize -Wall -Wno-unused-function"
FILES=${FILES:-pt_abi pt_megakernel pt_wavefront pt_adaptive pt_denoise pt_guide}
TMP=$(mktemp -d "${TMPDIR:-/tmp}/ptmi_identity.XXXXXX")
trap 'rm -rf "$TMP"' EXIT

mkdir -p "$TMP/parent" "$TMP/new/path-tracer-python_amd"
git -C "$ROOT" archive "$REV" path-tracer-python_amd/csrc include | tar -x -C "$TMP/parent"
cp -r "$ROOT/include" "$TMP/new/include"
cp -r "$ROOT/path-tracer-python_amd/csrc" "$TMP/new/path-tracer-python_amd/csrc"

one() {  # tree build defs file
  local dir="$TMP/$1/path-tracer-python_amd/csrc" out="$TMP/$1/$2" f=$4
  mkdir -p "$out"
  (cd "$dir" && "$HIPCC" $FLAGS $3 --cuda-device-only -c -o "$out/$f.o" "$f.hip")
  "$LLVM/clang-offload-bundler" --unbundle --type=o --targets=hipv4-amdgcn-amd-amdhsa--gfx950 \
    --input="$out/$f.o" --output="$out/$f.co"
  "$LLVM/llvm-objdump" -d "$out/$f.co" | grep -v 'file format' > "$out/$f.dis"
  "$LLVM/llvm-readelf" --notes "$out/$f.co" > "$out/$f.notes"
  "$LLVM/llvm-readelf" -sW "$out/$f.co" | grep '\.kd$' | awk '{print $NF}' | sort -u > "$out/$f.kd"
}

pids=""
for tree in parent new; do
  for f in $FILES; do
    one $tree shipped "" $f & pids="$pids $!"
    one $tree stress "-DPTMI_STRESS_WAVES=8" $f & pids="$pids $!"
  done
done
for p in $pids; do wait "$p"; done

same() { cmp -s "$TMP/parent/$1" "$TMP/new/$1" && echo identical || { echo DIFFERENT; bad=1; }; }
bad=0
n=0
echo "| file | build | kernels (\`.kd\`) | disassembly lines | disassembly | notes | \`.kd\` symbols |"
echo "|---|---|---|---|---|---|---|"
for f in $FILES; do
  for b in shipped stress; do
    nk=$(wc -l < "$TMP/new/$b/$f.kd")
    nd=$(wc -l < "$TMP/new/$b/$f.dis")
    r1=$(same $b/$f.dis) && r2=$(same $b/$f.notes) && r3=$(same $b/$f.kd)
    case "$r1$r2$r3" in *DIFFERENT*) bad=1 ;; esac
    n=$((n + 3))
    echo "| \`$f.hip\` | $b | $nk | $nd | $r1 | $r2 | $r3 |"
  done
done
[ $bad -eq 0 ] && echo "all $n comparisons identical" || echo "DEVICE CODE DIFFERS"
exit $bad
