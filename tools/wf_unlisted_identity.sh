#!/bin/bash
# Are the unlisted wavefront kernels of the working tree the same gfx950 code as a revision's?
#   bash tools/wf_unlisted_identity.sh REV
# tools/device_code_identity.sh compares whole code objects, so it reports
# pt_wavefront.hip as different as soon as a kernel is added or a template
# parameter renames one. This compares kernel by kernel instead: pt_wavefront.hip
# is compiled device-only from REV and from the working tree, in the shipped and
# the register-stress build; the tree's LISTED instantiations (mangled ...Lb1E...)
# are set aside, the unlisted ones' new template arguments (LISTED = false, an
# empty pack) are mapped back to REV's names, and each kernel's instructions
# (encodings included, addresses stripped) and its metadata entry (registers,
# LDS, scratch, kernarg size, every argument's offset) are compared. Prints a
# markdown table and any differing lines; exit 0 iff nothing differs. Needs no GPU.
set -eu
REV=$1
ROOT=$(cd "$(dirname "$0")/.." && pwd)
ROCM=${ROCM_PATH:-/opt/rocm}
HIPCC=${HIPCC:-$ROCM/bin/hipcc}
LLVM=$ROCM/lib/llvm/bin
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -fhip-fp32-correctly-rounded-divide-sqrt -fno-fast-math -fno-slp-vectorize -Wall -Wno-unused-function"
TMP=$(mktemp -d "${TMPDIR:-/tmp}/ptmi_wf_identity.XXXXXX")
trap 'rm -rf "$TMP"' EXIT
NEW_SUFFIX='ELb0EJEEEvNS_8DevSceneENS_8DevFrameENS_6WfBufsEiPyDpT2_'
OLD_SUFFIX='EEEvNS_8DevSceneENS_8DevFrameENS_6WfBufsEiPy'

mkdir -p "$TMP/parent" "$TMP/new/path-tracer-python_amd"
git -C "$ROOT" archive "$REV" path-tracer-python_amd/csrc include | tar -x -C "$TMP/parent"
cp -r "$ROOT/include" "$TMP/new/include"
cp -r "$ROOT/path-tracer-python_amd/csrc" "$TMP/new/path-tracer-python_amd/csrc"

one() {  # tree build defs
  local dir="$TMP/$1/path-tracer-python_amd/csrc" out="$TMP/$1/$2"
  mkdir -p "$out"
  (cd "$dir" && "$HIPCC" $FLAGS $3 --cuda-device-only -c -o "$out/wf.o" pt_wavefront.hip 2> "$out/warnings.txt")
  "$LLVM/clang-offload-bundler" --unbundle --type=o --targets=hipv4-amdgcn-amd-amdhsa--gfx950 \
    --input="$out/wf.o" --output="$out/wf.co"
  # one block per function: "<name>:" then its instructions without their addresses
  "$LLVM/llvm-objdump" -d "$out/wf.co" | sed -e "s/$NEW_SUFFIX/$OLD_SUFFIX/g" |
    awk '/^[0-9a-f]+ <.*>:$/ { keep = ($2 !~ /Lb1E/); if (keep) print $2; next }
         keep && NF && $1 != "..." { sub(/\/\/ [0-9A-F]+:/, "//"); print }' > "$out/unlisted.dis"  # ("...": padding)
  # one metadata entry per kernel, sorted by name
  "$LLVM/llvm-readelf" --notes "$out/wf.co" | sed -e "s/$NEW_SUFFIX/$OLD_SUFFIX/g" |
    awk '/^ +- \.agpr_count:/ { n++; k = 0; on = 1 } /^amdhsa\./ && !/kernels/ { on = 0 }
         on { line[n, ++k] = $0; len[n] = k; if ($1 == ".name:") name[n] = $2 }
         END { for (i = 1; i <= n; i++) if (name[i] !~ /Lb1E/) for (j = 1; j <= len[i]; j++) printf "%s\t%d\t%s\n", name[i], j, line[i, j] }' |
    sort -t "$(printf '\t')" -k1,1 -k2,2n | cut -f3- > "$out/unlisted.notes"
  "$LLVM/llvm-readelf" -sW "$out/wf.co" | grep '\.kd$' | awk '{print $NF}' | sed -e "s/$NEW_SUFFIX/$OLD_SUFFIX/g" | sort -u > "$out/all.kd"
  grep -v 'Lb1E' "$out/all.kd" > "$out/unlisted.kd" || true
}

pids=""
for tree in parent new; do
  one $tree shipped "" & pids="$pids $!"
  one $tree stress "-DPTMI_STRESS_WAVES=8" & pids="$pids $!"
done
for p in $pids; do wait "$p"; done

bad=0
echo "| build | unlisted kernels | listed kernels | instruction lines (unlisted) | instructions | metadata | \`.kd\` symbols |"
echo "|---|---|---|---|---|---|---|"
for b in shipped stress; do
  nk=$(wc -l < "$TMP/new/$b/unlisted.kd")
  nl=$(grep -c 'Lb1E' "$TMP/new/$b/all.kd" || true)
  nd=$(wc -l < "$TMP/new/$b/unlisted.dis")
  r=""
  for f in unlisted.dis unlisted.notes unlisted.kd; do
    if cmp -s "$TMP/parent/$b/$f" "$TMP/new/$b/$f"; then r="$r identical |"; else r="$r DIFFERENT |"; bad=1; fi
  done
  echo "| $b | $nk | $nl | $nd |$r"
done
for b in shipped stress; do
  for f in unlisted.dis unlisted.notes unlisted.kd; do
    if ! cmp -s "$TMP/parent/$b/$f" "$TMP/new/$b/$f"; then
      echo; echo "$b $f: differing lines (parent <, tree >), first 40:"
      diff "$TMP/parent/$b/$f" "$TMP/new/$b/$f" | head -40 || true
    fi
  done
done
if [ -n "${KEEP:-}" ]; then mkdir -p "$KEEP"; for t in parent new; do for b in shipped stress; do mkdir -p "$KEEP/$t/$b"; cp "$TMP/$t/$b"/*.dis "$TMP/$t/$b"/*.notes "$TMP/$t/$b"/*.kd "$TMP/$t/$b/wf.co" "$KEEP/$t/$b/"; done; done; fi
[ $bad -eq 0 ] && echo "every unlisted wavefront kernel is identical" || echo "UNLISTED KERNELS DIFFER"
exit $bad
