#!/bin/bash
# One line per gfx950 kernel of the library's .hip units:
#   name size vgpr sgpr lds scratch hash
# (symbol size, register counts, static LDS and scratch bytes from the code
# object's notes, a hash of the instruction encodings).  Two trees whose
# tables are equal run the same device code:
#   bash tools/kernel_table.sh [TREE] > table.txt     (TREE: default this one)
set -e -o pipefail
T=$(cd "${1:-$(dirname "$0")/..}" && pwd)
C=$T/huffmandecoderongpus_amd/csrc
R=${ROCM_PATH:-/opt/rocm}
W=$(mktemp -d)
trap 'rm -rf "$W"' EXIT
for u in "$C"/*.hip; do
    (n=$W/$(basename "$u" .hip)
     "$R/bin/hipcc" -O3 -std=c++17 --offload-arch=gfx950 -I"$T/include" -I"$C" -Wno-unused-value \
         --cuda-device-only --no-gpu-bundle-output -c "$u" -o "$n.co"
     "$R/llvm/bin/llvm-readelf" -sW --notes "$n.co" > "$n.elf"
     "$R/llvm/bin/llvm-objdump" -d "$n.co" > "$n.dis") &
done
wait
for e in "$W"/*.elf; do
    # notes: a kernel's keys come in alphabetical order, .vgpr_count last
    awk '$4 == "FUNC" { size[$8] = $3 }
         /\.group_segment_fixed_size:/ { lds = $2 }
         /^ *\.name:/ { nm = $2 }
         /\.private_segment_fixed_size:/ { scr = $2 }
         /\.sgpr_count:/ { sg = $2 }
         /^ *\.vgpr_count:/ { print nm, size[nm], $2, sg, lds, scr }' "$e" | sort > "$W/meta"
    # disassembly: the encoding column of every instruction, per symbol (less
    # the padding after its end)
    awk 'function out() { sub(/(BF800000|BF9F0000)+$/, "", enc); if (k != "") print k, enc }
         /^[0-9a-f]+ <.*>:$/ { out(); k = substr($2, 2, length($2) - 3); enc = ""; next }
         { i = index($0, "// "); if (!i) next
           x = substr($0, i + 3); sub(/^[0-9A-F]+: /, "", x); sub(/ *<.*$/, "", x); gsub(/ /, "", x); enc = enc x }
         END { out() }' "${e%.elf}.dis" |
        while read -r k enc; do echo "$k $(printf %s "$enc" | md5sum | cut -c1-32)"; done | sort > "$W/hash"
    join "$W/meta" "$W/hash"
done | sort
