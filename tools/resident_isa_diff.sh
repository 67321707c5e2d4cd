#!/bin/bash
# Device disassembly of every k_resident instantiation in two builds of libpyitd_hip.so, compared instruction by instruction
# (address / encoding comments and PC-relative call offsets stripped: they move whenever the code object's layout does).
# usage: bash tools/resident_isa_diff.sh parent.so new.so [symbol-substring]     (exit 0: identical)
set -e
pat=${3:-k_resident}
d=$(mktemp -d)
for side in a b; do
    lib=$1; [ $side = b ] && lib=$2
    objcopy --dump-section .hip_fatbin=$d/$side.fb "$lib"
    /opt/rocm/llvm/bin/clang-offload-bundler --unbundle --type=o --input=$d/$side.fb \
        --targets=hipv4-amdgcn-amd-amdhsa--gfx950 --output=$d/$side.co
    /opt/rocm/llvm/bin/llvm-objdump -d --no-show-raw-insn --no-leading-addr $d/$side.co |
        awk -v p="$pat" '/>:$/ {on = index($0, p) > 0} on' |
        sed -e 's#//.*##' -e 's/<[^>]*+0x[0-9a-f]*>/<off>/' -e 's/[[:space:]]*$//' > $d/$side.s
done
echo "$(grep -c '>:$' $d/a.s) / $(grep -c '>:$' $d/b.s) functions, $(wc -l < $d/a.s) / $(wc -l < $d/b.s) lines"
diff $d/a.s $d/b.s > $d/diff.txt && echo "identical" || { echo "$(grep -c '^[<>]' $d/diff.txt) differing lines"; exit 1; }
