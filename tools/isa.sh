#!/bin/bash
# The gfx950 resource table of the path kernels: mrt_kernels.hip's four builds (exact / fast / fastz /
# pex, the Makefile's flag sets) and mrt_aux.hip, device code only, from the tree this script sits in.
#   tools/isa.sh [extra flags...]  > table        (e.g. tools/isa.sh -DMRT_EXPERIMENTS -DMRT_PHASES)
# The assembly goes to $ISA_OUT (default build/isa)/<build>.s.  Per mrt_path_kernel*, mrt_retrace_kernel
# and mrt_aux_kernel instance: VGPRs, SGPRs (amdhsa_next_free_*), VGPR and SGPR spill counts, private
# segment bytes, the scratch instructions in the code (a private segment with none is the backend's
# reserved scavenging slot, never touched), instructions.
root=$(cd "$(dirname "$0")/.." && pwd)
out=${ISA_OUT:-$root/build/isa}
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
mkdir -p "$out"
base="--offload-arch=${ARCH:-gfx950} -O3 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math -fno-slp-vectorize -Wno-unused-function -Wno-unused-command-line-argument \
 -mllvm -disable-promote-alloca-to-vector -mllvm -structurizecfg-skip-uniform-regions"
fast="-DMRT_FAST=1 -ffp-contract=fast -freciprocal-math -fno-hip-fp32-correctly-rounded-divide-sqrt"
build() {  # <name> <source> <flags...>
    local name=$1 src=$2; shift 2
    $HIPCC $base "$@" --cuda-device-only -S "$root/miniraytracer_amd/csrc/$src" -o "$out/$name.s" || exit 1
}
build exact mrt_kernels.hip -DMRT_FAST=0 "$@" &
build fast mrt_kernels.hip $fast "$@" &
build fastz mrt_kernels.hip $fast -fgpu-flush-denormals-to-zero -DMRT_TABLE_FTZ=1 "$@" &
build pex mrt_kernels.hip -DMRT_FAST=0 -DMRT_FWD_FOLD=1 -DMRT_TABLE_PEX=1 -DMRT_TREE_WG=768 -DMRT_WPE_WIDE=6 "$@" &
build aux mrt_aux.hip -DMRT_FAST=0 "$@" &
fail=0
for j in $(jobs -p); do wait "$j" || fail=1; done
[ $fail = 0 ] || { echo "isa.sh: a build failed" >&2; exit 1; }
for b in exact fast fastz pex aux; do
    awk -v b=$b '
     /^_Z(N4mrtd)?[0-9]+mrt_(path_kernel|retrace_kernel|aux_kernel).*:/{k=$1; n=0; sc=0; inb=1}
     inb && /^[ \t]+[sv]_|^[ \t]+(global|ds|scratch|buffer|flat)_/{n++} inb && /^[ \t]+scratch_/{sc++}
     /^\.Lfunc_end/{if(inb) {ins[k]=n; scr[k]=sc}; inb=0}
     /\.amdhsa_kernel /{kk=""} /\.amdhsa_kernel _Z(N4mrtd)?[0-9]+mrt_(path_kernel|retrace_kernel|aux_kernel)/{kk=$2":"}
     kk!="" && /amdhsa_private_segment_fixed_size/{ps[kk]=$2} kk!="" && /amdhsa_next_free_vgpr/{vg[kk]=$2} kk!="" && /amdhsa_next_free_sgpr/{sg[kk]=$2}
     /^[ \t]+.name:/{mk=""} /^[ \t]+.name:[ \t]+_Z(N4mrtd)?[0-9]+mrt_(path_kernel|retrace_kernel|aux_kernel)/{mk=$2":"}
     mk!="" && /\.sgpr_spill_count:/{ss[mk]=$2} mk!="" && /\.vgpr_spill_count:/{vs[mk]=$2}
     END{for (k in ins) printf "%-5s %-50s vgpr %4s sgpr %4s vspill %4s sspill %4s scratch %4s (scratch insts %3d) insts %6d\n", b, k, vg[k], sg[k], vs[k], ss[k], ps[k], scr[k], ins[k]}' "$out/$b.s" | sort
done
