#!/bin/bash
# kernel_regs.sh <file.hip> [name filter] [extra hipcc flags...]: registers / spills / occupancy per kernel (compiler remarks, no GPU)
# kernel_regs.sh --x16 [extra hipcc flags...]: every X16 instance of k_rowpass_v2 -- the 20 pair instances <NKC, NU, 4, true, true>
#   (<.., true, true, true, false>: the 18 with phase C deferred; <.., true, true, true, true>: their byte form) and the one-block ones <NKC, NU, 4 or 8, true, false>; each must show scratch 0, spill 0 / 0, at most 256 VGPRs and, at
#   four waves, occupancy >= 2
if [ "$1" = "--x16" ]; then
  shift
  set -- "$(dirname "$0")/../demethify_amd/csrc/dmf_kernels_rowpass2.hip" 'k_rowpass_v2<[0-4], [1-4], [48], true, ' "$@"
fi
f=$1; filt=${2:-.}; shift; shift
/opt/rocm/bin/hipcc -O3 -std=c++17 --offload-arch=gfx950 --offload-device-only -c "$f" -o /dev/null -Rpass-analysis=kernel-resource-usage "$@" 2>&1 | \
  awk '/Function Name:/ {name=$(NF-1)} /TotalSGPRs:/ {s=$(NF-1)} / VGPRs:/ {v=$(NF-1)} /ScratchSize/ {sc=$(NF-1)} /Occupancy/ {o=$(NF-1)} /SGPRs Spill/ {ss=$(NF-1)} /VGPRs Spill/ {print name, "vgpr", v, "sgpr", s, "scratch", sc, "spill", $(NF-1) "/" ss, "occ", o}' | \
  c++filt | sed 's/([^)]*)//; s/void dmf:://' | grep -E "$filt"
