#!/bin/bash
# Instruction census of ONE instantiation of the one-launch solve (the probe instantiation of fused_one.sh: six blocks, plain
# Gauss-Newton; MMX_PROBE_RULE=1 / -1: LM schedule / generic rule), compiled to gfx950 assembly with the solve kernels' flags
# (momentum_amd/build.py SOLVE_KERNEL_FLAGS).  For every barrier-to-barrier region of the kernel, in program order: its
# instructions, the lane reads (and how many of them read v124-v127, where the spilled SGPRs are parked), the lane writes, the
# no-ops, the LDS instructions, the matrix-core instructions and the memory loads.  Static counts of the text -- a region inside
# a loop is counted once, the label column says where it starts.  Classifies by mnemonic prefix, nothing else.
#   bash scripts/probes/fused_census.sh [extra hipcc flags ...]      CSRC=<dir>: another tree's momentum_amd/csrc
#   KEEP_ASM=<file> keeps the assembly
cd "${CSRC:-$(dirname "$0")/../../momentum_amd/csrc}" || exit 1
tmp=$(mktemp -d)
asm=${KEEP_ASM:-$tmp/one.s}
hipcc --offload-arch=gfx950 -O3 -std=c++17 -DMMX_FUSED_GROUP=9 -mllvm -disable-machine-licm -mllvm -disable-lsr "$@" \
  -S --cuda-device-only mmx_fused.hip -o "$asm" -Rpass-analysis=kernel-resource-usage 2> $tmp/one.txt || { cat $tmp/one.txt; exit 1; }
grep -E "Function Name|VGPRs:|ScratchSize|Occupancy|SGPRs Spill|VGPRs Spill|LDS Size" $tmp/one.txt | sed 's/.*remark: //; s/ \[-Rpass.*//' |
  awk '/Function Name/ { keep = /fusedSolveKernel/ } keep { printf "%s ", $0 } END { print "" }' | sed 's/  */ /g'
awk '
  function flush() {
    printf "%4d  %-12s %6d %6d %6d %6d %6d %6d %6d %6d\n", region, label, n, rl, rlp, wl, nop, ds, mf, ld
    tn += n; trl += rl; trlp += rlp; twl += wl; tnop += nop; tds += ds; tmf += mf; tld += ld
    n = rl = rlp = wl = nop = ds = mf = ld = 0
    ++region
    label = last
  }
  /^_Z.*fusedSolveKernel.*:/ { inside = 1; region = 0; label = "entry"; last = "entry"
    printf "%4s  %-12s %6s %6s %6s %6s %6s %6s %6s %6s\n", "#", "starts at", "insts", "rdlane", "park", "wrlane", "s_nop", "ds_*", "mfma", "loads"; next }
  !inside { next }
  /^\.Lfunc_end/ { flush(); inside = 0
    printf "%4s  %-12s %6d %6d %6d %6d %6d %6d %6d %6d\n", "", "total", tn, trl, trlp, twl, tnop, tds, tmf, tld; next }
  /^\.LBB[0-9_]*:/ { last = $1; sub(/:.*/, "", last); next }
  /^[ \t]*[;.]/ || /^[ \t]*$/ || /^[A-Za-z_.$0-9]*:/ { next }
  {
    op = $1; ++n
    if (op ~ /^v_readlane_b32/) { ++rl; if ($0 ~ /, v12[4-7],/) ++rlp }
    else if (op ~ /^v_writelane_b32/) ++wl
    else if (op ~ /^s_nop/) ++nop
    else if (op ~ /^ds_/) ++ds
    else if (op ~ /^v_mfma/) ++mf
    else if (op ~ /^(global|flat|scratch|buffer)_load/ || op ~ /^s_load/ || op ~ /^s_buffer_load/) ++ld
    if (op ~ /^s_barrier/) flush()
  }
' "$asm"
rm -rf $tmp
