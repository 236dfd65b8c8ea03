#!/bin/bash
# Register / LDS / spill figures of every kernel in libmixgan_hip.so whose name matches $1 (default: all).
# A single-launch denoiser form that also has a TIMING build (the one tools/persist_timeline.py stamps) gets a second
# line under the listing with the production and the TIMING build's figures side by side: the two are allocated
# differently, so the stamps describe the TIMING binary, not the one bench.py times.
set -e
here=$(cd "$(dirname "$0")/.." && pwd)
tmp=$(mktemp -d)
cd "$tmp"
cp "$here/mixgan-tts_amd/libmixgan_hip.so" lib.so
/opt/rocm/lib/llvm/bin/llvm-objdump --offloading lib.so > /dev/null
for f in *.hipv4-amdgcn-amd-amdhsa--gfx950; do
    /opt/rocm/lib/llvm/bin/llvm-readelf --notes "$f" | awk -v pat="${1:-.}" '
        /\.agpr_count:/ {a=$2} /\.group_segment_fixed_size:/ {l=$2} /\.name:/ {n=$2} /\.private_segment_fixed_size:/ {p=$2}
        /\.sgpr_count:/ {s=$2} /\.vgpr_count:/ {v=$2} /\.vgpr_spill_count:/ {sp=$2; if (n ~ pat) printf "%-110s vgpr %3d agpr %3d sgpr %3d lds %6d scratch %4d spills %d\n", n, v, a, s, l, p, sp}'
done | sort -u | awk '{print}
    $1 ~ /denoiser_persist_kernelILi[0-9]+ELb[01]ELb[01]E/ {   # <NT, VEC4, TIMING, ...>: the key is the name without TIMING
        match($1, /kernelILi[0-9]+ELb[01]/); k = substr($1, RSTART, RLENGTH) "|" substr($1, RSTART + RLENGTH + 4)
        fig = "vgpr " $3 " scratch " $(NF - 2) " spills " $NF
        if (substr($1, RSTART + RLENGTH, 4) == "ELb1") t[k] = fig; else { p[k] = fig; name[k] = $1 }
    }
    END { for (k in p) if (k in t) printf "production | TIMING  %-86s %s | %s\n", name[k], p[k], t[k] }'
rm -rf "$tmp"
