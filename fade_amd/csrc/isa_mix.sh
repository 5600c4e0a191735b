#!/bin/bash
# usage: isa_mix.sh <mangled-kernel-prefix> [rows]  — instruction mix of the kernel's sweep loops: every loop (a label and the
# last backward branch to it) that holds v_pk_maximum3_f16 and no loop of its own, i.e. the general and the FAST sweep of
# sw_pk_kernel per block of 4 steps; a kernel without such a loop: its longest innermost loop.  Per loop the VALU / SALU / s_nop
# counts and what must not be there (scratch_* and v_readlane / v_writelane: spills), then the `rows` most frequent opcodes.
# (one listing per translation unit: the kernel is in one of them; a prefix that ends where the template arguments end, e.g.
# ..ELb1ELb1EE for the row-and-step drift frame and ..ELb1ELb0EE for the column-drift frame, picks one instantiation)
T=$(mktemp -d)
trap 'rm -rf "$T"' EXIT
cat "$(dirname "$0")"/build/*-gfx950.s | awk -v k="^$1" '$0 ~ k && /:/ && !p {p=1} p {print} p && /s_endpgm/ {exit}' > "$T/kern.s"
[ -s "$T/kern.s" ] || { echo "kernel not found"; exit 1; }
# loops as a label and the last conditional branch back to it; innermost = no other loop's label inside; per loop its max3 count
pick=$(awk '{line[NR] = $0}
     /^\.LBB[0-9]+_[0-9]+:/ {l = $1; sub(":.*", "", l); at[l] = NR}
     /^[ \t]+s_cbranch_/ {if ($2 in at) {a = at[$2]; if (!(a in last)) order[++n] = a; last[a] = NR}}
     END {
       for (i = 1; i <= n; i++) {
         a = order[i]; inner = 1
         for (j = 1; j <= n; j++) if (order[j] > a && last[order[j]] <= last[a]) inner = 0
         if (!inner) continue
         m = 0
         for (k = a; k <= last[a]; k++) if (line[k] ~ /v_pk_maximum3_f16/) m++
         if (m) {sweeps = sweeps " " a ":" last[a]}
         if (last[a] - a > longest) {longest = last[a] - a; lp = a ":" last[a]}
       }
       print (sweeps != "" ? sweeps : lp)
     }' "$T/kern.s")
[ -z "$pick" ] && { echo "loop not found"; exit 1; }
for p in $pick; do
  A=${p%:*}; B=${p#*:}
  sed -n "${A},${B}p" "$T/kern.s" > "$T/loop.s"
  echo "== loop at $(sed -n "${A}p" "$T/kern.s" | cut -d: -f1): $((B - A + 1)) lines, $(grep -c v_perm_b32 "$T/loop.s") v_perm_b32"
  grep -E "^\s+[vs]_|^\s+ds_|^\s+global_|^\s+buffer_|^\s+scratch_" "$T/loop.s" | awk '{print $1}' | sort | uniq -c | sort -rn | head -${2:-18}
  echo "total VALU in loop: $(grep -cE '^\s+v_' "$T/loop.s")   SALU: $(grep -E '^\s+s_' "$T/loop.s" | grep -cvE 's_nop|s_waitcnt')   s_nop: $(grep -c s_nop "$T/loop.s")   scratch: $(grep -cE '^\s+scratch_' "$T/loop.s")   lane moves: $(grep -cE 'v_(read|write)lane' "$T/loop.s")"
done
