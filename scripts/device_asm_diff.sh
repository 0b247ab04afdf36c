#!/usr/bin/env bash
# Device assembly of every translation unit, working tree against a parent revision: scripts/device_asm_diff.sh <rev>
# Prints one same/DIFFERENT line per unit and exits non-zero on any difference; an instance group the parent does not have prints "new".
# Needs hipcc, no GPU.
# Both sides are compiled with build.py's flags plus --cuda-device-only -S from the same relative layout; lines with
# __hip_cuid_ (a hash of path and file) are dropped.  WORK=<dir> keeps the outputs and reuses the parent's; JOBS caps the jobs.
set -euo pipefail
rev=${1:?usage: device_asm_diff.sh <parent-revision>}
root=$(git -C "$(dirname "$0")" rev-parse --show-toplevel)
work=${WORK:-$(mktemp -d)}
[ -n "${WORK:-}" ] || trap 'rm -rf "$work"' EXIT  # (a directory of our own making goes again)
hipcc=${ROCM_PATH:-/opt/rocm}/bin/hipcc
flags="--offload-arch=gfx950 -O3 -std=c++17 -fPIC --cuda-device-only -S -Wno-unused-command-line-argument"
# the working tree's list of translation units (librosa_amd/build.py) and its instance groups
units=$(cd "$root" && python -c "from librosa_amd.build import UNITS, n_groups; print(*UNITS, *(f'inst:{g}' for g in range(n_groups())))")

mkdir -p "$work/parent" "$work/new"
[ -d "$work/parent/librosa_amd" ] || git -C "$root" archive "$rev" librosa_amd/csrc include | tar -x -C "$work/parent"
rm -rf "$work/new/librosa_amd" "$work/new/include" "$work/new"/*.s
(cd "$root" && tar -c librosa_amd/csrc include) | tar -x -C "$work/new"

parent_groups=$(sed -n 's/^#define LRA_INST_NUM_GROUPS \([0-9]*\).*/\1/p' "$work/parent/librosa_amd/csrc/lra_fused.h")
is_new() { [ "${1#inst:}" != "$1" ] && [ "${1#inst:}" -ge "$parent_groups" ]; }

for side in parent new; do
    for u in $units; do
        [ "$side" = parent ] && is_new "$u" && continue
        [ "$side" = parent ] && [ -s "$work/parent/$u.s" ] && continue
        g=${u#*:}; f=${u%%:*}
        [ "$g" = "$u" ] && def= || def=-DLRA_INST_GROUP=$g
        echo "cd $work/$side && $hipcc $flags $def librosa_amd/csrc/lra_$f.hip -o - | grep -v __hip_cuid_ > $u.tmp && mv $u.tmp $u.s"
    done
done | xargs -P "${JOBS:-16}" -d '\n' -n 1 bash -o pipefail -c || true  # (a unit that does not compile leaves no .s: DIFFERENT below)

rc=0
for u in $units; do
    if is_new "$u"; then [ -s "$work/new/$u.s" ] && echo "new        $u" || { echo "DIFFERENT  $u (does not compile)"; rc=1; }
    elif cmp -s "$work/parent/$u.s" "$work/new/$u.s"; then echo "same       $u"; else echo "DIFFERENT  $u"; rc=1; fi
done
exit $rc
