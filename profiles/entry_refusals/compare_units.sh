#!/bin/bash
# Device code of every .hip unit, parent tree against this tree: the device side only, compiled with the flags of _build.py, the
# per-file id of the HIP front end normalised, the two listings compared byte for byte.  Prints one table row per unit.
#   usage: profiles/entry_refusals/compare_units.sh PARENT_TREE [OUT_DIR]     (PARENT_TREE: e.g. a `git worktree` of the parent commit)
#   UNITS="la3d_depth16 la3d_masks" limits the run to those units (default: every .hip file of this tree)
set -o pipefail
here=$(cd "$(dirname "$0")/../.." && pwd)
parent=$(cd "${1:?give the tree of the parent commit}" && pwd)
out=${2:-$(mktemp -d)}
hipcc=${HIPCC:-/opt/rocm/bin/hipcc}
mkdir -p "$out/parent" "$out/branch"
one() {   # tree, side, unit
  (cd "$1" && "$hipcc" --offload-arch=gfx950 -O3 -std=c++17 -fPIC -I include --cuda-device-only -S "labelany3d_amd/csrc/$3.hip" -o "$out/$2/$3.raw.s" &&
     sed -E 's/__hip_cuid_[0-9a-f]+/__hip_cuid_X/g' "$out/$2/$3.raw.s" > "$out/$2/$3.s")
}
units=${UNITS:-$(cd "$here/labelany3d_amd/csrc" && ls *.hip | sed 's/\.hip$//')}
echo "| unit | lines | identical |"
echo "|---|---|---|"
for u in $units; do
  one "$parent" parent "$u" & one "$here" branch "$u" & wait
  if [ -s "$out/parent/$u.s" ] && cmp -s "$out/parent/$u.s" "$out/branch/$u.s"; then same=yes; else same=NO; fi
  echo "| \`$u.hip\` | $(wc -l < "$out/branch/$u.s") | $same |"
done
