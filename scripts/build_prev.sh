#!/bin/bash
# Build ncf_amd/libncf_hip_prev.so from the kernel sources at a git revision
# (default HEAD), for A/B timing against the working tree:
#   scripts/build_prev.sh [rev] && python scripts/ab_kernel.py default prev
# include/ and ncf_amd/csrc/ of the revision are exported whole and built with the
# revision's own Makefile, so this does not depend on which sources it has.
set -euo pipefail
REV=${1:-HEAD}
ROOT=$(cd "$(dirname "$0")/.." && pwd)
T=$(mktemp -d)
trap 'rm -rf "$T"' EXIT
git -C "$ROOT" archive "$REV" include ncf_amd/csrc | tar -x -C "$T"
make -C "$T/ncf_amd/csrc" -j"${MAX_JOBS:-16}" ../libncf_hip.so
cp "$T/ncf_amd/libncf_hip.so" "$ROOT/ncf_amd/libncf_hip_prev.so"
echo "built ncf_amd/libncf_hip_prev.so from $REV"
