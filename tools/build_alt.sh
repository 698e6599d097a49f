#!/bin/bash
# Build gan-control_amd/csrc/alt/libalt_<name>.so for same-box A/B runs (GANCONTROL_HIP_LIB=...): the whole library compiled under extra flags, by the
# Makefile's `alt` target (one unit list, one set of rules; objects in csrc/build/alt_<name>/).  alt/ is git-ignored but, unlike build/, it travels to
# the GPU box.  The library carries its own gc_source_hash ("alt:<name>:..."), so counters collected on it are never quoted for the in-tree library.
#   tools/build_alt.sh <name> "<extra flags>"
# A build of another revision's sources: check that revision out somewhere (git worktree) and run its own Makefile with LIB=<this tree>/.../alt/libalt_<name>.so.
set -e
[ -n "$1" ] || { echo 'usage: tools/build_alt.sh <name> "<extra flags>"'; exit 2; }
R=$(cd "$(dirname "$0")/.." && pwd)/gan-control_amd/csrc
make -C "$R" -j"${MAX_JOBS:-4}" alt NAME="$1" EXTRA="$2" > /dev/null
echo built $R/alt/libalt_$1.so
