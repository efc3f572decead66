#!/bin/bash
# Builds a measurement variant of libbeluga_mcl.so with extra compiler flags into build/variants/<name>/ (never the product
# library): tools/build_variant.sh <name> "<flags>" [r04 | <git revision>];  use with BELUGA_MCL_LIB=build/variants/<name>/libbeluga_mcl.so
#
# Third argument: a git revision whose sources the variant is built from (A/B against an earlier tree on the same box).
# "r04": the variant is built from ROUND 4's sources (git commit 83dc34d - kernels.hip, context.hip, kernels.h with the
# ablation / timing / statistics blocks the measurement scripts of rounds 2 - 4 drive: -DMCL_ABLATE, -DMCL_LF_TIMING, -DMCL_PIPE_ABLATE,
# -DMCL_DRAW_ABLATE, -DMCL_BEAM_STATS, -DMCL_BEAM_ABLATE, -DMCL_PATCH_LDS_PAD, k_reweight_lf_pipe, the LDS-direct lf_producer = 0 form).
# Round 5 took those blocks out of the product's kernels.hip; the numbers in profiles/r0[2-4]_* were measured on that tree.
# Every variant is tagged -DMCL_MEASUREMENT_BUILD: beluga_amd/capi.py refuses to load it as the product library.
set -eu
name=$1; flags=${2:-}; tree=${3:-}
root=$(cd "$(dirname "$0")/.." && pwd)
out=$root/build/variants/$name
mkdir -p $out
src=$root/beluga_amd/csrc
if [ -n "$tree" ]; then
  rev=$tree; [ "$tree" = "r04" ] && rev=83dc34d
  src=$out/src_$tree
  mkdir -p $src
  for f in kernels.hip context.hip kernels.h se2.h rng.h map_build.h map_build.cpp cluster_host.h cluster_host.cpp; do git -C $root show $rev:beluga_amd/csrc/$f > $src/$f; done
  # (translation units and headers that older revisions do not have)
  for f in beam_kernels.hip device_common.hpp sensor_records.h ndt_host.h ndt_host.cpp landmark_host.h landmark_host.cpp scan_host.cpp set_facts.h cycle_types.h cycle_host.h cycle_host.cpp \
           ndt_kernels.hip ndt_build_kernels.hip landmark_kernels.hip batch_host.h batch_host.cpp map_store.h map_store_host.h map_store_host.cpp; do
    git -C $root show $rev:beluga_amd/csrc/$f > $src/$f 2>/dev/null || rm -f $src/$f
  done
  git -C $root show $rev:include/beluga_mcl.h > $src/beluga_mcl.h
fi
common="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -Wno-unused-result -I$src -I$root/include -DMCL_MEASUREMENT_BUILD $flags"
/opt/rocm/bin/hipcc $common -x hip -c $src/kernels.hip -o $out/kernels.o
beam=""   # (the beam model's kernels are a translation unit of their own from round 5 on; older revisions have them inside kernels.hip)
if [ -f $src/beam_kernels.hip ]; then /opt/rocm/bin/hipcc $common -x hip -c $src/beam_kernels.hip -o $out/beam_kernels.o; beam=$out/beam_kernels.o; fi
# Every other translation unit: the list is beluga_amd.build's SOURCES, so a file added there needs no edit here.  A revision's own tree
# is compiled name by name, skipping what that revision lacks (older revisions have the later files' code inside context.hip).
units=$(cd $root && python -c "from beluga_amd.build import SOURCES; print(' '.join(s for s in SOURCES if s not in ('kernels.hip', 'beam_kernels.hip')))")
rest=""
if [ -n "$tree" ]; then
  for f in $units; do
    [ -f $src/$f ] || continue
    case $f in *.hip) lang="-x hip";; *) lang="";; esac
    /opt/rocm/bin/hipcc $common $lang -c $src/$f -o $out/${f%.*}.o
    rest="$rest $out/${f%.*}.o"
  done
else
  [ -f $root/beluga_amd/lib/context.o ] || python -m beluga_amd.build
  for f in $units; do rest="$rest $root/beluga_amd/lib/${f%.*}.o"; done
fi
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o $out/libbeluga_mcl.so $out/kernels.o $beam $rest
echo built $out/libbeluga_mcl.so
