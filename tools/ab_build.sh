#!/bin/bash
# Build the library of another git revision next to the working tree's, for same-session A/B timing:
#   tools/ab_build.sh <rev>   ->  build/ab_old.so     (then: GCGCN_LIB=$PWD/build/ab_old.so python bench.py ...)
# Only meaningful while both revisions speak the same C ABI (include/gcgcn.h).
set -e
rev=${1:-HEAD}
root=$(cd $(dirname $0)/.. && pwd)
d=/tmp/ab_src
rm -rf $d && mkdir -p $d/gcgcn_amd/csrc $d/include   # the tree's layout: the sources include "../../include/*.h"
for f in $(git ls-tree --name-only $rev gcgcn_amd/csrc/ | grep -E '\.(hip|hpp)$') $(git ls-tree --name-only $rev include/ | grep -E '\.h$'); do
  git show $rev:$f > $d/$f
done
cd $d/gcgcn_amd/csrc
objs=""
for f in *.hip; do
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -c $f -o ${f%.hip}.o &
  objs="$objs ${f%.hip}.o"
done
wait
mkdir -p $root/build
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o $root/build/ab_old.so $objs
ls -la $root/build/ab_old.so
