#!/bin/bash
# Build whole-library variants with extra compiler flags:  tools/build_lib_variant.sh [--only "conv3x3 wgrad"] name "-DFOO=1" [name flags]...
# -> fabric_amd/csrc/variants/lib_<name>.so (git-ignored; select with BIDATE_LIB or tools/ab_lib.sh)
# The sources are the Makefile's.  --only: recompile just the listed sources with the flags and take every other object from the
# regular build (run `make -C fabric_amd/csrc` first) -- for flags that only one source reads.
cd "$(dirname "$0")/../fabric_amd/csrc" && mkdir -p variants
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
all=$(sed -n 's/^SRCS *= *//p' Makefile | sed 's/\.hip//g')
only="$all"
if [ "$1" == "--only" ]; then only="$2"; shift 2; fi
while [ $# -gt 1 ]; do
  name=$1; flags=$2; shift 2
  (
    objs=""
    for s in $all; do
      if [[ " $only " == *" $s "* ]]; then
        $HIPCC --offload-arch=gfx950 -O3 -std=c++17 -fPIC $flags -c $s.hip -o variants/${s}_$name.o 2>variants/${s}_$name.log || { echo "FAILED $s ($name)"; grep -m5 error variants/${s}_$name.log; }
        objs="$objs variants/${s}_$name.o"
      else
        objs="$objs $s.o"
      fi
    done
    $HIPCC --offload-arch=gfx950 -shared -fPIC $objs -o variants/lib_$name.so && echo built $name
  ) &
done
wait
