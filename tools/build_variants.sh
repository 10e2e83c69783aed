#!/bin/bash
# Build A/B variants of libm3s_backend.so, the product plus extra flags, into
# mast3r-slam_amd/lib/variants/<name>.so (select one with M3S_BACKEND_LIB=...).
# usage: [ONLY="gn_accum ..."] [JOBS=n] tools/build_variants.sh name1 "-DFOO=1" name2 "-DFOO=2" ...
# Every file is compiled by the Makefile's own rule, so with its own per-file flags, plus the
# variant's (EXTRA), into build/variants/<name>/.
# ONLY: recompile just these sources with the variant's flags and link them with the normal
# build's objects of the others (run `make` first).
set -e
cd "$(dirname "$0")/../mast3r-slam_amd"
mkdir -p lib/variants
all=$(sed -n 's/^SRCS := //p' Makefile | sed 's|csrc/||g; s|\.hip||g')
while [ $# -ge 2 ]; do
    name=$1; flags=$2; shift 2
    obj=build/variants/$name
    mkdir -p $obj
    sel=""
    for f in $all; do
        if [ -n "${ONLY:-}" ] && ! echo " $ONLY " | grep -q " $f "; then
            cp -p build/$f.o $obj/$f.o
        else
            sel="$sel $obj/$f.o"
        fi
    done
    make -B -j"${JOBS:-8}" OBJ=$obj EXTRA="$flags" $sel
    make OBJ=$obj OUT=$obj EXTRA="$flags" $obj/libm3s_backend.so
    cp $obj/libm3s_backend.so lib/variants/$name.so
    echo "built lib/variants/$name.so ($flags)"
done
