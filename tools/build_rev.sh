#!/bin/bash
# builds the library as of git revision $1 into build/variants/lib_$2.so (developer A/B on one GPU box)
set -e
rev=$1; name=$2; shift 2
d=$(mktemp -d)
mkdir -p $d/rustray_amd/csrc $d/include build/variants
# the files of THAT revision (today's names are wrong for an older one)
for f in $(git ls-tree --name-only $rev rustray_amd/csrc/); do git show $rev:$f > $d/$f; done
git show $rev:include/rustray_hip.h > $d/include/rustray_hip.h
# with THAT revision's flags (the Makefile's FLAGS line)
flags=$(sed -n 's/^FLAGS ?= //p' $d/rustray_amd/csrc/Makefile | sed 's/\$(ARCH)/gfx950/')
(cd $d/rustray_amd/csrc && hipcc $flags "$@" -shared -o $OLDPWD/build/variants/lib_$name.so rr_api.hip rr_bvh.cpp)
rm -rf $d
