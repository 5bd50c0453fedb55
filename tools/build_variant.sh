#!/bin/bash
# Developer tool: build a variant of the library with extra device-compile flags, for A/B runs on the GPU box (ADYPT_LIB=<path>).
#   tools/build_variant.sh <name> [--transform adypt_amd/csrc/measure/x.py]... [-DADYPT_PATH_SLOTS=320 ...]   ->  adypt_amd/libadypt_<name>.so
# Measurement variants live as source transforms under csrc/measure/: applied (in the order given) to a scratch copy of the device sources, which
# csrc/Makefile then compiles and links by the product's own rules (measure/_variant.py; build/tracer_<name>.o, build/multi_<name>.o).
exec python3 "$(dirname "$0")/../adypt_amd/csrc/measure/_variant.py" "$@"
