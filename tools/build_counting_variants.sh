#!/bin/bash
# CPU side: the seven counting variants of the library tools/full_cycle.sh runs on the GPU box (source transform adypt_amd/csrc/measure/k_path_blocks.py):
#   wave entries per block: blockcnt (trip set), shadecnt, rarecnt;  active lanes per block: lanes_trip, lanes_shade, lanes_rare, lanes_wait
# (COUNTING and VARIANTS of adypt_amd/csrc/measure/_variant.py: each name's ADYPT_BLOCKS_* environment)
exec python3 "$(dirname "$0")/../adypt_amd/csrc/measure/_variant.py" --counting
