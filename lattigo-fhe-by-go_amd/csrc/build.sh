#!/bin/bash
# Builds liblattigo_ring_hip.so (gfx950 code object + host ABI) in-tree with hipcc.
set -e
cd "$(dirname "$0")"
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math -I../../include -I. -Wall -Wno-unused-function"
# LR_BUILD_DIAG=1: the diagnostics build -- adds the clock-stamping ("t") and persistent ("p") code objects of the negative-result
# experiments and lets lr_options::ntt_timeline / ntt_persist select them; the default build ships neither
[ -n "$LR_BUILD_DIAG" ] && FLAGS="$FLAGS -DLR_BUILD_DIAG=1"
mkdir -p build
# The sources: every kernel file and every host unit of this directory (the C ABI, one translation unit per handle family, with lr_host.hpp
# as what they share; lr_precompute.cpp; lr_asm.cpp), and the generated build/lr_asm_blob.cpp.  An object is named after its whole source
# file name -- lr_keygen.hip and lr_keygen.cpp give build/lr_keygen.hip.o and build/lr_keygen.cpp.o -- and the library links all of them.
SOURCES="$(echo lr_*.hip lr_*.cpp) build/lr_asm_blob.cpp"
objects() { for f in "$@"; do echo "build/$(basename "$f").o"; done; }
compile() {
  case $1 in
    build/*.cpp) g++ -O1 -fPIC -c "$1" -o "$(objects "$1")" ;;             # generated tables: no device code
    *.hip) $HIPCC $FLAGS -c "$1" -o "$(objects "$1")" ;;
    *.cpp) $HIPCC $FLAGS -x hip -c "$1" -o "$(objects "$1")" ;;
  esac
}
# compiles the named sources, at most ${MAX_JOBS:-16} at a time (a failed compile stops the script where it is waited for: set -e)
compile_all() {
  local pids=()
  for f in "$@"; do
    if [ ${#pids[@]} -ge "${MAX_JOBS:-16}" ]; then
      wait "${pids[0]}"
      pids=("${pids[@]:1}")
    fi
    compile "$f" &
    pids+=($!)
  done
  for p in "${pids[@]}"; do wait "$p"; done
}
link() {
  $HIPCC --offload-arch=gfx950 -shared -fPIC -o ../liblattigo_ring_hip.so $(objects $SOURCES)
  echo "built $(cd .. && pwd)/liblattigo_ring_hip.so"
}
# developer shortcut: `build.sh lr_abi_ckks.cpp lr_ewise.hip` recompiles only the named sources and relinks (everything else must
# have been built before); without arguments the whole library is built from scratch, which is what __graft_entry__.build() runs
if [ $# -gt 0 ]; then
  compile_all "$@"
  link
  exit 0
fi
# hand-scheduled assembly kernels: generate -> assemble -> embed, every code object of asmgen/catalogue.py (shipped(); with LR_BUILD_DIAG
# the diagnostics ones too) on a bounded pool, and build/lr_asm_blob.cpp with their names and block sizes.  LLVM overrides the tools' directory
python3 asmgen/catalogue.py build build
compile_all $SOURCES
link
