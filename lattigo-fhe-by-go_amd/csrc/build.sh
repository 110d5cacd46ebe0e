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
# the C ABI, one translation unit per handle family (lr_host.hpp is what they share)
ABI_UNITS="lr_abi_core lr_abi_ring lr_abi_bext lr_abi_ckks lr_abi_batcher lr_abi_bfv lr_abi_bfv_eval lr_abi_bfv_batcher lr_abi_peer lr_bfv_encoder lr_ckks_encoder lr_bfv_encryptor lr_ckks_encryptor lr_keygen lr_collective lr_refresh lr_setup lr_abi_ckks_eval lr_abi_ckks_scalar"
link() {
  $HIPCC --offload-arch=gfx950 -shared -fPIC -o ../liblattigo_ring_hip.so build/lr_ntt.o build/lr_ewise.o build/lr_bext.o build/lr_bfv_encode.o build/lr_ckks_encode.o build/lr_bfv_encrypt.o build/lr_ckks_encrypt.o build/lr_ckks_eval.o build/lr_keygen_kernels.o build/lr_collective_kernels.o build/lr_refresh_kernels.o build/lr_setup_kernels.o $(for u in $ABI_UNITS; do echo build/$u.o; done) build/lr_precompute.o build/lr_asm.o build/lr_asm_blob.o
  echo "built $(cd .. && pwd)/liblattigo_ring_hip.so"
}
# developer shortcut: `build.sh lr_abi_ckks.cpp lr_ewise.hip` recompiles only the named sources and relinks (everything else must
# have been built before); without arguments the whole library is built from scratch, which is what __graft_entry__.build() runs
if [ $# -gt 0 ]; then
  spids=()
  for f in "$@"; do
    case $f in
      lr_keygen.hip) $HIPCC $FLAGS -c $f -o build/lr_keygen_kernels.o & spids+=($!) ;;
      lr_collective.hip) $HIPCC $FLAGS -c $f -o build/lr_collective_kernels.o & spids+=($!) ;;
      lr_refresh.hip) $HIPCC $FLAGS -c $f -o build/lr_refresh_kernels.o & spids+=($!) ;;
      lr_setup.hip) $HIPCC $FLAGS -c $f -o build/lr_setup_kernels.o & spids+=($!) ;;
      *.hip) $HIPCC $FLAGS -c $f -o build/${f%.hip}.o & spids+=($!) ;;
      *.cpp) $HIPCC $FLAGS -x hip -c $f -o build/${f%.cpp}.o & spids+=($!) ;;
    esac
  done
  for p in "${spids[@]}"; do wait $p; done     # (a failed compile stops here: set -e)
  link
  exit 0
fi
# hand-scheduled assembly kernels: generate -> assemble -> embed, every code object of asmgen/catalogue.py (shipped(); with LR_BUILD_DIAG
# the diagnostics ones too) on a bounded pool, and build/lr_asm_blob.cpp with their names and block sizes.  LLVM overrides the tools' directory
python3 asmgen/catalogue.py build build
pids=()
for f in lr_ntt.hip lr_ewise.hip lr_bext.hip lr_bfv_encode.hip lr_ckks_encode.hip lr_bfv_encrypt.hip lr_ckks_encrypt.hip lr_ckks_eval.hip; do
  $HIPCC $FLAGS -c $f -o build/${f%.hip}.o &
  pids+=($!)
done
# (lr_keygen.cpp and lr_keygen.hip share a stem, as do lr_collective.*, lr_refresh.* and lr_setup.*: the kernels' objects take another name)
$HIPCC $FLAGS -c lr_keygen.hip -o build/lr_keygen_kernels.o &
pids+=($!)
$HIPCC $FLAGS -c lr_collective.hip -o build/lr_collective_kernels.o &
pids+=($!)
$HIPCC $FLAGS -c lr_refresh.hip -o build/lr_refresh_kernels.o &
pids+=($!)
$HIPCC $FLAGS -c lr_setup.hip -o build/lr_setup_kernels.o &
pids+=($!)
for u in $ABI_UNITS; do
  $HIPCC $FLAGS -x hip -c $u.cpp -o build/$u.o &
  pids+=($!)
done
$HIPCC $FLAGS -x hip -c lr_precompute.cpp -o build/lr_precompute.o &
pids+=($!)
$HIPCC $FLAGS -x hip -c lr_asm.cpp -o build/lr_asm.o &
pids+=($!)
g++ -O1 -fPIC -c build/lr_asm_blob.cpp -o build/lr_asm_blob.o &
pids+=($!)
for p in "${pids[@]}"; do wait $p; done
link
