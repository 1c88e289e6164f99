#!/bin/bash
# tests/c/plan_walk.c under AddressSanitizer + UBSan, as a stand-alone program: the host units of the library (HOST_UNITS of
# demfi_amd/csrc/build.sh) and the program are instrumented, the kernel objects of an ordinary build are linked as they are.
# No GPU needed (nothing is launched).  usage: tests/c/plan_walk_san.sh
set -e
cd "$(dirname "$0")"
ROOT=$(cd ../.. && pwd)
CSRC=$ROOT/demfi_amd/csrc
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
[ -f $CSRC/conv.o ] || bash $CSRC/build.sh > /dev/null
HOST_UNITS=$(sed -n 's/^HOST_UNITS="\(.*\)"$/\1/p' $CSRC/build.sh)
# pointer-overflow is off on purpose: the sizing pass of demfi_ctx_create lays the plan out on a NULL base (addresses == workspace offsets)
SAN="-Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize=pointer-overflow -Xarch_host -fno-sanitize-recover=undefined"
OUT=$(mktemp -d)
trap 'rm -rf "$OUT"' EXIT
objs=()
for o in $CSRC/*.o; do
  u=$(basename "$o" .o)
  case "$u" in *_asan|*_trace) continue ;; esac
  [[ " $HOST_UNITS " == *" $u "* ]] || objs+=("$o")
done
for u in $HOST_UNITS; do
  $HIPCC --offload-arch=gfx950 -O1 -g -std=c++17 -fPIC -ffp-contract=off -I$ROOT/include -Wno-unused-result -fno-omit-frame-pointer $SAN -x hip -c $CSRC/$u.cpp -o $OUT/$u.o &
done
$HIPCC -O1 -g -fno-omit-frame-pointer $SAN -I$ROOT/include -x c -std=c99 -c plan_walk.c -o $OUT/plan_walk.o &
wait
for u in $HOST_UNITS plan_walk; do [ -f $OUT/$u.o ] || { echo "compile of $u failed"; exit 1; }; objs+=("$OUT/$u.o"); done
$HIPCC --offload-arch=gfx950 -fno-gpu-sanitize -fsanitize=address,undefined "${objs[@]}" -o $OUT/plan_walk -lz -lpthread      # host link only
(cd $ROOT && python -c "from tests.test_gpu_cabi import _write_weights; _write_weights('$OUT/weights.bin')")
nm $OUT/plan.o | grep -q __asan_report || { echo "host units are not instrumented"; exit 1; }
ASAN_OPTIONS=detect_leaks=1 UBSAN_OPTIONS=print_stacktrace=1:halt_on_error=1 $OUT/plan_walk $OUT/weights.bin
